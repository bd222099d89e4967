"""The linear MMSE receiver of the codebook rate (DMX_FLAG_RX_LINEAR_MMSE, `receiver="mmse"`) without a GPU: the header and the
C-ABI's host-only answers on every entry point, the `receiver` argument of every Python call that takes one, the reference of
tests/_mmse_rate_ref.py on hand cases, and on the oracle the conditions that make the GPU comparison worth something - on
every case of tests/test_gpu_mmse_rate.py the two receivers differ by far more than the tolerances, and the tolerance is
small beside the rate."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import _mmse_rate_ref as M
from tests._codebook_rate_ref import codebook_rate_from_channel, codebook_rate_tolerance
from tests.test_beam_rsrp_cpu import _every
from tests.test_near_field_cpu import _params as _nf_params
from tests.test_wideband_cpu import _header, _lib

FLAG, ADAPTIVE, WIDEBAND, NEAR_FIELD, BEAM_POWER = 256, 1, 4, 16, 64
NAME = b"DMX_FLAG_RX_LINEAR_MMSE"
TAKEN = ("dmx_codebook_rate", "dmx_codebook_rate_subbands", "dmx_codebook_rate_supported", "dmx_codebook_rate_subbands_supported")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. header and ABI -------------------------------------------------------------------------------------------------------------
def test_header_defines_the_flag_and_the_abi_is_unchanged():
    nat, lib = _lib()
    header = _header()
    assert re.search(r"#define\s+DMX_FLAG_RX_LINEAR_MMSE\s+256u\b", header) and re.search(r"#define\s+DMX_ABI_VERSION\s+3\b", header)
    assert nat.FLAG_RX_LINEAR_MMSE == FLAG and nat.ABI_VERSION == 3 and lib.dmx_version() == 3
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(dmx_\w+)\s*\(", code)) == set(nat.EXPORTED_SYMBOLS) and len(nat.EXPORTED_SYMBOLS) == 37
    assert len(re.findall(r"void\*\s+stream", code)) == 18
    assert [f[0] for f in nat.DmxParams._fields_][-2:] == ["flags", "reserved0"]
    # the comment: the definition, the table, the single-layer statement; it names no function that is not exported
    said = [m for m in re.findall(r"/\*.*?\*/", header, flags=re.S) if "DMX_FLAG_RX_LINEAR_MMSE" in m]
    assert len(said) == 1
    text = said[0]
    assert set(re.findall(r"\b(dmx_\w+)\s*\(", text)) <= set(nat.EXPORTED_SYMBOLS)
    for word in ("1 / [A_ck^-1]_ii - 1", "log2(1 + sinr", "At L = 1", "bit-equal", "value 256", "128 stay unknown", "DMX_FLAG_ADAPTIVE_TERMS and",
                 "DMX_FLAG_NEAR_FIELD", "dmx_path_prep", "dmx_fd_kernel_choice", "every link of dmx_cell_rate", "WITHOUT the flag") + TAKEN:
        assert word in text, word


def test_kernel_source_selects_the_epilogue_by_a_template_parameter():
    src = lambda *p: re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "deepmimo_amd", "csrc", *p)).read())   # noqa: E731
    k10, body = src("k10_codebook_rate.hip"), src("k7_rate_body.h")
    assert k10.count("__global__") == 2 and "epilogue_mmse<L>" in k10 and "epilogue_logdet<L>" in k10 and k10.count("launch_dyn_lds(") == 4
    assert "epilogue_mmse" in body and "atomic" not in k10 and "__syncthreads" not in k10


# ---- 2. the flag matrix, zero-user calls -------------------------------------------------------------------------------------------
def test_the_two_calls_and_their_queries_alone_take_the_flag():
    nat, lib = _lib()
    p = _nf_params(nat, flags=0)
    calls, _keep = _every(nat, lib, p)
    assert len(calls) == 26 and set(TAKEN) <= set(calls)
    for flags in (FLAG, FLAG | ADAPTIVE, FLAG | NEAR_FIELD, FLAG | NEAR_FIELD | ADAPTIVE):
        p.flags = flags
        for name, call in calls.items():
            if name in TAKEN:
                p.flags = flags & ~FLAG
                want = call()
                p.flags = flags
                assert call() == want == (1 if name.endswith("_supported") else 0), (name, flags, lib.dmx_last_error())
                continue
            assert call() == -1, (name, flags)
            assert NAME in lib.dmx_last_error(), (name, flags, lib.dmx_last_error())
    # a link of dmx_cell_rate that is not the first
    ps = [_nf_params(nat, 0), _nf_params(nat, NEAR_FIELD), _nf_params(nat, FLAG)]
    links = (nat.DmxLink * 3)()
    for i, q in enumerate(ps):
        links[i].prm, links[i].n_paths_loaded, links[i].snr_linear = C.pointer(q), 5, 10.0
    for call in (lambda: lib.dmx_cell_rate_supported(links, 3), lambda: lib.dmx_cell_rate(links, 3, 0, 0, 0, None, None, None, None, None, None)):
        assert call() == -1 and NAME in lib.dmx_last_error(), lib.dmx_last_error()
    ps[2].flags = 0
    assert lib.dmx_cell_rate_supported(links, 3) == 1, lib.dmx_last_error()
    # without the flag every call answers as before
    p.flags = 0
    for name, call in calls.items():
        if name not in ("dmx_channels_fd_lpf", "dmx_channels_td", "dmx_channels_fd_direct"):      # refuse these parameters anyway
            assert call() in (0, 1, 9, 12, 2), (name, lib.dmx_last_error())


def test_other_bits_and_other_checks_answer_as_before():
    nat, lib = _lib()
    p = _nf_params(nat, flags=0)
    calls, _keep = _every(nat, lib, p)
    del calls["dmx_fd_kernel_choice"]                                            # never looked at unknown bits
    for flags in (FLAG | 2, FLAG | 8, FLAG | 32, FLAG | 128, FLAG | 512, FLAG | (1 << 31), 512):
        p.flags = flags
        for name, call in calls.items():
            assert call() == -1, (name, flags)
            assert b"unknown bits in dmx_params.flags / reserved0" in lib.dmx_last_error(), (name, flags, lib.dmx_last_error())
    p.flags, p.reserved0 = FLAG, 1
    for name, call in calls.items():
        assert call() == -1 and b"unknown bits" in lib.dmx_last_error(), name
    p.reserved0 = 0
    rate = calls["dmx_codebook_rate"]
    # neither the wide band nor the power average of the beam sweep is an option of the codebook rate; near field needs its carrier
    p.flags = FLAG | WIDEBAND
    assert rate() == -1 and b"DMX_FLAG_SPATIAL_WIDEBAND" in lib.dmx_last_error()
    p.flags = FLAG | BEAM_POWER
    assert rate() == -1 and b"DMX_FLAG_BEAM_MEAN_POWER" in lib.dmx_last_error()
    assert calls["dmx_beam_power"]() == -1 and NAME in lib.dmx_last_error()
    p.flags, p.carrier_freq = FLAG | NEAR_FIELD, 0.0
    assert rate() == -1 and b"DMX_FLAG_NEAR_FIELD" in lib.dmx_last_error() and b"carrier_freq" in lib.dmx_last_error()
    # the flag changes none of the call's other checks, and no shape limit
    p.flags = FLAG
    assert rate() == 0, lib.dmx_last_error()
    pp = C.byref(p)
    for flags in (0, FLAG):
        p.flags = flags
        assert lib.dmx_codebook_rate_supported(pp, 5, 4, 5) == 0 and b"n_layers = 5" in lib.dmx_last_error()     # above four layers
        assert lib.dmx_codebook_rate_subbands_supported(pp, 5, 4, 1, 0) == -1 and b"subband_size" in lib.dmx_last_error()
        assert lib.dmx_codebook_rate(pp, None, 0, 5, 0, 0, None, 4, 1, None, 0, -1.0, None, None, None, None) == -1
        assert b"snr_linear" in lib.dmx_last_error()
    p.rx_filter = 1
    assert rate() == -1 and b"dmx_codebook_rate does not cover rx_filter = 1" in lib.dmx_last_error()


# ---- 3. the Python layer -----------------------------------------------------------------------------------------------------------
def _dataset(n=6):
    import deepmimo_amd as dm
    ds = dm.Dataset(dict(onp.synth_rays(n, 5, seed=2)))
    ds["rt_params"] = {"frequency": 28e9}
    return ds


def _dm_params():
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 1])
    p.ofdm.selected_subcarriers = np.arange(8)
    return p


BAD_RECEIVERS = ["MMSE", "zf", "mrc", "", None, 1, True, b"mmse", ("mmse",)]


@pytest.mark.parametrize("receiver", BAD_RECEIVERS)
def test_a_bad_receiver_is_a_value_error_on_every_call(receiver, monkeypatch):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd import engine

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    cb = np.ones((2, 2, 8), np.complex64)
    ds, p = _dataset(), _dm_params()
    kw = dict(snr_db=10.0, receiver=receiver)
    calls = {
        "check": lambda: engine.check_receiver("x", receiver),
        "host check": lambda: engine.check_codebook_rate_call(_dm_params().validate(6), 5, 2, 2, 10.0, receiver),
        # the first thing the engine's methods do: no engine (and so no GPU) is needed to be refused
        "engine": lambda: engine.ChannelEngine.codebook_rate(None, None, cb, 10.0, receiver=receiver),
        "engine subbands": lambda: engine.ChannelEngine.codebook_rate_subbands(None, None, cb, 10.0, 2, receiver=receiver),
        "engine query": lambda: engine.ChannelEngine.codebook_rate_supported(None, None, 2, 2, receiver),
        "engine subband query": lambda: engine.ChannelEngine.codebook_rate_subbands_supported(None, None, 2, 2, 2, receiver),
        "codebook rate": lambda: ds.compute_codebook_rate(p, codebook=cb, **kw),
        "subband pmi": lambda: ds.compute_subband_pmi(p, codebook=cb, subband_size=2, **kw),
        "csi report": lambda: ds.compute_csi_report(p, codebooks=[cb[:, :1], cb], **kw),
        "near field": lambda: ds.near_field().compute_codebook_rate(p, codebook=cb, **kw),
        "macro fan-out": lambda: dm.MacroDataset([_dataset(), _dataset()]).compute_csi_report(p, codebooks=[cb], **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="receiver must be 'joint' or 'mmse'"):
            call()


def test_receiver_names_defaults_and_the_host_check_with_the_flag(monkeypatch):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd import engine
    assert engine.RECEIVERS == ("joint", "mmse")
    assert engine.check_receiver("x", "joint") is False and engine.check_receiver("x", "mmse") is True
    for f in (engine.ChannelEngine.codebook_rate, engine.ChannelEngine.codebook_rate_subbands, engine.ChannelEngine.codebook_rate_supported,
              engine.ChannelEngine.codebook_rate_subbands_supported, engine.check_codebook_rate_call, dm.Dataset.compute_codebook_rate,
              dm.Dataset.compute_subband_pmi, dm.Dataset.compute_csi_report):
        assert inspect.signature(f).parameters["receiver"].default == "joint", f
    assert list(inspect.signature(dm.Dataset.compute_codebook_rate).parameters)[1:] == ["params", "codebook", "snr_db", "per_codeword", "receiver"]
    ok = _dm_params().validate(6)
    assert engine.check_codebook_rate_call(ok, 5, 4, 2, 20.0, "mmse") == engine.check_codebook_rate_call(ok, 5, 4, 2, 20.0) == 100.0
    # the receiver changes no other refusal: they come before any GPU work, with the library's words
    monkeypatch.setattr(dsm, "_engine", lambda: (_ for _ in ()).throw(AssertionError("the GPU engine was asked for")))
    ds = _dataset()
    with pytest.raises(ValueError, match="n_layers = 3"):
        ds.compute_codebook_rate(_dm_params(), codebook=np.ones((2, 3, 8), np.complex64), snr_db=10.0, receiver="mmse")
    with pytest.raises(ValueError, match="snr_db"):
        ds.compute_subband_pmi(_dm_params(), receiver="mmse")
    with pytest.raises(ValueError, match="subband_size"):
        ds.compute_csi_report(_dm_params(), codebooks=[np.ones((2, 8))], snr_db=10.0, subband_size=0, receiver="mmse")
    td = _dm_params()
    td.freq_domain = 0
    with pytest.raises(ValueError, match="freq_domain"):
        ds.compute_codebook_rate(td, snr_db=10.0, receiver="mmse")


def test_valid_call_without_a_gpu_raises_the_usual_error(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    with pytest.raises(RuntimeError, match="no GPU"):
        _dataset().compute_codebook_rate(_dm_params(), codebook=np.ones((3, 2, 8), np.complex64), snr_db=20.0, receiver="mmse")


# ---- 4. the reference, by hand -----------------------------------------------------------------------------------------------------
def _random(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def test_reference_one_layer_is_the_joint_reference():
    H, W = _random((5, 3, 6, 4), 8), _random((7, 1, 6), 9)
    for snr in (0.3, 2.5, 4e3):
        a, ak = M.mmse_rate_from_channel(H, W, snr)
        b, bk = codebook_rate_from_channel(H, W, snr)
        np.testing.assert_allclose(a, b, rtol=1e-12)
        np.testing.assert_allclose(ak, bk, rtol=1e-12)
        assert M.mmse_sinr_from_channel(H, W, snr).shape == (5, 7, 1, 4)


def test_reference_orthogonal_layers_give_the_joint_reference():
    """E^H E diagonal: no layer leaks into another and the linear receiver loses nothing"""
    rng = np.random.default_rng(3)
    for m_rx, L in ((2, 2), (4, 3), (4, 4), (8, 4)):
        Q = np.linalg.qr(_random((6, 5, m_rx, m_rx), 10 + L))[0][..., :L]                  # [n, K, M_rx, L], orthonormal columns
        E = Q * 10 ** rng.uniform(-1, 1, (6, 5, 1, L))
        H = np.moveaxis(E, 1, -1)                                                          # [n, M_rx, L = M_tx, K]
        W = np.eye(L)[None]                                                                # one codeword, layer i = BS element i
        a, ak = M.mmse_rate_from_channel(H, W, 7.0)
        b, bk = codebook_rate_from_channel(H, W, 7.0)
        np.testing.assert_allclose(ak, bk, rtol=1e-11)
        sinr = M.mmse_sinr_from_channel(H, W, 7.0)                                         # [n, 1, L, K]
        want = (7.0 / L) * (np.abs(E) ** 2).sum(axis=2)                                    # s |e_i|^2, [n, K, L]
        np.testing.assert_allclose(sinr[:, 0], np.moveaxis(want, 1, -1), rtol=1e-10)


def test_reference_two_identical_layers():
    """rank one under two layers: A = I + g 1 1^T, [A^-1]_ii = (1 + g) / (1 + 2 g), so each layer has sinr g / (1 + g)"""
    H = _random((4, 3, 6, 5), 21) * np.array([1e-2, 1.0, 30.0, 0.0])[:, None, None, None]
    w = _random((6,), 22)
    W = np.stack([w, w])[None]                                                             # [1, 2, 6]
    snr = 5.0
    e = np.einsum("t,urtk->urk", w, H)
    g = (snr / 2) * (np.abs(e) ** 2).sum(axis=1)                                           # [n, K]
    rate_c, rate_ck = M.mmse_rate_from_channel(H, W, snr)
    np.testing.assert_allclose(rate_ck[:, 0], 2 * np.log2(1 + g / (1 + g)), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(codebook_rate_from_channel(H, W, snr)[1][:, 0], np.log2(1 + 2 * g), rtol=1e-10, atol=1e-14)
    assert (rate_c[3] == 0).all() and rate_ck.max() < 2.0                                  # at most one bit per layer


def test_reference_two_by_two_by_hand():
    """E = [[1, j], [0, 1]], snr = 2 (s = 1): G = [[1, j], [-j, 2]], A = [[2, j], [-j, 3]], det A = 5,
    A^-1 = [[3, -j], [j, 2]] / 5: sinr = 5/3 - 1 and 5/2 - 1, rate = log2(5/3) + log2(5/2) against log2 5 of the joint receiver"""
    H = np.array([[1, 1j], [0, 1]], np.complex128)[None, :, :, None]                       # [1, M_rx = 2, M_tx = 2, K = 1]
    W = np.eye(2)[None]
    rate_c, rate_ck = M.mmse_rate_from_channel(H, W, 2.0)
    sinr = M.mmse_sinr_from_channel(H, W, 2.0)
    np.testing.assert_allclose(sinr[0, 0, :, 0], [2 / 3, 3 / 2], rtol=1e-14)
    np.testing.assert_allclose(rate_c[0, 0], np.log2(5 / 3) + np.log2(5 / 2), rtol=1e-14)
    np.testing.assert_allclose(codebook_rate_from_channel(H, W, 2.0)[0][0, 0], np.log2(5.0), rtol=1e-14)
    tol_c, tol_ck = M.mmse_rate_tolerance(H, W, 2.0)
    assert tol_c.shape == (1, 1) and tol_ck.shape == (1, 1, 1) and 0 < tol_c[0, 0] < 1e-3


def test_tolerance_bounds_what_an_admitted_perturbation_does():
    """the derivation, tried: a perturbation of E of Frobenius norm e moves the rate by less than the first term"""
    from tests._cases import TOL_REL
    from tests._codebook_rate_ref import precoded
    H, W = _random((6, 4, 4, 3), 31) * 10 ** np.random.default_rng(1).uniform(-2, 1, (6, 1, 1, 1)), np.eye(4)[None]
    snr = 50.0
    rate_ck = M.mmse_rate_from_channel(H, W, snr)[1]
    tol_ck = M.mmse_rate_tolerance(H, W, snr)[1]
    E = precoded(H, W)
    e = np.sqrt(4 * 4) * TOL_REL * np.abs(E).reshape(6, -1).max(axis=1)
    for seed in range(5):
        D = _random(H.shape, 40 + seed)
        D *= (e / np.sqrt((np.abs(D) ** 2).sum(axis=(1, 2)).max(axis=-1)))[:, None, None, None]    # |dE_k|_F <= e for every k
        moved = np.abs(M.mmse_rate_from_channel(H + D, W, snr)[1] - rate_ck)
        assert (moved <= tol_ck).all() and moved.max() > 0


# ---- 5. on the oracle: the test tells the receivers apart, and the tolerance hides nothing ----------------------------------------
def _gpu_cases():
    from tests import test_gpu_mmse_rate as g
    return g


def test_the_case_table_covers_what_can_go_wrong():
    from tests import _consumer_shapes as shapes
    g = _gpu_cases()
    ids = [c["id"] for c in g.CASES]
    assert len(set(ids)) == len(ids) and all(c["layers"] >= 2 for c in g.CASES)
    assert {(int(np.prod(c["ue_shape"])), c["layers"]) for c in g.CASES} >= {(m, L) for m, L in shapes.ML_PAIRS if L >= 2}
    by = g.BY_ID
    assert by["mmse_counts_L2"]["rays"] == "counts" and by["mmse_counts_L2"]["ue_shape"] == [2, 1] and by["mmse_counts_L2"]["layers"] == 2
    assert len(by["mmse_K65_L2"]["selected"]) == 65 and len(by["mmse_K70_L2"]["selected"]) == 70
    assert by["mmse_K70_L2"]["bs_shape"] == [8, 1] and by["mmse_K70_L2"]["ue_shape"] == [2, 1]
    assert {len(by[f"slices_K{K}"]["selected"]) for K in (1, 3, 7, 33)} == {1, 3, 7, 33} and "every_count" in by
    for cid, Bs in g.SUBBAND_CASES:
        K = len(by[cid]["selected"])
        assert Bs[0] == 1 and K % Bs[1] != 0 and 1 < Bs[1] < K and Bs[2] >= K
    with open(g.HASHES) as f:
        assert set(json.load(f)) == {c["id"] for c in g.gcb.CASES}


def test_receivers_differ_by_more_than_the_tolerances_on_every_gpu_case():
    g = _gpu_cases()
    for c in g.CASES:
        _, _, H, W, snr, (joint_c, tol_joint) = g.gcb.case_inputs(c)
        mmse_c, tol_mmse = g.mmse_ref(c)
        live = M.live_users(H)
        assert live.any() and mmse_c.shape == joint_c.shape == (c["n"], c["C"])
        loss = (joint_c - mmse_c)[live]
        apart = float((loss > 10 * (tol_mmse + tol_joint)[live]).mean())
        loose = M.loose_share(H, W, snr)
        changed = int((joint_c[live].argmax(axis=1) != mmse_c[live].argmax(axis=1)).sum())
        print(f"{c['id']}: median loss {np.median(loss):.3f} bit, share above 10 tolerances {apart:.2f}, share of loose tolerances "
              f"{loose:.3f}, best codeword differs for {changed} of {int(live.sum())} users")
        assert (loss >= -1e-9).all(), c["id"]                                    # Hadamard: never above the joint rate
        assert (mmse_c >= 0).all() and (mmse_c[~live] == 0).all() and (tol_mmse > 0).all()
        assert apart >= 0.5, (c["id"], apart)
        assert loose <= 0.25, (c["id"], loose)


def test_tolerances_agree_at_one_layer():
    """one elimination of a 1 x 1 matrix: the two modules admit the same"""
    H, W = _random((5, 2, 8, 4), 51) * 1e-3, _random((6, 1, 8), 52)
    a, _ = M.mmse_rate_tolerance(H, W, 3e6)
    b, _ = codebook_rate_tolerance(H, W, 3e6)
    np.testing.assert_allclose(a, b, rtol=1e-10)
