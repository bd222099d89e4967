"""Angle-delay power matrix and delay profile (DMX_FLAG_ANGLE_DELAY_POWER, DMX_FLAG_ANGLE_DELAY_PROFILE) without a GPU: the
header and the C-ABI's host-only answers over every entry point, the `output=` argument of the Python layer, the two
conditions on the oracle that give the GPU criterion of tests/test_gpu_angle_delay_power.py its meaning
(tests/_angle_delay_power_ref.py has the bounds), and the array helpers `dm.tap_delays` and `dm.delay_spread`."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import _angle_delay_power_ref as R
from tests._angle_delay_cases import BY_ID, case_inputs
from tests._angle_delay_ref import adp_from_channel, drop_delta, swap_delta
from tests.test_beam_rsrp_cpu import _every
from tests.test_near_field_cpu import _params as _nf_params
from tests.test_wideband_cpu import _header, _lib

POWER, PROFILE, ADAPTIVE, WIDEBAND, NEAR_FIELD, BEAM_POWER, MMSE = 1024, 4096, 1, 4, 16, 64, 256
BOTH = POWER | PROFILE
N_POWER, N_PROFILE = b"DMX_FLAG_ANGLE_DELAY_POWER", b"DMX_FLAG_ANGLE_DELAY_PROFILE"
TAKEN = ("dmx_channels_angle_delay", "dmx_angle_delay_supported")
NO_NEAR_FIELD = ("dmx_channels_fd_lpf", "dmx_channels_td", "dmx_channels_fd_beams", "dmx_channels_fd_direct", "dmx_fd_direct_supported")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. header, ABI and kernel source ---------------------------------------------------------------------------------------------
def test_header_defines_the_flags_and_the_abi_is_unchanged():
    nat, lib = _lib()
    header = _header()
    assert re.search(r"#define\s+DMX_FLAG_ANGLE_DELAY_POWER\s+1024u\b", header)
    assert re.search(r"#define\s+DMX_FLAG_ANGLE_DELAY_PROFILE\s+4096u\b", header)
    assert re.search(r"#define\s+DMX_ABI_VERSION\s+3\b", header)
    assert nat.FLAG_ANGLE_DELAY_POWER == POWER and nat.FLAG_ANGLE_DELAY_PROFILE == PROFILE
    assert nat.ABI_VERSION == 3 and lib.dmx_version() == 3
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(dmx_\w+)\s*\(", code)) == set(nat.EXPORTED_SYMBOLS) and len(nat.EXPORTED_SYMBOLS) == 37
    assert len(re.findall(r"void\*\s+stream", code)) == 18
    assert [f[0] for f in nat.DmxParams._fields_][-2:] == ["flags", "reserved0"]
    said = [m for m in re.findall(r"/\*.*?\*/", header, flags=re.S) if "DMX_FLAG_ANGLE_DELAY_PROFILE" in m]
    assert len(said) == 2                                                        # at the definitions and at the call
    text = said[0]
    assert set(re.findall(r"\b(dmx_\w+)\s*\(", text)) <= set(nat.EXPORTED_SYMBOLS)
    for word in ("sum_{rx < M_rx} |X[u, rx, r, t]|^2", "sum_{r < n_rows} P[u, r, t]", "values 1024 and 4096",
                 "2, 8, 32, 128, 512 and 2048 stay unknown bits", "valid only together with DMX_FLAG_ANGLE_DELAY_POWER",
                 "DMX_FLAG_ADAPTIVE_TERMS and", "DMX_FLAG_NEAR_FIELD", "dmx_path_prep", "dmx_fd_kernel_choice",
                 "every link of dmx_cell_rate", "WITHOUT", "the options of the beam sweep and of the codebook rate", "FLT_MIN") + TAKEN:
        assert word in text, word
    assert "DMX_FLAG_BEAM_MEAN_POWER" not in text and "DMX_FLAG_RX_LINEAR_MMSE" not in text


def test_kernel_source_selects_the_output_by_a_template_parameter():
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k9_angle_delay.hip")).read())
    assert src.count("__global__") == 1 and "template <int M, int OUT>" in src
    assert all(f"k9_angle_delay<M, {o}>" in src for o in (0, 1, 2)) and src.count("launch_dyn_lds(") == 3
    assert "if constexpr (OUT == 0)" in src and "rows_pair<M>" in src
    assert "atomic" not in src and "__syncthreads" not in src and "blockIdx.y" not in src


# ---- 2. the flag matrix, zero-user calls -------------------------------------------------------------------------------------------
def test_the_call_and_its_query_alone_take_the_flags():
    nat, lib = _lib()
    p = _nf_params(nat, flags=0)
    calls, _keep = _every(nat, lib, p)
    assert len(calls) == 26 and set(TAKEN) <= set(calls)
    for out in (POWER, BOTH):
        for extra in (0, ADAPTIVE, NEAR_FIELD, NEAR_FIELD | ADAPTIVE):
            flags = out | extra
            for name, call in calls.items():
                p.flags = flags
                if name in TAKEN:
                    p.flags = extra
                    want = call()
                    p.flags = flags
                    assert call() == want == (1 if name.endswith("_supported") else 0), (name, flags, lib.dmx_last_error())
                    continue
                assert call() == -1, (name, flags)
                # the new refusal comes after the older ones: where the near field is not taken either, that is what is named
                first = b"DMX_FLAG_NEAR_FIELD" if extra & NEAR_FIELD and name in NO_NEAR_FIELD else N_POWER
                assert first in lib.dmx_last_error(), (name, flags, lib.dmx_last_error())
    # the profile bit alone: refused by name everywhere, by both names where the power bit would be taken
    for extra in (0, ADAPTIVE, NEAR_FIELD):
        p.flags = PROFILE | extra
        for name, call in calls.items():
            assert call() == -1, (name, extra)
            err = lib.dmx_last_error()
            if extra & NEAR_FIELD and name in NO_NEAR_FIELD:
                assert b"DMX_FLAG_NEAR_FIELD" in err, (name, err)
                continue
            assert N_PROFILE in err, (name, err)
            if name in TAKEN:
                assert N_POWER in err, (name, err)
    # a link of dmx_cell_rate that is not the first
    ps = [_nf_params(nat, 0), _nf_params(nat, NEAR_FIELD), _nf_params(nat, POWER)]
    links = (nat.DmxLink * 3)()
    for i, q in enumerate(ps):
        links[i].prm, links[i].n_paths_loaded, links[i].snr_linear = C.pointer(q), 5, 10.0
    for flags, word in ((POWER, N_POWER), (BOTH, N_POWER), (PROFILE, N_PROFILE)):
        ps[2].flags = flags
        for call in (lambda: lib.dmx_cell_rate_supported(links, 3),
                     lambda: lib.dmx_cell_rate(links, 3, 0, 0, 0, None, None, None, None, None, None)):
            assert call() == -1 and word in lib.dmx_last_error(), lib.dmx_last_error()
    ps[2].flags = 0
    assert lib.dmx_cell_rate_supported(links, 3) == 1, lib.dmx_last_error()
    # with the bits clear every call answers as before
    p.flags = 0
    for name, call in calls.items():
        if name not in ("dmx_channels_fd_lpf", "dmx_channels_td", "dmx_channels_fd_direct"):      # refuse these parameters anyway
            assert call() in (0, 1, 9, 12, 2), (name, lib.dmx_last_error())


def test_other_bits_and_other_checks_answer_as_before():
    nat, lib = _lib()
    p = _nf_params(nat, flags=0)
    calls, _keep = _every(nat, lib, p)
    del calls["dmx_fd_kernel_choice"]                                            # never looked at unknown bits
    for flags in (POWER | 2, POWER | 8, BOTH | 32, POWER | 128, BOTH | 512, POWER | 2048, POWER | (1 << 31), 2048, 8192):
        p.flags = flags
        for name, call in calls.items():
            assert call() == -1, (name, flags)
            assert b"unknown bits in dmx_params.flags / reserved0" in lib.dmx_last_error(), (name, flags, lib.dmx_last_error())
    p.flags, p.reserved0 = BOTH, 1
    for name, call in calls.items():
        assert call() == -1 and b"unknown bits" in lib.dmx_last_error(), name
    p.reserved0 = 0
    ad, q = calls["dmx_channels_angle_delay"], calls["dmx_angle_delay_supported"]
    # the refusals of the older options come first, in their words; the wide band stays refused; near field needs its carrier
    for flags, word in ((POWER | WIDEBAND, b"DMX_FLAG_SPATIAL_WIDEBAND"), (BOTH | BEAM_POWER, b"DMX_FLAG_BEAM_MEAN_POWER"),
                        (POWER | MMSE, b"DMX_FLAG_RX_LINEAR_MMSE")):
        p.flags = flags
        for call in (ad, q):
            assert call() == -1 and word in lib.dmx_last_error() and N_POWER not in lib.dmx_last_error(), (flags, lib.dmx_last_error())
    p.flags = BOTH | BEAM_POWER
    assert calls["dmx_beam_power"]() == -1 and N_POWER in lib.dmx_last_error()
    p.flags = POWER | MMSE
    assert calls["dmx_codebook_rate"]() == -1 and N_POWER in lib.dmx_last_error()
    p.flags, p.carrier_freq = BOTH | NEAR_FIELD, 0.0
    assert ad() == -1 and b"DMX_FLAG_NEAR_FIELD" in lib.dmx_last_error() and b"carrier_freq" in lib.dmx_last_error()
    p.carrier_freq = 28e9
    # the flags change none of the call's other checks, and no shape limit
    pp = C.byref(p)
    for flags in (0, POWER, BOTH):
        p.flags = flags
        assert ad() == 0 and q() == 1, lib.dmx_last_error()
        assert lib.dmx_angle_delay_supported(pp, 5, 8, 8, 9) == 0 and b"n_taps = 9" in lib.dmx_last_error()
        assert lib.dmx_angle_delay_supported(pp, 5, 0, 8, 4) == 0 and b"n_rows = 0" in lib.dmx_last_error()
        assert lib.dmx_channels_angle_delay(pp, None, 0, 5, 0, 0, None, 7, None, 0, 8, 4, None, None) == -1
        assert b"without a codebook the rows are the" in lib.dmx_last_error()
        assert lib.dmx_channels_angle_delay(pp, None, 4, 5, 0, 2, None, 8, None, 0, 8, 4, None, None) == -1
        assert b"workspace/out is NULL" in lib.dmx_last_error()
    # the float32 outputs need 4-byte alignment where the complex one needs 8
    for flags, addr, want in ((0, 4, b"out must be 8-byte aligned"), (POWER, 4, None), (BOTH, 4, None), (POWER, 2, b"out must be 4-byte aligned"),
                              (BOTH, 6, b"out must be 4-byte aligned"), (0, 8, None)):
        p.flags = flags
        rc = lib.dmx_channels_angle_delay(pp, None, 0, 5, 0, 0, None, 8, None, 0, 8, 4, C.c_void_p(addr), None)
        assert (rc, None) == (0, want) or (rc == -1 and want in lib.dmx_last_error()), (flags, addr, rc, lib.dmx_last_error())
    p.flags = BOTH
    p.rx_filter = 1
    assert ad() == -1 and b"dmx_channels_angle_delay does not cover rx_filter = 1" in lib.dmx_last_error()


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


BAD_OUTPUTS = ["Power", "adp", "pdp", "", None, 1, True, b"power", ("power",)]


@pytest.mark.parametrize("output", BAD_OUTPUTS)
def test_a_bad_output_is_a_value_error_on_every_call(output, monkeypatch):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd import engine

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    ds, p = _dataset(), _dm_params()
    calls = {
        "check": lambda: engine.check_angle_delay_output("x", output),
        "host check": lambda: engine.check_angle_delay_call(_dm_params().validate(6), 5, 8, 8, 4, output),
        # the first thing the engine's methods do: no engine (and so no GPU) is needed to be refused
        "engine": lambda: engine.ChannelEngine.angle_delay(None, None, 4, output=output),
        "engine query": lambda: engine.ChannelEngine.angle_delay_supported(None, None, 8, 8, 4, output),
        "dataset": lambda: ds.compute_angle_delay(p, n_taps=4, output=output),
        "before n_taps": lambda: ds.compute_angle_delay(p, output=output),
        "near field": lambda: ds.near_field().compute_angle_delay(p, n_taps=4, output=output),
        "macro fan-out": lambda: dm.MacroDataset([_dataset(), _dataset()]).compute_angle_delay(p, n_taps=4, output=output),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="output must be 'complex', 'power' or 'profile'"):
            call()


def test_output_names_defaults_and_the_host_check_with_the_flags(monkeypatch):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd import engine
    assert engine.ANGLE_DELAY_OUTPUTS == ("complex", "power", "profile")
    assert [engine.check_angle_delay_output("x", o) for o in engine.ANGLE_DELAY_OUTPUTS] == [0, POWER, BOTH]
    for f in (engine.ChannelEngine.angle_delay, engine.ChannelEngine.angle_delay_supported, engine.check_angle_delay_call,
              dm.Dataset.compute_angle_delay):
        assert inspect.signature(f).parameters["output"].default == "complex", f
    assert list(inspect.signature(dm.Dataset.compute_angle_delay).parameters)[1:] == ["params", "n_taps", "n_fft", "codebook", "output"]
    ok = _dm_params().validate(6)
    assert [engine.check_angle_delay_call(ok, 5, 8, None, 4, o) for o in engine.ANGLE_DELAY_OUTPUTS] == [8, 8, 8]
    # the output changes no other refusal: they come before any GPU work, with the library's words
    monkeypatch.setattr(dsm, "_engine", lambda: (_ for _ in ()).throw(AssertionError("the GPU engine was asked for")))
    ds = _dataset()
    for output in ("power", "profile"):
        with pytest.raises(ValueError, match="n_taps = 9"):
            ds.compute_angle_delay(_dm_params(), n_taps=9, output=output)
        with pytest.raises(ValueError, match="n_taps .keyword. is required"):
            ds.compute_angle_delay(_dm_params(), output=output)
        td = _dm_params()
        td.freq_domain = 0
        with pytest.raises(ValueError, match="freq_domain"):
            ds.compute_angle_delay(td, n_taps=4, output=output)
        uneven = _dm_params()
        uneven.ofdm.selected_subcarriers = np.array([0, 1, 3])
        with pytest.raises(ValueError, match="uniformly spaced"):
            ds.compute_angle_delay(uneven, n_taps=2, output=output)


def test_host_copy_guard_counts_the_chosen_output(monkeypatch):
    """n_ue * 8 M_rx R T bytes for the complex tensor, 4 R T for the power matrix, 4 T for the profile"""
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    seen = []
    monkeypatch.setattr(dm.Dataset, "_guard_host_copy", lambda self, nbytes: seen.append(int(nbytes)))
    monkeypatch.setattr(dsm, "_engine", lambda: (_ for _ in ()).throw(RuntimeError("stop here")))
    ds = _dataset()
    for output in ("complex", "power", "profile"):
        with pytest.raises(RuntimeError, match="stop here"):
            ds.compute_angle_delay(_dm_params(), n_taps=4, output=output)
    assert seen == [6 * 8 * 2 * 8 * 4, 6 * 4 * 8 * 4, 6 * 4 * 4]


# ---- 4. the two conditions on the oracle that give the GPU criterion its meaning ------------------------------------------------------
@pytest.mark.parametrize("cid", ["equal_power_dft", "equal_power_ant"])
def test_a_wrong_path_moves_both_references_by_ten_bounds(cid):
    """every dropped kept path, and every exchanged pair of neighbouring delay rows, of every user"""
    c = BY_ID[cid]
    X_cf, facs = case_inputs(c)[4:6]
    P_ref, p_ref, tol_P, tol_p = R.case_power_ref(c)
    worst = {"drop P": np.inf, "drop p": np.inf, "swap P": np.inf, "swap p": np.inf}
    for u, fac in enumerate(facs):
        assert fac is not None
        n = len(fac[2])
        P0, p0 = R.power_from_adp(X_cf[u:u + 1])
        for kind, delta, count in (("drop", drop_delta, n), ("swap", swap_delta, n - 1)):
            for l in range(count):
                P1, p1 = R.power_from_adp((X_cf[u] + delta(fac, l))[None])
                worst[kind + " P"] = min(worst[kind + " P"], float((np.abs(P1 - P0)[0] / tol_P[u]).max()))
                worst[kind + " p"] = min(worst[kind + " p"], float((np.abs(p1 - p0)[0] / tol_p[u]).max()))
    print(cid, {k: round(v, 1) for k, v in worst.items()})
    assert all(v >= 10 for v in worst.values()), worst


@pytest.mark.parametrize("cid", ["equal_power_dft", "equal_power_ant", "defaults_K512_dft", "mrx8", "rows65", "taps128_ant"])
def test_the_complex64_rounding_of_the_reference_stays_inside_the_bound(cid):
    c = BY_ID[cid]
    X_ref = case_inputs(c)[3]
    P_ref, p_ref, tol_P, tol_p = R.case_power_ref(c)
    P64, p64 = R.power_from_adp(X_ref.astype(np.complex64))
    assert R.worst_ratio(P64, P_ref, tol_P) <= 1 and R.worst_ratio(p64, p_ref, tol_p) <= 1
    peak = P_ref.reshape(c["n"], -1).max(axis=1)
    live = peak > 0
    assert (tol_P.reshape(c["n"], -1).max(axis=1)[live] <= 2e-4 * peak[live]).all()      # the bound is tight: 1.4e-4 of the peak at most


def test_reference_is_the_definition_and_the_bounds_are_those_of_the_module():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(3, 2, 5, 4)) + 1j * rng.normal(size=(3, 2, 5, 4))
    X[1] = 0
    P, p = R.power_from_adp(X)
    assert np.allclose(P, (np.abs(X) ** 2).sum(axis=1), rtol=1e-14) and np.allclose(p, P.sum(axis=1), rtol=1e-14)
    tol_P, tol_p = R.power_bounds(X)
    from tests._cases import TOL_REL
    b = TOL_REL * np.abs(X[0]).max()
    want = (2 * np.abs(X[0]) * b + b * b).sum(axis=0) + 4 * 2.0 ** -24 * P[0]
    assert np.allclose(tol_P[0], want, rtol=1e-13) and np.allclose(tol_p[0], want.sum(axis=0) + 6 * 2.0 ** -24 * p[0], rtol=1e-13)
    assert (tol_P[1] == 0).all() and (tol_p[1] == 0).all() and (tol_P[[0, 2]] > 0).all()


# ---- 5. the array helpers ------------------------------------------------------------------------------------------------------------
def test_tap_delays():
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.ofdm.subcarriers, p.ofdm.bandwidth = 512, 20e6
    p.ofdm.selected_subcarriers = np.arange(512)
    d = dm.tap_delays(p, 32)
    assert d.dtype == np.float64 and d.shape == (32,) and np.array_equal(d, np.arange(32) / 20e6)     # the sample time
    p.ofdm.selected_subcarriers = np.arange(3, 3 + 8 * 40, 8)
    assert np.allclose(dm.tap_delays(p, 24, n_fft=64), np.arange(24) * 512 / (64 * 8 * 20e6), rtol=1e-15)
    assert np.allclose(dm.tap_delays(p, 40), np.arange(40) * 512 / (40 * 8 * 20e6), rtol=1e-15)
    p.ofdm.selected_subcarriers = np.array([7])
    assert np.array_equal(dm.tap_delays(p, 1), [0.0])
    for bad, kw in ((np.array([0, 1, 3]), dict(n_taps=2)), (np.arange(8), dict(n_taps=9)), (np.arange(8), dict(n_taps=0)),
                    (np.arange(8), dict(n_taps=4, n_fft=7)), (np.arange(8), dict(n_taps=4.0)), (np.arange(8), dict(n_taps=4, n_fft=True))):
        p.ofdm.selected_subcarriers = bad
        with pytest.raises(ValueError, match="tap_delays"):
            dm.tap_delays(p, **kw)


def test_delay_spread_on_hand_made_profiles():
    import torch
    import deepmimo_amd as dm
    delays = np.arange(8) * 50e-9
    prof = np.zeros((4, 8), np.float32)
    prof[0, 5] = 3e-9                                                        # one tap
    prof[1, 2] = prof[1, 6] = 1.0                                            # two equal taps: mean between, spread half the distance
    prof[2] = [4, 0, 0, 0, 1, 0, 0, 0]                                       # user 3: all zero
    mean, rms = dm.delay_spread(prof, delays)
    assert isinstance(mean, np.ndarray) and mean.dtype == rms.dtype == np.float64 and mean.shape == rms.shape == (4,)
    assert mean[0] == delays[5] and rms[0] == 0
    assert np.isclose(mean[1], 200e-9, rtol=1e-15) and np.isclose(rms[1], 100e-9, rtol=1e-15)
    m2 = 0.2 * 200e-9
    assert np.isclose(mean[2], m2, rtol=1e-14) and np.isclose(rms[2], np.sqrt(0.8 * m2 ** 2 + 0.2 * (200e-9 - m2) ** 2), rtol=1e-14)
    assert np.isnan(mean[3]) and np.isnan(rms[3])
    tm, tr = dm.delay_spread(torch.from_numpy(prof), delays)
    assert isinstance(tm, torch.Tensor) and tm.dtype == tr.dtype == torch.float64 and tm.device.type == "cpu"
    assert np.array_equal(tm.numpy(), mean, equal_nan=True) and np.allclose(tr.numpy(), rms, rtol=1e-15, atol=0, equal_nan=True)
    one_m, one_r = dm.delay_spread(prof[1], delays)                          # a single profile
    assert np.shape(one_m) == () and float(one_m) == mean[1] and float(one_r) == rms[1]
    with pytest.raises(ValueError, match="delay_spread"):
        dm.delay_spread(prof, delays[:7])


def test_a_single_path_on_tap_5_of_a_full_grid():
    """the oracle's channel of one path sitting exactly on tap 5, full grid: the profile is that tap alone, up to rounding
    1e-25 below it, so the mean excess delay is delays[5] and the spread vanishes"""
    import deepmimo_amd as dm
    c = BY_ID["on_tap_ant"]
    rays = {k: v[1:2, :1].copy() if v.ndim == 2 and v.shape[1] == c["L"] else v[1:2].copy() for k, v in case_inputs(c)[0].items()}
    from tests._cases import oracle_params
    op = oracle_params(dict(c, n=1, L=1, num_paths=1), np.array(c["ue_rot"]))
    H = onp.compute_channels(rays, op)["channel"]
    P, p = R.power_from_adp(adp_from_channel(H, None, 512, 512))
    assert p[0].argmax() == 5 and (np.delete(p[0], 5) <= 1e-12 * p[0, 5]).all()
    prm = dm.ChannelGenParameters()
    prm.ofdm.subcarriers, prm.ofdm.bandwidth = 512, c["bandwidth"]
    prm.ofdm.selected_subcarriers = np.arange(512)
    delays = dm.tap_delays(prm, 512)
    assert delays[5] == float(rays["delay"][0, 0])                               # the tap's delay is the path's
    mean, rms = dm.delay_spread(np.where(p >= 1e-12 * p.max(), p, 0.0), delays)
    assert mean[0] == delays[5] and rms[0] == 0
    mean, rms = dm.delay_spread(p, delays)                                       # with the rounding residue of the other taps
    assert abs(mean[0] - delays[5]) <= 1e-9 * delays[5] and rms[0] <= 1e-4 * delays[1]


def test_profile_of_an_orthonormal_codebook_is_the_antenna_domain_profile():
    """Parseval over the rows: F unitary leaves sum_r |F a|^2 = sum_tx |a|^2, tap by tap"""
    for a, b in (("equal_power_dft", "equal_power_ant"), ("defaults_K64_dft", "defaults_K64_ant"), ("taps65_dft", "taps65_ant")):
        pa, pb = R.case_power_ref(BY_ID[a])[1], R.case_power_ref(BY_ID[b])[1]
        assert pa.shape == pb.shape and np.allclose(pa, pb, rtol=1e-12, atol=0)
        assert not np.allclose(R.case_power_ref(BY_ID[a])[0], R.case_power_ref(BY_ID[b])[0], rtol=1e-3, atol=0)     # the matrices differ
