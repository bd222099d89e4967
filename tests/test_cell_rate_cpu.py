"""Host side of the multi-cell rate (dmx_cell_rate_supported / dmx_cell_rate, k8_cell_rate.hip) - no GPU: the symbols, the
"taken / refused" list of the shape query against a restatement of the launcher's LDS rule, the errors that must come before
any GPU call, the pinned reference of the GPU tests (hand cases, float64 NumPy) and the condition on the GPU tests' inputs
(the derived tolerance must stay below 1 % of the rate on all but 5 % of a case's live entries)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._cell_rate_ref import (cell_rate_from_channels, cell_rate_tolerance, link_snr_reference, link_snrs,
                                  reference_serving, tolerance_share)
from tests._rate_ref import rate_from_channel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepmimo_amd", "lib", "libdeepmimo_amd.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

LDS_MAX = 156 * 1024
SYMBOLS = ("dmx_cell_rate_supported", "dmx_cell_rate")


def _params(bs=(8, 1), ue=(1, 1), K=1, num_paths=25, freq_domain=1, rx_filter=0, N=512):
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = num_paths, freq_domain, N, K, 10e6
    p.rx_filter = rx_filter
    sel = (C.c_int32 * max(K, 1))()
    p._keep = sel
    p.selected_subcarriers = C.addressof(sel)
    return p


def _links(params, loaded=25, snr=100.0, ws=None):
    from deepmimo_amd import _native as n
    arr = (n.DmxLink * max(len(params), 1))()
    loaded = loaded if isinstance(loaded, (list, tuple)) else [loaded] * len(params)
    snr = snr if isinstance(snr, (list, tuple)) else [snr] * len(params)
    for b, p in enumerate(params):
        arr[b].prm = C.pointer(p)
        arr[b].workspace = ws
        arr[b].n_paths_loaded = loaded[b]
        arr[b].snr_linear = snr[b]
    arr._keep = list(params)
    return arr


def cell_lds_rule(shapes, K):
    """Waves per workgroup of the launcher, restated (0: not taken).  shapes: (bs, ue, P) per link.  One wave holds the
    tables of the largest link, max_b (M_rx + M_tx_b + kc) * P_b * 8 bytes, kc = min(K, 64), M_rx <= 8, P_b in 1..32."""
    most = 0
    for bs, ue, P in shapes:
        m_tx, m_rx = bs[0] * bs[1], ue[0] * ue[1]
        if not (1 <= P <= 32) or K < 1 or m_rx > 8:
            return 0
        most = max(most, (m_rx + m_tx + min(K, 64)) * P * 8)
    return 4 if 4 * most <= 65536 else 2 if 2 * most <= 65536 else 1 if most <= LDS_MAX else 0


def test_header_and_binding_name_the_new_entry_points():
    from deepmimo_amd import _native as n
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, hdr) and sym in n.EXPORTED_SYMBOLS
    flat = re.sub(r"[ \t]+", " ", hdr)
    assert n.ABI_VERSION == 3 and "#define DMX_ABI_VERSION 3" in flat
    assert "#define DMX_MAX_LINKS 8" in flat and n.MAX_LINKS == 8 and "typedef struct dmx_link" in flat
    assert "max_b (M_rx + M_tx,b + kc) * P_b * 8" in hdr and "159744" in hdr    # the header states the LDS formula
    assert C.sizeof(n.DmxLink) == 32 and n.DmxLink.snr_linear.offset == 24 and n.DmxLink.n_paths_loaded.offset == 16


@needs_lib
def test_library_exports_the_symbols_with_abi_3():
    from deepmimo_amd import _native as n
    lib = n.load()
    assert lib.dmx_version() == 3
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None


@needs_lib
def test_supported_links_without_a_gpu():
    """the whole "taken / refused" list; workspace NULL throughout"""
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    q = lambda ps, loaded=25: lib.dmx_cell_rate_supported(_links(ps, loaded), len(ps))    # noqa: E731
    assert q([_params()]) == 1                                                # one link: DeepMIMO's defaults
    assert q([_params()] * 8) == 1
    assert q([_params((64, 4), (2, 2), 512)] * 3) == 1                        # the headline panel, 25 paths, three cells
    assert q([_params((64, 4), (2, 2), 512)] * 8) == 1                        # ... for any number of cells
    assert q([_params((8, 8), (2, 1), 3), _params((4, 2), (2, 1), 3), _params((16, 1), (2, 1), 3)], [25, 10, 32]) == 1
    assert q([_params((2, 1), (4, 2), 3)] * 3) == 1                           # M_tx < M_rx: the Gram stays on the UE side
    assert q([_params((8, 4), (4, 2), 3)] * 2) == 1                           # M_rx = 8
    assert q([_params(), _params((32, 32), (1, 1))]) == 0 and "LDS" in err() and "link 1" in err()   # a 32 x 32 panel on one link
    assert q([_params((8, 4), (3, 3), 3)] * 2) == 0 and "8 elements" in err()                  # M_rx = 9
    assert q([_params((2, 1), (4, 4), 3)]) == 0 and "8 elements" in err()                      # M_rx = 16 although M_tx = 2
    assert q([_params(ue=(2, 1)), _params(ue=(1, 2))]) == 0 and "ue_shape" in err()
    assert q([_params(ue=(2, 1)), _params(ue=(1, 1))]) == 0 and "ue_shape" in err()
    assert q([_params(K=3), _params(K=4)]) == 0 and "selection" in err()
    assert q([_params(N=512), _params(N=256)]) == 0 and "n_subcarriers" in err()
    assert lib.dmx_cell_rate_supported(_links([_params()]), 0) == 0 and "DMX_MAX_LINKS" in err()
    assert q([_params()] * 9) == 0 and "1..8" in err()
    assert q([_params(), _params(num_paths=33)], 40) == 0 and "32" in err() and "link 1" in err()      # P = 33
    assert q([_params(), _params(num_paths=32)], 40) == 1
    assert q([_params(), _params()], [25, 0]) == 0
    assert q([_params(), _params(freq_domain=0)]) == 0 and "freq_domain" in err()
    assert q([_params(rx_filter=1), _params()]) == 0 and "rx_filter" in err()
    assert q([_params(K=0)] * 2) == 0
    assert q([_params(), _params()], [25, -1]) == -1
    assert lib.dmx_cell_rate_supported(None, 2) == -1 and "links is NULL" in err()
    broken = _links([_params(), _params()])
    broken[1].prm = None
    assert lib.dmx_cell_rate_supported(broken, 2) == -1 and "params is NULL" in err()
    # the edge of the byte rule at 25 paths on the last link: M_rx + M_tx + kc <= 798
    assert q([_params(), _params((796, 1), (1, 1))]) == 1 and q([_params(), _params((797, 1), (1, 1))]) == 0
    assert "(1 + 797 + 1) * 25 * 8 = 159800 bytes" in err() and str(LDS_MAX) in err()


@needs_lib
def test_supported_equals_the_lds_rule():
    from deepmimo_amd import _native as n
    lib = n.load()
    rng = np.random.default_rng(14)
    seen = {0: 0, 1: 0}
    for _ in range(1500):
        B = int(rng.integers(1, 9))
        ue = (int(rng.integers(1, 5)), int(rng.integers(1, 4)))
        K = int(rng.integers(1, 100))
        shapes, ps, loaded = [], [], []
        for _b in range(B):
            bs = (int(rng.integers(1, 65)), int(rng.integers(1, 17)))
            L, num_paths = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            shapes.append((bs, ue, min(L, num_paths)))
            ps.append(_params(bs, ue, K, num_paths))
            loaded.append(L)
        want = 1 if cell_lds_rule(shapes, K) else 0
        seen[want] += 1
        got = lib.dmx_cell_rate_supported(_links(ps, loaded), B)
        assert got == want, (shapes, K, want, got)
    assert all(v > 100 for v in seen.values()), seen


@needs_lib
def test_argument_errors_without_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    buf = (C.c_char * 65536)()
    base = (C.addressof(buf) + 255) // 256 * 256
    out = C.c_void_p(base + 4096)

    def call(ps, b=0, cnt=4, snr=100.0, o=out, ok=None, sv=None, osv=None, ols=None, L=25, ws=base, n_links=None):
        return lib.dmx_cell_rate(_links(ps, L, snr, ws), len(ps) if n_links is None else n_links, 4, b, cnt, sv, o, ok, osv, ols, None)
    two = [_params(), _params()]
    assert call([_params(), _params(freq_domain=0)]) == -1 and "freq_domain" in err()
    assert call([_params(rx_filter=1), _params()]) == -1 and "rx_filter" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(two, snr=[100.0, bad]) == -1 and "snr_linear" in err() and "link 1" in err()
    assert call(two, b=2, cnt=4) == -1 and "user range" in err()
    assert call(two, o=None) == -1 and "NULL" in err()
    assert call(two, ws=None) == -1 and "NULL" in err()
    assert call(two, ws=base + 8) == -4 and "256-byte aligned" in err()
    for kw in ("o", "ok", "sv", "osv", "ols"):
        assert call(two, **{kw: C.c_void_p(base + 8194)}) == -1 and "4-byte aligned" in err()
    assert lib.dmx_cell_rate(None, 2, 4, 0, 4, None, out, None, None, None, None) == -1 and "links is NULL" in err()
    assert call([_params(), _params((32, 32), (1, 1), 1)]) == -2 and "LDS" in err()
    assert call([_params((8, 4), (3, 3), 2)] * 2) == -2 and "8 elements" in err()
    assert call([_params(), _params(num_paths=33)], L=40) == -2 and "32" in err()
    assert call([_params(K=3), _params(K=4)]) == -2 and "selection" in err()
    assert call([_params(ue=(2, 1)), _params()]) == -2 and "ue_shape" in err()
    assert call(two, n_links=0) == -2 and call([_params()] * 9) == -2 and "DMX_MAX_LINKS" in err()
    assert call(two, cnt=0) == 0                                              # nothing to do: success before any GPU call


def _macro(n_ues=(5, 5), L=25):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    ds = [dm.Dataset({k: v.copy() for k, v in onp.synth_rays(n, L, seed=2 + i).items()}) for i, n in enumerate(n_ues)]
    return dm, dm.MacroDataset(ds)


@needs_lib
def test_check_cell_rate_call_and_macro_dataset_errors_come_before_any_gpu_call(monkeypatch):
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd.engine import check_cell_rate_call
    dm, macro = _macro()

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    ok = dm.ChannelGenParameters().validate(5)
    assert check_cell_rate_call([ok, ok], [25, 25], 20.0) == [100.0, 100.0]
    assert check_cell_rate_call([ok, ok, ok], [25, 10, 32], [20.0, 3, 0]) == [100.0, 10.0 ** 0.3, 1.0]
    for bad in (float("nan"), float("inf"), None, "20", [20.0, float("nan")], [20.0], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="snr_db"):
            check_cell_rate_call([ok, ok], [25, 25], bad)
    for bad in (float("nan"), "20", [20.0, float("inf")], [20.0] * 3):
        with pytest.raises(ValueError, match="snr_db"):
            macro.compute_cell_rate(dm.ChannelGenParameters(), snr_db=bad)
    with pytest.raises(ValueError, match="snr_db"):                           # missing
        macro.compute_cell_rate(dm.ChannelGenParameters())
    with pytest.raises(TypeError):                                            # keyword-only
        macro.compute_cell_rate(dm.ChannelGenParameters(), 20.0)
    with pytest.raises(ValueError, match="n_ue"):
        _macro((5, 6))[1].compute_cell_rate(snr_db=20.0)
    with pytest.raises(ValueError, match="1..8"):
        _macro((3,) * 9)[1].compute_cell_rate(snr_db=20.0)
    with pytest.raises(ValueError, match="1..8"):
        dm.MacroDataset([]).compute_cell_rate(snr_db=20.0)
    with pytest.raises(ValueError, match="1..8"):
        check_cell_rate_call([ok] * 9, [25] * 9, 20.0)
    with pytest.raises(ValueError, match="parameter sets"):
        macro.compute_cell_rate([dm.ChannelGenParameters()] * 3, snr_db=20.0)
    for bad in (np.zeros(4, np.int32), np.zeros(5), "0", 1.5):
        with pytest.raises(ValueError, match="serving"):
            macro.compute_cell_rate(snr_db=20.0, serving=bad)

    def both(change):
        a, b = dm.ChannelGenParameters(), dm.ChannelGenParameters()
        change(b)
        return [a, b]
    p = both(lambda b: setattr(b, "freq_domain", 0))
    with pytest.raises(ValueError, match="freq_domain"):
        macro.compute_cell_rate(p, snr_db=20.0)
    with pytest.raises(ValueError, match="freq_domain"):
        check_cell_rate_call(p, [25, 25], 20.0)
    p = both(lambda b: setattr(b.ofdm, "rx_filter", 1))
    with pytest.raises(ValueError, match="rx_filter"):
        macro.compute_cell_rate(p, snr_db=20.0)
    p = both(lambda b: setattr(b.bs_antenna, "shape", np.array([32, 32])))
    with pytest.raises(ValueError, match=r"link 1.*LDS"):
        macro.compute_cell_rate(p, snr_db=20.0)
    p = both(lambda b: setattr(b.ue_antenna, "shape", np.array([2, 1])))
    with pytest.raises(ValueError, match="ue_shape"):
        macro.compute_cell_rate(p, snr_db=20.0)
    p = both(lambda b: setattr(b.ofdm, "selected_subcarriers", np.array([1])))
    with pytest.raises(ValueError, match="selection"):
        macro.compute_cell_rate(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([3, 3])
    with pytest.raises(ValueError, match="8 elements"):
        macro.compute_cell_rate(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.num_paths = 33
    with pytest.raises(ValueError, match=r"1\.\.32 paths"):
        _macro(L=40)[1].compute_cell_rate(p, snr_db=20.0)


@needs_lib
def test_valid_call_without_a_gpu_raises_the_usual_error_and_the_method_is_real(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    dm, macro = _macro()
    with pytest.raises(RuntimeError, match="no GPU"):
        macro.compute_cell_rate(dm.ChannelGenParameters(), snr_db=20.0)
    with pytest.raises(RuntimeError, match="no GPU"):
        dm.MacroDataset(macro.datasets[:1]).compute_cell_rate(snr_db=[20.0])             # one child is valid
    assert "compute_cell_rate" in vars(dm.MacroDataset) and "compute_cell_rate" not in dm.MacroDataset.PROPAGATE_METHODS
    assert not hasattr(dm.Dataset, "compute_cell_rate")                                  # Dataset itself gets nothing new
    assert "compute_rate" in dm.MacroDataset.PROPAGATE_METHODS                           # the fan-out is unchanged


def _random_links(rng, n, m_rx, m_txs, K, scale=1.0):
    return [(rng.normal(size=(n, m_rx, m, K)) + 1j * rng.normal(size=(n, m_rx, m, K))) * scale for m in m_txs]


def test_reference_one_link_is_the_single_link_rate():
    rng = np.random.default_rng(5)
    for m_rx, m_tx in ((2, 8), (4, 4), (1, 5), (3, 2)):
        H = _random_links(rng, 6, m_rx, [m_tx], 7)[0] * 10 ** rng.uniform(-3, 1, (6, 1, 1, 1))
        a, ak = cell_rate_from_channels([H], [37.0], np.zeros(6, int))
        b, bk = rate_from_channel(H, 37.0)
        np.testing.assert_allclose(a, b, rtol=1e-10)
        np.testing.assert_allclose(ak, bk, rtol=1e-10)
        tol, tol_k = cell_rate_tolerance([H], [37.0], np.zeros(6, int))
        assert (tol > 0).all() and (tol_k > 0).all() and tol.shape == (6,) and tol_k.shape == (6, 7)


def test_reference_two_identical_links_single_antenna_ue():
    """M_rx = 1, two identical links: x = rho |h|^2 on both, rate = log2(1 + x / (1 + x))"""
    rng = np.random.default_rng(6)
    H = _random_links(rng, 5, 1, [4], 3)[0]
    x = 2.5 / 4 * (np.abs(H) ** 2).sum(axis=(1, 2))
    for s in (0, 1):
        rate, rate_k = cell_rate_from_channels([H, H], [2.5, 2.5], np.full(5, s))
        np.testing.assert_allclose(rate_k, np.log2(1 + x / (1 + x)), rtol=1e-12)
        np.testing.assert_allclose(rate, np.log2(1 + x / (1 + x)).mean(axis=1), rtol=1e-12)


def test_reference_zero_interferer_changes_nothing_and_interference_never_raises_the_rate():
    rng = np.random.default_rng(7)
    Hs = _random_links(rng, 8, 3, [6, 2, 5], 4, scale=0.3)
    snrs = [20.0, 5.0, 9.0]
    s = np.array([0, 1, 2, 0, 1, 2, -1, 3])
    rate, rate_k = cell_rate_from_channels(Hs, snrs, s)
    assert (rate[6:] == 0).all() and (rate_k[6:] == 0).all()                  # not served
    with_zero = cell_rate_from_channels(Hs + [np.zeros((8, 3, 7, 4))], snrs + [1e6], s)
    np.testing.assert_allclose(with_zero[1], rate_k, rtol=1e-12, atol=1e-15)
    for b in range(3):                                                        # each user alone on its serving link
        u = s == b
        alone, alone_k = cell_rate_from_channels([Hs[b][u]], [snrs[b]], np.zeros(int(u.sum()), int))
        assert (rate_k[u] <= alone_k + 1e-12).all() and (rate_k[u] < alone_k).any()
    louder = cell_rate_from_channels(Hs, [20.0, 50.0, 90.0], np.zeros(8, int))[1]
    assert (louder <= cell_rate_from_channels(Hs, snrs, np.zeros(8, int))[1] + 1e-12).all()
    assert (rate_k >= 0).all()


def test_reference_link_snr_and_serving():
    """|H_td[u, 0, 0, s]|^2 is the path power: link_snr = snr / N * sum of powers; the serving index is the first argmax"""
    p = np.array([[4.0, 1.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0]])
    H_td = np.sqrt(p)[:, None, None, :] * np.exp(1j * np.arange(6).reshape(1, 2, 3, 1)) * np.ones((3, 2, 3, 3))
    ref, tol = link_snr_reference(H_td, 640.0, 64)
    np.testing.assert_allclose(ref, [50.0, 0.0, 60.0])
    assert (tol >= 40 * 2.0 ** -24 * ref).all() and (tol[[0, 2]] < 1e-3 * ref[[0, 2]]).all() and tol[1] == 0
    ls = np.array([[1.0, 3.0, 3.0], [0.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
    live = ls > 0
    assert list(reference_serving(ls, live)) == [1, -1, 0]
    Hs = [np.ones((4, 1, 2, 1)) * g for g in (1.0, 2.0)]
    assert link_snrs(Hs, 20.0, 10.0) == [100.0 * 2 / 2.0, 10.0 * 2 / 8.0]


@needs_lib
def test_tolerance_share_condition_of_every_gpu_case():
    """The tolerance may exceed 1 % of max(1, rate_ref) on at most 5 % of a case's live (user, k) entries, otherwise the GPU
    test would hide failures.  The inputs are the GPU tests' own (tests/test_gpu_cell_rate.py), from the NumPy oracle alone:
    the serving index is the first argmax of the reference link_snr, and for the cases the GPU test also runs with a given
    serving index, that one."""
    from tests import test_gpu_cell_rate as g
    for cell in g.CASES:
        links, snrs = g.case_inputs(cell)
        Hs = [l[2] for l in links]
        ls_ref, _, live = g.link_snr_refs(cell)
        s = reference_serving(ls_ref, live)
        share = tolerance_share(Hs, snrs, s)
        print(f"{cell['id']}: snr {', '.join(f'{10 * np.log10(x):.1f}' for x in snrs)} dB, {int((s >= 0).sum())} served, share of "
              f"entries with tol > 1 % = {share:.4f}")
        assert share <= 0.05, (cell["id"], share)
        assert snrs == link_snrs(Hs, cell["serving_db"], cell["inr_db"])
    n = g.BY_ID["counts_and_holes"]["links"][0]["n"]
    links, snrs = g.case_inputs(g.BY_ID["counts_and_holes"])
    assert tolerance_share([l[2] for l in links], snrs, np.zeros(n, int)) <= 0.05
    for cid in ("defaults", "panel", "B8"):                                  # test_explicit_serving's arrays
        links, snrs = g.case_inputs(g.BY_ID[cid])
        B, n = len(links), links[0][2].shape[0]
        given = np.array([(-1, 0, 1, B - 1, B, 2 ** 31 - 1, -7, 0)[u % 8] for u in range(n)])
        for s in (given, np.full(n, B - 1)):
            share = tolerance_share([l[2] for l in links], snrs, s)
            print(f"{cid} given: share {share:.4f}")
            assert share <= 0.05, (cid, share)


def test_kernel_source_has_a_flat_grid_and_shares_the_header():
    csrc = os.path.join(ROOT, "deepmimo_amd", "csrc")
    src = open(os.path.join(csrc, "k8_cell_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "gridDim" not in code and "__syncthreads" not in code and "atomic" not in code and "asm" not in code
    assert '#include "k7_rate_body.h"' in code and '#include "dmx_common.h"' in code
    assert "rows_pair<M>" in code and "epilogue_logdet<M>" in code and "wave_lds_fence" in code
    assert "launch_dyn_lds" in code and "lds_waves_per_block" in code
    k7 = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "k7_rate.hip")).read())
    body = open(os.path.join(csrc, "k7_rate_body.h")).read()
    assert '#include "k7_rate_body.h"' in k7
    for fn in ("void rows_pair(", "float epilogue_logdet(", "void fill_array_table(", "void fill_w_chunk(", "void copy_rows_to_lds(",
               "int kept_paths(", "int gram_slices_log2("):                                # defined once, in the shared header
        assert body.count(fn) == 1 and fn not in k7 and fn not in code, fn
    for call in ("fill_w_chunk(", "kept_paths(", "gram_slices_log2("):
        assert call in k7 and call in code, call
    assert code.count("fill_array_table(") == 2 and "fill_array_table(" not in k7         # k7 keeps its own two table loops
    assert "sincos_rev" in body and "sincos_rev" not in code and "frac_rev" not in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "k8_cell_rate.hip" in mk and "k7_rate_body.h" in mk
