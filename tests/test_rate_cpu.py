"""Host side of the per-user achievable rate (dmx_rate_supported / dmx_channel_rate, k7_rate.hip) - no GPU: the symbols, the
shape query against a restatement of the launcher's LDS rule, the errors that must come before any GPU call, the pinned
reference of the GPU tests (hand cases and the determinant identity, float64 NumPy) and the condition on the GPU tests'
inputs (the derived tolerance must stay below 1 % of the rate on all but 5 % of a case's entries)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._rate_ref import median_snr, rate_from_channel, rate_tolerance, tolerance_share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepmimo_amd", "lib", "libdeepmimo_amd.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

LDS_MAX = 156 * 1024
SYMBOLS = ("dmx_rate_supported", "dmx_channel_rate")


def _params(bs=(8, 1), ue=(1, 1), K=1, num_paths=25, freq_domain=1, rx_filter=0, flags=0):
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = num_paths, freq_domain, 512, K, 10e6
    p.rx_filter, p.flags = rx_filter, flags
    sel = (C.c_int32 * max(K, 1))()
    p._keep = sel
    p.selected_subcarriers = C.addressof(sel)
    return p


def rate_lds_rule(bs, ue, K, P):
    """Waves per workgroup of the launcher, restated (0: not taken): one wave holds both array tables and a chunk of
    kc = min(K, 64) subcarriers of w, (m + M_big + kc) * P * 8 bytes with m = min(M_rx, M_tx) <= 8; 4 / 2 / 1 waves per
    workgroup while 4 x / 2 x fit 64 KB / one fits 156 KB."""
    m_tx, m_rx = bs[0] * bs[1], ue[0] * ue[1]
    m, big = min(m_tx, m_rx), max(m_tx, m_rx)
    if not (1 <= P <= 32) or K < 1 or m > 8:
        return 0
    b = (m + big + min(K, 64)) * P * 8
    return 4 if 4 * b <= 65536 else 2 if 2 * b <= 65536 else 1 if b <= LDS_MAX else 0


def test_header_and_binding_name_the_new_entry_points():
    from deepmimo_amd import _native as n
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, hdr) and sym in n.EXPORTED_SYMBOLS
    flat = re.sub(r"[ \t]+", " ", hdr)
    assert n.ABI_VERSION == 3 and "#define DMX_ABI_VERSION 3" in flat
    assert "(m + M_big + kc) * P * 8" in hdr and "159744" in hdr             # the header states the LDS formula


@needs_lib
def test_library_exports_the_symbols_with_abi_3():
    from deepmimo_amd import _native as n
    lib = n.load()
    assert lib.dmx_version() == 3
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None


@needs_lib
def test_supported_shapes_without_a_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    q = lambda p, L=25: lib.dmx_rate_supported(C.byref(p), L)                 # noqa: E731
    assert q(_params()) == 1                                                  # DeepMIMO's defaults
    assert q(_params(K=512)) == 1
    assert q(_params((64, 4), (2, 2), 512)) == 1                              # the headline panel, 25 paths
    assert q(_params((2, 1), (4, 4), 5)) == 1                                 # the Gram over the BS side
    assert q(_params((8, 4), (4, 2), 3)) == 1                                 # m = 8
    assert q(_params((8, 4), (3, 3), 3)) == 0 and "8 elements" in err()       # m = 9
    assert q(_params((3, 3), (8, 4), 3)) == 0 and "8 elements" in err()
    assert q(_params(num_paths=33), 40) == 0 and "32" in err()                # P = 33
    assert q(_params(num_paths=32), 40) == 1
    assert q(_params(num_paths=40), 32) == 1                                  # num_paths above the loaded count
    assert q(_params(freq_domain=0)) == 0 and "freq_domain" in err()
    assert q(_params(rx_filter=1)) == 0 and "rx_filter" in err()
    assert q(_params(K=0)) == 0 and q(_params(), 0) == 0 and q(_params(num_paths=0)) == 0
    assert q(_params(flags=n.FLAG_ADAPTIVE_TERMS)) == 1                       # either arithmetic mode
    assert q(_params(), -1) == -1
    assert lib.dmx_rate_supported(None, 25) == -1 and "params is NULL" in err()
    # the edge of the byte rule at 25 paths: m + M_big + kc <= 798
    assert q(_params((796, 1), (1, 1))) == 1 and q(_params((797, 1), (1, 1))) == 0
    assert "(1 + 797 + 1) * 25 * 8 = 159800 bytes" in err() and str(LDS_MAX) in err()
    assert q(_params((733, 1), (1, 1), 64)) == 1 and q(_params((734, 1), (1, 1), 64)) == 0
    assert q(_params((733, 1), (1, 1), 512)) == 1 and q(_params((734, 1), (1, 1), 512)) == 0
    assert q(_params((32, 32), (1, 1), 2)) == 0 and "LDS" in err()


@needs_lib
def test_supported_equals_the_lds_rule():
    from deepmimo_amd import _native as n
    lib = n.load()
    rng = np.random.default_rng(13)
    seen = {0: 0, 1: 0, 2: 0, 4: 0}
    for _ in range(4000):
        bs = (int(rng.integers(1, 65)), int(rng.integers(1, 17)))
        ue = (int(rng.integers(1, 6)), int(rng.integers(1, 4)))
        L, num_paths, K = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(1, 100))
        want = rate_lds_rule(bs, ue, K, min(L, num_paths))
        seen[want] += 1
        got = lib.dmx_rate_supported(C.byref(_params(bs, ue, K, num_paths)), L)
        assert got == (1 if want else 0), (bs, ue, K, num_paths, L, want, got)
    assert all(v > 50 for v in seen.values()), seen
    # the shapes the GPU tests rely on
    assert rate_lds_rule((8, 1), (1, 1), 2, 25) == 4 and rate_lds_rule((16, 16), (2, 2), 64, 25) == 1
    assert rate_lds_rule((64, 4), (2, 2), 512, 25) == 1 and rate_lds_rule((8, 8), (2, 2), 74, 25) == 2


@needs_lib
def test_argument_errors_without_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    buf = (C.c_char * 65536)()
    base = (C.addressof(buf) + 255) // 256 * 256
    ws, out = C.c_void_p(base), C.c_void_p(base + 4096)

    def call(p, b=0, cnt=4, snr=100.0, o=out, ok=None, L=25):
        return lib.dmx_channel_rate(C.byref(p), ws, 4, L, b, cnt, snr, o, ok, None)
    assert call(_params(freq_domain=0)) == -1 and "freq_domain" in err()
    assert call(_params(rx_filter=1)) == -1 and "rx_filter" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(_params(), snr=bad) == -1 and "snr_linear" in err()
    assert call(_params(), b=2, cnt=4) == -1 and "user range" in err()
    assert call(_params(), o=None) == -1 and "NULL" in err()
    assert call(_params(), o=C.c_void_p(base + 4098)) == -1 and "4-byte aligned" in err()
    assert call(_params(), ok=C.c_void_p(base + 8194)) == -1 and "4-byte aligned" in err()
    assert call(_params((32, 32), (1, 1), 2)) == -2 and "LDS" in err()
    assert call(_params((8, 4), (3, 3), 2)) == -2 and "8 elements" in err()
    assert call(_params(num_paths=33), L=40) == -2 and "32" in err()
    assert call(_params(K=0)) == -2
    assert call(_params(), cnt=0) == 0                                        # nothing to do: success before any GPU call


def _dataset(n=5, L=25):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=2)
    return dm, dm.Dataset({k: v.copy() for k, v in rays.items()})


@needs_lib
def test_check_rate_call_and_dataset_errors_come_before_any_gpu_call(monkeypatch):
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd.engine import check_rate_call
    dm, ds = _dataset()

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    ok = dm.ChannelGenParameters().validate(5)
    assert check_rate_call(ok, 25, 20.0) == 100.0
    assert check_rate_call(ok, 25, 3) == 10.0 ** 0.3
    for bad in (float("nan"), float("inf"), -float("inf"), None, "20"):
        with pytest.raises(ValueError, match="snr_db"):
            check_rate_call(ok, 25, bad)
        with pytest.raises(ValueError, match="snr_db"):
            ds.compute_rate(dm.ChannelGenParameters(), snr_db=bad)
    with pytest.raises(ValueError, match="snr_db"):                           # missing
        ds.compute_rate(dm.ChannelGenParameters())
    with pytest.raises(TypeError):                                            # keyword-only
        ds.compute_rate(dm.ChannelGenParameters(), 20.0)
    p = dm.ChannelGenParameters()
    p.freq_domain = 0
    with pytest.raises(ValueError, match="freq_domain"):
        ds.compute_rate(p, snr_db=20.0)
    with pytest.raises(ValueError, match="freq_domain"):
        check_rate_call(p, 25, 20.0)
    p = dm.ChannelGenParameters()
    p.ofdm.rx_filter = 1
    with pytest.raises(ValueError, match="rx_filter"):
        ds.compute_rate(p, snr_db=20.0)
    with pytest.raises(ValueError, match="rx_filter"):
        check_rate_call(p, 25, 20.0)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape = np.array([32, 32])
    with pytest.raises(ValueError, match=r"LDS"):
        ds.compute_rate(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array([4, 4]), np.array([3, 3])
    with pytest.raises(ValueError, match=r"8 elements"):
        ds.compute_rate(p, snr_db=20.0)
    _, ds40 = _dataset(L=40)
    p = dm.ChannelGenParameters()
    p.num_paths = 33
    with pytest.raises(ValueError, match=r"1\.\.32 paths"):
        ds40.compute_rate(p, snr_db=20.0)


@needs_lib
def test_valid_call_without_a_gpu_raises_the_usual_error(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    dm, ds = _dataset()
    with pytest.raises(RuntimeError, match="no GPU"):
        ds.compute_rate(dm.ChannelGenParameters(), snr_db=20.0)
    assert "compute_rate" in dm.MacroDataset.PROPAGATE_METHODS


def test_reference_single_path_single_antenna_ue():
    """one path, 1 x 1 UE: |H[t, k]|^2 = |c|^2 / N on every BS element, so rate = log2(1 + snr |c|^2 / N)"""
    m_tx, K, N, snr = 8, 5, 512, 3.0e9
    c = np.array([0.3e-3 - 0.4e-3j, 0.0, 2e-4j])                             # per user; the second has no path
    t, k = np.arange(m_tx)[:, None], np.arange(K)[None, :]
    steer = np.exp(2j * np.pi * (0.21 * t - 0.013 * k))
    H = (c[:, None, None, None] / np.sqrt(N)) * steer[None, None]
    rate, rate_k = rate_from_channel(H, snr)
    want = np.log2(1 + snr * np.abs(c) ** 2 / N)
    np.testing.assert_allclose(rate, want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(rate_k, np.repeat(want[:, None], K, axis=1), rtol=1e-12, atol=1e-15)
    assert rate[1] == 0 and (rate_k[1] == 0).all()


def test_reference_two_orthogonal_rank_one_paths():
    """H = sum_p c_p u_p v_p^H with orthonormal u (UE side) and orthogonal v (BS side, |v_p|^2 = M_tx): the eigenvalues of
    H H^H are |c_p|^2 M_tx, so rate = sum_p log2(1 + snr |c_p|^2)"""
    m_rx, m_tx, snr = 2, 4, 50.0
    u = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    v = np.array([[1, 1, 1, 1], [1, -1, 1, -1]], dtype=np.complex128) * np.exp(0.7j)
    c = np.array([0.8 + 0.1j, -0.05 + 0.3j])
    H = sum(c[p] * np.outer(u[:, p], v[p].conj()) for p in range(2))[None, :, :, None]
    rate, _ = rate_from_channel(H, snr)
    np.testing.assert_allclose(rate[0], np.log2(1 + snr * np.abs(c) ** 2).sum(), rtol=1e-12)


def test_reference_determinant_identity_when_the_arrays_swap_roles():
    """det(I + s H H^H) = det(I + s H^H H): the channel with the arrays exchanged, at the SNR that keeps s, has the same rate
    although the Gram is then formed from the other side's index"""
    rng = np.random.default_rng(5)
    for m_rx, m_tx in ((2, 8), (4, 4), (1, 5), (3, 2)):
        H = (rng.normal(size=(6, m_rx, m_tx, 7)) + 1j * rng.normal(size=(6, m_rx, m_tx, 7))) * 10 ** rng.uniform(-3, 1, (6, 1, 1, 1))
        snr = 37.0
        a, ak = rate_from_channel(H, snr)
        b, bk = rate_from_channel(np.conj(np.swapaxes(H, 1, 2)), snr * m_rx / m_tx)
        np.testing.assert_allclose(a, b, rtol=1e-10)
        np.testing.assert_allclose(ak, bk, rtol=1e-10)
        tol, tol_k = rate_tolerance(H, snr)
        assert (tol > 0).all() and (tol_k > 0).all() and tol.shape == (6,) and tol_k.shape == (6, 7)


@needs_lib
def test_tolerance_share_condition_of_every_gpu_case():
    """The tolerance may exceed 1 % of max(1, rate_ref) on at most 5 % of a case's live (user, k) entries, otherwise the GPU
    test would hide failures.  The inputs are the GPU tests' own (tests/test_gpu_rate.py), from the NumPy oracle."""
    from tests import test_gpu_rate as g
    for c in g.CASES:
        _, _, H, snr = g.case_inputs(c)
        share = tolerance_share(H, snr)
        print(f"{c['id']}: snr {10 * np.log10(snr):.1f} dB, share of entries with tol > 1 % = {share:.4f}")
        assert share <= 0.05, (c["id"], share)
        assert snr == median_snr(H)


def test_kernel_source_has_a_flat_grid_and_shares_the_headers():
    src = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k7_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "gridDim" not in code and "__syncthreads" not in code and "atomic" not in code and "asm" not in code
    assert '#include "k2_small_body.h"' in code and '#include "dmx_common.h"' in code
    assert "wave_lds_fence" in code and "sincos_rev" in code and "launch_dyn_lds" in code and "lds_waves_per_block" in code
    # the w chunk and the kept-path count are the shared header's; the two array tables stay here (sincos_rev above)
    body = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k7_rate_body.h")).read()
    assert '#include "k7_rate_body.h"' in code and code.count("fill_w_chunk(") == 1 and code.count("kept_paths(") == 1
    assert "void fill_w_chunk(" in body and "int kept_paths(" in body and code.count("sincos_rev") == 2 and "rint(" not in code
    assert "k7_rate.hip" in open(os.path.join(ROOT, "deepmimo_amd", "csrc", "Makefile")).read()
