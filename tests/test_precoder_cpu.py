"""Host side of the eigenbeam precoders and combiners (dmx_precoder_supported / dmx_channel_precoders, the third epilogue of
k7_rate.hip) - no GPU: the symbols, the shape query against the rate's plus the n_layers range, the errors that must come
before any GPU call, the pinned reference of the GPU tests (hand cases, float64 NumPy), the float32 model of the kernel's
Jacobi iteration with the accumulated basis and the 2^-50 gate, and the conditions on the GPU tests' inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _precoder_ref as pr
from tests import _spectrum_ref as sr
from tests._rate_ref import _gram
from tests.test_rate_cpu import LIB, ROOT, _dataset, _params

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")
SYMBOLS = ("dmx_precoder_supported", "dmx_channel_precoders")


def test_header_and_binding_name_the_new_entry_points():
    from deepmimo_amd import _native as n
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, hdr) and sym in n.EXPORTED_SYMBOLS
    assert n.ABI_VERSION == 3 and "#define DMX_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    # the header states the gauge, the presence floor, the gate and the accuracy
    for words in ("real and positive", "c_J * 2^-24 * sum_j gamma_j, 1e-30", "|G_pq| >= 2^-50", "69 * 2^-24", "7.5 * 2^-24 |G|_F",
                  "-45 dB", "-38 dB"):
        assert words in hdr, words


@needs_lib
def test_library_exports_the_symbols_with_abi_3():
    from deepmimo_amd import _native as n
    lib = n.load()
    assert lib.dmx_version() == 3
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None


@needs_lib
def test_supported_equals_the_rate_query_and_the_layer_range():
    from deepmimo_amd import _native as n
    lib = n.load()
    rng = np.random.default_rng(15)
    seen = {0: 0, 1: 0}
    for _ in range(3000):
        bs = (int(rng.integers(1, 65)), int(rng.integers(1, 17)))
        ue = (int(rng.integers(1, 6)), int(rng.integers(1, 4)))
        L, num_paths, K = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(1, 100))
        p = _params(bs, ue, K, num_paths)
        want = lib.dmx_rate_supported(C.byref(p), L)
        m = min(bs[0] * bs[1], ue[0] * ue[1])
        for layers in (1, m):
            assert lib.dmx_precoder_supported(C.byref(p), L, layers) == want, (bs, ue, K, num_paths, L, layers)
        for layers in (0, -1, m + 1, 2 ** 31 - 1, -2 ** 31):
            assert lib.dmx_precoder_supported(C.byref(p), L, layers) == 0, (bs, ue, K, num_paths, L, layers)
        seen[want] += 1
    assert all(v > 200 for v in seen.values()), seen
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    q = lambda p, layers=1, L=25: lib.dmx_precoder_supported(C.byref(p), L, layers)   # noqa: E731
    assert q(_params()) == 1 and q(_params((64, 4), (2, 2), 512), 4) == 1 and q(_params((2, 1), (4, 4), 5), 2) == 1
    assert q(_params((8, 4), (4, 2), 3), 8) == 1 and q(_params((8, 4), (4, 2), 3), 9) == 0 and "n_layers = 9" in err() and "1..8" in err()
    assert q(_params(), 2) == 0 and "n_layers = 2" in err() and q(_params(), 0) == 0 and "n_layers = 0" in err()
    assert q(_params((8, 4), (3, 3), 3)) == 0 and "8 elements" in err()
    assert q(_params(num_paths=33), L=40) == 0 and "32" in err()
    assert q(_params(freq_domain=0)) == 0 and "freq_domain" in err()
    assert q(_params(rx_filter=1)) == 0 and "rx_filter" in err()
    assert q(_params((796, 1), (1, 1))) == 1 and q(_params((797, 1), (1, 1))) == 0 and "LDS" in err()
    assert q(_params(), L=-1) == -1 and lib.dmx_precoder_supported(None, 25, 1) == -1 and "params is NULL" in err()


@needs_lib
def test_argument_errors_without_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    buf = (C.c_char * 65536)()
    base = (C.addressof(buf) + 255) // 256 * 256
    ws, out = C.c_void_p(base), C.c_void_p(base + 4096)

    def call(p, b=0, cnt=4, snr=100.0, layers=1, og=out, ot=None, orx=None, L=25):
        return lib.dmx_channel_precoders(C.byref(p), ws, 4, L, b, cnt, snr, layers, og, ot, orx, None)
    assert call(_params(), og=None) == -1 and "all NULL" in err()
    assert call(_params(freq_domain=0)) == -1 and "freq_domain" in err()
    assert call(_params(rx_filter=1)) == -1 and "rx_filter" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e71, 1e-71):
        assert call(_params(), snr=bad) == -1 and "snr_linear" in err()
    assert call(_params(), b=2, cnt=4) == -1 and "user range" in err()
    assert call(_params(), og=C.c_void_p(base + 8194)) == -1 and "aligned" in err()
    for which in ("ot", "orx"):
        assert call(_params(), **{which: C.c_void_p(base + 8196)}) == -1 and "8-byte aligned" in err()
    for layers in (0, 2, -1):
        assert call(_params(), layers=layers) == -2 and "n_layers" in err()
    assert call(_params((4, 2), (2, 1)), layers=3) == -2 and "1..2" in err()
    assert call(_params((32, 32), (1, 1), 2)) == -2 and "LDS" in err()
    assert call(_params((8, 4), (3, 3), 2)) == -2 and "8 elements" in err()
    assert call(_params(num_paths=33), L=40) == -2 and "32" in err()
    assert call(_params(), cnt=0) == 0 and call(_params(), cnt=0, og=None) == 0   # nothing to do: success before any GPU call
    assert call(_params(), cnt=0, layers=2) == -2                             # but the shape is still checked


@needs_lib
def test_dataset_errors_come_before_any_gpu_call(monkeypatch):
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd.engine import check_precoder_call
    dm, ds = _dataset()

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    ok = dm.ChannelGenParameters().validate(5)
    assert check_precoder_call(ok, 25, 20.0, 1) == 100.0
    for bad in (float("nan"), float("inf"), -float("inf"), None, "20"):
        with pytest.raises(ValueError, match="snr_db"):
            ds.compute_precoders(dm.ChannelGenParameters(), snr_db=bad)
    with pytest.raises(ValueError, match="snr_db"):                           # missing
        ds.compute_precoders(dm.ChannelGenParameters())
    with pytest.raises(TypeError):                                            # keyword-only
        ds.compute_precoders(dm.ChannelGenParameters(), 20.0)
    for bad in (0, 2, -1, 1.0, "1", None, True, 2 ** 40):                     # the defaults have a 1 x 1 UE: m = 1
        with pytest.raises(ValueError, match="n_layers"):
            ds.compute_precoders(dm.ChannelGenParameters(), snr_db=20.0, n_layers=bad)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 1])
    with pytest.raises(ValueError, match=r"n_layers = 3.*1\.\.2"):
        ds.compute_precoders(p, snr_db=20.0, n_layers=3)
    p = dm.ChannelGenParameters()
    p.freq_domain = 0
    with pytest.raises(ValueError, match="freq_domain"):
        ds.compute_precoders(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.ofdm.rx_filter = 1
    with pytest.raises(ValueError, match="rx_filter"):
        ds.compute_precoders(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape = np.array([32, 32])
    with pytest.raises(ValueError, match=r"LDS"):
        ds.compute_precoders(p, snr_db=20.0)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array([4, 4]), np.array([3, 3])    # m = 9
    with pytest.raises(ValueError, match=r"8 elements"):
        ds.compute_precoders(p, snr_db=20.0)
    _, ds40 = _dataset(L=40)
    p = dm.ChannelGenParameters()
    p.num_paths = 33
    with pytest.raises(ValueError, match=r"1\.\.32 paths"):
        ds40.compute_precoders(p, snr_db=20.0)
    assert "compute_precoders" in dm.MacroDataset.PROPAGATE_METHODS


@needs_lib
def test_valid_call_without_a_gpu_raises_the_usual_error(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    dm, ds = _dataset()
    with pytest.raises(RuntimeError, match="no GPU"):
        ds.compute_precoders(dm.ChannelGenParameters(), snr_db=20.0)


# ---- the reference, by hand ---------------------------------------------------------------------------------------------

def _as_outputs(H, snr, L=None):
    """the definition cast to the kernel's output types"""
    gamma, w_tx, w_rx = pr.precoders_from_channel(H, snr)
    L = gamma.shape[-1] if L is None else L
    return gamma.astype(np.float32), w_tx[:, :, :L].astype(np.complex64), w_rx[:, :, :L].astype(np.complex64)


def test_reference_one_path():
    """H = c a_rx a_tx^T: one mode, sigma = |c| |a_rx| |a_tx|, u = a_rx / |a_rx| with its first largest component turned
    real, v = conj(a_tx) / |a_tx| times the phase that makes u^H H v = sigma"""
    m_rx, m_tx, snr = 2, 8, 4.0e9
    c = 0.3e-3 - 0.4e-3j
    a_rx = np.exp(2j * np.pi * (0.1 + 0.31 * np.arange(m_rx)))
    a_tx = np.exp(2j * np.pi * (0.7 - 0.12 * np.arange(m_tx)))
    H = (c * np.outer(a_rx, a_tx))[None, :, :, None]
    gamma, w_tx, w_rx = pr.precoders_from_channel(H, snr)
    sigma = abs(c) * np.sqrt(m_rx * m_tx)
    np.testing.assert_allclose(gamma[0, 0], [snr * sigma ** 2, 0.0], rtol=1e-12, atol=1e-9)
    ph = np.exp(-2j * np.pi * 0.1)                                            # turns a_rx[0], the first of equal moduli
    np.testing.assert_allclose(w_rx[0, 0, 0], a_rx * ph / np.sqrt(m_rx), atol=1e-12)
    np.testing.assert_allclose(w_tx[0, 0, 0], np.conj(a_tx) / np.sqrt(m_tx) * np.conj(c) / abs(c) * ph, atol=1e-12)
    assert w_rx[0, 0, 0, 0].imag == 0 and not np.signbit(w_rx[0, 0, 0, 0].imag)
    np.testing.assert_allclose(np.conj(w_rx[0, 0, 0]) @ H[0, :, :, 0] @ w_tx[0, 0, 0], sigma, rtol=1e-12)
    ga, wt, wr = _as_outputs(H, snr)
    present, border = pr.presence(ga)
    assert present[0, 0].tolist() == [True, False] and not border.any()


def test_reference_two_orthogonal_paths():
    """H = sum_p c_p u_p v_p^H with orthonormal u (UE side, 4 elements) and orthogonal v (BS side): layer p is (u_p, v_p / |v_p|)
    up to the gauge, gamma = snr M_tx |c_p|^2, two zero modes"""
    m_tx, snr = 4, 50.0
    u = np.array([[1, 1, 1, 1], [1, -1, 1, -1]]).T / 2.0
    v = np.array([[1, 1, 1, 1], [1, 1, -1, -1]], dtype=np.complex128) * np.exp(0.7j)
    c = np.array([0.8 + 0.1j, -0.05 + 0.3j])
    H = sum(c[p] * np.outer(u[:, p], v[p].conj()) for p in range(2))[None, :, :, None]
    gamma, w_tx, w_rx = pr.precoders_from_channel(H, snr)
    np.testing.assert_allclose(gamma[0, 0], [snr * m_tx * abs(c[0]) ** 2, snr * m_tx * abs(c[1]) ** 2, 0, 0], rtol=1e-12, atol=1e-12)
    for p in range(2):
        np.testing.assert_allclose(w_rx[0, 0, p], u[:, p], atol=1e-12)       # real, first component positive: in the gauge
        np.testing.assert_allclose(w_tx[0, 0, p], v[p] / 2.0 * np.conj(c[p]) / abs(c[p]), atol=1e-12)
        s = np.conj(w_rx[0, 0, p]) @ H[0, :, :, 0] @ w_tx[0, 0, p]
        np.testing.assert_allclose(s, np.sqrt(gamma[0, 0, p] / snr), rtol=1e-12)


def test_reference_bs_smaller_than_ue_and_the_checker():
    """M_tx < M_rx: the gauge sits on v; the definition passes its own criteria in both orientations, and a conjugated
    small-side vector (the mistake a kernel whose Gram is the conjugate of H^H H can make) does not"""
    rng = np.random.default_rng(8)
    for m_rx, m_tx in ((4, 2), (2, 4), (8, 3), (1, 5), (5, 1), (3, 3)):
        H = (rng.normal(size=(5, m_rx, m_tx, 3)) + 1j * rng.normal(size=(5, m_rx, m_tx, 3))) * 10 ** rng.uniform(-6, -4, (5, 1, 1, 1))
        H[3] = 0
        snr = 1e11
        gamma, w_tx, w_rx = pr.precoders_from_channel(H, snr)
        small = w_rx if m_rx <= m_tx else w_tx
        piv = np.take_along_axis(small, np.abs(small).argmax(axis=-1)[..., None], axis=-1)
        assert (piv.imag == 0)[[0, 1, 2, 4]].all() and (piv.real > 0)[[0, 1, 2, 4]].all()
        Hk = np.moveaxis(H, 3, 1)
        np.testing.assert_allclose(np.einsum("nkrt,nklt->nklr", Hk, w_tx), np.sqrt(gamma / snr)[..., None] * w_rx, atol=1e-12 * np.abs(H).max())
        ga, wt, wr = _as_outputs(H, snr)
        wt[3], wr[3] = 0, 0                                                  # what the kernel writes for a user without a path
        res = pr.check_vectors(ga, wt, wr, H, snr)
        assert res["borderline"] == 0 and all(res[k] <= 1.0 for k in ("C1", "C2", "C3", "C4", "C5", "gauge", "zeros")), res
        if min(m_rx, m_tx) > 1:
            bad = pr.check_vectors(ga, np.conj(wt), wr, H, snr) if m_tx < m_rx else pr.check_vectors(ga, wt, np.conj(wr), H, snr)
            assert bad["C2"] > 1.0 and bad["C1"] > 1.0, bad
        only_small = pr.check_vectors(ga, wt if m_tx < m_rx else None, None if m_tx < m_rx else wr, H, snr)
        assert "C1" not in only_small and "C4" not in only_small and only_small["C2"] <= 1.0


# ---- the float32 model of the kernel's iteration -------------------------------------------------------------------------

def _case_grams():
    """m -> the float32-scale Grams (mode SNRs) of every GPU case with that m"""
    from tests import test_gpu_spectrum as gs
    by = {}
    for c in gs.CASES:
        _, _, H, _ = gs.g.case_inputs(c)
        G = _gram(H) * gs.case_snr(H)
        by.setdefault(G.shape[-1], []).append(G.reshape(-1, G.shape[-1], G.shape[-1]))
    return by


def test_model_one_element_and_exact_inputs():
    d, X, norm = pr.jacobi_vec_f32(np.array([[[5.0]]]), sr.SWEEPS[1])
    assert d.tolist() == [[5.0]] and X.tolist() == [[[1.0]]]
    d, X, _ = pr.jacobi_vec_f32(np.diag([1.0, 7.0, 3.0])[None], sr.SWEEPS[3])            # diagonal: only the sort acts
    assert d.tolist() == [[7.0, 3.0, 1.0]] and np.array_equal(X[0], np.eye(3)[:, [1, 2, 0]])
    tiny = np.array([[[2.0, 1e-16 + 1e-16j], [1e-16 - 1e-16j, 1.0]]])                     # below the gate: skipped, X stays I
    d, X, _ = pr.jacobi_vec_f32(tiny, sr.SWEEPS[2])
    assert d.tolist() == [[2.0, 1.0]] and np.array_equal(X[0], np.eye(2))
    d, X, _ = pr.jacobi_vec_f32(tiny, sr.SWEEPS[2], gate=False)
    assert not np.array_equal(X[0], np.eye(2))


@needs_lib
def test_model_orthogonality_and_residual_with_the_gate():
    """For m = 2 .. 8 on the hard set, the repeated-eigenvalue set and the Grams of every GPU case: the columns of X are
    orthonormal to C3's bound and each satisfies C2 with the Jacobi term alone; the eigenvalues stay within the bound of
    tests/test_spectrum_cpu.py.  With the gate removed C3 fails on the hard set for every m >= 3: the gate is not padding."""
    by = _case_grams()
    assert set(range(1, 9)) <= set(by)                                       # every order the kernel is instantiated for
    for m in range(2, 9):
        cj = sr.c_jacobi(m)
        worst = {}
        for name, G in (("hard", sr.hard_grams(m)), ("repeated", sr.repeated_grams(m)), ("cases", np.concatenate(by[m]) if m in by else None)):
            if G is None:
                continue
            G = G[np.abs(G).reshape(len(G), -1).max(axis=1) > 0]             # users without a path have no matrix
            orth, res = pr.model_quality(G, m)
            d, X, norm = pr.jacobi_vec_f32(G, sr.SWEEPS[m])
            gram = np.conj(np.swapaxes(X, 1, 2)) @ X - np.eye(m)
            c3 = float(np.abs(gram).max() / (2 * cj * sr.U24))
            c2 = float((res / ((3 * cj + 64) * sr.U24 * (1 + cj * sr.U24))).max())
            lam = np.maximum(np.linalg.eigvalsh(G)[:, ::-1], 0.0)
            ev = float((np.abs(d - lam) / ((cj + 4) * sr.U24 * norm)[:, None]).max())
            worst[name] = (c2, c3, ev, float(orth.max() / sr.U24), float(res.max() / sr.U24))
            assert c2 <= 1.0 and c3 <= 1.0 and ev <= 1.0, (m, name, worst[name])
        print(f"m = {m}: (C2 ratio, C3 ratio, eigenvalue ratio, |X^H X - I|_F / 2^-24, residual / (2^-24 |G|_F)) = {worst}")
        # the accuracy statement of the header
        assert max(w[3] for w in worst.values()) <= 69.0 * (1 + 1e-6) and max(w[4] for w in worst.values()) <= 7.5
        if m >= 3:
            _, X, _ = pr.jacobi_vec_f32(sr.hard_grams(m), sr.SWEEPS[m], gate=False)
            gram = np.conj(np.swapaxes(X, 1, 2)) @ X - np.eye(m)
            bad = np.abs(gram).reshape(len(X), -1).max(axis=1) > 2 * cj * sr.U24
            print(f"m = {m}: without the gate C3 fails on {int(bad.sum())} of {len(X)} hard inputs, worst |X^H X - I|_F = "
                  f"{float(np.linalg.norm(gram, axis=(1, 2)).max()):.3g}")
            assert bad.any()
    orth, _ = pr.model_quality(sr.hard_grams(2), 2)
    assert orth.max() <= 7.0 * sr.U24 * (1 + 1e-6)


@needs_lib
def test_model_outputs_pass_the_gpu_criteria_in_both_orientations():
    """The model run end to end on two GPU cases - float32 Gram, iteration, gauge, larger-side vector as B x / sqrt(gamma)
    - passes every criterion the GPU test applies; where the BS array is the smaller one the kernel's Gram is the
    conjugate of snr H^H H and the precoder the conjugate of the column."""
    from tests import test_gpu_spectrum as gs
    by = {c["id"]: c for c in gs.CASES}
    for cid in ("irregular", "ue_larger", "L2_m4"):
        _, _, H, _ = gs.g.case_inputs(by[cid])
        snr = gs.case_snr(H)
        n, m_rx, m_tx, K = H.shape
        m, rx_small = min(m_rx, m_tx), m_rx <= m_tx
        G = _gram(H) * snr
        Gk = G if rx_small else np.conj(G)                                   # the Gram of the rows h_i the kernel forms
        d, X, _ = pr.jacobi_vec_f32(Gk.reshape(-1, m, m), sr.SWEEPS[m])
        gamma = d.reshape(n, K, m).astype(np.float32)
        x = np.swapaxes(X, 1, 2).reshape(n, K, m, m)                         # [.., layer, component]
        x = x if rx_small else np.conj(x)
        Hk = np.moveaxis(H.astype(np.complex128), 3, 1)
        B = np.conj(np.swapaxes(Hk, -1, -2)) if rx_small else Hk
        present, _ = pr.presence(gamma)
        x = np.where(present[..., None], x, 0.0)
        w_small = x.astype(np.complex64)
        w_tx, w_rx = pr.apply_gauge(w_small if not rx_small else np.ones_like(w_small), w_small if rx_small else np.ones_like(w_small), rx_small)
        w_small = (w_rx if rx_small else w_tx).astype(np.complex64)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.sqrt(snr) * np.einsum("nkam,nklm->nkla", B, w_small.astype(np.complex128)) / np.sqrt(gamma.astype(np.float64))[..., None]
        w_big = np.where(present[..., None], y, 0.0).astype(np.complex64)
        res = pr.check_vectors(gamma, w_big if rx_small else w_small, w_small if rx_small else w_big, H, snr)
        print(cid, res)
        assert res["borderline"] == 0 and all(res[k] <= 1.0 for k in ("C1", "C2", "C3", "C4", "C5", "gauge", "zeros")), (cid, res)


# ---- the conditions on the GPU tests' inputs -------------------------------------------------------------------------------

@needs_lib
def test_conditions_of_every_gpu_case():
    """From the reference alone, per case of tests/test_gpu_precoders.py: layer 0 is present on every live entry with
    tol_v <= 1 % of gamma_0; C5's gap condition holds on >= 95 % of the live entries where m >= 2; among the entries whose
    layer 1 is present, tol_g exceeds 10 % of gamma_1 on <= 25 %.  Higher layers are held to C1, C3 and C4, which need no
    such condition; their shares are printed."""
    from tests import test_gpu_spectrum as gs
    assert len(gs.CASES) == len(gs.g.CASES) + 6
    assert {"L1_m4", "L2_m4", "L1_m3", "L2_m3", "L1_m5", "L2_m5"} <= {c["id"] for c in gs.CASES}
    worst0 = 0.0
    for c in gs.CASES:
        _, _, H, _ = gs.g.case_inputs(c)
        snr = gs.case_snr(H)
        m = min(H.shape[1], H.shape[2])
        live = np.abs(H).reshape(H.shape[0], -1).max(axis=1) > 0
        gamma = sr.eigenmodes_from_channel(H, snr)
        present, border = pr.presence(gamma.astype(np.float32))
        tol_v, tol_g = pr.vector_tolerance(H, snr), sr.mode_tolerance(H, snr)
        assert present[live][..., 0].all() and not present[~live].any(), c["id"]
        r0 = float((tol_v[live] / gamma[live][..., 0]).max())
        worst0 = max(worst0, r0)
        assert r0 <= 1e-2, (c["id"], r0)
        line = f"{c['id']}: m {m}, tol_v / gamma_0 worst {r0:.2e}"
        if m >= 2:
            gap = (gamma[..., 0] - gamma[..., 1] > 10 * tol_v)[live]
            p1 = present[..., 1] & live[:, None]
            weak = float((tol_g[p1] / gamma[..., 1][p1] > 0.1).mean()) if p1.any() else 0.0
            line += f", gap condition on {gap.mean():.4f}, layer 1 present on {p1[live].mean():.3f} with tol_g > 10 % on {weak:.3f} of them"
            assert gap.mean() >= 0.95, (c["id"], float(gap.mean()))
            assert weak <= 0.25, (c["id"], weak)
            for i in range(2, m):
                pi = present[..., i] & live[:, None]
                share = float((tol_g[pi] / gamma[..., i][pi] > 0.1).mean()) if pi.any() else 0.0
                line += f"; layer {i}: present {pi[live].mean():.3f}, weak {share:.3f}"
        print(line + f"; borderline {int(border.sum())}")
    print(f"worst tol_v / gamma_0 over the cases: {worst0:.2e}")


def test_kernel_source_keeps_one_body_and_the_sweep_table():
    src = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k7_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    table = re.findall(r"SWEEPS\[9\] = \{([0-9, ]+)\}", code)
    assert len(table) == 1 and [int(x) for x in table[0].split(",")][1:] == [sr.SWEEPS[m] for m in range(1, 9)]
    assert code.count("__global__") == 1                                      # one kernel body, templated on its epilogue
    assert "gridDim" not in code and "__syncthreads" not in code and "atomic" not in code and "asm" not in code
    assert "EPI_VECTORS" in code and "0x1p-50f" in code                       # the third epilogue and its gate
