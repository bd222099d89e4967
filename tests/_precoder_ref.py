"""References of the precoder tests (tests/test_precoder_cpu.py, tests/test_gpu_precoders.py): the definition of the eigenbeam
precoders and combiners from np.linalg.svd of a channel tensor in complex128, a float32 model of the kernel's Jacobi
iteration with the accumulated basis, and the criteria the GPU tests hold the kernel to.  A plain module: NumPy only, no
torch, no GPU.

    H_k = H[u, :, :, k] = U S V^H (M_rx x M_tx, strongest modes first),  m = min(M_rx, M_tx),  L = n_layers in 1..m
    gamma[u, k, i]   = snr s_i^2                      float32   [n, K, m]        (as tests/_spectrum_ref.py)
    w_tx[u, k, i, :] = v_i  (precoder, unit norm)     complex64 [n, K, L, M_tx]
    w_rx[u, k, i, :] = u_i  (combiner, unit norm)     complex64 [n, K, L, M_rx]
    H_k v_i = s_i u_i,   H_k^H u_i = s_i v_i,   s_i = sqrt(gamma_i / snr)
Gauge: the component of largest modulus (first on ties) of the smaller-side vector of a pair (u_i if M_rx <= M_tx, else
v_i) is real and positive, its imaginary part exactly +0; the other vector follows from the relation.
Presence: layer i of an entry is present iff  gamma_i > max(c_J 2^-24 sum_j gamma_j, 1e-30)  in float32 (one constant per m
times the sum of the sorted gamma in index order), c_J of tests/_spectrum_ref.py; an absent layer is +0.0 in both vectors.

Model (jacobi_vec_f32): tests/_spectrum_ref.jacobi_f32 operation by operation, with two changes.  A pair is rotated only
where |G_pq| >= 2^-50 (else t = 0, e = 1): below that the squares behind |G_pq| leave the normal float32 range and e loses
its unit modulus, which the eigenvalues do not feel but which rescales a column of X.  And X (the identity at the start)
takes on all m rows the column update of G:  x = X_kp,  y = X_kq conj(e),  X_kp = c x - s y,  X_kq = s x + c y.
The columns are then sorted with d (the kernel's odd-even network swaps on a strict comparison: a stable sort).

Notation of the criteria: e = sqrt(M_rx M_tx) TOL_REL max|H[u]| (the Frobenius norm of a channel error the project's channel
criterion admits), c_J and U24 = 2^-24 of tests/_spectrum_ref.py, G = snr Gram(H_k) over the smaller array,
B = H_k^H where the UE array is the smaller one, else B = H_k (so G = snr B^H B, B x_i = s_i y_i); x_i the smaller-side
vector of layer i, y_i the larger-side one, gamma the KERNEL'S OWN output.

    tol_v[u, k] = snr (2 |H_k|_F e + e^2) + (3 c_J + 64) 2^-24 |G|_F
        snr (2 |H_k|_F e + e^2)  the channel criterion's share: |dG|_2 of an admitted dH_k, as in tol_g
        c_J 2^-24 |G|_F          the rotations' rounding on G (each an exact unitary similarity plus <= 13 roundings of |G|_F)
        2 c_J 2^-24 |G|_F        the same roundings accumulated in X (|X^H X - I| <= c_J 2^-24 per side), times |G|_2 <= |G|_F
                                 in G X - X D, on both sides of the product
        64 * 2^-24 |G|_F         the off-diagonal norm that is left: <= 2^-24 |G|_F where the iteration converges and about
                                 40 * 2^-24 |G|_F where a non-zero eigenvalue is repeated three times or more (the sweep
                                 table's own note), rounded up to the next power of two
    C1  |sqrt(snr) B x_i - sqrt(gamma_i) y_i|_2 <= 2 sqrt(snr) e
        by construction: the kernel forms y_i as its own B x_i / sqrt(gamma_i); its B is within e of the reference's and
        |x_i| is 1 to rounding, so e alone would do in exact arithmetic; the factor 2 covers the float32 sums.
    C2  |snr B^H B x_i - gamma_i x_i|_2 <= tol_v (1 + c_J 2^-24)
        the eigen-residual, free of gaps: G X = X D + R with |R| bounded by the terms above, and |x_i| <= 1 + c_J 2^-24.
    C3  |x_i^H x_j - delta_ij| <= 2 c_J 2^-24 over the present layers of an entry
        X is a product of SWEEPS m (m - 1) / 2 rotations, each unitary to the roundings of c and s e; c_J counts 13 per
        rotation, of which a column of X sees fewer; the factor 2 is for the inner product of two columns.
    C4  | |y_i|^2 - 1 | <= 2 c_J 2^-24 + (3 c_J + 64) 2^-24 |gamma|_2 / gamma_i
        |y_i|^2 = x_i^H G' x_i / gamma_i with G' the kernel's own Gram (no channel term): |x_i|^2 to C3, and the residual
        of C2 without its first term, relative to gamma_i, with |G'|_F = |gamma|_2 to the same rounding.
    C5  where delta = gamma_0 - gamma_1^ref > 10 tol_v:  1 - |<x_0, x_0^ref>|^2 / |x_0|^2 <= (tol_v / delta)^2
        Davis-Kahan for the dominant vector: sin(angle) <= residual / gap.  The left side is the squared sine of the angle
        between x_0 and the reference, so x_0 is normalised in float64 first; its norm is C3's business.  Without that
        division the left side is (1 - |x_0|^2) + |x_0|^2 sin^2, and the first term - the rounding of a unit vector to
        float32 components, up to about m 2^-24 = 1e-7 and admitted by C3 up to 2 c_J 2^-24 - is set against a bound
        that goes down to 1.2e-8 on the committed cases (tol_v / delta >= 2 TOL_REL): the reference's own u_0 cast to
        complex64 then sits at 0.5 of the bound, the model's x_0 renormalised and rounded to float32 at 6.0, the
        model's x_0 as it is at 17 and the kernel's on an MI355X at 23 (adaptive_workspace), while the sine itself is at
        2e-6 of it; both figures are printed by the tests (C5 and C5_unnormalised).
gamma itself is held to the mode and trace criteria of tests/test_gpu_spectrum.check_spectrum (tol_g)."""
from __future__ import annotations

import numpy as np

from tests import _spectrum_ref as sr
from tests._cases import TOL_REL
from tests._rate_ref import _gram
from tests._spectrum_ref import SWEEPS, U24, _fma, c_jacobi

GATE = np.float32(2.0 ** -50)


# ---- the float64 definition -------------------------------------------------------------------------------------------

def small_is_rx(H):
    return H.shape[1] <= H.shape[2]


def apply_gauge(w_tx, w_rx, rx_small):
    """both vectors of every pair times conj(phase) of the largest-modulus component (first on ties) of the smaller-side one"""
    small = w_rx if rx_small else w_tx
    j = np.abs(small).argmax(axis=-1)[..., None]
    piv = np.take_along_axis(small, j, axis=-1)
    ph = np.where(np.abs(piv) > 0, np.conj(piv) / np.where(np.abs(piv) > 0, np.abs(piv), 1.0), 1.0)
    w_tx, w_rx = w_tx * ph, w_rx * ph
    np.put_along_axis(w_rx if rx_small else w_tx, j, np.abs(piv).astype(small.dtype), axis=-1)   # exactly (|x|, +0)
    return w_tx, w_rx


def precoders_from_channel(H, snr):
    """(gamma [n, K, m] float64, w_tx [n, K, m, M_tx], w_rx [n, K, m, M_rx] complex128) of the definition, all m layers, in
    the gauge, from np.linalg.svd; no presence floor (a zero mode has an arbitrary unit vector)"""
    Hk = np.moveaxis(np.asarray(H).astype(np.complex128), 3, 1)                          # [n, K, M_rx, M_tx]
    U, s, Vh = np.linalg.svd(Hk, full_matrices=False)
    w_tx, w_rx = apply_gauge(np.conj(Vh), np.swapaxes(U, -1, -2), small_is_rx(H))
    return float(snr) * s ** 2, w_tx, w_rx


# ---- presence -----------------------------------------------------------------------------------------------------------

def presence(gamma):
    """(present [.., m] bool, borderline [.., m] bool) of float32 mode SNRs gamma [.., m], by the floor formula in float32;
    borderline: within 1e-5 relative of the floor, where either answer is admitted"""
    g = np.asarray(gamma, dtype=np.float32)
    m = g.shape[-1]
    tot = np.zeros(g.shape[:-1], dtype=np.float32)
    for i in range(m):
        tot = (tot + g[..., i]).astype(np.float32)
    floor = np.maximum(np.float32(c_jacobi(m) * U24) * tot, np.float32(1e-30))[..., None]
    border = np.abs(g.astype(np.float64) - floor) <= 1e-5 * floor.astype(np.float64)
    return g > floor, border


# ---- the tolerances -----------------------------------------------------------------------------------------------------

def channel_error(H):
    """e [n] of the module docstring"""
    H = np.asarray(H)
    n = H.shape[0]
    peak = np.abs(H).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    return np.sqrt(H.shape[1] * H.shape[2]) * TOL_REL * peak


def vector_tolerance(H, snr):
    """tol_v [n, K] of the module docstring"""
    H = np.asarray(H).astype(np.complex128)
    m = min(H.shape[1], H.shape[2])
    e = channel_error(H)[:, None]
    h_f = np.sqrt((np.abs(H) ** 2).sum(axis=(1, 2)))
    g_f = np.linalg.norm(_gram(H), axis=(-2, -1))
    return float(snr) * (2 * h_f * e + e * e) + (3 * c_jacobi(m) + 64) * U24 * float(snr) * g_f


def _ratio(err, tol, mask):
    """worst err / tol over mask (0 / 0 = 0, x / 0 = inf)"""
    err, tol = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(tol, np.float64))
    if not mask.any():
        return 0.0
    e, t = err[mask], tol[mask]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e <= t, np.where(t > 0, e / np.where(t > 0, t, 1.0), 0.0), np.where(t > 0, e / np.where(t > 0, t, 1.0), np.inf))
    return float(r.max())


def check_vectors(gamma, w_tx, w_rx, H, snr, what=""):
    """The worst ratio error / tolerance per criterion, {"C1": .., "C2": .., "C3": .., "C4": .., "C5": .., "gauge": 0 or inf,
    "zeros": 0 or inf, "borderline": count}, of outputs gamma [n, K, m] float32, w_tx [n, K, L, M_tx], w_rx [n, K, L, M_rx]
    complex64 (NumPy; w_tx or w_rx may be None: the criteria that need it are left out) against the reference channel H.
    Every ratio must be <= 1 and borderline must be 0 on the committed cases; the caller asserts."""
    H = np.asarray(H)
    n, m_rx, m_tx, K = H.shape
    m, rx_small = min(m_rx, m_tx), small_is_rx(H)
    snr = float(snr)
    cj = c_jacobi(m)
    gamma = np.asarray(gamma)
    Hk = np.moveaxis(H.astype(np.complex128), 3, 1)                                      # [n, K, M_rx, M_tx]
    B = np.conj(np.swapaxes(Hk, -1, -2)) if rx_small else Hk                             # [n, K, M_big, m]
    xs, ys = (w_rx, w_tx) if rx_small else (w_tx, w_rx)
    L = (xs if xs is not None else ys).shape[2]
    pres_all, border = presence(gamma)
    pres = pres_all[..., :L]
    g64 = gamma.astype(np.float64)
    e = channel_error(H)[:, None, None]
    tol_v = vector_tolerance(H, snr)[..., None]                                          # [n, K, 1]
    out = {"borderline": int(border[..., :L].sum())}
    zeros = True
    for w in (xs, ys):
        if w is not None:
            v = np.ascontiguousarray(w).view(np.float32).reshape(w.shape + (2,))
            gone = ~pres
            zeros = zeros and bool((v[gone] == 0).all()) and not bool(np.signbit(v[gone]).any()) and bool(np.isfinite(v).all())
    out["zeros"] = 0.0 if zeros else np.inf
    if xs is not None:
        x = xs.astype(np.complex128)                                                     # [n, K, L, m]
        Bx = np.einsum("nkam,nklm->nkla", B, x)
        GBx = snr * np.einsum("nkam,nkla->nklm", np.conj(B), Bx)
        out["C2"] = _ratio(np.linalg.norm(GBx - g64[..., :L, None] * x, axis=-1), tol_v * (1 + cj * U24), pres)
        gram = np.einsum("nkim,nkjm->nkij", np.conj(x), x)
        both = pres[..., :, None] & pres[..., None, :]
        out["C3"] = _ratio(np.abs(gram - np.eye(L)), 2 * cj * U24, both)
        # the gauge: a component with imaginary part exactly +0 and a positive real part carries the largest modulus (to
        # the rounding of the phase rotation: the kernel picks the largest before it rotates)
        v = np.ascontiguousarray(xs).view(np.float32).reshape(xs.shape + (2,))
        real_pos = (v[..., 1] == 0) & ~np.signbit(v[..., 1]) & (v[..., 0] > 0)
        ax = np.abs(x)
        ok = (np.where(real_pos, ax, 0.0).max(axis=-1) >= ax.max(axis=-1) * (1 - 8 * U24))
        out["gauge"] = 0.0 if bool(ok[pres].all()) else np.inf
        if m >= 1 and pres[..., 0].any():
            ref_g, ref_tx, ref_rx = precoders_from_channel(H, snr)
            x_ref = (ref_rx if rx_small else ref_tx)[..., 0, :]
            g1 = ref_g[..., 1] if m > 1 else np.zeros_like(ref_g[..., 0])
            delta = g64[..., 0] - g1
            gap = pres[..., 0] & (delta > 10 * tol_v[..., 0])
            x0 = x[..., 0, :]
            n0 = (np.abs(x0) ** 2).sum(axis=-1)
            ip2 = np.abs(np.einsum("nkm,nkm->nk", np.conj(x_ref), x0)) ** 2
            bound = (tol_v[..., 0] / np.where(gap, delta, 1.0)) ** 2
            out["C5"] = _ratio(1.0 - ip2 / np.where(n0 > 0, n0, 1.0), bound, gap)
            out["C5_unnormalised"] = _ratio(1.0 - ip2, bound, gap)                       # reported, not a criterion
            out["C5_share"] = float(gap[pres[..., 0]].mean())
    if xs is not None and ys is not None:
        y = ys.astype(np.complex128)
        r1 = np.sqrt(snr) * Bx - np.sqrt(g64[..., :L, None]) * y
        out["C1"] = _ratio(np.linalg.norm(r1, axis=-1), 2 * np.sqrt(snr) * e, pres)
    if ys is not None:
        y = ys.astype(np.complex128)
        gn = np.linalg.norm(g64, axis=-1)[..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            tol4 = 2 * cj * U24 + (3 * cj + 64) * U24 * gn / np.where(pres, g64[..., :L], 1.0)
        out["C4"] = _ratio(np.abs((np.abs(y) ** 2).sum(axis=-1) - 1.0), tol4, pres)
    return out


# ---- the float32 model of the kernel's iteration ------------------------------------------------------------------------

def jacobi_vec_f32(G, sweeps, gate=True):
    """(d [B, m] descending and clamped to >= 0, X [B, m, m] complex128 holding the float32 columns sorted with d,
    |G|_F [B]) after `sweeps` cyclic sweeps of the kernel's EPI_VECTORS rotation on G [B, m, m] (Hermitian; cast to float32
    pairs), every operation in float32.  gate=False: rotation wherever |G_pq| > 0, as the eigenvalue-only epilogue."""
    G = np.asarray(G)
    m = G.shape[-1]
    gr = np.array(G.real, dtype=np.float32).reshape(-1, m, m)
    gi = np.array(G.imag, dtype=np.float32).reshape(-1, m, m)
    for i in range(m):                                                                   # the kernel keeps the upper triangle
        gi[:, i, i] = 0
        gr[:, i + 1:, i] = 0
        gi[:, i + 1:, i] = 0
    norm = np.sqrt((gr.astype(np.float64) ** 2).sum(axis=(1, 2)) * 2 + (gi.astype(np.float64) ** 2).sum(axis=(1, 2)) * 2
                   - (np.einsum("bii->bi", gr).astype(np.float64) ** 2).sum(axis=1))
    xr = np.broadcast_to(np.eye(m, dtype=np.float32), gr.shape).copy()
    xi = np.zeros_like(gr)
    one, half = np.float32(1), np.float32(0.5)

    def get(k, p):
        return (gr[:, k, p], gi[:, k, p]) if k < p else (gr[:, p, k], -gi[:, p, k])

    def put(k, p, re, im):
        if k < p:
            gr[:, k, p], gi[:, k, p] = re, im
        else:
            gr[:, p, k], gi[:, p, k] = re, -im

    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for sw in range(sweeps):
            for p in range(m - 1):
                for q in range(p + 1, m):
                    a, b = gr[:, p, q].copy(), gi[:, p, q].copy()
                    ag = np.sqrt(_fma(a, a, b * b))
                    nz = ag >= GATE if gate else ag > 0
                    inv = one / ag
                    er, ei = np.where(nz, a * inv, one), np.where(nz, b * inv, np.float32(0))
                    dp, dq = gr[:, p, p].copy(), gr[:, q, q].copy()
                    tau = (dq - dp) * (half * inv)
                    t = np.copysign(one, tau) / (np.abs(tau) + np.sqrt(_fma(tau, tau, one)))
                    t = np.where(nz, t, np.float32(0)).astype(np.float32)
                    c = one / np.sqrt(_fma(t, t, one))
                    s = t * c
                    gr[:, p, p], gr[:, q, q] = _fma(-t, ag, dp), _fma(t, ag, dq)
                    gr[:, p, q] = 0
                    gi[:, p, q] = 0
                    for k in range(m):
                        if k == p or k == q:
                            continue
                        ur, ui = (v.copy() for v in get(k, p))
                        zr, zi = (v.copy() for v in get(k, q))
                        yr, yi = _fma(zr, er, zi * ei), _fma(zi, er, -(zr * ei))
                        put(k, p, _fma(c, ur, -(s * yr)), _fma(c, ui, -(s * yi)))
                        put(k, q, _fma(s, ur, c * yr), _fma(s, ui, c * yi))
                    for k in range(m):
                        ur, ui, zr, zi = xr[:, k, p].copy(), xi[:, k, p].copy(), xr[:, k, q].copy(), xi[:, k, q].copy()
                        yr, yi = _fma(zr, er, zi * ei), _fma(zi, er, -(zr * ei))
                        xr[:, k, p], xi[:, k, p] = _fma(c, ur, -(s * yr)), _fma(c, ui, -(s * yi))
                        xr[:, k, q], xi[:, k, q] = _fma(s, ur, c * yr), _fma(s, ui, c * yi)
    d = np.minimum(np.maximum(np.einsum("bii->bi", gr), np.float32(0)), np.finfo(np.float32).max).astype(np.float64)
    order = np.argsort(-d, axis=1, kind="stable")
    X = xr.astype(np.float64) + 1j * xi.astype(np.float64)
    return np.take_along_axis(d, order, axis=1), np.take_along_axis(X, order[:, None, :], axis=2), norm


def model_quality(G, m, gate=True):
    """(|X^H X - I|_F [B], worst column residual |G x_i - d_i x_i|_2 / |G|_F [B]) of the model with SWEEPS[m] sweeps on the
    float32 cast of G (the matrix the model sees), in float64"""
    G = np.asarray(G).reshape(-1, m, m)
    G32 = G.real.astype(np.float32).astype(np.float64) + 1j * G.imag.astype(np.float32).astype(np.float64)
    G32 = np.triu(G32, 1) + np.conj(np.swapaxes(np.triu(G32, 1), 1, 2)) + np.real(G32) * np.eye(m)
    d, X, norm = jacobi_vec_f32(G, SWEEPS[m], gate)
    orth = np.linalg.norm(np.conj(np.swapaxes(X, 1, 2)) @ X - np.eye(m), axis=(1, 2))
    res = np.linalg.norm(G32 @ X - X * d[:, None, :], axis=1).max(axis=1)
    return orth, res / np.where(norm > 0, norm, 1.0)
