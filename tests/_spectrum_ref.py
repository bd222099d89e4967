"""References of the spectrum tests (tests/test_spectrum_cpu.py, tests/test_gpu_spectrum.py): the per-user channel eigenmodes
and the water-filling rate from a channel tensor in complex128, a float32 model of the kernel's Jacobi iteration, and the
tolerances the GPU tests hold the kernel to.  A plain module: NumPy only, no torch, no GPU.

    gamma[u, k, i] = snr * lambda_i(H_k H_k^H),  i = 0 .. m-1 descending,  H_k = H[u, :, :, k],  m = min(M_rx, M_tx)
    rate_k[u, k]   = max over p_i >= 0, sum p_i = 1 of sum_i log2(1 + p_i gamma_i)
                   = sum_{i < a} log2(mu gamma_i),  mu = (1 + sum_{i < a} 1 / gamma_i) / a,
                     a the largest count of strongest modes with mu > 1 / gamma_{a-1}
    rate[u]        = mean over k of rate_k[u, k]
The non-zero eigenvalues of H H^H and H^H H agree, so the m x m Gram over the smaller array (tests/_rate_ref._gram) has
them all.

Jacobi model (jacobi_f32): the kernel's rotation loop restated operation by operation in float32, FMAs included, on the
upper triangle.  Pair (p, q), g = G_pq, in cyclic row order:
    |g| = sqrt(fma(a, a, b b)),  inv = 1 / |g|,  e = g inv,  tau = (G_qq - G_pp) (0.5 inv),
    t = sign(tau) / (|tau| + sqrt(fma(tau, tau, 1))),  t = 0 where |g| = 0,  c = 1 / sqrt(fma(t, t, 1)),  s = t c
    G_pp = fma(-t, |g|, G_pp),  G_qq = fma(t, |g|, G_qq),  G_pq = 0,  and for every other k:  x = G_kp,  y = G_kq conj(e),
    G_kp = c x - s y,  G_kq = s x + c y
SWEEPS[m] is the fixed sweep count of the kernel: per m the smallest count that leaves the off-diagonal Frobenius norm
<= 2^-24 |G|_F on every matrix of hard_grams(m) and on the float32 Grams of every GPU case (the search is
sweeps_needed; tests/test_spectrum_cpu.py repeats it for every m), plus one sweep of margin:
    needed  m = 1: 0   2: 1   3: 4   4: 5   5: 5   6: 6   7: 7   8: 7
    SWEEPS  m = 1: 0   2: 2   3: 5   4: 6   5: 6   6: 7   7: 8   8: 8

Eigenmode tolerance (derived, not chosen):
    tol_g[u, k] = snr (2 |H_k|_F e + e^2)  +  c_J 2^-24 |snr G_k|_F,     e = sqrt(M_rx M_tx) TOL_REL max|H[u]|
First term: a channel error the project's channel criterion admits (every entry of H[u] within TOL_REL of the user's peak,
tests/_cases.py) has |dH_k|_F <= e, so |dG|_2 <= |dG|_F <= 2 |H_k|_F e + e^2, and by Weyl's theorem no eigenvalue of a
Hermitian matrix moves by more than |dG|_2.  Second term: each rotation is an exact unitary similarity plus a rounding
perturbation E with |E|_F <= ROUNDINGS 2^-24 |G|_F, and Weyl again adds them up over the rotations:
    c_J = SWEEPS[m] * m (m - 1) / 2 * ROUNDINGS
ROUNDINGS = 13 is the longest chain of roundings one rotation puts on an entry, counted from the loop above: e carries 5
(b b, the fma, the square root, 1 / |g|, the product with inv), y = G_kq conj(e) adds 2 (one product, one fma), s carries 4
of its own (the fma, the square root, the division, t c; c carries 3) and the combination c x - s y adds 2.  The diagonal
pair takes t |g| with 10 roundings in t (3 in |g|, inv, the difference, the product, the fma, the square root, the sum, the
division) and 1 in the update: 11, below the 13.  The Frobenius norm of the Gram's own float32 accumulation is inside the
first term: the channel criterion is two orders above fp32 rounding.

Rate tolerance: the water-filling rate is monotone in every mode SNR, so the criterion is the bracket
    wf(max(gamma - tol_g, 0)) - r  <=  rate_k  <=  wf(gamma + tol_g) + r,     r = 8 * 2^-24 (m + rate_k)
(r: the fp32 rounding of the logarithms, as in tests/_rate_ref.py), which is rigorous where the number of modes in use
changes and a first-order formula is not."""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL
from tests._rate_ref import _gram

SWEEPS = {1: 0, 2: 2, 3: 5, 4: 6, 5: 6, 6: 7, 7: 8, 8: 8}
ROUNDINGS = 13
U24 = 2.0 ** -24


def c_jacobi(m, sweeps=None):
    """c_J of the module docstring"""
    return (SWEEPS[m] if sweeps is None else sweeps) * (m * (m - 1) // 2) * ROUNDINGS


# ---- float64 definitions ----------------------------------------------------------------------------------------------

def eigenmodes_from_channel(H, snr):
    """gamma [n, K, m], float64, descending: snr times the eigenvalues of the Gram over the smaller array"""
    lam = np.linalg.eigvalsh(_gram(H))[..., ::-1]
    return float(snr) * np.maximum(lam, 0.0)


def waterfill(gamma):
    """water-filling rate [...] in bit/s/Hz of mode SNRs gamma [..., m] under unit total power, float64, closed form"""
    g = -np.sort(-np.asarray(gamma, dtype=np.float64), axis=-1)
    m = g.shape[-1]
    pos = g > 0
    with np.errstate(divide="ignore"):
        inv = np.where(pos, 1.0 / np.where(pos, g, 1.0), np.inf)
    a = np.arange(1, m + 1)
    with np.errstate(invalid="ignore"):
        mu = (1.0 + np.cumsum(np.where(pos, inv, 0.0), axis=-1)) / a                         # mu of the a strongest modes
        ok = np.logical_and.accumulate(pos & (mu > inv), axis=-1)
    cnt = ok.sum(axis=-1)
    mu_a = np.take_along_axis(mu, np.maximum(cnt - 1, 0)[..., None], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(ok, np.log2(np.where(ok, mu_a * g, 1.0)), 0.0)
    return terms.sum(axis=-1)


def wf_rate_from_channel(H, snr):
    """(rate [n], rate_k [n, K], gamma [n, K, m]) of the definition"""
    gamma = eigenmodes_from_channel(H, snr)
    rate_k = waterfill(gamma)
    return rate_k.mean(axis=1), rate_k, gamma


# ---- the tolerances ---------------------------------------------------------------------------------------------------

def mode_tolerance(H, snr, cj=None):
    """tol_g [n, K] of the module docstring (the same for every mode of an entry)"""
    H = np.asarray(H).astype(np.complex128)
    n, m_rx, m_tx, K = H.shape
    m = min(m_rx, m_tx)
    peak = np.abs(H).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    e = (np.sqrt(m_rx * m_tx) * TOL_REL * peak)[:, None]
    h_f = np.sqrt((np.abs(H) ** 2).sum(axis=(1, 2)))
    g_f = np.linalg.norm(_gram(H), axis=(-2, -1))
    return float(snr) * (2 * h_f * e + e * e) + (c_jacobi(m) if cj is None else cj) * U24 * float(snr) * g_f


def log_rounding(m, rate_k):
    """r of the module docstring"""
    return 8 * U24 * (m + np.asarray(rate_k, dtype=np.float64))


def rate_bracket(H, snr, cj=None):
    """(lo [n, K], hi [n, K]) the water-filling rate of any admitted gamma lies in, r included"""
    _, rate_k, gamma = wf_rate_from_channel(H, snr)
    tol = mode_tolerance(H, snr, cj)[..., None]
    r = log_rounding(gamma.shape[-1], rate_k)
    return waterfill(np.maximum(gamma - tol, 0.0)) - r, waterfill(gamma + tol) + r


def _live(H):
    H = np.asarray(H)
    return np.abs(H).reshape(H.shape[0], -1).max(axis=1) > 0


def mode_share(H, snr, cj=None):
    """share of the live (user, k) entries whose eigenmode tolerance exceeds 1 % of the strongest mode"""
    live = _live(H)
    if not live.any():
        return 0.0
    g0 = eigenmodes_from_channel(H, snr)[..., 0]
    return float((mode_tolerance(H, snr, cj)[live] > 0.01 * g0[live]).mean())


def bracket_share(H, snr, cj=None):
    """share of the live (user, k) entries whose bracket half-width exceeds 1 % of max(1, rate_ref)"""
    live = _live(H)
    if not live.any():
        return 0.0
    _, rate_k, _ = wf_rate_from_channel(H, snr)
    lo, hi = rate_bracket(H, snr, cj)
    return float(((hi - lo)[live] / 2 > 0.01 * np.maximum(1.0, rate_k[live])).mean())


# ---- the float32 model of the kernel's iteration ----------------------------------------------------------------------

def _fma(a, b, c):
    """fma in float32: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def jacobi_f32(G, sweeps, history=None):
    """(diagonal [B, m] descending and clamped to >= 0, off-diagonal Frobenius norm [B], |G|_F [B]) after `sweeps` cyclic
    sweeps of the kernel's rotation on G [B, m, m] (Hermitian; cast to float32 pairs), every operation in float32.
    `history`: a list that receives the off-diagonal norm [B] after 0, 1, .., sweeps sweeps."""
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
    one, half = np.float32(1), np.float32(0.5)

    def off_norm():
        d = np.einsum("bii->bi", gr).astype(np.float64)
        return np.sqrt(np.maximum((gr.astype(np.float64) ** 2).sum(axis=(1, 2)) * 2 + (gi.astype(np.float64) ** 2).sum(axis=(1, 2)) * 2
                                  - 2 * (d ** 2).sum(axis=1), 0.0))

    def get(k, p):
        return (gr[:, k, p], gi[:, k, p]) if k < p else (gr[:, p, k], -gi[:, p, k])

    def put(k, p, re, im):
        if k < p:
            gr[:, k, p], gi[:, k, p] = re, im
        else:
            gr[:, p, k], gi[:, p, k] = re, -im

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for sw in range(sweeps):
            if history is not None:
                history.append(off_norm())
            for p in range(m - 1):
                for q in range(p + 1, m):
                    a, b = gr[:, p, q].copy(), gi[:, p, q].copy()
                    ag = np.sqrt(_fma(a, a, b * b))
                    nz = ag > 0
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
                        xr, xi = (v.copy() for v in get(k, p))
                        zr, zi = (v.copy() for v in get(k, q))
                        yr, yi = _fma(zr, er, zi * ei), _fma(zi, er, -(zr * ei))
                        put(k, p, _fma(c, xr, -(s * yr)), _fma(c, xi, -(s * yi)))
                        put(k, q, _fma(s, xr, c * yr), _fma(s, xi, c * yi))
    d = np.einsum("bii->bi", gr).astype(np.float64)
    off = off_norm()
    if history is not None:
        history.append(off)
    return -np.sort(-np.maximum(d, 0.0), axis=1), off, norm


def _unitary(rng, m):
    q, r = np.linalg.qr(rng.normal(size=(m, m)) + 1j * rng.normal(size=(m, m)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def hard_grams(m, draws=300, seed=99):
    """[B, m, m] complex128 positive semidefinite matrices that are hard for a fixed sweep count, at mode-SNR scale: rank
    one, two equal eigenvalues (small and large against the rest), clustered eigenvalues, a 1e6 spread up and down, diagonal,
    all ones, the identity, Wishart draws and steering-vector outer products; 8 matrices per draw, 2403 in all.  The last
    sweep of the need is decided by a handful of them (8 of 2403 at m = 8, 1 at m = 4), hence the 300 draws."""
    rng = np.random.default_rng(seed + m)
    out = [np.diag(np.logspace(0, 6, m)).astype(np.complex128), np.eye(m, dtype=np.complex128) * 37.0,
           np.ones((m, m), dtype=np.complex128) * 1e3]
    spectra = [np.r_[1e3, np.zeros(m - 1)], np.r_[5.0, 5.0, 1.0 + 0.5 * np.arange(max(m - 2, 0))][:m] * 1e2,
               (1 + 1e-4 * np.arange(m)) * 1e4, np.logspace(0, 6, m), np.logspace(-3, 3, m)[::-1].copy(),
               np.r_[7e5, 7e5, np.logspace(4, 0, max(m - 2, 0))][:m]]
    for _ in range(draws):
        for lam in spectra:
            u = _unitary(rng, m)
            out.append((u * lam) @ u.conj().T)
        x = rng.normal(size=(m, 2 * m)) + 1j * rng.normal(size=(m, 2 * m))
        out.append(x @ x.conj().T * 10 ** rng.uniform(-2, 5))
        v = np.exp(2j * np.pi * rng.uniform(size=m))                                     # a steering vector: equal diagonal
        out.append(np.outer(v, v.conj()) * 10 ** rng.uniform(0, 6))
    G = np.stack(out)
    return (G + np.conj(np.swapaxes(G, 1, 2))) / 2


def repeated_grams(m, draws=24, seed=29):
    """[B, m, m] matrices with a non-zero eigenvalue repeated three times or more (5, 5, 1, .., 1 times 100, and one half of
    the spectrum at 7e5 with the other at 3).  Inside such a cluster the diagonal differences sit at the float32 spacing of the eigenvalue itself, the angles carry no information
    and the off-diagonal norm falls only linearly, a factor of about 1.5 per sweep, from about 40 * 2^-24 |G|_F: these are
    NOT part of the search for SWEEPS.  The eigenvalues are not affected (a residual inside a cluster moves them by at
    most its norm), which is what tests/test_spectrum_cpu.py holds on this set."""
    rng = np.random.default_rng(seed + m)
    out = []
    for _ in range(draws):
        for lam in (np.r_[5.0, 5.0, np.ones(max(m - 2, 0))][:m] * 1e2, np.r_[np.full((m + 1) // 2, 7e5), np.full(m // 2, 3.0)]):
            u = _unitary(rng, m)
            out.append((u * lam) @ u.conj().T)
    G = np.stack(out)
    return (G + np.conj(np.swapaxes(G, 1, 2))) / 2


def sweeps_needed(G, limit=12):
    """the smallest sweep count <= limit that leaves off <= 2^-24 |G|_F on every matrix of G (one run of the model)"""
    history = []
    _, _, norm = jacobi_f32(G, limit, history)
    for s, off in enumerate(history):
        if (off <= U24 * norm).all():
            return s
    raise AssertionError(f"no convergence within {limit} sweeps")
