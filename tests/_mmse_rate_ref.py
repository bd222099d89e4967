"""Reference of the linear-MMSE codebook rate (DMX_FLAG_RX_LINEAR_MMSE; tests/test_mmse_rate_cpu.py,
tests/test_gpu_mmse_rate.py): the definition from a channel tensor in complex128 via np.linalg.inv, and the tolerance the GPU
tests hold the kernel to.  A plain module: NumPy only, no torch, no GPU.

    E, s = snr / L and G_ck = E_ck^H E_ck as in tests/_codebook_rate_ref.py,   A_ck = I_L + s G_ck
    sinr[u, c, i, k] = 1 / [A_ck^-1]_ii - 1
    rate_ck[u, c, k] = sum_i log2(1 + sinr[u, c, i, k]) = -sum_i log2 [A_ck^-1]_ii
    rate_c[u, c]     = mean over k of rate_ck[u, c, k]

Tolerance (derived, not chosen).  Write f_i = -log2 [A^-1]_ii and r_i = A^-1 e_i, the i-th column of the inverse.  A is
Hermitian, so for a perturbation dA

    d [A^-1]_ii = -(A^-1 dA A^-1)_ii = -r_i^H dA r_i,          d f_i = r_i^H dA r_i / ([A^-1]_ii ln 2)
    |r_i^H dA r_i| <= |r_i|^2 |dA|_2 <= [A^-2]_ii |dA|_F       (|r_i|^2 = (A^-1 A^-1)_ii)
    |d sum_i f_i|  <= sum_i ([A^-2]_ii / [A^-1]_ii) |dA|_F / ln 2

The admitted dA is that of tests/_codebook_rate_ref.py: the projection E is held to TOL_REL of the user's peak over all rows,
so dE_ck has a Frobenius norm of at most e and dA = s (dE^H E + E^H dE + dE^H dE):

    e       = sqrt(M_rx L) TOL_REL max |E[u]|
    |dA|_F <= s (2 |E_ck|_F e + e^2)

The rounding of the elimination itself: the kernel's epilogue runs L eliminations of the matrix the joint rate eliminates
once (layer i ordered last, i = 0 .. L-1), and reports one pivot of each.  tests/_codebook_rate_ref.py admits
8 * 2^-24 (L + rate_joint_ck) for the log2 of the pivots of one such elimination; a single pivot's log2 errs by no more than
all of them together, so that term is added once per elimination, L times:

    tol_ck = sum_i ([A^-2]_ii / [A^-1]_ii) s (2 |E_ck|_F e + e^2) / ln 2  +  L * 8 * 2^-24 (L + rate_joint_ck)
    tol_c  = mean over k of tol_ck
"""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL
from tests._codebook_rate_ref import _gram, codebook_rate_from_channel, precoded


def _inverse(E, snr):
    """A^-1 [n, C, K, L, L] of the definition, complex128"""
    L = E.shape[3]
    return np.linalg.inv(np.eye(L) + (float(snr) / L) * _gram(E))


def mmse_sinr_from_channel(H, W, snr):
    """sinr [n, C, L, K] of the definition, float64"""
    inv = _inverse(precoded(H, W), snr)
    d = np.real(np.einsum("uckii->ucik", inv))
    return 1.0 / d - 1.0


def mmse_rate_from_channel(H, W, snr):
    """(rate_c [n, C], rate_ck [n, C, K]) of the definition, float64"""
    inv = _inverse(precoded(H, W), snr)
    rate_ck = -np.log2(np.real(np.einsum("uckii->ucki", inv))).sum(axis=-1)
    return rate_ck.mean(axis=2), rate_ck


def mmse_rate_tolerance(H, W, snr):
    """(tol_c [n, C], tol_ck [n, C, K]) of the module docstring"""
    E = precoded(H, W)
    n, C, m_rx, L, K = E.shape
    s = float(snr) / L
    inv = _inverse(E, snr)
    d1 = np.real(np.einsum("uckii->ucki", inv))                                              # [A^-1]_ii
    d2 = (np.abs(inv) ** 2).sum(axis=-2)                                                     # [A^-2]_ii = |column i|^2
    sens = (d2 / d1).sum(axis=-1)                                                            # [n, C, K]
    peak = np.abs(E).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    e = (np.sqrt(m_rx * L) * TOL_REL * peak)[:, None, None]
    e_f = np.sqrt((np.abs(E) ** 2).sum(axis=(2, 3)))                                         # [n, C, K]
    _, joint_ck = codebook_rate_from_channel(H, W, snr)
    tol_ck = sens * s * (2 * e_f * e + e * e) / np.log(2.0) + L * 8 * 2.0 ** -24 * (L + joint_ck)
    return tol_ck.mean(axis=2), tol_ck


def live_users(H):
    """users whose reference channel is not all zero"""
    return np.abs(np.asarray(H)).reshape(np.shape(H)[0], -1).max(axis=1) > 0


def loose_share(H, W, snr):
    """share of the live (user, codeword) entries whose MMSE tolerance exceeds 1 % of max(1, rate_ref)"""
    live = live_users(H)
    if not live.any():
        return 0.0
    rate_c, tol_c = mmse_rate_from_channel(H, W, snr)[0], mmse_rate_tolerance(H, W, snr)[0]
    return float((tol_c[live] > 0.01 * np.maximum(1.0, rate_c[live])).mean())
