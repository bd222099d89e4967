"""References of the rate tests (tests/test_rate_cpu.py, tests/test_gpu_rate.py): the definition of the per-user achievable
rate from a channel tensor in complex128, and the tolerance the GPU tests hold the kernel to.  A plain module: NumPy only,
no torch, no GPU.

    rate_k[u, k] = log2 det(I + (snr / M_tx) H_k H_k^H),   H_k = H[u, :, :, k]
    rate[u]      = mean over k of rate_k[u, k]

Tolerance (derived, not chosen): the change of the rate, to first order, under any channel error the project's own channel
criterion admits (every entry of H[u] within TOL_REL of the user's peak, tests/_cases.py), plus the fp32 rounding of the
logarithms.  d log det(A) = tr(A^-1 dA) and |tr(X Y)| <= |X|_F |Y|_F, with dA = s (dH H^H + H dH^H + dH dH^H):

    e      = sqrt(M_rx M_tx) TOL_REL max|H[u]|                                  (the Frobenius norm of an admitted dH_k)
    tol_k  = |(I + s G_k)^-1|_F  s (2 |H_k|_F e + e^2) / ln 2  +  8 * 2^-24 (m + rate_k)
    tol[u] = mean over k of tol_k
with s = snr / M_tx and G_k the m x m Gram over the smaller array."""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL


def _gram(H):
    """[n, K, m, m] Gram over the smaller array, complex128, from H [n, M_rx, M_tx, K]"""
    H = np.asarray(H).astype(np.complex128)
    if H.shape[1] <= H.shape[2]:
        return np.einsum("uitk,ujtk->ukij", H, H.conj())
    return np.einsum("urik,urjk->ukij", H.conj(), H)


def rate_from_channel(H, snr):
    """(rate [n], rate_k [n, K]) of the definition, float64, slogdet over the smaller Gram"""
    H = np.asarray(H)
    s = float(snr) / H.shape[2]
    G = _gram(H)
    m = G.shape[-1]
    sign, logdet = np.linalg.slogdet(np.eye(m) + s * G)
    rate_k = logdet / np.log(2.0)
    return rate_k.mean(axis=1), rate_k


def rate_tolerance(H, snr):
    """(tol [n], tol_k [n, K]) of the module docstring"""
    H = np.asarray(H).astype(np.complex128)
    n, m_rx, m_tx, K = H.shape
    s = float(snr) / m_tx
    G = _gram(H)
    m = G.shape[-1]
    inv_f = np.linalg.norm(np.linalg.inv(np.eye(m) + s * G), axis=(-2, -1))                 # [n, K]
    peak = np.abs(H).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    e = (np.sqrt(m_rx * m_tx) * TOL_REL * peak)[:, None]
    h_f = np.sqrt((np.abs(H) ** 2).sum(axis=(1, 2)))                                        # [n, K]
    _, rate_k = rate_from_channel(H, snr)
    tol_k = inv_f * s * (2 * h_f * e + e * e) / np.log(2.0) + 8 * 2.0 ** -24 * (m + rate_k)
    return tol_k.mean(axis=1), tol_k


def median_snr(H):
    """The SNR every case uses, from the reference alone: 100 M_tx / median over live users of mean_k |H_k|_F^2, which
    puts the median user at 20 dB"""
    H = np.asarray(H)
    p = (np.abs(H.astype(np.complex128)) ** 2).sum(axis=(1, 2)).mean(axis=1)
    live = p > 0
    return 100.0 * H.shape[2] / float(np.median(p[live]))


def tolerance_share(H, snr):
    """share of the live (user, k) entries whose tolerance exceeds 1 % of max(1, rate_ref)"""
    _, rate_k = rate_from_channel(H, snr)
    _, tol_k = rate_tolerance(H, snr)
    live = (np.abs(np.asarray(H)).reshape(H.shape[0], -1).max(axis=1) > 0)
    if not live.any():
        return 0.0
    return float((tol_k[live] > 0.01 * np.maximum(1.0, rate_k[live])).mean())
