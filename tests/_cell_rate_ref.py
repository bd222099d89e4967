"""References of the cell-rate tests (tests/test_cell_rate_cpu.py, tests/test_gpu_cell_rate.py): the definition of the
downlink rate under inter-cell interference from the per-link channel tensors in complex128, and the tolerances the GPU
tests hold the kernel to.  A plain module: NumPy only, no torch, no GPU.

Links b = 0 .. B-1, H_b [n, M_rx, M_tx_b, K] over the same users, rho_b = snr_b / M_tx_b, serving link s = serving[u]:

    N_k          = I + sum_{b != s} rho_b H_{b,k} H_{b,k}^H            (M_rx x M_rx)
    A_k          = N_k + rho_s H_{s,k} H_{s,k}^H
    rate_k[u, k] = log2 det A_k - log2 det N_k,    rate[u] = mean over k
    a user whose serving index is outside 0 .. B-1 gets 0

Tolerance (derived, not chosen; extends tests/_rate_ref.py): the first-order change of the rate under any channel error the
project's channel criterion admits on each link, plus the fp32 rounding of the two logarithms.  With
e_b = sqrt(M_rx M_tx_b) TOL_REL max|H_b[u]| the Frobenius norm of an admitted dH_{b,k}, the Gram of link b moves by at most
rho_b (2 |H_{b,k}|_F e_b + e_b^2) in Frobenius norm; d log det X = tr(X^-1 dX) and |tr(X Y)| <= |X|_F |Y|_F.  The serving link
enters A only, an interferer enters A and N with the same error (the kernel adds the serving Gram to the floats of the
interference Gram), so its share is tr((A^-1 - N^-1) dG_b):

    d_b   = rho_b (2 |H_{b,k}|_F e_b + e_b^2) / ln 2
    tol_k = |A^-1|_F d_s + sum_{b != s} |A^-1 - N^-1|_F d_b + 8 * 2^-24 (2 M_rx + log2 det A + log2 det N)
    tol[u] = mean over k of tol_k

link_snr[u, b] = snr_b * sum over the kept paths of |c_{b,l}|^2, c the frequency-domain coefficient sqrt(p / N) e^{j phase}:
from the oracle's TIME-domain tensor of the same link, whose entry [u, 0, 0, s] is sqrt(p_s) e^{j phase} of the s-th kept path
(valid while no path is clipped: max delay < N / bandwidth),

    link_snr_ref = snr_b / N * sum_s |H_td[u, 0, 0, s]|^2
    tol          = snr_b / N * (2 TOL_REL peak sum_s |H_td[u, 0, 0, s]| + L (TOL_REL peak)^2) + 40 * 2^-24 link_snr_ref

with peak = max|H_td[u]| and L the path slots: each entry within TOL_REL of the user's peak (the channel criterion), and 40
float32 roundings for the 32 squares, the xor tree and the scaling."""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL

LN2 = np.log(2.0)


def link_grams(Hs, snrs):
    """[B, n, K, M_rx, M_rx]: rho_b H_{b,k} H_{b,k}^H per link, complex128"""
    out = []
    for H, snr in zip(Hs, snrs):
        H = np.asarray(H).astype(np.complex128)
        out.append(float(snr) / H.shape[2] * np.einsum("uitk,ujtk->ukij", H, H.conj()))
    return np.stack(out)


def _split(Hs, snrs, serving):
    """(A, N, served) of the definition: [n, K, M, M] each, served [n] bool"""
    G = link_grams(Hs, snrs)
    B, n, K, M, _ = G.shape
    s = np.asarray(serving).astype(np.int64)
    served = (s >= 0) & (s < B)
    sc = np.where(served, s, 0)
    mine = (np.arange(B)[:, None] == sc[None, :]) & served[None, :]                       # [B, n]
    Gs = (G * mine[:, :, None, None, None]).sum(axis=0)
    Gi = (G * (~mine)[:, :, None, None, None]).sum(axis=0)
    N = np.eye(M) + Gi
    return N + Gs, N, served


def cell_rate_from_channels(Hs, snrs, serving):
    """(rate [n], rate_k [n, K]) of the definition, float64"""
    A, N, served = _split(Hs, snrs, serving)
    rate_k = (np.linalg.slogdet(A)[1] - np.linalg.slogdet(N)[1]) / LN2
    rate_k = np.where(served[:, None], rate_k, 0.0)
    return rate_k.mean(axis=1), rate_k


def cell_rate_tolerance(Hs, snrs, serving):
    """(tol [n], tol_k [n, K]) of the module docstring"""
    A, N, served = _split(Hs, snrs, serving)
    B = len(Hs)
    n, K, M, _ = A.shape
    Ai, Ni = np.linalg.inv(A), np.linalg.inv(N)
    a_f, d_f = np.linalg.norm(Ai, axis=(-2, -1)), np.linalg.norm(Ai - Ni, axis=(-2, -1))  # [n, K]
    s = np.asarray(serving).astype(np.int64)
    tol_k = 8 * 2.0 ** -24 * (2 * M + (np.linalg.slogdet(A)[1] + np.linalg.slogdet(N)[1]) / LN2)
    for b, (H, snr) in enumerate(zip(Hs, snrs)):
        H = np.asarray(H).astype(np.complex128)
        m_rx, m_tx = H.shape[1], H.shape[2]
        peak = np.abs(H).reshape(n, -1).max(axis=1) if n else np.zeros(0)
        e = (np.sqrt(m_rx * m_tx) * TOL_REL * peak)[:, None]
        h_f = np.sqrt((np.abs(H) ** 2).sum(axis=(1, 2)))                                   # [n, K]
        d = float(snr) / m_tx * (2 * h_f * e + e * e) / LN2
        tol_k = tol_k + np.where((s == b)[:, None], a_f, d_f) * d
    return tol_k.mean(axis=1), tol_k


def link_power(H):
    """[n] mean over k of |H_k|_F^2 of one link"""
    return (np.abs(np.asarray(H).astype(np.complex128)) ** 2).sum(axis=(1, 2)).mean(axis=1)


def link_snrs(Hs, serving_db=20.0, inr_db=10.0):
    """The per-link SNRs every case uses, from the reference alone: link 0 - the nominal serving cell - puts its median live
    user at `serving_db` (tests/_rate_ref.median_snr's rule: 10^(dB/10) M_tx / median over live users of mean_k |H_k|_F^2),
    every other link puts its median live user at `inr_db`."""
    out = []
    for b, H in enumerate(Hs):
        p = link_power(H)
        out.append(10.0 ** ((serving_db if b == 0 else inr_db) / 10.0) * np.asarray(H).shape[2] / float(np.median(p[p > 0])))
    return out


def link_snr_reference(H_td, snr, n_subcarriers):
    """(link_snr_ref [n], tol [n]) of one link from the oracle's time-domain tensor [n, M_rx, M_tx, L]"""
    H_td = np.asarray(H_td).astype(np.complex128)
    n, L = H_td.shape[0], H_td.shape[3]
    a = np.abs(H_td[:, 0, 0, :])
    peak = np.abs(H_td).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    ref = float(snr) / n_subcarriers * (a ** 2).sum(axis=1)
    tol = float(snr) / n_subcarriers * (2 * TOL_REL * peak * a.sum(axis=1) + L * (TOL_REL * peak) ** 2) + 40 * 2.0 ** -24 * ref
    return ref, tol


def reference_serving(ls_ref, live):
    """argmax_b of the reference link_snr [n, B], the first on ties, -1 where no link of the user is live ([n, B] bool)"""
    s = np.argmax(ls_ref, axis=1).astype(np.int64)
    s[~np.asarray(live).any(axis=1)] = -1
    return s


def tolerance_share(Hs, snrs, serving):
    """share of the live (user, k) entries - served, and the serving link reaches the user - whose tolerance exceeds 1 % of
    max(1, rate_ref)"""
    _, rate_k = cell_rate_from_channels(Hs, snrs, serving)
    _, tol_k = cell_rate_tolerance(Hs, snrs, serving)
    s = np.asarray(serving).astype(np.int64)
    n = rate_k.shape[0]
    live = np.zeros(n, bool)
    for b, H in enumerate(Hs):
        live |= (s == b) & (np.abs(np.asarray(H)).reshape(n, -1).max(axis=1) > 0)
    if not live.any():
        return 0.0
    return float((tol_k[live] > 0.01 * np.maximum(1.0, rate_k[live])).mean())
