"""Reference of the subband-PMI tests (tests/test_subband_pmi_cpu.py, tests/test_gpu_subband_pmi.py), built on
tests/_codebook_rate_ref.py: NumPy only, no torch, no GPU, and no tolerance of its own.

Subbands partition the selection in its own order: subband s covers the positions s B .. min((s + 1) B, K) - 1,
n_sb = ceil(K / B), the last one possibly short, B >= K one subband.

    rate_sb_c[u, s, c] = mean over k in subband s of rate_ck[u, c, k]
    tol_sb_c[u, s, c]  = mean over k in subband s of tol_ck[u, c, k]
    rate_c, tol_c      = the wideband values of _codebook_rate_ref (the mean over all k)

The mean of the per-subcarrier tolerances bounds the error of the mean of the per-subcarrier rates exactly as tol_c does for the
whole selection; the float32 summation term 8 * 2^-24 (L + rate_ck) is part of every tol_ck already."""
from __future__ import annotations

import numpy as np

from tests._codebook_rate_ref import codebook_rate_from_channel, codebook_rate_tolerance


def subband_edges(K, B):
    """[(first, end)] of the subbands of a selection of K positions; B None: one subband"""
    K = int(K)
    B = K if B is None else min(int(B), K)
    assert B >= 1 and K >= 1, (K, B)
    return [(k0, min(k0 + B, K)) for k0 in range(0, K, B)]


def subband_means(x_ck, B):
    """[n, n_sb, C] from [n, C, K]: the mean over each subband's own length"""
    x_ck = np.asarray(x_ck)
    return np.stack([x_ck[:, :, a:b].mean(axis=2) for a, b in subband_edges(x_ck.shape[2], B)], axis=1)


def subband_reference(H, W, snr, B):
    """dict of rate_c, tol_c [n, C] and rate_sb_c, tol_sb_c [n, n_sb, C] of the channel tensor H, float64"""
    rate_c, rate_ck = codebook_rate_from_channel(H, W, snr)
    tol_c, tol_ck = codebook_rate_tolerance(H, W, snr)
    return dict(rate_c=rate_c, tol_c=tol_c, rate_sb_c=subband_means(rate_ck, B), tol_sb_c=subband_means(tol_ck, B))


def subband_tolerance_share(H, ref):
    """share of the live (user, subband, codeword) entries whose tolerance exceeds 1 % of max(1, rate_sb_ref)"""
    live = np.abs(np.asarray(H)).reshape(np.shape(H)[0], -1).max(axis=1) > 0
    if not live.any():
        return 0.0
    return float((ref["tol_sb_c"][live] > 0.01 * np.maximum(1.0, ref["rate_sb_c"][live])).mean())


def reference_ranks(refs, ranks):
    """(rank [n], best wideband rate [n], its tolerance [n]) the references of several layer counts pick: `refs` the
    subband_reference of each entry of `ranks` (ascending L); the first maximum of the best wideband rate per rank"""
    best = np.stack([r["rate_c"].max(axis=1) for r in refs], axis=1)                      # [n, n_ranks]
    tol = np.stack([np.take_along_axis(r["tol_c"], r["rate_c"].argmax(axis=1)[:, None], axis=1)[:, 0] for r in refs], axis=1)
    i = best.argmax(axis=1)
    rows = np.arange(len(i))
    return np.asarray(ranks)[i], best[rows, i], tol[rows, i]
