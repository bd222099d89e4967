"""References and cases of the serving-set tests (tests/test_serving_set_cpu.py, tests/test_gpu_serving_set.py): the cell rate
of tests/_cell_rate_ref.py with set membership in place of `s == b`, and the multi-stream form of tests/_mu_ref.py.  A plain
module: NumPy only at module level, no torch, no GPU, nothing of the package.

Links b = 0 .. B-1, H_b [n, M_rx, M_tx_b, K] over the same users, rho_b = snr_b / M_tx_b, member [n, B] bool the set S_u:

    N_k          = I + sum_{b not in S_u} rho_b H_{b,k} H_{b,k}^H
    A_k          = N_k + sum_{b in S_u} rho_b H_{b,k} H_{b,k}^H
    rate_k[u, k] = log2 det A_k - log2 det N_k,    rate[u] = mean over k        (slogdet in complex128; A = N gives 0 exactly)

Tolerance: the derived rule of tests/_cell_rate_ref.py, unchanged but for who carries which weight.  A member of the set
enters A only, so its admitted Gram error d_b is carried with |A^-1|_F; every other link enters A and N with the same error
(the kernel forms A on the floats of the interference Gram), so it is carried with |A^-1 - N^-1|_F; the logarithm term is the
same:

    d_b   = rho_b (2 |H_{b,k}|_F e_b + e_b^2) / ln 2,       e_b = sqrt(M_rx M_tx_b) TOL_REL max|H_b[u]|
    tol_k = sum_{b in S_u} |A^-1|_F d_b + sum_{b not in S_u} |A^-1 - N^-1|_F d_b + 8 * 2^-24 (2 M_rx + log2 det A + log2 det N)

The multi-user form adds, per link j, the rounding term of tests/_mu_ref.py with the same weights:
w_j rho_j 2 |Y_{j,k}|_F r_j / ln 2, r_j = sqrt(M_rx) second[j, u].

A user is live if some link of its set reaches it; the cap condition of the project is that the tolerance exceeds 1 % of
max(1, rate_ref) on at most 5 % of a case's live (user, k) entries."""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL
from tests._cell_rate_ref import link_grams

LN2 = np.log(2.0)


def members_of(masks, n_links):
    """bool [n, B] of the bit masks `masks` [n] as dmx_cell_rate reads them: bit b < B = link b, a negative entry = nobody"""
    m = np.asarray(masks).astype(np.int64)
    return ((np.where(m < 0, 0, m)[:, None] >> np.arange(n_links)[None, :]) & 1).astype(bool)


def masks_of(member):
    """int32 [n]: the bit mask of each row of bool [n, B]"""
    member = np.asarray(member).astype(bool)
    return (member * (1 << np.arange(member.shape[1]))[None, :]).sum(axis=1).astype(np.int32)


def _split(Hs, snrs, member):
    """(A, N) of the definition, [n, K, M, M] each"""
    G = link_grams(Hs, snrs)
    mine = np.asarray(member).astype(bool).T                                  # [B, n]
    assert mine.shape == G.shape[:2]
    Gs = (G * mine[:, :, None, None, None]).sum(axis=0)
    Gi = (G * (~mine)[:, :, None, None, None]).sum(axis=0)
    N = np.eye(G.shape[-1]) + Gi
    return N + Gs, N


def set_rate_from_channels(Hs, snrs, member):
    """(rate [n], rate_k [n, K]) of the definition, float64"""
    A, N = _split(Hs, snrs, member)
    rate_k = (np.linalg.slogdet(A)[1] - np.linalg.slogdet(N)[1]) / LN2
    rate_k = np.where(np.asarray(member).any(axis=1)[:, None], rate_k, 0.0)
    return rate_k.mean(axis=1), rate_k


def set_rate_tolerance(Hs, snrs, member, second=None):
    """(tol [n], tol_k [n, K]) of the module docstring.  `second` [B, n]: the rounding term of tests/_mu_ref.py per link, for
    links behind a precoder; None for plain links."""
    A, N = _split(Hs, snrs, member)
    n, K, M, _ = A.shape
    member = np.asarray(member).astype(bool)
    Ai, Ni = np.linalg.inv(A), np.linalg.inv(N)
    a_f, d_f = np.linalg.norm(Ai, axis=(-2, -1)), np.linalg.norm(Ai - Ni, axis=(-2, -1))
    tol_k = 8 * 2.0 ** -24 * (2 * M + (np.linalg.slogdet(A)[1] + np.linalg.slogdet(N)[1]) / LN2)
    for b, (H, snr) in enumerate(zip(Hs, snrs)):
        H = np.asarray(H).astype(np.complex128)
        m_rx, m_tx = H.shape[1], H.shape[2]
        peak = np.abs(H).reshape(n, -1).max(axis=1) if n else np.zeros(0)
        e = (np.sqrt(m_rx * m_tx) * TOL_REL * peak)[:, None]
        h_f = np.sqrt((np.abs(H) ** 2).sum(axis=(1, 2)))                      # [n, K]
        d = float(snr) / m_tx * (2 * h_f * e + e * e) / LN2
        if second is not None:
            d = d + float(snr) / m_tx * 2 * h_f * (np.sqrt(m_rx) * np.asarray(second[b]))[:, None] / LN2
        tol_k = tol_k + np.where(member[:, b][:, None], a_f, d_f) * d
    return tol_k.mean(axis=1), tol_k


def reached(Hs):
    """bool [n, B]: link b has a non-zero channel to the user"""
    n = np.asarray(Hs[0]).shape[0]
    return np.stack([np.abs(np.asarray(H)).reshape(n, -1).max(axis=1) > 0 for H in Hs], axis=1)


def live_users(Hs, member):
    """bool [n]: some link of the user's set reaches it"""
    return (np.asarray(member).astype(bool) & reached(Hs)).any(axis=1)


def tolerance_share(Hs, snrs, member, second=None):
    """(share of the live (user, k) entries whose tolerance exceeds 1 % of max(1, rate_ref), median rate_k over them)"""
    _, rate_k = set_rate_from_channels(Hs, snrs, member)
    _, tol_k = set_rate_tolerance(Hs, snrs, member, second)
    live = live_users(Hs, member)
    if not live.any():
        return 0.0, 0.0
    return float((tol_k[live] > 0.01 * np.maximum(1.0, rate_k[live])).mean()), float(np.median(rate_k[live]))


# ---- the kernel-level cases: links of tests/test_gpu_cell_rate.py's helpers, a set per user ------------------------------------
B8_SETS = (0xFF, 0x80, 0x55, 0x01, 0xAA, 0x7E, 0, 0x18)


def set_cells():
    """[(cell, masks int64 [n])]: the cases of the issue and the launch residues.  The links come from `_cell` and `_case` of
    tests/test_gpu_cell_rate.py (imported here: that module needs the built library), the SNRs from `link_snrs`."""
    from tests import test_gpu_cell_rate as g
    c, cell = g._case, g._cell
    sel65 = range(3, 68)
    cells = [
        (cell("sets3_K1", [c("", 41, 25, [8, 1], [1, 1], 512, [0])] * 3), lambda u: u % 8),
        (cell("sets3_K65", [c("", 43, 25, [8, 1], [2, 1], 512, sel65)] * 3), lambda u: u % 8),
        (cell("sets_mixed", [c("", 31, 25, [8, 8], [2, 1], 512, [0, 17, 100]), c("", 31, 10, [4, 2], [2, 1], 512, [0, 17, 100]),
                             c("", 31, 32, [16, 1], [2, 1], 512, [0, 17, 100])]), lambda u: u % 8),
        (cell("sets_B8", [c("", 19, 25, [4, 2], [2, 1], 512, sel65)] * 8, inr_db=0.0), lambda u: B8_SETS[u % 8]),
        (cell("sets_m8", [c("", 21, 25, [8, 4], [4, 2], 512, [0, 17, 100])] * 2, serving_db=10.0), lambda u: (3, 1, 2, 0)[u % 4]),
        (cell("sets_counts", [c("", 48, 25, [4, 2], [2, 1], 512, [0, 3, 200], rays="counts")] * 3), lambda u: (u // 6) % 8),
        (cell("sets_panel", [c("", 23, 25, [8, 8], [2, 2], 512, range(0, 512, 7))] * 3), lambda u: u % 8),
    ]
    # launch residue: 4 k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 1-wave shape (two links: every subset)
    for n in (41, 42, 43):
        cells.append((cell(f"sets_wpb4_users{n}", [c("", n, 25, [8, 1], [1, 1], 512, [0, 5])] * 2), lambda u: u % 4))
    cells.append((cell("sets_wpb1_users7", [c("", 7, 25, [16, 16], [2, 2], 512, range(64))] * 2), lambda u: u % 4))
    return [(cl, np.array([f(u) for u in range(cl["links"][0]["n"])], np.int64)) for cl, f in cells]


# ---- several streams per user in compute_mu_rate -------------------------------------------------------------------------------
# name -> (case of tests/_mu_cases.MU_CASES: its rays, codebook and snr_db; group width G; power shift in dB; streams L)
MU_SET_CASES = {
    "G1_L3": ("G1_ue1x1_K1_P3_snr10", 1, 85.0, 3),
    "G2_L2": ("G2_ue2x1_K64_P25_snr30", 2, 62.0, 2),
    "G4_L2": ("G4_ue2x2_K70_P32_snr-10", 4, 102.0, 2),
    "G2_L4": ("G8_ue4x2_K130_P25_snr10", 2, 85.0, 4),
}


def mu_set_setup(name):
    """(case, oracle parameters, rays, F, beams [n_ue, L], groups [n_groups, G], snr_db, where the rays live).  Beams: L
    distinct rows of F per user, the last entry -1 for the users with u % 3 == 1."""
    from tests import _mu_cases as CS
    from tests._cases import oracle_params
    base, G, shift, L = MU_SET_CASES[name]
    changes, n, loaded, cb, G_base, snr_db, place, _ = CS.MU_CASES[base]
    case = {**CS.BASE, **changes}
    F = CS.codebook(cb, case["bs_shape"])
    rng = np.random.default_rng(700 + 10 * G + L)
    beams = np.stack([rng.permutation(len(F))[:L] for _ in range(n)]).astype(np.int64)
    beams[np.arange(n) % 3 == 1, L - 1] = -1
    return case, oracle_params(case, CS.UE_ROT), CS.rays(n, loaded, seed=20 + G_base, shift=shift), F, beams, CS.groups_of(n, G), snr_db, place


def stream_table(beams, groups, n_ue):
    """(idx [G L, n], streams of the group [n], member [n, G L], partners [n, G - 1]) by the definition: link j L + i is stream i
    of member j of the user's group, the user itself member 0; -1 where there is none, or the user is in no group"""
    from tests._mu_ref import partners_of
    beams = np.asarray(beams).reshape(n_ue, -1)
    L = beams.shape[1]
    partners, size = partners_of(groups, n_ue)
    G = partners.shape[1] + 1
    idx = -np.ones((G * L, n_ue), np.int64)
    total = np.zeros(n_ue, np.int64)
    for u in range(n_ue):
        if size[u] == 0:
            continue
        for j, v in enumerate([u] + [int(p) for p in partners[u] if p >= 0]):
            idx[j * L:(j + 1) * L, u] = beams[v]
            total[u] += (beams[v] >= 0).sum()
    member = (idx[:L] >= 0).T
    member = np.concatenate([member, np.zeros((n_ue, (G - 1) * L), bool)], axis=1)
    return idx, total, member, partners


def mu_set_reference(rays, params, F, beams, groups, snr_db):
    """dict(rate, rate_k, tol, tol_k, partners, stream_snr, stream_tol, member, live, Ys, second) of a multi-stream
    `compute_mu_rate` call; the stream SNR and its tolerance as tests/_mu_ref.mu_reference forms them"""
    from tests import _mu_ref as MR
    n = rays["power"].shape[0]
    snr = 10.0 ** (snr_db / 10.0)
    H = MR.oracle_channels(rays, params)
    idx, total, member, partners = stream_table(beams, groups, n)
    J = len(idx)
    scale = np.broadcast_to(1.0 / np.sqrt(np.maximum(total, 1)), (J, n))
    Y = MR.precoded(H, F, idx, scale)
    Ys = [Y[j][:, :, None, :] for j in range(J)]
    rate, rate_k = set_rate_from_channels(Ys, [snr] * J, member)
    prep = MR.R.prepared(rays, params, None, None)
    second = MR.rounding_term(rays, prep, params, F, idx, scale)
    tol, tol_k = set_rate_tolerance(Ys, [snr] * J, member, second)
    a, rel = MR._moduli(rays, prep, params, F, idx, scale)
    delta = TOL_REL * a.max(axis=2) + (a * rel).max(axis=2)
    stream = snr * (a * a).sum(axis=2)
    stream_tol = snr * (2 * delta * a.sum(axis=2) + a.shape[2] * delta ** 2) + 40 * 2.0 ** -24 * stream
    return dict(rate=rate, rate_k=rate_k, tol=tol, tol_k=tol_k, partners=partners, stream_snr=stream.T, stream_tol=stream_tol.T,
                member=member, live=live_users(Ys, member), Ys=Ys, second=second, snr=snr)
