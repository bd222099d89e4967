"""References of the transmit-precoding and multi-user rate tests (tests/test_mu_rate_cpu.py, tests/test_gpu_mu_rate.py),
restated in NumPy complex128 on the NumPy oracle without a line of the package.  A plain module: NumPy only, no torch, no GPU.

The link table.  beams [n] is the codebook row of each user, groups [n_groups, G] the users served together (-1 pads a row).
With g_u the members of u's group and partners[u] the other members in the order of the row,

    idx[0, u] = beams[u], idx[j, u] = beams[partners[u, j - 1]]            -1 where there is none, or u is in no group
    Y_j[u, r, 0, k] = sum_t H[u, r, t, k] F[idx[j, u], t] / sqrt(g_u)       0 where idx = -1;  H: the oracle's channels

and the rate is tests/_cell_rate_ref.cell_rate_from_channels(Ys, [snr] * G, serving) with serving = 0 for a user in a group,
-1 else: each Y_j is a link from a single-antenna base station, so rho_j = snr, and the split 1 / g_u sits in Y_j.

Tolerance of a channel of a `with_tx_precoder` view against ref[j, u] = H[u] @ F[idx[j, u]] (derived, not chosen): the
project's parity criterion plus the one float32 rounding of the power (dB) and the phase (degrees) the view stores - the
term tests/_combiner_ref.rounding_term builds for the receive side, restated for the transmit response
e[j, u, l] = s[j, u] sum_t F[idx[j, u], t] a_tx[u, t, l]  (s: the amplitude of the power split, 1 in a plain view):

    second[j, u] = sum_l |c_l| |e_l| (2 pi 2^-24 + 2^-24 |power'_l| ln 10 / 20),   power'_l = power_l + 10 log10 max(|e_l|^2, 2^-100)
    tol[j, u]    = TOL_REL max|ref[j, u]| + second[j, u]

|a_rx| = 1 and the subcarrier phasor has modulus 1, so `second` bounds the error the rounding leaves in every entry
Y_j[u, r, 0, k].

Tolerance of the multi-user rate.  tests/_cell_rate_ref.cell_rate_tolerance admits on link j a channel error of Frobenius
norm e_j = sqrt(M_rx) TOL_REL max|Y_j[u]| and carries it to the rate through d log det X = tr(X^-1 dX): the serving link
with |A^-1|_F, an interferer with |A^-1 - N^-1|_F.  The rounding adds r_j = sqrt(M_rx) second[j, u] to the norm of the error
of link j; to first order the Gram of the link moves by another rho (2 |Y_{j,k}|_F r_j), so

    tol_k = cell_rate_tolerance_k + sum_j w_j snr 2 |Y_{j,k}|_F r_j / ln 2,    w_0 = |A^-1|_F, w_j = |A^-1 - N^-1|_F for j > 0
    tol[u] = mean over k of tol_k

stream_snr[u, j] = snr sum over the kept paths of (|c_l| |e[j, u, l]|)^2 (tests/_cell_rate_ref's link_snr, from the path
moduli).  Each modulus a_l = |c_l| |e_l| is held to delta = TOL_REL max_l a_l + max_l a_l 2^-24 |power'_l| ln 10 / 20:

    tol = snr (2 delta sum_l a_l + L delta^2) + 40 * 2^-24 stream_snr_ref"""
from __future__ import annotations

import numpy as np

from tests import _cell_rate_ref as CR
from tests import _combiner_ref as R
from tests._cases import TOL_REL

E2_FLOOR = R.E2_FLOOR
LN2 = np.log(2.0)


def partners_of(groups, n_ue, shift=0):
    """(partners [n, G - 1], group size [n]) by the definition, one user at a time.  `shift`: take the partners from the
    group `shift` rows further on (the user's own place in the row left out) - a wrong table the cases have to tell apart."""
    groups = np.asarray(groups)
    n_groups, G = groups.shape
    partners = -np.ones((n_ue, max(G - 1, 0)), np.int64)
    size = np.zeros(n_ue, np.int64)
    for r in range(n_groups):
        row, src = groups[r], groups[(r + shift) % n_groups]
        for a, u in enumerate(row):
            if u < 0:
                continue
            others = [v for b, v in enumerate(src) if v >= 0 and (b != a if shift else v != u)]
            partners[u, :len(others)] = others
            size[u] = (row >= 0).sum()
    return partners, size


def link_table(beams, groups, n_ue, shift=0, swap=False):
    """(idx [G, n], group size [n]) of the module docstring.  `swap`: own and first partner's beam exchanged."""
    partners, size = partners_of(groups, n_ue, shift)
    beams = np.asarray(beams)
    G = partners.shape[1] + 1
    idx = -np.ones((G, n_ue), np.int64)
    idx[0] = np.where(size > 0, beams, -1)
    for j in range(1, G):
        p = partners[:, j - 1]
        idx[j] = np.where(p >= 0, beams[np.maximum(p, 0)], -1)
    if swap and G > 1:
        has = idx[1] >= 0
        idx[0, has], idx[1, has] = idx[1, has].copy(), idx[0, has].copy()
    return idx, size


def oracle_channels(rays, params, bs_fov=None, ue_fov=None):
    """the oracle's H [n, M_rx, M_tx, K] in complex128"""
    with R.oracle(params) as onp:
        return onp.compute_channels(rays, params, bs_fov, ue_fov)["channel"].astype(np.complex128)


def precoded(H, F, idx, scale=None):
    """Y [J, n, M_rx, K]: H[u] @ F[idx[j, u]] (times scale[j, u]), zeros where idx = -1"""
    F = np.asarray(F, np.complex128)
    idx = np.asarray(idx).reshape(-1, H.shape[0])
    W = np.where((idx >= 0)[:, :, None], F[np.maximum(idx, 0)], 0.0)                       # [J, n, M_tx]
    if scale is not None:
        W = W * np.asarray(scale, np.float64)[:, :, None]
    return np.einsum("urtk,jut->jurk", H, W)


def tx_responses(prep, params, F, idx, scale=None):
    """e [J, n, L] complex128 of the module docstring; 0 where the path has no departure angle or idx = -1"""
    from oracle import oracle_np as onp
    bs = params["bs_antenna"]
    a_tx = onp.array_response_batch(bs["shape"], bs["spacing"], prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"])
    idx = np.asarray(idx).reshape(-1, a_tx.shape[0])
    W = np.where((idx >= 0)[:, :, None], np.asarray(F, np.complex128)[np.maximum(idx, 0)], 0.0)
    if scale is not None:
        W = W * np.asarray(scale, np.float64)[:, :, None]
    return np.einsum("jut,utl->jul", W, a_tx)


def _moduli(rays, prep, params, F, idx, scale):
    """(a [J, n, P] the path moduli behind the precoder, 2^-24 |power'| ln 10 / 20 [J, n, P])"""
    P = int(params["num_paths"])
    e = np.abs(tx_responses(prep, params, F, idx, scale))[:, :, :P]
    c = R.path_moduli(prep, params)[None]
    with np.errstate(invalid="ignore"):
        power = np.asarray(rays["power"], np.float64)[None, :, :P] + 10 * np.log10(np.maximum(e * e, E2_FLOOR))
    rel = np.where(c > 0, 2.0 ** -24 * np.abs(np.nan_to_num(power)) * np.log(10.0) / 20.0, 0.0)
    return np.where(c > 0, c * e, 0.0), rel


def rounding_term(rays, prep, params, F, idx, scale=None):
    """second [J, n] of the module docstring"""
    a, rel = _moduli(rays, prep, params, F, idx, scale)
    return (a * (2 * np.pi * 2.0 ** -24 + rel)).sum(axis=2)


def view_reference(rays, params, F, idx, bs_fov=None, ue_fov=None):
    """(ref [J, n, M_rx, K], tol [J, n]) of a `with_tx_precoder` view"""
    ref = precoded(oracle_channels(rays, params, bs_fov, ue_fov), F, idx)
    second = rounding_term(rays, R.prepared(rays, params, bs_fov, ue_fov), params, F, idx)
    return ref, TOL_REL * np.abs(ref).max(axis=(2, 3)) + second


def split_scale(size, G):
    """[G, n]: 1 / sqrt(g_u), 1 for a user in no group"""
    return np.broadcast_to(1.0 / np.sqrt(np.maximum(size, 1)), (G, len(size)))


def mu_rate(H, F, idx, size, snr, split=True):
    """(rate [n], rate_k [n, K], the links Ys, serving) of the definition.  `split`: False leaves the power split out."""
    G = len(idx)
    Y = precoded(H, F, idx, split_scale(size, G) if split else None)
    Ys = [Y[j][:, :, None, :] for j in range(G)]
    serving = np.where(idx[0] >= 0, 0, -1)
    rate, rate_k = CR.cell_rate_from_channels(Ys, [snr] * G, serving)
    return rate, rate_k, Ys, serving


def mu_tolerance(Ys, snr, serving, second):
    """(tol [n], tol_k [n, K]) of the module docstring; `second` [G, n]"""
    G = len(Ys)
    _, tol_k = CR.cell_rate_tolerance(Ys, [snr] * G, serving)
    A, N, _ = CR._split(Ys, [snr] * G, serving)
    Ai, Ni = np.linalg.inv(A), np.linalg.inv(N)
    a_f, d_f = np.linalg.norm(Ai, axis=(-2, -1)), np.linalg.norm(Ai - Ni, axis=(-2, -1))
    for j, Y in enumerate(Ys):
        m_rx = Y.shape[1]
        y_f = np.sqrt((np.abs(Y) ** 2).sum(axis=(1, 2)))                                    # [n, K]
        r = (np.sqrt(m_rx) * second[j])[:, None]
        tol_k = tol_k + np.where((np.asarray(serving) == j)[:, None], a_f, d_f) * float(snr) * 2 * y_f * r / LN2
    return tol_k.mean(axis=1), tol_k


def mu_reference(rays, params, F, beams, groups, snr_db, bs_fov=None, ue_fov=None, H=None):
    """dict(rate, rate_k, tol, tol_k, partners, stream_snr, stream_tol, idx, size) of a `compute_mu_rate` call"""
    n = rays["power"].shape[0]
    snr = 10.0 ** (snr_db / 10.0)
    H = oracle_channels(rays, params, bs_fov, ue_fov) if H is None else H
    idx, size = link_table(beams, groups, n)
    G = len(idx)
    rate, rate_k, Ys, serving = mu_rate(H, F, idx, size, snr)
    prep = R.prepared(rays, params, bs_fov, ue_fov)
    scale = split_scale(size, G)
    tol, tol_k = mu_tolerance(Ys, snr, serving, rounding_term(rays, prep, params, F, idx, scale))
    a, rel = _moduli(rays, prep, params, F, idx, scale)
    delta = TOL_REL * a.max(axis=2) + (a * rel).max(axis=2)
    stream = snr * (a * a).sum(axis=2)
    stream_tol = snr * (2 * delta * a.sum(axis=2) + a.shape[2] * delta ** 2) + 40 * 2.0 ** -24 * stream
    return dict(rate=rate, rate_k=rate_k, tol=tol, tol_k=tol_k, partners=partners_of(groups, n)[0], stream_snr=stream.T,
                stream_tol=stream_tol.T, idx=idx, size=size, H=H)


def worst(got, want, tol, what=""):
    """worst |got - want| / tol over the entries with tol > 0; where tol is 0 the two are equal"""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(tol, np.float64)
    assert got.shape == want.shape == tol.shape, f"{what}: shapes {got.shape}, {want.shape}, {tol.shape}"
    assert np.isfinite(got).all(), f"{what}: not finite"
    zero = tol == 0
    assert np.all(got[zero] == want[zero]), f"{what}: differs where the tolerance is 0"
    ratio = float((np.abs(got - want)[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: worst error / tolerance {ratio:.3f}")
    return ratio
