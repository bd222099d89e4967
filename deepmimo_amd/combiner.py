"""Host-side helpers of UE receive combining and of transmit precoding (extensions; DESIGN.md "UE receive combining" and
"Transmit precoding and multi-user rates"): the response of a combiner or precoder row to a path, and the power and phase
of the path a single-antenna terminal would see behind it.

With H[r, t, k] = sum_l c_l a_rx[r, l] a_tx[t, l] g[l, k] and a combiner row w_q,

    (w_q H)[t, k] = sum_l (c_l e[q, l]) a_tx[t, l] g[l, k],      e[q, l] = sum_r W[q, r] a_rx[r, l]

which is the channel of a 1 x 1 UE whose path l has its complex gain multiplied by e[q, l].  ``power`` (dB) and ``phase``
(degrees) are inputs of every entry point of the library, so nothing here is a kernel: as in doppler.py the functions take
the ray matrices where they live - NumPy arrays on the host, torch tensors in HBM - and evaluate in float64 there, rounding
to the float32 the ray matrices are stored in once at the end.

The transmit side is the mirror image: for a precoder row f, sum_t f[t] H[r, t, k] = sum_l (c_l e_l) a_rx[r, l] g[l, k] with
e_l = sum_t f[t] a_tx[t, l] - the channel from a single-antenna base station.  `combiner_response` serves a shared codebook
[B, M_tx] as it is; `precoder_response` is the per-user form, the row of each user chosen by an index array, and
`precode_rays` the ray matrices behind it; `mu_partners` turns scheduling groups into the per-user tables of
`Dataset.compute_mu_rate`."""
from __future__ import annotations

import numpy as np

from .doppler import _f64, _is_tensor, _xp, wrap_degrees

E2_FLOOR = 2.0 ** -100               # |e|^2 of a path the combiner nulls: it stays a path, about 301 dB down


def check_rx_codebook(who: str, codebook, ue_shape) -> np.ndarray:
    """The UE combining codebook of a call as complex128 [Q, M_rx], Q >= 1: ``"dft"`` is ``dm.dft_codebook(ue_shape)``, an
    array [Q, M_rx] of finite values is taken as given; anything else is a ValueError under `who`."""
    from .geometry import dft_codebook
    m_rx = int(ue_shape[0]) * int(ue_shape[1])
    what = f"{who}: the UE codebook must be 'dft' or a finite array [Q, {m_rx}] with Q >= 1"
    if isinstance(codebook, str):
        if codebook != "dft":
            raise ValueError(f"{what}, got {codebook!r}")
        return dft_codebook(ue_shape).astype(np.complex128)
    if codebook is None or isinstance(codebook, (bool, int, float, complex)):
        raise ValueError(f"{what}, got {codebook!r}")
    try:
        W = np.asarray(codebook.detach().cpu().numpy() if _is_tensor(codebook) else codebook).astype(np.complex128)
    except (TypeError, ValueError):
        raise ValueError(f"{what}, got {codebook!r}") from None
    if W.ndim != 2 or W.shape[1] != m_rx or W.shape[0] < 1:
        raise ValueError(f"{what}, got shape {W.shape}")
    if not np.all(np.isfinite(W)):
        raise ValueError(f"{what}, got a value that is not finite")
    return W


def combiner_response(W, shape, spacing: float, theta, phi):
    """e[u, q, l] = sum_r W[q, r] exp(j 2 pi spacing (y_r sin theta sin phi + z_r cos theta)), complex128 [n_ue, Q, L]:
    the rows of `W` (complex [Q, M_rx], applied without a conjugate, as ``codebook @ H`` applies a BS codebook) on the
    response of an [Mh, Mv] panel, element r = y + Mh z, to the arrival angles `theta` (zenith) and `phi` (azimuth) in
    radians, float64 [n_ue, L] - the formula of ``Dataset.array_response_product``.  NaN where `theta` is NaN.  NumPy
    angles give a NumPy array, torch angles a tensor on their device."""
    from .geometry import _ant_indices
    xp = _xp(theta)
    W = np.asarray(W, dtype=np.complex128)
    th, ph = _f64(theta), _f64(phi)
    kd = 2 * np.pi * float(spacing)
    gy, gz = kd * (xp.sin(th) * xp.sin(ph)), kd * xp.cos(th)
    nan = xp.isnan(th)
    e_re = e_im = None
    for r, (_, y, z) in enumerate(_ant_indices(shape).tolist()):
        arg = (y * gy + z * gz)[:, None, :]
        co, si = xp.cos(arg), xp.sin(arg)
        if xp is np:
            w_re, w_im = W[None, :, r, None].real, W[None, :, r, None].imag
        else:
            w_re = xp.as_tensor(W[:, r].real.copy(), device=th.device)[None, :, None]
            w_im = xp.as_tensor(W[:, r].imag.copy(), device=th.device)[None, :, None]
        t_re, t_im = w_re * co - w_im * si, w_re * si + w_im * co
        e_re, e_im = (t_re, t_im) if e_re is None else (e_re + t_re, e_im + t_im)
    if xp is np:
        e = e_re + 1j * e_im
        e[np.broadcast_to(nan[:, None, :], e.shape)] = np.nan
        return e
    hole = nan[:, None, :].expand_as(e_re)
    return xp.complex(e_re.masked_fill(hole, float("nan")), e_im.masked_fill(hole, float("nan")))


def combine_rays(power, phase, e_q):
    """(power', phase') of the paths behind a combiner, float32, for the stored ``power`` (dB) and ``phase`` (degrees) and the
    responses `e_q` (complex128) of one or more combiner rows, the three broadcast against each other:

        power' = power + 10 log10(max(|e|^2, 2^-100))
        phase' = wrap(phase + degrees(arg e)) into [-180, 180)

    in float64, rounded to float32 once.  Where e == 1 exactly the stored values are kept bit for bit; NaN stays NaN.  The
    floor keeps a path the combiner nulls finite, about 301 dB down - far below the float32 resolution of any sum it is part
    of - so it stays a path.  NumPy in, NumPy out; torch in, torch out on the same device."""
    xp = _xp(power)
    if xp is np:
        e = np.asarray(e_q, dtype=np.complex128)
        e_re, e_im = e.real, e.imag
        stored = np.asarray(power, dtype=np.float32), np.asarray(phase, dtype=np.float32)
        f32 = lambda v: v.astype(np.float32)                                               # noqa: E731
    else:
        e_re, e_im = e_q.real, e_q.imag
        stored = power.float(), phase.float()
        f32 = lambda v: v.float()                                                          # noqa: E731
    same = (e_re == 1.0) & (e_im == 0.0)
    m2 = e_re * e_re + e_im * e_im
    m2 = xp.where(m2 < E2_FLOOR, E2_FLOOR, m2)                                             # NaN compares False and stays
    p = _f64(power) + 10.0 * xp.log10(m2)
    x = wrap_degrees(_f64(phase) + xp.rad2deg(xp.arctan2(e_im, e_re)))
    return tuple(xp.where(same, s, f32(v)) for s, v in zip(stored, (p, x)))


def combine_all(power, phase, W, shape, spacing: float, theta, phi):
    """The ray matrices of the Q * n_ue single-antenna users behind the Q rows of `W`, combiner-major - row q * n_ue + u is
    user u behind row q - as float32 (power', phase') [Q * n_ue, L]: ``combine_rays`` with ``combiner_response``.  A path
    whose arrival angle is NaN - it is not there, or the field of view masks it - has no response and keeps its stored
    power and phase: stage 1 masks it again from the unchanged angles, and a time-domain slot stays where it was."""
    xp = _xp(power)
    e = combiner_response(W, shape, spacing, theta, phi)
    e = xp.swapaxes(xp.where(xp.isnan(e.real), 1.0, e), 0, 1)
    p, x = combine_rays(power[None], phase[None], e)
    return p.reshape(-1, p.shape[-1]), x.reshape(-1, x.shape[-1])


# ---------------------------------------------------------------------------------------------- transmit precoding
def check_tx_codebook(who: str, codebook, bs_shape) -> np.ndarray:
    """The BS precoding codebook of a call as complex128 [B, M_tx], B >= 1, by the rules of `check_rx_codebook`: ``"dft"`` is
    ``dm.dft_codebook(bs_shape)``, an array [B, M_tx] of finite values is taken as given; anything else is a ValueError
    under `who`."""
    try:
        return check_rx_codebook(who, codebook, bs_shape)
    except ValueError as err:
        m_tx = int(bs_shape[0]) * int(bs_shape[1])
        raise ValueError(str(err).replace(f"the UE codebook must be 'dft' or a finite array [Q, {m_tx}] with Q >= 1",
                                          f"the BS codebook must be 'dft' or a finite array [B, {m_tx}] with B >= 1")) from None


def check_tx_beams(who: str, beams, n_ue: int, n_beams: int, ndim=(1, 2)) -> np.ndarray:
    """The `beams` argument of the transmit-precoding calls as int64 [J, n_ue]: an integer array [n_ue] (J = 1) or
    [J, n_ue], J >= 1 - an [n_ue] one only when `ndim` is (1,) - with values in -1 .. n_beams - 1; anything else is a
    ValueError under `who`."""
    shapes = " or ".join(f"[{n_ue}]" if d == 1 else f"[J, {n_ue}]" for d in ndim)
    what = f"{who}: beams must be an integer array of shape {shapes} with values in -1 .. {n_beams - 1}"
    if beams is None or isinstance(beams, (bool, str)):
        raise ValueError(f"{what}, got {beams!r}")
    try:
        b = np.asarray(beams.detach().cpu().numpy() if _is_tensor(beams) else beams)
    except (TypeError, ValueError):
        raise ValueError(f"{what}, got {beams!r}") from None
    if b.dtype.kind not in "iu" or b.ndim not in ndim or b.shape[-1] != n_ue or b.size == 0 and n_ue > 0:
        raise ValueError(f"{what}, got {b.dtype} of shape {b.shape}")
    b = b.astype(np.int64).reshape(-1, n_ue)
    if b.size and (b.min() < -1 or b.max() >= n_beams):
        raise ValueError(f"{what}, got {int(b.min() if b.min() < -1 else b.max())}")
    return b


def precoder_response(F, idx, shape, spacing: float, theta, phi):
    """e[j, u, l] = sum_t F[idx[j, u], t] exp(j 2 pi spacing (y_t sin theta sin phi + z_t cos theta)), complex128
    [J, n_ue, L]: the precoder row each user is served with - `idx` int [J, n_ue] (or [n_ue], J = 1) into the rows of `F`
    (complex [B, M_tx], applied without a conjugate) - on the response of an [Mh, Mv] panel, element t = y + Mh z, to the
    departure angles `theta` (zenith) and `phi` (azimuth) in radians, float64 [n_ue, L].  ``idx = -1`` is no transmission:
    e = 0.  NaN where `theta` is NaN.  Accumulated over the elements in float64 with the weight gathered per element
    ([J, n_ue]); no [n_ue, B, L] table is built.  NumPy angles give a NumPy array, torch angles a tensor on their device.
    ``combiner_response(F, ...)[u, idx[j, u], l]`` is the same number from the shared-codebook form."""
    from .geometry import _ant_indices
    xp = _xp(theta)
    F = np.asarray(F, dtype=np.complex128)
    idx = np.asarray(idx.detach().cpu().numpy() if _is_tensor(idx) else idx).astype(np.int64)
    idx = idx.reshape(-1, idx.shape[-1])
    off = idx < 0
    rows = np.where(off, 0, idx)
    th, ph = _f64(theta), _f64(phi)
    kd = 2 * np.pi * float(spacing)
    gy, gz = kd * (xp.sin(th) * xp.sin(ph)), kd * xp.cos(th)
    nan = xp.isnan(th)
    e_re = e_im = None
    for t, (_, y, z) in enumerate(_ant_indices(shape).tolist()):
        arg = (y * gy + z * gz)[None, :, :]
        co, si = xp.cos(arg), xp.sin(arg)
        w = np.where(off, 0.0, F[rows, t])                                                 # [J, n_ue]
        if xp is np:
            w_re, w_im = w.real[:, :, None], w.imag[:, :, None]
        else:
            w_re = xp.as_tensor(w.real.copy(), device=th.device)[:, :, None]
            w_im = xp.as_tensor(w.imag.copy(), device=th.device)[:, :, None]
        t_re, t_im = w_re * co - w_im * si, w_re * si + w_im * co
        e_re, e_im = (t_re, t_im) if e_re is None else (e_re + t_re, e_im + t_im)
    if xp is np:
        e = e_re + 1j * e_im
        e[np.broadcast_to(nan[None], e.shape)] = np.nan
        return e
    hole = nan[None].expand_as(e_re)
    return xp.complex(e_re.masked_fill(hole, float("nan")), e_im.masked_fill(hole, float("nan")))


def precode_rays(power, phase, F, idx, shape, spacing: float, theta, phi, scale=None):
    """The ray matrices of the J * n_ue users behind the precoder rows `idx` [J, n_ue] of `F`, row j * n_ue + u user u behind
    ``F[idx[j, u]]``, as float32 (power', phase') [J * n_ue, L]: ``combine_rays`` with ``precoder_response``.  `scale`: an
    optional real [J, n_ue] (NumPy) that multiplies e before it - the amplitude of a power split - so it passes through the
    one float32 rounding together with e.  A row with ``idx = -1`` does not transmit: every entry of its power is NaN -
    what stage 1 takes for an absent path - and its phase is the stored one.  A path whose departure angle is NaN - it is
    not there, or the field of view masks it - has no response and keeps its stored power and phase, as in
    ``combine_all``."""
    xp = _xp(power)
    idx = np.asarray(idx.detach().cpu().numpy() if _is_tensor(idx) else idx).astype(np.int64)
    idx = idx.reshape(-1, idx.shape[-1])
    e = precoder_response(F, idx, shape, spacing, theta, phi)
    off = idx < 0
    if scale is not None:
        s = np.where(off, 1.0, np.asarray(scale, dtype=np.float64).reshape(idx.shape))
        e = e * (s[:, :, None] if xp is np else xp.as_tensor(s, device=e.device)[:, :, None])
    e = xp.where(xp.isnan(e.real), 1.0, e)
    p, x = combine_rays(power[None], phase[None], e)
    if off.any():
        gone = off[:, :, None] if xp is np else xp.as_tensor(off, device=p.device)[:, :, None]
        p = xp.where(gone, xp.full_like(p, float("nan")), p)
        x = xp.where(gone, (np.asarray(phase, dtype=np.float32) if xp is np else phase.float())[None], x)
    return p.reshape(-1, p.shape[-1]), x.reshape(-1, x.shape[-1])


def mu_partners(groups, n_ue: int, who: str = "mu_partners"):
    """The per-user tables of scheduling groups: `groups` int [n_groups, G], 1 <= G <= 8, the users served together, a row
    padded with -1, every user in at most one place.  Returns (partners int32 [n_ue, G - 1]: the other members of the
    user's group in the order of the group's row, padded with -1; group_size int32 [n_ue]: members of the user's group, 0
    for a user in no group; scheduled bool [n_ue]).  Pure NumPy; anything else is a ValueError under `who`."""
    what = f"{who}: groups must be an integer array [n_groups, G], 1 <= G <= 8, of user indices in -1 .. {int(n_ue) - 1}"
    if groups is None or isinstance(groups, (bool, str)):
        raise ValueError(f"{what}, got {groups!r}")
    try:
        g = np.asarray(groups.detach().cpu().numpy() if _is_tensor(groups) else groups)
    except (TypeError, ValueError):
        raise ValueError(f"{what}, got {groups!r}") from None
    if g.dtype.kind not in "iu" or g.ndim != 2 or not 1 <= g.shape[1] <= 8:
        raise ValueError(f"{what}, got {g.dtype} of shape {g.shape}")
    g = g.astype(np.int64)
    if g.size and (g.min() < -1 or g.max() >= n_ue):
        raise ValueError(f"{what}, got {int(g.min() if g.min() < -1 else g.max())}")
    members = g[g >= 0]
    seen, counts = np.unique(members, return_counts=True)
    if (counts > 1).any():
        raise ValueError(f"{who}: user {int(seen[counts > 1][0])} appears more than once in groups")
    G = g.shape[1]
    partners = np.full((int(n_ue), G - 1), -1, np.int32)
    group_size = np.zeros(int(n_ue), np.int32)
    at = g >= 0
    group_size[g[at]] = np.broadcast_to(at.sum(axis=1)[:, None], g.shape)[at]
    if G > 1:
        cols = np.array([[b for b in range(G) if b != a] for a in range(G)])               # [G, G - 1]: the row without a
        others = g[:, cols]                                                                # [n_groups, G, G - 1]
        others = np.take_along_axis(others, np.argsort(others < 0, axis=2, kind="stable"), axis=2)
        partners[g[at]] = others[at]
    return partners, group_size, group_size > 0
