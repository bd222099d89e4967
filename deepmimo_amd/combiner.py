"""Host-side helpers of UE receive combining (extension; DESIGN.md "UE receive combining"): the response of a combiner
row to a path, and the power and phase of the path a single-antenna UE would see behind that combiner.

With H[r, t, k] = sum_l c_l a_rx[r, l] a_tx[t, l] g[l, k] and a combiner row w_q,

    (w_q H)[t, k] = sum_l (c_l e[q, l]) a_tx[t, l] g[l, k],      e[q, l] = sum_r W[q, r] a_rx[r, l]

which is the channel of a 1 x 1 UE whose path l has its complex gain multiplied by e[q, l].  ``power`` (dB) and ``phase``
(degrees) are inputs of every entry point of the library, so nothing here is a kernel: as in doppler.py the functions take
the ray matrices where they live - NumPy arrays on the host, torch tensors in HBM - and evaluate in float64 there, rounding
to the float32 the ray matrices are stored in once at the end."""
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
