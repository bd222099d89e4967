"""Host-side helpers of the channel time series (extension; DESIGN.md "Channel time series"): the per-path Doppler
velocity a pair of terminal velocities gives, and the phase matrix of a snapshot at time t.

A snapshot only turns each path's phase, and ``phase`` is an input of every entry point of the library, so nothing here
is a kernel: the functions take the ray matrices where they live - NumPy arrays on the host, torch tensors in HBM - and
evaluate in float64 there, rounding to the float32 the ray matrices are stored in once at the end."""
from __future__ import annotations

import numpy as np

LIGHTSPEED = 299792458.0            # the constant of the kernels' own Doppler term (csrc/k1_path_math.h)
_HOST_CHUNK_ELEMS = 1 << 20         # elements of the float64 temporaries of `advance_phase` on the host (8 MiB each)


def _is_tensor(v) -> bool:
    return hasattr(v, "detach")


def _f64(v):
    return v.double() if _is_tensor(v) else np.asarray(v, dtype=np.float64)


def check_times(who: str, times):
    """(`times` as a float64 array [T], whether it was given as a scalar): finite seconds, T >= 1, at most 1-D; anything
    else is a ValueError under `who`."""
    try:
        t = np.asarray(times.detach().cpu().numpy() if _is_tensor(times) else times, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: times must be a scalar or a 1-D array of seconds, got {times!r}") from None
    if t.ndim > 1:
        raise ValueError(f"{who}: times must be a scalar or a 1-D array of seconds, got shape {t.shape}")
    scalar = t.ndim == 0
    t = t.reshape(-1)
    if t.size == 0:
        raise ValueError(f"{who}: times is empty, a series needs at least one snapshot")
    if not np.all(np.isfinite(t)):
        raise ValueError(f"{who}: times must be finite seconds, got {t[~np.isfinite(t)][0]}")
    return t, scalar


def check_velocity(who: str, name: str, vel, n_ue=None) -> np.ndarray:
    """A velocity argument of `set_velocities` as float64 [3] (`n_ue` None) or [n_ue, 3]: None is 0, a [3] vector holds
    for every user."""
    rows = () if n_ue is None else (int(n_ue),)
    if vel is None:
        return np.zeros(rows + (3,))
    v = np.asarray(vel.detach().cpu().numpy() if _is_tensor(vel) else vel, dtype=np.float64)
    if v.shape == (3,):
        v = np.broadcast_to(v, rows + (3,)).copy()
    if v.shape != rows + (3,) or not np.all(np.isfinite(v)):
        takes = "[3]" if n_ue is None else f"[3] or [{int(n_ue)}, 3]"
        raise ValueError(f"{who}: {name} must be finite m/s of shape {takes} (global x, y, z), got shape {np.shape(vel)}")
    return v


def direction(az_deg, el_deg):
    """The three components of k(phi, theta) = (sin theta cos phi, sin theta sin phi, cos theta) in float64, for an azimuth
    phi and a zenith angle theta in degrees: the vector the array response multiplies an element position with
    (exp(+j k p . k))."""
    xp = _xp(az_deg)
    phi, theta = xp.deg2rad(_f64(az_deg)), xp.deg2rad(_f64(el_deg))
    st = xp.sin(theta)
    return st * xp.cos(phi), st * xp.sin(phi), xp.cos(theta)


def _xp(v):
    if _is_tensor(v):
        import torch
        return torch
    return np


def doppler_velocity(aoa_az, aoa_el, aod_az, aod_el, rx_vel: np.ndarray, tx_vel: np.ndarray):
    """``-(rx_vel[u] . k(aoa) + tx_vel . k(aod))`` per path, float32 [n_ue, n_paths], NaN where the path is NaN.  The angles
    are the stored, unrotated ones in degrees (NumPy or torch: the result lives where they live); rx_vel float64
    [n_ue, 3], tx_vel float64 [3]."""
    if _is_tensor(aoa_az):
        import torch
        rx = torch.as_tensor(rx_vel, dtype=torch.float64, device=aoa_az.device)
        to_f32 = lambda v: v.float()                                                       # noqa: E731
    else:
        rx = rx_vel
        to_f32 = lambda v: v.astype(np.float32)                                            # noqa: E731
    ax, ay, az = direction(aoa_az, aoa_el)
    dx, dy, dz = direction(aod_az, aod_el)
    along_rx = rx[:, 0:1] * ax + rx[:, 1:2] * ay + rx[:, 2:3] * az
    along_tx = float(tx_vel[0]) * dx + float(tx_vel[1]) * dy + float(tx_vel[2]) * dz
    return to_f32(-(along_rx + along_tx))


def wrap_degrees(x):
    """The float64 degrees `x` (NumPy or torch) wrapped into [-180, 180), in place; returns `x`."""
    xp = _xp(x)
    # x - 360 floor((x + 180) / 360): 360 k and the difference are exact in float64 (|x| stays far below 2^53 / 360),
    # so only the choice of k can be off, by one float64 rounding at a boundary - -180 for +180, the same angle
    k = x + 180.0
    k /= 360.0
    with np.errstate(invalid="ignore"):                                                    # NaN paths stay NaN, silently
        xp.floor(k, out=k)
    k *= 360.0
    x -= k
    return x


def advance_phase(phase, vel, acc, times: np.ndarray, carrier_freq: float):
    """The phase matrices of the snapshots at `times` (float64 [T], seconds), time-major float32 [T * n_ue, n_paths]:

        delta = -360 (f_c / c) (v t + a t^2 / 2)           degrees, float64
        phase[t] = wrap(phase + delta) into [-180, 180), rounded to float32 once

    Where delta == 0 (t = 0, or v = a = 0) the stored phase is kept bit for bit; NaN stays NaN.  `acc` None counts as
    zeros.  NumPy in, NumPy out; torch in, torch out on the same device."""
    xp = _xp(phase)
    scale = -360.0 * (float(carrier_freq) / LIGHTSPEED)
    if xp is np:
        t = np.asarray(times, dtype=np.float64)[:, None, None]
        stored = np.asarray(phase, dtype=np.float32)[None]
        f32 = lambda v: v.astype(np.float32)                                               # noqa: E731
    else:
        t = xp.as_tensor(np.asarray(times, dtype=np.float64), device=phase.device)[:, None, None]
        stored = phase.float()[None]
        f32 = lambda v: v.float()                                                          # noqa: E731
    v64, p64 = _f64(vel)[None], _f64(phase)[None]
    half_a = None if acc is None else (0.5 * _f64(acc))[None]
    T, per_snapshot = int(t.shape[0]), max(1, int(np.prod(stored.shape)))
    # On the host the passes over the float64 temporaries are the cost of a view: a few snapshots at a time keep them in
    # the caches.  On the device one pass over all snapshots saves launches.
    step = max(1, _HOST_CHUNK_ELEMS // per_snapshot) if xp is np else T
    out = np.empty((T,) + tuple(stored.shape[1:]), dtype=np.float32) if xp is np else None
    for b in range(0, T, step):
        tb = t[b:b + step]
        x = v64 * tb
        if half_a is not None:
            x += half_a * (tb * tb)
        x *= scale
        still = x == 0
        x += p64
        wrap_degrees(x)
        if out is None:                                                                    # the device: all snapshots at once
            out = xp.where(still, stored, f32(x))
        else:
            o = out[b:b + step]
            np.copyto(o, x, casting="same_kind")                                           # the one rounding to float32
            np.copyto(o, np.broadcast_to(stored, o.shape), where=still)
    return out.reshape(-1, out.shape[-1])
