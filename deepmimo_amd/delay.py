"""Delay-domain helpers for the outputs of ``Dataset.compute_angle_delay`` (extension): the delay every tap sits at and the
delay spread of a power-delay profile.  Pure array code, no kernel: NumPy in gives NumPy out, torch in gives torch out on
its device."""
from __future__ import annotations

import numpy as np

from . import consts as c


def tap_delays(params, n_taps, n_fft=None) -> np.ndarray:
    """The delay in seconds that tap t of ``compute_angle_delay(params, n_taps=n_taps, n_fft=n_fft)`` sits at, float64
    [n_taps].  The selection ``first + k * stride`` samples the band every ``stride * bandwidth / N`` Hz (N =
    ``ofdm.subcarriers``), so an inverse DFT of ``n_fft`` points (None: the number of selected subcarriers) resolves
    ``N / (n_fft * stride * bandwidth)`` seconds per tap:

        delays[t] = t * N / (n_fft * stride * bandwidth)

    A path of delay tau lands on tap ``tau / delays[1]`` modulo ``n_fft`` (a single selected subcarrier counts as stride 1).
    ValueError for a selection that is not uniformly spaced, ``n_taps`` outside 1 .. n_fft or ``n_fft`` below the number of
    selected subcarriers - what ``compute_angle_delay`` refuses."""
    from .engine import uniform_stride
    ofdm = params[c.PARAMSET_OFDM]
    sel = np.asarray(ofdm[c.PARAMSET_OFDM_SC_SAMP]).ravel()
    _, stride = uniform_stride(sel)
    if stride <= 0:
        raise ValueError("tap_delays: ofdm.selected_subcarriers must be uniformly spaced, first + k * stride with stride > 0")
    for name, v in (("n_taps", n_taps),) + ((("n_fft", n_fft),) if n_fft is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"tap_delays: {name} must be an integer, got {v!r}")
    n_fft = int(sel.size) if n_fft is None else int(n_fft)
    if n_fft < sel.size:
        raise ValueError(f"tap_delays: n_fft = {n_fft} is below the {sel.size} selected subcarriers")
    if not 1 <= int(n_taps) <= n_fft:
        raise ValueError(f"tap_delays: n_taps = {n_taps} is outside 1 .. n_fft = {n_fft}")
    n, bw = float(ofdm[c.PARAMSET_OFDM_SC_NUM]), float(ofdm[c.PARAMSET_OFDM_BANDWIDTH])
    if not (np.isfinite(bw) and bw > 0 and n >= 1):
        raise ValueError("tap_delays: ofdm.bandwidth must be finite and > 0 and ofdm.subcarriers >= 1")
    return np.arange(int(n_taps), dtype=np.float64) * n / (n_fft * float(stride) * bw)


def delay_spread(profile, delays):
    """(mean excess delay, RMS delay spread) per user of a power-delay profile: ``profile`` real [..., n_taps], >= 0 (what
    ``compute_angle_delay(output="profile")`` returns), ``delays`` [n_taps] in seconds (``tap_delays``).  In float64,

        mean = sum_t p[t] delays[t] / sum_t p[t]
        rms  = sqrt(sum_t p[t] (delays[t] - mean)**2 / sum_t p[t])

    each of shape ``profile.shape[:-1]``; NaN where the profile is all zero (a user without a path).  The second moment is
    taken about the mean, so nothing is cancelled and rms is exactly 0 for a profile with one occupied tap.  NumPy in gives
    NumPy out; a torch tensor in gives torch tensors on its device."""
    if type(profile).__module__.split(".")[0] == "torch":
        import torch
        p = profile.to(torch.float64)
        d = torch.as_tensor(np.asarray(delays.cpu() if hasattr(delays, "cpu") else delays, dtype=np.float64), device=p.device)
        xp_sqrt, nan = torch.sqrt, float("nan")
        where = lambda m, a: torch.where(m, a, torch.full_like(a, nan))
    else:
        p = np.asarray(profile, dtype=np.float64)
        d = np.asarray(delays, dtype=np.float64)
        xp_sqrt = np.sqrt
        where = lambda m, a: np.where(m, a, np.nan)
    if d.ndim != 1 or p.ndim < 1 or p.shape[-1] != d.shape[0]:
        raise ValueError(f"delay_spread: profile must be [..., n_taps] and delays [n_taps], got {tuple(p.shape)} and {tuple(d.shape)}")
    tot = p.sum(-1)
    some = tot > 0
    w = p / where(some, tot)[..., None]                                        # NaN, not a division by zero; one tap: exactly 1
    mean = (w * d).sum(-1)
    rms = xp_sqrt((w * (d - mean[..., None]) ** 2).sum(-1))
    return mean, rms
