"""References of the time-series tests (tests/test_time_series_cpu.py, tests/test_gpu_time_series.py), restated in NumPy
float64 without a line of the package: the direction vector of a pair of stored angles, the per-path Doppler velocity of
a pair of terminal velocities, the phase of a snapshot as an UNWRAPPED float64 sum, and the channels of a series from the
NumPy oracle on those phases.  A plain module: NumPy only, no torch, no GPU.

    k(phi, theta)     = (sin theta cos phi, sin theta sin phi, cos theta)             theta: the zenith angle
    doppler_vel[u, l] = -(rx_vel[u] . k(aoa) + tx_vel . k(aod))
    phase[t, u, l]    = phase[u, l] - 360 (f_c / c) (v t + a t^2 / 2)                 degrees

Tolerance of a channel against `reference_channels`, per snapshot and user (derived, not chosen):

    TOL_REL max|H_ref[t, u]|  +  2 pi 2^-24 sum_l |c_l|

the project's parity criterion (tests/_cases.py) plus the float32 rounding of the advanced phase - at most half a float32
ulp below 180 degrees, pi 2^-24 rad, on a path of modulus |c_l| - doubled for the complex64 rounding of the oracle's own
output.  |c_l| = sqrt(power_linear_ant_gain / N) in the frequency domain (sqrt(power_linear_ant_gain) in the time domain,
where a tap holds one path) from `oracle_np.prepare_paths`, over the paths the call keeps."""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL

LIGHTSPEED = 299792458.0
PHASE_ULP_DEG = 180.0 * 2.0 ** -23           # one float32 ulp at the top of [-180, 180)


def k_hat(az_deg, el_deg):
    """[..., 3] float64 direction of (azimuth, zenith) in degrees"""
    phi, theta = np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(np.asarray(el_deg, np.float64))
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=-1)


def doppler_vel(rays, rx_vel=None, tx_vel=None):
    """float64 [n, L]; rx_vel [3] or [n, 3], tx_vel [3], None = 0"""
    n = rays["aoa_az"].shape[0]
    rx = np.broadcast_to(np.zeros(3) if rx_vel is None else np.asarray(rx_vel, np.float64), (n, 3))
    tx = np.zeros(3) if tx_vel is None else np.asarray(tx_vel, np.float64)
    return -(np.einsum("uc,ulc->ul", rx, k_hat(rays["aoa_az"], rays["aoa_el"])) + k_hat(rays["aod_az"], rays["aod_el"]) @ tx)


def advanced_phase(phase, vel, acc, times, fc):
    """float64 [T, n, L], unwrapped; acc None = 0"""
    t = np.asarray(times, np.float64).reshape(-1, 1, 1)
    v = np.asarray(vel, np.float64)[None]
    a = np.zeros_like(v) if acc is None else np.asarray(acc, np.float64)[None]
    return np.asarray(phase, np.float64)[None] - 360.0 * fc / LIGHTSPEED * (v * t + 0.5 * a * t * t)


def wrap_deg(d):
    """a difference of angles in degrees, into [-180, 180)"""
    return np.remainder(np.asarray(d, np.float64) + 180.0, 360.0) - 180.0


def _snapshot_rays(rays, phase64):
    out = {k: v for k, v in rays.items()}
    out["phase"] = phase64
    return out


def reference_channels(rays, oracle_params, times, fc, bs_fov=None, ue_fov=None, doppler_fc=None):
    """complex64 [T, n, M_rx, M_tx, K or P] from `oracle_np.compute_channels` on the unwrapped float64 phases.  `rays`
    carries doppler_vel (and doppler_acc).  `doppler_fc`: the carrier frequency of the v3 term when
    oracle_params['enable_doppler'] is set."""
    from oracle import oracle_np as onp
    ph = advanced_phase(rays["phase"], rays["doppler_vel"], rays.get("doppler_acc"), times, fc)
    dop = None
    if oracle_params["enable_doppler"]:
        dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=doppler_fc)
    return np.stack([onp.compute_channels(_snapshot_rays(rays, ph[i]), oracle_params, bs_fov, ue_fov, doppler=dop)["channel"]
                     for i in range(ph.shape[0])])


def path_moduli_sum(rays, oracle_params, bs_fov=None, ue_fov=None):
    """[n] sum over the kept paths of |c_l| (module docstring)"""
    from oracle import oracle_np as onp
    np.random.seed(1001)
    prep = onp.prepare_paths(rays, oracle_params, bs_fov, ue_fov)
    P = int(oracle_params["num_paths"])
    g = np.asarray(prep["_power_linear_ant_gain"], np.float64)[:, :P]
    g = np.where(np.isnan(prep["_aod_el_rot_fov"][:, :P]), np.nan, g)            # a path the field of view masks adds nothing
    if oracle_params["freq_domain"]:
        g = g / oracle_params["ofdm"]["subcarriers"]
    return np.nansum(np.sqrt(g), axis=1)


def channel_tolerance(H_ref, moduli_sum, factor=1.0):
    """[T, n] bound of the module docstring for H_ref [T, n, ...] and `path_moduli_sum`"""
    H_ref = np.asarray(H_ref)
    peak = np.abs(H_ref.astype(np.complex128)).reshape(H_ref.shape[0], H_ref.shape[1], -1).max(axis=2)
    return factor * (TOL_REL * peak + 2 * np.pi * 2.0 ** -24 * np.asarray(moduli_sum)[None, :])


def assert_series_close(H, H_ref, moduli_sum, what=""):
    """every entry of H [T, n, ...] within `channel_tolerance` of H_ref; returns the worst error / bound"""
    H, H_ref = np.asarray(H), np.asarray(H_ref)
    assert H.shape == H_ref.shape, f"{what}: shape {H.shape} vs {H_ref.shape}"
    assert H.dtype == np.complex64, f"{what}: dtype {H.dtype}"
    assert np.isfinite(H.astype(np.complex128)).all() and np.isfinite(H_ref.astype(np.complex128)).all(), f"{what}: not finite"
    d = np.abs(H.astype(np.complex128) - H_ref.astype(np.complex128)).reshape(H.shape[0], H.shape[1], -1).max(axis=2)
    tol = channel_tolerance(H_ref, moduli_sum)
    zero = tol == 0
    assert np.all(d[zero] == 0), f"{what}: a user without a path is not zero"
    ratio = float((d[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst error / bound {ratio:.3f}"
    return ratio
