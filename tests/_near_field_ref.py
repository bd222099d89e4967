"""Reference of the near-field tests (tests/test_near_field_cpu.py, tests/test_gpu_near_field*.py): the spherical-wavefront
array response of include/deepmimo_amd.h, DMX_FLAG_NEAR_FIELD, in NumPy complex128.  A plain module: NumPy and the oracle only,
nothing of deepmimo_amd.

    R_l     = tau_l f_c                                  path length in wavelengths, from the float64 value of the stored delay
    q[e,l]  = y_e d sin(th_l) sin(ph_l) + z_e d cos(th_l)        the plane-wave phase, revolutions, element e = y + Mh z
    s[e]    = d^2 (y_e^2 + z_e^2)
    psi     = R - sqrt(R^2 - 2 R q + s) = (2 R q - s) / (R + sqrt(R^2 - 2 R q + s)),   0 where 2 R q = s
    H_nf[u, r, t, k] = sum_l c_l exp(j 2pi (psi_rx[r,l] + psi_tx[t,l])) exp(-j 2pi dn_l sc_k / N)

Everything per path is the oracle's, exactly as in tests/_wideband_ref.py (whose `element_phase` gives q): `prepare_paths`
gives the rotated, FoV-masked angles, the powers with the pattern gains and so the kept paths; `ofdm_path_gains` gives
c_l exp(-j 2pi dn_l sc_k / N) with the clip at dn >= N and the Doppler term.  `far_field_channels` is the twin with psi = q.

`near_field_tolerance` is the project's criterion per user, TOL_REL max|H_ref[u]|, plus what the record's float32 delay can
move: the kernels take R from dn = float32(tau B), one rounding away from the float64 tau, so R is off by at most
2^-24 R (twice that is taken), which moves psi of an element by |psi(R (1 + 2^-23)) - psi(R)| and a path's term by at most
2 pi |c_l| (max over rx elements + max over tx elements) of it."""
from __future__ import annotations

import copy

import numpy as np

from oracle import oracle_np as onp
from tests._cases import TOL_REL
from tests._wideband_ref import element_phase, narrowband_channels as far_field_channels  # noqa: F401  (the twin)


def psi(q, s, R):
    """psi of the module docstring, float64, broadcast over q [..., M, L], s [M, 1] and R [..., 1, L]"""
    q, s, R = np.broadcast_arrays(np.asarray(q, np.float64), np.asarray(s, np.float64), np.asarray(R, np.float64))
    num = 2.0 * R * q - s
    den = R + np.sqrt(np.maximum(R * R - num, 0.0))
    return np.where(num == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))


def element_s(shape, spacing):
    """s [M, 1] = d^2 (y^2 + z^2)"""
    idx = onp.ant_indices(shape).astype(np.float64)
    return (float(spacing) ** 2 * (idx[:, 1] ** 2 + idx[:, 2] ** 2))[:, None]


def _paths(rays, params, bs_fov, ue_fov, doppler, users):
    """per user: (path gains [L', K] complex128, q_rx [M_rx, L'], q_tx [M_tx, L'], delay [L'] float64 seconds) of the paths
    that enter the sum - the extraction of tests/_wideband_ref.py with the delays kept"""
    params = copy.deepcopy(params)
    np.random.seed(1001)
    prep = onp.prepare_paths(rays, params, bs_fov, ue_fov)
    P = int(params["num_paths"])
    bs, ue, ofdm = params["bs_antenna"], params["ue_antenna"], params["ofdm"]
    sel = slice(None) if users is None else users
    q_tx = element_phase(bs["shape"], bs["spacing"], prep["_aod_el_rot_fov"][sel], prep["_aod_az_rot_fov"][sel])[..., :P]
    q_rx = element_phase(ue["shape"], ue["spacing"], prep["_aoa_el_rot_fov"][sel], prep["_aoa_az_rot_fov"][sel])[..., :P]
    power = prep["_power_linear_ant_gain"][sel][..., :P]
    delay, phase = rays["delay"][sel][..., :P], rays["phase"][sel][..., :P]
    use_dop = bool(params["enable_doppler"]) and doppler is not None
    out = []
    for i in range(power.shape[0]):
        v = ~np.isnan(power[i])
        if not v.any():
            out.append(None)
            continue
        dop = (doppler["vel"][sel][i, :P][v], doppler["acc"][sel][i, :P][v], doppler["carrier_freq"]) if use_dop else None
        g = onp.ofdm_path_gains(power[i, v], delay[i, v], phase[i, v], ofdm, dop)
        qr, qt = q_rx[i][:, v], q_tx[i][:, v]
        ok = ~(np.isnan(qr).any(axis=0) | np.isnan(qt).any(axis=0) | np.isnan(g).any(axis=1))   # nansum: a NaN path adds 0
        out.append((g[ok].astype(np.complex128), qr[:, ok], qt[:, ok], delay[i, v][ok].astype(np.float64)))
    return out, params


def _user_phases(pth, params, carrier_freq, stretch=1.0):
    """(psi_rx [M_rx, L'], psi_tx [M_tx, L']) of one user's paths with R = tau f_c stretch"""
    _, qr, qt, tau = pth
    R = (tau * float(carrier_freq) * stretch)[None, :]
    bs, ue = params["bs_antenna"], params["ue_antenna"]
    return psi(qr, element_s(ue["shape"], ue["spacing"]), R), psi(qt, element_s(bs["shape"], bs["spacing"]), R)


def near_field_channels(rays, params, carrier_freq, bs_fov=None, ue_fov=None, doppler=None, users=None):
    """complex128 [N, M_rx, M_tx, K] of the module docstring.  Arguments as `oracle_np.compute_channels`; `carrier_freq` in
    Hz is the f_c of R (the Doppler term takes its own from `doppler`)."""
    paths, params = _paths(rays, params, bs_fov, ue_fov, doppler, users)
    m_rx, m_tx = int(np.prod(params["ue_antenna"]["shape"])), int(np.prod(params["bs_antenna"]["shape"]))
    K = len(params["ofdm"]["selected_subcarriers"])
    H = np.zeros((len(paths), m_rx, m_tx, K), dtype=np.complex128)
    for i, pth in enumerate(paths):
        if pth is None:
            continue
        prx, ptx = _user_phases(pth, params, carrier_freq)
        t = np.exp(2j * np.pi * prx)[:, None, :] * np.exp(2j * np.pi * ptx)[None, :, :]
        H[i] = np.einsum("rtl,lk->rtk", t, pth[0])
    return H


def delay_rounding_term(rays, params, carrier_freq, bs_fov=None, ue_fov=None, doppler=None, users=None):
    """float64 [N]: 2 pi sum_l |c_l| (max_r + max_t) |psi(R_l (1 + 2^-23)) - psi(R_l)|, the second term of the tolerance"""
    paths, params = _paths(rays, params, bs_fov, ue_fov, doppler, users)
    out = np.zeros(len(paths))
    for i, pth in enumerate(paths):
        if pth is None:
            continue
        a = _user_phases(pth, params, carrier_freq)
        b = _user_phases(pth, params, carrier_freq, stretch=1.0 + 2.0 ** -23)
        move = np.abs(b[0] - a[0]).max(axis=0) + np.abs(b[1] - a[1]).max(axis=0)
        out[i] = 2 * np.pi * np.sum(np.abs(pth[0]).max(axis=1) * move)
    return out


def near_field_tolerance(H_ref, rays, params, carrier_freq, bs_fov=None, ue_fov=None, doppler=None, users=None):
    """float64 [N]: the largest |H - H_ref[u]| an element of user u may show (module docstring)"""
    peak = np.abs(H_ref).reshape(len(H_ref), -1).max(axis=1)
    return TOL_REL * peak + delay_rounding_term(rays, params, carrier_freq, bs_fov, ue_fov, doppler, users)


def assert_within(H, H_ref, tol, what=""):
    """every element of H within the per-user `tol` of H_ref; users whose reference is all-zero exactly zero.  Returns the
    worst error / tolerance."""
    H = np.asarray(H).astype(np.complex128)
    assert H.shape == H_ref.shape, f"{what}: shape {H.shape} vs {H_ref.shape}"
    assert np.all(np.isfinite(H)), f"{what}: not finite"
    err = np.abs(H - H_ref).reshape(len(H), -1).max(axis=1)
    zero = np.abs(H_ref).reshape(len(H), -1).max(axis=1) == 0
    assert np.all(err[zero] == 0), f"{what}: a user without paths is not all-zero"
    ratio = np.max(err[~zero] / tol[~zero]) if (~zero).any() else 0.0
    assert ratio <= 1.0, f"{what}: worst error is {ratio:.3f} of the tolerance (user {int(np.argmax(np.where(zero, 0, err / np.maximum(tol, 1e-300))))})"
    return float(ratio)
