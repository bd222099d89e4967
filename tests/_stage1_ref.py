"""A plain NumPy reference for what stage 1 (k1_path_prep.hip, stage1_path in k1_path_math.h) itself writes: the per-path
side products for all loaded paths and the records of each user's kept paths in slot order.

Dtype flow up to the rotated direction is the reference's, as in oracle_np.rotate_angles_batch: float32 deg2rad, float32
sin / cos of the zenith, float64 for everything that touches the rotation.  The direction is exposed as (zc, re, im) BEFORE
arccos / angle; the angles are arccos(zc) and np.angle(re + 1j * im) exactly as the oracle takes them (so an imaginary part
of -0.0 becomes +0.0 and the azimuth on the branch cut is +pi), the steering steps are evaluated from (zc, re, im) in
np.longdouble.

Decidability.  GPU libm and glibc may differ in the last bits of the float64 sin / cos, and that must not decide a test.
Each of zc, re, im is a sum of products of factors bounded by 1; the kernel's value differs from the one here by at most
eight rounding errors of 2.2e-16 relative to the magnitudes of the terms that are summed, so each component is shifted by
-e, 0, +e (27 combinations) with e = EPS * (sum of the |terms| of that component).  A component whose terms are exact in
any arithmetic (zero tilt: zc is the float32 cosine itself; a factor that is exactly 0) has e = 0, which is what keeps the
poles and the branch cut testable.  arccos / angle of the GPU's libm are allowed ANG_REL relative to the angle (4.5 ulp).
A point is undecidable for a configuration when, under any of these perturbations, a decision changes: NaN-ness of the
zenith (|zc| crossing 1), the field-of-view mask of a restricted side, or "gain is zero" of a dipole side.  The same
perturbation gives each steering step and each rotated angle its tolerance.
"""
from __future__ import annotations

import itertools

import numpy as np

EPS = 2e-15            # eight roundings of 2.2e-16, relative to the summed term magnitudes
ANG_REL = 1e-15        # arccos / atan2 of another libm, relative to the angle
LIGHTSPEED = 299792458.0
C_RTOL = 1e-6          # the project's power_linear rtol, halved by the square root and doubled for the product
_SHIFTS = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))      # [27, 3]


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def rotated_direction(rot_deg, el_deg, az_deg):
    """geometry.py:284-310 up to (cos zenith', re, im), float64 [N, L], and the summed term magnitudes (mz, mr, mi) the
    perturbation is relative to.  rot_deg: [3] or [N, 3] degrees; el / az: float32 [N, L] degrees."""
    rot = np.asarray(rot_deg)
    if rot.ndim == 1:
        rot = rot[None, :]
    rot = np.deg2rad(rot)
    th = np.deg2rad(np.asarray(el_deg, dtype=np.float32))
    ph = np.deg2rad(np.asarray(az_deg, dtype=np.float32))
    rx, ry, rz = rot[:, 0:1], rot[:, 1:2], rot[:, 2:3]
    d = ph - rz
    with np.errstate(invalid="ignore"):
        sd, cd = np.sin(d), np.cos(d)
        sy, cy = np.sin(ry), np.cos(ry)
        sx, cx = np.sin(rx), np.cos(rx)
        st, ct = np.sin(th), np.cos(th)            # float32
        zc = cy * cx * ct + st * (sy * cx * cd - sx * sd)
        re = cy * st * cd - sy * ct
        im = cy * sx * ct + st * (sy * sx * cd + cx * sd)
        first_exact = np.isin(cy * cx, (-1.0, 0.0, 1.0))       # cos zenith times +-1 or 0: no rounding in any arithmetic
        mz = np.where(first_exact, 0.0, np.abs(cy * cx * ct)) + np.abs(st * sy * cx * cd) + np.abs(st * sx * sd)
        mr = np.abs(cy * st * cd) + np.abs(sy * ct)
        mi = np.abs(cy * sx * ct) + np.abs(st * sy * sx * cd) + np.abs(st * cx * sd)
    mag = tuple(np.nan_to_num(m, nan=0.0) * np.ones_like(zc) for m in (mz, mr, mi))
    return zc, re, im, mag


def angles_of(zc, re, im):
    """(zenith', azimuth') = (arccos(zc), np.angle(re + 1j * im)), geometry.py:305-310"""
    with np.errstate(invalid="ignore"):
        return np.arccos(zc), np.angle(re + 1j * im)


def fov_mask(fov_deg, theta, phi):
    """geometry.py:162-195 on rotated radians"""
    with np.errstate(invalid="ignore"):
        th, ph = np.mod(theta, 2 * np.pi), np.mod(phi, 2 * np.pi)
        fov = np.deg2rad(fov_deg)
        az_ok = np.logical_or(ph <= 0 + fov[0] / 2, ph >= 2 * np.pi - fov[0] / 2)
        el_ok = np.logical_and(th <= np.pi / 2 + fov[1] / 2, th >= np.pi / 2 - fov[1] / 2)
        return np.logical_and(az_ok, el_ok)


def is_full_fov(fov):
    return fov[0] >= 360 and fov[1] >= 180


def stored_fovs(bs_fov, ue_fov):
    """(bs_fov, ue_fov, enabled, bs_restricted, ue_restricted) as Dataset.apply_fov stores them (dataset.py:423-504)"""
    if bs_fov is None and ue_fov is None:
        return None, None, False, False, False
    bs = np.array([360, 180]) if bs_fov is None else np.asarray(bs_fov)
    ue = np.array([360, 180]) if ue_fov is None else np.asarray(ue_fov)
    bf, uf = is_full_fov(bs), is_full_fov(ue)
    enabled = not (bf and uf)
    return bs, ue, enabled, enabled and not bf, enabled and not uf


def perturbed(zc, re, im, mag):
    """The 27 shifted directions, each [27, N, L]"""
    s = _SHIFTS.reshape((27, 3) + (1,) * zc.ndim)
    return (zc[None] + EPS * s[:, 0] * mag[0][None], re[None] + EPS * s[:, 1] * mag[1][None],
            im[None] + EPS * s[:, 2] * mag[2][None])


def dipole_nonzero(theta):
    with np.errstate(invalid="ignore"):
        return np.abs(np.sin(theta)) > 1e-10


def side_undecidable(rot_deg, el_deg, az_deg, fov_deg=None, dipole=False):
    """bool [N, L]: some decision of this array side changes under the perturbation.  fov_deg: the side's FoV when it is
    restricted, else None."""
    zc, re, im, mag = rotated_direction(rot_deg, el_deg, az_deg)
    th0, ph0 = angles_of(zc, re, im)
    thp, php = angles_of(*perturbed(zc, re, im, mag))
    bad = (np.isnan(thp) != np.isnan(th0)[None]).any(axis=0)
    m0 = fov_mask(fov_deg, th0, ph0) if fov_deg is not None else None
    g0 = dipole_nonzero(th0) if dipole else None
    for a in (-1.0, 0.0, 1.0):
        t = thp * (1.0 + a * ANG_REL)
        if dipole:
            bad |= (dipole_nonzero(t) != g0[None]).any(axis=0)
        if fov_deg is not None:
            for b in (-1.0, 0.0, 1.0):
                bad |= (fov_mask(fov_deg, t, php * (1.0 + b * ANG_REL)) != m0[None]).any(axis=0)
    return bad & ~np.isnan(zc)


def undecidable(config, points):
    """config = (rotation in degrees [3] or [N, 3], the side's FoV in degrees when it is restricted else None, dipole or
    not); points = (elevations, azimuths) in float32 degrees [N, L].  bool [N, L]."""
    rot, fov, dipole = config
    return side_undecidable(rot, points[0], points[1], fov, dipole)


def steps_ld(zc, re, im, spacing):
    """(y step, z step) in revolutions, spacing sin(zenith') sin(azimuth') and spacing cos(zenith') (geometry.py:99-101
    with kd / 2pi = spacing), in np.longdouble from the direction: sin(arccos zc) = sqrt(1 - zc^2), sin(angle(re + j im)) =
    im / |re + j im| and 0 where both vanish (np.angle gives 0 there)."""
    z, r, i = (np.asarray(v, dtype=np.longdouble) for v in (zc, re, im))
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(r * r + i * i)
        sphi = np.where(rho > 0, i / np.where(rho > 0, rho, 1), np.longdouble(0))
        sth = np.sqrt(np.maximum(1 - z * z, 0))
    sp = np.longdouble(spacing)
    return sp * sth * sphi, sp * z


def _side(rot_deg, el_deg, az_deg, spacing):
    """Everything of one array side: angles, steps, and the tolerances the perturbation gives them"""
    zc, re, im, mag = rotated_direction(rot_deg, el_deg, az_deg)
    th, ph = angles_of(zc, re, im)
    zp, rp, ip = perturbed(zc, re, im, mag)
    thp, php = angles_of(zp, rp, ip)
    y0, z0 = steps_ld(zc, re, im, spacing)
    yp, zq = steps_ld(zp, rp, ip, spacing)
    ulp4 = 4 * np.spacing(np.float64(spacing))
    with np.errstate(invalid="ignore"):
        tol_y = np.nan_to_num(np.abs(yp - y0[None]).max(axis=0).astype(np.float64), nan=0.0) + ulp4
        tol_z = np.nan_to_num(np.abs(zq - z0[None]).max(axis=0).astype(np.float64), nan=0.0) + ulp4
        tol_th = np.nan_to_num(np.fmax.reduce(np.abs(thp - th[None]), axis=0), nan=0.0) + ANG_REL * np.nan_to_num(np.abs(th))
        tol_ph = np.nan_to_num(np.fmax.reduce(np.abs(php - ph[None]), axis=0), nan=0.0) + ANG_REL * np.nan_to_num(np.abs(ph))
    return dict(zc=zc, re=re, im=im, th=th, ph=ph, y=y0, z=z0, tol_y=tol_y, tol_z=tol_z, tol_th=tol_th, tol_ph=tol_ph)


# ---------------------------------------------------------------------------------------------------------------------
# powers, LoS, delay maximum
# ---------------------------------------------------------------------------------------------------------------------
def pattern_gain(name, theta):
    """ant_patterns.py:21-71: 1.0, or the half-wave dipole 1.643 cos^2(pi/2 cos t) / sin t where |sin t| > 1e-10, else 0"""
    if name == "isotropic":
        return 1.0
    assert name == "halfwave-dipole", name
    g = np.zeros_like(theta, dtype=np.float64)
    ok = dipole_nonzero(theta)
    t = theta[ok]
    g[ok] = 1.643 * (np.cos(np.pi / 2 * np.cos(t)) ** 2 / np.sin(t))
    return g


def max_delay_key(delay_used):
    """The launch's running maximum as stage 1 leaves it: 0 when no used delay is a number, else the order-preserving key
    of nanmax (float_order_key in k1_path_math.h; dmx_decode_max_delay inverts it).  Returned as int32 bits."""
    d = np.asarray(delay_used, dtype=np.float32)
    if d.size == 0 or np.all(np.isnan(d)):
        return np.int32(0)
    b = np.array([np.nanmax(d)], dtype=np.float32).view(np.uint32)[0]
    key = (~b) & np.uint32(0xFFFFFFFF) if b & np.uint32(0x80000000) else b | np.uint32(0x80000000)
    return np.array([key], dtype=np.uint32).view(np.int32)[0]


def decode_max_delay(key_i32):
    """dmx_decode_max_delay restated"""
    key = int(np.array([key_i32], dtype=np.int32).view(np.uint32)[0])
    if key == 0:
        return np.float32(np.nan)
    b = (key & 0x7FFFFFFF) if key & 0x80000000 else (~key) & 0xFFFFFFFF
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the whole of stage 1
# ---------------------------------------------------------------------------------------------------------------------
def stage1_reference(case, rays, ue_rot):
    """case: dict with bs_rot, bs_fov, ue_fov, bs_pattern, ue_pattern, bs_spacing, ue_spacing, num_paths, freq_domain,
    subcarriers, bandwidth, rx_filter, doppler, fc, adaptive.  rays: float32 [n, L] matrices (+ doppler_vel / doppler_acc).
    ue_rot: [3] or [n, 3] degrees.  Returns the side products [n, L] / [n] and the records padded to [n, P] with
    `slot_path` = the path a slot holds (-1 past n_keep)."""
    power = rays["power"]
    n, L = power.shape
    P = min(int(case["num_paths"]), L)
    fd = bool(case["freq_domain"])
    N = int(case["subcarriers"])
    iso = case["bs_pattern"] == "isotropic" and case["ue_pattern"] == "isotropic"
    T = _side(case["bs_rot"], rays["aod_el"], rays["aod_az"], case["bs_spacing"])
    R = _side(ue_rot, rays["aoa_el"], rays["aoa_az"], case["ue_spacing"])
    bs_fov, ue_fov, enabled, bs_res, ue_res = stored_fovs(case["bs_fov"], case["ue_fov"])
    mask = None
    if enabled:
        mask = np.ones((n, L), dtype=bool)
        if bs_res:
            mask &= fov_mask(bs_fov, T["th"], T["ph"])
        if ue_res:
            mask &= fov_mask(ue_fov, R["th"], R["ph"])
    m = np.ones((n, L), dtype=bool) if mask is None else mask
    th_t, ph_t = np.where(m, T["th"], np.nan), np.where(m, T["ph"], np.nan)
    th_r, ph_r = np.where(m, R["th"], np.nan), np.where(m, R["ph"], np.nan)

    with np.errstate(all="ignore"):
        pl = 10 ** (power / 10)                                            # float32
        gain = pattern_gain(case["bs_pattern"], th_t) * pattern_gain(case["ue_pattern"], th_r)
        pw = pl * gain                                                     # float32 isotropic, float64 dipole
    num_paths = (~np.isnan(ph_r)).sum(axis=1)
    inter = rays["inter"]
    los = np.full(n, -1)
    if mask is not None:
        has = mask.any(axis=1)
        first = np.full(n, -1.0)
        j = np.argmax(mask, axis=1)
        first[has] = inter[np.arange(n)[has], j[has]]
    else:
        has = num_paths > 0
        first = inter[:, 0]
    los[has] = 0
    with np.errstate(invalid="ignore"):
        los[(first == 0) & has] = 1

    out = dict(n=n, L=L, P=P, aod_el_rot=T["th"], aod_az_rot=T["ph"], aoa_el_rot=R["th"], aoa_az_rot=R["ph"],
               tol_aod_el=T["tol_th"], tol_aod_az=T["tol_ph"], tol_aoa_el=R["tol_th"], tol_aoa_az=R["tol_ph"],
               fov_mask=mask, power_linear=pl, power_linear_ant_gain=pw, num_paths=num_paths, los=los,
               max_delay_key=max_delay_key(rays["delay"][:, :P]), dir_t=(T["zc"], T["re"], T["im"]),
               dir_r=(R["zc"], R["re"], R["im"]), iso=iso)
    # the golden bound of power_linear_ant_gain (tests/test_gpu_parity.py::test_golden), per path
    pw_bound = 2e-6 * 1.643 ** 2 * np.nan_to_num(pl.astype(np.float64)) + 5e-5 * np.nan_to_num(np.abs(pw.astype(np.float64)))
    out["pw_bound"] = pw_bound

    # ---- records of the first P paths
    s = np.s_[:, :P]
    phase64 = np.deg2rad(rays["phase"][s]).astype(np.float64)              # float32 deg2rad, as the complex64 exp takes it
    with np.errstate(all="ignore"):
        e = np.exp(1j * phase64)
        pwu = pw[s].astype(np.float64)
        valid = ~np.isnan(pw[s])                                           # channel.py:260
        ang_ok = ~np.isnan(th_t[s]) & ~np.isnan(th_r[s])                    # geometry.py:65
        if fd:
            dn = rays["delay"][s] / np.float32(1.0 / case["bandwidth"])    # float32 / float32 (channel.py:183)
            over = dn >= N                                                 # channel.py:187-189
            pwu = np.where(over, 0.0, pwu)
            dn = np.where(over, np.float32(N), dn).astype(np.float32)
            c = np.sqrt(pwu / N) * e
            scale = N
            if case.get("doppler") and "doppler_vel" in rays and not case["rx_filter"]:   # construct_deepmimo.py:267-280
                tau = rays["delay"][s].astype(np.float64)
                v, a = rays["doppler_vel"][s].astype(np.float64), rays["doppler_acc"][s].astype(np.float64)
                c = c * np.exp(-2j * np.pi * case["fc"] * (v * tau / LIGHTSPEED + a * tau ** 2 / (2 * LIGHTSPEED)))
            keep = (valid & ang_ok & ~np.isnan(ph_t[s]) & ~np.isnan(ph_r[s]) & ~np.isnan(c) & ~np.isnan(dn) &
                    (c.astype(np.complex64) != 0))                          # nansum: NaN factors and exact zeros add nothing
        else:
            dn = np.zeros((n, P), dtype=np.float32)
            c = np.sqrt(pwu) * e
            c = np.where(ang_ok, c, c * 0.0)                               # zero array response, NaN stays NaN
            scale = 1
            keep = valid                                                   # the slot is kept even with a zero coefficient
    amp = np.abs(np.nan_to_num(c))
    if iso:
        tol_c = C_RTOL * amp
    else:
        bn = pw_bound[s] / scale
        with np.errstate(all="ignore"):
            tol_c = np.minimum(np.sqrt(bn), np.where(amp > 0, bn / np.where(amp > 0, amp, 1), np.inf)) + C_RTOL * amp
    dop = bool(case.get("doppler")) and "doppler_vel" in rays
    dv = rays["doppler_vel"][s].astype(np.float32) if dop else np.zeros((n, P), np.float32)
    da = rays["doppler_acc"][s].astype(np.float32) if dop else np.zeros((n, P), np.float32)
    z = np.longdouble(0)
    ty, tz = np.where(ang_ok, T["y"][s], z), np.where(ang_ok, T["z"][s], z)
    ry, rz = np.where(ang_ok, R["y"][s], z), np.where(ang_ok, R["z"][s], z)

    sort = fd and bool(case.get("adaptive")) and L <= 64                   # launch_path_prep: sort_paths && L <= LPU
    slot_path = np.full((n, P), -1, dtype=np.int64)
    n_keep = keep.sum(axis=1).astype(np.int32)
    for u in range(n):
        idx = np.flatnonzero(keep[u])
        if sort:
            idx = idx[np.lexsort((idx, -(np.abs(c[u, idx]) ** 2)))]      # falling |c|^2, ties by path index
        slot_path[u, :idx.size] = idx
    filled = slot_path >= 0
    g = np.where(filled, slot_path, 0)
    def take(a):                                                           # [n, P] by slot, zero past n_keep
        return np.where(filled, np.take_along_axis(a, g, axis=1), np.zeros((), dtype=a.dtype))
    out.update(slot_path=slot_path, n_keep=n_keep, filled=filled, c=take(c), dn=take(dn), tol_c=take(tol_c),
               tx_y=take(ty), tx_z=take(tz), rx_y=take(ry), rx_z=take(rz),
               tol_tx_y=take(T["tol_y"][s]), tol_tx_z=take(T["tol_z"][s]), tol_rx_y=take(R["tol_y"][s]),
               tol_rx_z=take(R["tol_z"][s]), dop_v=take(dv), dop_a=take(da), keep=keep, c_all=c)
    return out


def channel_from_records(ref, case):
    """The channel as a direct sum over the reference's records, complex128: [n, M_rx, M_tx, K] in the frequency domain
    (no rx_filter), [n, M_rx, M_tx, P] in the time domain (one slot per tap)."""
    def idx(shape):
        mh, mv = int(shape[0]), int(shape[1])
        m = np.arange(mh * mv)
        return m % mh, m // mh
    ty_i, tz_i = idx(case["bs_shape"])
    ry_i, rz_i = idx(case["ue_shape"])
    f = ref["filled"]
    c = np.where(f, ref["c"], 0)
    ph_t = np.exp(2j * np.pi * (ty_i[None, :, None] * ref["tx_y"].astype(np.float64)[:, None, :] +
                                tz_i[None, :, None] * ref["tx_z"].astype(np.float64)[:, None, :]))      # [n, M_tx, P]
    ph_r = np.exp(2j * np.pi * (ry_i[None, :, None] * ref["rx_y"].astype(np.float64)[:, None, :] +
                                rz_i[None, :, None] * ref["rx_z"].astype(np.float64)[:, None, :]))
    if case["freq_domain"]:
        k = np.asarray(case["selected"], dtype=np.float64)
        g = c[:, :, None] * np.exp(-2j * np.pi * ref["dn"].astype(np.float64)[:, :, None] * k[None, None, :] / case["subcarriers"])
        return np.einsum("nrp,ntp,npk->nrtk", ph_r, ph_t, g)
    return ph_r[:, :, None, :] * ph_t[:, None, :, :] * c[:, None, None, :]
