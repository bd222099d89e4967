"""The case table of the near-field tests: tests/test_near_field_cpu.py checks on the reference alone that no case is vacuous
and that the delay-rounding term of the tolerance is negligible, tests/test_gpu_near_field.py runs every channel case on the
GPU against tests/_near_field_ref.py, tests/test_gpu_near_field_consumers.py the consumer cases.  A plain module: NumPy and
the oracle only.  The case dicts are those of tests/_wideband_cases.py (its `oracle_params`, `dm_params`, `fovs`,
`ue_rotation` read them); `beta` is not used.

Rays: oracle_np.synth_rays, then the delays redrawn so that every path length R = tau f_c lies between 2 and 1000 apertures
of the BS panel (log-uniform; the aperture is the panel diagonal in wavelengths, and 1000 apertures is cut at 0.45 N samples
so that no path is clipped), path 0 of user 0 at delay 0 (R = 0), user 2 emptied.

Each channel case is there for a way the vector kernel's near-field instantiations can go wrong (k2_channel_fd.hip): the
one-wave and the four-wave form, RB = 1 and 2, the 64-subcarrier chunk tail, a single subcarrier, z rows, odd panels, negative
indices and indices beyond N, every table size (8, 16, 28, 32 slots), the accumulate pass beyond 32 slots, compaction."""
from __future__ import annotations

import numpy as np

from tests import _wideband_cases as WC

BANDWIDTH = WC.BANDWIDTH
CARRIER = 28e9
N_SC = 512


def _case(id, bs, ue, sel, n=7, L=10, P=None, kept=None, holes=False, **extras):
    return dict(id=id, bs=list(bs), ue=list(ue), N=N_SC, sel=np.asarray(sel, dtype=np.int64), n=n, L=L, P=L if P is None else P,
                beta=None, kept=kept, holes=holes, extras=extras)


FULL_CASE = _case("rotation_fov_patterns_doppler", [8, 4], [2, 2], np.arange(-10, 11), n=9, L=12, kept=12,
                  bs_rot=[10, -20, 30], ue_rot="per_user", bs_fov=[150, 120], ue_fov=[300, 160], bs_pattern="tr38901",
                  ue_pattern="halfwave-dipole", doppler=True)

CHANNEL_CASES = (
    _case("one_wave_4x2", [4, 2], [1, 1], np.arange(64)),
    _case("ula16_k64", [16, 1], [1, 1], np.arange(64)),
    _case("ula33_2x2_k70_kept7", [33, 1], [2, 2], np.arange(70), n=5, L=7, kept=7),
    _case("upa8x4_3x1_k5_far_indices", [8, 4], [3, 1], [-3, 0, 7, 600, 5000], n=9),
    _case("odd3x5_2x2_k1_kept1", [3, 5], [2, 2], [5], n=6, L=1, kept=1),
    _case("ula16_2x2_kept32", [16, 1], [2, 2], np.arange(0, 24, 2), n=5, L=32, kept=32),
    _case("upa8x4_3x1_loaded40", [8, 4], [3, 1], np.arange(0, 24, 2), n=6, L=40, kept=40),
    _case("ula16_2x2_holes", [16, 1], [2, 2], np.arange(-32, 32), n=21, L=25, holes=True),
    FULL_CASE,
)

# the consumers: at most 32 paths, a uniformly spaced selection (compute_angle_delay), indices within the beam kernels' bound
CONSUMER_CASES = (
    _case("c_ula16_1x1_k70_p7", [16, 1], [1, 1], np.arange(70), n=6, L=7, kept=7),
    _case("c_upa8x4_2x2_k5_p32", [8, 4], [2, 2], np.arange(0, 10, 2), n=5, L=32, kept=32),
    _case("c_ula16_2x2_k1_p1", [16, 1], [2, 2], [3], n=5, L=1, kept=1),
)

CASES = CHANNEL_CASES + CONSUMER_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

oracle_params, dm_params, fovs, ue_rotation = WC.oracle_params, WC.dm_params, WC.fovs, WC.ue_rotation


def single_antenna(case):
    """the case with a 1 x 1 array at both ends, on rays drawn for the aperture of the case it comes from"""
    return dict(case, id=case["id"] + "_1x1", bs=[1, 1], ue=[1, 1], aperture_of=case["bs"])


def aperture(case):
    """the BS panel diagonal in wavelengths"""
    mh, mv = case.get("aperture_of", case["bs"])
    return WC.SPACING_BS * float(np.hypot(mh - 1, mv - 1))


_RAYS = {}


def case_rays(case, which="a"):
    """the float32 rays of a case (shared, read-only); `which`: "a", the rays of the references, or "b", a second draw"""
    from oracle import oracle_np as onp
    key = (case["id"], which)
    if key not in _RAYS:
        n, L = case["n"], case["L"]
        dop = bool(case["extras"].get("doppler"))
        seed = 7300 + sum(map(ord, case["id"])) + (0 if which == "a" else 10000)
        r = onp.synth_rays(n, L, seed=seed, all_valid=case["kept"] is not None, with_doppler=dop)
        keys = list(onp.RAY_KEYS) + (["doppler_vel", "doppler_acc"] if dop else [])
        r = {k: r[k] for k in keys}
        rng = np.random.default_rng(seed + 1)
        D = aperture(case)
        r_max = min(1000 * D, 0.45 * case["N"] * CARRIER / BANDWIDTH)
        R = np.exp(rng.uniform(np.log(2 * D), np.log(r_max), (n, L)))
        # the float32 delay moves psi of a path at R by about (D^2 / 2 R) 2^-23 revolutions: a user's strongest path is put at
        # 64 apertures or more and a path nearer than that is weakened in proportion, so that the sum stays within 1 % of the
        # criterion (tests/test_near_field_cpu.py asserts it)
        power = r["power"].astype(np.float64)
        strongest = np.nanargmax(np.where(np.isnan(power), -np.inf, power), axis=1)
        rows = np.arange(n)
        R[rows, strongest] = np.maximum(R[rows, strongest], min(64 * D, r_max))
        power -= 20 * np.log10(np.maximum(64 * D / R, 1.0))
        r["power"] = power.astype(np.float32)
        delay = (R / CARRIER).astype(np.float32)
        delay[0, 0] = 0.0
        delay[np.isnan(r["delay"])] = np.nan
        r["delay"] = delay
        if case["kept"] is not None:
            for v in r.values():
                v[:, case["kept"]:] = np.nan
        if case["holes"]:
            hole = rng.uniform(size=(n, L)) < 0.25
            hole[0, 0] = False
            for v in r.values():
                v[hole] = np.nan
        for v in r.values():
            v[2, :] = np.nan                                            # a user with no path: all-zero output
            v.setflags(write=False)
        _RAYS[key] = r
    return _RAYS[key]


def dataset(case, which="a", device=None):
    """a Dataset on the rays of a case, its fields of view applied; `device`: the ray matrices as resident tensors there"""
    import deepmimo_amd as dm
    rays = {k: v.copy() for k, v in case_rays(case, which).items()}
    if device is not None:
        import torch
        rays = {k: torch.from_numpy(v).to(device) for k, v in rays.items()}
    rays["rx_pos"], rays["tx_pos"] = np.zeros((case["n"], 3), np.float32), np.zeros((1, 3), np.float32)
    ds = dm.Dataset(rays)
    bs_fov, ue_fov = fovs(case)
    if bs_fov is not None or ue_fov is not None:
        ds.apply_fov(**{k: v for k, v in (("bs_fov", bs_fov), ("ue_fov", ue_fov)) if v is not None})
    return ds


def doppler_arg(case, rays):
    """the `doppler` argument of the references: the carrier of the Doppler term is the view's carrier"""
    if not case["extras"].get("doppler"):
        return None
    return dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=CARRIER)


_REF = {}


def references(case):
    """(H_nf, H_ff, tol) of a case, computed once: complex128 near-field and far-field references (tests/_near_field_ref.py;
    "tr38901" through tests/_pattern_ref.py) and the per-user channel tolerance"""
    from tests import _near_field_ref as NF
    from tests._pattern_ref import patched_oracle
    key = case["id"]
    if key not in _REF:
        rays, op = case_rays(case), oracle_params(case)
        bs_fov, ue_fov = fovs(case)
        dop = doppler_arg(case, rays)
        with patched_oracle():
            nf = NF.near_field_channels(rays, op, CARRIER, bs_fov, ue_fov, dop)
            ff = NF.far_field_channels(rays, op, bs_fov, ue_fov, dop)
            tol = NF.near_field_tolerance(nf, rays, op, CARRIER, bs_fov, ue_fov, dop)
        for a in (nf, ff, tol):
            a.setflags(write=False)
        _REF[key] = (nf, ff, tol)
    return _REF[key]
