"""Inputs of the stage-1 tests (tests/test_stage1_cases_cpu.py, tests/test_gpu_stage1_records.py) and the reader of the
record arrays stage 1 leaves in the workspace.

Two families.  LATTICE cases put every direction of an exact-degree lattice (poles, the azimuth branch cut, angles outside
the nominal range, FoV edges) through 29 rotation / FoV / pattern configurations; lattice points that are undecidable
for a configuration (tests/_stage1_ref.py) are replaced by the next decidable point BEFORE the rays are built, so every
assertion on them is exact and nothing is excluded at assert time.  STRUCTURAL cases use random decidable angles; what
matters there is where things sit in a row: path counts around the 32 / 64 / 128 lane boundaries, num_paths cutting a
pass, users built by hand (first in-FoV path at a given index, holes, single-field NaN, clip-edge delays, equal powers).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import _stage1_ref as s1

ELEVATIONS = np.array(list(range(0, 181, 15)) + [-15, 195, 270, 360], dtype=np.float32)
AZIMUTHS = np.array([-360, -270, -180, -135, -90, -45, -30, 0, 30, 45, 60, 90, 120, 135, 180, 225, 270, 360, 540], dtype=np.float32)
LAT_EL = np.repeat(ELEVATIONS, AZIMUTHS.size)                  # 17 x 19 = 323 directions
LAT_AZ = np.tile(AZIMUTHS, ELEVATIONS.size)
N_LAT = LAT_EL.size

ROTATIONS = [[0, 0, 0], [0, 0, 90], [0, 0, -180], [0, 0, 45], [90, 0, 0], [0, 90, 0], [0, -90, 0], [180, 0, 0], [0, 180, 0],
             [90, 90, 90], [45, 0, 0], [0, 45, 0], [30, 60, -45], [0, 0, 360], [-90, 0, 180]]
FOVS = [[180, 180], [90, 90], [360, 90], [180, 60], [120, 120], [60, 30], [270, 180], [0, 0], [360, 0], [359, 179], [90, 180]]
CAP_ANY, CAP_ALL = 0.15, 0.03                                  # dropped lattice points: any configuration side, all together

FC = 28e9
WANT_SIDES = (True, "light", False)


def _case(cid, kind, n, L, **kw):
    d = dict(id=cid, kind=kind, n=n, L=L, num_paths=L, bs_shape=[4, 2], ue_shape=[2, 1], bs_spacing=0.5, ue_spacing=0.37,
             bs_rot=[0, 0, 0], ue_rot=[0, 0, 0], per_user_rot=False, bs_fov=None, ue_fov=None, bs_pattern="isotropic",
             ue_pattern="isotropic", freq_domain=1, subcarriers=64, selected=[0, 5, 63], bandwidth=20e6, rx_filter=0,
             doppler=0, fc=FC, adaptive=False, hand=None, seed=0)
    d.update(kw)
    d["seed"] = d["seed"] or (1000 + 7 * n + L + sum(ord(ch) for ch in cid))
    return d


def _lat(cid, bs_rot=(0, 0, 0), bs_fov=None, ue_rot=(0, 0, 0), ue_fov=None, L=25, **kw):
    n = -(-N_LAT // L)
    return _case("lat_" + cid, "lattice", n, L, bs_rot=list(bs_rot), bs_fov=bs_fov, ue_rot=list(ue_rot), ue_fov=ue_fov, **kw)


DIP = "halfwave-dipole"
LATTICE_CASES = [
    _lat("zero_nofov"),                                                        # the zero-rotation lean form; azimuth of -0.0
    _lat("zero_bs180", bs_fov=[180, 180]),
    _lat("z90_bs180", (0, 0, 90), [180, 180]),
    _lat("zm180_bs90", (0, 0, -180), [90, 90], ue_rot=(0, 0, 45)),
    _lat("z45_bs360_90", (0, 0, 45), [360, 90]),
    _lat("x90_bs180_60", (90, 0, 0), [180, 60]),
    _lat("y90_bs120", (0, 90, 0), [120, 120]),
    _lat("ym90_bs60_30", (0, -90, 0), [60, 30]),
    _lat("x180_bs270", (180, 0, 0), [270, 180]),
    _lat("y180_bs0", (0, 180, 0), [0, 0]),
    _lat("xyz90_bs360_0", (90, 90, 90), [360, 0]),
    _lat("x45_bs359", (45, 0, 0), [359, 179]),
    _lat("y45_bs90_180", (0, 45, 0), [90, 180]),
    _lat("gen_bs120", (30, 60, -45), [120, 120]),
    _lat("z360_bs180", (0, 0, 360), [180, 180]),
    _lat("xm90z180_bs90", (-90, 0, 180), [90, 90]),
    _lat("ue_zero_180", ue_fov=[180, 180]),
    _lat("ue_z90_180_60", ue_rot=(0, 0, 90), ue_fov=[180, 60]),
    _lat("ue_x90_0", ue_rot=(90, 0, 0), ue_fov=[0, 0]),
    _lat("ue_gen_359", (0, 0, 45), None, (30, 60, -45), [359, 179]),
    _lat("both_sides", (0, 0, 45), [270, 180], (0, 90, 0), [90, 90]),
    _lat("per_user_fov", (0, 0, 90), None, ue_fov=[120, 120], per_user_rot=True),
    _lat("per_user_nofov", (45, 0, 0), per_user_rot=True),
    _lat("dipole_bs", (45, 0, 0), bs_pattern=DIP),
    _lat("dipole_ue_fov", (0, 0, 0), None, (0, 45, 0), [180, 60], ue_pattern=DIP),
    _lat("gen_nofov_L70", (30, 60, -45), None, (-90, 0, 180), L=70),
    _lat("td_zero_bs180", bs_fov=[180, 180], freq_domain=0),
    _lat("td_gen_nofov", (30, 60, -45), None, (0, 0, 90), freq_domain=0),
    _lat("td_dipole_ue", (0, 90, 0), None, (180, 0, 0), ue_pattern=DIP, freq_domain=0),
]

# hand-built users of the three-pass case: what each row is made to hold
FIRST_IN_FOV = (0, 31, 32, 63, 64, 127, 128)
HAND_USERS = ([("first_in_fov", k) for k in FIRST_IN_FOV] +
              [("none_in_fov", None), ("first_hole", None), ("all_holes", None), ("holes_pass1", None), ("holes_pass2", None),
               ("max_delay_pass2", None), ("max_delay_past_P", None), ("delay_all_nan", None)])
SINGLE_NAN_FIELDS = ("power", "phase", "delay", "aoa_az", "aod_el", "inter")
EDGE_USERS = ("power_minus_inf", "clip_edge", "weak_path", "equal_powers")
FOV_S = [120, 100]                                              # the structural cases' BS field of view
ROT_S = [5, -20, 60]


def _st(cid, n, L, **kw):
    return _case("st_" + cid, "struct", n, L, **kw)


STRUCT_CASES = [
    _st("L1", 7, 1, bs_rot=ROT_S, bs_fov=FOV_S),
    _st("L25", 37, 25, bs_rot=ROT_S, bs_fov=FOV_S),
    _st("L32", 37, 32, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L33", 7, 33, bs_rot=ROT_S, bs_fov=FOV_S),
    _st("L64", 7, 64, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L64_P32", 7, 64, bs_rot=ROT_S, bs_fov=FOV_S, num_paths=32, holes=True),
    _st("L65", 7, 65, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L70", 37, 70, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L70_n1", 1, 70, bs_rot=ROT_S, bs_fov=FOV_S),
    _st("L70_P64", 7, 70, bs_rot=ROT_S, bs_fov=FOV_S, num_paths=64, holes=True),
    _st("L70_P65", 7, 70, bs_rot=ROT_S, bs_fov=FOV_S, num_paths=65, holes=True),
    _st("L128", 7, 128, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L130", 7, 130, bs_rot=ROT_S, bs_fov=FOV_S, holes=True),
    _st("L25_P10", 37, 25, bs_rot=ROT_S, bs_fov=FOV_S, num_paths=10),
    _st("L25_P40", 7, 25, bs_rot=ROT_S, bs_fov=FOV_S, num_paths=40),
    # the lean forms: no FoV, isotropic
    _st("lean_L1", 7, 1),
    _st("lean_L25_zero", 37, 25, holes=True),
    _st("lean_L32_rot", 37, 32, bs_rot=ROT_S, ue_rot=[10, 20, 30], holes=True),
    _st("lean_L25_per_user", 7, 25, per_user_rot=True),
    _st("lean_L33", 7, 33, holes=True),
    _st("lean_L64_rot", 7, 64, bs_rot=ROT_S),
    _st("lean_L70", 37, 70, bs_rot=ROT_S, holes=True),
    _st("lean_L70_P65", 7, 70, num_paths=65, holes=True),
    _st("lean_L130", 7, 130, ue_rot=[10, 20, 30], holes=True),
    # users built by hand
    _st("hand_L130", len(HAND_USERS), 130, bs_fov=FOV_S, num_paths=100, hand="fov"),
    _st("hand_L130_td", len(HAND_USERS), 130, bs_fov=FOV_S, num_paths=100, hand="fov", freq_domain=0),
    _st("all_delay_nan", 7, 25, bs_rot=ROT_S, hand="delay_nan"),
    _st("single_nan_fov", 7, 25, bs_fov=FOV_S, hand="single_nan"),
    _st("single_nan_lean", 7, 25, hand="single_nan"),
    _st("single_nan_td", 7, 25, bs_fov=FOV_S, hand="single_nan", freq_domain=0),
    _st("edges", 7, 25, bs_rot=ROT_S, hand="edges"),
    _st("edges_sorted", 7, 25, bs_rot=ROT_S, hand="edges", adaptive=True),
    _st("edges_td", 7, 25, bs_rot=ROT_S, hand="edges", freq_domain=0),
    # amplitude order (frequency domain, at most 64 loaded paths) and the path order beyond
    _st("order_L25", 37, 25, adaptive=True, holes=True),
    _st("order_L64_fov", 7, 64, bs_rot=ROT_S, bs_fov=FOV_S, adaptive=True, holes=True),
    _st("order_L70", 7, 70, bs_rot=ROT_S, adaptive=True, holes=True),
    _st("order_td", 7, 25, adaptive=True, holes=True, freq_domain=0),
    # Doppler rays: the rotation is applied to c without rx_filter and not with it
    _st("doppler", 37, 25, bs_rot=ROT_S, doppler=1),
    _st("doppler_lpf", 37, 25, bs_rot=ROT_S, doppler=1, rx_filter=1, selected=list(range(0, 64, 7))),
]
CASES = LATTICE_CASES + STRUCT_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# which kernel a case runs
# ---------------------------------------------------------------------------------------------------------------------
def fov_enabled(c):
    return s1.stored_fovs(c["bs_fov"], c["ue_fov"])[2]


def stage1_form_name(c, want_side):
    """(instantiation, passes) of launch_path_prep for a case: `stage1_form` (k1_path_math.h) with the side tensors
    ChannelEngine._side_tensors attaches, plus the L <= 32 split.  FULL when a FoV is on, a pattern is a dipole or the angle /
    power outputs are wanted (want_side = True); the zero-rotation lean form only with both rotations zero, no per-user
    rotation and at most 32 loaded paths."""
    L = c["L"]
    lpu = 32 if L <= 32 else 64
    passes = -(-L // lpu)
    iso = c["bs_pattern"] == "isotropic" and c["ue_pattern"] == "isotropic"
    if fov_enabled(c) or not iso or want_side is True:
        return f"k1_path_prep_full<{lpu}>", passes
    zrot = (not c["per_user_rot"]) and L <= 32 and not any(c["bs_rot"]) and not any(c["ue_rot"])
    return ("k1_path_prep<32,true>" if zrot else f"k1_path_prep<{lpu}>"), passes


def direct_taken(c):
    """fd_direct_waves_per_block's scope for these small panels: frequency domain, no rx_filter, no flags, at most 64
    loaded and 32 used paths"""
    return bool(c["freq_domain"]) and not c["rx_filter"] and not c["adaptive"] and c["L"] <= 64 and min(c["num_paths"], c["L"]) <= 32


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def case_ue_rot(c):
    """[3], or [n, 3] for a per-user case: the listed rotations, one per user in turn"""
    if not c["per_user_rot"]:
        return np.array(c["ue_rot"])
    return np.array([ROTATIONS[(3 + 7 * u) % len(ROTATIONS)] for u in range(c["n"])], dtype=np.float64)


def _side_args(c):
    """((rotation, fov or None, dipole) of the BS side, the same of the UE side) as `side_undecidable` takes them"""
    bs_fov, ue_fov, _, bs_res, ue_res = s1.stored_fovs(c["bs_fov"], c["ue_fov"])
    return ((np.array(c["bs_rot"]), bs_fov if bs_res else None, c["bs_pattern"] == DIP),
            (case_ue_rot(c), ue_fov if ue_res else None, c["ue_pattern"] == DIP))


def undecidable_rays(c, rays):
    """bool [n, L] per side for the rays of a case"""
    bs, ue = _side_args(c)
    return s1.undecidable(bs, (rays["aod_el"], rays["aod_az"])), s1.undecidable(ue, (rays["aoa_el"], rays["aoa_az"]))


def _place(und, perm, n, L):
    """Lattice indices [n, L]: the shuffled lattice row by row (wrapping), every entry undecidable for its user replaced by
    the next decidable lattice point.  und: bool [1 or n, N_LAT].  Also the number of the N_LAT first placements dropped."""
    idx = perm[np.arange(n * L) % N_LAT].reshape(n, L)
    dropped = 0
    for u in range(n):
        bad = und[u % und.shape[0]]
        assert not bad.all()
        for j in range(L):
            k = idx[u, j]
            if bad[k]:
                dropped += int(u * L + j < N_LAT)
                while bad[k]:
                    k = (k + 1) % N_LAT
                idx[u, j] = k
    return idx, dropped


def lattice_rays(c):
    """(rays, dropped AoD points, dropped AoA points)"""
    from oracle import oracle_np as onp
    n, L = c["n"], c["L"]
    rays = onp.synth_rays(n, L, seed=c["seed"], all_valid=True)            # powers, phases, delays as every test draws them
    rng = np.random.default_rng(c["seed"] + 1)
    (rt, ft, dt), (rr, fr, dr) = _side_args(c)
    und_t = s1.side_undecidable(rt, LAT_EL[None, :], LAT_AZ[None, :], ft, dt)
    rows = n if c["per_user_rot"] else 1
    und_r = s1.side_undecidable(rr, np.tile(LAT_EL, (rows, 1)), np.tile(LAT_AZ, (rows, 1)), fr, dr)
    it, drop_t = _place(und_t, rng.permutation(N_LAT), n, L)
    ir, drop_r = _place(und_r, rng.permutation(N_LAT), n, L)
    rays["aod_el"], rays["aod_az"] = LAT_EL[it].copy(), LAT_AZ[it].copy()
    rays["aoa_el"], rays["aoa_az"] = LAT_EL[ir].copy(), LAT_AZ[ir].copy()
    return rays, drop_t, drop_r


RAY_FIELDS = ("power", "phase", "delay", "aoa_az", "aoa_el", "aod_az", "aod_el", "inter")
_IN = dict(el=(60, 120), az=(-40, 40))                                     # decisively inside FOV_S at zero rotation
_OUT = dict(el=(60, 120), az=(140, 220))                                   # decisively outside


def _hole(rays, u, j):
    for k in RAY_FIELDS:
        rays[k][u, j] = np.nan


def _draw(rng, box, size):
    return (rng.uniform(*box["el"], size).astype(np.float32), rng.uniform(*box["az"], size).astype(np.float32))


def _hand_fov(c, rays, rng):
    """Zero rotation, BS FoV = FOV_S: every AoD drawn inside, then rows edited.  num_paths = 100 of 130 loaded."""
    n, L, P = c["n"], c["L"], min(c["num_paths"], c["L"])
    rays["aod_el"], rays["aod_az"] = _draw(rng, _IN, (n, L))
    rays["inter"][:] = rng.integers(1, 5, (n, L)).astype(np.float32)
    rays["delay"][:] = np.minimum(rays["delay"], np.float32(1.9e-6))
    for u, (what, k) in enumerate(HAND_USERS):
        if what == "first_in_fov":
            rays["aod_el"][u, :k], rays["aod_az"][u, :k] = _draw(rng, _OUT, k)
            rays["inter"][u, :] = 0.0 if u % 2 else 3.0                 # the first in-FoV path alone decides LoS
            rays["inter"][u, k] = 3.0 if u % 2 else 0.0
        elif what == "none_in_fov":
            rays["aod_el"][u], rays["aod_az"][u] = _draw(rng, _OUT, L)
        elif what == "first_hole":
            _hole(rays, u, 0)
            rays["inter"][u, 1] = 0.0
        elif what == "all_holes":
            _hole(rays, u, slice(None))
        elif what == "holes_pass1":
            _hole(rays, u, [0, 3, 4, 31, 32, 62, 63])
        elif what == "holes_pass2":
            _hole(rays, u, [64, 65, 90, 99, 100, 127])
        elif what == "max_delay_pass2":
            rays["delay"][u, 70] = np.float32(2.5e-6)                     # the launch's maximum, in the second pass
        elif what == "max_delay_past_P":
            rays["delay"][u, P + 10] = np.float32(3.0e-6)                 # larger still, but not a used path
        elif what == "delay_all_nan":
            rays["delay"][u, :] = np.nan


def _hand_single_nan(c, rays, rng):
    """User f: only field f of path 0 is NaN; the last user is whole.  AoDs inside FOV_S (the FoV variant runs at zero
    rotation), so every decision is the NaN's."""
    n, L = c["n"], c["L"]
    rays["aod_el"], rays["aod_az"] = _draw(rng, _IN, (n, L))
    rays["inter"][:] = 2.0
    rays["inter"][:, 0] = 0.0
    for u, f in enumerate(SINGLE_NAN_FIELDS):
        rays[f][u, 0] = np.nan


def clip_edge_delays(c):
    """float32 delays one ulp below, at, and one ulp above N / bandwidth"""
    t = np.float32(c["subcarriers"] / c["bandwidth"])
    return np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], dtype=np.float32)


EQUAL_PATHS, EQUAL_HOLES = (2, 5, 9, 11), (3, 6, 10)


def _hand_edges(c, rays, rng):
    for u, what in enumerate(EDGE_USERS):
        if what == "power_minus_inf":
            rays["power"][u, 3] = -np.inf
        elif what == "clip_edge":
            rays["delay"][u, 0:3] = clip_edge_delays(c)
        elif what == "weak_path":
            rays["power"][u, 7] = np.float32(-300.0)
        elif what == "equal_powers":                                       # equal |c|: the order falls back on the path index
            for j in EQUAL_PATHS:
                rays["power"][u, j], rays["phase"][u, j] = np.float32(-71.5), np.float32(33.0)
            _hole(rays, u, list(EQUAL_HOLES))


def struct_rays(c):
    from oracle import oracle_np as onp
    n, L = c["n"], c["L"]
    rays = onp.synth_rays(n, L, seed=c["seed"], all_valid=True, with_doppler=bool(c["doppler"]))
    rng = np.random.default_rng(c["seed"] + 1)
    if c.get("holes"):                                                     # NaN inside rows, the same entries of every field
        hole = rng.uniform(size=(n, L)) < 0.2
        hole[:, 0] |= rng.uniform(size=n) < 0.3
        for k in [k for k in rays if k not in ("rx_pos", "tx_pos")]:
            rays[k][hole] = np.nan
    if c["hand"] == "fov":
        _hand_fov(c, rays, rng)
    elif c["hand"] == "single_nan":
        _hand_single_nan(c, rays, rng)
    elif c["hand"] == "edges":
        _hand_edges(c, rays, rng)
    elif c["hand"] == "delay_nan":
        rays["delay"][:] = np.nan
    for _ in range(20):                                                    # random angles: redraw the (rare) undecidable ones
        ut, ur = undecidable_rays(c, rays)
        if not (ut.any() or ur.any()):
            break
        rays["aod_az"][ut] += np.float32(0.37)
        rays["aoa_az"][ur] += np.float32(0.37)
    else:
        raise AssertionError(f"{c['id']}: undecidable angles left")
    return rays


@functools.lru_cache(maxsize=None)
def _built(cid):
    c = BY_ID[cid]
    if c["kind"] == "lattice":
        rays, dt, dr = lattice_rays(c)
    else:
        rays, dt, dr = struct_rays(c), 0, 0
    for v in rays.values():
        v.setflags(write=False)
    ref = s1.stage1_reference(c, rays, case_ue_rot(c))
    return rays, (dt, dr), ref


def case_rays(c):
    """The case's rays (read-only, built once per process)"""
    return _built(c["id"])[0]


def case_dropped(c):
    """(dropped AoD, dropped AoA) lattice points of the case's first N_LAT placements"""
    return _built(c["id"])[1]


def case_reference(c):
    """tests/_stage1_ref.stage1_reference of the case, computed once per process and shared (callers do not modify it)"""
    return _built(c["id"])[2]


def oracle_params(c):
    from oracle import oracle_np as onp
    return onp.make_params(
        bs_antenna=dict(shape=c["bs_shape"], spacing=c["bs_spacing"], rotation=np.array(c["bs_rot"]), radiation_pattern=c["bs_pattern"]),
        ue_antenna=dict(shape=c["ue_shape"], spacing=c["ue_spacing"], rotation=case_ue_rot(c), radiation_pattern=c["ue_pattern"]),
        num_paths=c["num_paths"], freq_domain=c["freq_domain"], enable_doppler=int(bool(c["doppler"])),
        ofdm=dict(subcarriers=c["subcarriers"], selected_subcarriers=np.array(c["selected"]), bandwidth=c["bandwidth"],
                  rx_filter=c["rx_filter"]))


def oracle_fovs(c):
    bs_fov, ue_fov = s1.stored_fovs(c["bs_fov"], c["ue_fov"])[:2]
    return bs_fov, ue_fov


# ---------------------------------------------------------------------------------------------------------------------
# the record arrays in the workspace
# ---------------------------------------------------------------------------------------------------------------------
RECORD_REGIONS = (("c_re", np.float32), ("c_im", np.float32), ("dn", np.float32), ("tx_y", np.float64), ("tx_z", np.float64),
                  ("rx_y", np.float64), ("rx_z", np.float64), ("dop_v", np.float32), ("dop_a", np.float32), ("n_keep", np.int32))


def record_layout(n, P):
    """({name: (byte offset, dtype, shape)}, total bytes): `ws_carve` (dmx_common.h) restated - ten regions in this order,
    each starting at the previous end rounded up to 256 bytes, n * P entries each except n_keep, which has n."""
    off, out = 0, {}
    for name, dt in RECORD_REGIONS:
        shape = (n,) if name == "n_keep" else (n, P)
        out[name] = (off, dt, shape)
        off = -(-(off + int(np.prod(shape)) * np.dtype(dt).itemsize) // 256) * 256
    return out, off


def stage1_records(prep):
    """The record arrays of a PrepResult as host NumPy arrays [n, P] (n_keep: [n]); slots at or past n_keep[u] are
    unspecified."""
    n, P = prep.n_ue, min(int(prep.params_struct.num_paths), prep.n_paths_loaded)
    layout, total = record_layout(n, P)
    assert total == prep.workspace_bytes, (total, prep.workspace_bytes)
    raw = prep.workspace.cpu().numpy()
    out = {}
    for name, (off, dt, shape) in layout.items():
        cnt = int(np.prod(shape))
        out[name] = raw[off:off + cnt * np.dtype(dt).itemsize].view(dt).reshape(shape).copy()
    return out
