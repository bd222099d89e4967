"""Case table and inputs shared by tests/test_angle_delay_cpu.py and tests/test_gpu_angle_delay.py.  A plain module: NumPy
and the oracle only, no torch, no GPU.  The case dictionaries have the form of tests/test_gpu_fd_direct.py `_case` (its
`_dm_params` / `_kwargs` take them), with three more keys: `n_fft`, `n_taps` and `rows` - "dft" (dm.dft_codebook of the BS
panel), "ant" (no codebook: the BS elements), ("rand", R) (R random complex rows) or "identity" (an identity codebook).
"""
from __future__ import annotations

import numpy as np

from tests import _consumer_shapes as shapes
from tests._angle_delay_ref import adp_from_channel, adp_from_paths, dft_codebook
from tests._cases import fov_args, oracle_params
from tests._path_count_cases import flat

FC = 28e9
RC = 32                 # rows of the row table per LDS chunk (k9_angle_delay.hip AD_RC)
TAP_CHUNK = 64          # taps per chunk of w
LDS_MAX = 159744        # 156 KB: what one wave can get (dmx_common.h WAVE_LDS_MAX)
POW2_BW = float(2 ** 24)   # a bandwidth whose sample time is a power of two: delay / ts is exact in float32


def lds_rule(ue_shape, n_rows, n_taps, P):
    """waves per workgroup (4, 2, 1; 0 = refused) from the LDS bytes of one wave: the launcher's rule, restated"""
    b = (int(np.prod(ue_shape)) + min(n_rows, RC) + min(n_taps, TAP_CHUNK)) * P * 8
    return 4 if 4 * b <= 65536 else 2 if 2 * b <= 65536 else 1 if b <= LDS_MAX else 0


def _case(cid, n, L, bs, ue, N, sel, n_fft, n_taps, rows, **kw):
    d = dict(id=cid, n=n, L=L, bs_shape=bs, ue_shape=ue, subcarriers=N, selected=list(sel), num_paths=kw.pop("num_paths", L),
             bs_rot=[0, 0, 0], ue_rot=[0, 0, 0], bs_pattern="isotropic", ue_pattern="isotropic", bs_fov=None, ue_fov=None,
             bs_spacing=0.5, ue_spacing=0.37, bandwidth=20e6, freq_domain=1, rx_filter=0, doppler=None, all_valid=False,
             max_delay=2e-6, rays="plain", per_user_rot=False, adaptive=False, n_fft=n_fft, n_taps=n_taps, rows=rows)
    d.update(kw)
    return d


def _both(cs, cid, *a, **kw):
    """a selection with the DFT codebook and with antenna rows"""
    cs.append(_case(cid + "_dft", *a, "dft", **kw))
    cs.append(_case(cid + "_ant", *a, "ant", **kw))


def _cases():
    cs = []
    # DeepMIMO's default arrays: 8 rows under two slices
    _both(cs, "defaults_K64", 40, 25, [8, 1], [1, 1], 512, range(64), 64, 32)
    _both(cs, "defaults_K512", 40, 25, [8, 1], [1, 1], 512, range(512), 512, 32)
    # tap counts: one tap of one subcarrier; the slice count changes between 32 and 33 taps, 31 and 33 leave lanes idle; 65 is a
    # second tap chunk of one tap; the full grid
    _both(cs, "taps1", 23, 25, [4, 2], [2, 1], 512, [7], 1, 1)
    for T in (31, 32, 33, 64, 65, 128):
        _both(cs, f"taps{T}", 17, 25, [4, 2], [2, 1], 512, range(128), 128, T)
    # zero padding and the selection's first index and stride
    _both(cs, "pad_K40_d8_s3", 33, 25, [4, 2], [2, 1], 512, range(3, 3 + 8 * 40, 8), 64, 24)
    _both(cs, "s0_minus5", 33, 25, [4, 2], [2, 1], 512, range(-5, 59), 64, 32)
    _both(cs, "s0_40001", 33, 25, [4, 2], [2, 1], 512, range(40001, 40001 + 64), 64, 32)
    # rows: codebooks around the chunk of RC rows, antenna rows on a small and on a two-chunk panel, identity against antenna
    for R in (1, 3, RC - 1, RC, RC + 1, 2 * RC + 1):
        bs = [4, 2] if R <= 3 else [8, 4]
        cs.append(_case(f"rows{R}", 13, 25, bs, [2, 1], 512, range(64), 64, 32, ("rand", R)))
    cs.append(_case("ant_8x8", 13, 25, [8, 8], [2, 1], 512, range(64), 64, 32, "ant"))
    cs.append(_case("identity_4x2", 29, 25, [4, 2], [2, 1], 512, range(64), 64, 32, "identity"))
    cs.append(_case("identity_4x2_ant", 29, 25, [4, 2], [2, 1], 512, range(64), 64, 32, "ant"))
    for ue in ([1, 1], [2, 1], [3, 1], [2, 2], [4, 2]) + shapes.ANGLE_DELAY_UE:      # every M_rx the kernel is instantiated for
        cs.append(_case(f"mrx{ue[0] * ue[1]}", 19, 25, [4, 2], ue, 512, range(64), 64, 32, "dft"))
    # antenna rows of an odd BS panel (15 rows, bs_mh = 5) under a UE whose first dimension is neither 1 nor M_rx
    cs.append(_case(shapes.ANGLE_DELAY_ODD_TX, 13, 25, [5, 3], [3, 2], 512, range(64), 64, 32, "ant"))
    # every kept-path count 0 .. 32 (tests/_consumer_shapes.py), on that table's selection of three subcarriers
    ec = shapes.EVERY_COUNT
    cs.append(_case(shapes.ANGLE_DELAY_EVERY_COUNT, ec["n"], ec["L"], ec["bs_shape"], ec["ue_shape"], 512, ec["selected"], 64, 32, "ant",
                    num_paths=ec["num_paths"], rays="every_count"))
    # path counts
    _both(cs, "counts_and_holes", 45, 25, [4, 2], [2, 1], 512, range(64), 64, 32, rays="counts")
    # one loaded path: its delay inside the tap window (28 of 32 samples) - outside it a user keeps nothing but one sidelobe,
    # 1.5 % of the path, and the complex64 rounding of the oracle's own tensor is then above 1e-2 of that user's bound
    _both(cs, "L1", 50, 1, [4, 2], [1, 1], 64, range(64), 64, 32, max_delay=1.4e-6)
    _both(cs, "P32_num_paths_below_loaded", 19, 40, [4, 2], [2, 1], 256, range(64), 64, 32, num_paths=32, all_valid=True)
    _both(cs, "P32_num_paths_above_loaded", 19, 32, [4, 2], [2, 1], 256, range(64), 64, 32, num_paths=40, all_valid=True)
    # on a tap and beside it; the equal-power inputs whose delays the tap window covers
    _both(cs, "on_tap", 10, 3, [4, 2], [2, 1], 512, range(512), 512, 32, rays="on_tap", bandwidth=POW2_BW)
    _both(cs, "equal_power", 31, 25, [4, 2], [2, 1], 512, range(512), 512, 32, rays="flat", max_delay=1.4e-6, all_valid=True)
    # stage-1 features arrive through the records: the parameters of tests/test_gpu_rate.py
    cs.append(_case("rot_fov_dipole", 53, 25, [4, 2], [1, 1], 512, range(64), 64, 32, "dft", bs_rot=[5, -20, 60], ue_rot=[10, 20, 30],
                    bs_fov=[150, 110], ue_fov=[200, 100], bs_pattern="halfwave-dipole", ue_pattern="halfwave-dipole"))
    cs.append(_case("per_user_rot", 45, 25, [8, 1], [2, 2], 512, range(64), 64, 32, "ant", per_user_rot=True))
    cs.append(_case("doppler", 37, 25, [4, 2], [2, 1], 64, range(64), 64, 32, "dft", doppler=1))
    cs.append(_case("adaptive_workspace", 61, 25, [8, 4], [2, 1], 512, range(0, 192, 3), 64, 32, "dft", adaptive=True))
    # launch residue: 4k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 2-wave shape (the rule has no 1-wave shape)
    for n in (41, 42, 43):
        cs.append(_case(f"wpb4_users{n}", n, 25, [8, 1], [1, 1], 512, range(64), 64, 32, "dft"))
    cs.append(_case("wpb2_users7", 7, 32, [8, 4], [4, 2], 512, range(128), 128, 64, "dft", all_valid=True))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}


def live_counts(n, L):
    """live paths per user, cycled: 0, 1, 2, L - 1, L (tests/test_gpu_rate.py)"""
    return [min(L, (0, 1, 2, L - 1, L)[u % 5]) for u in range(n)]


def on_tap_delays():
    """[10, 3] sample delays: the first path of a user sits exactly on tap 0, 5 or 31, one float32 ulp beside tap 5 on either
    side, 1e-4 of a sample beside it or halfway between two taps; the other two lie elsewhere inside the window"""
    five = np.float32(5)
    first = [0.0, 5.0, 31.0, np.nextafter(five, np.float32(6)), np.nextafter(five, np.float32(4)), np.float32(5 + 1e-4), 5.5,
             5.0, 0.0, 31.0]
    second = [12.25, 17.5, 3.75, 20.0, 9.0, 26.5, 14.0, 5.0, 31.0, 0.0]     # users 7 .. 9: two or three paths exactly on taps
    third = [22.0, 28.125, 11.0, 13.5, 24.75, 2.0, 30.0, 6.0, 5.0, 30.0]
    return np.array([first, second, third], np.float32).T


def case_rays(c):
    from oracle import oracle_np as onp
    kind = c["rays"]
    if kind == "every_count":
        return shapes.every_count_rays(c)
    if kind == "counts":                                        # tests/test_gpu_rate.py `_case_rays`
        rays = onp.synth_rays(c["n"], c["L"], seed=900 + c["n"], all_valid=True, max_delay=c["max_delay"])
        keys = [k for k in rays if k not in ("rx_pos", "tx_pos")]
        rng = np.random.default_rng(4)
        for u, cnt in enumerate(live_counts(c["n"], c["L"])):
            hole = np.zeros(c["L"], bool)
            hole[cnt:] = True
            if cnt == c["L"] and u % 2:
                hole[rng.choice(c["L"], size=3, replace=False)] = True
            for k in keys:
                rays[k][u, hole] = np.nan
        return rays
    rays = onp.synth_rays(c["n"], c["L"], seed=500 + c["n"] + c["L"], all_valid=c["all_valid"] or kind in ("on_tap", "flat"),
                          max_delay=c["max_delay"], with_doppler=c["doppler"] is not None)     # tests/test_gpu_fd_direct.py `_rays`
    if kind == "flat":
        rays = flat(rays, 31)                                     # every power in [-66, -60] dB
    if kind == "on_tap":
        rays["power"][:] = np.float32(-60)
        rays["delay"][:] = on_tap_delays() / np.float32(c["bandwidth"])      # exact: the sample time is 2^-24 s
    return rays


def case_ue_rot(c):
    if not c["per_user_rot"]:
        return np.array(c["ue_rot"])
    return np.random.default_rng(11).uniform(-180, 180, (c["n"], 3))


def case_codebook(c):
    """the codebook of a case, complex128 [R, M_tx], or None for antenna rows"""
    rows, m_tx = c["rows"], c["bs_shape"][0] * c["bs_shape"][1]
    if rows == "ant":
        return None
    if rows == "dft":
        return dft_codebook(c["bs_shape"])
    if rows == "identity":
        return np.eye(m_tx, dtype=np.complex128)
    R = rows[1]
    rng = np.random.default_rng(40 + R)
    return (rng.normal(size=(R, m_tx)) + 1j * rng.normal(size=(R, m_tx))) / np.sqrt(2 * m_tx)


def _oracle_args(c, rays, ue_rot):
    op = oracle_params(c, ue_rot)
    bs_fov, ue_fov = fov_args(c)
    if bs_fov is not None or ue_fov is not None:
        bs_fov = np.array([360, 180]) if bs_fov is None else bs_fov
        ue_fov = np.array([360, 180]) if ue_fov is None else ue_fov
    dop = None
    if c["doppler"]:
        op["enable_doppler"] = 1
        dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC)
    return op, bs_fov, ue_fov, dop


_INPUTS = {}


def case_inputs(c):
    """(rays, ue_rot, codebook, X_ref by the definition from the oracle's tensor, X by the closed form, per-path factors) of a
    case: computed once, shared and left unchanged"""
    if c["id"] not in _INPUTS:
        from oracle import oracle_np as onp
        rays, ue_rot, F = case_rays(c), case_ue_rot(c), case_codebook(c)
        op, bs_fov, ue_fov, dop = _oracle_args(c, rays, ue_rot)
        H = onp.compute_channels(rays, op, bs_fov=bs_fov, ue_fov=ue_fov, doppler=dop)["channel"]
        X_ref = adp_from_channel(H, F, c["n_fft"], c["n_taps"])
        X_cf, facs = adp_from_paths(rays, op, F, c["n_fft"], c["n_taps"], bs_fov=bs_fov, ue_fov=ue_fov, doppler=dop)
        X_ref.setflags(write=False)
        X_cf.setflags(write=False)
        _INPUTS[c["id"]] = (rays, ue_rot, F, X_ref, X_cf, facs)
    return _INPUTS[c["id"]]
