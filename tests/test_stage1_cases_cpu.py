"""The stage-1 reference and case list (tests/_stage1_ref.py, tests/_stage1_cases.py) checked without a GPU: the reference
against oracle_np.prepare_paths bit for bit, the channel rebuilt from its records against oracle_np.compute_channels, the
caps on dropped lattice points, which kernel forms and hand-built situations the case list reaches, the workspace layout
against the library's own byte count, and the keep rule on the hand-built users as literals."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import _stage1_ref as s1
from tests._cases import assert_channel_close, assert_taps_close
from tests._stage1_cases import (BY_ID, CAP_ALL, CAP_ANY, CASES, EDGE_USERS, EQUAL_HOLES, EQUAL_PATHS, FIRST_IN_FOV, FOVS,
                                 HAND_USERS, LATTICE_CASES, N_LAT, ROTATIONS, SINGLE_NAN_FIELDS, STRUCT_CASES, WANT_SIDES,
                                 case_dropped, case_rays, case_reference, case_ue_rot, clip_edge_delays, direct_taken,
                                 fov_enabled, oracle_fovs, oracle_params, record_layout, stage1_form_name, undecidable_rays)

IDS = [c["id"] for c in CASES]


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_side_products_are_the_oracles(c):
    """The same arithmetic, so the same bits: angles (rows that are exactly +-pi included), mask, powers, counts, LoS"""
    rays, ref = case_rays(c), case_reference(c)
    bs_fov, ue_fov = oracle_fovs(c)
    want = onp.prepare_paths(rays, oracle_params(c), bs_fov, ue_fov)
    for k in ("aod_el_rot", "aod_az_rot", "aoa_el_rot", "aoa_az_rot"):
        assert _bits_equal(ref[k], want["_" + k]), k
    assert (ref["fov_mask"] is None) == (want["_fov_mask"] is None)
    if ref["fov_mask"] is not None:
        assert np.array_equal(ref["fov_mask"], want["_fov_mask"])
    assert _bits_equal(ref["power_linear"], want["power_linear"])
    assert _bits_equal(ref["power_linear_ant_gain"], want["_power_linear_ant_gain"])
    assert np.array_equal(ref["num_paths"], want["num_paths"]) and np.array_equal(ref["los"], want["los"])
    ut, ur = undecidable_rays(c, rays)
    assert not ut.any() and not ur.any(), "an undecidable direction reached the rays"


def test_branch_cut_azimuths_are_plus_pi():
    """Zero rotation, azimuth 0 and an elevation whose float32 sine is negative: im = -0.0, re < 0, and the reference's
    azimuth is +pi (np.angle of a complex built from the parts), not atan2's -pi"""
    c = BY_ID["lat_zero_nofov"]
    rays, ref = case_rays(c), case_reference(c)
    zc, re, im = ref["dir_t"]
    cut = (rays["aod_az"] == 0) & np.isin(rays["aod_el"], (180.0, 195.0))
    assert cut.sum() >= 2
    assert np.all(np.signbit(im[cut]) & (im[cut] == 0) & (re[cut] < 0))
    assert np.all(ref["aod_az_rot"][cut] == np.pi) and np.all(np.arctan2(im[cut], re[cut]) == -np.pi)
    for k in ("aod_az_rot", "aoa_az_rot"):
        assert (np.abs(ref[k]) == np.pi).sum() >= 2


@pytest.mark.parametrize("c", [c for c in CASES if not c["rx_filter"]], ids=[c["id"] for c in CASES if not c["rx_filter"]])
def test_channel_from_the_reference_records(c):
    """What the records mean: their direct sum is the oracle's channel, in both domains"""
    rays, ref = case_rays(c), case_reference(c)
    bs_fov, ue_fov = oracle_fovs(c)
    dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=c["fc"]) if c["doppler"] else None
    want = onp.compute_channels(rays, oracle_params(c), bs_fov=bs_fov, ue_fov=ue_fov, doppler=dop)
    H = s1.channel_from_records(ref, c).astype(np.complex64)
    if c["freq_domain"]:
        assert_channel_close(H, want["channel"], what=c["id"])
        assert ref["max_delay_key"] == s1.max_delay_key(np.array([want["max_delay"]]))
    else:
        assert_taps_close(H, want["channel"], what=c["id"])


def test_rx_filter_leaves_the_doppler_rotation_to_stage_two():
    a, b = BY_ID["st_doppler"], BY_ID["st_doppler_lpf"]
    plain = s1.stage1_reference(dict(b, doppler=0), case_rays(b), case_ue_rot(b))
    got = case_reference(b)
    assert np.array_equal(got["c"], plain["c"]) and np.array_equal(got["slot_path"], plain["slot_path"])
    assert np.array_equal(got["dop_v"], np.take_along_axis(case_rays(b)["doppler_vel"], np.where(got["filled"], got["slot_path"], 0), 1))
    rot = case_reference(a)
    f = rot["filled"]
    assert np.abs(rot["c"] - s1.stage1_reference(dict(a, doppler=0), case_rays(a), case_ue_rot(a))["c"])[f].max() > 0


def test_dropped_lattice_points_stay_under_the_caps():
    total, seen, worst = 0, 0, (0.0, "")
    for c in LATTICE_CASES:
        for side, d in zip(("aod", "aoa"), case_dropped(c)):
            share = d / N_LAT
            assert share <= CAP_ANY, f"{c['id']} {side}: {d} of {N_LAT} lattice points dropped"
            worst = max(worst, (share, f"{c['id']} {side}"))
            total, seen = total + d, seen + N_LAT
    print(f"dropped lattice points: {total} of {seen} = {total / seen:.4f} overall; worst {worst[1]} {worst[0]:.4f}")
    assert total / seen <= CAP_ALL


def test_lattice_configurations_cover_the_lists():
    rots = [c["bs_rot"] for c in LATTICE_CASES] + [c["ue_rot"] for c in LATTICE_CASES]
    assert all(r in rots for r in ROTATIONS)
    fovs = [c["bs_fov"] for c in LATTICE_CASES] + [c["ue_fov"] for c in LATTICE_CASES]
    assert all(f in fovs for f in FOVS)
    assert any(c["bs_fov"] and not c["ue_fov"] for c in LATTICE_CASES) and any(c["ue_fov"] and not c["bs_fov"] for c in LATTICE_CASES)
    assert any(c["bs_fov"] and c["ue_fov"] for c in LATTICE_CASES)
    assert any(c["per_user_rot"] and c["ue_fov"] for c in LATTICE_CASES)
    assert any(c["bs_pattern"] != "isotropic" for c in LATTICE_CASES) and any(c["ue_pattern"] != "isotropic" for c in LATTICE_CASES)
    for c in LATTICE_CASES:                                     # every lattice direction is in the rays of a no-drop case
        assert c["n"] * c["L"] >= N_LAT


def test_case_list_reaches_every_form_and_pass_count():
    reached = {stage1_form_name(c, w) for c in CASES for w in WANT_SIDES}
    forms = {f for f, _ in reached}
    assert forms == {"k1_path_prep<32,true>", "k1_path_prep<32>", "k1_path_prep<64>", "k1_path_prep_full<32>",
                     "k1_path_prep_full<64>"}
    for f in ("k1_path_prep<64>", "k1_path_prep_full<64>"):
        assert {p for g, p in reached if g == f} == {1, 2, 3}, f
    # with a FoV on the multi-pass forms, and num_paths cutting inside the second pass
    assert {c["L"] for c in STRUCT_CASES} >= {1, 25, 32, 33, 64, 65, 70, 128, 130}
    assert {c["n"] for c in STRUCT_CASES} >= {1, 7, 37}
    assert any(c["L"] == 70 and c["num_paths"] == p for c in STRUCT_CASES for p in (64,))
    assert any(c["L"] == 70 and c["num_paths"] == 65 for c in STRUCT_CASES)
    assert any(c["num_paths"] > c["L"] for c in STRUCT_CASES) and any(c["num_paths"] == 10 < c["L"] for c in STRUCT_CASES)
    assert any(fov_enabled(c) and c["L"] > 128 for c in STRUCT_CASES)
    assert any(direct_taken(c) and fov_enabled(c) and c["L"] > 32 for c in STRUCT_CASES)
    assert any(c["adaptive"] and c["L"] <= 64 for c in STRUCT_CASES) and any(c["adaptive"] and c["L"] > 64 for c in STRUCT_CASES)
    assert any(c["doppler"] and c["rx_filter"] for c in STRUCT_CASES) and any(c["doppler"] and not c["rx_filter"] for c in STRUCT_CASES)
    assert any(not c["freq_domain"] for c in LATTICE_CASES) and any(not c["freq_domain"] for c in STRUCT_CASES)


def test_form_rule_follows_the_launcher_text():
    """`stage1_form_name` restates stage1_form / launch_path_prep; the lines it restates are still there"""
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "csrc")
    math_h = open(os.path.join(root, "k1_path_math.h")).read()
    prep = open(os.path.join(root, "k1_path_prep.hip")).read()
    assert "bool zrot = !prm.ue_rotation_per_user && n_paths_loaded <= 32;" in math_h
    assert "const bool lean = !stage1_need_angles(prm, side) && !side.power_linear && !side.power_linear_ant_gain && !side.fov_mask;" in math_h
    assert "const bool two = rays.n_paths <= 32;" in prep
    assert "two ? k1_path_prep_full<32> : k1_path_prep_full<64>" in prep
    assert "!two ? k1_path_prep<64> : (form == STAGE1_LEAN_ZROT ? k1_path_prep<32, true> : k1_path_prep<32>)" in prep
    assert "const bool sorted = a.sort_paths && L <= LPU;" in prep


@pytest.mark.parametrize("n,P,L", [(1, 1, 1), (7, 25, 25), (37, 10, 25), (7, 65, 70), (13, 25, 40), (64, 1, 5), (3, 21, 21), (0, 25, 25)])
def test_record_layout_is_the_librarys(n, P, L):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from deepmimo_amd import _native as nat
    p = nat.DmxParams()
    p.num_paths = P
    layout, total = record_layout(n, min(P, L))
    assert total == nat.load().dmx_workspace_bytes(C.byref(p), n, L)
    assert all(off % 256 == 0 for off, _, _ in layout.values())
    assert [k for k in layout] == ["c_re", "c_im", "dn", "tx_y", "tx_z", "rx_y", "rx_z", "dop_v", "dop_a", "n_keep"]


def test_record_layout_cases_include_unaligned_regions():
    assert (7 * 25 * 4) % 256 and (37 * 10 * 4) % 256 and (3 * 21 * 4) % 256 and (64 * 1 * 4) % 256 == 0


# ---- the hand-built users ------------------------------------------------------------------------------------------
def test_hand_built_fov_users():
    c = BY_ID["st_hand_L130"]
    rays, ref = case_rays(c), case_reference(c)
    m, P = ref["fov_mask"], ref["P"]
    assert P == 100 and ref["L"] == 130
    who = {w if k is None else (w, k): u for u, (w, k) in enumerate(HAND_USERS)}
    for k in FIRST_IN_FOV:
        u = who[("first_in_fov", k)]
        assert m[u].any() and int(np.argmax(m[u])) == k
        assert ref["los"][u] == (0 if u % 2 else 1)             # the other paths carry the opposite interaction code
        assert ref["n_keep"][u] == max(0, P - k) and ref["num_paths"][u] == 130 - k
    u = who["none_in_fov"]
    assert not m[u].any() and ref["los"][u] == -1 and ref["n_keep"][u] == 0 and ref["num_paths"][u] == 0
    u = who["first_hole"]
    assert not m[u, 0] and m[u, 1] and ref["los"][u] == 1 and ref["n_keep"][u] == 99 and ref["slot_path"][u, 0] == 1
    u = who["all_holes"]
    assert ref["los"][u] == -1 and ref["n_keep"][u] == 0 and ref["num_paths"][u] == 0
    u = who["holes_pass1"]
    assert ref["n_keep"][u] == 93 and list(ref["slot_path"][u, :3]) == [1, 2, 5] and ref["slot_path"][u, 92] == 99
    u = who["holes_pass2"]
    assert ref["n_keep"][u] == 96 and list(ref["slot_path"][u, 63:67]) == [63, 66, 67, 68] and ref["num_paths"][u] == 124
    u = who["delay_all_nan"]
    assert ref["n_keep"][u] == 0 and ref["num_paths"][u] == 130
    # the maximum sits in the second pass of one user; the larger delay past num_paths does not count
    assert rays["delay"][who["max_delay_pass2"], 70] == np.float32(2.5e-6)
    assert np.nanmax(rays["delay"]) == np.float32(3.0e-6) and np.nanargmax(rays["delay"][who["max_delay_past_P"]]) == 110
    assert s1.decode_max_delay(ref["max_delay_key"]) == np.float32(2.5e-6)
    td = case_reference(BY_ID["st_hand_L130_td"])
    assert td["n_keep"][who["delay_all_nan"]] == 100 and td["n_keep"][who["none_in_fov"]] == 100
    assert np.all(td["c"][who["none_in_fov"]] == 0)             # outside the FoV: the slot is kept with a zero coefficient
    assert case_reference(BY_ID["st_all_delay_nan"])["max_delay_key"] == 0


def test_single_field_nan_users_literals():
    """User order: power, phase, delay, aoa_az, aod_el, inter on path 0; the last user is whole.  P = L = 25."""
    assert SINGLE_NAN_FIELDS == ("power", "phase", "delay", "aoa_az", "aod_el", "inter")
    fov, lean, td = (case_reference(BY_ID[k]) for k in ("st_single_nan_fov", "st_single_nan_lean", "st_single_nan_td"))
    for r in (fov, lean):                                      # frequency domain: any NaN factor drops the path
        assert list(r["n_keep"]) == [24, 24, 24, 24, 24, 25, 25]
        assert [int(v) for v in r["slot_path"][:, 0]] == [1, 1, 1, 1, 1, 0, 0]
    assert list(td["n_keep"]) == [24, 25, 25, 25, 25, 25, 25]   # time domain: "valid" is the power alone
    assert np.isnan(td["c"][1, 0]) and td["c"][3, 0] == 0 and td["c"][4, 0] == 0 and td["c"][2, 0] != 0
    # the path count follows the rotated AoA azimuth (after the FoV): with a BS FoV a NaN AoD masks the path too
    assert list(lean["num_paths"]) == [25, 25, 25, 24, 25, 25, 25]
    assert list(fov["num_paths"]) == [25, 25, 25, 24, 24, 25, 25]
    assert list(fov["fov_mask"][:, 0]) == [True, True, True, True, False, True, True]
    # LoS: the first path's code (0) where it is in the FoV, the next one's (2) where it is not; NaN code -> 0
    assert list(lean["los"]) == [1, 1, 1, 1, 1, 0, 1]
    assert list(fov["los"]) == [1, 1, 1, 1, 0, 0, 1]
    # the delay maximum ignores only the NaN delay itself
    rays = case_rays(BY_ID["st_single_nan_lean"])
    assert s1.decode_max_delay(lean["max_delay_key"]) == np.nanmax(rays["delay"])


def test_value_edge_users_literals():
    assert EDGE_USERS == ("power_minus_inf", "clip_edge", "weak_path", "equal_powers")
    c = BY_ID["st_edges"]
    fd, srt, td = (case_reference(BY_ID[k]) for k in ("st_edges", "st_edges_sorted", "st_edges_td"))
    d = clip_edge_delays(c)
    dn = d / np.float32(1.0 / c["bandwidth"])
    assert dn.dtype == np.float32 and dn.tolist() == [63.999996185302734, 64.0, 64.00000762939453]
    # frequency domain: -inf dBW is a zero coefficient (dropped); dn >= N is clipped to a zero coefficient (dropped)
    assert list(fd["n_keep"]) == [24, 23, 25, 22, 25, 25, 25] and list(srt["n_keep"]) == list(fd["n_keep"])
    assert list(fd["slot_path"][1, :2]) == [0, 3] and fd["dn"][1, 0] == np.float32(63.999996)
    # time domain: both keep their slot
    assert list(td["n_keep"]) == [25, 25, 25, 22, 25, 25, 25] and td["c"][0, 3] == 0 and td["c"][1, 1] != 0
    # amplitude order: equal coefficients fall back on the path index, holes between them take no slot
    pos = [int(np.flatnonzero(srt["slot_path"][3] == j)[0]) for j in EQUAL_PATHS]
    assert pos == list(range(pos[0], pos[0] + 4)) and not np.isin(srt["slot_path"][3], EQUAL_HOLES).any()
    assert len(set(srt["c"][3, pos])) == 1
    assert srt["slot_path"][2, 24] == 7                         # the -300 dBW path is the weakest
    assert np.array_equal(np.sort(srt["slot_path"], axis=1), np.sort(fd["slot_path"], axis=1))   # the same paths, reordered


@pytest.mark.parametrize("c", [c for c in CASES if c["adaptive"]], ids=[c["id"] for c in CASES if c["adaptive"]])
def test_amplitude_order_has_no_near_ties(c):
    """The kernel orders by the float32 |c|^2; the reference's order is the same wherever neighbours differ by more than the
    float32 noise of that key (4e-7) or are exactly equal"""
    ref = case_reference(c)
    key = np.abs(ref["c"]) ** 2
    sorted_case = c["freq_domain"] and c["L"] <= 64
    for u in range(ref["n"]):
        k = key[u, :ref["n_keep"][u]]
        if sorted_case:
            assert np.all(np.diff(k) <= 0)
            ratio = k[1:] / k[:-1]
            assert np.all((ratio == 1.0) | (ratio < 1 - 1e-5))
        else:
            assert np.all(np.diff(ref["slot_path"][u, :ref["n_keep"][u]]) > 0)
    if sorted_case:
        assert any(np.any(np.diff(ref["slot_path"][u, :ref["n_keep"][u]]) < 0) for u in range(ref["n"]))


@pytest.mark.parametrize("cid", ["lat_zero_nofov", "lat_zero_bs180", "lat_y180_bs0", "lat_ue_zero_180"])
def test_c_oracle_follows_np_angle_at_poles_and_on_the_branch_cut(cid):
    """oracle/oracle_c.c restates np.angle(re + 1j * im) with its zeros: the azimuth at a pole (re = -0) is 0 and on the
    branch cut (im = -0) +pi, and the FoV masks that follow are the NumPy oracle's"""
    from oracle import oracle_c as oc
    c = BY_ID[cid]
    rays, ref = case_rays(c), case_reference(c)
    bs_fov, ue_fov = oracle_fovs(c)
    got = oc.compute_channels(rays, oracle_params(c), bs_fov=bs_fov, ue_fov=ue_fov)
    for k, tol in (("aod_az_rot", "tol_aod_az"), ("aoa_az_rot", "tol_aoa_az")):
        assert np.all(np.abs(got["_" + k] - ref[k]) <= ref[tol]), k
        cut = np.abs(ref[k]) == np.pi
        assert cut.any() and np.array_equal(np.signbit(got["_" + k][cut]), np.signbit(ref[k][cut]))
    if ref["fov_mask"] is not None:
        assert np.array_equal(got["_fov_mask"], ref["fov_mask"])
    assert np.array_equal(got["num_paths"], ref["num_paths"]) and np.array_equal(got["los"], ref["los"])
