"""Stage 1 (k1_path_prep.hip: k1_path_prep<32,true>, <32>, <64>, k1_path_prep_full<32>, <64>) on the GPU, held to its OWN
output: the record arrays in the workspace and every side product, against tests/_stage1_ref.py.

Integers and copies are exact (n_keep, the slot -> path mapping as seen through the copied dn / Doppler terms, num_paths,
los, fov_mask, the delay maximum).  The coefficient is held to 1e-6 of its own magnitude per slot, every steering step and
rotated angle to the spread of the reference under its own rounding perturbation (plus 4 ulp of the spacing for a step).
The cases (tests/_stage1_cases.py) put exact-degree directions - poles, the azimuth branch cut, FoV edges - through every
form, and rows built by hand through the pass loop; undecidable directions were replaced before the rays were built, so
nothing is excluded here.  tests/test_stage1_cases_cpu.py ties the reference to the oracle.
"""
import numpy as np
import pytest

from tests._stage1_cases import (BY_ID, CASES, FC, WANT_SIDES, case_rays, case_reference, case_ue_rot, direct_taken, fov_enabled,
                                 stage1_form_name, stage1_records)

pytestmark = pytest.mark.gpu

STEPS = (("tx_y", "aod"), ("tx_z", "aod"), ("rx_y", "aoa"), ("rx_z", "aoa"))
WORST = {}                                                     # quantity -> (worst ratio to its bound, where)
RAN = {}                                                       # case id -> {want_side: (instantiation, passes)}


def _note(what, ratio, where):
    if ratio > WORST.get(what, (-1.0, ""))[0]:
        WORST[what] = (float(ratio), where)


def _dm_params(c):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(c["bs_shape"]), np.array(c["ue_shape"])
    p.bs_antenna.spacing, p.ue_antenna.spacing = c["bs_spacing"], c["ue_spacing"]
    p.bs_antenna.rotation = np.array(c["bs_rot"])
    p.ue_antenna.rotation = np.array([0, 0, 0]) if c["per_user_rot"] else np.array(c["ue_rot"])
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = c["bs_pattern"], c["ue_pattern"]
    p.num_paths, p.freq_domain = c["num_paths"], c["freq_domain"]
    p.ofdm.subcarriers, p.ofdm.selected_subcarriers = c["subcarriers"], np.array(c["selected"], dtype=np.int64)
    p.ofdm.bandwidth, p.ofdm.rx_filter = c["bandwidth"], c["rx_filter"]
    p.enable_doppler = int(bool(c["doppler"]))
    return p.validate(c["n"])


def _kwargs(c):
    kw = dict(bs_fov=None if c["bs_fov"] is None else np.array(c["bs_fov"]),
              ue_fov=None if c["ue_fov"] is None else np.array(c["ue_fov"]), carrier_freq=FC)
    if c["per_user_rot"]:
        kw["ue_rotation_per_user"] = np.ascontiguousarray(case_ue_rot(c), dtype=np.float64)
    return kw


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _upload(eng, c):
    return eng.upload_rays({k: v.copy() for k, v in case_rays(c).items()})      # the shared rays are read-only


def _prepare(eng, c, want_side, dr=None):
    import torch
    dr = dr or _upload(eng, c)
    prep = eng.prepare(dr, _dm_params(c), want_side=want_side, adaptive_terms=c["adaptive"], **_kwargs(c))
    torch.cuda.synchronize()
    RAN.setdefault(c["id"], {})[want_side] = stage1_form_name(c, want_side)
    return prep


def _same_bits(got, want, what):
    """torch.equal on int32 views of two float32 / int32 host arrays"""
    import torch
    a = torch.from_numpy(np.ascontiguousarray(got)).view(torch.int32)
    b = torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32)
    if not torch.equal(a, b):
        bad = np.argwhere(a.numpy() != b.numpy())
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: "
                             f"{np.asarray(got)[tuple(bad[0])]!r} vs {np.asarray(want)[tuple(bad[0])]!r}")


def _where(c, ref, u, slot, side):
    """The path a slot holds, its input angles and its rotated direction, for a failure message"""
    j = int(ref["slot_path"][u, slot])
    rays = case_rays(c)
    zc, re, im = ref["dir_t" if side == "aod" else "dir_r"]
    return (f"user {u} slot {slot} = path {j}: {side}_el {rays[side + '_el'][u, j]!r} {side}_az {rays[side + '_az'][u, j]!r}, "
            f"(zc, re, im) = ({zc[u, j]!r}, {re[u, j]!r}, {im[u, j]!r})")


def _check_records(c, prep, ref, tag):
    rec = stage1_records(prep)
    _same_bits(rec["n_keep"], ref["n_keep"], f"{tag}: n_keep")
    f = ref["filled"]
    for k in ("dn", "dop_v", "dop_a"):                          # copies: the slot -> path mapping, bit for bit
        _same_bits(np.where(f, rec[k], np.float32(0)), np.where(f, ref[k], np.float32(0)).astype(np.float32), f"{tag}: {k}")
    with np.errstate(invalid="ignore"):                         # slots past n_keep hold whatever the workspace held
        got = rec["c_re"].astype(np.float64) + 1j * rec["c_im"].astype(np.float64)
    nan = np.isnan(ref["c"])
    assert np.array_equal(np.isnan(got)[f], nan[f]), f"{tag}: NaN pattern of c differs"
    ok = f & ~nan
    d, tol = np.abs(got - ref["c"])[ok], ref["tol_c"][ok]
    if d.size:
        ratio = np.where(tol > 0, d / np.where(tol > 0, tol, 1), np.where(d == 0, 0.0, np.inf))
        i = int(np.argmax(ratio))
        u, s = np.argwhere(ok)[i]
        _note("c", ratio[i], f"{tag} user {u} slot {s}")
        assert ratio[i] <= 1.0, (f"{tag}: c of {_where(c, ref, u, s, 'aod')}: |dc| {d[i]:.3e}, bound {tol[i]:.3e}, got {got[u, s]!r}, "
                                 f"want {ref['c'][u, s]!r}")
    for k, side in STEPS:
        d = np.abs(rec[k].astype(np.longdouble) - ref[k]).astype(np.float64)[f]
        tol = ref["tol_" + k][f]
        if d.size:
            ratio = d / tol
            i = int(np.argmax(ratio))
            u, s = np.argwhere(f)[i]
            _note("step " + k, ratio[i], f"{tag} user {u} slot {s}")
            assert ratio[i] <= 1.0, (f"{tag}: {k} of {_where(c, ref, u, s, side)}: |d| {d[i]:.3e}, bound {tol[i]:.3e}, got "
                                     f"{rec[k][u, s]!r}, want {float(ref[k][u, s])!r}")
    return rec


def _check_side(c, prep, ref, want_side, tag):
    side = {k: (None if v is None else v.cpu().numpy()) for k, v in prep.side.items()}
    _same_bits(side["max_delay_key"], np.array([ref["max_delay_key"]], dtype=np.int32), f"{tag}: max_delay_key")
    if not want_side:
        return
    _same_bits(side["num_paths"], ref["num_paths"].astype(np.int32), f"{tag}: num_paths")
    _same_bits(side["los"], ref["los"].astype(np.int32), f"{tag}: los")
    assert (side["fov_mask"] is None) == (ref["fov_mask"] is None)
    if ref["fov_mask"] is not None:
        assert np.array_equal(side["fov_mask"].astype(bool), ref["fov_mask"]) and side["fov_mask"].max() <= 1, \
            f"{tag}: fov_mask differs at {np.argwhere(side['fov_mask'].astype(bool) != ref['fov_mask'])[:4].tolist()}"
    if want_side is not True:
        return
    rays = case_rays(c)
    for k, side_name, kind in (("aod_el_rot", "aod", "el"), ("aod_az_rot", "aod", "az"), ("aoa_el_rot", "aoa", "el"),
                               ("aoa_az_rot", "aoa", "az")):
        got, want, tol = side[k], ref[k], ref[f"tol_{side_name}_{kind}"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{tag}: NaN pattern of {k}"
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        d = np.where(ok, np.abs(got - want), 0.0)               # raw numbers: an azimuth off by 2 pi is an error
        ratio = np.where(ok, d / np.where(tol > 0, tol, 1), 0.0)
        ratio = np.where(ok & (tol == 0) & (d > 0), np.inf, ratio)
        u, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        zc, re, im = ref["dir_t" if side_name == "aod" else "dir_r"]
        msg = (f"{tag}: {k} user {u} path {j}: {side_name}_el {rays[side_name + '_el'][u, j]!r} {side_name}_az "
               f"{rays[side_name + '_az'][u, j]!r}, (zc, re, im) = ({zc[u, j]!r}, {re[u, j]!r}, {im[u, j]!r}): got {got[u, j]!r}, "
               f"want {want[u, j]!r}, bound {tol[u, j]:.3e}")
        _note("angle " + k, ratio[u, j], f"{tag} user {u} path {j}")
        assert ratio[u, j] <= 1.0, msg
        if kind == "az":                                       # on the branch cut the sign is the reference's
            cut = ok & (np.abs(want) == np.pi)
            assert np.array_equal(np.signbit(got[cut]), np.signbit(want[cut])), \
                f"{tag}: {k}: {int((np.signbit(got[cut]) != np.signbit(want[cut])).sum())} of {int(cut.sum())} azimuths on the branch cut have the other sign"
    pl, pw = ref["power_linear"], ref["power_linear_ant_gain"]
    assert side["power_linear"].dtype == np.float32
    np.testing.assert_allclose(side["power_linear"], pl, rtol=1e-6, atol=0, equal_nan=True, err_msg=f"{tag}: power_linear")
    g = side["power_linear_ant_gain"]
    if ref["iso"]:
        np.testing.assert_allclose(g, pw, rtol=2e-6, atol=1e-30, equal_nan=True, err_msg=f"{tag}: power_linear_ant_gain")
    else:                                                      # the bound of tests/test_gpu_parity.py::test_golden
        assert np.array_equal(np.isnan(g), np.isnan(pw))
        err = np.abs(g - pw)
        assert np.all(err[~np.isnan(err)] <= ref["pw_bound"][~np.isnan(err)]), f"{tag}: power_linear_ant_gain"


@pytest.mark.parametrize("want_side", WANT_SIDES, ids=["side_all", "side_light", "side_none"])
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_records_and_side_products(c, want_side):
    eng = _engine()
    ref = case_reference(c)
    prep = _prepare(eng, c, want_side)
    tag = f"{c['id']} [{stage1_form_name(c, want_side)[0]}, {stage1_form_name(c, want_side)[1]} pass(es)]"
    _check_records(c, prep, ref, tag)
    _check_side(c, prep, ref, want_side, tag)


LEAN_AND_FULL = [c for c in CASES if not fov_enabled(c) and c["bs_pattern"] == "isotropic" and c["ue_pattern"] == "isotropic"]


@pytest.mark.parametrize("c", LEAN_AND_FULL, ids=[c["id"] for c in LEAN_AND_FULL])
def test_lean_forms_against_the_full_form(c):
    """No FoV, isotropic: want_side = True runs the FULL form, "light" and False a lean one, on the same uploaded rays.
    Records identical but for the steps, which stay within the reference's bound of each other (the zero-rotation form is
    documented to differ in the last bits of the y steps)."""
    eng = _engine()
    ref = case_reference(c)
    dr = _upload(eng, c)
    assert stage1_form_name(c, True)[0].startswith("k1_path_prep_full") and not stage1_form_name(c, False)[0].startswith("k1_path_prep_full")
    full, light, lean = (_prepare(eng, c, w, dr) for w in WANT_SIDES)
    rf, rl, rn = (stage1_records(p) for p in (full, light, lean))
    f = ref["filled"]
    for other, name in ((rl, "light"), (rn, "none")):
        _same_bits(other["n_keep"], rf["n_keep"], f"{c['id']} {name}: n_keep")
        for k in ("dn", "c_re", "c_im", "dop_v", "dop_a"):
            _same_bits(np.where(f, other[k], np.float32(0)), np.where(f, rf[k], np.float32(0)), f"{c['id']} {name}: {k}")
        for k, _ in STEPS:
            d, tol = np.abs(other[k] - rf[k])[f], ref["tol_" + k][f]
            if d.size:
                _note("lean - full " + k, float((d / tol).max()), c["id"])
                assert np.all(d <= tol), f"{c['id']} {name}: {k} differs from the FULL form by {d.max():.3e}"
    import torch
    for k in ("num_paths", "los"):
        assert torch.equal(light.side[k], full.side[k]), k
    for p in (light, lean):
        assert torch.equal(p.side["max_delay_key"], full.side["max_delay_key"])


def test_direct_scope_is_the_restated_one():
    eng = _engine()
    for c in CASES:
        dr = _upload(eng, c)
        assert eng.direct_supported(dr, _dm_params(c), adaptive_terms=c["adaptive"], **_kwargs(c)) == direct_taken(c), c["id"]


DIRECT = [c for c in CASES if c["kind"] == "struct" and direct_taken(c)]


@pytest.mark.parametrize("c", DIRECT, ids=[c["id"] for c in DIRECT])
def test_single_pass_side_products(c):
    """dmx_channels_fd_direct runs stage1_path too: its light side products are those of prepare(want_side="light")"""
    import torch
    eng = _engine()
    ref = case_reference(c)
    dr = _upload(eng, c)
    prep = _prepare(eng, c, "light", dr)
    _, side = eng.channels_direct(dr, _dm_params(c), want_side="light", **_kwargs(c))
    torch.cuda.synchronize()
    for k in ("los", "num_paths", "fov_mask", "max_delay_key"):
        assert (side.get(k) is None) == (prep.side.get(k) is None), k
        if side.get(k) is not None:
            assert torch.equal(side[k], prep.side[k]), f"{c['id']}: {k}"
    _same_bits(side["num_paths"].cpu().numpy(), ref["num_paths"].astype(np.int32), "num_paths")
    _same_bits(side["los"].cpu().numpy(), ref["los"].astype(np.int32), "los")


def test_zz_report():
    """Last in the file: the worst ratio to each bound over what ran, and the instantiation / pass count of each case
    (BASELINE.md quotes them)."""
    for what, (ratio, where) in sorted(WORST.items()):
        print(f"stage 1, {what}: worst ratio to the bound {ratio:.3e} ({where})")
        assert ratio <= 1.0
    for cid, forms in RAN.items():
        print(f"stage 1 case {cid}: " + "; ".join(f"want_side={w!r}: {f} x{p}" for w, (f, p) in forms.items()))
    assert BY_ID
