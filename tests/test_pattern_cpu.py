"""Host side of the TR 38.901 sector element pattern ("tr38901", DMX_PATTERN_TR38901 = 2) - no GPU: the id in the header and
in the binding, the name in the parameter validation, the host-only queries of the library on ids 2 / 3 / 7 / -1, and
`dm.pattern_gain` against closed-form points and against the independent restatement of tests/_pattern_ref.py.
tests/test_gpu_pattern.py runs the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _pattern_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepmimo_amd", "lib", "libdeepmimo_amd.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

DEG = np.pi / 180.0
G0 = 10.0 ** 0.8                                  # 8 dBi
FLOOR = 10.0 ** -2.2                              # 8 - 30 dBi


def _db(g):
    return 10.0 * np.log10(g)


def test_header_define_and_binding_ids():
    from deepmimo_amd import _native as nat, consts
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DMX_PATTERN_(\w+)\s+(-?\d+)", hdr)}
    assert ids == {"ISOTROPIC": 0, "HALFWAVE_DIPOLE": 1, "TR38901": 2}
    assert nat.PATTERN_IDS == {"isotropic": 0, "halfwave-dipole": 1, "tr38901": 2}
    assert consts.PARAMSET_ANT_RAD_PAT_VALS == ["isotropic", "halfwave-dipole", "tr38901"]
    assert re.search(r"#define\s+DMX_ABI_VERSION\s+3\b", hdr) and nat.ABI_VERSION == 3


def test_pattern_gain_is_exported():
    import deepmimo_amd as dm
    from deepmimo_amd import geometry
    assert "pattern_gain" in dm.__all__ and dm.pattern_gain is geometry.pattern_gain


@pytest.mark.parametrize("bs,ue", [("tr38901", "isotropic"), ("isotropic", "tr38901"), ("tr38901", "halfwave-dipole"),
                                   ("tr38901", "tr38901")])
def test_validate_accepts_the_name_on_either_side(bs, ue):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = bs, ue
    q = p.validate(4)
    assert q.bs_antenna.radiation_pattern == bs and q.ue_antenna.radiation_pattern == ue


@pytest.mark.parametrize("side", ["bs_antenna", "ue_antenna"])
@pytest.mark.parametrize("name", ["yagi", "patch", "TR38901"])
def test_validate_still_refuses_other_names(side, name):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p[side].radiation_pattern = name
    with pytest.raises(AssertionError, match="radiation pattern"):
        p.validate(4)


def _params(bs_pattern=0, ue_pattern=0):
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = 8, 1, 1, 1
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = 25, 1, 512, 1, 10e6
    sel = (C.c_int32 * 1)()
    p._keep = sel
    p.selected_subcarriers = C.addressof(sel)
    p.bs_pattern, p.ue_pattern = bs_pattern, ue_pattern
    return p


def _queries(lib):
    return {"dmx_fd_kernel_choice": lambda p: lib.dmx_fd_kernel_choice(C.byref(p), 25),
            "dmx_fd_direct_supported": lambda p: lib.dmx_fd_direct_supported(C.byref(p), 25),
            "dmx_rate_supported": lambda p: lib.dmx_rate_supported(C.byref(p), 25),
            "dmx_covariance_supported": lambda p: lib.dmx_covariance_supported(C.byref(p), 25, 0)}


@needs_lib
@pytest.mark.parametrize("query", ["dmx_fd_kernel_choice", "dmx_fd_direct_supported", "dmx_rate_supported", "dmx_covariance_supported"])
def test_host_queries_take_id_2_and_refuse_the_rest(query):
    from deepmimo_amd import _native as n
    lib = n.load()
    q = _queries(lib)[query]
    want = q(_params())
    assert want >= 1                                                          # the shape itself is taken
    for bs, ue in ((2, 0), (0, 2), (2, 1), (1, 2), (2, 2)):
        assert q(_params(bs, ue)) == want, (bs, ue)                           # the pattern does not move the answer
    for bad in (3, 7, -1):
        for bs, ue in ((bad, 0), (0, bad), (bad, 2)):
            assert q(_params(bs, ue)) == -1, (bs, ue)                         # DMX_ERR_ARG
            assert lib.dmx_last_error().decode() == "unknown radiation pattern id"


def test_isotropic_and_dipole():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    assert dm.pattern_gain("isotropic", np.array([0.3, np.nan])) == 1.0
    assert dm.pattern_gain("isotropic", 0.3, 1.0) == 1.0
    th = np.concatenate([np.linspace(0, np.pi, 181), [np.nan, 1e-12, np.pi / 2]])
    got = dm.pattern_gain("halfwave-dipole", th)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, onp.pattern_gain("halfwave-dipole", th))
    np.testing.assert_array_equal(dm.pattern_gain("halfwave-dipole", th, np.zeros_like(th)), got)     # phi is not used
    assert got[-3] == 0.0 and got[-2] == 0.0 and got[-1] == 1.643
    with pytest.raises(NotImplementedError):
        dm.pattern_gain("yagi", 0.0, 0.0)
    with pytest.raises(ValueError):
        dm.pattern_gain("tr38901", 0.0)


def test_closed_form_points():
    import deepmimo_amd as dm
    g = lambda th_deg, ph_deg: dm.pattern_gain("tr38901", np.float64(th_deg) * DEG, np.float64(ph_deg) * DEG)   # noqa: E731
    eps = 1e-12                                                     # dB: a few float64 roundings of values <= 30
    assert g(90, 0).dtype == np.float64
    assert abs(_db(g(90, 0)) - 8.0) <= eps and abs(g(90, 0) - G0) <= 4e-15 * G0
    for th, ph in ((90, 32.5), (90, -32.5), (90 + 32.5, 0), (90 - 32.5, 0)):        # half the beamwidth: exactly -3 dB
        assert abs(_db(g(th, ph)) - 5.0) <= eps, (th, ph)
    assert abs(_db(g(90 + 32.5, 32.5)) - 2.0) <= eps                               # the cuts add
    # the floor: behind the panel, and at the poles wherever the azimuth's share brings the sum to 30 dB - the vertical cut
    # alone stops at 12 (90 / 65)^2 = 23.0 dB, so a pole reached at azimuth 0 is at 8 - 23.0 dBi
    for th, ph in ((90, 180), (90, -180), (0, 180), (180, 180), (0, 60), (180, -60), (0, 50), (10, 170)):
        assert abs(g(th, ph) - FLOOR) <= 1e-15 * FLOOR, (th, ph)
    for th in (0, 180):
        assert abs(_db(g(th, 0)) - (8.0 - 12.0 * (90.0 / 65.0) ** 2)) <= eps
    assert abs(dm.pattern_gain("tr38901", np.pi / 2, np.pi) - FLOOR) <= 1e-15 * FLOOR
    # symmetric in both cuts about boresight
    x = np.linspace(0, 90, 91)
    np.testing.assert_array_equal(g(90, x), g(90, -x))
    np.testing.assert_allclose(g(90 + x, 10), g(90 - x, 10), rtol=1e-13)
    # arrays broadcast, shape kept
    assert dm.pattern_gain("tr38901", np.full((3, 4), 1.0), np.full((3, 4), 0.5)).shape == (3, 4)


def test_continuity_across_the_three_corners():
    """Each `min` switches where its two arguments are equal, so the gain is continuous there: on either side of the
    corner, one float64 step away, it differs by no more than the slope allows (|d gain / d angle| <= 24 x / b^2 ln10/10
    gain, under 8 per radian relative at the cap), and past the corner it is the constant floor."""
    import deepmimo_amd as dm
    cap = R.CAP_ANGLE_DEG * DEG
    d = 1e-9
    floor = dm.pattern_gain("tr38901", np.pi / 2, np.pi)           # the helper's own floor: past a cap it is this very number
    assert abs(floor - FLOOR) <= 1e-15 * FLOOR
    # the horizontal cap (vertical cut at 0), the vertical cap (horizontal cut at 0)
    for th, ph in ((lambda t: np.pi / 2, lambda t: t), (lambda t: np.pi / 2 + t, lambda t: 0.0),
                   (lambda t: np.pi / 2 - t, lambda t: 0.0), (lambda t: np.pi / 2, lambda t: -t)):
        below, at, above = (dm.pattern_gain("tr38901", th(t), ph(t)) for t in (cap - d, cap, cap + d))
        assert above == floor and abs(at - floor) <= 1e-12 * floor
        assert 0 <= below - floor <= 8 * d * 1.01 * floor
    # only the sum is capped: 12 (x / b)^2 = 15 in each cut
    x = 65.0 * np.sqrt(15.0 / 12.0) * DEG
    assert 12 * (x / R.BEAMWIDTH) ** 2 < 30
    below, at, above = (dm.pattern_gain("tr38901", np.pi / 2 + t, t) for t in (x - d, x, x + d))
    assert above == floor and abs(at - floor) <= 1e-12 * floor and 0 <= below - floor <= 2 * 6 * d * 1.01 * floor
    # and the floor holds everywhere past the caps
    t = np.linspace(cap, np.pi, 50)
    assert np.all(np.abs(dm.pattern_gain("tr38901", np.full_like(t, np.pi / 2), t) - FLOOR) <= 1e-15 * FLOOR)


def test_nan_gives_zero():
    import deepmimo_amd as dm
    th = np.array([np.nan, 1.0, np.nan, 1.0])
    ph = np.array([0.5, np.nan, np.nan, 0.5])
    got = dm.pattern_gain("tr38901", th, ph)
    assert np.array_equal(got[:3], [0.0, 0.0, 0.0]) and got[3] > 0
    assert dm.pattern_gain("halfwave-dipole", np.array([np.nan]))[0] == 0.0
    np.testing.assert_array_equal(R.tr38901_gain(th, ph), got)


def test_helper_against_the_reference_on_random_angles():
    """1e4 random angle pairs: two float64 evaluations of the same formula, operations in another order.  The exponent
    (8 - A) / 10 is at most 2.2 in magnitude and carries a few roundings of A <= 30 (each <= 30 x 2^-53 = 3.3e-15, /10),
    which 10^x turns into a relative ln(10) x 1e-15: 1e-13 relative covers it fifty times over."""
    import deepmimo_amd as dm
    rng = np.random.default_rng(38901)
    th, ph = rng.uniform(0, np.pi, 10_000), rng.uniform(-np.pi, np.pi, 10_000)
    got, want = dm.pattern_gain("tr38901", th, ph), R.tr38901_gain(th, ph)
    assert got.dtype == want.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert (want <= FLOOR * (1 + 1e-15)).mean() > 0.2 and (want > 1.0).mean() > 0.05          # both regimes are among them
    for name in ("isotropic", "halfwave-dipole"):
        np.testing.assert_allclose(dm.pattern_gain(name, th, ph), R.side_gain(name, th, ph), rtol=1e-13, atol=0)


def test_patched_oracle_restores_and_multiplies():
    """The wrapper: isotropic untouched (float32 powers stay float32), the dipole the oracle's own product, the sector
    element the float64 gain on the FoV-masked angles, NaN kept where the path is padding and 0 where the FoV masks."""
    from oracle import oracle_np as onp
    rays = onp.synth_rays(9, 6, seed=5)
    original = onp.prepare_paths
    fov = np.array([120, 90])
    plain = onp.prepare_paths(rays, onp.make_params(), fov, None)
    dip = onp.prepare_paths(rays, onp.make_params(bs_antenna=dict(radiation_pattern="halfwave-dipole")), fov, None)
    with pytest.raises(NotImplementedError):
        onp.prepare_paths(rays, onp.make_params(bs_antenna=dict(radiation_pattern="tr38901")))
    with R.patched_oracle() as o:
        assert o.prepare_paths is not original
        a = o.prepare_paths(rays, onp.make_params(), fov, None)
        assert a["_power_linear_ant_gain"].dtype == np.float32
        np.testing.assert_array_equal(a["_power_linear_ant_gain"], plain["_power_linear_ant_gain"])
        b = o.prepare_paths(rays, onp.make_params(bs_antenna=dict(radiation_pattern="halfwave-dipole")), fov, None)
        np.testing.assert_array_equal(b["_power_linear_ant_gain"], dip["_power_linear_ant_gain"])
        t = o.prepare_paths(rays, onp.make_params(bs_antenna=dict(radiation_pattern="tr38901"),
                                                  ue_antenna=dict(radiation_pattern="tr38901")), fov, None)
        pw = t["_power_linear_ant_gain"]
        assert pw.dtype == np.float64
        pad, masked = np.isnan(rays["power"]), ~t["_fov_mask"] & ~np.isnan(rays["power"])
        assert masked.any() and np.isnan(pw[pad]).all() and (pw[masked] == 0).all()
        live = ~pad & ~masked
        want = plain["power_linear"].astype(np.float64) * R.tr38901_gain(t["_aod_el_rot_fov"], t["_aod_az_rot_fov"]) * \
            R.tr38901_gain(t["_aoa_el_rot_fov"], t["_aoa_az_rot_fov"])
        np.testing.assert_allclose(pw[live], want[live], rtol=1e-15)
        for k in ("num_paths", "los", "_fov_mask"):
            np.testing.assert_array_equal(t[k], plain[k])
        H = o.compute_channels(rays, onp.make_params(bs_antenna=dict(radiation_pattern="tr38901")), fov, None)["channel"]
        assert H.dtype == np.complex64 and np.isfinite(H).all() and np.abs(H).max() > 0
    assert onp.prepare_paths is original
