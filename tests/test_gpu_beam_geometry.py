"""Every route of the codebook projection and every row geometry of the beam kernels, against the NumPy oracle in float64.

The cases are those of tests/_beam_cases.py: the matrix-core projection with 1, 2 and 4 beam tiles and with a partly
filled last K-step (M_tx = 1, odd, bs_mh no power of two), the scalar projection for each of its three reasons and its
refusal; k2c_beam_power with every tile count of a row block, last blocks whose wave grouping differs from the first
block's, three blocks, and its LDS cap from both sides; the beam-space contraction with two and three row blocks and with
each of its tile-loop bodies.  tests/test_beam_cases_cpu.py ties the route of each case to the launchers' text and holds
the condition that makes the comparison able to fail.  The checks and tolerances are those of tests/test_gpu_parity.py
(`check_beam_channels`, `check_beam_power`): TOL_REL of the user's peak for F @ H, 1e-5 of the user's strongest beam for
the mean amplitudes.
"""
import os

import numpy as np
import pytest

from tests import _beam_cases as B
from tests._cases import TOL_ABS, TOL_REL, assert_channel_close, channel_err, oracle_params
from tests._path_count_cases import BOUND_BEAM_POWER

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_parity import _dm_params, check_beam_channels, check_beam_power  # noqa: E402

WORST = {}                                   # (projection route, consumer) -> worst error / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module: the worst error / bound per projection route and consumer over what ran (BASELINE.md quotes
    them; every figure was asserted where it was measured)"""
    yield
    for key in sorted(WORST):
        print(f"beam geometry: {key[0]} {key[1]}: worst error / bound {WORST[key]:.3f}")


def _record(route, consumer, ratio):
    WORST[(route, consumer)] = max(WORST.get((route, consumer), 0.0), float(ratio))


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _copy(rays):
    return {k: v.copy() for k, v in rays.items()}


def _amp_ratio(amp, want, has):
    return (np.abs(amp - want)[has] / (BOUND_BEAM_POWER * want[has].max(axis=1, keepdims=True))).max()


@pytest.mark.parametrize("codebook", B.CODEBOOKS)
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_beam_consumers_on_every_route(name, codebook):
    """compute_beam_channels and compute_beam_power with the suite's own checks"""
    import deepmimo_amd as dm
    c = B.BY_NAME[name]
    rays, ref = B.reference(c)
    route = B.routes(c)["projection"]
    p = _dm_params(B.fd_case(c), np.zeros(3))
    F = B.codebooks(c["bs"], c["nb"])[codebook]
    Href = ref["channel"].astype(np.complex128)
    has = ref["los"] != -1
    Y = check_beam_channels(dm.Dataset(_copy(rays)), p, F, Href)
    assert Y.shape == (c["n"], B.m_rx(c), c["nb"], c["K"]) and np.all(Y[~has] == 0)
    d, peak = channel_err(Y, (F @ Href).astype(np.complex64))
    ratio = (d[has] / (TOL_REL * peak[has] + TOL_ABS)).max()
    print(f"{name} {codebook} ({route}): beam-space channel, worst error / bound {ratio:.3f}")
    _record(route, "channels", ratio)
    ds = check_beam_power(_copy(rays), p, F, Href, ref["los"], part=(5, 13))
    amp = ds["beam_mean_amplitude"]
    want = B.beam_amplitudes(F @ Href)
    ratio = _amp_ratio(amp, want, has)
    print(f"{name} {codebook} ({route}): beam power, worst amplitude error / bound {ratio:.3f}")
    _record(route, "power", ratio)
    assert ratio <= 1.0 and np.all(amp[~has] == 0)
    np.testing.assert_array_equal(ds.num_paths, ref["num_paths"])


@pytest.mark.parametrize("name", ["rows600", "scalar_image"])
def test_contraction_user_sub_range_on_several_row_blocks(name):
    """a user sub-range of the beam-space contraction is bit-identical to the same rows of the full call, with two and
    three row blocks per user (work item = user x row block)"""
    import torch
    c = B.BY_NAME[name]
    assert B.routes(c)["contraction"][1] in (2, 3)
    rays, ref = B.reference(c)
    F = B.codebooks(c["bs"], c["nb"])["random"]
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(B.fd_case(c), np.zeros(3)).validate(c["n"]))
    full = eng.channels(prep, tx_codebook=F).clone()
    b0, cnt = 7, 11
    sub = eng.channels(prep, tx_codebook=F, user_begin=b0, user_count=cnt)
    torch.cuda.synchronize()
    assert sub.shape == (cnt,) + tuple(full.shape[1:])
    assert torch.equal(torch.view_as_real(sub).view(torch.int32), torch.view_as_real(full[b0:b0 + cnt]).view(torch.int32))
    assert (ref["los"][b0:b0 + cnt] != -1).any() and np.abs(sub.cpu().numpy()).max() > 0


def test_projection_routes_agree_on_shared_rows():
    """One random codebook on a [4, 2] panel: its first 64 rows (mfma2), its 128 rows (mfma4) and the same 128 rows with
    one appended (scalar) give beam-space channels that agree with the oracle and, on the rows they share, with one another
    at the parity tolerance (of the shared rows' peak).  Not bit for bit: the per-user exponent depends on the rows."""
    from oracle import oracle_np as onp
    c = dict(name="cross", bs=[4, 2], ue=[2, 1], nb=129, L=12, K=33, n=24, seed=6401)
    assert [B.projection_route(8, nb, c["L"]) for nb in (64, 128, 129)] == ["mfma2", "mfma4", "scalar"]
    rays = B.rays_of(c)
    Href = onp.compute_channels(rays, oracle_params(B.fd_case(c), np.zeros(3)))["channel"].astype(np.complex128)
    rng = np.random.default_rng(64)
    F = (rng.normal(size=(129, 8)) + 1j * rng.normal(size=(129, 8))) * 11.0
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(B.fd_case(c), np.zeros(3)).validate(c["n"]))
    Y = {nb: eng.channels(prep, tx_codebook=F[:nb]).cpu().numpy() for nb in (64, 128, 129)}
    for nb, route in ((64, "mfma2"), (128, "mfma4"), (129, "scalar")):
        assert Y[nb].shape == (c["n"], 2, nb, c["K"])
        assert_channel_close(Y[nb], (F[:nb] @ Href).astype(np.complex64), what=f"{route} against the oracle")
    assert_channel_close(Y[128][:, :, :64], Y[64], what="mfma4 against mfma2, rows 0..63")
    assert_channel_close(Y[129][:, :, :64], Y[64], what="scalar against mfma2, rows 0..63")
    assert_channel_close(Y[129][:, :, :128], Y[128], what="scalar against mfma4, rows 0..127")
    assert np.abs(Y[64]).max() > 0


def _cap_setup():
    from oracle import oracle_np as onp
    fit, over = B.cap_beam_counts()
    c = B.cap_case(over)
    rays = B.rays_of(c)
    ref = onp.compute_channels(rays, oracle_params(B.fd_case(c), np.zeros(3)))
    F = B.codebooks(c["bs"], over)["random"]
    return c, rays, ref, F, fit, over


def test_beam_power_at_its_lds_cap_and_one_beam_over():
    """256 receive elements: 95 beams are 24 320 rows, 95 row blocks and 163 344 B of LDS, the largest launch taken; its
    amplitudes hold check_beam_power's bounds.  96 beams are refused by launch_beam_power's host check, in front of every
    launch (tests/test_beam_cases_cpu.py reads that order off the source) - an argument error: the next call on the same
    engine is answered as if nothing had happened."""
    from deepmimo_amd._native import NativeError
    c, rays, ref, F, fit, over = _cap_setup()
    assert B.power_geometry(256, fit, c["K"])["fits"] and not B.power_geometry(256, over, c["K"])["fits"]
    has = ref["los"] != -1
    assert 0 < has.sum()
    Href = ref["channel"].astype(np.complex128)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(B.fd_case(c), np.zeros(3)).validate(c["n"]))

    def hold(nb, what):
        amp_d, best_d = eng.beam_power(prep, F[:nb])
        amp, best = amp_d.cpu().numpy(), best_d.cpu().numpy()
        want = B.beam_amplitudes(F[:nb] @ Href)
        assert amp.shape == (c["n"], nb) and amp.dtype == np.float32
        peak = want[has].max(axis=1, keepdims=True)
        ratio = _amp_ratio(amp, want, has)
        print(f"{what}: worst amplitude error / bound {ratio:.3f}")
        assert np.all(np.abs(amp[has] - want[has]) <= 1e-5 * peak)
        strong = want[has] >= peak * 10 ** (-30 / 20)
        np.testing.assert_allclose(amp[has][strong], want[has][strong], rtol=1e-5, atol=0)
        assert np.all(amp[~has] == 0) and np.all(best[~has] == -1)
        np.testing.assert_array_equal(best[has], np.argmax(amp[has], axis=1))
        return ratio

    assert B.projection_route(8, fit, c["L"]) == "mfma4"
    _record("mfma4", "power at the LDS cap", hold(fit, f"{fit} beams x 256 receive elements"))
    with pytest.raises(NativeError, match=rf"status -2.*256 x {over} \(rx, beam\) rows"):
        eng.beam_power(prep, F)
    hold(5, "5 beams after the refusal")


def test_scalar_projection_refuses_a_panel_beyond_its_table():
    """512 BS elements x 25 path slots are 100 KiB of a_tx table: neither form of the projection takes it, and both
    consumers say so (DMX_ERR_SHAPE) instead of launching"""
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    c = B.REFUSED_PROJECTION
    assert B.projection_route(B.m_tx(c), c["nb"], c["L"]) == "error" and c["n"] == 2
    rays = B.rays_of(c)
    assert rays["power"].shape == (2, c["L"])
    p = _dm_params(B.fd_case(c), np.zeros(3))
    F = B.codebooks(c["bs"], c["nb"])["random"]
    ds = dm.Dataset(_copy(rays))
    with pytest.raises(NativeError, match=r"status -2.*BS panel of 512 elements x 25 paths"):
        ds.compute_beam_channels(F, p)
    with pytest.raises(NativeError, match=r"status -2.*BS panel of 512 elements x 25 paths"):
        ds.compute_beam_power(F, p)
    # one path slot fewer than the table holds at 256 elements is taken (the scalar_64k case runs exactly 64 KiB)
    assert B.projection_route(256, c["nb"], 32) == "scalar"
