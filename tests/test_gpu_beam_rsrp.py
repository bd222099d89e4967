"""The power-averaged beam sweep (DMX_FLAG_BEAM_MEAN_POWER, `metric="power"`) on the GPU, against the NumPy oracle in float64.

Reference and bound are those of tests/_beam_rsrp_ref.py: P = (|F @ H_ref|^2).mean(rx).mean(k) and the project's element
tolerance carried through ||Y + d|^2 - |Y|^2| <= 2 |Y| |d| + |d|^2.  The cases are those of tests/_beam_cases.py (every
projection route, 1 / 2 / 4 / 8 row tiles, two and three row blocks, K = 1 ... 130, 3 ... 32 kept paths) with both codebooks;
then the wrong indices of that module, the identity with the covariance kernel, the exactness properties the header states,
one case each of the adaptive terms, 32 of 40 loaded paths, the near field and the two-sided sweep, and what the Python
layer makes of the means."""
import os

import numpy as np
import pytest

from tests import _beam_cases as B
from tests import _beam_rsrp_ref as R
from tests._cases import TOL_ABS, TOL_REL

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_parity import _dm_params  # noqa: E402

WORST = {}                                   # what -> worst error / bound seen
DISAGREE = {}                                # (case, codebook) -> users whose power argmax is not the amplitude argmax


@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the module: the worst error / bound over what ran (README.md quotes it; every figure was asserted where it was
    measured)"""
    yield
    if WORST:
        what = max(WORST, key=WORST.get)
        print(f"beam rsrp: worst power error / bound over {len(WORST)} comparisons {WORST[what]:.3f} ({what}); "
              f"{sum(DISAGREE.values())} users with another best beam than the amplitude metric's")


def _engine():
    from deepmimo_amd.dataset import _engine
    return _engine()


def _copy(rays):
    return {k: v.copy() for k, v in rays.items()}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _case(name, codebook):
    """(case, rays, oracle result, F, Y = F @ H_ref complex128, has) of a case of tests/_beam_cases.py"""
    c = B.BY_NAME[name]
    rays, ref = B.reference(c)
    F = B.codebooks(c["bs"], c["nb"])[codebook]
    return c, rays, ref, F, F @ ref["channel"].astype(np.complex128), ref["los"] != -1


def _prepare(eng, c, rays, **kw):
    return eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(B.fd_case(c), np.zeros(3)).validate(c["n"]), want_side="light", **kw)


def _hold(P, best, Y, has, what, delta=None):
    """the means within their tolerance, zeros and -1 without a path, the beam the reference's or a tie within tolerance"""
    assert P.dtype == np.float32 and P.shape == Y.shape[:1] + Y.shape[2:3] and np.isfinite(P).all(), what
    ratio = R.power_ratio(P, Y, has, delta)
    WORST[what] = float(ratio.max())
    print(f"{what}: worst power error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (what, ratio.max())
    assert np.all(P[~has] == 0)
    if best is not None:
        assert best.dtype == np.int32 and R.best_beam_faults(best, Y, has, delta) == [], what
        np.testing.assert_array_equal(best[has], np.argmax(P[has], axis=1))      # the first maximum of what it returned
        assert np.all(best[~has] == -1)


# ---- 1. every case, both codebooks ---------------------------------------------------------------------------------------------------
def _run_case(name, codebook):
    """one case against the oracle, once per session: DISAGREE remembers that it held"""
    if (name, codebook) in DISAGREE:
        return
    c, rays, ref, F, Y, has = _case(name, codebook)
    eng = _engine()
    prep = _prepare(eng, c, rays)
    P_d, best_d = eng.beam_power(prep, F, metric="power")
    P, best = P_d.cpu().numpy(), best_d.cpu().numpy()
    _hold(P, best, Y, has, f"{name} {codebook}")
    assert prep.params_struct.flags == 0                                        # the bit was set on a copy, for the call
    # where the two metrics name different beams the kernel follows the power
    differ = R.metrics_disagree(Y, has)
    want = R.beam_powers(Y)
    np.testing.assert_array_equal(best[differ], np.argmax(want[differ], axis=1))
    amp_best = eng.beam_power(prep, F)[1].cpu().numpy()
    np.testing.assert_array_equal(amp_best[differ], np.argmax(np.abs(Y).mean(axis=(1, 3))[differ], axis=1))
    assert np.all(best[differ] != amp_best[differ])
    # a reference that gets one index wrong fails the same comparison
    Href = ref["channel"].astype(np.complex128)
    for kind in B.MUTATIONS:
        if not B.mutation_is_void(kind, F, c):
            assert R.power_ratio(P, B.mutate(kind, F, Href), has).max() > 1.0, (name, codebook, kind)
    DISAGREE[(name, codebook)] = len(differ)


@pytest.mark.parametrize("codebook", B.CODEBOOKS)
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_mean_power_on_every_route(name, codebook):
    _run_case(name, codebook)
    assert (name, codebook) in DISAGREE


def test_the_kernel_follows_the_power_argmax_where_the_metrics_disagree():
    """over the cases above (run here where they have not run yet) at least 10 users - the oracle says 47 - have another
    power argmax than amplitude argmax, and `_run_case` held the kernel to the power argmax for each of them"""
    for name in B.CASE_NAMES:
        for codebook in B.CODEBOOKS:
            _run_case(name, codebook)
    assert sum(DISAGREE.values()) == 47 >= 10


# ---- 2. mutations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mtx9", "rows600"])
def test_a_wrong_index_in_the_reference_fails_the_comparison(name):
    """the kernel's means against a reference that gets one index wrong: each mutation is out of tolerance, by how much
    (`_run_case` asserts the same for every case and codebook)"""
    c, rays, ref, F, Y, has = _case(name, "random")
    eng = _engine()
    P = eng.beam_power(_prepare(eng, c, rays), F, want_best=False, metric="power")[0].cpu().numpy()
    assert R.comparison_passes(P, Y, has)
    Href = ref["channel"].astype(np.complex128)
    kinds = [k for k in B.MUTATIONS if not B.mutation_is_void(k, F, c)]
    assert len(kinds) == 4
    for kind in kinds:
        ratio = R.power_ratio(P, B.mutate(kind, F, Href), has)
        print(f"{name} {kind}: worst error / bound against the mutated reference {ratio.max():.0f}")
        assert ratio.max() > 1.0, (name, kind)
    # and the amplitude metric squared is not the power metric
    amp = eng.beam_power(_prepare(eng, c, rays), F, want_best=False)[0].cpu().numpy().astype(np.float64)
    assert not R.comparison_passes((amp ** 2).astype(np.float32), Y, has)


# ---- 3. the covariance kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows40", "mtx9", "mfma4_largest"])
def test_identity_with_the_covariance_kernel(name):
    """P[u, b] = Re(F_b R_tx[u] F_b^H), both from the path records; the bound: the power tolerance plus ||F_b||_1^2 times the
    covariance tolerance (TOL_REL max|R_ref[u]| + TOL_ABS, tests/test_gpu_covariance.py)"""
    from tests._covariance_ref import cov_from_channel
    c, rays, ref, F, Y, has = _case(name, "random")
    eng = _engine()
    prep = _prepare(eng, c, rays)
    assert eng.covariance_supported(prep, "tx")
    P = eng.beam_power(prep, F, want_best=False, metric="power")[0].cpu().numpy().astype(np.float64)
    Rtx = eng.covariance(prep, side="tx").cpu().numpy().astype(np.complex128)
    quad = np.einsum("bi,uij,bj->ub", F, Rtx, F.conj())
    assert np.abs(quad.imag).max() <= 1e-6 * np.abs(quad.real).max()
    Rref = cov_from_channel(ref["channel"], "tx")
    np.testing.assert_allclose(np.einsum("bi,uij,bj->ub", F, Rref, F.conj()).real, R.beam_powers(Y), rtol=1e-10, atol=1e-30)
    cov_tol = TOL_REL * np.abs(Rref).reshape(len(Rref), -1).max(axis=1) + TOL_ABS
    bound = R.power_tolerance(Y) + (np.abs(F).sum(axis=1) ** 2)[None, :] * cov_tol[:, None]
    ratio = np.abs(P - quad.real)[has] / bound[has]
    print(f"{name}: worst |P - F R F^H| / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0 and np.all(P[~has] == 0) and np.all(quad[~has] == 0)


# ---- 4. exactness --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,part", [("rows128", (11, 30)), ("rows600", (5, 18)), ("mtx12", (11, 24))])
def test_launches_repeat_bit_for_bit(name, part):
    """`part`: the users [begin, end) of the sub-range - 11 ... 29 of the 40 users of rows128, some of them without a path"""
    import torch
    import deepmimo_amd as dm
    c, rays, ref, F, Y, has = _case(name, "steering")
    b0, cnt = part[0], part[1] - part[0]
    assert part[1] <= c["n"] and has[b0:part[1]].any() and (name != "rows128" or (~has[b0:part[1]]).any())
    eng = _engine()
    prep = _prepare(eng, c, rays)
    amp0 = _bits(eng.beam_power(prep, F)[0])
    P_d, best_d = eng.beam_power(prep, F, metric="power")
    P, best = _bits(P_d), best_d.cpu().numpy()
    # a repeat launch, a launch without `best`, a user sub-range
    P2_d, best2_d = eng.beam_power(prep, F, metric="power")
    assert np.array_equal(_bits(P2_d), P) and np.array_equal(best2_d.cpu().numpy(), best)
    assert np.array_equal(_bits(eng.beam_power(prep, F, want_best=False, metric="power")[0]), P)
    sub_d, sub_best = eng.beam_power(prep, F, user_begin=b0, user_count=cnt, metric="power")
    assert np.array_equal(_bits(sub_d), P[b0:b0 + cnt]) and np.array_equal(sub_best.cpu().numpy(), best[b0:b0 + cnt])
    # the amplitude call of the same process is what it was before the power call, and the two are different numbers
    assert np.array_equal(_bits(eng.beam_power(prep, F)[0]), amp0)
    assert not np.array_equal(amp0[has], P[has])
    # rays on the host and in HBM
    p = _dm_params(B.fd_case(c), np.zeros(3))
    host = dm.Dataset(_copy(rays))
    host.compute_beam_power(F, p, metric="power")
    hbm = dm.Dataset({k: torch.from_numpy(v.copy()).cuda() for k, v in rays.items()})
    hbm.compute_beam_power(F, p, metric="power")
    assert np.array_equal(host["beam_mean_power"].view(np.uint32), P) and np.array_equal(hbm["beam_mean_power"].view(np.uint32), P)


# ---- 5. one case each -----------------------------------------------------------------------------------------------------------------------
def test_adaptive_terms():
    """DMX_FLAG_ADAPTIVE_TERMS | DMX_FLAG_BEAM_MEAN_POWER on the weak-tail batch of tests/_path_count_cases.py, rays in stage
    1's order: within the tolerance, and different bits from the three-term result exactly where the rule fires"""
    from tests import _path_count_cases as PC
    case, rays, fires, n_keep, ref = PC.weak_tail_reference("beam", True)
    F = PC.codebooks(case["bs_shape"])["steering"]
    Y = F @ ref["channel"].astype(np.complex128)
    has = ref["los"] != -1
    eng = _engine()
    out = {}
    for adaptive in (False, True):
        prep = eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(case, np.zeros(3)).validate(len(fires)), want_side="light",
                           adaptive_terms=adaptive)
        assert prep.params_struct.flags == (1 if adaptive else 0)
        P_d, best_d = eng.beam_power(prep, F, metric="power")
        out[adaptive] = P_d.cpu().numpy()
        _hold(out[adaptive], best_d.cpu().numpy(), Y, has, f"weak tail {'flag' if adaptive else 'default'}")
    differ = np.array([not np.array_equal(out[True][u].view(np.uint32), out[False][u].view(np.uint32)) for u in range(len(fires))])
    np.testing.assert_array_equal(differ, fires)


def test_32_of_40_loaded_paths():
    """num_paths = 32 on 40 loaded paths: the ladder of tests/_path_count_cases.py, 0 ... 32 and 33, 40 valid paths"""
    from tests import _path_count_cases as PC
    case, rays, kept, ref = PC.ladder_reference("beam", "L40")
    assert rays["power"].shape[1] == 40 and case["num_paths"] == 32 and kept.max() == 32 and kept.min() == 0
    F = PC.codebooks(case["bs_shape"])["random"]
    Y = F @ ref["channel"].astype(np.complex128)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(_copy(rays)), _dm_params(case, np.zeros(3)).validate(len(kept)), want_side="light")
    P_d, best_d = eng.beam_power(prep, F, metric="power")
    _hold(P_d.cpu().numpy(), best_d.cpu().numpy(), Y, kept > 0, "32 of 40 loaded paths")


@pytest.mark.parametrize("cid", ["c_upa8x4_2x2_k5_p32", "c_ula16_1x1_k70_p7"])
def test_near_field_view(cid):
    """`metric="power"` on a near-field view against tests/_near_field_ref.py.  That module's tolerance of a channel element
    is TOL_REL of the user's peak plus a term for the record's float32 delay; behind a codebook row the term grows by at most
    ||F_b||_1, so delta[u, b] = TOL_REL max|Y[u]| + TOL_ABS + ||F_b||_1 term[u], carried into the power as everywhere else"""
    from tests import _near_field_cases as NC
    from tests.test_gpu_near_field_consumers import _beam_codebook
    case = NC.BY_ID[cid]
    H, _far, tol_h = NC.references(case)
    F = _beam_codebook(case).astype(np.complex128)
    Y = F @ H
    has = np.abs(H).reshape(len(H), -1).max(axis=1) > 0
    term = tol_h - TOL_REL * np.abs(H).reshape(len(H), -1).max(axis=1)
    assert np.all(term >= 0)
    delta = R.element_delta(Y)[:, None] + np.abs(F).sum(axis=1)[None, :] * term[:, None]
    view = NC.dataset(case).near_field(NC.CARRIER)
    pwr, best = view.compute_beam_power(F.astype(np.complex64), NC.dm_params(case), return_best=True, metric="power")
    P = view["beam_mean_power"]
    _hold(P, None, Y, has, f"near field {cid}", delta)
    assert np.array_equal(np.isnan(pwr[:, 0]), ~has) and "beam_mean_amplitude" not in view._data
    far = NC.dataset(case)
    far.compute_beam_power(F.astype(np.complex64), NC.dm_params(case), metric="power")
    assert R.power_ratio(far["beam_mean_power"], Y, has, delta).max() > 100      # the plane-wave kernel misses this reference


def test_beam_pair_power():
    """`compute_beam_pair_power(metric="power")`, UE 2 x 2 with Q = 3 combiners, against the einsum; the element tolerance
    behind the combiner is that of tests/_combiner_ref.py (`amplitude_tolerance`: it bounds every |dY|, not only the mean)"""
    from tests import _combiner_cases as CS
    from tests import _combiner_ref as CR
    name = "ue2x2_K64_Q3_B33_per_user_rot_folded"
    case, ue_rot, op, fov, rays, W, F = CS.setup(name)
    assert case["ue_shape"] == [2, 2] and len(W) == 3
    import deepmimo_amd as dm
    ref, _tol, second = CR.reference(rays, op, W, *fov)
    Y = np.einsum("uqtk,bt->uqbk", ref, F)                                       # ref = einsum('qr,urtk->uqtk', W, H_oracle)
    n, Q, Bn = Y.shape[:3]
    want = (np.abs(Y) ** 2).mean(axis=-1)
    delta = CR.amplitude_tolerance(ref, second, F) + TOL_ABS
    tol = 2 * delta * np.abs(Y).mean(axis=-1) + delta ** 2
    ds = dm.Dataset(_copy(rays))
    p = _dm_params(case, ue_rot)
    pwr, best_rx, best_tx = ds.compute_beam_pair_power(F, W, p, return_best=True, metric="power")
    P = ds["beam_pair_mean_power"]
    none = np.asarray(ds.los) == -1
    assert P.shape == (n, Q, Bn) and P.dtype == np.float32 and pwr.dtype == np.float64 and "beam_pair_mean_amplitude" not in ds._data
    assert none[CS.NO_PATH_USER] and np.all(P[none] == 0)
    ratio = (np.abs(P - want)[~none] / tol[~none]).max()
    print(f"{name}: worst pair power error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(np.isnan(pwr), np.broadcast_to(none[:, None, None], pwr.shape))
    with np.errstate(divide="ignore"):
        assert np.array_equal(pwr[~none], np.around(10 * np.log10(P[~none]) + 30, 1))
    first = np.argmax(pwr.reshape(n, Q * Bn)[~none], axis=1)
    assert np.array_equal(best_rx[~none], first // Bn) and np.array_equal(best_tx[~none], first % Bn)
    assert np.isnan(best_rx[none]).all() and np.isnan(best_tx[none]).all()
    # the default metric of the same dataset is what it is without this feature's argument
    a = ds.compute_beam_pair_power(F, W, p)
    assert np.array_equal(a[~none], np.around(20 * np.log10(ds["beam_pair_mean_amplitude"][~none]) + 30, 1))


# ---- 6. what Python makes of the means ------------------------------------------------------------------------------------------------------
def test_dbm_nan_and_best_are_exact_functions_of_the_means():
    import deepmimo_amd as dm
    c, rays, ref, F, Y, has = _case("rows128", "random")
    p = _dm_params(B.fd_case(c), np.zeros(3))
    ds = dm.Dataset(_copy(rays))
    pwr, best = ds.compute_beam_power(F, p, return_best=True, metric="power")
    P = ds["beam_mean_power"]
    assert "beam_mean_amplitude" not in ds._data and P.dtype == np.float32 and pwr.dtype == np.float64 and pwr.shape == P.shape
    none = np.asarray(ds.los) == -1
    np.testing.assert_array_equal(none, ~has)
    assert none.sum() >= 4
    want = np.full(P.shape, np.nan)
    want[~none] = np.around(10 * np.log10(P[~none]) + 30, 1)
    assert np.array_equal(pwr, want, equal_nan=True)
    want_best = np.argmax(want, axis=1).astype(float)
    want_best[none] = np.nan
    assert np.array_equal(best, want_best, equal_nan=True)
    assert np.array_equal(ds.compute_beam_power(F, p, metric="power"), pwr, equal_nan=True)
    eng = _engine()
    np.testing.assert_array_equal(eng.beam_power(_prepare(eng, c, rays), F, want_best=False, metric="power")[0].cpu().numpy(), P)
    # in dB the power average is never below the amplitude average (Jensen), and the default call still returns the latter
    amp_dbm = ds.compute_beam_power(F, p)
    assert np.array_equal(amp_dbm[~none], np.around(20 * np.log10(ds["beam_mean_amplitude"][~none]) + 30, 1))
    assert np.all(pwr[~none] >= amp_dbm[~none] - 0.1 - 1e-9) and np.any(pwr[~none] > amp_dbm[~none] + 0.5)


def _cells():
    """three cells over the same 24 users: three draws of rays, one BS panel; user 3 has no path to any cell, user 5 to
    cell 1 only"""
    from oracle import oracle_np as onp
    import deepmimo_amd as dm
    out = []
    for i, seed in enumerate((801, 802, 803)):
        rays = onp.synth_rays(24, 6, seed=seed)
        for k in onp.RAY_KEYS:
            rays[k][3] = np.nan
            if i != 1:
                rays[k][5] = np.nan
        out.append(dm.Dataset(dict(rays)))
    return out


def test_serving_beam_of_three_cells_and_the_cell_rate_it_feeds():
    import deepmimo_amd as dm
    from deepmimo_amd.engine import select_serving_beam
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape = np.array([4, 2])
    p.ue_antenna.shape = np.array([2, 1])
    p.ofdm.subcarriers = 64
    p.ofdm.selected_subcarriers = np.arange(0, 64, 4)
    F = dm.dft_codebook([4, 2])
    cells = _cells()
    macro = dm.MacroDataset(cells)
    got = macro.compute_serving_beam(F, p)
    # the NumPy selection over three plain calls
    dbm = np.full((24, 3), np.nan)
    beam = np.full((24, 3), -1, np.int32)
    for i, ds in enumerate(_cells()):
        pwr, best = ds.compute_beam_power(F, p, return_best=True, metric="power")
        ok = ~np.isnan(best)
        beam[ok, i] = best[ok].astype(np.int32)
        dbm[ok, i] = pwr[ok, beam[ok, i]]
        assert np.array_equal(cells[i]["beam_mean_power"], ds["beam_mean_power"])
    serving, b, v = select_serving_beam(dbm, beam)
    assert np.array_equal(got.dbm_by_cell, dbm, equal_nan=True) and np.array_equal(got["beam_by_cell"], beam)
    assert np.array_equal(got.serving, serving) and np.array_equal(got.beam, b) and np.array_equal(got.dbm, v, equal_nan=True)
    assert got.serving.dtype == got.beam.dtype == got.beam_by_cell.dtype == np.int32 and got.dbm_by_cell.dtype == got.dbm.dtype == np.float64
    assert got.serving[3] == -1 and got.beam[3] == -1 and np.isnan(got.dbm[3]) and got.serving[5] == 1
    assert set(got.serving.tolist()) == {-1, 0, 1, 2}
    rows = np.flatnonzero(got.serving >= 0)
    assert np.array_equal(got.dbm[rows], np.nanmax(dbm[rows], axis=1))
    # a list per child gives the same, and the amplitude metric is another selection rule
    again = macro.compute_serving_beam([F, F, F], [p, p, p], metric="power")
    assert np.array_equal(again.serving, got.serving) and np.array_equal(again.dbm_by_cell, got.dbm_by_cell, equal_nan=True)
    amp = macro.compute_serving_beam(F, p, metric="amplitude")
    seen = ~np.isnan(got.dbm_by_cell)
    assert np.array_equal(np.isnan(amp.dbm_by_cell), ~seen) and np.all(amp.dbm_by_cell[seen] <= got.dbm_by_cell[seen] + 0.1 + 1e-9)
    assert np.any(amp.dbm_by_cell[seen] < got.dbm_by_cell[seen] - 0.5)
    # `serving` goes straight into compute_cell_rate
    rate, served, _snr = macro.compute_cell_rate(p, snr_db=100.0, serving=got.serving, details=True)
    assert np.array_equal(served, got.serving)
    assert np.all(rate[got.serving < 0] == 0) and np.all(rate[rows] >= 0) and np.any(rate[rows] > 0) and np.isfinite(rate).all()
