"""UE receive combining on the host - no GPU: `deepmimo_amd.combiner`, the structure of the `with_rx_combiner` view,
`split_rx_beams`, every refusal of the view and of `compute_beam_pair_power`, and the identity the view rests on, checked
with the NumPy oracle for every case of tests/test_gpu_rx_combiner.py.  `dataset._engine` raises AssertionError throughout
(as in tests/test_time_series_cpu.py), so everything that passes here ran without the GPU; where a view is built, stage 1's
arrival angles are stood in for by the oracle's.  The references are those of tests/_combiner_ref.py."""
import numpy as np
import pytest

from tests import _combiner_cases as CS
from tests import _combiner_ref as R

ENGINE_ASKED = "the GPU engine was asked for"


@pytest.fixture(autouse=True)
def _no_engine(monkeypatch):
    from deepmimo_amd import dataset as dsm

    def no_engine():
        raise AssertionError(ENGINE_ASKED)
    monkeypatch.setattr(dsm, "_engine", no_engine)


def _dm_params(case, ue_rot):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(case["bs_shape"]), np.array(case["ue_shape"])
    p.bs_antenna.spacing, p.ue_antenna.spacing = case["bs_spacing"], case["ue_spacing"]
    p.bs_antenna.rotation, p.ue_antenna.rotation = np.array(case["bs_rot"]), np.array(ue_rot)
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = case["bs_pattern"], case["ue_pattern"]
    p.num_paths, p.freq_domain = case["num_paths"], case["freq_domain"]
    p.ofdm.subcarriers, p.ofdm.selected_subcarriers = case["subcarriers"], np.array(case["selected"])
    p.ofdm.bandwidth, p.ofdm.rx_filter = case["bandwidth"], case["rx_filter"]
    return p


def _dataset(rays, case=CS.BASE):
    import deepmimo_amd as dm
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    if case["ue_fov"] is not None:
        ds.apply_fov(ue_fov=np.array(case["ue_fov"]))
    return ds


@pytest.fixture
def oracle_angles(monkeypatch):
    """`Dataset._rx_arrival_angles` answers with the oracle's angles for the stored parameters, without the GPU"""
    import deepmimo_amd as dm
    from oracle import oracle_np as onp

    def angles(self):
        p = self.ch_params
        op = onp.make_params(ue_antenna=dict(shape=p.ue_antenna.shape, spacing=p.ue_antenna.spacing,
                                             rotation=np.asarray(p.ue_antenna.rotation)))
        if op["ue_antenna"]["rotation"].shape == (3, 2):
            np.random.seed(1001)
            op["ue_antenna"]["rotation"] = self._resolved_ue_rotation()
        rays = {k: np.asarray(self[k]) for k in CS_RAY_KEYS}
        prep = onp.prepare_paths(rays, op, self.get("bs_fov"), self.get("ue_fov"))
        return prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"]
    monkeypatch.setattr(dm.Dataset, "_rx_arrival_angles", angles)


CS_RAY_KEYS = ("power", "phase", "delay", "aoa_az", "aoa_el", "aod_az", "aod_el", "inter")


# ---------------------------------------------------------------------------------------------- 1. the response
@pytest.mark.parametrize("shape, spacing", [([2, 2], 0.5), ([3, 1], 0.5), ([2, 3], 0.7), ([1, 1], 0.5)])
def test_combiner_response_is_the_codebook_on_the_oracle_array_response(shape, spacing):
    import torch
    from deepmimo_amd.combiner import combiner_response
    from oracle import oracle_np as onp
    rng = np.random.default_rng(1)
    m = shape[0] * shape[1]
    theta, phi = rng.uniform(0, np.pi, (9, 8)), rng.uniform(-np.pi, np.pi, (9, 8))
    theta[3, 2:] = phi[3, 2:] = np.nan
    theta[5] = phi[5] = np.nan
    W = rng.normal(size=(3, m)) + 1j * rng.normal(size=(3, m))
    want = np.einsum("qr,url->uql", W, onp.array_response_batch(shape, spacing, theta, phi))
    hole = np.broadcast_to(np.isnan(theta)[:, None, :], want.shape)
    for got in (combiner_response(W, shape, spacing, theta, phi),
                combiner_response(W, shape, spacing, torch.from_numpy(theta), torch.from_numpy(phi)).numpy()):
        assert got.shape == (9, 3, 8) and got.dtype == np.complex128
        assert np.array_equal(np.isnan(got), hole)                         # NaN where theta is NaN, and only there
        err = np.abs(got - want)[~hole].max()
        print(f"{shape}: worst error {err:.2e}")
        assert err <= 1e-12
    # without a conjugate: the conjugated codebook gives another response
    assert np.abs(combiner_response(W.conj(), shape, spacing, theta, phi) - want)[~hole].max() > 1e-3


# ---------------------------------------------------------------------------------------------- 2. the ray matrices
def test_combine_rays_identities():
    import torch
    from deepmimo_amd.combiner import combine_rays
    rays = CS.rays()
    power, phase = rays["power"], rays["phase"]
    hole = np.isnan(power)
    shape = power.shape
    for to, back in ((lambda v: v, lambda v: v), (torch.from_numpy, lambda v: v.numpy())):
        def run(e):
            return tuple(back(v) for v in combine_rays(to(power), to(phase), to(np.full(shape, e, np.complex128))))
        p, x = run(1.0)                                                     # e = 1: the stored bits
        assert p.dtype == x.dtype == np.float32 and p.tobytes() == power.tobytes() and x.tobytes() == phase.tobytes()
        p, x = run(-1.0)                                                    # e = -1: half a turn, the power untouched
        assert p.tobytes() == power.tobytes() and np.array_equal(np.isnan(x), hole)
        turned = np.remainder(phase.astype(np.float64)[~hole] + 360.0, 360.0) - 180.0
        assert np.all(np.abs(x[~hole] - turned) <= 180.0 * 2.0 ** -23) and x[~hole].min() >= -180 and x[~hole].max() <= 180
        p, x = run(0.0)                                                     # |e| = 0: a finite power, no new NaN
        assert np.array_equal(np.isnan(p), hole) and np.array_equal(np.isnan(x), hole)
        assert np.all(np.isfinite(p[~hole])) and np.array_equal(x, phase, equal_nan=True)
        want = power.astype(np.float64)[~hole] + 10 * np.log10(2.0 ** -100)
        assert np.all(np.abs(p[~hole] - want) <= np.abs(want) * 2.0 ** -23) and np.all(p[~hole] < power[~hole] - 300)
        p, x = run(2j)                                                      # 6.02 dB up, a quarter turn
        assert np.allclose(p[~hole], power[~hole] + 20 * np.log10(2.0), rtol=0, atol=1e-4)
        assert np.all(np.abs(np.remainder(x[~hole].astype(np.float64) - phase[~hole] - 90.0 + 180.0, 360.0) - 180.0) <= 1e-4)
        p, x = run(np.nan)                                                  # NaN stays NaN
        assert np.isnan(p).all() and np.isnan(x).all()
    # one rounding: the float64 sum rounded once, not a float32 sum
    e = np.full(shape, 0.3 - 0.2j)
    p, _ = combine_rays(power, phase, e)
    once = (power.astype(np.float64) + 10 * np.log10(0.13)).astype(np.float32)
    assert np.array_equal(p[~hole], once[~hole])


def test_every_codebook_refusal():
    import deepmimo_amd as dm
    from deepmimo_amd.combiner import check_rx_codebook
    W = check_rx_codebook("who", "dft", [2, 2])
    assert W.dtype == np.complex128 and np.array_equal(W, dm.dft_codebook([2, 2]).astype(np.complex128))
    W = check_rx_codebook("who", [[1, 0, 0, 1j]], [2, 2])
    assert W.dtype == np.complex128 and W.shape == (1, 4)
    for bad in ("DFT", None, 3, np.zeros((2, 3)), np.zeros(4), np.zeros((1, 2, 4)), np.zeros((0, 4)),
                np.array([[1, np.nan, 0, 0]]), np.array([[1, np.inf, 0, 0]]), [["a", "b", "c", "d"]]):
        with pytest.raises(ValueError, match="^who: the UE codebook"):
            check_rx_codebook("who", bad, [2, 2])
    # the two methods refuse the same things under their own names, before the engine
    ds = _dataset(CS.rays())
    p = _dm_params(CS.BASE, np.zeros(3))
    F = dm.dft_codebook(CS.BASE["bs_shape"])
    for bad in ("DFT", np.zeros((2, 3)), np.zeros((0, 4)), np.array([[1, np.nan, 0, 0]])):
        with pytest.raises(ValueError, match="^with_rx_combiner: the UE codebook"):
            ds.with_rx_combiner(bad, p)
        with pytest.raises(ValueError, match="^compute_beam_pair_power: the UE codebook"):
            ds.compute_beam_pair_power(F, bad, p)
    for bad in ("dft", None, np.zeros((2, 7)), np.zeros(8), np.zeros((0, 8))):
        with pytest.raises(ValueError, match="^compute_beam_pair_power: the BS codebook"):
            ds.compute_beam_pair_power(bad, "dft", p)
    for change, word in ((dict(freq_domain=0), "freq_domain"), (dict(rx_filter=1), "rx_filter"),
                         (dict(selected=[0, 32768]), "32768")):
        with pytest.raises(ValueError, match=word):
            ds.compute_beam_pair_power(F, "dft", _dm_params({**CS.BASE, **change}, np.zeros(3)))
    with pytest.raises(AssertionError, match=ENGINE_ASKED):                # a fault-free call gets as far as the engine
        ds.compute_beam_pair_power(F, "dft", p)
    with pytest.raises(AssertionError, match=ENGINE_ASKED):
        ds.with_rx_combiner("dft", p)


# ---------------------------------------------------------------------------------------------- 3. structure of the view
def test_view_is_a_combiner_major_dataset_of_single_antenna_users(oracle_angles):
    import deepmimo_amd as dm
    name = "ue2x2_K64_Q3_B33_per_user_rot_folded"
    case, ue_rot, op, fov, rays, W, F = CS.setup(name)
    ds = _dataset(rays, case)
    scene = object()
    ds["scene"], ds["note"] = scene, "kept"
    ds["inter_pos"] = np.arange(CS.N_UE * CS.L * 3, dtype=np.float32).reshape(CS.N_UE, CS.L, 3)
    ds["beam_mean_amplitude"] = np.ones((CS.N_UE, 4), np.float32)          # results of the uncombined rays
    ds["beam_pair_mean_amplitude"] = np.ones((CS.N_UE, 3, 4), np.float32)
    ds._data["channel"] = np.ones((CS.N_UE, 4, 8, 1), np.complex64)
    ds._data["los"] = np.ones(CS.N_UE, np.int64)
    p = _dm_params(case, ue_rot)
    view = ds.with_rx_combiner(W, p)
    Q, n = 3, CS.N_UE
    assert type(view) is dm.Dataset and view.n_ue == Q * n and view.n_rx_beams == Q and view.n_ue_per_rx_beam == n
    assert view.rx_combiner.dtype == np.complex128 and np.array_equal(view.rx_combiner, W) and view.rx_combiner is not W
    for k, v in rays.items():
        if k in ("power", "phase", "tx_pos"):
            continue
        got = view[k]
        assert got.shape == (Q * n,) + v.shape[1:] and got.dtype == v.dtype, k
        for q in range(Q):                                                  # row q * n_ue + u is user u
            assert np.array_equal(got[q * n:(q + 1) * n], v, equal_nan=True), (k, q)
    assert np.array_equal(view.inter_pos.reshape(Q, n, CS.L, 3)[2], ds.inter_pos)
    assert np.array_equal(view.tx_pos, rays["tx_pos"]) and view.note == "kept" and view["scene"] is scene
    assert not [k for k in view.keys() if k.startswith("_")]
    assert not {"channel", "los", "beam_mean_amplitude", "beam_pair_mean_amplitude"} & set(view.keys())
    # the parameters: a single antenna, the rotation of every user tiled, everything else as given, and a copy
    vp = view.ch_params
    assert list(vp.ue_antenna.shape) == [1, 1] and list(ds.ch_params.ue_antenna.shape) == [2, 2]
    assert np.array_equal(vp.ue_antenna.rotation, np.tile(ue_rot, (Q, 1)))
    assert np.array_equal(vp.bs_antenna.shape, p.bs_antenna.shape) and vp.bs_antenna.shape is not ds.ch_params.bs_antenna.shape
    assert np.array_equal(vp.ofdm.selected_subcarriers, p.ofdm.selected_subcarriers)
    # the ray matrices: those of the module under test, NaN where the parent has none, float32
    prep = R.prepared(rays, op, *fov)
    e = R.responses(prep, op, W)                                            # [n, Q, L]
    pw, ph = view.split_rx_beams(view.power), view.split_rx_beams(view.phase)
    assert pw.shape == ph.shape == (Q, n, CS.L) and pw.dtype == ph.dtype == np.float32 and np.shares_memory(pw, view.power)
    hole = np.isnan(rays["power"])
    assert np.array_equal(np.isnan(pw), np.broadcast_to(hole, pw.shape)) and np.array_equal(np.isnan(ph), np.isnan(pw))
    with np.errstate(divide="ignore"):                                      # e is 0 where there is no path
        want = rays["power"].astype(np.float64)[None] + 20 * np.log10(np.abs(e)).transpose(1, 0, 2)
    assert np.all(np.abs(pw - want)[:, ~hole] <= np.abs(want[:, ~hole]) * 2.0 ** -23)
    turn = np.angle(e.transpose(1, 0, 2)[:, ~hole] * np.exp(1j * np.deg2rad(rays["phase"].astype(np.float64)[~hole])) *
                    np.exp(-1j * np.deg2rad(ph[:, ~hole].astype(np.float64))))
    assert np.all(np.abs(turn) <= 3 * np.pi * 2.0 ** -24) and np.nanmin(ph) >= -180 and np.nanmax(ph) <= 180
    # the parent is what it was
    assert ds.n_ue == n and ds.power.tobytes() == rays["power"].tobytes() and "rx_combiner" not in ds.keys()
    # split_rx_beams maps over tuples and dicts, never copies, and refuses another first axis or another dataset
    pair = view.split_rx_beams((np.zeros(Q * n), {"a": np.zeros((Q * n, 2))}))
    assert pair[0].shape == (Q, n) and pair[1]["a"].shape == (Q, n, 2)
    import torch
    t = torch.zeros(Q * n, 5)
    assert view.split_rx_beams(t).shape == (Q, n, 5) and view.split_rx_beams(t).data_ptr() == t.data_ptr()
    for bad in (np.zeros(n), np.zeros((Q * n + 1, 2)), np.float32(1.0)):
        with pytest.raises(ValueError, match="^split_rx_beams: the first axis"):
            view.split_rx_beams(bad)
    with pytest.raises(ValueError, match="^split_rx_beams: this dataset is not a view"):
        ds.split_rx_beams(np.zeros(Q * n))
    with pytest.raises(ValueError, match="^split_times: "):
        view.split_times(np.zeros(Q * n))
    sub = view.subset(np.arange(5))
    assert "n_rx_beams" not in sub.keys() and "rx_combiner" not in sub.keys()
    # a UE array on the view is refused by name; a single antenna gets as far as the engine
    array = view.ch_params.deepcopy()
    array.ue_antenna.shape = np.array([2, 2])
    with pytest.raises(ValueError, match="with_rx_combiner"):
        view.compute_channels(array)
    with pytest.raises(ValueError, match="with_rx_combiner"):
        view.compute_rate(array, snr_db=10.0)
    assert list(view.ch_params.ue_antenna.shape) == [1, 1]                 # and the refused parameters were not stored
    with pytest.raises(AssertionError, match=ENGINE_ASKED):
        view.compute_channels()
    # an identity codebook on a single antenna keeps every stored bit
    one = _dataset(rays).with_rx_combiner(np.ones((1, 1)), _dm_params({**case, "ue_shape": [1, 1]}, np.zeros(3)))
    assert one.power.tobytes() == rays["power"].tobytes() and one.phase.tobytes() == rays["phase"].tobytes()


class _FakeEngine:
    """stands where the engine stands, up to the upload: `_prep_inputs` shows the rotation a call would run with"""

    def upload_rays(self, data):
        return None


def _rotation_a_call_would_use(ds, monkeypatch):
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(dsm, "_engine", _FakeEngine)
    return ds._prep_inputs()[3]["ue_rotation_per_user"]


def test_rotation_draw_time_views_and_macro_dataset(oracle_angles, monkeypatch):
    import deepmimo_amd as dm
    name = "ue3x1_K64_Q3_B5_rot_range_matrix_core"
    case, ue_rot, op, fov, _, W, F = CS.setup(name)
    rays = CS.rays(with_doppler=True)
    p = _dm_params(case, ue_rot)
    Q, n, T = 3, CS.N_UE, 2
    ds = _dataset(rays, case)
    view = ds.with_rx_combiner(W, p)
    np.random.seed(1001)
    drawn = np.random.uniform(ue_rot[:, 0], ue_rot[:, 1], (n, 3))           # the parent's draw, with the seed of every call
    assert np.array_equal(ds._data["_ue_rotation_resolved"], drawn)
    np.random.seed(5)
    assert np.array_equal(_rotation_a_call_would_use(view, monkeypatch), np.tile(drawn, (Q, 1)))
    # drawn anew (the parameters set again on the view): one orientation per UE, tiled over the UE beams
    view.set_channel_params(view.ch_params)
    view._clear_cache_rotated_angles()
    np.random.seed(1001)
    assert np.array_equal(_rotation_a_call_would_use(view, monkeypatch), np.tile(drawn, (Q, 1)))
    # either order with at_times: Q * T * n users; the Doppler matrices are per-user arrays and get tiled
    fc, times = 28e9, [0.0, 1e-3]
    a = ds.at_times(times, carrier_freq=fc).with_rx_combiner(W, p)
    b = ds.with_rx_combiner(W, p).at_times(times, carrier_freq=fc)
    for v in (a, b):
        assert v.n_ue == Q * T * n and v.doppler_vel.shape == (Q * T * n, CS.L) and v.n_rx_beams == Q and v.n_times == T
        assert list(v.ch_params.ue_antenna.shape) == [1, 1]
    assert a.n_ue_per_rx_beam == T * n and b.n_ue_per_time == Q * n
    assert np.array_equal(a.split_rx_beams(a.doppler_vel)[1], np.tile(rays["doppler_vel"], (T, 1)), equal_nan=True)
    pa, pb = a.phase.reshape(Q, T, n, CS.L), b.phase.reshape(T, Q, n, CS.L).transpose(1, 0, 2, 3)
    assert np.array_equal(np.isnan(pa), np.isnan(pb))
    d = np.abs(np.remainder(pa.astype(np.float64) - pb + 180.0, 360.0) - 180.0)
    assert np.nanmax(d) <= 2 * 180.0 * 2.0 ** -23                          # the two float32 roundings in the other order
    assert np.array_equal(a.power.reshape(Q, T, n, CS.L), b.power.reshape(T, Q, n, CS.L).transpose(1, 0, 2, 3), equal_nan=True)
    np.random.seed(1001)
    assert np.array_equal(_rotation_a_call_would_use(a, monkeypatch), np.tile(drawn, (Q * T, 1)))
    # MacroDataset: a view per child
    assert "with_rx_combiner" in vars(dm.MacroDataset) and "split_rx_beams" in vars(dm.MacroDataset)
    kids = [_dataset(CS.rays(seed=1), case), _dataset(CS.rays(seed=2), case)]
    mv = dm.MacroDataset(kids).with_rx_combiner(W, p)
    assert type(mv) is dm.MacroDataset and [d.n_ue for d in mv.datasets] == [Q * n, Q * n]
    assert mv.split_rx_beams(np.zeros(Q * n)).shape == (Q, n)
    with pytest.raises(ValueError, match="^with_rx_combiner: 3 parameter sets"):
        dm.MacroDataset(kids).with_rx_combiner(W, [p, p, p])


# ---------------------------------------------------------------------------------------------- 4. the identity
_worst = {}


@pytest.mark.parametrize("name", list(CS.CASES))
def test_single_antenna_users_on_combined_rays_give_the_combined_channel(name):
    """What the view rests on, without the GPU: the oracle's channels of 1 x 1 users on the combined ray matrices against
    W @ H of the oracle on the stored ones, within the tolerance of tests/_combiner_ref.py (worst seen: 0.083, at K = 1)."""
    from deepmimo_amd.combiner import combine_all
    case, ue_rot, op, fov, rays, W, F = CS.setup(name)
    ref, tol, _ = R.reference(rays, op, W, *fov)
    prep = R.prepared(rays, op, *fov)
    power, phase = combine_all(rays["power"], rays["phase"], W, case["ue_shape"], case["ue_spacing"],
                               prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"])
    H = R.single_antenna_channels(rays, op, prep, power, phase, *fov)
    assert (tol > 0).sum() >= len(W) * 3 and np.all(tol[CS.NO_PATH_USER] == 0) and np.all(ref[CS.NO_PATH_USER] == 0)
    _worst[name] = R.worst_ratio(H, ref, tol, what=name)
    assert _worst[name] <= 1.0


@pytest.mark.parametrize("name", list(CS.CASES))
def test_the_tolerance_sees_a_wrong_combiner(name):
    case, ue_rot, op, fov, rays, W, F = CS.setup(name)
    ref, tol, _ = R.reference(rays, op, W, *fov)
    live = tol > 0

    def moved(other):
        d = np.abs(other - ref).reshape(ref.shape[0], ref.shape[1], -1).max(axis=2)
        return float((d[live] / tol[live]).max())
    # one kept path less: the strongest one of the user with all eight
    strongest = int(np.argmax(R.path_moduli(R.prepared(rays, op, *fov), op)[0]))
    fewer = {k: v.copy() for k, v in rays.items()}
    for k in CS_RAY_KEYS:
        fewer[k][0, strongest] = np.nan
    drop = moved(R.reference(fewer, op, W, *fov)[0])
    print(f"{name}: dropping path {strongest} of user 0 moves the reference by {drop:.3g} bounds")
    assert drop > 2.0
    if np.abs(W.imag).max() > 1e-3:
        conj = moved(R.reference(rays, op, W.conj(), *fov)[0])
        print(f"{name}: the conjugated codebook moves the reference by {conj:.3g} bounds")
        assert conj > 2.0


def test_the_cases_cover_what_they_have_to():
    seen = {k: set() for k in ("ue", "K", "Q", "B", "rot", "route", "rays", "output", "pattern")}
    complex_codebooks = 0
    for name, (changes, rot, _, B, run) in CS.CASES.items():
        case = {**CS.BASE, **changes}
        W = CS.ue_codebook(name)
        seen["ue"].add(tuple(case["ue_shape"])), seen["K"].add(len(case["selected"])), seen["B"].add(B)
        seen["Q"].add("M_rx" if len(W) == W.shape[1] and len(W) > 1 else len(W))
        seen["rot"].add(np.shape(rot)), seen["pattern"].add(case["ue_pattern"])
        seen["route"].add(run["route"]), seen["rays"].add(run["rays"]), seen["output"].add(run["output"])
        complex_codebooks += bool(np.abs(W.imag).max() > 1e-3)
        assert CS.bs_codebook(name).shape == (B, 8)
    assert seen["ue"] == {(2, 2), (3, 1), (1, 1)} and seen["K"] == {1, 5, 64} and seen["B"] == {1, 5, 33}
    assert seen["Q"] == {1, 3, "M_rx"} and seen["rot"] == {(3,), (CS.N_UE, 3), (3, 2)}
    assert seen["pattern"] == {"isotropic", "halfwave-dipole", "tr38901"}
    assert seen["route"] >= {"direct", 12, 2, 1} and seen["rays"] == {"host", "hbm"} and seen["output"] == {"numpy", "torch"}
    assert any({**CS.BASE, **c[0]}["ue_fov"] is not None for c in CS.CASES.values()) and complex_codebooks >= 3
    r = CS.rays()
    assert tuple((~np.isnan(r["power"])).sum(axis=1)) == CS.PATH_COUNTS
    assert CS.PATH_COUNTS[CS.NO_PATH_USER] == 0 and CS.PATH_COUNTS[CS.ONE_PATH_USER] == 1
