"""Transmit precoding and multi-user rates on the host - no GPU: `deepmimo_amd.combiner`'s transmit side, `mu_partners`,
the structure of the `with_tx_precoder` view, every refusal of the view and of `compute_mu_rate`, and the references of
tests/_mu_ref.py checked on the NumPy oracle alone - closed forms, and that every case of tests/_mu_cases.py can tell a
wrong link table, exchanged beams and a missing power split from the truth.  `dataset._engine` raises AssertionError
throughout (as in tests/test_combiner_cpu.py), so everything that passes here ran without the GPU; where a view is built,
stage 1's departure angles are stood in for by the oracle's."""
import numpy as np
import pytest

from tests import _mu_cases as CS
from tests import _mu_ref as MR
from tests._cases import RAY_KEYS

ENGINE_ASKED = "the GPU engine was asked for"


@pytest.fixture(autouse=True)
def _no_engine(monkeypatch):
    from deepmimo_amd import dataset as dsm

    def no_engine():
        raise AssertionError(ENGINE_ASKED)
    monkeypatch.setattr(dsm, "_engine", no_engine)


def _dm_params(case, ue_rot=(10, -20, 30)):
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
    if case["bs_fov"] is not None:
        ds.apply_fov(bs_fov=np.array(case["bs_fov"]))
    return ds


@pytest.fixture
def oracle_angles(monkeypatch):
    """`Dataset._tx_departure_angles` / `_rx_arrival_angles` answer with the oracle's angles for the stored parameters"""
    import deepmimo_amd as dm
    from oracle import oracle_np as onp

    def angles(side):
        def get(self):
            p = self.ch_params
            op = onp.make_params(bs_antenna=dict(shape=p.bs_antenna.shape, spacing=p.bs_antenna.spacing,
                                                 rotation=np.asarray(p.bs_antenna.rotation)),
                                 ue_antenna=dict(shape=p.ue_antenna.shape, spacing=p.ue_antenna.spacing,
                                                 rotation=np.asarray(p.ue_antenna.rotation)))
            prep = onp.prepare_paths({k: np.asarray(self[k]) for k in RAY_KEYS}, op, self.get("bs_fov"), self.get("ue_fov"))
            return prep[f"_{side}_el_rot_fov"], prep[f"_{side}_az_rot_fov"]
        return get
    monkeypatch.setattr(dm.Dataset, "_tx_departure_angles", angles("aod"))
    monkeypatch.setattr(dm.Dataset, "_rx_arrival_angles", angles("aoa"))


# ---------------------------------------------------------------------------------------------- 1. the response
@pytest.mark.parametrize("shape, spacing", [([8, 1], 0.5), ([4, 2], 0.5), ([3, 5], 0.7), ([1, 1], 0.5)])
def test_precoder_response_per_user(shape, spacing):
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd.combiner import combiner_response, precoder_response
    rng = np.random.default_rng(2)
    m, n, L, B = shape[0] * shape[1], 6, 4, 5
    theta, phi = rng.uniform(0, np.pi, (n, L)), rng.uniform(-np.pi, np.pi, (n, L))
    theta[3, 2:] = phi[3, 2:] = np.nan
    F = rng.normal(size=(B, m)) + 1j * rng.normal(size=(B, m))
    idx = rng.integers(0, B, (3, n))
    idx[1, 4] = idx[2, 0] = -1
    # sums built from steering vectors, element by element: a(theta, phi) = sqrt(M) steering_vec(phi=theta, theta=phi - 90 deg)
    want = np.full((3, n, L), np.nan, complex)
    for j in range(3):
        for u in range(n):
            for l in range(L):
                if np.isnan(theta[u, l]):
                    continue
                a = np.sqrt(m) * dm.steering_vec(np.array(shape), phi=np.rad2deg(theta[u, l]), theta=np.rad2deg(phi[u, l]) - 90.0,
                                                 spacing=spacing).reshape(-1)
                want[j, u, l] = sum(F[idx[j, u], t] * a[t] for t in range(m)) if idx[j, u] >= 0 else 0.0
    hole = np.broadcast_to(np.isnan(theta)[None], want.shape)
    shared = combiner_response(F, shape, spacing, theta, phi)                           # [n, B, L]
    for got in (precoder_response(F, idx, shape, spacing, theta, phi),
                precoder_response(F, idx, shape, spacing, torch.from_numpy(theta), torch.from_numpy(phi)).numpy()):
        assert got.shape == (3, n, L) and got.dtype == np.complex128
        assert np.array_equal(np.isnan(got), hole)                                      # NaN angles stay NaN, and only they
        err = np.abs(got - want)[~hole].max()
        print(f"{shape}: worst error {err:.2e}")
        assert err <= 1e-12 * max(1.0, np.sqrt(m))
        assert np.all(got[1, 4][~hole[1, 4]] == 0) and np.all(got[2, 0][~hole[2, 0]] == 0)          # no transmission
        # the shared-codebook form gives the same numbers
        for j in range(3):
            for u in range(n):
                if idx[j, u] >= 0:                                                      # sin / cos of another array shape: an ulp
                    assert np.allclose(got[j, u], shared[u, idx[j, u]], rtol=0, atol=1e-13 * m, equal_nan=True), (j, u)
    # a 1-D index is J = 1; a shared row is combiner_response's
    one = precoder_response(F, idx[0], shape, spacing, theta, phi)
    assert one.shape == (1, n, L) and np.array_equal(one[0], precoder_response(F, idx, shape, spacing, theta, phi)[0], equal_nan=True)
    row = precoder_response(F, np.full((1, n), 2), shape, spacing, theta, phi)
    assert np.allclose(row[0], shared[:, 2], rtol=0, atol=1e-13 * m, equal_nan=True)


def test_precode_rays_rows_without_transmission_scale_and_stored_bits():
    import torch
    from deepmimo_amd.combiner import combine_all, precode_rays
    n, L = 7, 8
    rays = CS.rays(n, L)
    power, phase = rays["power"], rays["phase"]
    rng = np.random.default_rng(4)
    theta, phi = rng.uniform(0, np.pi, (n, L)), rng.uniform(-np.pi, np.pi, (n, L))
    theta[np.isnan(power)] = phi[np.isnan(power)] = np.nan
    theta[0, 1] = phi[0, 1] = np.nan                                                    # a path the field of view masks
    F = CS.codebook(("random", 4), [4, 2])
    idx = rng.integers(0, 4, (2, n))
    idx[1, 3] = -1
    scale = rng.uniform(0.3, 1.0, (2, n))
    for to, back in ((lambda v: v, lambda v: v), (torch.from_numpy, lambda v: v.numpy())):
        p, x = (back(v) for v in precode_rays(to(power), to(phase), F, idx, [4, 2], 0.5, to(theta), to(phi)))
        assert p.shape == x.shape == (2 * n, L) and p.dtype == x.dtype == np.float32
        p, x = p.reshape(2, n, L), x.reshape(2, n, L)
        assert np.isnan(p[1, 3]).all() and x[1, 3].tobytes() == phase[3].tobytes()       # idx = -1: NaN power, stored phase
        assert p[0, 0, 1] == power[0, 1] and x[0, 0, 1] == phase[0, 1]                   # no angle: the stored values
        assert np.array_equal(np.isnan(p[0]), np.isnan(power))
        # a shared row is combine_all's row
        pa, xa = (back(v) for v in combine_all(to(power), to(phase), F, [4, 2], 0.5, to(theta), to(phi)))
        for u in range(n):
            if idx[0, u] >= 0:
                assert p[0, u].tobytes() == pa.reshape(4, n, L)[idx[0, u], u].tobytes()
                assert x[0, u].tobytes() == xa.reshape(4, n, L)[idx[0, u], u].tobytes()
        # the scale goes through the one rounding with e: 20 log10(s) dB in float64 before it, the phase untouched
        ps, xs = (back(v).reshape(2, n, L) for v in precode_rays(to(power), to(phase), F, idx, [4, 2], 0.5, to(theta), to(phi), scale))
        live = ~np.isnan(p) & ~np.isnan(np.broadcast_to(theta, p.shape))
        want = p.astype(np.float64) + 20 * np.log10(scale)[:, :, None]
        assert np.all(np.abs(ps - want)[live] <= 2 * np.abs(want[live]) * 2.0 ** -23)
        assert np.array_equal(xs[live], x[live]) and np.isnan(ps[1, 3]).all()
        # e = 1 (a single antenna, weight 1) keeps every stored bit, with a scale of 1 too
        for s in (None, np.ones((1, n))):
            p1, x1 = (back(v) for v in precode_rays(to(power), to(phase), np.ones((1, 1)), np.zeros((1, n), int), [1, 1], 0.5,
                                                    to(theta), to(phi), s))
            assert p1.tobytes() == power.tobytes() and x1.tobytes() == phase.tobytes()


def test_codebook_and_beams_refusals():
    import deepmimo_amd as dm
    from deepmimo_amd.combiner import check_tx_beams, check_tx_codebook
    F = check_tx_codebook("who", "dft", [4, 2])
    assert F.dtype == np.complex128 and np.array_equal(F, dm.dft_codebook([4, 2]).astype(np.complex128))
    assert check_tx_codebook("who", np.ones((3, 8)), [4, 2]).shape == (3, 8)
    for bad in ("DFT", None, 3, np.zeros((2, 3)), np.zeros(8), np.zeros((0, 8)), np.array([[1, np.nan, 0, 0, 0, 0, 0, 0]])):
        with pytest.raises(ValueError, match="^who: the BS codebook must be 'dft' or a finite array \\[B, 8\\]"):
            check_tx_codebook("who", bad, [4, 2])
    assert check_tx_beams("who", [0, 2, -1], 3, 3).tolist() == [[0, 2, -1]]
    assert check_tx_beams("who", np.zeros((2, 3), np.int32), 3, 1).shape == (2, 3)
    for bad in (None, "all", [0.0, 1.0, 2.0], [0, 1], np.zeros((2, 2), int), np.zeros((1, 2, 3), int), [0, 1, 3], [0, -2, 1], True):
        with pytest.raises(ValueError, match="^who: beams must be an integer array"):
            check_tx_beams("who", bad, 3, 3)


# ---------------------------------------------------------------------------------------------- 2. the groups
def test_mu_partners_on_hand_made_groups():
    import deepmimo_amd as dm
    groups = [[4, 0, 6, -1], [1, -1, -1, -1], [5, 2, 7, 8], [-1, -1, -1, -1]]           # ragged, a group of one, an empty row
    partners, size, scheduled = dm.mu_partners(groups, 10)
    assert partners.dtype == np.int32 and size.dtype == np.int32 and scheduled.dtype == bool
    assert partners.tolist() == [[4, 6, -1], [-1, -1, -1], [5, 7, 8], [-1, -1, -1], [0, 6, -1], [2, 7, 8], [4, 0, -1],
                                 [5, 2, 8], [5, 2, 7], [-1, -1, -1]]                     # the order of the group's row
    assert size.tolist() == [3, 1, 4, 0, 3, 4, 3, 4, 4, 0] and scheduled.tolist() == [s > 0 for s in size.tolist()]
    # padding anywhere in the row, not only at its end
    partners, size, _ = dm.mu_partners(np.array([[-1, 2, -1, 0]]), 3)
    assert partners.tolist() == [[2, -1, -1], [-1, -1, -1], [0, -1, -1]] and size.tolist() == [2, 0, 2]
    partners, size, scheduled = dm.mu_partners(np.array([[1], [0]]), 3)                  # G = 1: no partner column
    assert partners.shape == (3, 0) and size.tolist() == [1, 1, 0]
    # the cases' tables against the reference's, built one user at a time
    for name in CS.MU_CASES:
        n, G = CS.MU_CASES[name][1], CS.MU_CASES[name][4]
        groups = CS.groups_of(n, G)
        partners, size, scheduled = dm.mu_partners(groups, n)
        want, want_size = MR.partners_of(groups, n)
        assert np.array_equal(partners, want) and np.array_equal(size, want_size)
        assert (~scheduled).sum() >= 1 and (G == 1 or ((size > 0) & (size < G)).any())     # someone in no group; a ragged row
    for bad in (None, "x", [0, 1], np.zeros((2, 2)), np.zeros((1, 9), int), np.zeros((1, 0), int), [[0, 3]], [[0, -2]], [[0, 1], [1, 2]],
                [[1, 1]]):
        with pytest.raises(ValueError, match="^mu_partners: "):
            dm.mu_partners(bad, 3)


# ---------------------------------------------------------------------------------------------- 3. every refusal
def test_every_refusal_of_compute_mu_rate_comes_before_the_gpu():
    n, L = 7, 8
    case = {**CS.BASE, "bs_shape": [4, 2], "ue_shape": [2, 2]}
    ds = _dataset(CS.rays(n, L))
    p = _dm_params(case)
    F = CS.codebook(("random", 3), [4, 2])
    beams, groups = np.array([0, 1, 2, 0, 1, 2, 0]), np.array([[0, 1, 2], [3, 4, -1]])
    ok = dict(snr_db=10.0)

    def refused(match, codebook=F, beams=beams, groups=groups, params=p, on=ds, **kw):
        with pytest.raises(ValueError, match=match):
            on.compute_mu_rate(codebook, beams, groups, params, **{**ok, **kw})
    refused("snr_db", snr_db=None)
    refused("snr_db", snr_db=float("nan"))
    refused("snr_db", snr_db=float("inf"))
    refused("snr_db", snr_db="10")
    for bad in ("DFT", None, np.zeros((3, 7)), np.zeros((0, 8)), np.full((2, 8), np.inf)):
        refused("^compute_mu_rate: the BS codebook", codebook=bad)
    for bad in (None, beams.astype(float), beams[:-1], beams[None], "dft"):
        refused("^compute_mu_rate: beams must be an integer array", beams=bad)
    refused("^compute_mu_rate: user 1 is scheduled on beam 3, outside 0 .. 2", beams=np.array([0, 3, 2, 0, 1, 2, 0]))
    refused("^compute_mu_rate: user 4 is scheduled on beam -1", beams=np.array([0, 1, 2, 0, -1, 2, 0]))
    for bad in (None, np.array([0, 1]), groups.astype(float), np.zeros((1, 9), int), np.zeros((2, 0), int), np.array([[0, 7]]),
                np.array([[0, -2]])):
        refused("^compute_mu_rate: groups must be an integer array", groups=bad)
    refused("^compute_mu_rate: user 1 appears more than once", groups=np.array([[0, 1], [1, 2]]))
    refused("freq_domain|time", params=_dm_params({**case, "freq_domain": 0}))
    refused("rx_filter", params=_dm_params({**case, "rx_filter": 1}))
    refused("M_rx = 9", params=_dm_params({**case, "ue_shape": [3, 3]}))
    refused("^compute_mu_rate: not covered on a near-field view", on=ds.near_field(28e9))
    with pytest.raises(ValueError, match="^with_tx_precoder: not covered on a near-field view"):
        ds.near_field(28e9).with_tx_precoder(F, beams, p)
    # a user in no group may carry any beam; a fault-free call gets as far as the engine
    with pytest.raises(AssertionError, match=ENGINE_ASKED):
        ds.compute_mu_rate(F, np.array([0, 1, 2, 0, 1, 99, -5]), groups, p, snr_db=10.0)
    with pytest.raises(AssertionError, match=ENGINE_ASKED):
        ds.with_tx_precoder(F, beams, p)
    for bad in ("DFT", np.zeros((3, 7))):
        with pytest.raises(ValueError, match="^with_tx_precoder: the BS codebook"):
            ds.with_tx_precoder(bad, beams, p)
    for bad in (beams.astype(float), beams[:-1], np.full(n, 3), np.full(n, -2), np.zeros((1, 2, n), int)):
        with pytest.raises(ValueError, match="^with_tx_precoder: beams must be an integer array"):
            ds.with_tx_precoder(F, bad, p)


# ---------------------------------------------------------------------------------------------- 4. structure of the view
def test_view_is_a_dataset_of_users_behind_a_single_bs_antenna(oracle_angles):
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd.combiner import precode_rays
    name = "bs4x2_ue2x1_K5_per_user_bs_rot_fov_hbm"
    case, op, fov, rays, F, beams, _ = CS.view_setup(name)
    n, L, B = rays["power"].shape[0], rays["power"].shape[1], len(F)
    ds = _dataset(rays, case)
    ds["note"] = "kept"
    ds._data["los"] = np.ones(n, np.int64)
    p = _dm_params(case)
    prep = MR.R.prepared(rays, op, *fov)
    th, ph = prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"]
    # beams = None: every beam, beam-major
    view = ds.with_tx_precoder(F, None, p)
    assert type(view) is dm.Dataset and view.n_ue == B * n and view.n_tx_beams == B and view.n_ue_per_tx_beam == n
    assert view.tx_precoder.dtype == np.complex128 and np.array_equal(view.tx_precoder, F) and view.tx_precoder is not F
    assert list(view.ch_params.bs_antenna.shape) == [1, 1] and list(ds.ch_params.bs_antenna.shape) == [4, 2]
    assert list(view.ch_params.ue_antenna.shape) == [2, 1] and np.array_equal(view.ch_params.bs_antenna.rotation, p.bs_antenna.rotation)
    assert np.array_equal(view.bs_fov, ds.bs_fov) and view.bs_fov is not ds.bs_fov and view.note == "kept" and "los" not in view.keys()
    for k in ("delay", "aod_az", "aod_el", "aoa_az", "inter", "rx_pos"):
        assert np.array_equal(view[k].reshape((B, n) + rays[k].shape[1:])[B - 1], rays[k], equal_nan=True), k
    want = precode_rays(rays["power"], rays["phase"], F, np.broadcast_to(np.arange(B)[:, None], (B, n)), [4, 2], 0.5, th, ph)
    assert view.power.tobytes() == want[0].tobytes() and view.phase.tobytes() == want[1].tobytes()
    e = MR.tx_responses(prep, op, F, np.broadcast_to(np.arange(B)[:, None], (B, n)))     # the oracle's response
    live = ~np.isnan(th)
    got = view.split_tx_beams(view.power).astype(np.float64) - rays["power"]
    assert np.shares_memory(view.split_tx_beams(view.power), view.power)
    assert np.all(np.abs(got[:, live] - 20 * np.log10(np.abs(e[:, live]))) <= 1e-4)
    # beams [n_ue] with a -1: n_ue users; the -1 row has no path
    one = ds.with_tx_precoder(F, beams, p)
    assert one.n_ue == n and one.n_tx_beams == 1 and one.n_ue_per_tx_beam == n and beams[1] == -1
    assert np.isnan(one.power[1]).all() and one.phase[1].tobytes() == rays["phase"][1].tobytes()
    for k in ("delay", "aoa_az", "aoa_el", "aod_az", "aod_el", "inter"):                # what num_paths and los are read from
        assert np.isnan(one[k][1]).all() and np.array_equal(np.delete(one[k], 1, axis=0), np.delete(rays[k], 1, axis=0), equal_nan=True), k
    assert not np.isnan(ds.aoa_az[1]).all()                                            # the parent keeps its own
    for u in range(n):
        if beams[u] >= 0:
            assert one.power[u].tobytes() == view.split_tx_beams(view.power)[beams[u], u].tobytes()
    # beams [J, n_ue]; per-user weights are B = n_ue with beams = arange(n_ue)
    table = np.stack([beams, np.roll(beams, 1)])
    two = ds.with_tx_precoder(F, table, p)
    assert two.n_ue == 2 * n and two.split_tx_beams(two.power).shape == (2, n, L) and two.split_tx_beams(two.power)[0].tobytes() == one.power.tobytes()
    own = CS.codebook(("random", n), [4, 2])
    per_user = ds.with_tx_precoder(own, np.arange(n), p)
    assert per_user.n_ue == n and per_user.tx_precoder.shape == (n, 8)
    # torch rays are precoded where they live
    dt = dm.Dataset({k: torch.from_numpy(v.copy()) for k, v in rays.items()})
    dt.apply_fov(bs_fov=np.array(case["bs_fov"]))
    monkey_angles = dm.Dataset._tx_departure_angles
    dm.Dataset._tx_departure_angles = lambda self: tuple(torch.from_numpy(a) for a in monkey_angles(self))
    try:
        vt = dt.with_tx_precoder(F, beams, p)
    finally:
        dm.Dataset._tx_departure_angles = monkey_angles
    assert isinstance(vt.power, torch.Tensor) and np.allclose(vt.power.numpy(), one.power, rtol=0, atol=1e-4, equal_nan=True)
    # split_tx_beams refuses another first axis or another dataset; subset drops the view's keys
    with pytest.raises(ValueError, match="^split_tx_beams: the first axis"):
        view.split_tx_beams(np.zeros(n))
    with pytest.raises(ValueError, match="^split_tx_beams: this dataset is not a view"):
        ds.split_tx_beams(np.zeros(n))
    assert not {"tx_precoder", "n_tx_beams", "n_ue_per_tx_beam"} & set(per_user.subset(np.arange(3)).keys())
    # a BS array on the view is refused by name and not stored; a single antenna gets as far as the engine
    array = view.ch_params.deepcopy()
    array.bs_antenna.shape = np.array([4, 2])
    with pytest.raises(ValueError, match="with_tx_precoder"):
        view.compute_channels(array)
    assert list(view.ch_params.bs_antenna.shape) == [1, 1]
    with pytest.raises(AssertionError, match=ENGINE_ASKED):
        view.compute_channels()
    with pytest.raises(ValueError, match="^near_field: not covered on a view of with_tx_precoder"):
        view.near_field(28e9)
    # the parent is what it was
    assert ds.n_ue == n and ds.power.tobytes() == rays["power"].tobytes() and "tx_precoder" not in ds.keys()


def test_view_composes_with_time_and_receive_views_and_fans_out(oracle_angles):
    import deepmimo_amd as dm
    case = {**CS.BASE, "bs_shape": [4, 2], "ue_shape": [2, 2], "selected": [0, 5]}
    n, L, T, Q = 7, 8, 2, 3
    rays = CS.rays(n, L, with_doppler=True)
    p = _dm_params(case)
    F = CS.codebook(("random", n), [4, 2])                                              # B = n_ue: never taken for a per-user array
    W = CS.codebook(("random", Q), [2, 2])
    beams = np.arange(n)
    ds = _dataset(rays, case)
    a = ds.at_times([0.0, 1e-3], carrier_freq=28e9).with_tx_precoder(F, np.tile(beams, T), p)
    b = ds.with_tx_precoder(F, beams, p).at_times([0.0, 1e-3], carrier_freq=28e9)
    assert a.n_ue == b.n_ue == T * n and a.tx_precoder.shape == b.tx_precoder.shape == (n, 8)
    assert np.array_equal(a.power, b.power, equal_nan=True)
    d = np.abs(np.remainder(a.phase.astype(np.float64) - b.phase + 180.0, 360.0) - 180.0)
    assert np.nanmax(d) <= 2 * 180.0 * 2.0 ** -23                                        # the two float32 roundings in the other order
    rx_tx = ds.with_rx_combiner(W, p).with_tx_precoder(F, np.tile(beams, Q))
    tx_rx = ds.with_tx_precoder(F, beams, p).with_rx_combiner(W)
    for v in (rx_tx, tx_rx):
        assert v.n_ue == Q * n and list(v.ch_params.bs_antenna.shape) == [1, 1] and list(v.ch_params.ue_antenna.shape) == [1, 1]
        assert v.n_rx_beams == Q and v.tx_precoder.shape == (n, 8)
    assert np.allclose(rx_tx.power, tx_rx.power, rtol=0, atol=1e-3, equal_nan=True)
    # MacroDataset: a view per child, one argument for all or one per child
    assert "with_tx_precoder" in vars(dm.MacroDataset) and "split_tx_beams" in vars(dm.MacroDataset)
    kids = [_dataset(CS.rays(n, L, seed=1), case), _dataset(CS.rays(n, L, seed=2), case)]
    mv = dm.MacroDataset(kids).with_tx_precoder(F, beams, p)
    assert type(mv) is dm.MacroDataset and [v.n_ue for v in mv.datasets] == [n, n] and mv.split_tx_beams(np.zeros(n)).shape == (1, n)
    mv = dm.MacroDataset(kids).with_tx_precoder([F, F[:3]], [beams, beams % 3], [p, p])
    assert [v.tx_precoder.shape[0] for v in mv.datasets] == [n, 3]
    with pytest.raises(ValueError, match="^with_tx_precoder: "):
        dm.MacroDataset(kids).with_tx_precoder(F, beams, [p, p, p])


# ---------------------------------------------------------------------------------------------- 5. the reference alone
def _los_ula(beam_of_user, n_sc=64):
    """single-path line-of-sight rays of a y-axis ULA of 8 whose departure direction makes DFT row b the matched beam:
    sin(phi) = 2 b / 8 at theta = 90 degrees"""
    from oracle import oracle_np as onp
    n = len(beam_of_user)
    r = onp.synth_rays(n, 1, seed=3, all_valid=True)
    r["aod_el"][:] = 90.0
    r["aod_az"][:, 0] = np.rad2deg(np.arcsin(2 * np.asarray(beam_of_user) / 8.0))
    r["power"][:] = 0.0
    op = onp.make_params(bs_antenna=dict(shape=[8, 1]), ue_antenna=dict(shape=[1, 1]), num_paths=1,
                         ofdm=dict(subcarriers=n_sc, selected_subcarriers=np.arange(0, n_sc, 7)))
    return r, op


def test_reference_closed_forms():
    # G = 1 on a 1 x 1 UE: log2(1 + snr |y|^2)
    name = "G1_ue1x1_K1_P3_snr10"
    case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
    ref = MR.mu_reference(rays, op, F, beams, groups, snr_db)
    y = MR.precoded(ref["H"], F, ref["idx"])[0][:, 0, :]
    want = np.where((ref["size"] > 0)[:, None], np.log2(1 + 10 ** (snr_db / 10) * np.abs(y) ** 2), 0.0)
    assert np.abs(ref["rate_k"] - want).max() <= 1e-12 and ref["rate"].max() > 1.0
    assert ref["rate"][CS.NO_PATH_USER] == 0 and (ref["size"] == 0).sum() == 1 and np.all(ref["rate"][ref["size"] == 0] == 0)
    # two users with the same rays on the same beam: the signal is the interference, 1 bit at most and nearly so at high SNR
    r, op2 = _los_ula([1, 1])
    for k in RAY_KEYS:
        r[k][1] = r[k][0]
    H = MR.oracle_channels(r, op2)
    F8 = CS.codebook("dft", [8, 1])
    idx, size = MR.link_table([1, 1], [[0, 1]], 2)
    rate = MR.mu_rate(H, F8, idx, size, 1e6)[0]
    assert np.all(rate < 1.0) and np.all(rate > 0.999) and rate[0] == rate[1]
    # beams orthogonal to each other's direction: the multi-user rate is the single-user rate at snr / g
    beam_of_user = [0, 1, 2, 3, 2]
    r, op3 = _los_ula(beam_of_user)
    H = MR.oracle_channels(r, op3)
    groups = [[0, 1, 2, 3], [4, -1, -1, -1]]
    idx, size = MR.link_table(beam_of_user, groups, 5)
    snr = 100.0
    mu = MR.mu_rate(H, F8, idx, size, snr)[0]
    alone_idx, alone_size = MR.link_table(beam_of_user, np.arange(5)[:, None], 5)
    for g in (1, 4):
        alone = MR.mu_rate(H, F8, alone_idx, alone_size, snr / g)[0]
        assert np.abs(mu - alone)[size == g].max() <= 1e-6 and alone.min() > 1.0
    assert size.tolist() == [4, 4, 4, 4, 1]
    # and without the split it is not
    assert np.abs(MR.mu_rate(H, F8, idx, size, snr, split=False)[0] - mu)[size == 4].min() > 1.0


_MULTI = [name for name in CS.MU_CASES if CS.MU_CASES[name][4] > 1]


@pytest.mark.parametrize("name", _MULTI)
def test_the_cases_tell_a_wrong_table_exchanged_beams_and_a_missing_split_apart(name):
    case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
    n = rays["power"].shape[0]
    ref = MR.mu_reference(rays, op, F, beams, groups, snr_db)
    H, snr, size = ref["H"], 10 ** (snr_db / 10), ref["size"]
    multi = size >= 2
    wrong = {"partners of the next group": MR.mu_rate(H, F, MR.link_table(beams, groups, n, shift=1)[0], size, snr)[0],
             "own and first partner's beam exchanged": MR.mu_rate(H, F, MR.link_table(beams, groups, n, swap=True)[0], size, snr)[0],
             "no power split": MR.mu_rate(H, F, ref["idx"], size, snr, split=False)[0]}
    for what, rate in wrong.items():
        far = (np.abs(rate - ref["rate"]) > 10 * ref["tol"]) & multi
        print(f"{name}: {what}: {far.sum()} of {multi.sum()} users in groups of two or more move by more than 10 tolerances; "
              f"median move {np.median(np.abs(rate - ref['rate'])[multi] / ref['tol'][multi]):.3g} tolerances")
        assert 2 * far.sum() >= multi.sum(), what
    # the tolerance is small against the rates it guards
    live = multi & (ref["rate"] > 0)
    assert np.median(ref["tol"][live] / ref["rate"][live]) < 0.05


def test_the_cases_cover_what_they_have_to():
    seen = {k: set() for k in ("G", "m_rx", "K", "P", "snr", "rays")}
    for name, (changes, n, L, cb, G, snr_db, place, shift) in CS.MU_CASES.items():
        case = {**CS.BASE, **changes}
        seen["G"].add(G), seen["m_rx"].add(int(np.prod(case["ue_shape"]))), seen["K"].add(len(case["selected"]))
        seen["P"].add(case["num_paths"]), seen["snr"].add(snr_db), seen["rays"].add(place)
        assert n <= 70 and case["num_paths"] <= L
        r = CS.rays(n, L, seed=20 + G)
        counts = (~np.isnan(r["power"])).sum(axis=1)
        assert counts[CS.NO_PATH_USER] == 0 and counts[CS.ONE_PATH_USER] == 1
    assert seen == {"G": {1, 2, 4, 8}, "m_rx": {1, 2, 4, 8}, "K": {1, 64, 70, 130}, "P": {3, 25, 32}, "snr": {-10.0, 10.0, 30.0},
                    "rays": {"host", "hbm"}}
    seen = {k: set() for k in ("bs", "ue", "K", "beams", "pattern", "rays")}
    for name, (changes, n, L, cb, beams, place) in CS.VIEW_CASES.items():
        case = {**CS.BASE, **changes}
        seen["bs"].add(tuple(case["bs_shape"])), seen["ue"].add(tuple(case["ue_shape"])), seen["K"].add(len(case["selected"]))
        seen["beams"].add(beams if isinstance(beams, str) else beams[0]), seen["pattern"].add(case["bs_pattern"]), seen["rays"].add(place)
    assert seen == {"bs": {(8, 1), (4, 2), (3, 5), (8, 8)}, "ue": {(1, 1), (2, 1), (2, 2)}, "K": {1, 5, 64, 70},
                    "beams": {"all", "per_user", "table"}, "pattern": {"isotropic", "halfwave-dipole", "tr38901"},
                    "rays": {"host", "hbm"}}
    assert any({**CS.BASE, **c[0]}["bs_fov"] is not None and any({**CS.BASE, **c[0]}["bs_rot"]) for c in CS.VIEW_CASES.values())


# ---------------------------------------------------------------------------------------------- 6. the identity
def _links_through_the_oracle(case, op, rays, F, idx, scale, fov=(None, None)):
    """[J, n, M_rx, K]: the oracle's channels from a single-antenna base station on the ray matrices `precode_rays` gives"""
    import copy
    from deepmimo_amd.combiner import precode_rays
    prep = MR.R.prepared(rays, op, *fov)
    one = copy.deepcopy(op)
    one["bs_antenna"]["shape"] = np.array([1, 1])
    out = []
    for j in range(len(idx)):
        power, phase = precode_rays(rays["power"], rays["phase"], F, idx[j:j + 1], case["bs_shape"], case["bs_spacing"],
                                    prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"], None if scale is None else scale[j:j + 1])
        out.append(MR.oracle_channels({**rays, "power": power, "phase": phase}, one, *fov)[:, :, 0, :])
    return np.stack(out)


@pytest.mark.parametrize("name", list(CS.VIEW_CASES))
def test_a_single_bs_antenna_on_precoded_rays_gives_the_precoded_channel(name):
    """What the view rests on, without the GPU: the oracle in place of the kernels, within the tolerance of the GPU test."""
    case, op, fov, rays, F, beams, _ = CS.view_setup(name)
    n, B = rays["power"].shape[0], len(F)
    idx = np.broadcast_to(np.arange(B)[:, None], (B, n)) if beams is None else np.asarray(beams).reshape(-1, n)
    ref, tol = MR.view_reference(rays, op, F, idx, *fov)
    got = _links_through_the_oracle(case, op, rays, F, idx, None, fov)
    assert MR.R.worst_ratio(got, ref, tol, what=name) <= 1.0
    assert (tol > 0).sum() >= len(idx) * 3 and np.all(tol[:, CS.NO_PATH_USER] == 0) and np.all(tol[idx < 0] == 0)


@pytest.mark.parametrize("name", list(CS.MU_CASES))
def test_links_on_precoded_rays_give_the_reference_rate(name):
    """What `compute_mu_rate` rests on, without the GPU: G single-antenna links on the precoded, power-split ray matrices,
    their channels from the oracle, through the cell-rate definition - within the tolerance the GPU test holds the call to."""
    from tests import _cell_rate_ref as CR
    case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
    ref = MR.mu_reference(rays, op, F, beams, groups, snr_db)
    G = len(ref["idx"])
    Y = _links_through_the_oracle(case, op, rays, F, ref["idx"], MR.split_scale(ref["size"], G))
    rate, rate_k = CR.cell_rate_from_channels([Y[j][:, :, None, :] for j in range(G)], [10 ** (snr_db / 10)] * G,
                                              np.where(ref["size"] > 0, 0, -1))
    assert MR.worst(rate, ref["rate"], ref["tol"], what=f"{name}: rate") <= 1.0
    assert MR.worst(rate_k, ref["rate_k"], ref["tol_k"], what=f"{name}: rate_k") <= 1.0
