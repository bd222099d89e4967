"""UE receive combining on the GPU: the channels of the `with_rx_combiner` view on every route against W @ H of the NumPy
oracle, a view per codebook row bit for bit, `compute_beam_pair_power` (amplitudes, the rounded powers, the best pair, NaN,
the identity codebook, blocks of UE beams), and one case each of the view under `at_times`, `compute_rate` through the view
and `MacroDataset.with_rx_combiner`.

The cases are those of tests/_combiner_cases.py - 7 users x 8 loaded paths, one user without a path and one with a single
one - and the references and tolerances those of tests/_combiner_ref.py: TOL_REL of the peak of (user, UE beam) plus the one
extra float32 rounding of phase and power, and for the beam-pair amplitudes the same two terms behind the BS codebook."""
import os

import numpy as np
import pytest

from tests import _combiner_cases as CS
from tests import _combiner_ref as R
from tests._cases import TOL_REL

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_parity import _dm_params  # noqa: E402

N, L = CS.N_UE, CS.L
NAMES = list(CS.CASES)


def _dataset(rays, case, place="host"):
    import torch
    import deepmimo_amd as dm
    put = (lambda v: torch.from_numpy(v.copy()).cuda()) if place == "hbm" else (lambda v: v.copy())
    ds = dm.Dataset({k: put(v) for k, v in rays.items()})
    if case["ue_fov"] is not None:
        ds.apply_fov(ue_fov=np.array(case["ue_fov"]))
    return ds


def _setup(name):
    """(case, dataset, package parameters, W, F, how the GPU test runs it) of CS.CASES[name]"""
    case, ue_rot, op, fov, rays, W, F = CS.setup(name)
    run = CS.CASES[name][4]
    return case, _dataset(rays, case, run["rays"]), _dm_params(case, ue_rot), W, F, run


_refs = {}


def _reference(name):
    """(ref [n, Q, M_tx, K], tol [n, Q], the rounding term [n, Q]) of a case, computed once"""
    if name not in _refs:
        case, ue_rot, op, fov, rays, W, F = CS.setup(name)
        _refs[name] = R.reference(rays, op, W, *fov)
        for a in _refs[name]:
            a.setflags(write=False)
    return _refs[name]


@pytest.fixture
def calls(monkeypatch):
    """the engine calls a test makes, in order: (name, positional arguments, keywords)"""
    from deepmimo_amd.engine import ChannelEngine
    log = []
    for name in ("prepare", "channels", "channels_direct", "beam_power"):
        real = getattr(ChannelEngine, name)

        def spy(self, *a, _real=real, _name=name, **k):
            log.append((_name, a, k))
            return _real(self, *a, **k)
        monkeypatch.setattr(ChannelEngine, name, spy)
    return log


class _configured:
    """the configuration a case runs with, put back afterwards"""

    def __init__(self, run):
        self.run = run

    def __enter__(self):
        import deepmimo_amd as dm
        direct = self.run["route"] == "direct"
        dm.config("fd_kernel_variant", 0 if direct else self.run["route"])
        dm.config("single_pass", True if direct else "auto")
        dm.config("channel_output", self.run["output"])

    def __exit__(self, *exc):
        import deepmimo_amd as dm
        dm.config("fd_kernel_variant", 0)
        dm.config("single_pass", "auto")
        dm.config("channel_output", "numpy")


def _users_first(view, H):
    """the channels [Q * n, 1, M_tx, K] of a view as NumPy [n, Q, M_tx, K], through split_rx_beams"""
    split = view.split_rx_beams(H)
    if hasattr(H, "detach"):
        assert split.data_ptr() == H.data_ptr()
        split = split.cpu().numpy()
    else:
        assert np.shares_memory(split, H)
    assert split.shape[:3] == (view.n_rx_beams, view.n_ue_per_rx_beam, 1)
    return split[:, :, 0].transpose(1, 0, 2, 3)


# ---------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", NAMES)
def test_view_channels_match_the_combined_oracle_channels(name, calls):
    import torch
    case, ds, p, W, F, run = _setup(name)
    ref, tol, _ = _reference(name)
    view = ds.with_rx_combiner(W, p)
    Q = len(W)
    assert view.n_ue == Q * N and list(view.ch_params.ue_antenna.shape) == [1, 1]
    assert hasattr(view.power, "detach") == (run["rays"] == "hbm")          # combined where the rays live
    del calls[:]
    with _configured(run):
        H = view.compute_channels()
        ran = list(calls)
        rows = [ds.with_rx_combiner(W[q:q + 1], p).compute_channels() for q in range(Q)]
    if run["route"] == "direct":
        assert [c[0] for c in ran] == ["channels_direct"], [c[0] for c in ran]
    elif run["route"]:
        assert [c[0] for c in ran] == ["prepare", "channels"] and ran[1][2]["variant"] == run["route"]
    assert isinstance(H, torch.Tensor if run["output"] == "torch" else np.ndarray)
    assert tuple(H.shape) == (Q * N, 1) + ref.shape[2:]
    got = _users_first(view, H)
    assert got.dtype == np.complex64
    ratio = R.worst_ratio(got, ref, tol, what=name)
    assert ratio <= 1.0
    assert np.all(got[CS.NO_PATH_USER] == 0)
    assert np.any(got[CS.ONE_PATH_USER] != 0) or case["ue_fov"] is not None   # a field of view may mask its one path
    # a view of one codebook row gives the rows of that UE beam, bit for bit
    for q, row in enumerate(rows):
        row = row.cpu().numpy() if hasattr(row, "detach") else row
        assert row.shape == (N, 1) + ref.shape[2:] and row[:, 0].tobytes() == np.ascontiguousarray(got[:, q]).tobytes(), q


# ---------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", NAMES)
def test_beam_pair_power(name):
    case, ds, p, W, F, run = _setup(name)
    ref, tol, second = _reference(name)
    Q, B = len(W), len(F)
    pwr, best_rx, best_tx = ds.compute_beam_pair_power(F, W, p, return_best=True)
    amp = ds["beam_pair_mean_amplitude"]
    assert isinstance(pwr, np.ndarray) and pwr.shape == amp.shape == (N, Q, B) and pwr.dtype == np.float64 and amp.dtype == np.float32
    assert best_rx.shape == best_tx.shape == (N,) and best_rx.dtype == best_tx.dtype == np.float64
    none = np.asarray(ds.los) == -1
    assert none[CS.NO_PATH_USER] and (not none[CS.ONE_PATH_USER] or case["ue_fov"] is not None)
    # the amplitudes against the reference
    want, _ = R.pair_amplitudes(ref, F)
    tol_amp = R.amplitude_tolerance(ref, second, F)
    assert np.array_equal(none, tol_amp.max(axis=(1, 2)) == 0)
    assert np.all(amp[none] == 0)
    ratio = float((np.abs(amp - want)[~none] / tol_amp[~none]).max())
    print(f"{name}: worst amplitude error / bound {ratio:.3f}")
    assert ratio <= 1.0
    # the powers are those of the returned amplitudes, NaN exactly where there is no path
    assert np.array_equal(np.isnan(pwr), np.broadcast_to(none[:, None, None], pwr.shape))
    with np.errstate(divide="ignore"):
        assert np.array_equal(pwr[~none], np.around(20 * np.log10(amp[~none]) + 30, 1))
    # the best pair is the first maximum of the returned powers
    flat = pwr.reshape(N, Q * B)
    first = np.argmax(flat[~none], axis=1)
    assert np.array_equal(best_rx[~none], first // B) and np.array_equal(best_tx[~none], first % B)
    assert np.isnan(best_rx[none]).all() and np.isnan(best_tx[none]).all()
    # and the reference's best pair is no better than it by more than the tolerance and the 0.1 dB the powers are rounded to
    want_flat, tol_flat = want.reshape(N, Q * B), tol_amp.reshape(N, Q * B)
    for u, g in zip(np.flatnonzero(~none), first):
        r = int(np.argmax(want_flat[u]))
        assert want_flat[u, g] + tol_flat[u, g] >= (want_flat[u, r] - tol_flat[u, r]) * R.ROUNDING_STEP, (u, g, r)
    # without return_best: the powers alone
    assert np.array_equal(ds.compute_beam_pair_power(F, W, p), pwr, equal_nan=True)


def test_identity_codebook_is_compute_beam_power_bit_for_bit():
    name = "ue1x1_K5_Q1_B33_identity"
    case, ds, p, W, F, run = _setup(name)
    one, best = ds.compute_beam_power(F, p, return_best=True)
    one_amp = ds["beam_mean_amplitude"].copy()
    pwr, best_rx, best_tx = ds.compute_beam_pair_power(F, W, p, return_best=True)
    assert pwr.shape == (N, 1, len(F)) and pwr[:, 0, :].tobytes() == one.tobytes()
    assert ds["beam_pair_mean_amplitude"][:, 0, :].tobytes() == one_amp.tobytes()
    assert np.array_equal(best_tx, best, equal_nan=True) and np.array_equal(best_rx, np.where(np.isnan(best), np.nan, 0.0), equal_nan=True)
    assert (~np.isnan(best)).sum() >= 3


def test_blocks_of_ue_beams_give_the_same_bits(calls, monkeypatch):
    from deepmimo_amd import dataset as dsm
    name = "ue2x2_K64_Q4_B1_tr38901_ue_fov_rot_range"
    case, ds, p, W, F, run = _setup(name)
    whole = ds.compute_beam_pair_power(F, W, p)
    whole_amp = ds["beam_pair_mean_amplitude"].copy()
    assert [c[0] for c in calls].count("beam_power") == 1
    del calls[:]
    monkeypatch.setattr(dsm, "_TIME_BLOCK_BYTES", 4 * N * L * 10 + 1)      # one UE beam of ten ray matrices
    assert ds._time_blocks(4) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    split = ds.compute_beam_pair_power(F, W, p)
    sweeps = [c for c in calls if c[0] == "beam_power"]
    assert len(sweeps) == 4 and all(c[1][0].n_ue == N for c in sweeps)
    assert split.tobytes() == whole.tobytes() and ds["beam_pair_mean_amplitude"].tobytes() == whole_amp.tobytes()


# ---------------------------------------------------------------------------------------------- G3
_PLAIN = {**CS.BASE, "selected": list(range(64))}
_W3 = CS.ue_codebook("ue2x2_K64_Q3_B33_per_user_rot_folded")


def test_combiner_on_the_time_series():
    """`at_times(t).with_rx_combiner(W)` against the time-series reference (tests/_time_series_ref.py) combined with W; the
    tolerance adds the float32 rounding of the advanced phase, 2 pi 2^-24 on the path moduli behind the combiner."""
    from tests import _time_series_ref as TS
    from tests._cases import oracle_params
    times, fc = (0.0, 1e-4, 0.7), 28e9
    rot = np.array([10, -20, 30])
    rays = CS.rays(with_doppler=True)
    op, p = oracle_params(_PLAIN, rot), _dm_params(_PLAIN, rot)
    H_t = TS.reference_channels(rays, op, times, fc).astype(np.complex128)            # [T, n, M_rx, M_tx, K]
    prep = R.prepared(rays, op)
    extra = 2 * np.pi * 2.0 ** -24 * R.combined_moduli_sum(prep, op, _W3) + R.rounding_term(rays, prep, op, _W3)
    view = _dataset(rays, _PLAIN).at_times(times, carrier_freq=fc).with_rx_combiner(_W3, p)
    Q, T = len(_W3), len(times)
    assert view.n_ue == Q * T * N and view.n_ue_per_rx_beam == T * N
    H = view.split_rx_beams(view.compute_channels())                                  # [Q, T * n, 1, M_tx, K]
    H = H.reshape((Q, T, N) + H.shape[3:])
    for t in range(T):
        ref = np.einsum("qr,urtk->uqtk", _W3, H_t[t])
        tol = TOL_REL * np.abs(ref).max(axis=(2, 3)) + extra
        assert R.worst_ratio(H[:, t].transpose(1, 0, 2, 3), ref, tol, what=f"snapshot {t}") <= 1.0
    # the snapshots differ by far more than the tolerance: the comparison can fail
    moved = np.abs(np.einsum("qr,urtk->uqtk", _W3, H_t[2] - H_t[0])).max(axis=(2, 3))
    assert (moved > 100 * tol).sum() >= Q * N // 2


def test_rate_through_the_view():
    """`compute_rate` of the view against tests/_rate_ref.py on W @ H.  That tolerance admits a channel error of TOL_REL of
    the peak; the view's admits f = tol / (TOL_REL peak) >= 1 times as much, and the rate tolerance grows by at most f^2."""
    from tests._rate_ref import median_snr, rate_from_channel, rate_tolerance
    name = "ue2x2_K64_Q3_B33_per_user_rot_folded"
    case, ds, p, W, F, run = _setup(name)
    ref, tol, _ = _reference(name)
    Q = len(W)
    H_ref = ref.transpose(1, 0, 2, 3).reshape((Q * N, 1) + ref.shape[2:])             # combiner-major single-antenna users
    peak = np.abs(ref).max(axis=(2, 3))
    f = np.where(peak > 0, tol / np.where(peak > 0, TOL_REL * peak, 1.0), 1.0).T.reshape(-1)
    view = ds.with_rx_combiner(W, p)
    for snr_db in (10.0, 10 * np.log10(median_snr(H_ref))):
        rate = view.compute_rate(snr_db=snr_db)
        assert rate.shape == (Q * N,) and rate.dtype == np.float32
        want, _ = rate_from_channel(H_ref, 10 ** (snr_db / 10))
        bound = rate_tolerance(H_ref, 10 ** (snr_db / 10))[0] * f * f
        ratio = float(np.max(np.abs(rate - want) / bound))
        print(f"rate at {snr_db:.1f} dB: worst error / bound {ratio:.3f}, largest rate {want.max():.3g}")
        assert ratio <= 1.0
        assert np.all(view.split_rx_beams(rate)[:, CS.NO_PATH_USER] == 0)
    assert want.max() > 1.0


def test_cell_rate_per_ue_beam():
    import deepmimo_amd as dm
    rot = np.array([10, -20, 30])
    p = _dm_params(_PLAIN, rot)
    kids = [_dataset(CS.rays(seed=s), _PLAIN) for s in (1, 2)]
    macro = dm.MacroDataset(kids).with_rx_combiner(_W3, p)
    Q = len(_W3)
    assert type(macro) is dm.MacroDataset and [d.n_ue for d in macro.datasets] == [Q * N, Q * N]
    rate, serving, link_snr = macro.compute_cell_rate(snr_db=110.0, details=True)
    assert rate.shape == (Q * N,) and rate.dtype == np.float32 and np.isfinite(rate).all() and rate.max() > 0
    assert macro.split_rx_beams(rate).shape == (Q, N) and link_snr.shape == (Q * N, 2)
    again = dm.MacroDataset([k.with_rx_combiner(_W3, p) for k in kids]).compute_cell_rate(snr_db=110.0, details=True)
    for a, b in zip((rate, serving, link_snr), again):
        assert a.tobytes() == b.tobytes()
    # one child is that child's compute_rate on its view
    alone = dm.MacroDataset([kids[0]]).with_rx_combiner(_W3, p).compute_cell_rate(snr_db=110.0)
    assert alone.tobytes() == kids[0].with_rx_combiner(_W3, p).compute_rate(snr_db=110.0).tobytes()
