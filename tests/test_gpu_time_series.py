"""Channel time series on the GPU: `compute_channels(times=...)` on every route against the NumPy oracle on unwrapped float64
phases, time zero bit for bit, the array-shift identity that pins the sign of `set_velocities`, the consumers through the
`at_times` view, `MacroDataset.at_times`, blocks of snapshots, and device-resident rays.

13 users x 25 paths, three snapshots at (0, 1e-4, 0.7) s, f_c = 28 GHz (passed as `carrier_freq`) unless a test says
otherwise.  The references and the channel tolerance - TOL_REL of the user's peak plus 2 pi 2^-24 sum |c_l| for the float32
rounding of the advanced phase - are those of tests/_time_series_ref.py."""
import os

import numpy as np
import pytest

from tests import _time_series_ref as R
from tests._cases import TOL_REL, oracle_params

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_parity import _dm_params  # noqa: E402

N_UE, L, FC = 13, 25, 28e9
TIMES = (0.0, 1e-4, 0.7)
FC_RT = 3.5e9                                  # rt_params.frequency where a case sets it: the v3 term's, not the advance's

BASE = dict(bs_shape=[8, 1], ue_shape=[1, 1], bs_spacing=0.5, ue_spacing=0.5, bs_rot=[0, 0, 0], bs_pattern="isotropic",
            ue_pattern="isotropic", num_paths=L, freq_domain=1, subcarriers=512, selected=[0], bandwidth=10e6, rx_filter=0,
            bs_fov=None, ue_fov=None)
_K64 = dict(subcarriers=64, selected=list(range(64)))
_4X2 = dict(bs_shape=[4, 2], ue_shape=[2, 1])
_PER_USER_ROT = np.random.default_rng(3).uniform(-60, 60, (N_UE, 3))

# name -> (changes of BASE, fd_kernel_variant, the route the call has to take, extras)
# routes: "direct" the single pass; an int the stage-2 kernel (for variant 0 the library's own choice); "lpf"; "td"
CASES = {
    "single_pass_K1_defaults": ({}, 0, "direct", {}),
    "folded_K64_8x1": (_K64, 0, 12, {}),
    "matrix_core_K64_4x2_2x1": ({**_K64, **_4X2}, 2, 2, {}),
    "vector_K64_4x2_2x1": ({**_K64, **_4X2}, 1, 1, {}),
    "rx_filter_N64": (dict(subcarriers=64, selected=list(range(0, 64, 3)), rx_filter=1, **_4X2), 0, "lpf", {}),
    "time_domain": (dict(freq_domain=0, **_4X2), 0, "td", {}),
    "bs_rotation_and_fov": ({**_K64, **_4X2, "bs_rot": [10, -20, 30], "bs_fov": [150, 100]}, 0, None, {}),
    "per_user_ue_rotation": ({**_K64, **_4X2}, 0, None, dict(ue_rot=_PER_USER_ROT)),
    "v3_doppler_on_top": ({**_K64, **_4X2}, 0, None, dict(enable_doppler=1)),
}


def _rays(seed=5, with_doppler=True):
    from oracle import oracle_np as onp
    return onp.synth_rays(N_UE, L, seed=seed, with_doppler=with_doppler)


def _dataset(rays, case=BASE):
    import deepmimo_amd as dm
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    if case["bs_fov"] is not None:
        ds.apply_fov(bs_fov=np.array(case["bs_fov"]))
    return ds


def _setup(name):
    """(case, dataset, package parameters, oracle parameters, FoV arguments of the oracle, rays) of CASES[name]"""
    changes, variant, route, extra = CASES[name]
    case = {**BASE, **changes}
    rays = _rays()
    ue_rot = np.asarray(extra.get("ue_rot", [0, 0, 0]))
    p, op = _dm_params(case, ue_rot), oracle_params(case, ue_rot)
    ds = _dataset(rays, case)
    if extra.get("enable_doppler"):
        p.enable_doppler = 1
        op["enable_doppler"] = 1
        ds["rt_params"] = {"frequency": FC_RT}
    fov = (np.array(case["bs_fov"]), np.array([360, 180])) if case["bs_fov"] is not None else (None, None)
    return case, ds, p, op, fov, rays


_refs = {}


def _reference(name, times=TIMES):
    """(reference channels [T, n, ...], sum of the path moduli [n]) of a case, computed once"""
    key = (name, tuple(times))
    if key not in _refs:
        case, ds, p, op, fov, rays = _setup(name)
        _refs[key] = (R.reference_channels(rays, op, times, FC, *fov, doppler_fc=FC_RT), R.path_moduli_sum(rays, op, *fov))
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


@pytest.fixture
def calls(monkeypatch):
    """the engine calls a test makes, in order: (name, positional arguments, keywords)"""
    from deepmimo_amd.engine import ChannelEngine
    log = []
    for name in ("prepare", "channels", "channels_direct"):
        real = getattr(ChannelEngine, name)

        def spy(self, *a, _real=real, _name=name, **k):
            log.append((_name, a, k))
            return _real(self, *a, **k)
        monkeypatch.setattr(ChannelEngine, name, spy)
    return log


def _assert_route(calls, route, variant):
    """the calls of ONE block: a single pass, or one stage 1 and one stage 2 on the kernel the case names"""
    from deepmimo_amd.dataset import _engine
    names = [c[0] for c in calls]
    if route == "direct":
        assert names == ["channels_direct"], names
        return
    assert names == ["prepare", "channels"], names
    prep, kw = calls[1][1][0], calls[1][2]
    p = prep.params_struct
    assert kw["variant"] == variant
    if route == "lpf":
        assert p.freq_domain == 1 and p.rx_filter == 1
    elif route == "td":
        assert p.freq_domain == 0
    elif route is not None:
        assert p.freq_domain == 1 and p.rx_filter == 0
        ran = variant if variant else _engine().auto_fd_choice(p, prep.n_paths_loaded, prep.sc_abs_max)
        assert ran == route, (ran, route)


# ---------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", list(CASES))
def test_series_matches_the_oracle_on_every_route(name, calls):
    import deepmimo_amd as dm
    case, ds, p, op, fov, rays = _setup(name)
    variant, route = CASES[name][1], CASES[name][2]
    H_ref, moduli = _reference(name)
    dm.config("fd_kernel_variant", variant)
    try:
        H = ds.compute_channels(p, times=TIMES, carrier_freq=FC)
        first_call = list(calls)
        one = ds.compute_channels(p, times=TIMES[2], carrier_freq=FC)       # a scalar: the one snapshot, no leading axis
    finally:
        dm.config("fd_kernel_variant", 0)
    _assert_route(first_call, route, variant)
    assert isinstance(H, np.ndarray) and H.shape == (len(TIMES), N_UE) + H_ref.shape[2:]
    R.assert_series_close(H, H_ref, moduli, what=name)
    assert "channel" not in ds.keys()                                     # nothing is cached
    # the snapshots differ by far more than the tolerance: the comparison can fail
    d = np.abs(H_ref[2].astype(np.complex128) - H_ref[0]).reshape(N_UE, -1).max(axis=1)
    assert (d > 100 * R.channel_tolerance(H_ref, moduli)[0]).sum() >= N_UE // 2
    assert one.shape == H.shape[1:] and np.array_equal(one, H[2])


# ---------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", ["single_pass_K1_defaults", "matrix_core_K64_4x2_2x1"])
def test_time_zero_is_the_call_without_times(name):
    import deepmimo_amd as dm
    case, ds, p, op, fov, rays = _setup(name)
    variant = CASES[name][1]
    dm.config("fd_kernel_variant", variant)
    try:
        plain = _dataset(rays, case).compute_channels(p)
        at_zero = ds.compute_channels(p, times=[0.0], carrier_freq=FC)
        assert at_zero.shape == (1,) + plain.shape and at_zero[0].tobytes() == plain.tobytes()
        still = {k: v.copy() for k, v in rays.items()}
        still["doppler_vel"] = np.zeros_like(still["doppler_vel"])
        still["doppler_acc"] = np.zeros_like(still["doppler_acc"])
        ds0 = _dataset(still, case)
        series = ds0.compute_channels(p, times=TIMES, carrier_freq=FC)
        first = ds0.compute_channels(p, times=[0.0], carrier_freq=FC)[0]
    finally:
        dm.config("fd_kernel_variant", 0)
    assert first.tobytes() == plain.tobytes()
    for t in range(len(TIMES)):
        assert series[t].tobytes() == first.tobytes(), t


# ---------------------------------------------------------------------------------------------- G3
def _shift_case():
    case = {**BASE, "bs_shape": [4, 1], "ue_shape": [4, 1], "subcarriers": 64, "selected": list(range(16))}
    return case, _dm_params(case, np.zeros(3)), oracle_params(case, np.zeros(3))


def _shift_series(rx_vel):
    """(H at t = 0 and at the time a UE moving at 10 m/s along y has covered half a wavelength, the tolerance [n])"""
    fc, v = 3.5e9, 10.0
    t = 0.5 * R.LIGHTSPEED / (fc * v)
    case, p, op = _shift_case()
    rays = _rays(seed=9, with_doppler=False)
    ds = _dataset(rays, case)
    ds.set_velocities(rx_vel=rx_vel)
    H = ds.compute_channels(p, times=[0.0, t], carrier_freq=fc)
    peak = np.abs(H[0]).reshape(N_UE, -1).max(axis=1)
    tol = 2 * (TOL_REL * peak + 2 * np.pi * 2.0 ** -24 * R.path_moduli_sum(rays, op))
    return H.astype(np.complex128), tol


def test_moving_one_antenna_spacing_is_shifting_the_array_by_one_element():
    """UE elements lie along y, half a wavelength apart: after v t = lambda / 2 along y, element r stands where element
    r + 1 stood.  Both sides come from the GPU; the tolerance is twice the channel tolerance (one per side)."""
    H, tol = _shift_series((0.0, 10.0, 0.0))
    assert (tol > 0).sum() >= N_UE // 2
    for r in range(3):
        d = np.abs(H[1][:, r] - H[0][:, r + 1]).reshape(N_UE, -1).max(axis=1)
        print(f"shift identity, element {r}: worst error / bound {np.max(d[tol > 0] / tol[tol > 0]):.3f}")
        assert np.all(d <= tol), r
    # the opposite sign moves the array the other way, and the identity fails by far more than the tolerance
    Hm, _ = _shift_series((0.0, -10.0, 0.0))
    d = np.abs(Hm[1][:, 0] - Hm[0][:, 1]).reshape(N_UE, -1).max(axis=1)
    assert (d > 100 * tol).sum() >= N_UE // 2
    assert np.all(np.abs(Hm[1][:, 1] - Hm[0][:, 0]).reshape(N_UE, -1).max(axis=1) <= tol)


# ---------------------------------------------------------------------------------------------- G4
_CONSUMER = {**BASE, **_4X2, "subcarriers": 64, "selected": list(range(16))}


def _consumer_reference():
    if "consumer" not in _refs:
        rays = _rays()
        _refs["consumer"] = R.reference_channels(rays, oracle_params(_CONSUMER, np.zeros(3)), TIMES, FC)
        _refs["consumer"].setflags(write=False)
    return _refs["consumer"]


def test_rate_through_the_view():
    from tests._rate_ref import median_snr, rate_from_channel, rate_tolerance
    H_ref = _consumer_reference()
    p = _dm_params(_CONSUMER, np.zeros(3))
    view = _dataset(_rays(), _CONSUMER).at_times(TIMES, carrier_freq=FC)
    assert view.n_ue == len(TIMES) * N_UE
    # the issue's 10 dB, and the SNR that puts the median user of the reference at 20 dB, where the rate is of order 1
    for snr_db in (10.0, 10 * np.log10(median_snr(H_ref[0]))):
        rate = view.split_times(view.compute_rate(p, snr_db=snr_db))
        assert rate.shape == (len(TIMES), N_UE) and rate.dtype == np.float32
        for t in range(len(TIMES)):
            want, _ = rate_from_channel(H_ref[t], 10 ** (snr_db / 10))
            tol, _ = rate_tolerance(H_ref[t], 10 ** (snr_db / 10))
            ratio = np.max(np.abs(rate[t] - want) / tol)
            print(f"rate at {snr_db:.1f} dB, snapshot {t}: worst error / bound {ratio:.3f}, largest rate {want.max():.3g}")
            assert ratio <= 1.0
    # at the second SNR the snapshots differ by more than the tolerance
    big = 10 ** (snr_db / 10)
    assert np.any(np.abs(rate_from_channel(H_ref[2], big)[0] - rate_from_channel(H_ref[0], big)[0]) > 10 * rate_tolerance(H_ref[0], big)[0])


def test_beam_power_through_the_view():
    import deepmimo_amd as dm
    from tests._path_count_cases import BOUND_BEAM_POWER
    H_ref = _consumer_reference().astype(np.complex128)
    F = dm.dft_codebook(_CONSUMER["bs_shape"])
    assert F.shape == (8, 8)
    view = _dataset(_rays(), _CONSUMER).at_times(TIMES, carrier_freq=FC)
    pwr = view.split_times(view.compute_beam_power(F, _dm_params(_CONSUMER, np.zeros(3))))
    amp = view.split_times(view["beam_mean_amplitude"])
    assert pwr.shape == amp.shape == (len(TIMES), N_UE, 8)
    for t in range(len(TIMES)):
        want = np.abs(F.astype(np.complex128) @ H_ref[t]).mean(axis=1).mean(axis=-1)          # [n, 8]
        has = want.max(axis=1) > 0
        ratio = (np.abs(amp[t] - want)[has] / (BOUND_BEAM_POWER * want[has].max(axis=1, keepdims=True))).max()
        print(f"beam power, snapshot {t}: worst amplitude error / bound {ratio:.3f}")
        assert ratio <= 1.0 and np.all(amp[t][~has] == 0) and np.all(np.isnan(pwr[t][~has]))


# ---------------------------------------------------------------------------------------------- G5
def test_cell_rate_over_time():
    import deepmimo_amd as dm
    from tests._cell_rate_ref import cell_rate_from_channels, cell_rate_tolerance, link_snrs
    p, op = _dm_params(_CONSUMER, np.zeros(3)), oracle_params(_CONSUMER, np.zeros(3))
    rays = [_rays(seed=1), _rays(seed=2)]
    H_refs = [R.reference_channels(r, op, TIMES, FC) for r in rays]                     # [B][T, n, ...]
    macro = dm.MacroDataset([_dataset(r, _CONSUMER) for r in rays]).at_times(TIMES, carrier_freq=FC)
    T = len(TIMES)
    snrs_20 = [10 * np.log10(s) for s in link_snrs([H[0] for H in H_refs])]
    for snr_db in (10.0, snrs_20):
        rate, serving, link_snr = macro.compute_cell_rate(p, snr_db=snr_db, details=True)
        rate, serving = macro.split_times(rate), macro.split_times(serving)
        assert rate.shape == (T, N_UE) and all(np.array_equal(serving[t], serving[0]) for t in range(T))
        lin = [10 ** (s / 10) for s in (snr_db if isinstance(snr_db, list) else [snr_db] * 2)]
        for t in range(T):
            Hs = [H[t] for H in H_refs]
            want, _ = cell_rate_from_channels(Hs, lin, serving[t])
            tol, _ = cell_rate_tolerance(Hs, lin, serving[t])
            ratio = np.max(np.abs(rate[t] - want) / tol)
            print(f"cell rate, snapshot {t}: worst error / bound {ratio:.3f}, largest rate {want.max():.3g}")
            assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------- G6
TIMES5 = (0.0, 1e-4, 3e-3, 0.05, 0.7)


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_series_in_three_blocks(output, calls, monkeypatch):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    name = "folded_K64_8x1"
    case, ds, p, op, fov, rays = _setup(name)
    H_ref, moduli = _reference(name, TIMES5)
    monkeypatch.setattr(dsm, "_TIME_BLOCK_BYTES", 2 * 4 * N_UE * L * 10)   # two snapshots of ten ray matrices
    assert ds._time_blocks(5) == [(0, 2), (2, 2), (4, 1)]
    dm.config("channel_output", output)
    try:
        H = ds.compute_channels(p, times=TIMES5, carrier_freq=FC)
    finally:
        dm.config("channel_output", "numpy")
    assert [c[0] for c in calls] == ["prepare", "channels"] * 3             # one stage 1 and one stage 2 per block
    assert [c[1][0].n_ue for c in calls[1::2]] == [2 * N_UE, 2 * N_UE, N_UE]
    if output == "torch":
        assert H.is_cuda and H.is_contiguous()
        H = H.cpu().numpy()
    R.assert_series_close(H, H_ref, moduli, what=f"three blocks, {output}")


def test_iter_channels_over_time_in_blocks_and_chunks(calls, monkeypatch):
    from deepmimo_amd import dataset as dsm
    name = "folded_K64_8x1"
    case, ds, p, op, fov, rays = _setup(name)
    H_ref, moduli = _reference(name, TIMES5)
    monkeypatch.setattr(dsm, "_TIME_BLOCK_BYTES", 2 * 4 * N_UE * L * 10)
    H = np.zeros(H_ref.shape, np.complex64)
    seen = []
    for t, b, chunk in ds.iter_channels(p, 5, times=TIMES5, carrier_freq=FC):
        seen.append((t, b))
        assert chunk.shape == (min(5, N_UE - b),) + H_ref.shape[2:]
        H[t, b:b + len(chunk)] = chunk
    assert seen == [(t, b) for t in range(5) for b in (0, 5, 10)]
    assert [c[0] for c in calls].count("prepare") == 3
    R.assert_series_close(H, H_ref, moduli, what="iter_channels over time")
    # without times: today's pairs
    pairs = [(b, c.shape[0]) for b, c in ds.iter_channels(p, 5)]
    assert pairs == [(0, 5), (5, 5), (10, 3)]


# ---------------------------------------------------------------------------------------------- G7
def test_device_resident_rays_and_torch_output(calls):
    import torch
    import deepmimo_amd as dm
    name = "single_pass_K1_defaults"
    case, _, p, op, fov, rays = _setup(name)
    H_ref, moduli = _reference(name)
    ds = dm.Dataset({k: torch.from_numpy(v.copy()).cuda() for k, v in rays.items()})
    view = ds.at_times(TIMES, carrier_freq=FC)
    assert view.phase.is_cuda and view.phase.dtype == torch.float32 and tuple(view.phase.shape) == (len(TIMES) * N_UE, L)
    assert view.delay.is_cuda and view.n_ue == len(TIMES) * N_UE
    host = _dataset(rays).at_times(TIMES, carrier_freq=FC).phase
    got = view.phase.cpu().numpy()
    ok = ~np.isnan(host)
    assert np.array_equal(np.isnan(got), np.isnan(host))
    assert np.all(np.abs(R.wrap_deg(got[ok].astype(np.float64) - host[ok])) <= R.PHASE_ULP_DEG)
    assert got[:N_UE].tobytes() == rays["phase"].tobytes()
    dm.config("channel_output", "torch")
    try:
        H = ds.compute_channels(p, times=TIMES, carrier_freq=FC)
    finally:
        dm.config("channel_output", "numpy")
    _assert_route(calls, "direct", 0)
    assert isinstance(H, torch.Tensor) and H.is_cuda and H.dtype == torch.complex64
    R.assert_series_close(H.cpu().numpy(), H_ref, moduli, what="device-resident rays, torch output")
    # set_velocities where the angles live
    plain = {k: v for k, v in rays.items() if not k.startswith("doppler")}
    dev = dm.Dataset({k: torch.from_numpy(v.copy()).cuda() for k, v in plain.items()})
    cpu = _dataset(plain)
    for d in (dev, cpu):
        d.set_velocities(rx_vel=(3.0, -4.0, 1.0), tx_vel=(0.5, 0.0, -2.0))
    assert dev.doppler_vel.is_cuda and dev.doppler_acc.is_cuda and dev.doppler_vel.dtype == torch.float32
    a, b = dev.doppler_vel.cpu().numpy(), cpu.doppler_vel
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.all(np.abs(a - b)[~np.isnan(b)] <= np.abs(np.spacing(b[~np.isnan(b)])) + 1e-12)
