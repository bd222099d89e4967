"""GPU parity of the matrix-core kernel's factorised B' (uniformly spaced selections, k2_mfma_frag.h fact_b_step) and
of its packed last K-step (<= 2 paths in it), against the NumPy oracle.  Same tolerance as test_gpu_parity.py; LoS
and path counts bit-exact."""
import numpy as np
import pytest

from tests._cases import oracle_params, assert_channel_close, channel_err
from tests._path_count_cases import flat as _flat
from tests.test_gpu_parity import _dm_params

pytestmark = pytest.mark.gpu

# with every kept path within 6 dB of the strongest, an error in the weakest (last) K-step is an error of the channel:
# dropping the packed step's lo terms would leave ~2^-11 of a path's amplitude (~1e-4 of the peak), the 3-term
# products leave ~2e-6
TAIL_TOL = 1e-5


def _case(bs, ue, L, N, sel):
    return dict(bs_shape=bs, ue_shape=ue, bs_spacing=0.5, ue_spacing=0.37, bs_rot=[0, 0, 0],
                bs_pattern="isotropic", ue_pattern="isotropic", num_paths=L, freq_domain=1, subcarriers=N,
                selected=sel, bandwidth=20e6, rx_filter=0, bs_fov=None, ue_fov=None)


def _channels(rays, case, monkeypatch=None, sincos=False, doppler=False):
    """the library's channels; sincos=True withholds the uniform-spacing hint (dmx_params.sc_stride = 0), which sends
    the same selection through the sin/cos B' generation"""
    import deepmimo_amd as dm
    import deepmimo_amd.engine as eng
    if sincos:
        monkeypatch.setattr(eng, "uniform_stride", lambda sel: (0, 0))
    try:
        ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
        p = _dm_params(case, np.zeros(3))
        if doppler:
            ds["rt_params"] = {"frequency": 3.5e9}
            p.enable_doppler = 1
        return ds.compute_channels(p)
    finally:
        if sincos:
            monkeypatch.undo()


def _run(n, L, bs, ue, N, sel, variant, all_valid=True, max_delay=40e-6, seed=0):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=seed, all_valid=all_valid, max_delay=max_delay)
    case = dict(bs_shape=bs, ue_shape=ue, bs_spacing=0.5, ue_spacing=0.37, bs_rot=[0, 0, 0],
                bs_pattern="isotropic", ue_pattern="isotropic", num_paths=L, freq_domain=1, subcarriers=N,
                selected=sel, bandwidth=20e6, rx_filter=0, bs_fov=None, ue_fov=None)
    ue_rot = np.zeros(3)
    ref = onp.compute_channels(rays, oracle_params(case, ue_rot))
    dm.config("fd_kernel_variant", variant)
    try:
        ds = dm.Dataset(dict(rays))
        H = ds.compute_channels(_dm_params(case, ue_rot))
    finally:
        dm.config("fd_kernel_variant", 0)
    assert_channel_close(H, ref["channel"], what=f"{n} users L={L} {bs}x{ue} N={N} K={len(sel)} v{variant}")
    np.testing.assert_array_equal(ds.los, ref["los"])
    np.testing.assert_array_equal(ds.num_paths, ref["num_paths"])


# every kept path valid: n_keep = L, i.e. 1, 2, 3 and 8 paths in the last K-step (packed for 1 and 2)
@pytest.mark.parametrize("variant", [0, 4, 5])
@pytest.mark.parametrize("L", [25, 26, 27, 32])
def test_last_k_step_occupancy(L, variant):
    _run(24, L, [8, 8], [2, 2], 512, list(range(512)), variant, seed=L)


@pytest.mark.parametrize("L", [1, 2, 9, 10])
def test_packed_tail_on_short_chains(L):
    _run(16, L, [8, 8], [2, 2], 128, list(range(128)), 0, seed=100 + L)


@pytest.mark.parametrize("sel", [
    list(range(0, 512, 2)),                        # stride 2
    list(range(37, 37 + 3 * 150, 3)),              # stride 3, first != 0, K = 150 (not a multiple of 16)
    list(range(5, 5 + 41)),                        # stride 1, first != 0, K = 41
    [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377],   # not uniformly spaced: the sin/cos path
], ids=["stride2", "stride3_first37", "stride1_first5", "irregular"])
@pytest.mark.parametrize("L", [25, 26])
def test_selections(sel, L):
    _run(20, L, [8, 8], [2, 2], 512, sel, 0, seed=7 * L)


def test_random_path_counts_and_small_row_blocks():
    # valid paths per user 0..L (some users with one or two kept paths), 32 rows (the run-time-guarded tile body)
    _run(64, 25, [8, 4], [1, 1], 256, list(range(256)), 0, all_valid=False, seed=3)
    _run(64, 25, [8, 8], [2, 2], 256, list(range(256)), 0, all_valid=False, seed=4)


# flattened powers: the packed last K-step carries a path as strong as the others, and its error is measured tightly;
# the same selection without the spacing hint takes the sin/cos generation - a different rounding, so the two results
# must differ somewhere (the factorised kernel did run) while both meet the oracle
@pytest.mark.parametrize("L", [25, 26, 27, 32])
def test_flat_powers_tail_error_and_factorised_path_taken(L, monkeypatch):
    from oracle import oracle_np as onp
    rays = _flat(onp.synth_rays(24, L, seed=200 + L, all_valid=True, max_delay=40e-6), L)
    case = _case([8, 8], [2, 2], L, 512, list(range(512)))
    ref = onp.compute_channels(rays, oracle_params(case, np.zeros(3)))["channel"]
    H = _channels(rays, case)
    Hs = _channels(rays, case, monkeypatch, sincos=True)
    for what, X in (("factorised", H), ("sin/cos", Hs)):
        d, peak = channel_err(X, ref)
        assert np.max(d / peak) <= TAIL_TOL, (what, L, float(np.max(d / peak)))
    assert not np.array_equal(H, Hs), "the uniform selection did not take the factorised B' generation"


def test_doppler_c5_shaped(monkeypatch):
    """Doppler term on a c5-shaped sample (16x16 BS, 4x4 UE, 1024 subcarriers): factorised vs sin/cos generation of
    the same selection, flattened powers"""
    from oracle import oracle_np as onp
    rays = _flat(onp.synth_rays(6, 25, seed=5, all_valid=True, max_delay=80e-6, with_doppler=True), 5)
    case = _case([16, 16], [4, 4], 25, 1024, list(range(1024)))
    H = _channels(rays, case, doppler=True)
    Hs = _channels(rays, case, monkeypatch, sincos=True, doppler=True)
    d, peak = channel_err(H, Hs)
    assert np.max(d / peak) <= TAIL_TOL, float(np.max(d / peak))
    assert not np.array_equal(H, Hs)
    assert not np.array_equal(H, _channels(rays, case)), "the Doppler term changed nothing"


def test_beam_paths_with_a_uniform_selection():
    """The beam-space contraction keeps the sin/cos generation (its A' rows are not packed): with flattened powers and
    25 kept paths a packed B' tail against unpacked beam rows would be off by ~1e-4 of the peak.  Beam power (its own
    kernel, k2c_beam_power) from the same rays against the float64 reduction of the oracle's channel."""
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    bs, ue, sel = [8, 8], [2, 2], np.arange(0, 512, 4)
    rays = _flat(onp.synth_rays(40, 25, seed=77, all_valid=True), 77)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.num_paths = 25
    p.ofdm.selected_subcarriers = sel
    op = onp.make_params(bs_antenna=dict(shape=bs), ue_antenna=dict(shape=ue), num_paths=25,
                         ofdm=dict(selected_subcarriers=sel))
    Href = onp.compute_channels(rays, op)["channel"].astype(np.complex128)
    F = np.array([dm.steering_vec(np.array(bs), phi=a).squeeze() for a in np.linspace(-60, 60, 32)])
    Yref = F @ Href
    Y = dm.Dataset(dict(rays)).compute_beam_channels(F, p)
    d, peak = channel_err(Y, Yref)
    assert np.max(d / peak) <= TAIL_TOL, float(np.max(d / peak))
    ds = dm.Dataset(dict(rays))
    ds.compute_beam_power(F, p)
    want = np.abs(Yref).mean(axis=1).mean(axis=-1)
    amp = ds["beam_mean_amplitude"]
    assert np.all(np.abs(amp - want) <= TAIL_TOL * want.max(axis=1, keepdims=True))
