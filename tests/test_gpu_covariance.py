"""Per-user spatial covariance (dmx_channel_covariance, k6_covariance.hip) on the GPU.

Reference: the definition, an einsum in complex128 of the NumPy oracle's channel tensor (tests/_covariance_ref.py;
tests/test_covariance_cpu.py pins it against the closed form the kernel evaluates).  Criterion, per user:
max|R - R_ref| <= TOL_REL * max|R_ref[u]| + TOL_ABS with the constants of tests/_cases.py, and exactly zero where the
reference is all zero.  Every case also holds the structural properties: each block equals its conjugate transpose exactly,
diagonal imaginary parts are 0 and real parts >= 0, M_rx tr(R_tx) = M_tx tr(R_rx), and a second launch is torch.equal.
Waves per workgroup and the subcarrier chunk of a shape come from the rule restated in tests/test_covariance_cpu.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests._cases import TOL_ABS, TOL_REL, golden_names, load_golden
from tests._covariance_ref import SIDES, cov_err, cov_from_channel
from tests.test_covariance_cpu import RX, TX, lds_rule

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle, _rays, _ue_rot  # noqa: E402

WORST = {}                                   # case id -> worst max|dR| / max|R_ref[u]| seen (printed by the last test)


def live_counts(n, L):
    """live paths per user, cycled: 0, 1, 2, L - 1, L"""
    return [min(L, (0, 1, 2, L - 1, L)[u % 5]) for u in range(n)]


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _cases():
    cs = []
    # DeepMIMO's defaults: 8x1 / 1x1, K = 1, 25 paths; R_rx is [N, 1, 1], the mean power
    cs.append(_case("defaults", 70, 25, [8, 1], [1, 1], 512, [0]))
    # more than one subcarrier chunk (32 subcarriers at this shape): the full selection, one below and one above a chunk
    cs.append(_case("K512", 40, 25, [8, 1], [1, 1], 512, range(512)))
    cs.append(_case("K31", 21, 25, [8, 1], [1, 1], 512, range(3, 34)))
    cs.append(_case("K33", 21, 25, [8, 1], [1, 1], 512, range(3, 36)))
    cs.append(_case("irregular", 33, 25, [4, 2], [2, 1], 512, [-3, 0, 5, 511, 512, 700, -1000, 77, 2 ** 31 - 1, -(2 ** 31), 40001]))
    # a panel with a stride-7 selection (74 subcarriers): one wave per workgroup on the BS side, two on the UE side
    cs.append(_case("panel_stride7", 23, 25, [8, 8], [2, 2], 512, range(0, 512, 7)))
    cs.append(_case("L1", 50, 1, [4, 2], [2, 1], 64, [0, 9, 63]))
    cs.append(_case("P32_num_paths_below_loaded", 19, 40, [4, 2], [2, 1], 256, [0, 17, 100], num_paths=32, all_valid=True))
    cs.append(_case("P32_num_paths_above_loaded", 19, 32, [4, 2], [2, 1], 256, [0, 17, 100], num_paths=40, all_valid=True))
    cs.append(_case("counts_and_holes", 45, 25, [4, 2], [2, 1], 512, [0, 3, 200], rays="counts"))
    cs.append(_case("counts_and_holes_L32", 25, 32, [8, 1], [1, 2], 512, [1], rays="counts"))
    # waves per workgroup: 4k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 2-wave and of a 1-wave shape
    for n in (41, 42, 43):
        cs.append(_case(f"wpb4_users{n}", n, 25, [8, 1], [1, 1], 512, [0, 5]))
    cs.append(_case("wpb2_users13", 13, 25, [8, 4], [2, 2], 512, [0, 5, 9]))
    cs.append(_case("wpb1_users7", 7, 25, [8, 8], [2, 2], 512, [0, 5]))
    # stage-1 features arrive through the records
    cs.append(_case("rot_fov_dipole", 53, 25, [4, 2], [2, 1], 512, [0, 1, 2], bs_rot=[5, -20, 60], ue_rot=[10, 20, 30],
                    bs_fov=[150, 110], ue_fov=[200, 100], bs_pattern="halfwave-dipole", ue_pattern="halfwave-dipole"))
    cs.append(_case("per_user_rot", 45, 25, [8, 1], [2, 2], 512, [0, 7], per_user_rot=True))
    cs.append(_case("doppler", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], doppler=1))
    cs.append(_case("adaptive_workspace", 61, 25, [8, 4], [2, 1], 512, range(0, 64, 3), adaptive=True))
    for c in cs:
        c["selected"] = list(c["selected"])
        c.setdefault("adaptive", False)
    return cs


# and odd arrays on either side, K = 33, every kept-path count (tests/_consumer_shapes.py)
CASES = _cases() + shapes.COVARIANCE_CASES


def test_waves_per_workgroup_of_the_listed_shapes():
    """the shapes above drive what their names say (the launcher's rule, restated on the host)"""
    by = {c["id"]: c for c in CASES}
    rule = lambda cid, side: lds_rule(by[cid]["bs_shape"], by[cid]["ue_shape"], min(by[cid]["num_paths"], by[cid]["L"]), side)   # noqa: E731
    assert rule("K512", TX) == (4, 32) and rule("K512", RX) == (4, 32)
    assert rule("wpb4_users41", TX)[0] == 4 and rule("wpb2_users13", TX)[0] == 2 and rule("wpb1_users7", TX)[0] == 1
    assert rule("panel_stride7", TX) == (1, 64) and rule("panel_stride7", RX)[0] == 2
    assert rule("m5_ue_K33", TX) == (4, 32) and rule("m5_ue_K33", RX) == (4, 32)          # K = 33: a second chunk of one
    assert rule("every_count", TX) == (4, 8) and rule("every_count", RX) == (4, 16) and rule("ue_5x3", RX) == (4, 16)


def _case_rays(c):
    if c["rays"] == "every_count":
        return shapes.every_count_rays(c)
    if c["rays"] != "counts":
        return _rays(c)
    from oracle import oracle_np as onp
    rays = onp.synth_rays(c["n"], c["L"], seed=900 + c["n"], all_valid=True, max_delay=c["max_delay"])
    keys = [k for k in rays if k not in ("rx_pos", "tx_pos")]
    rng = np.random.default_rng(4)
    for u, cnt in enumerate(live_counts(c["n"], c["L"])):
        hole = np.zeros(c["L"], bool)
        hole[cnt:] = True
        if cnt == c["L"] and u % 2:                               # NaN holes in the middle of a full row
            hole[rng.choice(c["L"], size=3, replace=False)] = True
        for k in keys:
            rays[k][u, hole] = np.nan
    return rays


def check_covariance(R_tx, R_rx, H, what, again=None):
    """The criterion and the structural properties for one launch of each side against the reference channel H"""
    import torch
    m_rx, m_tx = H.shape[1], H.shape[2]
    worst, peaks = 0.0, {}
    for side, R in (("tx", R_tx), ("rx", R_rx)):
        m = m_tx if side == "tx" else m_rx
        assert R.dtype == torch.complex64 and tuple(R.shape) == (H.shape[0], m, m) and R.is_contiguous()
        assert torch.equal(R, R.conj().transpose(1, 2)), f"{what} {side}: a block differs from its conjugate transpose"
        dg = torch.diagonal(R, dim1=1, dim2=2)
        assert bool((dg.imag == 0).all()) and bool((dg.real >= 0).all()), f"{what} {side}: diagonal"
        ref = cov_from_channel(H, side)
        d, peak = cov_err(R.cpu().numpy(), ref)
        peaks[side] = peak
        assert np.all(d[peak == 0] == 0), f"{what} {side}: a user without paths is not exactly zero"
        ratio = float(np.max(d / np.maximum(peak, 1e-300))) if d.size else 0.0
        print(f"{what} {side}: worst max|dR| / max|R_ref[u]| = {ratio:.3e}")
        worst = max(worst, ratio)
        bad = d > TOL_REL * peak + TOL_ABS
        assert not bad.any(), f"{what} {side}: {bad.sum()} users out of tolerance, worst {ratio:.3e} (tol {TOL_REL})"
    # both traces are sum |H|^2 / K; each of the M diagonal entries is within TOL_REL of its side's peak
    t_tx = m_rx * torch.diagonal(R_tx, dim1=1, dim2=2).real.double().sum(dim=1).cpu().numpy()
    t_rx = m_tx * torch.diagonal(R_rx, dim1=1, dim2=2).real.double().sum(dim=1).cpu().numpy()
    assert np.all(np.abs(t_tx - t_rx) <= m_rx * m_tx * (TOL_REL * (peaks["tx"] + peaks["rx"]) + 2 * TOL_ABS)), f"{what}: traces"
    if again is not None:
        assert torch.equal(again[0], R_tx) and torch.equal(again[1], R_rx), f"{what}: a second launch differs"
    WORST[what] = worst
    return worst


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_covariance_against_the_definition(c):
    import torch
    eng = _engine()
    rays, ue_rot = _case_rays(c), _ue_rot(c)
    p = _dm_params(c).validate(c["n"])
    kw = _kwargs(c, ue_rot)
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **kw)
    assert eng.covariance_supported(prep, "tx") and eng.covariance_supported(prep, "rx")
    first = [eng.covariance(prep, side=s) for s in SIDES]
    second = [eng.covariance(prep, side=s) for s in SIDES]
    torch.cuda.synchronize()
    H = _oracle(c, rays, ue_rot)["channel"]
    if c["rays"] == "counts":
        assert (np.abs(H).reshape(c["n"], -1).max(axis=1) == 0).sum() >= c["n"] // 5      # the users without a path
    check_covariance(first[0], first[1], H, c["id"], again=second)


def _golden_ok(name):
    case, rays, _, ref = load_golden(name)
    return bool(case["freq_domain"]) and not case["rx_filter"] and "channel" in ref and \
        1 <= min(case["num_paths"], rays["power"].shape[1]) <= 32


GOLDENS = [g for g in golden_names() if _golden_ok(g)]


def test_some_goldens_store_their_channel():
    assert len(GOLDENS) >= 5, GOLDENS


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_covariance_of_the_reference_channel(name):
    """R from the channel tensor the real reference wrote (Doppler off: `channel` is the tensor without it)"""
    import torch
    case, rays, ue_rot, ref = load_golden(name)
    n = rays["power"].shape[0]
    if np.shape(ue_rot) == (3, 2):                                      # a range: drawn as Dataset.compute_channels draws it
        np.random.seed(1001)
        ue_rot = np.random.uniform(ue_rot[:, 0], ue_rot[:, 1], (n, 3))
    c = dict(case, per_user_rot=np.ndim(ue_rot) == 2, doppler=None, ue_rot=ue_rot if np.ndim(ue_rot) == 1 else [0, 0, 0])
    p = _dm_params(c).validate(n)
    kw = _kwargs(c, ue_rot)
    kw["carrier_freq"] = 3.5e9
    rays = {k: v for k, v in rays.items() if not k.startswith("doppler")}
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", **kw)
    R = [eng.covariance(prep, side=s) for s in SIDES]
    torch.cuda.synchronize()
    check_covariance(R[0], R[1], ref["channel"], name)


def _small(n=37, L=11, bs=(4, 2), ue=(2, 1), K=3, seed=403):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=seed)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.num_paths = L
    p.ofdm.selected_subcarriers = np.arange(3, 3 + K)
    p.validate(n)
    return rays, p


@pytest.mark.parametrize("side", SIDES)
def test_user_sub_range_with_guard_regions(side):
    """user_begin > 0 with a count that is no multiple of the four waves of a workgroup: the rows of the whole launch, and
    sentinel-filled guard regions before and after the output stay untouched"""
    import torch
    n = 37
    rays, p = _small(n)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    assert lds_rule((4, 2), (2, 1), 11, TX if side == "tx" else RX)[0] == 4
    full = eng.covariance(prep, side=side)
    m = full.shape[1]
    guard, size = 1 << 16, n * m * m
    sentinel = complex(-12345.5, 54321.25)
    big = torch.full((guard + size + guard,), sentinel, dtype=torch.complex64, device="cuda")
    out = big[guard:guard + size].view(n, m, m)
    eng.covariance(prep, side=side, out=out)
    torch.cuda.synchronize()
    assert bool((big[:guard] == sentinel).all()) and bool((big[guard + size:] == sentinel).all()), "write outside the output tensor"
    assert torch.equal(out, full)
    big.fill_(sentinel)
    b, cnt = 5, 15
    eng.covariance(prep, side=side, user_begin=b, user_count=cnt, out=out[b:b + cnt])
    torch.cuda.synchronize()
    assert bool((big[:guard] == sentinel).all()) and bool((big[guard + size:] == sentinel).all())
    assert bool((out[:b] == sentinel).all()) and bool((out[b + cnt:] == sentinel).all()), "rows outside the range written"
    assert torch.equal(out[b:b + cnt], full[b:b + cnt])
    assert torch.equal(eng.covariance(prep, side=side, user_begin=b, user_count=cnt), full[b:b + cnt])


def test_largest_shape_runs_and_the_next_one_is_refused():
    """25 paths: 2 M_out + M_avg <= 765 (include/deepmimo_amd.h).  A 382-element BS array with one UE element is the last
    BS side taken - one wave, 159600 bytes of LDS - and 383 elements the first refused: ValueError from the Dataset,
    DMX_ERR_SHAPE from the engine."""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    n, L = 3, 25
    rays = onp.synth_rays(n, L, seed=77, all_valid=True)
    c = _case("largest", n, L, [382, 1], [1, 1], 512, [0, 9])
    p = _dm_params(c).validate(n)
    eng = _engine()
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, p, want_side="light", carrier_freq=28e9)
    assert eng.covariance_supported(prep, "tx") and eng.covariance_supported(prep, "rx")
    R = [eng.covariance(prep, side=s) for s in SIDES]
    torch.cuda.synchronize()
    check_covariance(R[0], R[1], _oracle(c, rays, np.zeros(3))["channel"], "largest")
    c2 = dict(c, bs_shape=[383, 1])
    p2 = _dm_params(c2).validate(n)
    prep2 = eng.prepare(dr, p2, want_side="light", carrier_freq=28e9)
    assert not eng.covariance_supported(prep2, "tx") and eng.covariance_supported(prep2, "rx")
    with pytest.raises(NativeError, match=r"status -2.*LDS"):
        eng.covariance(prep2, side="tx")
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    with pytest.raises(ValueError, match="LDS"):
        ds.compute_covariance(_dm_params(c2), side="tx")
    assert ds.compute_covariance(_dm_params(c2), side="rx").shape == (n, 1, 1)


def test_public_api_numpy_and_torch_returns_are_the_same_bits():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 4, seed=22)
    for side in SIDES:
        ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
        ds.apply_fov(bs_fov=np.array([140, 120]))
        R_np = ds.compute_covariance(p, side=side)
        dm.config("channel_output", "torch")
        try:
            R_t = ds.compute_covariance(p, side=side)
        finally:
            dm.config("channel_output", "numpy")
        assert isinstance(R_np, np.ndarray) and R_np.dtype == np.complex64 and isinstance(R_t, torch.Tensor) and R_t.is_cuda
        assert np.array_equal(R_np.view(np.int32), R_t.cpu().numpy().view(np.int32))
        # and the definition, from the channel tensor of the same dataset
        H = ds.compute_channels(p)
        d, peak = cov_err(R_np, cov_from_channel(H, side))
        assert np.all(d <= TOL_REL * peak + TOL_ABS)
        np.testing.assert_array_equal(ds.num_paths == 0, peak == 0)


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    for side in SIDES:
        both = macro.compute_covariance(p, side=side)
        assert isinstance(both, list) and len(both) == 2
        for r, got in zip((a, b), both):
            alone = dm.Dataset({k: v.copy() for k, v in r.items()}).compute_covariance(p, side=side)
            assert got.shape == alone.shape and np.array_equal(got.view(np.int32), alone.view(np.int32))


def test_zz_report_worst_ratio():
    """Last in the file: the worst ratio over every case that ran (DESIGN.md quotes it); nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f"covariance: worst max|dR| / max|R_ref[u]| over {len(WORST)} cases = {WORST[k]:.3e} ({k}); tolerance {TOL_REL}")
        assert WORST[k] <= TOL_REL
