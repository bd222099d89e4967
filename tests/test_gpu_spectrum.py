"""Per-user channel eigenmodes and water-filling rate (dmx_channel_spectrum, the second epilogue of k7_rate.hip) on the GPU.

Reference: the definition in complex128 from the NumPy oracle's channel tensor (tests/_spectrum_ref.py, pinned against hand
cases by tests/test_spectrum_cpu.py).  The inputs are the cases of tests/test_gpu_rate.py, which hit every hazard of the
shared kernel body (tests/_consumer_shapes.py adds Gram orders 3, 5, 6, 7 in both orientations, odd arrays and every kept-path
count), and rank-deficient ones at m = 4 and, from that module, at m = 3 and m = 5.  One SNR per case, from its reference alone: a tenth of
tests/_rate_ref.median_snr, the median live user at 10 dB (tests/test_spectrum_cpu.py has the share condition that picks
it; the eigenmode criterion does not depend on the SNR, both sides scale with it).  Criteria, tests/_spectrum_ref.py:
    |gamma - ref| <= tol_g                                                 every mode
    |sum_i gamma_i - snr |H_k|_F^2| <= sqrt(m) tol_g                       the trace
    |rate_k - wf64(the kernel's own gamma)| <= r                           sharp at any rank and SNR
    wf(max(ref - tol_g, 0)) - r <= rate_k <= wf(ref + tol_g) + r           the bracket (not on the rank-deficient cases:
                                                                           their half-width exceeds 1 % of the rate on
                                                                           17 % and 13 % of the entries)
    rate_k >= rate_k of dmx_channel_rate at the same SNR, minus both tolerances
and the structure: dtype, shape, contiguity, finite, >= 0, sorted descending, +0.0 for users without a path, rate = mean of
rate_k, a second launch and every launch with fewer outputs bit-equal.
"""
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests import _spectrum_ref as sr
from tests._rate_ref import median_snr, rate_tolerance

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests import test_gpu_rate as g  # noqa: E402
from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle  # noqa: E402


def _extra():
    # rank 1 and rank 2 at m = 4: Jacobi meets exact zeros, the sort meets ties
    cs = [_case("L1_m4", 50, 1, [4, 2], [2, 2], 64, [0, 9, 63]), _case("L2_m4", 50, 2, [4, 2], [2, 2], 64, [0, 9, 63])]
    for c in cs:
        c["selected"] = list(c["selected"])
        c.setdefault("adaptive", False)
    return cs


EXTRA = _extra() + shapes.RANK_CASES                 # the same at m = 3 and m = 5
RANK_ONE = {c["id"] for c in EXTRA if c["L"] == 1}
RANK_DEFICIENT = {c["id"] for c in EXTRA}
CASES = g.CASES + EXTRA
# goldens whose stored tensor breaks the share condition of the bracket (many one-path users behind a FoV or a dipole null
# under a multi-antenna UE, far above the median SNR): every criterion but the bracket, as for the two cases above
GOLDENS_WITHOUT_BRACKET = {"g03_rot_fov", "g06_dipole", "g09_random_ue_rot"}
WORST = {}                                   # case id -> (worst mode err / tol, worst rate excess over the bracket, as a ratio)


def case_snr(H):
    """the SNR of a case: the median live user at 10 dB"""
    return median_snr(H) / 10.0


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def check_spectrum(gamma, rate, rate_k, H, snr, what, bracket=True, equal_rate_k=None):
    """every criterion of the module docstring for one launch against the reference channel H"""
    import torch
    n, K, m = H.shape[0], H.shape[3], min(H.shape[1], H.shape[2])
    for t, shape in ((gamma, (n, K, m)), (rate, (n,)), (rate_k, (n, K))):
        assert t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
    ga, r, rk = gamma.cpu().numpy(), rate.cpu().numpy(), rate_k.cpu().numpy()
    for a in (ga, r, rk):
        assert np.isfinite(a).all() and (a >= 0).all(), f"{what}: NaN, inf or negative"
    assert (ga[..., :-1] >= ga[..., 1:]).all(), f"{what}: gamma is not sorted descending"
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    for a in (ga, r, rk):
        assert (a[dead] == 0).all() and not np.signbit(a[dead]).any(), f"{what}: a user without paths is not +0.0"
    ref_rate, ref_k, ref_g = sr.wf_rate_from_channel(H, snr)
    tol_g = sr.mode_tolerance(H, snr)
    live = ~dead
    eg = np.abs(ga - ref_g)
    ratio_g = float((eg[live] / tol_g[live][..., None]).max()) if live.any() else 0.0
    print(f"{what}: snr {10 * np.log10(snr):.1f} dB, m {m}, modes worst err / tol = {ratio_g:.3f}")
    assert (eg <= tol_g[..., None]).all(), f"{what}: {(eg > tol_g[..., None]).sum()} modes out of tolerance, worst {ratio_g:.3f}"
    trace = snr * (np.abs(H.astype(np.complex128)) ** 2).sum(axis=(1, 2))
    assert (np.abs(ga.astype(np.float64).sum(axis=-1) - trace) <= np.sqrt(m) * tol_g).all(), f"{what}: the trace is off"
    if what in RANK_ONE:
        assert (ga[..., 1:] <= tol_g[..., None]).all(), f"{what}: a rank-1 channel shows a second mode"
    own = sr.waterfill(ga)                                                   # float64, from the kernel's own modes
    assert (np.abs(rk - own) <= sr.log_rounding(m, own)).all(), \
        f"{what}: rate_k is not the water-filling of gamma, worst {np.abs(rk - own).max():.3e} bit"
    if m == 1:
        one = np.log2(1.0 + ga[..., 0].astype(np.float64))
        assert (np.abs(rk - one) <= sr.log_rounding(1, one)).all(), f"{what}: m = 1 is not log2(1 + gamma_0)"
    mean = rk.astype(np.float64).mean(axis=1)
    assert (np.abs(r - mean) <= K * 2.0 ** -24 * rk.max(axis=1) + 2.0 ** -24).all(), f"{what}: rate is not the mean of rate_k"
    lo, hi = sr.rate_bracket(H, snr)
    ratio_r = 0.0
    if bracket:
        up, dn = (rk - ref_k) / (hi - ref_k), (ref_k - rk) / (ref_k - lo)
        ratio_r = float(np.maximum(up, dn)[live].max()) if live.any() else 0.0
        print(f"{what}: rate worst excess / bracket = {ratio_r:.3f}, largest rate {float(ref_k.max()):.2f}")
        assert ((lo <= rk) & (rk <= hi)).all(), f"{what}: {((rk < lo) | (rk > hi)).sum()} rate_k entries outside the bracket"
        assert (np.abs(r - ref_rate) <= np.maximum(hi - ref_k, ref_k - lo).mean(axis=1)).all()
    if equal_rate_k is not None:
        _, tol_eq = rate_tolerance(H, snr)
        assert (rk >= equal_rate_k.cpu().numpy() - tol_eq - (ref_k - lo)).all(), f"{what}: below the equal-power rate"
    WORST[what] = (ratio_g, ratio_r)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_spectrum_against_the_definition(c):
    import torch
    eng = _engine()
    rays, ue_rot, H, _ = g.case_inputs(c)
    snr_db = 10 * np.log10(case_snr(H))
    snr = 10.0 ** (snr_db / 10.0)
    p = _dm_params(c).validate(c["n"])
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot))
    assert eng.spectrum_supported(prep)
    kw = dict(gamma=True, rate=True, per_subcarrier=True)
    ga, r, rk = eng.spectrum(prep, snr_db, **kw)
    again = eng.spectrum(prep, snr_db, **kw)
    only_g = eng.spectrum(prep, snr_db)
    only_r = eng.spectrum(prep, snr_db, gamma=False, rate=True)
    only_k = eng.spectrum(prep, snr_db, gamma=False, per_subcarrier=True)
    g_k = eng.spectrum(prep, snr_db, per_subcarrier=True)
    r_k = eng.spectrum(prep, snr_db, gamma=False, rate=True, per_subcarrier=True)
    equal_k = eng.rate(prep, snr_db, per_subcarrier=True)[1]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, (ga, r, rk))), "a second launch differs"
    assert torch.equal(only_g, ga) and torch.equal(only_r, r) and torch.equal(only_k, rk), "a launch with one output differs"
    assert torch.equal(g_k[0], ga) and torch.equal(g_k[1], rk) and torch.equal(r_k[0], r) and torch.equal(r_k[1], rk), \
        "a launch with two outputs differs"
    check_spectrum(ga, r, rk, H, snr, c["id"], bracket=c["id"] not in RANK_DEFICIENT, equal_rate_k=equal_k)


@pytest.mark.parametrize("name", g.GOLDENS)
def test_goldens_spectrum_of_the_reference_channel(name):
    """against eigvalsh of the channel tensor the real reference wrote (Doppler off: `channel` is the tensor without it)"""
    import torch
    from tests._cases import load_golden
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
    H = ref["channel"]
    snr_db = 10 * np.log10(case_snr(H))
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", **kw)
    assert eng.spectrum_supported(prep)
    ga, r, rk = eng.spectrum(prep, snr_db, rate=True, per_subcarrier=True)
    torch.cuda.synchronize()
    # the bracket applies where the share condition of tests/test_spectrum_cpu.py holds for the stored tensor; which goldens
    # those are is fixed here by name and checked against the condition, so none loses the check silently
    snr = 10.0 ** (snr_db / 10.0)
    share = sr.bracket_share(H, snr)
    print(f"golden {name}: share of entries with a bracket half-width > 1 % = {share:.4f}")
    assert (share > 0.05) == (name in GOLDENS_WITHOUT_BRACKET), (name, share)
    check_spectrum(ga, r, rk, H, snr, "golden " + name, bracket=name not in GOLDENS_WITHOUT_BRACKET)


def test_most_goldens_get_the_bracket():
    assert GOLDENS_WITHOUT_BRACKET <= set(g.GOLDENS) and len(set(g.GOLDENS) - GOLDENS_WITHOUT_BRACKET) >= 7


def test_user_sub_range_with_guard_regions():
    """user_begin = 5, 15 of 37 users (no multiple of the four waves of a workgroup), all three outputs: the rows of the
    whole launch bit for bit, sentinel-filled guard regions around every output untouched, a count of zero is empty"""
    import torch
    n, K, m = 37, 3, 2
    rays, p = g._small(n, K=K)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    kw = dict(gamma=True, rate=True, per_subcarrier=True)
    full = eng.spectrum(prep, 17.0, **kw)
    assert tuple(full[0].shape) == (n, K, m)
    guard, sentinel = 1 << 16, -12345.5
    sizes = (n * K * m, n, n * K)
    bigs = [torch.full((guard + s + guard,), sentinel, dtype=torch.float32, device="cuda") for s in sizes]
    outs = [bigs[0][guard:guard + sizes[0]].view(n, K, m), bigs[1][guard:guard + n], bigs[2][guard:guard + sizes[2]].view(n, K)]

    def guards_untouched():
        return all(bool((b[:guard] == sentinel).all()) and bool((b[guard + s:] == sentinel).all()) for b, s in zip(bigs, sizes))
    eng.spectrum(prep, 17.0, out=tuple(outs), **kw)
    torch.cuda.synchronize()
    assert guards_untouched(), "write outside the output tensors"
    assert all(torch.equal(o, f) for o, f in zip(outs, full))
    for b in bigs:
        b.fill_(sentinel)
    b0, cnt = 5, 15
    eng.spectrum(prep, 17.0, user_begin=b0, user_count=cnt, out=tuple(o[b0:b0 + cnt] for o in outs), **kw)
    torch.cuda.synchronize()
    assert guards_untouched()
    for o, f in zip(outs, full):
        assert bool((o[:b0] == sentinel).all()) and bool((o[b0 + cnt:] == sentinel).all()), "rows outside the range written"
        assert torch.equal(o[b0:b0 + cnt], f[b0:b0 + cnt])
    assert torch.equal(eng.spectrum(prep, 17.0, user_begin=b0, user_count=cnt), full[0][b0:b0 + cnt])
    empty = eng.spectrum(prep, 17.0, user_begin=n, user_count=0, **kw)
    assert [tuple(t.shape) for t in empty] == [(0, K, m), (0,), (0, K)]


def test_largest_shape_runs_and_the_next_one_is_refused():
    """796 x 1 BS at 25 paths and one subcarrier is the last shape taken (tests/test_gpu_rate.py has the arithmetic), 797
    the first refused: NativeError from the engine, ValueError from the Dataset."""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    n, L = 3, 25
    rays = onp.synth_rays(n, L, seed=77, all_valid=True)
    c = _case("largest", n, L, [796, 1], [1, 1], 512, [9])
    eng = _engine()
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, _dm_params(c).validate(n), want_side="light", carrier_freq=28e9)
    assert eng.spectrum_supported(prep)
    H = _oracle(c, rays, np.zeros(3))["channel"]
    snr_db = 10 * np.log10(case_snr(H))
    ga, r, rk = eng.spectrum(prep, snr_db, rate=True, per_subcarrier=True)
    torch.cuda.synchronize()
    check_spectrum(ga, r, rk, H, 10.0 ** (snr_db / 10.0), "largest")
    c2 = dict(c, bs_shape=[797, 1])
    prep2 = eng.prepare(dr, _dm_params(c2).validate(n), want_side="light", carrier_freq=28e9)
    assert not eng.spectrum_supported(prep2)
    with pytest.raises(NativeError, match=r"status -2.*LDS"):
        eng.spectrum(prep2, snr_db)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    with pytest.raises(ValueError, match="LDS"):
        ds.compute_eigenmodes(_dm_params(c2), snr_db=snr_db)
    with pytest.raises(ValueError, match="LDS"):
        ds.compute_rate(_dm_params(c2), snr_db=snr_db, power_allocation="waterfilling")
    assert ds.compute_eigenmodes(_dm_params(c), snr_db=snr_db).shape == (n, 1, 1)


def test_public_api_numpy_and_torch_returns_and_the_definition():
    import torch
    import deepmimo_amd as dm
    n = 90
    rays, p = g._small(n, 25, (8, 1), (2, 1), 4, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    H = ds.compute_channels(p)
    snr_db = float(10 * np.log10(case_snr(H)))
    bits = lambda a: (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)      # noqa: E731
    plain = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True)
    equal = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True, power_allocation="equal")
    assert np.array_equal(bits(plain[0]), bits(equal[0])) and np.array_equal(bits(plain[1]), bits(equal[1]))
    assert np.array_equal(bits(ds.compute_rate(p, snr_db=snr_db)), bits(ds.compute_rate(p, snr_db=snr_db, power_allocation="equal")))
    g_np = ds.compute_eigenmodes(p, snr_db=snr_db)
    r_np = ds.compute_rate(p, snr_db=snr_db, power_allocation="waterfilling")
    pair = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True, power_allocation="waterfilling")
    dm.config("channel_output", "torch")
    try:
        g_t = ds.compute_eigenmodes(p, snr_db=snr_db)
        r_t = ds.compute_rate(p, snr_db=snr_db, power_allocation="waterfilling")
        pair_t = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True, power_allocation="waterfilling")
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(g_np, np.ndarray) and g_np.dtype == np.float32 and g_np.shape == (n, 4, 2)
    assert isinstance(r_np, np.ndarray) and r_np.dtype == np.float32 and r_np.shape == (n,)
    assert isinstance(g_t, torch.Tensor) and g_t.is_cuda and g_t.dtype == torch.float32
    assert isinstance(r_t, torch.Tensor) and r_t.is_cuda and isinstance(pair, tuple) and isinstance(pair_t, tuple)
    assert np.array_equal(bits(g_np), bits(g_t)) and np.array_equal(bits(r_np), bits(r_t))
    assert np.array_equal(bits(pair[0]), bits(r_np)) and pair[1].shape == (n, 4)
    assert np.array_equal(bits(pair_t[0]), bits(r_np)) and np.array_equal(bits(pair_t[1]), bits(pair[1]))
    # and the definition, from the channel tensor of the same dataset
    snr = 10.0 ** (snr_db / 10.0)
    check_spectrum(torch.from_numpy(g_np), torch.from_numpy(pair[0]), torch.from_numpy(pair[1]), H, snr, "public api",
                   equal_rate_k=torch.from_numpy(plain[1]))
    assert (g_np[ds.num_paths == 0] == 0).all() and (r_np[ds.num_paths == 0] == 0).all()


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 1])
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    assert {"compute_eigenmodes", "compute_rate"} <= dm.MacroDataset.PROPAGATE_METHODS
    modes = macro.compute_eigenmodes(p, snr_db=95.0)
    rates = macro.compute_rate(p, snr_db=95.0, power_allocation="waterfilling")
    assert isinstance(modes, list) and len(modes) == 2 and isinstance(rates, list) and len(rates) == 2
    for r, gm, gr in zip((a, b), modes, rates):
        ds = dm.Dataset({k: v.copy() for k, v in r.items()})
        am, ar = ds.compute_eigenmodes(p, snr_db=95.0), ds.compute_rate(p, snr_db=95.0, power_allocation="waterfilling")
        assert gm.shape == am.shape == (len(r["power"]), 6, 2) and np.array_equal(gm.view(np.int32), am.view(np.int32))
        assert gr.shape == ar.shape and np.array_equal(gr.view(np.int32), ar.view(np.int32))


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol of the modes and the worst position of rate_k inside its bracket (1 = at the
    edge) over every case that ran (DESIGN.md quotes both); nothing ran = nothing to report."""
    if WORST:
        kg = max(WORST, key=lambda i: WORST[i][0])
        kr = max(WORST, key=lambda i: WORST[i][1])
        print(f"spectrum: modes worst err / tol over {len(WORST)} cases = {WORST[kg][0]:.3f} ({kg}); "
              f"rate worst excess / bracket = {WORST[kr][1]:.3f} ({kr})")
        assert WORST[kg][0] <= 1.0 and WORST[kr][1] <= 1.0
