"""Per-user achievable rate (dmx_channel_rate, k7_rate.hip) on the GPU.

Reference: the definition, slogdet in complex128 of the NumPy oracle's channel tensor (tests/_rate_ref.py;
tests/test_rate_cpu.py pins it against hand cases).  Criterion per entry: |rate_k - ref| <= tol_k and |rate - ref| <= tol[u]
with the derived tolerance of tests/_rate_ref.py (the first-order change of the rate under a channel error the project's
channel criterion admits, plus the fp32 rounding of the logarithms).  The SNR of a case comes from its reference alone: the
median live user sits at 20 dB.  Every case also holds: exactly +0.0 where the reference channel is all zero, every value
finite and >= 0, |rate - float64 mean(rate_k)| <= K 2^-24 max_k rate_k + 2^-24, and a second launch is torch.equal.
Waves per workgroup of a shape come from the LDS rule restated in tests/test_rate_cpu.py.
"""
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests._cases import golden_names, load_golden
from tests._rate_ref import median_snr, rate_from_channel, rate_tolerance
from tests.test_rate_cpu import LDS_MAX, rate_lds_rule

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle, _rays, _ue_rot  # noqa: E402

WORST = {}                                   # case id -> (worst err / tol, worst |err| in bit), printed by the last test
IRREGULAR = [-3, 0, 5, 511, 512, 700, -1000, 77, 2 ** 31 - 1, -(2 ** 31), 40001]


def live_counts(n, L):
    """live paths per user, cycled: 0, 1, 2, L - 1, L"""
    return [min(L, (0, 1, 2, L - 1, L)[u % 5]) for u in range(n)]


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _cases():
    cs = []
    cs.append(_case("defaults", 70, 25, [8, 1], [1, 1], 512, [0]))                     # DeepMIMO's defaults, K = 1
    # chunk edges: one below, at and above the 64 subcarriers of a chunk, and the full selection
    cs.append(_case("K63", 40, 25, [8, 1], [1, 1], 512, range(3, 66)))
    cs.append(_case("K64", 40, 25, [8, 1], [1, 1], 512, range(3, 67)))
    cs.append(_case("K65", 40, 25, [8, 1], [1, 1], 512, range(3, 68)))
    cs.append(_case("K512", 40, 25, [8, 1], [1, 1], 512, range(512)))
    cs.append(_case("irregular", 33, 25, [4, 2], [2, 1], 512, IRREGULAR))
    cs.append(_case("panel", 23, 25, [8, 8], [2, 2], 512, range(0, 512, 7)))
    cs.append(_case("ue_larger", 29, 25, [2, 1], [4, 4], 512, [0, 9, 100, 300, 511]))  # the Gram runs over the BS side
    cs.append(_case("m8", 21, 25, [8, 4], [4, 2], 512, [0, 17, 100]))
    # one loaded path: every live user is rank 1, where the rate of a 2-element UE is ill-conditioned in the channel error
    # above 20 dB (the tolerance says so), so the single-antenna UE keeps the check sharp
    cs.append(_case("L1", 50, 1, [4, 2], [1, 1], 64, [0, 9, 63]))
    cs.append(_case("P32_num_paths_below_loaded", 19, 40, [4, 2], [2, 1], 256, [0, 17, 100], num_paths=32, all_valid=True))
    cs.append(_case("P32_num_paths_above_loaded", 19, 32, [4, 2], [2, 1], 256, [0, 17, 100], num_paths=40, all_valid=True))
    cs.append(_case("counts_and_holes", 45, 25, [4, 2], [2, 1], 512, [0, 3, 200], rays="counts"))
    # launch residue: 4k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 1-wave shape
    for n in (41, 42, 43):
        cs.append(_case(f"wpb4_users{n}", n, 25, [8, 1], [1, 1], 512, [0, 5]))
    cs.append(_case("wpb1_users7", 7, 25, [16, 16], [2, 2], 512, range(64)))
    # stage-1 features arrive through the records.  rot_fov_dipole: the covariance test's parameters but for a single-antenna
    # UE - the FoV leaves many users one path, and with the 2 x 1 UE 24 % of the entries had a tolerance above 1 % of the rate
    # (rank 1 far above the median SNR), more than the 5 % tests/test_rate_cpu.py admits
    cs.append(_case("rot_fov_dipole", 53, 25, [4, 2], [1, 1], 512, [0, 1, 2], bs_rot=[5, -20, 60], ue_rot=[10, 20, 30],
                    bs_fov=[150, 110], ue_fov=[200, 100], bs_pattern="halfwave-dipole", ue_pattern="halfwave-dipole"))
    cs.append(_case("per_user_rot", 45, 25, [8, 1], [2, 2], 512, [0, 7], per_user_rot=True))
    cs.append(_case("doppler", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], doppler=1))
    cs.append(_case("adaptive_workspace", 61, 25, [8, 4], [2, 1], 512, range(0, 64, 3), adaptive=True))
    for c in cs:
        c["selected"] = list(c["selected"])
        c.setdefault("adaptive", False)
    return cs


# and Gram orders 3, 5, 6, 7 in both orientations, odd arrays, every kept-path count (tests/_consumer_shapes.py)
CASES = _cases() + shapes.RATE_CASES + [shapes.EVERY_COUNT]
_INPUTS = {}


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


def case_inputs(c):
    """(rays, ue_rot, H of the oracle, snr) of a case: computed once, shared and left unchanged"""
    if c["id"] not in _INPUTS:
        rays, ue_rot = _case_rays(c), _ue_rot(c)
        H = _oracle(c, rays, ue_rot)["channel"]
        H.setflags(write=False)
        _INPUTS[c["id"]] = (rays, ue_rot, H, median_snr(H))
    return _INPUTS[c["id"]]


def test_waves_per_workgroup_of_the_listed_shapes():
    """the shapes above drive what their names say (the launcher's rule, restated on the host)"""
    by = {c["id"]: c for c in CASES}
    rule = lambda cid: rate_lds_rule(by[cid]["bs_shape"], by[cid]["ue_shape"], len(by[cid]["selected"]),   # noqa: E731
                                     min(by[cid]["num_paths"], by[cid]["L"]))
    assert rule("wpb4_users41") == 4 and rule("wpb4_users43") == 4 and rule("wpb1_users7") == 1
    assert rule("defaults") == 4 and rule("K512") == 4 and rule("panel") == 2
    assert rule("m5_ue_K1") == 4 and rule("m6_ue_K70") == 2 and rule("m7_ue_5x3_K70") == 2 and rule("every_count") == 4


def check_rate(rate, rate_k, H, snr, what, again=None):
    """The criterion and the structural properties of one launch against the reference channel H"""
    import torch
    n, K = H.shape[0], H.shape[3]
    assert rate.dtype == torch.float32 and tuple(rate.shape) == (n,) and rate.is_contiguous()
    assert rate_k.dtype == torch.float32 and tuple(rate_k.shape) == (n, K) and rate_k.is_contiguous()
    r, rk = rate.cpu().numpy(), rate_k.cpu().numpy()
    assert np.isfinite(r).all() and np.isfinite(rk).all() and (r >= 0).all() and (rk >= 0).all(), f"{what}: NaN, inf or negative"
    ref, ref_k = rate_from_channel(H, snr)
    tol, tol_k = rate_tolerance(H, snr)
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    assert (r[dead] == 0).all() and not np.signbit(r[dead]).any(), f"{what}: a user without paths is not +0.0"
    assert (rk[dead] == 0).all() and not np.signbit(rk[dead]).any(), f"{what}: rate_k of a user without paths is not +0.0"
    ek, e = np.abs(rk - ref_k), np.abs(r - ref)
    ratio = max(float((ek / tol_k).max()), float((e / tol).max())) if n else 0.0
    worst_abs = max(float(ek.max()), float(e.max())) if n else 0.0
    print(f"{what}: snr {10 * np.log10(snr):.1f} dB, worst err / tol = {ratio:.3f}, worst |err| = {worst_abs:.3e} bit, "
          f"largest rate {float(ref_k.max()):.2f}")
    WORST[what] = (ratio, worst_abs)
    assert (ek <= tol_k).all(), f"{what}: {(ek > tol_k).sum()} rate_k entries out of tolerance, worst err / tol {ratio:.3f}"
    assert (e <= tol).all(), f"{what}: {(e > tol).sum()} users out of tolerance, worst err / tol {ratio:.3f}"
    mean = rk.astype(np.float64).mean(axis=1)
    assert (np.abs(r - mean) <= K * 2.0 ** -24 * rk.max(axis=1) + 2.0 ** -24).all(), f"{what}: rate is not the mean of rate_k"
    if again is not None:
        assert torch.equal(again[0], rate) and torch.equal(again[1], rate_k), f"{what}: a second launch differs"
    return ratio


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_rate_against_the_definition(c):
    import torch
    eng = _engine()
    rays, ue_rot, H, snr = case_inputs(c)
    p = _dm_params(c).validate(c["n"])
    kw = _kwargs(c, ue_rot)
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **kw)
    assert eng.rate_supported(prep)
    snr_db = 10 * np.log10(snr)
    first = eng.rate(prep, snr_db, per_subcarrier=True)
    second = eng.rate(prep, snr_db, per_subcarrier=True)
    alone = eng.rate(prep, snr_db)                                          # without the optional output: the same bits
    torch.cuda.synchronize()
    if c["rays"] == "counts":
        assert (np.abs(H).reshape(c["n"], -1).max(axis=1) == 0).sum() >= c["n"] // 5      # the users without a path
    assert torch.equal(alone, first[0])
    check_rate(first[0], first[1], H, 10.0 ** (snr_db / 10.0), c["id"], again=second)


def _golden_ok(name):
    case, rays, _, ref = load_golden(name)
    return bool(case["freq_domain"]) and not case["rx_filter"] and "channel" in ref and \
        1 <= min(case["num_paths"], rays["power"].shape[1]) <= 32


GOLDENS = [g for g in golden_names() if _golden_ok(g)]


def test_some_goldens_store_their_channel():
    assert len(GOLDENS) >= 5, GOLDENS


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_rate_of_the_reference_channel(name):
    """the rate of the channel tensor the real reference wrote (Doppler off: `channel` is the tensor without it)"""
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
    H = ref["channel"]
    snr_db = 10 * np.log10(median_snr(H))
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", **kw)
    r, rk = eng.rate(prep, snr_db, per_subcarrier=True)
    torch.cuda.synchronize()
    check_rate(r, rk, H, 10.0 ** (snr_db / 10.0), name)


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


def test_user_sub_range_with_guard_regions():
    """user_begin > 0 with a count that is no multiple of the four waves of a workgroup, both outputs: the rows of the whole
    launch bit for bit, and sentinel-filled guard regions before and after the outputs stay untouched"""
    import torch
    n, K = 37, 3
    rays, p = _small(n, K=K)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    assert rate_lds_rule((4, 2), (2, 1), K, 11) == 4
    full, full_k = eng.rate(prep, 17.0, per_subcarrier=True)
    guard, sentinel = 1 << 16, -12345.5
    big = torch.full((guard + n + guard,), sentinel, dtype=torch.float32, device="cuda")
    big_k = torch.full((guard + n * K + guard,), sentinel, dtype=torch.float32, device="cuda")
    out, out_k = big[guard:guard + n], big_k[guard:guard + n * K].view(n, K)

    def guards_untouched():
        return bool((big[:guard] == sentinel).all()) and bool((big[guard + n:] == sentinel).all()) and \
            bool((big_k[:guard] == sentinel).all()) and bool((big_k[guard + n * K:] == sentinel).all())
    eng.rate(prep, 17.0, per_subcarrier=True, out=(out, out_k))
    torch.cuda.synchronize()
    assert guards_untouched(), "write outside the output tensors"
    assert torch.equal(out, full) and torch.equal(out_k, full_k)
    big.fill_(sentinel)
    big_k.fill_(sentinel)
    b, cnt = 5, 15
    eng.rate(prep, 17.0, user_begin=b, user_count=cnt, per_subcarrier=True, out=(out[b:b + cnt], out_k[b:b + cnt]))
    torch.cuda.synchronize()
    assert guards_untouched()
    assert bool((out[:b] == sentinel).all()) and bool((out[b + cnt:] == sentinel).all()), "rows outside the range written"
    assert bool((out_k[:b] == sentinel).all()) and bool((out_k[b + cnt:] == sentinel).all()), "rows outside the range written"
    assert torch.equal(out[b:b + cnt], full[b:b + cnt]) and torch.equal(out_k[b:b + cnt], full_k[b:b + cnt])
    assert torch.equal(eng.rate(prep, 17.0, user_begin=b, user_count=cnt), full[b:b + cnt])
    assert eng.rate(prep, 17.0, user_begin=n, user_count=0).shape == (0,)


def test_largest_shape_runs_and_the_next_one_is_refused():
    """25 paths, one subcarrier: m + M_big + 1 <= 798 (include/deepmimo_amd.h).  A 796-element BS array with one UE element
    is the last shape taken - one wave, 159600 bytes of LDS - and 797 elements the first refused: ValueError from the
    Dataset, DMX_ERR_SHAPE from the engine."""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    n, L = 3, 25
    assert (1 + 796 + 1) * 25 * 8 <= LDS_MAX < (1 + 797 + 1) * 25 * 8
    rays = onp.synth_rays(n, L, seed=77, all_valid=True)
    c = _case("largest", n, L, [796, 1], [1, 1], 512, [9])
    p = _dm_params(c).validate(n)
    eng = _engine()
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, p, want_side="light", carrier_freq=28e9)
    assert eng.rate_supported(prep)
    H = _oracle(c, rays, np.zeros(3))["channel"]
    snr_db = 10 * np.log10(median_snr(H))
    r, rk = eng.rate(prep, snr_db, per_subcarrier=True)
    torch.cuda.synchronize()
    check_rate(r, rk, H, 10.0 ** (snr_db / 10.0), "largest")
    c2 = dict(c, bs_shape=[797, 1])
    p2 = _dm_params(c2).validate(n)
    prep2 = eng.prepare(dr, p2, want_side="light", carrier_freq=28e9)
    assert not eng.rate_supported(prep2)
    with pytest.raises(NativeError, match=r"status -2.*LDS"):
        eng.rate(prep2, snr_db)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    with pytest.raises(ValueError, match="LDS"):
        ds.compute_rate(_dm_params(c2), snr_db=snr_db)
    assert ds.compute_rate(_dm_params(c), snr_db=snr_db).shape == (n,)


def test_rate_grows_with_the_snr():
    import torch
    c = next(c for c in CASES if c["id"] == "panel")
    eng = _engine()
    rays, ue_rot, H, snr = case_inputs(c)
    prep = eng.prepare(eng.upload_rays(rays), _dm_params(c).validate(c["n"]), want_side="light", **_kwargs(c, ue_rot))
    snr_db = 10 * np.log10(snr)
    lo, hi = eng.rate(prep, snr_db), eng.rate(prep, snr_db + 3)
    torch.cuda.synchronize()
    assert bool((hi >= lo).all()) and bool((hi > lo).any())


def test_public_api_numpy_and_torch_returns_are_the_same_bits():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 4, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    H = ds.compute_channels(p)
    snr_db = float(10 * np.log10(median_snr(H)))
    r_np = ds.compute_rate(p, snr_db=snr_db)
    pair = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True)
    dm.config("channel_output", "torch")
    try:
        r_t = ds.compute_rate(p, snr_db=snr_db)
        pair_t = ds.compute_rate(p, snr_db=snr_db, per_subcarrier=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(r_np, np.ndarray) and r_np.dtype == np.float32 and r_np.shape == (90,)
    assert isinstance(r_t, torch.Tensor) and r_t.is_cuda and r_t.dtype == torch.float32
    assert np.array_equal(r_np.view(np.int32), r_t.cpu().numpy().view(np.int32))
    assert isinstance(pair, tuple) and pair[0].shape == (90,) and pair[1].shape == (90, 4) and pair[1].dtype == np.float32
    assert np.array_equal(pair[0].view(np.int32), r_np.view(np.int32))
    assert isinstance(pair_t, tuple) and np.array_equal(pair_t[1].cpu().numpy().view(np.int32), pair[1].view(np.int32))
    # and the definition, from the channel tensor of the same dataset
    snr = 10.0 ** (snr_db / 10.0)
    ref, ref_k = rate_from_channel(H, snr)
    tol, tol_k = rate_tolerance(H, snr)
    assert (np.abs(r_np - ref) <= tol).all() and (np.abs(pair[1] - ref_k) <= tol_k).all()
    np.testing.assert_array_equal(ds.num_paths == 0, np.abs(H).reshape(90, -1).max(axis=1) == 0)
    assert (r_np[ds.num_paths == 0] == 0).all()


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    both = macro.compute_rate(p, snr_db=95.0)
    assert isinstance(both, list) and len(both) == 2
    for r, got in zip((a, b), both):
        alone = dm.Dataset({k: v.copy() for k, v in r.items()}).compute_rate(p, snr_db=95.0)
        assert got.shape == alone.shape and np.array_equal(got.view(np.int32), alone.view(np.int32))


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol and the worst absolute error over every case that ran (DESIGN.md quotes both);
    nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=lambda i: WORST[i][0])
        ka = max(WORST, key=lambda i: WORST[i][1])
        print(f"rate: worst err / tol over {len(WORST)} cases = {WORST[k][0]:.3f} ({k}); worst |err| = {WORST[ka][1]:.3e} bit ({ka})")
        assert WORST[k][0] <= 1.0
