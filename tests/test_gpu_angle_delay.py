"""Angle-delay representation (dmx_channels_angle_delay, k9_angle_delay.hip) on the GPU.

Reference: the definition - codebook product and np.fft.ifft in complex128 of the NumPy oracle's channel tensor
(tests/_angle_delay_ref.py `adp_from_channel`; tests/test_angle_delay_cpu.py holds the closed form to it).  Criterion per
user: max |X - X_ref[u]| <= TOL_REL max |X_ref[u]|, the project's per-user-peak criterion (tests/_cases.py) applied to this
output; tests/test_angle_delay_cpu.py shows for every case below that the fp32 summation error the user's amplification
admits is at most half of it, and on the equal-power case that a wrong path moves the reference by twice the bound.  Every
case also holds: exactly +0.0 where the reference user is all zero, everything finite, dtype / shape / contiguity, and a
second launch is torch.equal.  The case table and its inputs: tests/_angle_delay_cases.py.
"""
import os

import numpy as np
import pytest

from tests._angle_delay_cases import BY_ID, CASES, case_codebook, case_inputs, case_rays, lds_rule
from tests._angle_delay_ref import adp_from_channel
from tests._cases import TOL_REL, assert_channel_close

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_fd_direct import _dm_params, _kwargs, _oracle, _rays  # noqa: E402

WORST = {}                                   # case id -> worst error / bound, printed by the last test


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _launch(eng, c, **kw):
    """(prep, X) of a case: stage 1 and the fused call"""
    rays, ue_rot, F = case_inputs(c)[:3]
    p = _dm_params(c).validate(c["n"])
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot))
    return prep, eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=None if F is None else F.astype(np.complex64), **kw)


def check_adp(X, X_ref, what, again=None):
    """The criterion and the structural properties of one launch against the reference X_ref"""
    import torch
    assert X.dtype == torch.complex64 and tuple(X.shape) == X_ref.shape and X.is_contiguous()
    x = X.cpu().numpy()
    n = X_ref.shape[0]
    assert np.isfinite(x.view(np.float32)).all(), f"{what}: NaN or inf"
    peak = np.abs(X_ref).reshape(n, -1).max(axis=1)
    dead = peak == 0
    xd = x[dead].view(np.float32)
    assert (xd == 0).all() and not np.signbit(xd).any(), f"{what}: a user without paths is not +0.0"
    err = np.abs(x.astype(np.complex128) - X_ref).reshape(n, -1).max(axis=1)
    ratio = float((err[~dead] / (TOL_REL * peak[~dead])).max()) if (~dead).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.3f} over {int((~dead).sum())} live users")
    WORST[what] = ratio
    assert (err <= TOL_REL * peak).all(), f"{what}: {(err > TOL_REL * peak).sum()} users out of the bound, worst error / bound {ratio:.3f}"
    if again is not None:
        assert torch.equal(torch.view_as_real(again), torch.view_as_real(X)), f"{what}: a second launch differs"
    return ratio


def test_shared_inputs_are_those_of_the_tests_they_name():
    """tests/_angle_delay_cases.py restates the ray builders (it has to import without the library): the same arrays"""
    from tests.test_gpu_rate import CASES as RATE_CASES, _case_rays
    c = BY_ID["counts_and_holes_dft"]
    theirs = _case_rays(next(r for r in RATE_CASES if r["id"] == "counts_and_holes"))
    ours = case_rays(c)
    assert all(np.array_equal(ours[k], theirs[k], equal_nan=True) for k in theirs)
    c = BY_ID["doppler"]
    theirs, ours = _rays(c), case_rays(c)
    assert set(ours) == set(theirs) and all(np.array_equal(ours[k], theirs[k], equal_nan=True) for k in theirs)
    for cid in ("rot_fov_dipole", "per_user_rot", "doppler"):                # the stage-1 parameters of test_gpu_rate.py
        r = next(r for r in RATE_CASES if r["id"] == cid)
        for k in ("bs_rot", "ue_rot", "bs_fov", "ue_fov", "bs_pattern", "ue_pattern", "per_user_rot", "doppler", "bs_shape", "ue_shape"):
            assert BY_ID[cid][k] == r[k], (cid, k)
    c = BY_ID["per_user_rot"]
    X_ref = case_inputs(c)[3]
    H = _oracle(c, case_rays(c), case_inputs(c)[1])["channel"]
    assert np.array_equal(adp_from_channel(H, case_codebook(c), c["n_fft"], c["n_taps"]), X_ref)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_angle_delay_against_the_definition(c):
    import torch
    eng = _engine()
    X_ref = case_inputs(c)[3]
    prep, first = _launch(eng, c)
    F = case_inputs(c)[2]
    rows = c["bs_shape"][0] * c["bs_shape"][1] if F is None else len(F)
    assert eng.angle_delay_supported(prep, rows, c["n_fft"], c["n_taps"])
    second = eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=None if F is None else F.astype(np.complex64))
    torch.cuda.synchronize()
    if c["rays"] == "counts":
        assert (np.abs(X_ref).reshape(c["n"], -1).max(axis=1) == 0).sum() >= c["n"] // 5       # the users without a path
    check_adp(first, X_ref, c["id"], again=second)


def test_identity_codebook_and_antenna_rows_agree_within_the_bound_of_each():
    """not bit-equal: the identity goes through the projection kernel, antenna rows are computed in the wave"""
    import torch
    eng = _engine()
    a, b = BY_ID["identity_4x2"], BY_ID["identity_4x2_ant"]
    Xa, Xb = _launch(eng, a)[1], _launch(eng, b)[1]
    torch.cuda.synchronize()
    X_ref = case_inputs(a)[3]
    assert np.array_equal(X_ref, case_inputs(b)[3])
    peak = np.abs(X_ref).reshape(a["n"], -1).max(axis=1)
    diff = np.abs(Xa.cpu().numpy().astype(np.complex128) - Xb.cpu().numpy()).reshape(a["n"], -1).max(axis=1)
    assert (diff <= 2 * TOL_REL * peak).all()


def test_user_sub_range_with_guard_regions():
    """user_begin > 0 with a count that is no multiple of the four waves of a workgroup: the rows of the whole launch bit for
    bit, and sentinel-filled guard regions before and after the output stay untouched; with and without a codebook"""
    import torch
    eng = _engine()
    for cid in ("s0_minus5_dft", "s0_minus5_ant"):
        c = BY_ID[cid]
        F = case_inputs(c)[2]
        cb = None if F is None else F.astype(np.complex64)
        prep, full = _launch(eng, c)
        n, per = c["n"], int(np.prod(full.shape[1:]))
        assert lds_rule(c["ue_shape"], full.shape[2], c["n_taps"], 25) == 4
        guard, sentinel = 1 << 16, complex(-12345.5, 777.25)
        big = torch.full((guard + n * per + guard,), sentinel, dtype=torch.complex64, device="cuda")
        out = big[guard:guard + n * per].view(full.shape)

        def guards_untouched():
            return bool((big[:guard] == sentinel).all()) and bool((big[guard + n * per:] == sentinel).all())
        eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=cb, out=out)
        torch.cuda.synchronize()
        assert guards_untouched(), "write outside the output tensor"
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(full))
        big.fill_(sentinel)
        b, cnt = 5, 15
        eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=cb, user_begin=b, user_count=cnt, out=out[b:b + cnt])
        torch.cuda.synchronize()
        assert guards_untouched()
        assert bool((out[:b] == sentinel).all()) and bool((out[b + cnt:] == sentinel).all()), "rows outside the range written"
        assert torch.equal(torch.view_as_real(out[b:b + cnt]), torch.view_as_real(full[b:b + cnt]))
        empty = eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=cb, user_begin=n, user_count=0)
        assert tuple(empty.shape) == (0,) + tuple(full.shape[1:])


def test_largest_tables_run_and_what_lies_beyond_is_refused():
    """The LDS rule (M_rx + min(R, 32) + tc) * P * 8 is bounded by the limits on M_rx and P: its largest tables, 8 UE elements,
    32 rows and 64 taps per chunk at 32 paths (26624 bytes, two waves per workgroup), run and meet the criterion on a shape
    with several row and tap chunks; a ninth UE element or a 33rd path is refused - DMX_ERR_SHAPE from the engine,
    ValueError from the Dataset.  No shape within those limits reaches the 159744 bytes of one wave, so no launch needs the
    raised dynamic-LDS limit and none is refused with an LDS message."""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    from tests.test_gpu_fd_direct import _case
    n, L = 5, 32
    c = dict(_case("largest", n, L, [8, 5], [4, 2], 512, range(96)), n_fft=128, n_taps=70, all_valid=True)
    assert lds_rule(c["ue_shape"], 40, c["n_taps"], L) == 2 and (8 + 32 + 64) * 32 * 8 == 26624
    rays = onp.synth_rays(n, L, seed=77, all_valid=True)
    eng = _engine()
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, _dm_params(c).validate(n), want_side="light", carrier_freq=28e9)
    assert eng.angle_delay_supported(prep, 40, 128, 70)
    X = eng.angle_delay(prep, 70, n_fft=128, tx_codebook=dm.dft_codebook([8, 5]))
    torch.cuda.synchronize()
    H = _oracle(c, rays, np.zeros(3))["channel"]
    check_adp(X, adp_from_channel(H, dm.dft_codebook([8, 5]), 128, 70), "largest")
    c9 = dict(c, ue_shape=[3, 3])
    prep9 = eng.prepare(dr, _dm_params(c9).validate(n), want_side="light", carrier_freq=28e9)
    assert not eng.angle_delay_supported(prep9, 40, 128, 70)
    with pytest.raises(NativeError, match=r"status -2.*8 UE elements"):
        eng.angle_delay(prep9, 70, n_fft=128)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    with pytest.raises(ValueError, match="8 UE elements"):
        ds.compute_angle_delay(_dm_params(c9), n_taps=70, n_fft=128)
    rays40 = onp.synth_rays(n, 40, seed=78, all_valid=True)
    c33 = dict(c, L=40, num_paths=33)
    prep33 = eng.prepare(eng.upload_rays(rays40), _dm_params(c33).validate(n), want_side="light", carrier_freq=28e9)
    with pytest.raises(NativeError, match=r"status -2.*1\.\.32 paths"):
        eng.angle_delay(prep33, 70, n_fft=128)
    assert ds.compute_angle_delay(_dm_params(c), n_taps=70, n_fft=128).shape == (n, 8, 40, 70)


def _small(n=37, L=11, bs=(4, 2), ue=(2, 1), K=64, seed=403):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=seed)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.num_paths = L
    p.ofdm.selected_subcarriers = np.arange(3, 3 + K)
    p.validate(n)
    return rays, p


def test_public_api_numpy_and_torch_returns_are_the_same_bits():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 64, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    x_np = ds.compute_angle_delay(p, n_taps=32)
    x_cb = ds.compute_angle_delay(p, n_taps=32, codebook=dm.dft_codebook([8, 1]))
    x_ant = ds.compute_angle_delay(p, n_taps=16, n_fft=128, codebook=None)
    dm.config("channel_output", "torch")
    try:
        x_t = ds.compute_angle_delay(p, n_taps=32)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(x_np, np.ndarray) and x_np.dtype == np.complex64 and x_np.shape == (90, 2, 8, 32)
    assert isinstance(x_t, torch.Tensor) and x_t.is_cuda and x_t.dtype == torch.complex64
    assert np.array_equal(x_np.view(np.int32), x_t.cpu().numpy().view(np.int32))
    assert np.array_equal(x_np.view(np.int32), x_cb.view(np.int32))         # "dft" is dm.dft_codebook of the BS panel
    assert x_ant.shape == (90, 2, 8, 16)
    dead = ds.num_paths == 0                                                 # the field of view leaves some users no path
    assert (x_np[dead] == 0).all() and (np.abs(x_np[~dead]).reshape((~dead).sum(), -1).max(axis=1) > 0).all()


def test_full_grid_antenna_domain_transforms_back_to_the_channel():
    """codebook=None and n_taps = n_fft = K: np.fft.fft over the taps reproduces compute_channels within the channel criterion"""
    import deepmimo_amd as dm
    rays, p = _small(41, 25, (4, 2), (2, 1), 64, seed=9)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    X = ds.compute_angle_delay(p, n_taps=64, codebook=None)
    H = ds.compute_channels(p)
    assert_channel_close(np.fft.fft(X.astype(np.complex128), axis=-1), H, what="fft of the delay domain")


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(0, 512, 4)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    both = macro.compute_angle_delay(p, n_taps=24)
    assert isinstance(both, list) and len(both) == 2
    for r, got in zip((a, b), both):
        alone = dm.Dataset({k: v.copy() for k, v in r.items()}).compute_angle_delay(p, n_taps=24)
        assert got.shape == alone.shape == (len(r["power"]), 1, 8, 24) and np.array_equal(got.view(np.int32), alone.view(np.int32))


def test_zz_report_worst_ratio():
    """Last in the file: the worst error / bound over every case that ran (DESIGN.md quotes it); nothing ran = nothing to
    report."""
    if WORST:
        k = max(WORST, key=lambda i: WORST[i])
        print(f"angle-delay: worst error / bound over {len(WORST)} cases = {WORST[k]:.3f} ({k})")
        assert WORST[k] <= 1.0
