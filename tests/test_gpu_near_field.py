"""Near-field channels (DMX_FLAG_NEAR_FIELD, `Dataset.near_field`) on the GPU: every channel case of
tests/_near_field_cases.py against the complex128 reference of tests/_near_field_ref.py at its derived per-user tolerance, and
what has to hold bit for bit: a 1 x 1 / 1 x 1 link is the far-field vector kernel, a user sub-range equals the rows of the
whole launch, launches repeat, the call runs on a side stream and inside a captured graph, host rays equal HBM rays, NumPy
output equals torch output, `iter_channels` chunks equal `compute_channels`, and the view commutes with `at_times`.  The
geometry check of tests/test_near_field_cpu.py runs on the GPU result.  The closing test prints the worst error / tolerance
per case (pytest -s)."""
import numpy as np
import pytest

from tests import _entry_calls as E
from tests import _near_field_cases as NC
from tests import _near_field_ref as NF
from tests._cases import TOL_REL
from tests.test_gpu_stream_order import Delay, _behind_delay

pytestmark = pytest.mark.gpu

_REPORT = {}


@pytest.fixture(scope="module")
def eng():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _compute(case, variant=0, near=True, **dataset_kw):
    """`compute_channels` of a case on its near-field view (or, `near=False`, on the dataset itself) under
    `config('fd_kernel_variant', variant)`"""
    import deepmimo_amd as dm
    dm.config("fd_kernel_variant", variant)
    try:
        ds = NC.dataset(case, **dataset_kw)
        view = ds.near_field(NC.CARRIER) if near else ds
        return view.compute_channels(NC.dm_params(case)), view
    finally:
        dm.config("fd_kernel_variant", 0)


def _check(H, case, what):
    nf, _, tol = NC.references(case)
    ratio = NF.assert_within(H, nf, tol, what)
    _REPORT[what] = ratio
    print(f"near-field parity {what}: worst error {ratio:.3f} of the tolerance")
    return ratio


# ---- every case against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in NC.CHANNEL_CASES])
def test_case_meets_the_reference(cid):
    case = NC.BY_ID[cid]
    nf, ff, tol = NC.references(case)
    H, view = _compute(case)
    assert H.dtype == np.complex64 and np.all(H[2] == 0)                  # the user without paths
    _check(H, case, cid)
    if cid == "rotation_fov_patterns_doppler":
        from tests._pattern_ref import patched_oracle
        with patched_oracle() as onp:
            prep = onp.prepare_paths(NC.case_rays(case), NC.oracle_params(case), *NC.fovs(case))
        np.testing.assert_array_equal(view.los, prep["los"])
        np.testing.assert_array_equal(view.num_paths, prep["num_paths"])
    # the case is one the plane-wave kernels get wrong: the curvature is in the output
    d = np.abs(H - ff).reshape(len(H), -1).max(axis=1)
    assert np.max(d[tol > 0] / tol[tol > 0]) > 100


@pytest.mark.parametrize("cid", ["one_wave_4x2", "ula33_2x2_k70_kept7", "upa8x4_3x1_loaded40"])
def test_variant_1_is_variant_0(cid):
    case = NC.BY_ID[cid]
    np.testing.assert_array_equal(_compute(case, 0)[0], _compute(case, 1)[0])


@pytest.mark.parametrize("cid", ["ula16_k64", "upa8x4_3x1_k5_far_indices", "upa8x4_3x1_loaded40", "rotation_fov_patterns_doppler"])
def test_single_antenna_link_is_the_far_field_vector_kernel(cid):
    """psi = 0 at element 0 of both arrays: a 1 x 1 / 1 x 1 link has the bits of the far-field vector kernel (variant 1)"""
    import deepmimo_amd as dm
    case = NC.single_antenna(NC.BY_ID[cid])
    near, _ = _compute(case, 0)
    ds = NC.dataset(case)
    ds["rt_params"] = {"frequency": NC.CARRIER}                            # the carrier of the Doppler term, as in the view
    dm.config("fd_kernel_variant", 1)
    try:
        far = ds.compute_channels(NC.dm_params(case))
    finally:
        dm.config("fd_kernel_variant", 0)
    assert np.any(far != 0)
    np.testing.assert_array_equal(near, far)


def test_adaptive_precision_composes():
    import deepmimo_amd as dm
    case = NC.BY_ID["ula16_2x2_holes"]
    dm.config("adaptive_precision", True)
    try:
        H, _ = _compute(case)
    finally:
        dm.config("adaptive_precision", False)
    _check(H, case, "ula16_2x2_holes adaptive_precision")


# ---- the geometry check of the CPU file on the GPU result ------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [[33, 1], [5, 3]])
@pytest.mark.parametrize("apertures", [2, 10, 1000])
def test_gpu_result_is_the_distance_to_each_element(bs, apertures):
    import deepmimo_amd as dm
    from tests.test_near_field_cpu import los_geometry

    def channels(rays, op, fc):
        ds = dm.Dataset(dict({k: v.copy() for k, v in rays.items()}, rx_pos=np.zeros((1, 3), np.float32), tx_pos=np.zeros((1, 3), np.float32)))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape, p.bs_antenna.spacing = np.array(bs), np.array([1, 1]), op["bs_antenna"]["spacing"]
        p.num_paths, p.ofdm.subcarriers, p.ofdm.bandwidth = 1, op["ofdm"]["subcarriers"], op["ofdm"]["bandwidth"]
        p.ofdm.selected_subcarriers, p.ofdm.rx_filter, p.freq_domain = np.asarray(op["ofdm"]["selected_subcarriers"]), 0, 1
        H = ds.near_field(fc).compute_channels(p)
        ref = NF.near_field_channels(rays, op, fc)
        tol = NF.near_field_tolerance(ref, rays, op, fc)
        _REPORT[f"los {bs} at {apertures} apertures"] = NF.assert_within(H, ref, tol, f"los {bs} {apertures}")
        return H.astype(np.complex128), ref, tol

    (H, ref, tol), want = los_geometry(bs, apertures, channels)
    amp = np.abs(ref[0, 0, 0, 0])
    # H[t] / H[0] against the distances: the error of a quotient of two values each within tol of a value of modulus amp
    assert np.abs(H[0, 0, :, :] / H[0, 0, 0, :] - want[:, None]).max() <= 2 * tol[0] / (amp - tol[0]) + 1e-9


# ---- what a launch keeps -----------------------------------------------------------------------------------------------------------
def _prepared(eng, case, which="a"):
    rays = eng.upload_rays({k: v.copy() for k, v in NC.case_rays(case, which).items()})
    prep = eng.prepare(rays, NC.dm_params(case).validate(case["n"]), *NC.fovs(case), carrier_freq=NC.CARRIER,
                       want_side="light", near_field=True)
    return rays, prep


@pytest.mark.parametrize("cid", ["one_wave_4x2", "ula33_2x2_k70_kept7", "upa8x4_3x1_loaded40"])
def test_sub_range_and_repeat(cid, eng):
    import torch
    case = NC.BY_ID[cid]
    _, prep = _prepared(eng, case)
    whole = eng.channels(prep).clone()
    again = eng.channels(prep)
    torch.cuda.synchronize()
    assert E.same_bits(whole, again)
    nf, _, tol = NC.references(case)
    NF.assert_within(whole.cpu().numpy(), nf, tol, f"{cid} engine")
    for begin, count in ((0, 2), (1, 3), (3, case["n"] - 3), (case["n"] - 1, 1)):
        part = eng.channels(prep, user_begin=begin, user_count=count)
        assert E.same_bits(part, whole[begin:begin + count]), (cid, begin, count)


@pytest.mark.parametrize("cid", ["one_wave_4x2", "ula16_2x2_kept32", "upa8x4_3x1_loaded40"])
def test_side_stream_and_captured_graph(cid, eng):
    """the stream contract of tests/test_gpu_stream_order.py and the capture of tests/test_gpu_graph_capture.py for the
    near-field launch: stage 1 + stage 2 of a near-field preparation (`relaunch`) behind a device-side delay on a side stream,
    then captured and replayed on the rays of the capture and on new rays in the same tensors"""
    import torch
    case = NC.BY_ID[cid]
    want = {}
    for which in ("a", "b"):
        _, p = _prepared(eng, case, which)
        want[which] = eng.channels(p).clone()
    assert not E.same_bits(want["a"], want["b"])
    rays, prep = _prepared(eng, case, "a")
    b_dev = eng.upload_rays({k: v.copy() for k, v in NC.case_rays(case, "b").items()})
    out = torch.empty(eng.channel_shape(prep), dtype=torch.complex64, device=eng.device)
    side, delay = torch.cuda.Stream(), Delay(eng.device)
    with torch.cuda.stream(side):
        delay.run(2)
        eng.relaunch(prep, out)
    side.synchronize()
    assert E.same_bits(out, want["a"])

    def enqueue():
        E.copy_rays(rays, b_dev)
        return eng.relaunch(prep, out)

    res, ran_ahead, delay_ms, enqueue_ms = _behind_delay(side, delay, enqueue)
    assert ran_ahead, f"{cid}: delay too short (delay {delay_ms:.2f} ms, enqueue {enqueue_ms:.3f} ms), or the call synchronised"
    assert E.same_bits(res, want["b"]), f"{cid}: on a side stream behind the delay"

    a_dev = eng.upload_rays({k: v.copy() for k, v in NC.case_rays(case, "a").items()})
    E.copy_rays(rays, a_dev)
    eng.relaunch(prep, out)                                               # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.relaunch(prep, out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert E.same_bits(out, want["a"]), f"{cid}: replay on the rays of the capture"
    E.copy_rays(rays, b_dev)
    graph.replay()
    torch.cuda.synchronize()
    assert E.same_bits(out, want["b"]), f"{cid}: replay on new rays in the same tensors"


# ---- the view, whichever way it is asked ---------------------------------------------------------------------------------------------
def test_dataset_routes_agree(eng):
    import deepmimo_amd as dm
    case = NC.FULL_CASE
    p = NC.dm_params(case)
    H, _ = _compute(case)
    _check(H, case, "dataset host rays")
    # rays in HBM
    H_hbm, _ = _compute(case, device=eng.device)
    np.testing.assert_array_equal(H_hbm, H)
    # torch output
    dm.config("channel_output", "torch")
    try:
        Ht = NC.dataset(case).near_field(NC.CARRIER).compute_channels(p)
    finally:
        dm.config("channel_output", "numpy")
    assert Ht.is_cuda and np.array_equal(Ht.cpu().numpy(), H)
    # user chunks
    chunks = list(NC.dataset(case).near_field(NC.CARRIER).iter_channels(p, 4))
    assert [b for b, _ in chunks] == [0, 4, 8]
    np.testing.assert_array_equal(np.concatenate([h for _, h in chunks]), H)
    # the carrier of rt_params is the default
    ds = NC.dataset(case)
    ds["rt_params"] = {"frequency": NC.CARRIER}
    np.testing.assert_array_equal(ds.near_field().compute_channels(p), H)
    # a subset of the view is a view
    np.testing.assert_array_equal(NC.dataset(case).near_field(NC.CARRIER).subset(np.array([1, 3, 8])).compute_channels(
        _subset_params(case, [1, 3, 8])), H[[1, 3, 8]])
    # a MacroDataset fans the view out
    both = dm.MacroDataset([NC.dataset(case), NC.dataset(case)]).near_field(NC.CARRIER).compute_channels(p)
    assert len(both) == 2 and all(np.array_equal(h, H) for h in both)
    # without the view the same dataset gives the far-field channel
    far, _ = _compute(case, near=False)
    assert not np.array_equal(far, H)


def _subset_params(case, idxs):
    p = NC.dm_params(case)
    rot = np.asarray(p.ue_antenna.rotation)
    if rot.ndim == 2:
        p.ue_antenna.rotation = rot[idxs]
    return p


def test_the_view_commutes_with_at_times():
    case = NC.FULL_CASE
    p, times = NC.dm_params(case), [0.0, 1e-3]
    H, _ = _compute(case)
    ds = NC.dataset(case)
    ds.set_channel_params(NC.dm_params(case))
    a = ds.near_field(NC.CARRIER).at_times(times, carrier_freq=NC.CARRIER)
    b = ds.at_times(times, carrier_freq=NC.CARRIER).near_field(NC.CARRIER)
    Ha, Hb = a.compute_channels(), b.compute_channels()
    np.testing.assert_array_equal(Ha, Hb)
    np.testing.assert_array_equal(a.split_times(Ha)[0], H)                  # t = 0 keeps the stored phases bit for bit
    assert not np.array_equal(a.split_times(Ha)[1], H)
    series = NC.dataset(case).near_field(NC.CARRIER).compute_channels(p, times=times, carrier_freq=NC.CARRIER)
    np.testing.assert_array_equal(series, a.split_times(Ha))


def test_report():
    """worst error / tolerance of every comparison above (run the file as a whole)"""
    assert _REPORT, "run the whole file"
    worst = max(_REPORT, key=_REPORT.get)
    for what, ratio in sorted(_REPORT.items(), key=lambda kv: -kv[1])[:10]:
        print(f"near-field report: {ratio:.3f} of the tolerance  {what}")
    print(f"near-field report: worst error / tolerance = {_REPORT[worst]:.3f} ({worst}), {len(_REPORT)} comparisons")
    assert _REPORT[worst] <= 1.0 and TOL_REL == 5e-5
