"""Angle-delay power matrix and delay profile (DMX_FLAG_ANGLE_DELAY_POWER, DMX_FLAG_ANGLE_DELAY_PROFILE; k9_angle_delay.hip with
OUT = 1 and 2) on the GPU.

Reference: P_ref = sum_rx |X_ref|^2 and p_ref = sum_r P_ref in float64 of the complex128 definition X_ref of
tests/_angle_delay_ref.py, on every case of tests/_angle_delay_cases.py.  Criterion per entry: |P - P_ref| <= tol_P and
|p - p_ref| <= tol_p of tests/_angle_delay_power_ref.py - the project's per-user bound on X carried through
||X + d|^2 - |X|^2| <= 2 |X||d| + |d|^2 plus the float32 rounding of the sums; tests/test_angle_delay_power_cpu.py shows on the
oracle alone that a dropped path or an exchanged pair of delay rows moves both references by at least ten bounds.  Every
case also holds: exactly +0.0 for a user without a path, everything finite and >= 0, dtype / shape / contiguity, an untouched
guard region from the end of the smaller output to beyond the complex extent, a second launch torch.equal, and agreement with the complex call of the same
build at the rounding terms alone.

With the bits clear the complex output of every case hashes equal to tests/golden/angle_delay_complex_hashes.json, recorded
with a build of the parent commit (`DMX_LIB_PATH=<that build> python -m tests.test_gpu_angle_delay_power --record` writes it).

Worst error / bound over the 63 cases on an MI355X: see test_zz_report_worst_ratios (README.md quotes both).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import _angle_delay_power_ref as R
from tests._angle_delay_cases import BY_ID, CASES, case_inputs

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = os.path.join(_ROOT, "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_angle_delay import _launch  # noqa: E402

HASHES = os.path.join(_ROOT, "tests", "golden", "angle_delay_complex_hashes.json")
GUARD, SENTINEL = 4096, -12345.5             # floats behind the complex extent, and what they and the rest are filled with
WORST = {"power": {}, "profile": {}}         # output -> case id -> worst error / bound, printed by the last test
OUTPUTS = ("power", "profile")


@pytest.fixture(scope="module")
def eng():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _cb(c):
    F = case_inputs(c)[2]
    return None if F is None else F.astype(np.complex64)


def _shape(X, output):
    n, _, rows, taps = X.shape
    return (n, rows, taps) if output == "power" else (n, taps)


def _guarded(shape, X):
    """(the flat sentinel-filled buffer, the view of `shape` at its head, the untouched-guard check): the buffer covers the
    whole extent of the complex output X of the same users and GUARD floats more, so a store at the complex index of any
    user lands inside it and shows"""
    import torch
    size = int(np.prod(shape))
    big = torch.full((max(size, 2 * X.numel()) + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return big, big[:size].view(shape), lambda: bool((big[size:] == SENTINEL).all())


def _call(eng, c, prep, output, cb=None, **kw):
    """the call of a case; `cb`: the codebook as a device tensor, where the upload must not happen inside the call"""
    return eng.angle_delay(prep, c["n_taps"], n_fft=c["n_fft"], tx_codebook=_cb(c) if cb is None else cb, output=output, **kw)


def check_structure(got, shape, dead, what):
    import torch
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(shape) and got.is_contiguous(), what
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and (g >= 0).all(), f"{what}: NaN, inf or a negative value"
    gd = g[dead]
    assert (gd == 0).all() and not np.signbit(gd).any(), f"{what}: a user without paths is not +0.0"
    return g.astype(np.float64)


def check_power(c, P, p, X, what):
    """both outputs of a case against the reference at the derived bounds, and against the complex output X of the same build
    at the rounding terms alone; returns the two worst ratios"""
    P_ref, p_ref, tol_P, tol_p = R.case_power_ref(c)
    n, m_rx, rows, _ = X.shape
    dead = np.abs(case_inputs(c)[3]).reshape(n, -1).max(axis=1) == 0
    Pg = check_structure(P, P_ref.shape, dead, what + " power")
    pg = check_structure(p, p_ref.shape, dead, what + " profile")
    ratios = R.worst_ratio(Pg, P_ref, tol_P), R.worst_ratio(pg, p_ref, tol_p)
    print(f"{what}: worst error / bound = {ratios[0]:.3f} (power), {ratios[1]:.3f} (profile) over {int((~dead).sum())} live users")
    WORST["power"][what], WORST["profile"][what] = ratios
    assert ratios[0] <= 1 and ratios[1] <= 1, f"{what}: out of the bound, worst error / bound {ratios}"
    PX = R.power_from_adp(X.cpu().numpy())[0]
    assert (np.abs(Pg - PX) <= (m_rx + 2) * R.U32 * PX + R.FLT_MIN).all(), f"{what}: power is not the sum over the complex call's output"
    row_sum = Pg.sum(axis=1)
    assert (np.abs(pg - row_sum) <= (rows + 1) * R.U32 * row_sum + R.FLT_MIN).all(), f"{what}: profile is not the row sum of the power matrix"
    return ratios


# ---- 1. accuracy and structure on every case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_power_and_profile_against_the_definition(c, eng):
    import torch
    prep, X = _launch(eng, c)
    outs, bufs = {}, {}
    for output in OUTPUTS:
        rows = X.shape[2]
        assert eng.angle_delay_supported(prep, rows, c["n_fft"], c["n_taps"], output)
        _, view, bufs[output] = _guarded(_shape(X, output), X)
        outs[output] = _call(eng, c, prep, output, out=view)
        assert outs[output] is view
    again = {o: _call(eng, c, prep, o) for o in OUTPUTS}
    torch.cuda.synchronize()
    for output in OUTPUTS:
        assert bufs[output](), f"{c['id']} {output}: written beyond the smaller output"
        assert torch.equal(again[output], outs[output]), f"{c['id']} {output}: a second launch differs"
    if c["rays"] == "counts":
        assert (np.abs(case_inputs(c)[3]).reshape(c["n"], -1).max(axis=1) == 0).sum() >= c["n"] // 5     # the users without a path
    check_power(c, outs["power"], outs["profile"], X, c["id"])


# ---- 2. determinism: sub-ranges, a side stream, a captured graph ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["s0_minus5_dft", "s0_minus5_ant", "taps65_dft", "taps1_ant", "wpb2_users7"])
@pytest.mark.parametrize("output", OUTPUTS)
def test_user_sub_range_equals_the_rows_of_the_whole_launch(cid, output, eng):
    """user_begin > 0 with a count that is no multiple of the waves of a workgroup; rows outside the range stay untouched"""
    import torch
    c = BY_ID[cid]
    prep, X = _launch(eng, c)
    full = _call(eng, c, prep, output)
    b, cnt = (1, c["n"] - 3) if c["n"] < 30 else (5, 15)                     # taps1, profile: the range begins 4 bytes in
    _, view, untouched = _guarded(_shape(X, output), X)
    got = _call(eng, c, prep, output, user_begin=b, user_count=cnt, out=view[b:b + cnt])
    torch.cuda.synchronize()
    assert torch.equal(got, full[b:b + cnt])
    assert bool((view[:b] == SENTINEL).all()) and bool((view[b + cnt:] == SENTINEL).all()) and untouched()
    empty = _call(eng, c, prep, output, user_begin=c["n"], user_count=0)
    assert tuple(empty.shape) == (0,) + tuple(full.shape[1:]) and empty.dtype == torch.float32


@pytest.mark.parametrize("output", OUTPUTS)
def test_out_of_the_wrong_shape_or_dtype_is_refused(output, eng):
    import torch
    c = BY_ID["defaults_K64_dft"]
    prep, X = _launch(eng, c)
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor"):
        _call(eng, c, prep, output, out=torch.empty_like(X))
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor"):
        _call(eng, c, prep, output, out=torch.empty(_shape(X, output), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("cid", ["defaults_K512_dft", "taps33_ant", "rows65"])
def test_side_stream_and_captured_graph_give_the_same_bits(cid, eng):
    """the pattern of tests/test_gpu_graph_capture.py: an eager warm-up, `reprepare` + the call captured in one graph, a replay"""
    import torch
    c = BY_ID[cid]
    prep, X = _launch(eng, c)
    want = {o: _call(eng, c, prep, o) for o in OUTPUTS}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = {o: _call(eng, c, prep, o) for o in OUTPUTS}
    side.synchronize()
    for o in OUTPUTS:
        assert torch.equal(got[o], want[o]), f"{cid} {o}: a side stream gives other bits"
    outs = {o: torch.empty_like(want[o]) for o in OUTPUTS}
    records = prep.workspace.clone()
    cb = None if _cb(c) is None else torch.from_numpy(_cb(c)).to(eng.device)     # resident: a capture takes no host upload

    def sequence():
        eng.reprepare(prep)
        for o in OUTPUTS:
            _call(eng, c, prep, o, cb=cb, out=outs[o])
    sequence()                                                               # warm-up outside the capture
    torch.cuda.synchronize()
    assert torch.equal(prep.workspace, records), "the call changed the records"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence()
    for o in OUTPUTS:
        outs[o].fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for o in OUTPUTS:
        assert torch.equal(outs[o], want[o]), f"{cid} {o}: the replayed graph gives other bits"


# ---- 3. flag combinations ----------------------------------------------------------------------------------------------------------
def test_adaptive_terms_workspace(eng):
    """the records in order of falling amplitude (DMX_FLAG_ADAPTIVE_TERMS on the preparation) with the output bits on the call"""
    import torch
    c = BY_ID["adaptive_workspace"]
    assert c["adaptive"]
    prep, X = _launch(eng, c)
    from deepmimo_amd import _native as nat
    assert prep.params_struct.flags == nat.FLAG_ADAPTIVE_TERMS                   # the preparation keeps its own flags
    P, p = (_call(eng, c, prep, o) for o in OUTPUTS)
    torch.cuda.synchronize()
    assert prep.params_struct.flags == nat.FLAG_ADAPTIVE_TERMS
    check_power(c, P, p, X, "adaptive terms")


def _near_field_cases():
    from tests import _near_field_cases as NC
    return [c["id"] for c in NC.CONSUMER_CASES]


@pytest.mark.parametrize("cid", _near_field_cases())
@pytest.mark.parametrize("codebook", ["dft", None])
def test_near_field_view(cid, codebook):
    """on `Dataset.near_field`: the complex128 near-field channel of tests/_near_field_ref.py through the same reduction"""
    import deepmimo_amd as dm
    from tests import _near_field_cases as NC
    from tests._angle_delay_ref import adp_from_channel, dft_codebook
    from tests.test_gpu_near_field_consumers import _adp_sizes
    case, p = NC.BY_ID[cid], NC.dm_params(NC.BY_ID[cid])
    n_fft, n_taps = _adp_sizes(case)
    F = dft_codebook(case["bs"]) if codebook == "dft" else None
    view = NC.dataset(case, "a").near_field(NC.CARRIER)
    X_ref = adp_from_channel(NC.references(case)[0], None if F is None else F.astype(np.complex64), n_fft, n_taps)
    P_ref, p_ref = R.power_from_adp(X_ref)
    tol_P, tol_p = R.power_bounds(X_ref)
    P = view.compute_angle_delay(p, n_taps=n_taps, n_fft=n_fft, codebook=codebook, output="power")
    pr = view.compute_angle_delay(p, n_taps=n_taps, n_fft=n_fft, codebook=codebook, output="profile")
    assert P.dtype == np.float32 and P.shape == P_ref.shape and pr.dtype == np.float32 and pr.shape == p_ref.shape
    ratios = R.worst_ratio(P, P_ref, tol_P), R.worst_ratio(pr, p_ref, tol_p)
    print(f"near field {cid} {codebook}: worst error / bound = {ratios[0]:.3f} (power), {ratios[1]:.3f} (profile)")
    assert ratios[0] <= 1 and ratios[1] <= 1, ratios
    far = NC.dataset(case, "a").compute_angle_delay(NC.dm_params(case), n_taps=n_taps, n_fft=n_fft, codebook=codebook, output="power")
    if int(np.prod(case["bs"])) > 1 and codebook == "dft":
        assert (np.abs(far - P_ref) > tol_P).any(), "the far-field output meets the near-field reference: the test cannot tell them apart"


# ---- 4. the bits clear: the complex output of the parent commit -----------------------------------------------------------------------
def complex_hashes(eng):
    """case id -> sha256 over the complex output of the call without the new bits"""
    import torch
    out = {}
    for c in CASES:
        X = _launch(eng, c)[1]
        torch.cuda.synchronize()
        out[c["id"]] = hashlib.sha256(X.cpu().numpy().tobytes()).hexdigest()
    return out


def test_bits_clear_gives_the_bits_of_the_parent_commit(eng):
    with open(HASHES) as f:
        want = json.load(f)
    got = complex_hashes(eng)
    assert set(got) == set(want) and len(want) == len(CASES)
    assert [k for k in want if got[k] != want[k]] == []


# ---- 5. through Dataset -------------------------------------------------------------------------------------------------------------
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


def _from_complex(x):
    """the bounds of a result of the complex call itself standing in for the reference: twice, since both sides carry an error"""
    P_ref, p_ref = R.power_from_adp(x)
    tol_P, tol_p = R.power_bounds(x)
    return P_ref, p_ref, 2 * tol_P, 2 * tol_p


def test_public_api_numpy_torch_host_and_hbm_rays():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 64, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    x = ds.compute_angle_delay(p, n_taps=32)
    P_np = ds.compute_angle_delay(p, n_taps=32, output="power")
    p_np = ds.compute_angle_delay(p, n_taps=32, output="profile")
    assert isinstance(P_np, np.ndarray) and P_np.dtype == np.float32 and P_np.shape == (90, 8, 32)
    assert isinstance(p_np, np.ndarray) and p_np.dtype == np.float32 and p_np.shape == (90, 32)
    P_ref, p_ref, tol_P, tol_p = _from_complex(x)
    assert R.worst_ratio(P_np, P_ref, tol_P) <= 1 and R.worst_ratio(p_np, p_ref, tol_p) <= 1
    dead = ds.num_paths == 0                                                 # the field of view leaves some users no path
    assert dead.any() and (P_np[dead] == 0).all() and (p_np[dead] == 0).all() and (p_np[~dead].max(axis=1) > 0).all()
    dm.config("channel_output", "torch")
    try:
        P_t = ds.compute_angle_delay(p, n_taps=32, output="power")
        p_t = ds.compute_angle_delay(p, n_taps=32, output="profile")
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(P_t, torch.Tensor) and P_t.is_cuda and P_t.dtype == torch.float32
    assert np.array_equal(P_np.view(np.int32), P_t.cpu().numpy().view(np.int32))
    assert np.array_equal(p_np.view(np.int32), p_t.cpu().numpy().view(np.int32))
    # rays on the host and in HBM: the same bits
    host = dm.Dataset({k: v.copy() for k, v in rays.items()})
    hbm = dm.Dataset({k: torch.from_numpy(v.copy()).cuda() for k, v in rays.items()})
    for output in OUTPUTS:
        a, b = (d.compute_angle_delay(p, n_taps=32, output=output) for d in (host, hbm))
        assert isinstance(b, np.ndarray) and np.array_equal(a.view(np.int32), b.view(np.int32)), output
    # the helpers on the result
    delays = dm.tap_delays(p, 32)
    mean, rms = dm.delay_spread(p_np, delays)
    assert mean.shape == rms.shape == (90,) and np.isnan(mean[dead]).all() and np.isfinite(mean[~dead]).all()
    assert (mean[~dead] >= 0).all() and (mean[~dead] <= delays[-1]).all() and (rms[~dead] <= delays[-1]).all()
    tm, tr = dm.delay_spread(p_t, delays)
    assert tm.is_cuda and np.allclose(tm.cpu().numpy(), mean, rtol=1e-12, atol=0, equal_nan=True)


def test_orthonormal_codebook_profile_is_the_antenna_domain_profile():
    """Parseval: `"dft"` rows are orthonormal, so the two profiles agree within the sum of their bounds"""
    import deepmimo_amd as dm
    rays, p = _small(41, 25, (4, 2), (2, 1), 64, seed=9)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    pa = ds.compute_angle_delay(p, n_taps=24, n_fft=128, output="profile")
    pb = ds.compute_angle_delay(p, n_taps=24, n_fft=128, codebook=None, output="profile")
    tol = _from_complex(ds.compute_angle_delay(p, n_taps=24, n_fft=128))[3] / 2 + \
        _from_complex(ds.compute_angle_delay(p, n_taps=24, n_fft=128, codebook=None))[3] / 2
    assert pa.shape == pb.shape == (41, 24) and (pa > 0).any()
    assert (np.abs(pa.astype(np.float64) - pb) <= tol).all()


def test_macro_dataset_and_at_times():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(0, 512, 4)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    for output, tail in (("power", (8, 24)), ("profile", (24,))):
        both = macro.compute_angle_delay(p, n_taps=24, output=output)
        assert isinstance(both, list) and len(both) == 2
        for r, got in zip((a, b), both):
            alone = dm.Dataset({k: v.copy() for k, v in r.items()}).compute_angle_delay(p, n_taps=24, output=output)
            assert got.shape == alone.shape == (len(r["power"]),) + tail and got.dtype == np.float32
            assert np.array_equal(got.view(np.int32), alone.view(np.int32))
    # a view of at_times: time-major users, every snapshot against the reference channel of that time
    from tests import test_gpu_time_series as ts
    from tests._angle_delay_ref import adp_from_channel, dft_codebook
    H_ref = ts._consumer_reference()
    view = ts._dataset(ts._rays(), ts._CONSUMER).at_times(ts.TIMES, carrier_freq=ts.FC)
    pc = ts._dm_params(ts._CONSUMER, np.zeros(3))
    P = view.split_times(view.compute_angle_delay(pc, n_taps=8, output="power"))
    pr = view.split_times(view.compute_angle_delay(pc, n_taps=8, output="profile"))
    assert P.shape == (len(ts.TIMES), ts.N_UE, 8, 8) and pr.shape == (len(ts.TIMES), ts.N_UE, 8)
    for t in range(len(ts.TIMES)):
        X_ref = adp_from_channel(H_ref[t], dft_codebook(ts._CONSUMER["bs_shape"]), 16, 8)
        (P_ref, p_ref), (tol_P, tol_p) = R.power_from_adp(X_ref), R.power_bounds(X_ref)
        assert R.worst_ratio(P[t], P_ref, tol_P) <= 1 and R.worst_ratio(pr[t], p_ref, tol_p) <= 1, f"snapshot {t}"


def test_zz_report_worst_ratios():
    """Last in the file: the worst error / bound per output over every case that ran (README.md quotes both)"""
    for output, seen in WORST.items():
        if seen:
            k = max(seen, key=lambda i: seen[i])
            print(f"angle-delay {output}: worst error / bound over {len(seen)} cases = {seen[k]:.3f} ({k})")
            assert seen[k] <= 1.0


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:                                         # run with DMX_LIB_PATH at a build of the parent commit
        from deepmimo_amd.engine import ChannelEngine
        with open(HASHES, "w") as f:
            json.dump(complex_hashes(ChannelEngine(0)), f, indent=1, sort_keys=True)
        print(f"wrote {HASHES}")
