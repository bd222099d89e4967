"""The linear MMSE receiver of the codebook rate (DMX_FLAG_RX_LINEAR_MMSE, `receiver="mmse"`: epilogue_mmse of
k7_rate_body.h in k10_codebook_rate.hip) on the GPU.

Reference: the definition, np.linalg.inv in complex128 of the NumPy oracle's channel tensor times the codebook
(tests/_mmse_rate_ref.py; tests/test_mmse_rate_cpu.py pins it against hand cases and shows that its tolerance tells the two
receivers apart on every case here).  Criterion per entry: |rate_c - ref| <= tol_c with the derived tolerance of that module,
and rate_c_mmse <= rate_c_joint + tol_mmse + tol_joint against the joint call on the same preparation.  Every case also holds
the structural checks of tests/test_gpu_codebook_rate.py `check_result`.  The cases are that module's with two layers or
more, and three of this module's: users of rank one under two layers, and the subcarrier-chunk tail at K = 65 and K = 70.
With the flag clear every output of the existing cases hashes equal to tests/golden/mmse_rate_joint_hashes.json, recorded
with a build of the parent commit (`DMX_LIB_PATH=<that build> python -m tests.test_gpu_mmse_rate --record` writes the file).
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests import test_gpu_codebook_rate as gcb
from tests._codebook_rate_ref import case_codebook, case_snr
from tests._mmse_rate_ref import mmse_rate_from_channel, mmse_rate_tolerance

pytestmark = pytest.mark.gpu

HASHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmse_rate_joint_hashes.json")
HASH_SUBBAND = shapes.ML_SUBBAND

FROM_CODEBOOK_RATE = ["L2_4x2", "L4_4x4", "L3_C10", "L3_C11", "L4_C8", "L4_C9", "slices_K1", "slices_K3", "slices_K7", "slices_K33",
                      "C1", "irregular", "per_user_rot", "doppler", "adaptive_workspace", "P32_num_paths_below_loaded"]
L1_CASES = ["defaults", "panel_C64"]


def _cases():
    by = {c["id"]: c for c in gcb.CASES}
    cs = [by[i] for i in FROM_CODEBOOK_RATE]
    own = [gcb._cb("mmse_counts_L2", 45, 25, [4, 2], [2, 1], 512, [0, 3, 200], 2, 8, rays="counts"),   # a fifth of rank one
           gcb._cb("mmse_K65_L2", 24, 25, [4, 2], [2, 1], 512, range(3, 68), 2, 4),                    # a chunk and one subcarrier
           gcb._cb("mmse_K70_L2", 23, 25, [8, 1], [2, 1], 512, shapes.K70, 2, 4)]                      # a second chunk 6 wide
    for c in own:
        c["selected"] = list(c["selected"])
        c.setdefault("adaptive", False)
    # every (M_rx, L >= 2) the kernel is instantiated for, and every kept-path count under two layers
    return cs + own + [c for c in shapes.CODEBOOK_CASES if c["layers"] >= 2]


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
SUBBAND_CASES = [("L2_4x2", (1, 2, 5)), ("slices_K7", (1, 3, 9)), ("mmse_K70_L2", (1, 32, 70))]   # B = 1, a short last one, B >= K
WORST = {}                                   # case id -> (worst err / tol, worst |err| in bit), printed by the last test
_REFS = {}


def mmse_ref(c):
    """(ref_c, tol_c) of the linear MMSE rate of a case: computed once, shared and left unchanged"""
    if c["id"] not in _REFS:
        _, _, H, W, snr, _ = gcb.case_inputs(c)
        _REFS[c["id"]] = (mmse_rate_from_channel(H, W, snr)[0], mmse_rate_tolerance(H, W, snr)[0])
        for a in _REFS[c["id"]]:
            a.setflags(write=False)
    return _REFS[c["id"]]


def _prepare(eng, c, selected=None):
    rays, ue_rot = gcb.case_inputs(c)[:2]
    cc = c if selected is None else dict(c, selected=list(selected))
    p = gcb._dm_params(cc).validate(c["n"])
    return eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **gcb._kwargs(c, ue_rot))


def _db(snr):
    return float(10 * np.log10(snr))


def _equal(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def eng():
    return gcb._engine()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_mmse_rate_against_the_definition(c, eng):
    import torch
    _, _, H, W, snr, (ref_joint, tol_joint) = gcb.case_inputs(c)
    ref_c, tol_c = mmse_ref(c)
    prep = _prepare(eng, c)
    assert c["layers"] >= 2 and eng.codebook_rate_supported(prep, c["C"], c["layers"], receiver="mmse")
    db = _db(snr)
    first = eng.codebook_rate(prep, W, db, per_codeword=True, receiver="mmse")
    second = eng.codebook_rate(prep, W, db, per_codeword=True, receiver="mmse")
    alone = eng.codebook_rate(prep, W, db, receiver="mmse")
    joint = eng.codebook_rate(prep, W, db, per_codeword=True)
    torch.cuda.synchronize()
    assert len(first) == 3 and len(alone) == 2
    ratio = gcb.check_result(*first, H, (ref_c, tol_c), f"mmse {c['id']}", again=second, alone=alone)
    rc, rj = first[2].cpu().numpy(), joint[2].cpu().numpy()
    WORST[c["id"]] = (ratio, float(np.abs(rc - ref_c).max()))
    over = rc - rj - (tol_c + tol_joint)
    print(f"mmse {c['id']}: largest mmse - joint - tolerances = {over.max():.3e} bit, mean loss {float((rj - rc).mean()):.3f} bit")
    assert (over <= 0).all(), f"{c['id']}: the linear receiver beats the joint one by more than the two tolerances"
    assert not torch.equal(first[2], joint[2]), f"{c['id']}: the flag changed nothing"


@pytest.mark.parametrize("cid", L1_CASES)
def test_one_layer_is_bit_equal_to_the_call_without_the_flag(cid, eng):
    import torch
    c = {c["id"]: c for c in gcb.CASES}[cid]
    W, snr = gcb.case_inputs(c)[3:5]
    assert c["layers"] == 1
    prep = _prepare(eng, c)
    db = _db(snr)
    assert _equal(eng.codebook_rate(prep, W, db, per_codeword=True, receiver="mmse"), eng.codebook_rate(prep, W, db, per_codeword=True))
    assert _equal(eng.codebook_rate_subbands(prep, W, db, 2, per_codeword=True, receiver="mmse"),
                  eng.codebook_rate_subbands(prep, W, db, 2, per_codeword=True))
    torch.cuda.synchronize()


@pytest.mark.parametrize("cid,B", [(cid, B) for cid, Bs in SUBBAND_CASES for B in Bs], ids=lambda v: str(v))
def test_subbands_equal_the_wideband_flagged_call(cid, B, eng):
    import torch
    from tests._subband_pmi_ref import subband_edges
    from tests.test_gpu_subband_pmi import check_trio
    c = BY_ID[cid]
    _, _, H, W, snr, _ = gcb.case_inputs(c)
    sel, n, C = c["selected"], c["n"], c["C"]
    edges = subband_edges(len(sel), B)
    n_sb = len(edges)
    prep = _prepare(eng, c)
    db = _db(snr)
    assert eng.codebook_rate_subbands_supported(prep, C, c["layers"], B, receiver="mmse")
    six = eng.codebook_rate_subbands(prep, W, db, B, per_codeword=True, receiver="mmse")
    assert _equal(six, eng.codebook_rate_subbands(prep, W, db, B, per_codeword=True, receiver="mmse")), "a second launch differs"
    assert _equal(six[:4], eng.codebook_rate_subbands(prep, W, db, B, receiver="mmse")), "the call without rate_c differs"
    rate, pmi, rate_sb, pmi_sb, rate_c, rate_sb_c = six
    assert tuple(rate_sb_c.shape) == (n, n_sb, C) and tuple(pmi_sb.shape) == (n, n_sb)
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    ref_c, tol_c = mmse_ref(c)
    r, p, rsb, psb, rc, rsbc = (t.cpu().numpy() for t in six)
    check_trio(r, p, rc, dead, f"mmse {cid} B{B} wideband")
    assert (np.abs(rc - ref_c) <= tol_c).all(), "the wideband outputs of the subband form miss the tolerance"
    wide = eng.codebook_rate(prep, W, db, per_codeword=True, receiver="mmse")
    if n_sb == 1:
        assert _equal((rate, pmi, rate_c), wide), "one subband, but the wideband outputs are not the wideband call's"
    for s, (a, b) in enumerate(edges):
        check_trio(rsb[:, s], psb[:, s], rsbc[:, s], dead, f"mmse {cid} B{B} subband {s}")
        sub = wide if n_sb == 1 else eng.codebook_rate(_prepare(eng, c, sel[a:b]), W, db, per_codeword=True, receiver="mmse")
        for name, got, want in (("rate_sb", rate_sb[:, s], sub[0]), ("pmi_sb", pmi_sb[:, s], sub[1]), ("rate_sb_c", rate_sb_c[:, s], sub[2])):
            assert torch.equal(got.contiguous(), want), f"{name}[:, {s}] is not the wideband call on the selection [{a}:{b}]"


def test_user_sub_range_and_engine_blocks_give_the_same_bits(eng, monkeypatch):
    n = 37
    rays, p = gcb._small(n)
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    W = case_codebook([4, 2], 5, 2)
    full = eng.codebook_rate(prep, W, 97.0, per_codeword=True, receiver="mmse")
    full_sb = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True, receiver="mmse")
    assert bool((full[0] > 0).any()) and not _equal(full, eng.codebook_rate(prep, W, 97.0, per_codeword=True))
    b, cnt = 5, 15
    for whole, part in ((full, eng.codebook_rate(prep, W, 97.0, per_codeword=True, user_begin=b, user_count=cnt, receiver="mmse")),
                        (full_sb, eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True, user_begin=b, user_count=cnt,
                                                             receiver="mmse"))):
        assert _equal(part, [f[b:b + cnt] for f in whole])
    calls = []
    real = eng.lib.dmx_codebook_rate

    def counted(*a):
        calls.append(int(a[5]))
        return real(*a)
    monkeypatch.setattr(eng, "CODEBOOK_WS_BYTES", 512 + 6 * (5 * 2 * 11 * 8 + 4), raising=False)
    monkeypatch.setattr(eng.lib, "dmx_codebook_rate", counted, raising=False)
    assert _equal(eng.codebook_rate(prep, W, 97.0, per_codeword=True, receiver="mmse"), full) and calls == [6] * 6 + [1]
    assert _equal(eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True, receiver="mmse"), full_sb)


def test_side_stream_gives_the_bits_of_the_default_stream(eng):
    import torch
    c = BY_ID["L2_4x2"]
    W, snr = gcb.case_inputs(c)[3:5]
    prep = _prepare(eng, c)
    Wd = torch.from_numpy(W).to(eng.device)
    want = eng.codebook_rate(prep, Wd, _db(snr), per_codeword=True, receiver="mmse")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    with torch.cuda.stream(side):
        got = eng.codebook_rate(prep, Wd, _db(snr), per_codeword=True, receiver="mmse")
    side.synchronize()
    assert _equal(got, want)


def test_captured_graph_gives_the_bits_of_the_eager_call(eng):
    """one stream, no parallel branches: the projection, then the kernel"""
    import torch
    c = BY_ID["L4_4x4"]
    W, snr = gcb.case_inputs(c)[3:5]
    prep = _prepare(eng, c)
    Wd = torch.from_numpy(W).to(eng.device)
    want = eng.codebook_rate_subbands(prep, Wd, _db(snr), 2, per_codeword=True, receiver="mmse")    # the warm-up too
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = eng.codebook_rate_subbands(prep, Wd, _db(snr), 2, per_codeword=True, receiver="mmse")
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(got, want)


def test_csi_report_ranks_under_the_linear_receiver():
    import deepmimo_amd as dm
    c = BY_ID["L4_4x4"]
    rays, _, H, _, snr, _ = gcb.case_inputs(c)
    assert c["bs_shape"] == [4, 4] and c["ue_shape"] == [2, 2] and not c["per_user_rot"] and c["bs_fov"] is None and not c["doppler"]
    ranks = (1, 2, 4)
    cbs = [case_codebook(c["bs_shape"], 4, L) for L in ranks]
    db = _db(snr)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    joint = ds.compute_csi_report(gcb._dm_params(c), codebooks=cbs, snr_db=db, subband_size=2)
    mmse = ds.compute_csi_report(gcb._dm_params(c), codebooks=cbs, snr_db=db, subband_size=2, receiver="mmse")
    assert set(mmse.keys()) == set(joint.keys()) and mmse.rate_by_rank.shape == (c["n"], 3)
    assert np.array_equal(mmse.rate_by_rank[:, 0].view(np.int32), joint.rate_by_rank[:, 0].view(np.int32))
    from tests._codebook_rate_ref import codebook_rate_tolerance
    dead = np.abs(H).reshape(c["n"], -1).max(axis=1) == 0
    tol_m = np.zeros((c["n"], 3))
    tol_j = np.zeros((c["n"], 3))
    for i, W in enumerate(cbs):
        tol_j[:, i] = codebook_rate_tolerance(H, W, snr)[0].max(axis=1)
        if ranks[i] > 1:
            tol_m[:, i] = mmse_rate_tolerance(H, W, snr)[0].max(axis=1)
            # the wideband outputs of the subband form: the per-rank call's rate, and the definition's best within tolerance
            per_rank = ds.compute_subband_pmi(gcb._dm_params(c), codebook=W, snr_db=db, subband_size=2, receiver="mmse")
            assert np.array_equal(per_rank[0].view(np.int32), mmse.rate_by_rank[:, i].view(np.int32))
            assert (np.abs(mmse.rate_by_rank[:, i] - mmse_rate_from_channel(H, W, snr)[0].max(axis=1)) <= tol_m[:, i]).all()
    assert (mmse.rate_by_rank[:, 1:] <= joint.rate_by_rank[:, 1:] + tol_m[:, 1:] + tol_j[:, 1:]).all()
    # the rank: the first maximum over the columns, 0 without a path; never above the joint receiver's where the rates that
    # decide either clear their tolerances
    first_max = np.asarray(ranks, np.int32)[mmse.rate_by_rank.argmax(axis=1)]
    assert np.array_equal(mmse.rank, np.where(dead, 0, first_max)) and dead.any()
    srt_m, srt_j = np.sort(mmse.rate_by_rank, axis=1), np.sort(joint.rate_by_rank, axis=1)
    clear = (srt_m[:, -1] - srt_m[:, -2] > 2 * tol_m.max(axis=1)) & (srt_j[:, -1] - srt_j[:, -2] > 2 * tol_j.max(axis=1)) & ~dead
    assert clear.sum() >= c["n"] // 2 and (mmse.rank[clear] <= joint.rank[clear]).all()
    print(f"csi report: rank lower under the linear receiver for {(mmse.rank < joint.rank).sum()} of {(~dead).sum()} users")
    for k in ("rate", "pmi", "rate_sb", "pmi_sb"):
        assert mmse[k].shape == joint[k].shape and mmse[k].dtype == joint[k].dtype
    assert (mmse.rate[dead] == 0).all() and (mmse.pmi[dead] == -1).all() and (mmse.pmi_sb[dead] == -1).all()


def test_public_api_numpy_torch_host_and_hbm_rays_and_the_macro_fan_out():
    import torch
    import deepmimo_amd as dm
    rays, p = gcb._small(61, 25, (4, 2), (2, 1), 4, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    H = ds.compute_channels(p)
    db = _db(case_snr(H))
    snr = 10.0 ** (db / 10.0)
    W = case_codebook([4, 2], 4, 2)
    three = ds.compute_codebook_rate(p, codebook=W, snr_db=db, per_codeword=True, receiver="mmse")
    pair = ds.compute_codebook_rate(p, codebook=W, snr_db=db, receiver="mmse")
    six = ds.compute_subband_pmi(p, codebook=W, snr_db=db, subband_size=3, per_codeword=True, receiver="mmse")
    assert len(pair) == 2 and len(three) == 3 and len(six) == 6 and all(isinstance(t, np.ndarray) for t in three + six)
    assert np.array_equal(pair[0].view(np.int32), three[0].view(np.int32)) and np.array_equal(pair[1], three[1])
    ref_c, tol_c = mmse_rate_from_channel(H, W, snr)[0], mmse_rate_tolerance(H, W, snr)[0]
    assert (np.abs(three[2] - ref_c) <= tol_c).all() and (np.abs(six[4] - ref_c) <= tol_c).all()
    assert not np.array_equal(three[2], ds.compute_codebook_rate(p, codebook=W, snr_db=db, per_codeword=True)[2])
    dm.config("channel_output", "torch")
    try:
        three_t = ds.compute_codebook_rate(p, codebook=W, snr_db=db, per_codeword=True, receiver="mmse")
        # rays already in HBM
        dev = dm.Dataset({k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") if k not in ("rx_pos", "tx_pos") else v.copy()
                          for k, v in rays.items()})
        three_d = dev.compute_codebook_rate(p, codebook=W, snr_db=db, per_codeword=True, receiver="mmse")
    finally:
        dm.config("channel_output", "numpy")
    for a, b, d in zip(three, three_t, three_d):
        assert isinstance(b, torch.Tensor) and b.is_cuda and np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
        assert np.array_equal(a.view(np.int32), d.cpu().numpy().view(np.int32))
    # MacroDataset fans out unchanged
    other = gcb._small(18, 25, (4, 2), (2, 1), 4, seed=23)[0]
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (rays, other)])
    both = macro.compute_codebook_rate(p, codebook=W, snr_db=db, per_codeword=True, receiver="mmse")
    assert isinstance(both, list) and len(both) == 2
    for x, y in zip(both[0], three):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    reports = macro.compute_csi_report(p, codebooks=[W[:, :1], W], snr_db=db, receiver="mmse")
    assert len(reports) == 2 and np.array_equal(reports[0].rate_by_rank[:, 1].view(np.int32), three[0].view(np.int32))


def test_near_field_view_against_the_near_field_reference():
    from tests import _near_field_cases as NC
    case = NC.CONSUMER_CASES[0]
    for cand in NC.CONSUMER_CASES:                                    # the first case whose UE takes two layers
        if int(np.prod(cand["ue"])) >= 2:
            case = cand
            break
    assert int(np.prod(case["ue"])) >= 2
    p, H = NC.dm_params(case), NC.references(case)[0]
    W = case_codebook(case["bs"], 5, 2)
    snr = case_snr(H)
    view = NC.dataset(case, "a").near_field(NC.CARRIER)
    rate, pmi, rate_c = view.compute_codebook_rate(p, codebook=W, snr_db=_db(snr), per_codeword=True, receiver="mmse")
    ref_c, tol_c = mmse_rate_from_channel(H, W, snr)[0], mmse_rate_tolerance(H, W, snr)[0]
    ratio = float((np.abs(rate_c - ref_c) / tol_c).max())
    print(f"near field {case['id']}: worst err / tol = {ratio:.3f}")
    assert ratio <= 1.0 and np.array_equal(rate.view(np.int32), rate_c[np.arange(len(pmi)), np.maximum(pmi, 0)].view(np.int32))


def test_at_times_and_rx_combiner_views():
    from tests import test_gpu_time_series as ts
    H_ref = ts._consumer_reference()
    p = ts._dm_params(ts._CONSUMER, np.zeros(3))
    W = case_codebook(ts._CONSUMER["bs_shape"], 4, 2)
    snr = case_snr(H_ref[0])
    ds = ts._dataset(ts._rays(), ts._CONSUMER)
    view = ds.at_times(ts.TIMES, carrier_freq=ts.FC)
    rate_c = view.split_times(view.compute_codebook_rate(p, codebook=W, snr_db=_db(snr), per_codeword=True, receiver="mmse")[2])
    assert rate_c.shape == (len(ts.TIMES), ts.N_UE, 4)
    for t in range(len(ts.TIMES)):
        ref_c, tol_c = mmse_rate_from_channel(H_ref[t], W, snr)[0], mmse_rate_tolerance(H_ref[t], W, snr)[0]
        assert (np.abs(rate_c[t] - ref_c) <= tol_c).all(), f"snapshot {t}"
    # behind a UE combiner every user has one antenna and one layer: the two receivers are the same bits
    comb = ds.with_rx_combiner("dft", p)
    W1 = W[:, :1]
    a = comb.compute_codebook_rate(codebook=W1, snr_db=_db(snr), per_codeword=True, receiver="mmse")
    b = comb.compute_codebook_rate(codebook=W1, snr_db=_db(snr), per_codeword=True)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b)) and a[0].shape == (2 * ts.N_UE,)


# ---- the flag clear: the bits of the parent commit ---------------------------------------------------------------------------------
def joint_hashes(eng):
    """case id -> sha256 over the three outputs of codebook_rate and the six of codebook_rate_subbands (B = 2), flag clear"""
    import torch
    out = {}
    for c in gcb.CASES:
        W, snr = gcb.case_inputs(c)[3:5]
        prep = _prepare(eng, c)
        res = eng.codebook_rate(prep, W, _db(snr), per_codeword=True) + eng.codebook_rate_subbands(prep, W, _db(snr), HASH_SUBBAND,
                                                                                                   per_codeword=True)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in res:
            h.update(t.cpu().numpy().tobytes())
        out[c["id"]] = h.hexdigest()
    return out


def test_flag_clear_gives_the_bits_of_the_parent_commit(eng):
    with open(HASHES) as f:
        want = json.load(f)
    got = joint_hashes(eng)
    assert set(got) == set(want) == {c["id"] for c in gcb.CASES}
    assert [k for k in got if got[k] != want[k]] == []


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol and the worst absolute error over every case that ran (README.md quotes both)"""
    if WORST:
        for k in sorted(WORST):
            print(f"mmse rate {k}: worst err / tol = {WORST[k][0]:.3f}, worst |err| = {WORST[k][1]:.3e} bit")
        k = max(WORST, key=lambda i: WORST[i][0])
        ka = max(WORST, key=lambda i: WORST[i][1])
        print(f"mmse rate: worst err / tol over {len(WORST)} cases = {WORST[k][0]:.3f} ({k}); worst |err| = {WORST[ka][1]:.3e} bit ({ka})")
        assert WORST[k][0] <= 1.0


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:                                 # run with DMX_LIB_PATH at a build of the parent commit
        with open(HASHES, "w") as f:
            json.dump(joint_hashes(gcb._engine()), f, indent=1, sort_keys=True)
            f.write("\n")
