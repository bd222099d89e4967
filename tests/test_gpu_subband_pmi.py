"""Subband PMI and CSI report per user (dmx_codebook_rate_subbands, the subband form of k10_codebook_rate.hip;
Dataset.compute_subband_pmi / compute_csi_report) on the GPU.

Inputs: the cases of tests/test_gpu_codebook_rate.py (the same rays, codebooks, SNR and oracle tensor) with the subband sizes
of tests/_subband_pmi_cases.py.  Reference: tests/_subband_pmi_ref.py, the means of that module's per-subcarrier rates and
tolerances over each subband; no tolerance is chosen here.  Per case: |rate_sb_c - ref| <= tol_sb_c and |rate_c - ref| <= tol_c
entry by entry, the structural properties (first maximum, rate == rate_c[pmi] bit for bit, +0.0 / -1 for users without a path,
finite and >= 0), a second launch and a launch without the optional outputs give the same bits, and - what ties the subband
nest to the kernel the oracle tests already hold - column s of the three subband outputs equals, bit for bit,
ChannelEngine.codebook_rate on a preparation whose selection is that subband alone."""
import os

import numpy as np
import pytest

from tests._codebook_rate_ref import case_codebook, case_snr
from tests._subband_pmi_cases import RANK_CASES, RANK_CODEWORDS, RANK_LAYERS, RANK_SUBBANDS, SUBBAND_CASES, case_label
from tests._subband_pmi_ref import reference_ranks, subband_edges, subband_reference

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_codebook_rate import CASES, _small, case_inputs  # noqa: E402
from tests.test_gpu_fd_direct import _dm_params, _kwargs  # noqa: E402

BY_ID = {c["id"]: c for c in CASES}
WORST = {}                                   # label -> (worst err / tol, worst |err| in bit), printed by the last test


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _prepare(eng, c, rays, ue_rot, selected=None):
    cc = c if selected is None else dict(c, selected=list(selected))
    p = _dm_params(cc).validate(c["n"])
    return eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot))


def check_trio(r, p, rc, dead, what):
    """rate [m], pmi [m], rate_c [m, C] as NumPy: finite, >= 0, +0.0 / -1 where dead, the first maximum, rate = rate_c[pmi]"""
    C = rc.shape[1]
    assert np.isfinite(r).all() and np.isfinite(rc).all() and (r >= 0).all() and (rc >= 0).all(), f"{what}: NaN, inf or negative"
    assert (r[dead] == 0).all() and not np.signbit(r[dead]).any(), f"{what}: a user without paths is not +0.0"
    assert (rc[dead] == 0).all() and not np.signbit(rc[dead]).any(), f"{what}: rate_c of a user without paths is not +0.0"
    assert (p[dead] == -1).all() and (p[~dead] >= 0).all() and (p < C).all(), f"{what}: pmi outside -1 / 0..C-1"
    assert np.array_equal(p[~dead], rc[~dead].argmax(axis=1)), f"{what}: pmi is not the first maximum of rate_c"
    live = np.flatnonzero(~dead)
    assert np.array_equal(r[live].view(np.int32), rc[live, p[live]].view(np.int32)), f"{what}: rate is not rate_c[u, pmi]"


def check_against_reference(p, rc, ref_c, tol_c, dead, what):
    """|rc - ref| <= tol entry by entry and the slack rule of the chosen index; returns (worst err / tol, worst |err|)"""
    e = np.abs(rc - ref_c)
    ratio, worst_abs = (float((e / tol_c).max()), float(e.max())) if e.size else (0.0, 0.0)
    print(f"{what}: worst err / tol = {ratio:.3f}, worst |err| = {worst_abs:.3e} bit, largest rate {float(ref_c.max()):.2f}")
    assert (e <= tol_c).all(), f"{what}: {(e > tol_c).sum()} entries out of tolerance, worst err / tol {ratio:.3f}"
    live = np.flatnonzero(~dead)
    best = ref_c[live].argmax(axis=1)
    slack = tol_c[live, p[live]] + tol_c[live, best]
    assert (ref_c[live, p[live]] >= ref_c[live, best] - slack).all(), f"{what}: a pmi whose reference rate is not the best"
    return ratio, worst_abs


@pytest.mark.parametrize("cid,B", SUBBAND_CASES, ids=[case_label(*cb) for cb in SUBBAND_CASES])
def test_subbands_against_the_definition_and_the_wideband_call(cid, B):
    import torch
    c = BY_ID[cid]
    what = case_label(cid, B)
    eng = _engine()
    rays, ue_rot, H, W, snr, _ = case_inputs(c)
    n, C, sel = c["n"], c["C"], c["selected"]
    edges = subband_edges(len(sel), B)
    n_sb = len(edges)
    prep = _prepare(eng, c, rays, ue_rot)
    assert eng.codebook_rate_subbands_supported(prep, C, c["layers"], B)
    snr_db = 10 * np.log10(snr)
    first = eng.codebook_rate_subbands(prep, W, snr_db, B, per_codeword=True)
    second = eng.codebook_rate_subbands(prep, W, snr_db, B, per_codeword=True)
    alone = eng.codebook_rate_subbands(prep, W, snr_db, B)                   # without the optional outputs: the same bits
    torch.cuda.synchronize()
    assert len(first) == 6 and len(alone) == 4
    rate, pmi, rate_sb, pmi_sb, rate_c, rate_sb_c = first
    for t, dt, shape in ((rate, torch.float32, (n,)), (pmi, torch.int32, (n,)), (rate_sb, torch.float32, (n, n_sb)),
                         (pmi_sb, torch.int32, (n, n_sb)), (rate_c, torch.float32, (n, C)), (rate_sb_c, torch.float32, (n, n_sb, C))):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.is_cuda, (what, dt, shape)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), f"{what}: a second launch differs"
    assert all(torch.equal(a, b) for a, b in zip(first[:4], alone)), f"{what}: the call without the per-codeword outputs differs"

    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    if c["rays"] == "counts":
        assert dead.sum() >= n // 5
    r, p, rsb, psb, rc, rsbc = (t.cpu().numpy() for t in first)
    ref = subband_reference(H, W, snr, B)
    assert ref["rate_sb_c"].shape == (n, n_sb, C)
    check_trio(r, p, rc, dead, f"{what} wideband")
    worst = [check_against_reference(p, rc, ref["rate_c"], ref["tol_c"], dead, f"{what} wideband")]
    for s in range(n_sb):
        check_trio(rsb[:, s], psb[:, s], rsbc[:, s], dead, f"{what} subband {s}")
    # all subbands at once against the reference: [n, n_sb, C] as [n * n_sb, C]
    flat = lambda x: np.ascontiguousarray(x).reshape(n * n_sb, -1)           # noqa: E731
    worst.append(check_against_reference(flat(psb)[:, 0], flat(rsbc), flat(ref["rate_sb_c"]), flat(ref["tol_sb_c"]),
                                         np.repeat(dead, n_sb), f"{what} subbands"))
    WORST[what] = (max(w[0] for w in worst), max(w[1] for w in worst))

    # bit equality with the existing call on the sub-selection: every subband up to 10, else the first, a middle and the last
    wide = eng.codebook_rate(prep, W, snr_db, per_codeword=True)
    if n_sb == 1:
        assert torch.equal(rate, wide[0]) and torch.equal(pmi, wide[1]) and torch.equal(rate_c, wide[2]), \
            f"{what}: one subband, but the wideband outputs are not dmx_codebook_rate's"
    for s in (range(n_sb) if n_sb <= 10 else (0, n_sb // 2, n_sb - 1)):
        a, b = edges[s]
        sub = wide if n_sb == 1 else eng.codebook_rate(_prepare(eng, c, rays, ue_rot, sel[a:b]), W, snr_db, per_codeword=True)
        torch.cuda.synchronize()
        for name, got, want in (("rate_sb", rate_sb[:, s], sub[0]), ("pmi_sb", pmi_sb[:, s], sub[1]),
                                ("rate_sb_c", rate_sb_c[:, s], sub[2])):
            same = np.array_equal(_bits(got.contiguous()), _bits(want))
            assert same, f"{what}: {name}[:, {s}] is not dmx_codebook_rate of the selection [{a}:{b}] bit for bit"


def test_only_the_required_output():
    """the C call with every optional output NULL writes the same rate_sb bits, and each optional output alone its own"""
    import ctypes as C_
    import torch
    from deepmimo_amd.engine import snr_linear_from_db
    c = BY_ID["L1_C33"]
    eng = _engine()
    rays, ue_rot, H, W, snr, _ = case_inputs(c)
    prep = _prepare(eng, c, rays, ue_rot)
    snr_db = 10 * np.log10(snr)
    full = eng.codebook_rate_subbands(prep, W, snr_db, 2, per_codeword=True)
    names = ("rate", "pmi", "rate_sb", "pmi_sb", "rate_c", "rate_sb_c")
    cb = torch.from_numpy(W).to(eng.device)
    p = prep.params_struct
    nbytes = int(eng.lib.dmx_beam_workspace_bytes(C_.byref(p), c["n"], prep.n_paths_loaded, c["C"]))
    bws = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
    for keep in ((), ("pmi_sb",), ("rate_sb_c",), ("rate",), ("pmi",), ("rate_c",)):
        out = {k: torch.full_like(t, 77) for k, t in zip(names, full)}
        ptr = lambda k: C_.c_void_p(out[k].data_ptr()) if k == "rate_sb" or k in keep else None   # noqa: E731
        rc = eng.lib.dmx_codebook_rate_subbands(C_.byref(p), C_.c_void_p(prep.workspace.data_ptr()), prep.n_ue, prep.n_paths_loaded,
                                                0, c["n"], C_.c_void_p(cb.data_ptr()), c["C"], 1, C_.c_void_p(bws.data_ptr()),
                                                nbytes, snr_linear_from_db(snr_db), 2, ptr("rate_sb"), ptr("pmi_sb"),
                                                ptr("rate_sb_c"), ptr("rate"), ptr("pmi"), ptr("rate_c"), eng._stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, eng.lib.dmx_last_error()
        for k, want in zip(names, full):
            if k == "rate_sb" or k in keep:
                assert torch.equal(out[k], want), (keep, k)
            else:
                assert bool((out[k] == 77).all()), f"{k} was written although it was NULL"


def test_user_sub_range_equals_the_rows_of_the_whole_launch():
    import torch
    n = 37
    rays, p = _small(n)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    W = case_codebook([4, 2], 5, 2)
    full = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True)
    b, cnt = 5, 15
    part = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True, user_begin=b, user_count=cnt)
    torch.cuda.synchronize()
    assert bool((full[2] > 0).any()) and full[2].shape == (n, 2)
    for f, q in zip(full, part):
        assert q.shape[0] == cnt and torch.equal(q, f[b:b + cnt])
    empty = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True, user_begin=n, user_count=0)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 2), (0, 2), (0, 5), (0, 2, 5)]


def test_user_blocks_of_the_engine_are_invisible(monkeypatch):
    """with the beam workspace of a call forced down to a few users the blocked result equals the unblocked one"""
    import torch
    n = 37
    rays, p = _small(n)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    W = case_codebook([4, 2], 5, 2)
    whole = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True)
    calls = []
    real = eng.lib.dmx_codebook_rate_subbands

    def counted(*a):
        calls.append(int(a[5]))
        return real(*a)
    monkeypatch.setattr(eng, "CODEBOOK_WS_BYTES", 512 + 6 * (5 * 2 * 11 * 8 + 4), raising=False)
    monkeypatch.setattr(eng.lib, "dmx_codebook_rate_subbands", counted, raising=False)
    blocked = eng.codebook_rate_subbands(prep, W, 97.0, 2, per_codeword=True)
    torch.cuda.synchronize()
    assert calls == [6] * 6 + [1], calls
    for a, b in zip(whole, blocked):
        assert torch.equal(a, b)


def test_public_api_numpy_and_torch_returns_are_the_same_bits():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 5, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    H = ds.compute_channels(p)
    snr_db = float(10 * np.log10(case_snr(H)))
    four = ds.compute_subband_pmi(p, snr_db=snr_db, subband_size=2)
    six = ds.compute_subband_pmi(p, snr_db=snr_db, subband_size=2, per_codeword=True, codebook=dm.dft_codebook([8, 1]))
    one_sb = ds.compute_subband_pmi(p, snr_db=snr_db, per_codeword=True)                  # subband_size=None: one subband
    plain = ds.compute_codebook_rate(p, snr_db=snr_db, per_codeword=True)
    dm.config("channel_output", "torch")
    try:
        six_t = ds.compute_subband_pmi(p, snr_db=snr_db, subband_size=2, per_codeword=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(four, tuple) and len(four) == 4 and len(six) == 6
    shapes = [(90,), (90,), (90, 3), (90, 3), (90, 8), (90, 3, 8)]
    dtypes = [np.float32, np.int32, np.float32, np.int32, np.float32, np.float32]
    for t, sh, dt in zip(six, shapes, dtypes):
        assert isinstance(t, np.ndarray) and t.shape == sh and t.dtype == dt
    for a, b in zip(four, six):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in six_t)
    for a, b in zip(six, six_t):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    # one subband is compute_codebook_rate, bit for bit, in all six outputs
    assert one_sb[2].shape == (90, 1) and one_sb[5].shape == (90, 1, 8)
    for a, b in ((one_sb[0], plain[0]), (one_sb[1], plain[1]), (one_sb[4], plain[2]), (one_sb[2][:, 0], plain[0]),
                 (one_sb[3][:, 0], plain[1]), (one_sb[5][:, 0], plain[2])):
        assert np.array_equal(np.ascontiguousarray(a).view(np.int32), b.view(np.int32))
    # and the definition, from the channel tensor of the same dataset
    ref = subband_reference(H, dm.dft_codebook([8, 1])[:, None, :], 10.0 ** (snr_db / 10.0), 2)
    assert (np.abs(six[5] - ref["rate_sb_c"]) <= ref["tol_sb_c"]).all() and (np.abs(six[4] - ref["rate_c"]) <= ref["tol_c"]).all()
    dead = ds.num_paths == 0
    assert dead.any() and (six[2][dead] == 0).all() and (six[3][dead] == -1).all() and (six[3][~dead] >= 0).all()


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 1])
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    cbs = [case_codebook([8, 1], 8, 1), case_codebook([8, 1], 4, 2)]
    both = macro.compute_subband_pmi(p, snr_db=95.0, subband_size=4, per_codeword=True)
    reports = macro.compute_csi_report(p, codebooks=cbs, snr_db=95.0, subband_size=4)
    assert isinstance(both, list) and len(both) == 2 and isinstance(reports, list) and len(reports) == 2
    for r, got, rep in zip((a, b), both, reports):
        child = dm.Dataset({k: v.copy() for k, v in r.items()})
        alone = child.compute_subband_pmi(p, snr_db=95.0, subband_size=4, per_codeword=True)
        assert len(got) == 6
        for x, y in zip(got, alone):
            assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))
        rep_alone = child.compute_csi_report(p, codebooks=cbs, snr_db=95.0, subband_size=4)
        assert set(rep.keys()) == set(rep_alone.keys()) == {"rank", "rate", "pmi", "rate_sb", "pmi_sb", "rate_by_rank"}
        for k in rep.keys():
            assert rep[k].shape == rep_alone[k].shape and np.array_equal(rep[k].view(np.int32), rep_alone[k].view(np.int32)), k


@pytest.mark.parametrize("B", RANK_SUBBANDS, ids=[f"B{B}" for B in RANK_SUBBANDS])
@pytest.mark.parametrize("cid", RANK_CASES)
def test_csi_report_selects_the_rank_of_the_largest_rate(cid, B):
    import torch
    import deepmimo_amd as dm
    c = BY_ID[cid]
    rays, ue_rot, H, _, snr, _ = case_inputs(c)
    assert not c["per_user_rot"] and c["bs_fov"] is None and c["ue_fov"] is None and not c["doppler"]     # a plain Dataset call
    n = c["n"]
    snr_db = float(10 * np.log10(snr))
    cbs = {L: case_codebook(c["bs_shape"], RANK_CODEWORDS, L) for L in RANK_LAYERS}
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    per_rank = {L: ds.compute_subband_pmi(_dm_params(c), codebook=cbs[L], snr_db=snr_db, subband_size=B) for L in RANK_LAYERS}
    # codebooks handed over in no particular order: the report sorts by L
    rep = ds.compute_csi_report(_dm_params(c), codebooks=[cbs[3], cbs[1], cbs[4], cbs[2]], snr_db=snr_db, subband_size=B)
    n_sb = len(subband_edges(len(c["selected"]), B))
    want = dict(rank=(np.int32, (n,)), rate=(np.float32, (n,)), pmi=(np.int32, (n,)), rate_sb=(np.float32, (n, n_sb)),
                pmi_sb=(np.int32, (n, n_sb)), rate_by_rank=(np.float32, (n, len(RANK_LAYERS))))
    assert set(rep.keys()) == set(want)
    for k, (dt, sh) in want.items():
        assert isinstance(rep[k], np.ndarray) and rep[k].dtype == dt and rep[k].shape == sh and rep[k].flags.c_contiguous, k
    by_rank = np.stack([per_rank[L][0] for L in RANK_LAYERS], axis=1)
    assert np.array_equal(rep.rate_by_rank.view(np.int32), by_rank.view(np.int32)), "rate_by_rank is not the per-rank calls' rate"
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    first_max = np.asarray(RANK_LAYERS, np.int32)[by_rank.argmax(axis=1)]                 # the smallest L on ties
    assert np.array_equal(rep.rank, np.where(dead, 0, first_max)) and (rep.rank[dead] == 0).all() and dead.any()
    for u in range(n):
        src = per_rank[int(rep.rank[u]) if not dead[u] else RANK_LAYERS[0]]
        for k, t in zip(("rate", "pmi", "rate_sb", "pmi_sb"), src):
            assert np.array_equal(np.atleast_1d(rep[k][u]).view(np.int32), np.atleast_1d(t[u]).view(np.int32)), (u, k)
    assert (rep.rate[dead] == 0).all() and (rep.pmi[dead] == -1).all() and (rep.pmi_sb[dead] == -1).all()
    if B is None:
        assert np.array_equal(rep.rate_sb[:, 0].view(np.int32), rep.rate.view(np.int32)) and np.array_equal(rep.pmi_sb[:, 0], rep.pmi)
    # the reference's best rate of the chosen rank is within the summed tolerances of the reference's best rank
    refs = [subband_reference(H, cbs[L], snr, B) for L in RANK_LAYERS]
    ref_rank, ref_best, ref_tol = reference_ranks(refs, RANK_LAYERS)
    live = np.flatnonzero(~dead)
    assert len(set(rep.rank[live].tolist())) >= 2
    for u in live:
        i = RANK_LAYERS.index(int(rep.rank[u]))
        chosen = refs[i]["rate_c"][u].max()
        tol = np.take(refs[i]["tol_c"][u], refs[i]["rate_c"][u].argmax())
        assert chosen >= ref_best[u] - (tol + ref_tol[u]), (u, int(rep.rank[u]), int(ref_rank[u]), chosen, ref_best[u])
    # torch output mode: the same bits, on the device
    dm.config("channel_output", "torch")
    try:
        rep_t = ds.compute_csi_report(_dm_params(c), codebooks=[cbs[L] for L in RANK_LAYERS], snr_db=snr_db, subband_size=B)
    finally:
        dm.config("channel_output", "numpy")
    for k in want:
        assert isinstance(rep_t[k], torch.Tensor) and rep_t[k].is_cuda and np.array_equal(_bits(rep_t[k]), rep[k].view(np.int32)), k


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol and the worst absolute error over every case that ran (README.md and DESIGN.md
    quote both); nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=lambda i: WORST[i][0])
        ka = max(WORST, key=lambda i: WORST[i][1])
        print(f"subband pmi: worst err / tol over {len(WORST)} cases = {WORST[k][0]:.3f} ({k}); worst |err| = {WORST[ka][1]:.3e} bit ({ka})")
        assert WORST[k][0] <= 1.0
