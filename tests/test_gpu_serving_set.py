"""Serving sets in the cell rate (DMX_FLAG_SERVING_SET, k8_cell_rate<M, true>) on the GPU.

Reference: tests/_serving_set_ref.py - the definition in complex128 slogdet of the NumPy oracle's per-link channels with set
membership in place of `s == b`, entry by entry within the derived tolerance (a member weighted with |A^-1|_F, every other
link with |A^-1 - N^-1|_F); tests/test_serving_set_cpu.py holds every case to the cap condition.  The links of the
kernel-level cases come from the case helpers of tests/test_gpu_cell_rate.py, their SNRs from `link_snrs`; the multi-stream
`compute_mu_rate` cases run on the rays, codebooks and snr_db of tests/_mu_cases.py.  Every case also holds: exactly +0.0
where no link of the user's set reaches it, every value finite and >= 0, |rate - mean(rate_k)| <= K 2^-24 max_k rate_k + 2^-24,
and a second launch torch.equal.  A set of one bit has to give the bits of the launch without the flag.

Worst error / tolerance measured on the MI355X: 0.120 over the kernel-level cases (sets_mixed), 0.135 over the multi-stream
cases (G4_L2, rate_k), 0.006 for stream_snr.  The steps of a GPU visit run under a time limit each in the job that calls
pytest; no test here waits or sleeps."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _entry_calls as E
from tests import _serving_set_ref as SR

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests import test_gpu_cell_rate as g  # noqa: E402
from tests.test_gpu_fd_direct import _dm_params  # noqa: E402

CELLS = SR.set_cells()
BY_ID = {c["id"]: (c, m) for c, m in CELLS}
WORST = {}


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _setup(cid):
    """(engine, cell, masks, member [n, B], preparations, snr_db per link)"""
    cell, masks = BY_ID[cid]
    eng = _engine()
    _, snrs = g.case_inputs(cell)
    return eng, cell, masks, SR.members_of(masks, len(cell["links"])), g.prepare_links(eng, cell), g.snr_dbs(snrs)


def raw_call(eng, preps, db, serving, flagged=True, user_begin=0, user_count=None, outputs=(True, True, True)):
    """dmx_cell_rate itself, `serving` as the int32 array the library reads (None: NULL), the flag on copies of the parameter
    blocks.  Returns (rate, rate_k, out_serving, link_snr), None for an output not asked for."""
    import torch
    from deepmimo_amd import _native as nat
    from deepmimo_amd.engine import link_snrs_from_db
    B, n_ue = len(preps), preps[0].n_ue
    cnt = n_ue - user_begin if user_count is None else user_count
    links = eng._links(preps, link_snrs_from_db(db, B))
    keep = []
    for b, prep in enumerate(preps):
        p = nat.DmxParams.from_buffer_copy(prep.params_struct)
        p.flags |= nat.FLAG_SERVING_SET if flagged else 0
        keep.append(p)
        links[b].prm = C.pointer(p)
    serv = None if serving is None else torch.from_numpy(np.asarray(serving).astype(np.int32)).to(eng.device)
    K = int(preps[0].params_struct.n_selected)
    new = lambda want, shape, dt: torch.empty(shape, dtype=dt, device=eng.device) if want else None    # noqa: E731
    r = new(True, (cnt,), torch.float32)
    rk, sv, ls = new(outputs[0], (cnt, K), torch.float32), new(outputs[1], (cnt,), torch.int32), new(outputs[2], (cnt, B), torch.float32)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                    # noqa: E731
    with torch.cuda.device(eng.device):
        rc = eng.lib.dmx_cell_rate(links, B, n_ue, user_begin, cnt, ptr(serv), ptr(r), ptr(rk), ptr(sv), ptr(ls), eng._stream_ptr())
    nat.check(rc, "dmx_cell_rate")
    return r, rk, sv, ls


def check_properties(r, rk, dead, what):
    """what every launch holds: finite, >= 0, +0.0 where nothing serves, the rate the mean of rate_k"""
    K = rk.shape[1]
    for name, v in (("rate", r), ("rate_k", rk)):
        assert np.isfinite(v).all() and (v >= 0).all(), f"{what}: {name} has a NaN, an inf or a negative value"
    assert (r[dead] == 0).all() and not np.signbit(r[dead]).any(), f"{what}: rate of a user nobody serves is not +0.0"
    assert (rk[dead] == 0).all() and not np.signbit(rk[dead]).any(), f"{what}: rate_k of a user nobody serves is not +0.0"
    mean = rk.astype(np.float64).mean(axis=1)
    assert (np.abs(r - mean) <= K * 2.0 ** -24 * rk.max(axis=1) + 2.0 ** -24).all(), f"{what}: rate is not the mean of rate_k"


def check_sets(out, cell, member, what, again=None):
    """one flagged launch (rate, rate_k, the set as bool [n, B], link_snr) of a cell case against the reference"""
    import torch
    links, snrs = g.case_inputs(cell)
    snrs = [10.0 ** (d / 10.0) for d in g.snr_dbs(snrs)]                   # what the engine was given
    Hs = [l[2] for l in links]
    B, n, K = len(Hs), Hs[0].shape[0], Hs[0].shape[3]
    rate, rate_k, sets, link_snr = out
    assert rate.dtype == torch.float32 and tuple(rate.shape) == (n,) and rate.is_contiguous()
    assert rate_k.dtype == torch.float32 and tuple(rate_k.shape) == (n, K) and rate_k.is_contiguous()
    assert sets.dtype == torch.bool and tuple(sets.shape) == (n, B)
    assert link_snr.dtype == torch.float32 and tuple(link_snr.shape) == (n, B)
    r, rk, ls = rate.cpu().numpy(), rate_k.cpu().numpy(), link_snr.cpu().numpy()
    assert np.array_equal(sets.cpu().numpy(), member), f"{what}: the set read is not the set given"
    ls_ref, ls_tol, live = g.link_snr_refs(cell)
    assert np.isfinite(ls).all() and (np.abs(ls - ls_ref) <= ls_tol).all() and (ls[~live] == 0).all(), f"{what}: link_snr"
    ref, ref_k = SR.set_rate_from_channels(Hs, snrs, member)
    tol, tol_k = SR.set_rate_tolerance(Hs, snrs, member)
    dead = ~SR.live_users(Hs, member)
    assert np.array_equal(dead, ~(member & live).any(axis=1)) and (ref[dead] == 0).all()
    check_properties(r, rk, dead, what)
    ek, e = np.abs(rk - ref_k), np.abs(r - ref)
    ratio = max(float((ek / tol_k).max()), float((e / tol).max()))
    print(f"{what}: {int((~dead).sum())} of {n} users live, worst rate err / tol = {ratio:.3f}, worst |err| = "
          f"{max(float(ek.max()), float(e.max())):.3e} bit, largest rate {float(ref_k.max()):.2f}")
    WORST[what] = ratio
    assert (ek <= tol_k).all(), f"{what}: {(ek > tol_k).sum()} rate_k entries out of tolerance, worst err / tol {ratio:.3f}"
    assert (e <= tol).all(), f"{what}: {(e > tol).sum()} users out of tolerance, worst err / tol {ratio:.3f}"
    if again is not None:
        assert all(torch.equal(a, b) for a, b in zip(again, out)), f"{what}: a second launch differs"


# ---- 1. every case against the reference; the launch residues are four of them ---------------------------------------------------
@pytest.mark.parametrize("cid", list(BY_ID))
def test_sets_against_the_definition(cid):
    import torch
    eng, cell, masks, member, preps, db = _setup(cid)
    n, B = member.shape
    assert eng.cell_rate_supported(preps)
    first = eng.cell_rate(preps, db, serving_set=member, per_subcarrier=True, details=True)
    second = eng.cell_rate(preps, db, serving_set=torch.from_numpy(member.astype(np.uint8)).cuda(), per_subcarrier=True, details=True)
    alone = eng.cell_rate(preps, db, serving_set=member)                    # fewer outputs: the same bits
    pair = eng.cell_rate(preps, db, serving_set=member, details=True)
    full = eng.cell_rate(preps, db, serving_set="all", per_subcarrier=True, details=True)
    full_again = eng.cell_rate(preps, db, serving_set=np.ones((n, B), np.int64), per_subcarrier=True, details=True)
    torch.cuda.synchronize()
    assert torch.equal(alone, first[0])
    assert torch.equal(pair[0], first[0]) and torch.equal(pair[1], first[2]) and torch.equal(pair[2], first[3])
    check_sets(first, cell, member, cid, again=second)
    check_sets(full, cell, np.ones((n, B), bool), f"{cid}_all", again=full_again)
    assert bool((full[0] >= first[0]).all())                                # on the same floats: cooperation never lowers it
    if cid == "sets_counts":                                                # every kept-count pattern met every set
        _, _, live = g.link_snr_refs(cell)
        assert (member & ~live).any() and (member.any(axis=1) & ~(member & live).any(axis=1)).sum() >= 6


# ---- 2. one-bit sets: the bits of the launch without the flag ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["sets3_K65", "sets_mixed", "sets_B8"])
def test_one_bit_sets_equal_the_unflagged_launch(cid):
    import torch
    eng, cell, _, _, preps, db = _setup(cid)
    B, n = len(preps), cell["links"][0]["n"]
    given = [np.full(n, s, np.int64) for s in range(B)] + [np.array([(u % (B + 1)) - 1 for u in range(n)], np.int64)]
    for s in given:
        member = SR.members_of(np.where(s >= 0, 1 << np.clip(s, 0, 30), 0), B)
        want = eng.cell_rate(preps, db, serving=s, per_subcarrier=True, details=True)
        got = eng.cell_rate(preps, db, serving_set=member, per_subcarrier=True, details=True)
        low = raw_call(eng, preps, db, np.where(s >= 0, 1 << np.clip(s, 0, 30), -3))
        torch.cuda.synchronize()
        for a in (got, low):
            assert torch.equal(a[0], want[0]) and torch.equal(a[1], want[1]) and torch.equal(a[3], want[3]), (cid, s[:4])
        assert torch.equal(got[2], torch.from_numpy(member).cuda())
        assert bool((want[0] > 0).any())


# ---- 3. equivalent forms of a set, out_serving ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["sets_mixed", "sets_B8"])
def test_equivalent_forms_of_a_set_and_out_serving(cid):
    import torch
    eng, cell, masks, member, preps, db = _setup(cid)
    n, B = member.shape
    every = (1 << B) - 1
    base = raw_call(eng, preps, db, masks)
    null = raw_call(eng, preps, db, None)
    full = raw_call(eng, preps, db, np.full(n, every))
    high = raw_call(eng, preps, db, masks | np.array([(1 << B, 1 << 30, 0x7FFFFF00, 1 << (B + 3))[u % 4] for u in range(n)]))
    neg = np.array([(-1, -2, -(2 ** 31), -every)[u % 4] for u in range(n)], np.int64)
    nobody = raw_call(eng, preps, db, neg)
    zero = raw_call(eng, preps, db, np.zeros(n, np.int64))
    torch.cuda.synchronize()
    dev = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).cuda()                   # noqa: E731
    assert torch.equal(base[2], dev(masks)) and bool((base[0] > 0).any())
    for a, b in zip(null, full):                                            # NULL: every link serves
        assert torch.equal(a, b)
    assert torch.equal(null[2], dev(np.full(n, every)))
    for a, b in zip(high, base):                                            # bits at or above n_links are ignored, also in out_serving
        assert torch.equal(a, b)
    for a, b in zip(nobody, zero):                                          # a negative entry is the empty set
        assert torch.equal(a, b)
    assert torch.equal(nobody[2], dev(np.zeros(n))) and torch.equal(nobody[3], base[3])
    for t in (nobody[0], nobody[1]):
        assert bool((t == 0).all()) and not bool(torch.signbit(t).any())
    # the engine's form of the same sets
    eng_out = eng.cell_rate(preps, db, serving_set=member, per_subcarrier=True, details=True)
    torch.cuda.synchronize()
    assert torch.equal(eng_out[0], base[0]) and torch.equal(eng_out[1], base[1]) and torch.equal(eng_out[3], base[3])


# ---- 4. launch invariance ----------------------------------------------------------------------------------------------------------
def test_user_sub_range_and_fewer_outputs_write_the_same_bits():
    import torch
    eng, cell, masks, member, preps, db = _setup("sets3_K65")
    n = len(masks)
    whole = raw_call(eng, preps, db, masks)
    b, cnt = 5, 15                                                          # no multiple of the waves of a workgroup
    part = raw_call(eng, preps, db, masks[b:b + cnt], user_begin=b, user_count=cnt)
    part_null = raw_call(eng, preps, db, None, user_begin=b, user_count=cnt)
    whole_null = raw_call(eng, preps, db, None)
    only = raw_call(eng, preps, db, masks, outputs=(False, False, False))
    two = raw_call(eng, preps, db, masks, outputs=(True, False, False))
    none = eng.cell_rate(preps, db, serving_set=member[:0], user_begin=n, user_count=0, per_subcarrier=True, details=True)
    eng_part = eng.cell_rate(preps, db, serving_set=member[b:b + cnt], user_begin=b, user_count=cnt, per_subcarrier=True)
    torch.cuda.synchronize()
    for w, p in zip(whole + whole_null, part + part_null):
        assert torch.equal(p, w[b:b + cnt])
    assert torch.equal(only[0], whole[0]) and only[1] is None and torch.equal(two[0], whole[0]) and torch.equal(two[1], whole[1])
    assert [tuple(t.shape) for t in none] == [(0,), (0, 65), (0, 3), (0, 3)] and none[2].dtype == torch.bool
    assert torch.equal(eng_part[0], whole[0][b:b + cnt]) and torch.equal(eng_part[1], whole[1][b:b + cnt])


def test_refusals_of_the_engine():
    eng, cell, masks, member, preps, db = _setup("sets3_K1")
    for bad in ("some", member[:, :2], member[:-1], member.astype(np.float32)):
        with pytest.raises(ValueError, match="serving_set"):
            eng.cell_rate(preps, db, serving_set=bad)
    with pytest.raises(ValueError, match="serving_set"):
        eng.cell_rate(preps, db, serving=0, serving_set=member)
    with pytest.raises(ValueError, match="serving"):                        # `serving` keeps its own
        eng.cell_rate(preps, db, serving=np.zeros(3, np.int32))


# ---- 5. MacroDataset ---------------------------------------------------------------------------------------------------------------
def test_macro_dataset_serving_set_and_all_against_the_reference():
    import torch
    import deepmimo_amd as dm
    eng, cell, masks, member, preps, db = _setup("sets_mixed")
    n, B = member.shape
    links, _ = g.case_inputs(cell)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in l[0].items()}) for l in links])
    plist = [_dm_params(c) for c in cell["links"]]
    want = eng.cell_rate(preps, db, serving_set=member, per_subcarrier=True, details=True)
    got = macro.compute_cell_rate(plist, snr_db=db, serving_set=member, per_subcarrier=True, details=True)
    every = macro.compute_cell_rate(plist, snr_db=db, serving_set="all", per_subcarrier=True, details=True)
    only = macro.compute_cell_rate(plist, snr_db=db, serving_set=member.astype(np.int8))
    dm.config("channel_output", "torch")
    try:
        got_t = macro.compute_cell_rate(plist, snr_db=db, serving_set=torch.from_numpy(member).cuda(), per_subcarrier=True, details=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(got, tuple) and len(got) == 4 and all(isinstance(a, np.ndarray) for a in got)
    assert [a.dtype for a in got] == [np.float32, np.float32, np.bool_, np.float32]
    assert [a.shape for a in got] == [(n,), (n, 3), (n, B), (n, B)]
    assert isinstance(only, np.ndarray) and only.tobytes() == got[0].tobytes()
    for a, t, w in zip(got, got_t, want):
        assert isinstance(t, torch.Tensor) and t.is_cuda and torch.equal(t, w) and a.tobytes() == w.cpu().numpy().tobytes()
    check_sets(tuple(torch.from_numpy(a).cuda() for a in got), cell, member, "macro_sets_mixed")
    check_sets(tuple(torch.from_numpy(a).cuda() for a in every), cell, np.ones((n, B), bool), "macro_sets_mixed_all")
    # clusters from link_snr: the strongest link alone is the automatic serving index, larger clusters run and never lower the rate
    auto = macro.compute_cell_rate(plist, snr_db=db, details=True)
    one = dm.serving_clusters(auto[2], 1)
    assert np.array_equal(np.where(one.any(axis=1), one.argmax(axis=1), -1), auto[1])
    assert macro.compute_cell_rate(plist, snr_db=db, serving_set=one).tobytes() == auto[0].tobytes()
    pairs = dm.serving_clusters(auto[2], 2, within_db=20.0)
    two = macro.compute_cell_rate(plist, snr_db=db, serving_set=pairs, per_subcarrier=True, details=True)
    check_sets(tuple(torch.from_numpy(a).cuda() for a in two), cell, pairs, "macro_sets_mixed_clusters")
    assert (pairs.sum(axis=1) == 2).any() and (two[0] >= auto[0]).all()


# ---- 6. several streams per user in compute_mu_rate ------------------------------------------------------------------------------
def _mu_dataset(rays, place):
    import torch
    import deepmimo_amd as dm
    put = (lambda v: torch.from_numpy(v.copy()).cuda()) if place == "hbm" else (lambda v: v.copy())
    return dm.Dataset({k: put(v) for k, v in rays.items()})


@pytest.mark.parametrize("name", list(SR.MU_SET_CASES))
def test_multi_stream_mu_rate_matches_the_definition(name):
    from tests import _mu_cases as CS
    from tests import _mu_ref as MR
    from tests.test_gpu_parity import _dm_params as mu_params
    case, op, rays, F, beams, groups, snr_db, place = SR.mu_set_setup(name)
    ref = SR.mu_set_reference(rays, op, F, beams, groups, snr_db)
    n, L = beams.shape
    G, K = groups.shape[1], len(case["selected"])
    ds, p = _mu_dataset(rays, place), mu_params(case, CS.UE_ROT)
    rate, rate_k, partners, stream = ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db, per_subcarrier=True, details=True)
    assert rate.shape == (n,) and rate_k.shape == (n, K) and partners.shape == (n, G - 1) and stream.shape == (n, G * L)
    assert rate.dtype == rate_k.dtype == stream.dtype == np.float32 and partners.dtype == np.int32
    check_properties(rate, rate_k, ~ref["live"], name)
    assert MR.worst(rate, ref["rate"], ref["tol"], what=f"{name}: rate") <= 1.0
    assert MR.worst(rate_k, ref["rate_k"], ref["tol_k"], what=f"{name}: rate_k") <= 1.0
    assert np.array_equal(partners, ref["partners"])
    assert MR.worst(stream, ref["stream_snr"], ref["stream_tol"], what=f"{name}: stream_snr") <= 1.0
    idle = ~ref["member"].any(axis=1)
    assert idle.any() and np.all(stream[idle] == 0) and rate[CS.NO_PATH_USER] == 0 and rate[ref["live"]].max() > 0.05
    short = (beams[:, -1] < 0) & ~idle
    assert short.any() and np.all(stream[short, L - 1] == 0)                 # a padded stream is a link nobody transmits on
    # the rate alone, and a second call: the same bits
    assert ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db).tobytes() == rate.tobytes()
    again = ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db, per_subcarrier=True)
    assert again[0].tobytes() == rate.tobytes() and again[1].tobytes() == rate_k.tobytes()


@pytest.mark.parametrize("name", ["G2_ue2x1_K64_P25_snr30", "G8_ue4x2_K130_P25_snr10"])
def test_one_column_of_beams_gives_the_bits_of_the_vector(name):
    from tests import _mu_cases as CS
    from tests.test_gpu_parity import _dm_params as mu_params
    case, op, rays, F, beams, groups, snr_db, place = CS.mu_setup(name)
    ds, p = _mu_dataset(rays, place), mu_params(case, CS.UE_ROT)
    want = ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db, per_subcarrier=True, details=True)
    got = ds.compute_mu_rate(F, beams[:, None], groups, p, snr_db=snr_db, per_subcarrier=True, details=True)
    assert len(got) == len(want) == 4 and (want[0] > 0).any()
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 7. a side stream and a captured graph -----------------------------------------------------------------------------------------
def _flagged_case():
    """the two links of tests/_entry_calls.py's cell-rate case, called with a set per user: users in turn served by nobody,
    link 0, link 1 and both.  The sets are a device constant of the case."""
    links = [E.fd_case([4, 2], E.CONSUMER_UE, E.CONSUMER_SEL), E.fd_case([2, 2], E.CONSUMER_UE, E.CONSUMER_SEL, bs_rot=(0, 0, -120))]
    member = SR.members_of(np.arange(E.N_UE) % 4, 2)
    return E._built([E._prep(cd) for cd in links], lambda eng, rays, preps: dict(sets=E._dev(eng, member)),
                    lambda eng, rays, preps, outs: tuple(eng.cell_rate(preps, [E.SNR_DB, E.SNR_DB - 6.0], serving_set=outs["sets"],
                                                                       per_subcarrier=True, details=True)),
                    ("consumer", "cell_rate"))


def test_flagged_call_on_a_side_stream_and_in_a_captured_graph():
    import torch
    eng = _engine()
    built = _flagged_case()
    rays, b_dev = E.upload(eng, built, "a"), E.upload(eng, built, "b")
    preps = E.prepare_all(eng, built, rays)
    outs = built["state"](eng, rays, preps)
    want = {w: E.fresh_run(eng, built, w) for w in ("a", "b")}
    assert any(not E.same_bits(x, y) for x, y in zip(want["a"], want["b"]))
    assert bool((want["a"][0] > 0).any()) and bool((want["a"][0][::4] == 0).all())

    def sequence():
        for p in preps:
            eng.reprepare(p)
        return built["call"](eng, rays, preps, outs)

    def same(got, which, what):
        got = E.observed(got, preps)
        assert len(got) == len(want[which])
        for i, (x, y) in enumerate(zip(got, want[which])):
            assert E.same_bits(x, y), f"{what}: tensor {i} differs"

    warm = sequence()
    torch.cuda.synchronize()
    same(warm, "a", "eager warm-up")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        E.copy_rays(rays, b_dev)
        on_side = sequence()
    side.synchronize()
    same(on_side, "b", "on a side stream")
    E.copy_rays(rays, E.upload(eng, built, "a"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = sequence()
    graph.replay()
    torch.cuda.synchronize()
    same(result, "a", "replay on the rays of the capture")
    E.copy_rays(rays, b_dev)
    graph.replay()
    torch.cuda.synchronize()
    same(result, "b", "replay on new rays in the same tensors")


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol over every check that ran; nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f"serving sets: worst rate err / tol over {len(WORST)} checks = {WORST[k]:.3f} ({k})")
        assert WORST[k] <= 1.0
