"""The one-wave-per-user consumers (k6 .. k10) at the shapes of tests/_consumer_shapes.py, on the GPU: what the parametrised
`test_*_against_the_definition` tests, which take those cases through their tables, do not already give.

* every kept-path count 0 .. 32 on every consumer from ONE preparation, each output held to the checker of its own test
  module (no criterion is restated here), the user without a path exactly +0.0 everywhere, a second launch torch.equal;
* a user sub-range on the odd shapes [3,3] / [5,1] and [5,3] / [3,2] (M_big = 9 and 15: the lone last t, the scalar store)
  into `out=` views with sentinel guard regions - the rows of the whole launch bit for bit, the guards untouched;
* n_layers = 1 .. m at m = 3 and m = 5 in both orientations: the leading layers of n_layers = m bit for bit;
* the table of k8's one-link test holds every new UE-small shape.
tests/test_consumer_shapes_cpu.py holds the conditions on these inputs (ledger, shares, sensitivity).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _angle_delay_cases as adc
from tests import _consumer_shapes as S
from tests._cell_rate_ref import link_snrs
from tests._codebook_rate_ref import case_codebook
from tests._subband_pmi_ref import subband_edges, subband_reference

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests import test_gpu_angle_delay as gad  # noqa: E402
from tests import test_gpu_cell_rate as gcell  # noqa: E402
from tests import test_gpu_codebook_rate as gcb  # noqa: E402
from tests import test_gpu_covariance as gcov  # noqa: E402
from tests import test_gpu_precoders as gp  # noqa: E402
from tests import test_gpu_rate as gr  # noqa: E402
from tests import test_gpu_spectrum as gs  # noqa: E402
from tests import test_gpu_subband_pmi as gsb  # noqa: E402
from tests.test_gpu_fd_direct import _dm_params, _kwargs, _oracle  # noqa: E402

GUARD = 1 << 16
BY_ID = {c["id"]: c for c in S.RATE_CASES}


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _prepare(eng, c):
    rays, ue_rot, H, snr = gr.case_inputs(c)
    p = _dm_params(c).validate(c["n"])
    return eng.prepare(eng.upload_rays(rays), p, want_side="light", **_kwargs(c, ue_rot)), H, snr


def _db(snr):
    return float(10 * np.log10(snr))


def test_every_kept_count_on_every_consumer_from_one_prepare():
    """user u keeps exactly u % 33 of 32 loaded paths: rows_pair's path loop (unrolled by two) and k6's triangle of n paths
    at every n, odd and even"""
    import torch
    c = S.EVERY_COUNT
    eng = _engine()
    prep, H, snr20 = _prepare(eng, c)
    rays, ue_rot = gr.case_inputs(c)[:2]
    n, what = c["n"], "every_count (one prepare)"
    kept = np.isfinite(rays["power"]).sum(axis=1)
    assert kept.tolist() == [u % 33 for u in range(n)]
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    assert dead.tolist() == [k == 0 for k in kept.tolist()] and dead[0] and dead[33]
    db20, snr10 = _db(snr20), gs.case_snr(H)
    db10 = _db(snr10)
    zero_rows = []                                                            # every output's row of user 0

    # k7: the three epilogues
    rate = eng.rate(prep, db20, per_subcarrier=True)
    gr.check_rate(rate[0], rate[1], H, 10.0 ** (db20 / 10.0), what, again=eng.rate(prep, db20, per_subcarrier=True))
    zero_rows += [rate[0][:1], rate[1][:1]]
    kw = dict(gamma=True, rate=True, per_subcarrier=True)
    spec = eng.spectrum(prep, db10, **kw)
    assert all(torch.equal(a, b) for a, b in zip(spec, eng.spectrum(prep, db10, **kw))), "spectrum: a second launch differs"
    gs.check_spectrum(*spec, H, 10.0 ** (db10 / 10.0), what, equal_rate_k=eng.rate(prep, db10, per_subcarrier=True)[1])
    zero_rows += [t[:1] for t in spec]
    pre = eng.precoders(prep, db10, n_layers=2)
    assert all(torch.equal(a, b) for a, b in zip(pre, eng.precoders(prep, db10, n_layers=2))), "precoders: a second launch differs"
    gp.check_precoders(*pre, H, 10.0 ** (db10 / 10.0), what, 2)
    zero_rows += [t[:1] for t in pre]

    # k6, both sides
    R = [eng.covariance(prep, side=s) for s in gcov.SIDES]
    gcov.check_covariance(R[0], R[1], H, what, again=[eng.covariance(prep, side=s) for s in gcov.SIDES])
    zero_rows += [t[:1] for t in R]

    # k8: one link is k7's rate bit for bit; the same link twice is a serving link under its own copy as the interferer
    H_td = _oracle(dict(c, freq_domain=0), rays, ue_rot)["channel"]
    for B in (1, 2):
        cell = gcell._cell(f"every_count_x{B}", [c] * B)
        snrs = link_snrs([H] * B, cell["serving_db"], cell["inr_db"])
        gcell.set_case_inputs(cell, [(rays, ue_rot, H, H_td)] * B, snrs)     # the checker's inputs: this preparation's
        dbs = gcell.snr_dbs(snrs)
        out = eng.cell_rate([prep] * B, dbs, per_subcarrier=True, details=True)
        again = eng.cell_rate([prep] * B, dbs, per_subcarrier=True, details=True)
        torch.cuda.synchronize()
        gcell.check_cell(out, cell, f"{what} B = {B}", again=again)
        assert bool((out[2][~torch.from_numpy(dead).cuda()] == 0).all()) and bool((out[2][torch.from_numpy(dead).cuda()] == -1).all())
        if B == 1:
            assert snrs[0] == snr20 and torch.equal(out[0], rate[0]) and torch.equal(out[1], rate[1]), "one link is not k7's rate"
        zero_rows += [out[0][:1], out[1][:1], out[3][:1]]
        assert int(out[2][0]) == -1

    # k9, antenna rows
    ad = adc.BY_ID[S.ANGLE_DELAY_EVERY_COUNT]
    X_ref = adc.case_inputs(ad)[3]
    X = eng.angle_delay(prep, ad["n_taps"], n_fft=ad["n_fft"])
    gad.check_adp(X, X_ref, what, again=eng.angle_delay(prep, ad["n_taps"], n_fft=ad["n_fft"]))
    zero_rows.append(X[:1])

    # k10, wideband and per subband
    cbc = next(x for x in S.CODEBOOK_CASES if x["rays"] == "every_count")
    _, _, Hc, W, snr_c, ref = gcb.case_inputs(cbc)
    assert np.array_equal(Hc, H)
    dbc = _db(snr_c)
    first = eng.codebook_rate(prep, W, dbc, per_codeword=True)
    gcb.check_result(*first, H, ref, what, again=eng.codebook_rate(prep, W, dbc, per_codeword=True), alone=eng.codebook_rate(prep, W, dbc))
    zero_rows += [first[0][:1], first[2][:1]]
    assert int(first[1][0]) == -1
    Bsb = S.ML_SUBBAND
    six = eng.codebook_rate_subbands(prep, W, dbc, Bsb, per_codeword=True)
    assert all(torch.equal(a, b) for a, b in zip(six, eng.codebook_rate_subbands(prep, W, dbc, Bsb, per_codeword=True)))
    r, p, rsb, psb, rc, rsbc = (t.cpu().numpy() for t in six)
    sref = subband_reference(H, W, 10.0 ** (dbc / 10.0), Bsb)
    n_sb = len(subband_edges(len(c["selected"]), Bsb))
    gsb.check_trio(r, p, rc, dead, f"{what} wideband")
    gsb.check_against_reference(p, rc, sref["rate_c"], sref["tol_c"], dead, f"{what} wideband")
    for s in range(n_sb):
        gsb.check_trio(rsb[:, s], psb[:, s], rsbc[:, s], dead, f"{what} subband {s}")
    flat = lambda x: np.ascontiguousarray(x).reshape(n * n_sb, -1)           # noqa: E731
    gsb.check_against_reference(flat(psb)[:, 0], flat(rsbc), flat(sref["rate_sb_c"]), flat(sref["tol_sb_c"]), np.repeat(dead, n_sb),
                                f"{what} subbands")
    zero_rows += [six[0][:1], six[2][:1], six[4][:1], six[5][:1]]
    assert int(six[1][0]) == -1 and bool((six[3][0] == -1).all())

    torch.cuda.synchronize()
    assert len(zero_rows) == 23
    for t in zero_rows:                                                       # user 0 keeps no path: +0.0 in every float output
        v = (torch.view_as_real(t) if t.is_complex() else t).cpu().numpy()
        assert v.size > 0 and (v == 0).all() and not np.signbit(v).any()


def _guarded(full):
    """(buffers, views) for the outputs `full`: each view sits between two sentinel-filled guard regions"""
    import torch
    bufs, views = [], []
    for f in full:
        sentinel = complex(-12345.5, 54321.25) if f.is_complex() else (-12345.5 if f.is_floating_point() else -12345)
        b = torch.full((GUARD + f.numel() + GUARD,), sentinel, dtype=f.dtype, device=f.device)
        bufs.append((b, sentinel, f.numel()))
        views.append(b[GUARD:GUARD + f.numel()].view(f.shape))
    return bufs, views


def _guards_untouched(bufs):
    return all(bool((b[:GUARD] == s).all()) and bool((b[GUARD + n:] == s).all()) for b, s, n in bufs)


def _check_sub_range(launch, full, b0, cnt, what):
    """launch(user_begin, user_count, outs) writes into guarded views: the whole launch, then users b0 .. b0 + cnt"""
    import torch
    bufs, views = _guarded(full)
    launch(0, full[0].shape[0], views)
    torch.cuda.synchronize()
    assert _guards_untouched(bufs), f"{what}: write outside the output tensors"
    assert all(torch.equal(v, f) for v, f in zip(views, full)), f"{what}: the launch into views differs"
    for b, s, _ in bufs:
        b.fill_(s)
    launch(b0, cnt, [v[b0:b0 + cnt] for v in views])
    torch.cuda.synchronize()
    assert _guards_untouched(bufs), f"{what}: write outside the output tensors"
    for (_, s, _), v, f in zip(bufs, views, full):
        assert bool((v[:b0] == s).all()) and bool((v[b0 + cnt:] == s).all()), f"{what}: rows outside the range written"
        assert torch.equal(v[b0:b0 + cnt], f[b0:b0 + cnt]), f"{what}: the sub-range is not the rows of the whole launch"


def _codebook_into(eng, prep, W, snr_db, b0, cnt, outs):
    """dmx_codebook_rate into the given tensors.  ChannelEngine.codebook_rate has no `out=`, so this restates the body of
    that method for one user block through the engine's private helpers (_codebook_on_device, _record_args, _scratch,
    _stream_ptr): whoever changes the C call or those helpers in deepmimo_amd/engine.py has to change this with them."""
    import torch
    from deepmimo_amd import _native as nat
    from deepmimo_amd.engine import _ptr, snr_linear_from_db
    cb, n_cw, n_layers = eng._codebook_on_device(prep, W)
    with torch.cuda.device(eng.device):
        nbytes = int(eng.lib.dmx_beam_workspace_bytes(C.byref(prep.params_struct), cnt, prep.n_paths_loaded, n_cw * n_layers))
        bws = eng._scratch(nbytes)
        rc = eng.lib.dmx_codebook_rate(*eng._record_args(prep, b0, cnt), _ptr(cb), n_cw, n_layers, _ptr(bws), nbytes,
                                       snr_linear_from_db(snr_db), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), eng._stream_ptr())
    nat.check(rc, "dmx_codebook_rate")


@pytest.mark.parametrize("cid", ["m5_ue_K1", "m6_ue_K3"])
def test_user_sub_range_on_an_odd_shape_with_guard_regions(cid):
    """users 5 .. 19 of 33 (no multiple of the waves of a workgroup): an odd-M_big tail that stores one element too many, or
    a scalar store path that strays, lands in a neighbour's row or in a guard"""
    c = BY_ID[cid]
    m, _, _, M_big, _ = S.gram_order(c["bs_shape"], c["ue_shape"])
    assert c["n"] == 33 and M_big % 2 == 1 and not S.vec16(M_big) and (cid, M_big) in (("m5_ue_K1", 9), ("m6_ue_K3", 15))
    eng = _engine()
    prep, H, _ = _prepare(eng, c)
    db = _db(gs.case_snr(H))
    b0, cnt = 5, 15
    full = eng.precoders(prep, db, n_layers=m)
    assert tuple(full[1].shape) == (33, len(c["selected"]), m, M_big) and tuple(full[2].shape) == (33, len(c["selected"]), m, m)
    _check_sub_range(lambda b, k, o: eng.precoders(prep, db, n_layers=m, user_begin=b, user_count=k, out=tuple(o)), full, b0, cnt,
                     f"{cid} precoders")
    kw = dict(gamma=True, rate=True, per_subcarrier=True)
    _check_sub_range(lambda b, k, o: eng.spectrum(prep, db, user_begin=b, user_count=k, out=tuple(o), **kw), eng.spectrum(prep, db, **kw),
                     b0, cnt, f"{cid} spectrum")
    for side in gcov.SIDES:
        _check_sub_range(lambda b, k, o: eng.covariance(prep, side=side, user_begin=b, user_count=k, out=o[0]),
                         [eng.covariance(prep, side=side)], b0, cnt, f"{cid} covariance {side}")
    W = case_codebook(c["bs_shape"], S.ML_CODEWORDS, 3)
    _check_sub_range(lambda b, k, o: _codebook_into(eng, prep, W, db, b, k, o), list(eng.codebook_rate(prep, W, db, per_codeword=True)),
                     b0, cnt, f"{cid} codebook rate")


@pytest.mark.parametrize("cid", ["m3_ue_K1", "m3_bs_K3", "m5_ue_K70", "m5_bs_K3"])
def test_leading_layers_at_odd_order(cid):
    """n_layers = 1 .. m: gamma and the leading layers of n_layers = m, bit for bit, in both orientations"""
    import torch
    c = BY_ID[cid]
    m = S.gram_order(c["bs_shape"], c["ue_shape"])[0]
    assert m in (3, 5)
    eng = _engine()
    prep, H, _ = _prepare(eng, c)
    db = _db(gs.case_snr(H))
    full = eng.precoders(prep, db, n_layers=m)
    assert eng.precoder_supported(prep, m) and not eng.precoder_supported(prep, m + 1)
    for L in range(1, m + 1):
        ga, wt, wr = eng.precoders(prep, db, n_layers=L)
        torch.cuda.synchronize()
        assert tuple(wt.shape[2:]) == (L, H.shape[2]) and tuple(wr.shape[2:]) == (L, H.shape[1])
        assert torch.equal(ga, full[0]) and torch.equal(wt, full[1][:, :, :L]) and torch.equal(wr, full[2][:, :, :L]), \
            f"{cid}: n_layers = {L} is not the leading layers of n_layers = {m}"


def test_the_one_link_test_of_k8_holds_every_new_ue_small_shape():
    """tests/test_gpu_cell_rate.py `test_one_link_is_the_single_link_rate_bit_for_bit` runs on the cells whose link 0 has the
    UE as the smaller array: the new orders are among them, each with the shape tests/test_gpu_rate.py runs"""
    taken = {c["id"]: c for c in gcell.CASES if gcell._rx_small(c)}
    for m, cid in S.ONE_LINK_CELLS.items():
        link = taken[cid]["links"][0]
        assert (link["bs_shape"], link["ue_shape"]) == (list(S.UE_SMALL[m][0]), list(S.UE_SMALL[m][1]))
        assert any(r["bs_shape"] == link["bs_shape"] and r["ue_shape"] == link["ue_shape"] for r in gr.CASES)
        assert S.gram_order(link["bs_shape"], link["ue_shape"])[:2] == (m, 1)
