"""Multi-cell downlink rate under inter-cell interference (dmx_cell_rate, k8_cell_rate.hip) on the GPU.

Reference: the definition, slogdet in complex128 of the NumPy oracle's per-link channel tensors (tests/_cell_rate_ref.py;
tests/test_cell_rate_cpu.py pins it against hand cases).  Criterion per entry: |rate_k - ref| <= tol_k, |rate - ref| <= tol[u]
and |link_snr - ref| <= tol with the derived tolerances of tests/_cell_rate_ref.py; the rate reference is evaluated with the
serving index the kernel reported.  The per-link SNRs of a case come from its reference alone: link 0 puts its median live
user at the case's serving level (20 dB unless stated), every other link at the case's INR.  Every case also holds: exactly
+0.0 where the user is not served or the serving link does not reach it, every value finite and >= 0,
|rate - float64 mean(rate_k)| <= K 2^-24 max_k rate_k + 2^-24, the automatic serving index equal to the first argmax of the
kernel's own link_snr with the reference link_snr of the chosen link within twice its tolerance of the reference maximum,
and a second launch torch.equal.  Inputs come from `_case`, `_rays` and `_oracle` of tests/test_gpu_fd_direct.py, with a
different ray seed per link.
"""
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests._cell_rate_ref import cell_rate_from_channels, cell_rate_tolerance, link_snr_reference, link_snrs

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle, _rays, _ue_rot  # noqa: E402

WORST = {}                                   # case id -> (worst rate err / tol, worst link_snr err / tol, worst |err| in bit)
IRREGULAR = [-3, 0, 5, 511, 512, 700, -1000, 77, 2 ** 31 - 1, -(2 ** 31), 40001]
LDS_MAX = 156 * 1024


def cell_lds_rule(links):
    """Waves per workgroup of the launcher, restated (0: not taken): one wave holds the tables of the LARGEST link,
    max_b (M_rx + M_tx_b + kc) * P_b * 8 bytes; 4 / 2 / 1 waves while 4 x / 2 x fit 64 KB / one fits 156 KB."""
    most = 0
    for c in links:
        m_tx, m_rx = c["bs_shape"][0] * c["bs_shape"][1], c["ue_shape"][0] * c["ue_shape"][1]
        P, K = min(c["num_paths"], c["L"]), len(c["selected"])
        if not (1 <= P <= 32) or K < 1 or m_rx > 8:
            return 0
        most = max(most, (m_rx + m_tx + min(K, 64)) * P * 8)
    return 4 if 4 * most <= 65536 else 2 if 2 * most <= 65536 else 1 if most <= LDS_MAX else 0


def _cell(cid, links, serving_db=20.0, inr_db=10.0):
    links = [dict(c, id=f"{cid}_b{b}", selected=list(c["selected"]), adaptive=c.get("adaptive", False)) for b, c in enumerate(links)]
    return dict(id=cid, links=links, serving_db=serving_db, inr_db=inr_db)


def _cells():
    cs = []
    cs.append(_cell("defaults", [_case("", 70, 25, [8, 1], [1, 1], 512, [0])] * 3))           # DeepMIMO's defaults, K = 1
    for K in (63, 64, 65):                                                  # one below, at and above a chunk
        cs.append(_cell(f"K{K}", [_case("", 40, 25, [8, 1], [1, 1], 512, range(3, 3 + K))] * 2))
    cs.append(_cell("irregular", [_case("", 33, 25, [4, 2], [2, 1], 512, IRREGULAR)] * 2))
    cs.append(_cell("panel", [_case("", 23, 25, [8, 8], [2, 2], 512, range(0, 512, 7))] * 3))
    # a 4 x 2 UE: at a serving median of 20 dB 6 % of the entries have a tolerance above 1 % of the rate, at 10 dB none
    cs.append(_cell("m8", [_case("", 21, 25, [8, 4], [4, 2], 512, [0, 17, 100])] * 2, serving_db=10.0))
    cs.append(_cell("bs_smaller", [_case("", 29, 25, [2, 1], [4, 2], 512, [0, 9, 100])] * 3, serving_db=10.0, inr_db=0.0))
    # the LDS slice is sized by the largest link ((2 + 64 + 3) * 25), and S = 16, 8, 16
    cs.append(_cell("mixed_links", [_case("", 31, 25, [8, 8], [2, 1], 512, [0, 17, 100]),
                                    _case("", 31, 10, [4, 2], [2, 1], 512, [0, 17, 100]),
                                    _case("", 31, 32, [16, 1], [2, 1], 512, [0, 17, 100])]))
    cs.append(_cell("B8", [_case("", 19, 25, [4, 2], [2, 1], 512, range(3, 68))] * 8, inr_db=0.0))
    cs.append(_cell("counts_and_holes", [_case("", 48, 25, [4, 2], [2, 1], 512, [0, 3, 200], rays="counts")] * 3))
    # launch residue: 4k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 1-wave shape
    for n in (41, 42, 43):
        cs.append(_cell(f"wpb4_users{n}", [_case("", n, 25, [8, 1], [1, 1], 512, [0, 5])] * 2))
    cs.append(_cell("wpb1_users7", [_case("", 7, 25, [16, 16], [2, 2], 512, range(64))] * 2))
    # stage-1 features on one link only: they arrive through that link's records
    cs.append(_cell("feat_rot_fov_dipole", [
        _case("", 53, 25, [4, 2], [1, 1], 512, [0, 1, 2]),
        _case("", 53, 25, [4, 2], [1, 1], 512, [0, 1, 2], bs_rot=[5, -20, 60], ue_rot=[10, 20, 30], bs_fov=[150, 110],
              ue_fov=[200, 100], bs_pattern="halfwave-dipole", ue_pattern="halfwave-dipole")]))
    cs.append(_cell("feat_per_user_rot_doppler", [
        _case("", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], per_user_rot=True),
        _case("", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], doppler=1)]))
    cs.append(_cell("feat_adaptive", [
        _case("", 61, 25, [8, 4], [2, 1], 512, range(0, 64, 3)),
        _case("", 61, 25, [8, 4], [2, 1], 512, range(0, 64, 3), adaptive=True)]))
    return cs


# and M_rx = 3, 5, 6, 7, links of odd and even M_tx in one launch (tests/_consumer_shapes.py)
CASES = _cells() + shapes.CELL_CASES
BY_ID = {c["id"]: c for c in CASES}
_INPUTS = {}


def _counts(u, b, L):
    """kept paths of user u on link b in the `counts` rays: users without a path on every link, on link 0 only, on link 1
    only, and short, full and holed rows"""
    return ((0, 0, 0), (0, L, 2), (L, 0, L - 1), (1, 1, 1), (L, L, L), (L - 1, 2, L))[u % 6][b % 3]


def link_rays(c, b):
    """the rays of link b of a cell case: `_rays` of tests/test_gpu_fd_direct.py for link 0, the same generator with another
    seed for the others"""
    from oracle import oracle_np as onp
    if b == 0 and c["rays"] == "plain":
        return _rays(c)
    rays = onp.synth_rays(c["n"], c["L"], seed=500 + c["n"] + c["L"] + 1000 * b, all_valid=c["all_valid"] or c["rays"] != "plain",
                          max_delay=c["max_delay"], with_doppler=c["doppler"] is not None)
    keys = [k for k in rays if k not in ("rx_pos", "tx_pos")]
    if c["rays"] == "counts":
        rng = np.random.default_rng(4 + b)
        for u in range(c["n"]):
            cnt = _counts(u, b, c["L"])
            hole = np.zeros(c["L"], bool)
            hole[cnt:] = True
            if u % 6 == 4:                                            # NaN holes in the middle of a full row
                hole[rng.choice(c["L"], size=3, replace=False)] = True
            for k in keys:
                rays[k][u, hole] = np.nan
    if c["rays"] == "dead":                                           # a link that reaches nobody
        for k in keys:
            rays[k][:] = np.nan
    return rays


def case_inputs(cell):
    """per link (rays, ue_rot, H of the oracle, time-domain tensor of the oracle) and the per-link SNRs of a cell case:
    computed once, shared and left unchanged"""
    if cell["id"] not in _INPUTS:
        links = []
        for b, c in enumerate(cell["links"]):
            rays, ue_rot = link_rays(c, b), _ue_rot(c)
            H = _oracle(c, rays, ue_rot)["channel"]
            H_td = _oracle(dict(c, freq_domain=0), rays, ue_rot)["channel"]
            H.setflags(write=False)
            H_td.setflags(write=False)
            assert c["max_delay"] < c["subcarriers"] / c["bandwidth"]      # no path is clipped: the link_snr reference holds
            links.append((rays, ue_rot, H, H_td))
        snrs = link_snrs([l[2] for l in links], cell["serving_db"], cell["inr_db"])
        _INPUTS[cell["id"]] = (links, snrs)
    return _INPUTS[cell["id"]]


def set_case_inputs(cell, links, snrs):
    """The inputs of a cell case whose links were built elsewhere (tests/test_gpu_consumer_shapes.py: one preparation as
    every link): per link (rays, ue_rot, H, time-domain tensor) as `case_inputs` returns them, and the per-link SNRs.
    `check_cell` and `link_snr_refs` then hold a launch of that cell to these."""
    assert len(links) == len(cell["links"]) == len(snrs) and all(len(l) == 4 for l in links)
    _INPUTS[cell["id"]] = (list(links), list(snrs))


def link_snr_refs(cell):
    """(ref [n, B], tol [n, B], live [n, B]) of a cell case's link_snr"""
    links, snrs = case_inputs(cell)
    pairs = [link_snr_reference(l[3], snr, c["subcarriers"]) for l, snr, c in zip(links, snrs, cell["links"])]
    live = np.stack([np.abs(l[2]).reshape(l[2].shape[0], -1).max(axis=1) > 0 for l in links], axis=1)
    return np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1), live


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def snr_dbs(snrs):
    return [float(10 * np.log10(s)) for s in snrs]


def prepare_links(eng, cell):
    links, _ = case_inputs(cell)
    preps = []
    for c, (rays, ue_rot, _, _) in zip(cell["links"], links):
        p = _dm_params(c).validate(c["n"])
        preps.append(eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot)))
    return preps


def check_cell(out, cell, what, given=None, again=None):
    """The criteria and the structural properties of one launch (rate, rate_k, serving, link_snr) of a cell case"""
    import torch
    links, snrs = case_inputs(cell)
    snrs = [10.0 ** (d / 10.0) for d in snr_dbs(snrs)]                     # what the engine was given
    Hs = [l[2] for l in links]
    B, n, K = len(Hs), Hs[0].shape[0], Hs[0].shape[3]
    rate, rate_k, serving, link_snr = out
    assert rate.dtype == torch.float32 and tuple(rate.shape) == (n,) and rate.is_contiguous()
    assert rate_k.dtype == torch.float32 and tuple(rate_k.shape) == (n, K) and rate_k.is_contiguous()
    assert serving.dtype == torch.int32 and tuple(serving.shape) == (n,)
    assert link_snr.dtype == torch.float32 and tuple(link_snr.shape) == (n, B) and link_snr.is_contiguous()
    r, rk, s, ls = rate.cpu().numpy(), rate_k.cpu().numpy(), serving.cpu().numpy(), link_snr.cpu().numpy()
    for name, v in (("rate", r), ("rate_k", rk), ("link_snr", ls)):
        assert np.isfinite(v).all() and (v >= 0).all(), f"{what}: {name} has a NaN, an inf or a negative value"
    # link_snr against the time-domain tensors
    ls_ref, ls_tol, live = link_snr_refs(cell)
    ls_ratio = float((np.abs(ls - ls_ref)[live] / ls_tol[live]).max()) if live.any() else 0.0
    assert (np.abs(ls - ls_ref) <= ls_tol).all(), f"{what}: link_snr out of tolerance, worst err / tol {ls_ratio:.3f}"
    assert (ls[~live] == 0).all()
    # the serving index
    if given is None:
        want = np.where(live.any(axis=1), np.argmax(ls, axis=1), -1)
        assert np.array_equal(s, want), f"{what}: serving is not the first argmax of the kernel's link_snr"
        has = s >= 0
        u = np.arange(n)[has]
        assert (ls_ref.max(axis=1)[has] - ls_ref[u, s[has]] <= 2 * ls_tol[u, s[has]]).all(), f"{what}: a weaker link was chosen"
    else:
        g = np.asarray(given).astype(np.int64)
        assert np.array_equal(s, np.where((g >= 0) & (g < B), g, -1)), f"{what}: out_serving is not the given index"
    # the rate, with the serving index the kernel reported
    ref, ref_k = cell_rate_from_channels(Hs, snrs, s)
    tol, tol_k = cell_rate_tolerance(Hs, snrs, s)
    dead = (s < 0) | ~live[np.arange(n), np.clip(s, 0, B - 1)]
    assert (r[dead] == 0).all() and not np.signbit(r[dead]).any(), f"{what}: rate of a user who is not served is not +0.0"
    assert (rk[dead] == 0).all() and not np.signbit(rk[dead]).any(), f"{what}: rate_k of a user who is not served is not +0.0"
    assert (ref[dead] == 0).all()
    ek, e = np.abs(rk - ref_k), np.abs(r - ref)
    ratio = max(float((ek / tol_k).max()), float((e / tol).max()))
    worst_abs = max(float(ek.max()), float(e.max()))
    print(f"{what}: snr {', '.join(f'{d:.1f}' for d in snr_dbs(snrs))} dB, {int((~dead).sum())} of {n} users served, worst rate "
          f"err / tol = {ratio:.3f}, worst |err| = {worst_abs:.3e} bit, largest rate {float(ref_k.max()):.2f}, worst link_snr "
          f"err / tol = {ls_ratio:.4f}")
    WORST[what] = (ratio, ls_ratio, worst_abs)
    assert (ek <= tol_k).all(), f"{what}: {(ek > tol_k).sum()} rate_k entries out of tolerance, worst err / tol {ratio:.3f}"
    assert (e <= tol).all(), f"{what}: {(e > tol).sum()} users out of tolerance, worst err / tol {ratio:.3f}"
    mean = rk.astype(np.float64).mean(axis=1)
    assert (np.abs(r - mean) <= K * 2.0 ** -24 * rk.max(axis=1) + 2.0 ** -24).all(), f"{what}: rate is not the mean of rate_k"
    if again is not None:
        assert all(torch.equal(a, b) for a, b in zip(again, out)), f"{what}: a second launch differs"
    return ratio


def test_waves_per_workgroup_of_the_listed_shapes():
    """the shapes above drive what their names say (the launcher's rule, restated on the host)"""
    rule = lambda cid: cell_lds_rule(BY_ID[cid]["links"])                    # noqa: E731
    assert rule("wpb4_users41") == 4 and rule("wpb4_users43") == 4 and rule("wpb1_users7") == 1
    assert rule("defaults") == 4 and rule("panel") == 2 and rule("mixed_links") == 4
    assert rule("ue5_mixed") == 4 and rule("ue6") == 4 and rule("ue7") == 4
    one = lambda c: (c["ue_shape"][0] * c["ue_shape"][1] + c["bs_shape"][0] * c["bs_shape"][1] + 3) * min(c["L"], 25) * 8  # noqa: E731
    assert max(range(3), key=lambda b: one(BY_ID["mixed_links"]["links"][b])) == 0      # the 8 x 8 link sizes the slice


@pytest.mark.parametrize("cell", CASES, ids=[c["id"] for c in CASES])
def test_cell_rate_against_the_definition(cell):
    import torch
    eng = _engine()
    _, snrs = case_inputs(cell)
    preps = prepare_links(eng, cell)
    assert eng.cell_rate_supported(preps)
    db = snr_dbs(snrs)
    first = eng.cell_rate(preps, db, per_subcarrier=True, details=True)
    second = eng.cell_rate(preps, db, per_subcarrier=True, details=True)
    alone = eng.cell_rate(preps, db)                                        # fewer outputs: the same bits
    pair = eng.cell_rate(preps, db, details=True)
    torch.cuda.synchronize()
    assert torch.equal(alone, first[0])
    assert torch.equal(pair[0], first[0]) and torch.equal(pair[1], first[2]) and torch.equal(pair[2], first[3])
    check_cell(first, cell, cell["id"], again=second)
    if cell["id"] == "counts_and_holes":
        s = first[2].cpu().numpy()
        _, _, live = link_snr_refs(cell)
        assert (s == -1).sum() >= cell["links"][0]["n"] // 6 and (~live[:, 1] & (s >= 0)).sum() >= cell["links"][0]["n"] // 6
        # link 0 serves everybody: the users it does not reach get +0.0 although other links reach them
        forced = eng.cell_rate(preps, db, serving=0, per_subcarrier=True, details=True)
        torch.cuda.synchronize()
        assert (~live[:, 0] & live[:, 1:].any(axis=1)).sum() >= cell["links"][0]["n"] // 6
        check_cell(forced, cell, "counts_and_holes_serving0", given=np.zeros(len(s), np.int64))


@pytest.mark.parametrize("cid", ["defaults", "panel", "B8"])
def test_explicit_serving(cid):
    """a given serving array, with -1, B and a large value for "not served"; an int for all users"""
    import torch
    cell = BY_ID[cid]
    eng = _engine()
    _, snrs = case_inputs(cell)
    preps = prepare_links(eng, cell)
    B, n = len(preps), cell["links"][0]["n"]
    given = np.array([(-1, 0, 1, B - 1, B, 2 ** 31 - 1, -7, 0)[u % 8] for u in range(n)], dtype=np.int64)
    db = snr_dbs(snrs)
    out = eng.cell_rate(preps, db, serving=given, per_subcarrier=True, details=True)
    again = eng.cell_rate(preps, db, serving=torch.from_numpy(given.astype(np.int32)).cuda(), per_subcarrier=True, details=True)
    last = eng.cell_rate(preps, db, serving=B - 1, per_subcarrier=True, details=True)
    auto = eng.cell_rate(preps, db, per_subcarrier=True, details=True)
    as_auto = eng.cell_rate(preps, db, serving=auto[2], per_subcarrier=True)
    torch.cuda.synchronize()
    check_cell(out, cell, f"{cid}_given", given=given, again=again)
    check_cell(last, cell, f"{cid}_last", given=np.full(n, B - 1))
    assert torch.equal(as_auto[0], auto[0]) and torch.equal(as_auto[1], auto[1])      # the chosen index, given back
    assert torch.equal(out[3], auto[3])                                               # link_snr does not depend on serving


def _rx_small(cell):
    c = cell["links"][0]
    return c["ue_shape"][0] * c["ue_shape"][1] <= c["bs_shape"][0] * c["bs_shape"][1]


@pytest.mark.parametrize("cell", [c for c in CASES if _rx_small(c)], ids=[c["id"] for c in CASES if _rx_small(c)])
def test_one_link_is_the_single_link_rate_bit_for_bit(cell):
    """B = 1 writes the bits of dmx_channel_rate, and so does B = 3 with two links that reach nobody"""
    import torch
    eng = _engine()
    links, snrs = case_inputs(cell)
    c = cell["links"][0]
    rays, ue_rot = links[0][0], links[0][1]
    p = _dm_params(c).validate(c["n"])
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot))
    db = snr_dbs(snrs)[0]
    want = eng.rate(prep, db, per_subcarrier=True)
    got = eng.cell_rate([prep], db, per_subcarrier=True, details=True)
    dead = dict(c, rays="dead", per_user_rot=False, doppler=None)
    prep_dead = eng.prepare(eng.upload_rays(link_rays(dead, 1)), _dm_params(dead).validate(c["n"]), want_side="light")
    more = eng.cell_rate([prep_dead, prep, prep_dead], [db + 7.0, db, db - 3.0], per_subcarrier=True, details=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(more[0], want[0]) and torch.equal(more[1], want[1])
    live = torch.from_numpy(np.abs(links[0][2]).reshape(c["n"], -1).max(axis=1) > 0).cuda()
    assert torch.equal(got[2], torch.where(live, 0, -1).to(torch.int32))
    assert torch.equal(more[2], torch.where(live, 1, -1).to(torch.int32))
    assert bool((more[3][:, 0] == 0).all()) and bool((more[3][:, 2] == 0).all()) and torch.equal(more[3][:, 1], got[3][:, 0])


def test_user_sub_range_equals_the_rows_of_the_whole_launch():
    """user_begin > 0 with a count that is no multiple of the four waves of a workgroup; a given serving array is indexed
    from the first user of the range"""
    import torch
    cell = BY_ID["irregular"]
    eng = _engine()
    _, snrs = case_inputs(cell)
    preps = prepare_links(eng, cell)
    db, n = snr_dbs(snrs), cell["links"][0]["n"]
    full = eng.cell_rate(preps, db, per_subcarrier=True, details=True)
    b, cnt = 5, 15
    part = eng.cell_rate(preps, db, user_begin=b, user_count=cnt, per_subcarrier=True, details=True)
    given = np.array([(1, 0, -1)[u % 3] for u in range(n)], dtype=np.int32)
    full_g = eng.cell_rate(preps, db, serving=given, per_subcarrier=True, details=True)
    part_g = eng.cell_rate(preps, db, serving=given[b:b + cnt], user_begin=b, user_count=cnt, per_subcarrier=True, details=True)
    none = eng.cell_rate(preps, db, user_begin=n, user_count=0, per_subcarrier=True, details=True)
    torch.cuda.synchronize()
    for f, q in zip(full + full_g, part + part_g):
        assert torch.equal(q, f[b:b + cnt])
    assert [tuple(t.shape) for t in none] == [(0,), (0, len(IRREGULAR)), (0,), (0, 2)]


def test_refusals_of_the_engine():
    from deepmimo_amd._native import NativeError
    cell = BY_ID["defaults"]
    eng = _engine()
    _, snrs = case_inputs(cell)
    preps = prepare_links(eng, cell)
    db = snr_dbs(snrs)
    with pytest.raises(ValueError, match="links"):
        eng.cell_rate(preps * 3, db * 3)
    with pytest.raises(ValueError, match="snr_db"):
        eng.cell_rate(preps, db[:2])
    with pytest.raises(ValueError, match="snr_db"):
        eng.cell_rate(preps, float("nan"))
    with pytest.raises(ValueError, match="serving"):
        eng.cell_rate(preps, db, serving=np.zeros(3, np.int32))
    other = prepare_links(eng, BY_ID["panel"])
    assert not eng.cell_rate_supported([preps[0], other[0]])
    with pytest.raises((NativeError, ValueError)):
        eng.cell_rate([preps[0], other[0]], 10.0)


def _datasets(cell):
    import deepmimo_amd as dm
    links, _ = case_inputs(cell)
    return dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in l[0].items()}) for l in links])


def test_macro_dataset_equals_the_engine_call():
    """MacroDataset.compute_cell_rate: the bits of ChannelEngine.cell_rate, for both settings of config('channel_output')"""
    import torch
    import deepmimo_amd as dm
    cell = BY_ID["mixed_links"]
    eng = _engine()
    _, snrs = case_inputs(cell)
    db = snr_dbs(snrs)
    want = eng.cell_rate(prepare_links(eng, cell), db, per_subcarrier=True, details=True)
    plist = [_dm_params(c) for c in cell["links"]]
    n = cell["links"][0]["n"]
    macro = _datasets(cell)
    got = macro.compute_cell_rate(plist, snr_db=db, per_subcarrier=True, details=True)
    only = macro.compute_cell_rate(plist, snr_db=db)
    given = np.arange(n) % 4 - 1
    forced = macro.compute_cell_rate(plist, snr_db=db, serving=given, details=True)
    dm.config("channel_output", "torch")
    try:
        got_t = macro.compute_cell_rate(plist, snr_db=db, per_subcarrier=True, details=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(got, tuple) and len(got) == 4 and all(isinstance(a, np.ndarray) for a in got)
    assert [a.dtype for a in got] == [np.float32, np.float32, np.int32, np.float32]
    assert [a.shape for a in got] == [(n,), (n, 3), (n,), (n, 3)]
    assert isinstance(only, np.ndarray) and np.array_equal(only.view(np.int32), got[0].view(np.int32))
    for a, t, w in zip(got, got_t, want):
        assert isinstance(t, torch.Tensor) and t.is_cuda and torch.equal(t, w)
        assert np.array_equal(a.view(np.int32), w.cpu().numpy().view(np.int32))
    assert np.array_equal(forced[1], np.where(given < 3, given, -1)) and len(forced) == 3
    # one parameter set for all children, one child, a scalar snr_db: Dataset.compute_rate
    same = BY_ID["defaults"]
    p = _dm_params(same["links"][0])
    macro3 = _datasets(same)
    r3 = macro3.compute_cell_rate(p, snr_db=95.0)
    assert r3.shape == (70,) and r3.dtype == np.float32 and (r3 >= 0).all()
    one = dm.MacroDataset([macro3.datasets[0]])
    assert np.array_equal(one.compute_cell_rate(p, snr_db=95.0).view(np.int32), macro3.datasets[0].compute_rate(p, snr_db=95.0).view(np.int32))
    # the fan-out of every other name is unchanged
    both = macro3.compute_rate(p, snr_db=95.0)
    assert isinstance(both, list) and len(both) == 3


def test_interference_lowers_the_rate_of_the_same_serving_link():
    import torch
    cell = BY_ID["panel"]
    eng = _engine()
    _, snrs = case_inputs(cell)
    preps = prepare_links(eng, cell)
    db = snr_dbs(snrs)
    alone = eng.cell_rate(preps[:1], db[:1], serving=0)
    with_two = eng.cell_rate(preps, db, serving=0)
    louder = eng.cell_rate(preps, [db[0], db[1] + 6, db[2] + 6], serving=0)
    torch.cuda.synchronize()
    assert bool((with_two <= alone).all()) and bool((with_two < alone).any())
    assert bool((louder <= with_two).all()) and bool((louder < with_two).any())


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol of the rate and of link_snr and the worst absolute error over every case that ran
    (README and DESIGN.md quote them); nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=lambda i: WORST[i][0])
        kl = max(WORST, key=lambda i: WORST[i][1])
        ka = max(WORST, key=lambda i: WORST[i][2])
        print(f"cell rate: worst rate err / tol over {len(WORST)} checks = {WORST[k][0]:.3f} ({k}); worst link_snr err / tol = "
              f"{WORST[kl][1]:.4f} ({kl}); worst |err| = {WORST[ka][2]:.3e} bit ({ka})")
        assert WORST[k][0] <= 1.0 and WORST[kl][1] <= 1.0
