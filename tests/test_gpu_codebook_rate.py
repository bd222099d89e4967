"""Codebook-precoded rate and PMI per user (dmx_codebook_rate, k10_codebook_rate.hip) on the GPU.

Reference: the definition, slogdet in complex128 of the NumPy oracle's channel tensor times the codebook
(tests/_codebook_rate_ref.py; tests/test_codebook_rate_cpu.py pins it against hand cases).  Criterion per entry:
|rate_c - ref| <= tol_c with the derived tolerance of that module.  The SNR of a case comes from its reference alone: the median
live user sits at 10 dB before any beamforming gain.  Every case also holds: rate == rate_c[u, pmi] bit for bit, pmi is the
first index of max(rate_c[u]), the reference rate of the chosen codeword is within the two tolerances of the reference's
best, everything finite and >= 0, exactly +0.0 / -1 / +0.0 where the reference channel is all zero, a second launch is
torch.equal, and the call without rate_c gives the same rate / pmi bits.
Waves per workgroup of a shape come from the LDS rule restated in tests/test_codebook_rate_cpu.py; the rule's largest tables
are two waves per workgroup, so the launch-residue case beside the 4-wave one is a 2-wave shape.
"""
import os

import numpy as np
import pytest

from tests import _consumer_shapes as shapes
from tests._cases import golden_names, load_golden
from tests._codebook_rate_ref import case_codebook, case_snr, codebook_rate_from_channel, codebook_rate_tolerance
from tests._rate_ref import rate_from_channel, rate_tolerance

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle, _rays, _ue_rot  # noqa: E402

WORST = {}                                   # case id -> (worst err / tol, worst |err| in bit), printed by the last test
IRREGULAR = [-3, 0, 5, 511, 512, 700, -1000, 77, 2 ** 31 - 1, -(2 ** 31), 40001]      # of tests/test_gpu_rate.py


def live_counts(n, L):
    """live paths per user, cycled: 0, 1, 2, L - 1, L"""
    return [min(L, (0, 1, 2, L - 1, L)[u % 5]) for u in range(n)]


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _cb(cid, n, L, bs, ue, N, sel, layers, C, **kw):
    return _case(cid, n, L, bs, ue, N, sel, layers=layers, C=C, **kw)


def _cases():
    cs = []
    cs.append(_cb("defaults", 70, 25, [8, 1], [1, 1], 512, [0], 1, 8))                   # DeepMIMO's defaults, K = 1
    # subcarrier-chunk edges: one below, at and above the 64 subcarriers of a chunk, and the full selection
    cs.append(_cb("K63", 40, 25, [8, 1], [1, 1], 512, range(3, 66), 1, 8))
    cs.append(_cb("K64", 40, 25, [8, 1], [1, 1], 512, range(3, 67), 1, 8))
    cs.append(_cb("K65", 40, 25, [8, 1], [1, 1], 512, range(3, 68), 1, 8))
    cs.append(_cb("K512", 24, 25, [8, 1], [2, 1], 512, range(512), 1, 8))
    # lane slices: kcp = 1, 4, 8, 64 with S = 64, 16, 8, 1 codeword slices
    for K in (1, 3, 7, 33):
        cs.append(_cb(f"slices_K{K}", 30, 25, [4, 4], [2, 2], 512, [(37 * k) % 512 for k in range(K)], 2, 16))
    cs.append(_cb("C1", 30, 25, [4, 4], [2, 2], 512, [0, 9, 100], 2, 1))                  # fewer codewords than slices
    # codeword-chunk edges: 32 / 10 / 8 codewords of 1 / 3 / 4 layers fill a chunk; 32 loaded paths, all valid
    for C in (31, 32, 33):
        cs.append(_cb(f"L1_C{C}", 21, 32, [8, 4], [4, 2], 512, [0, 17, 100], 1, C, all_valid=True))
    for C in (10, 11):
        cs.append(_cb(f"L3_C{C}", 21, 32, [8, 4], [4, 2], 512, [0, 17, 100], 3, C, all_valid=True))
    for C in (8, 9):
        cs.append(_cb(f"L4_C{C}", 21, 32, [8, 4], [4, 2], 512, [0, 17, 100], 4, C, all_valid=True))
    cs.append(_cb("L2_4x2", 29, 25, [4, 2], [2, 1], 512, [0, 9, 100, 300, 511], 2, 4))
    cs.append(_cb("L4_4x4", 23, 25, [4, 4], [2, 2], 512, [0, 17, 100], 4, 4))
    cs.append(_cb("panel_C64", 23, 25, [8, 8], [2, 2], 512, range(0, 512, 37), 1, 64))
    cs.append(_cb("irregular", 33, 25, [4, 2], [2, 1], 512, IRREGULAR, 2, 4))
    cs.append(_cb("one_path", 50, 1, [4, 2], [1, 1], 64, [0, 9, 63], 1, 8))
    cs.append(_cb("P32_num_paths_below_loaded", 19, 40, [4, 2], [2, 1], 256, [0, 17, 100], 2, 4, num_paths=32, all_valid=True))
    cs.append(_cb("P32_num_paths_above_loaded", 19, 32, [4, 2], [2, 1], 256, [0, 17, 100], 2, 4, num_paths=40, all_valid=True))
    # users with 0 / 1 / 2 / L - 1 / L paths.  One layer: a fifth of the users have one path, rank one under a two-layer
    # codeword, where the tolerance outgrows 1 % of the rate (tests/test_codebook_rate_cpu.py holds the share)
    cs.append(_cb("counts_and_holes", 45, 25, [4, 2], [2, 1], 512, [0, 3, 200], 1, 8, rays="counts"))
    # launch residue: 4k + 1 / 2 / 3 users of a 4-wave shape, an odd count of a 2-wave shape
    for n in (41, 42, 43):
        cs.append(_cb(f"wpb4_users{n}", n, 25, [8, 1], [1, 1], 512, [0, 5], 1, 8))
    cs.append(_cb("wpb2_users7", 7, 25, [8, 4], [2, 2], 512, range(64), 1, 32))
    # stage-1 features arrive through the records.  rot_fov_dipole: the FoV leaves many users one path
    cs.append(_cb("rot_fov_dipole", 53, 25, [4, 2], [1, 1], 512, [0, 1, 2], 1, 8, bs_rot=[5, -20, 60], ue_rot=[10, 20, 30],
                  bs_fov=[150, 110], ue_fov=[200, 100], bs_pattern="halfwave-dipole", ue_pattern="halfwave-dipole"))
    cs.append(_cb("per_user_rot", 45, 25, [8, 1], [2, 2], 512, [0, 7], 2, 4, per_user_rot=True))
    cs.append(_cb("doppler", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], 2, 4, doppler=1))
    cs.append(_cb("adaptive_workspace", 61, 25, [8, 4], [2, 1], 512, range(0, 64, 3), 2, 16, adaptive=True))
    for c in cs:
        c["selected"] = list(c["selected"])
        c.setdefault("adaptive", False)
    return cs


# and every (M_rx, layers) pair the kernel is instantiated for, every kept-path count (tests/_consumer_shapes.py)
CASES = _cases() + shapes.CODEBOOK_CASES
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
    """(rays, ue_rot, H of the oracle, W, snr, (ref_c, tol_c)) of a case: computed once, shared and left unchanged"""
    if c["id"] not in _INPUTS:
        rays, ue_rot = _case_rays(c), _ue_rot(c)
        H = _oracle(c, rays, ue_rot)["channel"]
        H.setflags(write=False)
        W = case_codebook(c["bs_shape"], c["C"], c["layers"])
        snr = case_snr(H)
        ref = (codebook_rate_from_channel(H, W, snr)[0], codebook_rate_tolerance(H, W, snr)[0])
        _INPUTS[c["id"]] = (rays, ue_rot, H, W, snr, ref)
    return _INPUTS[c["id"]]


def test_waves_per_workgroup_of_the_listed_shapes():
    """the shapes above drive what their names say (the launcher's rule, restated on the host)"""
    from tests.test_codebook_rate_cpu import lds_rule
    by = {c["id"]: c for c in CASES}
    rule = lambda cid: lds_rule(by[cid]["ue_shape"], len(by[cid]["selected"]), min(by[cid]["num_paths"], by[cid]["L"]),   # noqa: E731
                                by[cid]["C"], by[cid]["layers"])
    assert rule("wpb4_users41") == 4 and rule("wpb4_users43") == 4 and rule("wpb2_users7") == 2
    assert rule("defaults") == 4 and rule("K512") == 4 and rule("panel_C64") == 4
    assert rule("ml_1_1") == 4 and rule("ml_8_4") == 4 and rule("ml_3_3_C11") == 4 and rule("every_count") == 4


def check_result(rate, pmi, rate_c, H, ref, what, again=None, alone=None):
    """The criterion and the structural properties of one launch against the reference (ref_c, tol_c) of channel H"""
    import torch
    ref_c, tol_c = ref
    n, C = ref_c.shape
    assert rate.dtype == torch.float32 and tuple(rate.shape) == (n,) and rate.is_contiguous()
    assert pmi.dtype == torch.int32 and tuple(pmi.shape) == (n,) and pmi.is_contiguous()
    assert rate_c.dtype == torch.float32 and tuple(rate_c.shape) == (n, C) and rate_c.is_contiguous()
    r, p, rc = rate.cpu().numpy(), pmi.cpu().numpy(), rate_c.cpu().numpy()
    assert np.isfinite(r).all() and np.isfinite(rc).all() and (r >= 0).all() and (rc >= 0).all(), f"{what}: NaN, inf or negative"
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    assert (r[dead] == 0).all() and not np.signbit(r[dead]).any(), f"{what}: a user without paths is not +0.0"
    assert (rc[dead] == 0).all() and not np.signbit(rc[dead]).any(), f"{what}: rate_c of a user without paths is not +0.0"
    assert (p[dead] == -1).all() and (p[~dead] >= 0).all() and (p < C).all(), f"{what}: pmi outside -1 / 0..C-1"
    live = np.flatnonzero(~dead)
    assert np.array_equal(p[live], rc[live].argmax(axis=1)), f"{what}: pmi is not the first maximum of rate_c"
    assert np.array_equal(r[live].view(np.int32), rc[live, p[live]].view(np.int32)), f"{what}: rate is not rate_c[u, pmi]"
    e = np.abs(rc - ref_c)
    ratio = float((e / tol_c).max()) if n else 0.0
    worst_abs = float(e.max()) if n else 0.0
    print(f"{what}: worst err / tol = {ratio:.3f}, worst |err| = {worst_abs:.3e} bit, largest rate {float(ref_c.max()):.2f}")
    WORST[what] = (ratio, worst_abs)
    assert (e <= tol_c).all(), f"{what}: {(e > tol_c).sum()} rate_c entries out of tolerance, worst err / tol {ratio:.3f}"
    best = ref_c[live].argmax(axis=1)
    slack = tol_c[live, p[live]] + tol_c[live, best]
    assert (ref_c[live, p[live]] >= ref_c[live, best] - slack).all(), f"{what}: a pmi whose reference rate is not the best"
    if again is not None:
        assert all(torch.equal(a, b) for a, b in zip(again, (rate, pmi, rate_c))), f"{what}: a second launch differs"
    if alone is not None:
        assert torch.equal(alone[0], rate) and torch.equal(alone[1], pmi), f"{what}: the call without rate_c differs"
    return ratio


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_codebook_rate_against_the_definition(c):
    import torch
    eng = _engine()
    rays, ue_rot, H, W, snr, ref = case_inputs(c)
    p = _dm_params(c).validate(c["n"])
    kw = _kwargs(c, ue_rot)
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **kw)
    assert eng.codebook_rate_supported(prep, c["C"], c["layers"])
    snr_db = 10 * np.log10(snr)
    first = eng.codebook_rate(prep, W, snr_db, per_codeword=True)
    second = eng.codebook_rate(prep, W, snr_db, per_codeword=True)
    alone = eng.codebook_rate(prep, W, snr_db)                              # without the optional output: the same bits
    torch.cuda.synchronize()
    assert len(alone) == 2 and len(first) == 3
    if c["rays"] == "counts":
        assert (np.abs(H).reshape(c["n"], -1).max(axis=1) == 0).sum() >= c["n"] // 5      # the users without a path
    check_result(*first, H, ref, c["id"], again=second, alone=alone)
    m_tx = c["bs_shape"][0] * c["bs_shape"][1]
    if c["C"] * c["layers"] > m_tx and c["layers"] == 1:                    # a repeated codeword repeats its bits
        rc, pm = first[2].cpu().numpy(), first[1].cpu().numpy()
        assert np.array_equal(rc[:, m_tx:].view(np.int32), rc[:, :c["C"] - m_tx].view(np.int32))
        assert (pm < m_tx).all(), "the first of two equal maxima wins"


def test_the_repeated_codeword_case_is_in_the_table():
    by = {c["id"]: c for c in CASES}
    assert by["L1_C33"]["C"] == 33 and by["L1_C33"]["bs_shape"] == [8, 4]
    W = case_codebook([8, 4], 33, 1)
    assert np.array_equal(W[32], W[0]) and not np.array_equal(W[1], W[0])


def _golden_ok(name):
    case, rays, _, ref = load_golden(name)
    return bool(case["freq_domain"]) and not case["rx_filter"] and "channel" in ref and \
        1 <= min(case["num_paths"], rays["power"].shape[1]) <= 32 and case["ue_shape"][0] * case["ue_shape"][1] <= 8


GOLDENS = [g for g in golden_names() if _golden_ok(g)]


def test_some_goldens_store_their_channel():
    assert len(GOLDENS) >= 5, GOLDENS


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_codebook_rate_of_the_reference_channel(name):
    """the channel tensor the real reference wrote (Doppler off: `channel` is the tensor without it), single-layer DFT beams"""
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
    m_tx = case["bs_shape"][0] * case["bs_shape"][1]
    W = case_codebook(case["bs_shape"], min(m_tx, 16), 1)
    snr_db = 10 * np.log10(case_snr(H))
    snr = 10.0 ** (snr_db / 10.0)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", **kw)
    res = eng.codebook_rate(prep, W, snr_db, per_codeword=True)
    torch.cuda.synchronize()
    check_result(*res, H, (codebook_rate_from_channel(H, W, snr)[0], codebook_rate_tolerance(H, W, snr)[0]), name)


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


def test_user_sub_range_equals_the_rows_of_the_whole_launch():
    """user_begin > 0 with a count that is no multiple of the four waves of a workgroup, all three outputs"""
    import torch
    n = 37
    rays, p = _small(n)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    W = case_codebook([4, 2], 5, 2)
    full = eng.codebook_rate(prep, W, 97.0, per_codeword=True)
    b, cnt = 5, 15
    part = eng.codebook_rate(prep, W, 97.0, per_codeword=True, user_begin=b, user_count=cnt)
    torch.cuda.synchronize()
    assert bool((full[0] > 0).any())
    for f, q in zip(full, part):
        assert q.shape[0] == cnt and torch.equal(q, f[b:b + cnt])
    empty = eng.codebook_rate(prep, W, 97.0, per_codeword=True, user_begin=n, user_count=0)
    assert empty[0].shape == (0,) and empty[1].shape == (0,) and empty[2].shape == (0, 5)


def test_user_blocks_of_the_engine_are_invisible(monkeypatch):
    """with the beam workspace of a call forced down to a few users the blocked result equals the unblocked one"""
    import torch
    n = 37
    rays, p = _small(n)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    W = case_codebook([4, 2], 5, 2)
    whole = eng.codebook_rate(prep, W, 97.0, per_codeword=True)
    calls = []
    real = eng.lib.dmx_codebook_rate

    def counted(*a):
        calls.append(int(a[5]))
        return real(*a)
    monkeypatch.setattr(eng, "CODEBOOK_WS_BYTES", 512 + 6 * (5 * 2 * 11 * 8 + 4), raising=False)
    monkeypatch.setattr(eng.lib, "dmx_codebook_rate", counted, raising=False)
    blocked = eng.codebook_rate(prep, W, 97.0, per_codeword=True)
    torch.cuda.synchronize()
    assert calls == [6] * 6 + [1], calls
    for a, b in zip(whole, blocked):
        assert torch.equal(a, b)


def test_identity_codebook_is_the_equal_power_rate():
    """W = I as one codeword of M_tx layers: E = H and snr / L = snr / M_tx, the rate of dmx_channel_rate, within the sum of
    the two derived tolerances (the Gram here runs over the 4 BS-side layers, there over the smaller array - the same)"""
    import torch
    c = _case("identity", 31, 25, [2, 2], [4, 2], 512, [0, 9, 100])
    rays, ue_rot = _rays(c), _ue_rot(c)
    H = _oracle(c, rays, ue_rot)["channel"]
    W = np.eye(4, dtype=np.complex64)[None]
    snr_db = 10 * np.log10(case_snr(H))
    snr = 10.0 ** (snr_db / 10.0)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), _dm_params(c).validate(c["n"]), want_side="light", **_kwargs(c, ue_rot))
    rate, pmi, rate_c = eng.codebook_rate(prep, W, snr_db, per_codeword=True)
    plain = eng.rate(prep, snr_db)
    torch.cuda.synchronize()
    ref_c, tol_c = codebook_rate_from_channel(H, W, snr)[0], codebook_rate_tolerance(H, W, snr)[0]
    ref, _ = rate_from_channel(H, snr)
    tol, _ = rate_tolerance(H, snr)
    np.testing.assert_allclose(ref_c[:, 0], ref, rtol=1e-9, atol=1e-12)
    check_result(rate, pmi, rate_c, H, (ref_c, tol_c), "identity")
    assert (np.abs(rate_c.cpu().numpy()[:, 0] - plain.cpu().numpy()) <= tol_c[:, 0] + tol).all()


def test_public_api_numpy_and_torch_returns_are_the_same_bits():
    import torch
    import deepmimo_amd as dm
    rays, p = _small(90, 25, (8, 1), (2, 1), 4, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    H = ds.compute_channels(p)
    snr_db = float(10 * np.log10(case_snr(H)))
    pair = ds.compute_codebook_rate(p, snr_db=snr_db)
    three = ds.compute_codebook_rate(p, snr_db=snr_db, per_codeword=True, codebook=dm.dft_codebook([8, 1]))
    W2 = case_codebook([8, 1], 4, 2)
    two_layers = ds.compute_codebook_rate(p, snr_db=snr_db, per_codeword=True, codebook=W2)
    dm.config("channel_output", "torch")
    try:
        three_t = ds.compute_codebook_rate(p, snr_db=snr_db, per_codeword=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(pair, tuple) and len(pair) == 2 and len(three) == 3
    r, pm, rc = three
    assert isinstance(r, np.ndarray) and r.dtype == np.float32 and r.shape == (90,)
    assert pm.dtype == np.int32 and pm.shape == (90,) and rc.dtype == np.float32 and rc.shape == (90, 8)
    assert np.array_equal(pair[0].view(np.int32), r.view(np.int32)) and np.array_equal(pair[1], pm)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in three_t)
    for a, b in zip(three, three_t):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    # and the definition, from the channel tensor of the same dataset
    snr = 10.0 ** (snr_db / 10.0)
    for W, got in ((dm.dft_codebook([8, 1])[:, None, :], rc), (W2, two_layers[2])):
        ref_c, tol_c = codebook_rate_from_channel(H, W, snr)[0], codebook_rate_tolerance(H, W, snr)[0]
        assert (np.abs(got - ref_c) <= tol_c).all()
    np.testing.assert_array_equal(ds.num_paths == 0, np.abs(H).reshape(90, -1).max(axis=1) == 0)
    assert (r[ds.num_paths == 0] == 0).all() and (pm[ds.num_paths == 0] == -1).all() and (pm[ds.num_paths > 0] >= 0).all()


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    assert "compute_codebook_rate" in dm.MacroDataset.PROPAGATE_METHODS
    both = macro.compute_codebook_rate(p, snr_db=95.0, per_codeword=True)
    assert isinstance(both, list) and len(both) == 2
    for r, got in zip((a, b), both):
        alone = dm.Dataset({k: v.copy() for k, v in r.items()}).compute_codebook_rate(p, snr_db=95.0, per_codeword=True)
        assert len(got) == 3
        for x, y in zip(got, alone):
            assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol and the worst absolute error over every case that ran (DESIGN.md quotes both);
    nothing ran = nothing to report."""
    if WORST:
        k = max(WORST, key=lambda i: WORST[i][0])
        ka = max(WORST, key=lambda i: WORST[i][1])
        print(f"codebook rate: worst err / tol over {len(WORST)} cases = {WORST[k][0]:.3f} ({k}); worst |err| = {WORST[ka][1]:.3e} bit ({ka})")
        assert WORST[k][0] <= 1.0
