"""Eigenbeam precoders and combiners per user (dmx_channel_precoders, the third epilogue of k7_rate.hip) on the GPU.

Reference: the definition in complex128 from the NumPy oracle's channel tensor (tests/_precoder_ref.py, pinned against hand
cases by tests/test_precoder_cpu.py).  The inputs are the cases of tests/test_gpu_rate.py, which hit every hazard of the
shared kernel body (chunk edges, K < 64 slices, m = 1, 2, 4, 8, the BS array as the smaller one, per-user rotation, FoV and
dipole, Doppler, the adaptive workspace; with tests/_consumer_shapes.py also m = 3, 5, 6, 7 in both orientations, an odd larger
array and every kept-path count), and the rank-deficient ones of tests/test_gpu_spectrum.py at m = 3, 4 and 5; one SNR per
case as there.  Every case runs at n_layers = m.  Criteria, tests/_precoder_ref.py (gamma is the kernel's own output, x_i the
smaller-side vector, y_i the larger-side one, B = H_k^H or H_k):
    C1  |sqrt(snr) B x_i - sqrt(gamma_i) y_i|_2 <= 2 sqrt(snr) e
    C2  |snr B^H B x_i - gamma_i x_i|_2 <= tol_v (1 + c_J 2^-24)
    C3  |x_i^H x_j - delta_ij| <= 2 c_J 2^-24 over the present layers
    C4  | |y_i|^2 - 1 | <= 2 c_J 2^-24 + (3 c_J + 64) 2^-24 |gamma|_2 / gamma_i
    C5  where gamma_0 - gamma_1^ref > 10 tol_v:  1 - |<x_0, x_0^ref>|^2 / |x_0|^2 <= (tol_v / (gamma_0 - gamma_1^ref))^2
        (the squared sine of the angle; the norm of x_0 is C3's: tests/_precoder_ref.py says why the division is there)
    gamma: the mode and trace criteria of tests/test_gpu_spectrum.py (tol_g); whether it equals dmx_channel_spectrum's gamma
           bit for bit is reported, not asserted (the 2^-50 gate)
    presence from the kernel's gamma by the floor formula (no entry within 1e-5 of the floor), +0.0 for absent layers and
    users without a path, the gauge (imaginary part exactly +0, real part > 0)
and the structure: dtype, shape, contiguity, finite; a second launch, every subset of the outputs, and n_layers = 1 and 2
against the leading layers of n_layers = m, all bit-equal.
"""
import itertools
import os

import numpy as np
import pytest

from tests import _precoder_ref as pr
from tests import _spectrum_ref as sr

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests import test_gpu_rate as g  # noqa: E402
from tests import test_gpu_spectrum as gs  # noqa: E402
from tests.test_gpu_fd_direct import _case, _dm_params, _kwargs, _oracle  # noqa: E402

CASES = gs.CASES
CRITERIA = ("C1", "C2", "C3", "C4", "C5", "gauge", "zeros", "modes", "trace")
WORST = {}                                   # case id -> {criterion: worst err / tol}


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def check_precoders(gamma, w_tx, w_rx, H, snr, what, n_layers):
    """every criterion of the module docstring for one launch (torch tensors) against the reference channel H"""
    import torch
    n, m_rx, m_tx, K = H.shape
    m = min(m_rx, m_tx)
    for t, shape, dt in ((gamma, (n, K, m), torch.float32), (w_tx, (n, K, n_layers, m_tx), torch.complex64),
                         (w_rx, (n, K, n_layers, m_rx), torch.complex64)):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), what
    ga, wt, wr = gamma.cpu().numpy(), w_tx.cpu().numpy(), w_rx.cpu().numpy()
    assert np.isfinite(ga).all() and (ga >= 0).all() and (ga[..., :-1] >= ga[..., 1:]).all(), f"{what}: gamma not finite, >= 0, sorted"
    dead = np.abs(H).reshape(n, -1).max(axis=1) == 0
    for a in (ga, wt.view(np.float32), wr.view(np.float32)):
        assert (a[dead] == 0).all() and not np.signbit(a[dead]).any(), f"{what}: a user without paths is not +0.0"
    ref_g = sr.eigenmodes_from_channel(H, snr)
    tol_g = sr.mode_tolerance(H, snr)
    live = ~dead
    res = pr.check_vectors(ga, wt, wr, H, snr, what)
    res["modes"] = float((np.abs(ga - ref_g)[live] / tol_g[live][..., None]).max()) if live.any() else 0.0
    trace = snr * (np.abs(H.astype(np.complex128)) ** 2).sum(axis=(1, 2))
    res["trace"] = float((np.abs(ga.astype(np.float64).sum(axis=-1) - trace)[live] / (np.sqrt(m) * tol_g[live])).max()) if live.any() else 0.0
    present, _ = pr.presence(ga)
    print(f"{what}: snr {10 * np.log10(snr):.1f} dB, m {m}, present layers per live entry {present[live].sum(axis=-1).mean() if live.any() else 0:.2f}, "
          + ", ".join(f"{k} {res[k]:.3g}" for k in CRITERIA if k in res) + f", C5 applies to {res.get('C5_share', 0.0):.3f} of the entries (without the division by |x_0|^2: {res.get('C5_unnormalised', 0.0):.3g})")
    WORST[what] = res
    assert res["borderline"] == 0, f"{what}: {res['borderline']} layers within 1e-5 of the presence floor"
    if what in gs.RANK_ONE:
        assert not present[..., 1:].any() and present[live][..., 0].all(), f"{what}: a rank-1 channel shows a second layer"
    for k in CRITERIA:
        assert res.get(k, 0.0) <= 1.0, f"{what}: criterion {k} missed, worst err / tol = {res[k]:.4g}"
    return res


def _prep(eng, c):
    rays, ue_rot, H, _ = g.case_inputs(c)
    p = _dm_params(c).validate(c["n"])
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", adaptive_terms=c["adaptive"], **_kwargs(c, ue_rot))
    return prep, H


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_precoders_against_the_definition(c):
    import torch
    eng = _engine()
    prep, H = _prep(eng, c)
    snr = gs.case_snr(H)
    snr_db = 10 * np.log10(snr)
    snr = 10.0 ** (snr_db / 10.0)
    m = min(H.shape[1], H.shape[2])
    assert eng.precoder_supported(prep, m) and not eng.precoder_supported(prep, m + 1) and not eng.precoder_supported(prep, 0)
    full = eng.precoders(prep, snr_db, n_layers=m)
    again = eng.precoders(prep, snr_db, n_layers=m)
    subsets = {flags: eng.precoders(prep, snr_db, n_layers=m, gamma=flags[0], tx=flags[1], rx=flags[2])
               for flags in itertools.product((False, True), repeat=3) if any(flags) and not all(flags)}
    fewer = {L: eng.precoders(prep, snr_db, n_layers=L) for L in (1, 2) if L < m}
    spectrum = eng.spectrum(prep, snr_db)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, full)), "a second launch differs"
    for flags, got in subsets.items():
        got = got if isinstance(got, tuple) else (got,)
        want = [t for t, f in zip(full, flags) if f]
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), f"outputs {flags} differ"
    for L, (ga, wt, wr) in fewer.items():
        assert torch.equal(ga, full[0]) and torch.equal(wt, full[1][:, :, :L]) and torch.equal(wr, full[2][:, :, :L]), \
            f"n_layers = {L} is not the leading layers of n_layers = {m}"
    print(f"{c['id']}: gamma bit-equal to dmx_channel_spectrum: {bool(torch.equal(spectrum, full[0]))}")
    check_precoders(*full, H, snr, c["id"], m)


def test_user_sub_range_with_guard_regions():
    """user_begin = 5, 15 of 37 users (no multiple of the four waves of a workgroup), all three outputs: the rows of the
    whole launch bit for bit, sentinel-filled guard regions around every output untouched, a count of zero is empty"""
    import torch
    n, K, m, m_tx, L = 37, 3, 2, 8, 2
    rays, p = g._small(n, K=K)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light")
    full = eng.precoders(prep, 17.0, n_layers=L)
    assert tuple(full[0].shape) == (n, K, m) and tuple(full[1].shape) == (n, K, L, m_tx) and tuple(full[2].shape) == (n, K, L, m)
    guard, sentinel = 1 << 16, -12345.5
    sizes = (n * K * m, n * K * L * m_tx, n * K * L * m)
    dts = (torch.float32, torch.complex64, torch.complex64)
    bigs = [torch.full((guard + s + guard,), sentinel, dtype=dt, device="cuda") for s, dt in zip(sizes, dts)]
    outs = [b[guard:guard + s].view(f.shape) for b, s, f in zip(bigs, sizes, full)]

    def guards_untouched():
        return all(bool((b[:guard] == sentinel).all()) and bool((b[guard + s:] == sentinel).all()) for b, s in zip(bigs, sizes))
    eng.precoders(prep, 17.0, n_layers=L, out=tuple(outs))
    torch.cuda.synchronize()
    assert guards_untouched(), "write outside the output tensors"
    assert all(torch.equal(o, f) for o, f in zip(outs, full))
    for b in bigs:
        b.fill_(sentinel)
    b0, cnt = 5, 15
    eng.precoders(prep, 17.0, n_layers=L, user_begin=b0, user_count=cnt, out=tuple(o[b0:b0 + cnt] for o in outs))
    torch.cuda.synchronize()
    assert guards_untouched()
    for o, f in zip(outs, full):
        assert bool((o[:b0] == sentinel).all()) and bool((o[b0 + cnt:] == sentinel).all()), "rows outside the range written"
        assert torch.equal(o[b0:b0 + cnt], f[b0:b0 + cnt])
    assert torch.equal(eng.precoders(prep, 17.0, user_begin=b0, user_count=cnt, gamma=False, rx=False), full[1][b0:b0 + cnt, :, :1])
    empty = eng.precoders(prep, 17.0, n_layers=L, user_begin=n, user_count=0)
    assert [tuple(t.shape) for t in empty] == [(0, K, m), (0, K, L, m_tx), (0, K, L, m)]


def test_largest_shape_runs_and_the_next_one_is_refused():
    """796 x 1 BS at 25 paths and one subcarrier is the last shape taken (tests/test_gpu_rate.py has the arithmetic), 797
    the first refused: NativeError from the engine, ValueError from the Dataset.  M_big = 796 with one subcarrier is also
    the widest slicing of the second pass (64 slices)."""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    n, L = 3, 25
    rays = onp.synth_rays(n, L, seed=77, all_valid=True)
    c = _case("largest", n, L, [796, 1], [1, 1], 512, [9])
    eng = _engine()
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, _dm_params(c).validate(n), want_side="light", carrier_freq=28e9)
    assert eng.precoder_supported(prep, 1)
    H = _oracle(c, rays, np.zeros(3))["channel"]
    snr_db = 10 * np.log10(gs.case_snr(H))
    out = eng.precoders(prep, snr_db)
    torch.cuda.synchronize()
    check_precoders(*out, H, 10.0 ** (snr_db / 10.0), "largest", 1)
    c2 = dict(c, bs_shape=[797, 1])
    prep2 = eng.prepare(dr, _dm_params(c2).validate(n), want_side="light", carrier_freq=28e9)
    assert not eng.precoder_supported(prep2, 1)
    with pytest.raises(NativeError, match=r"status -2.*LDS"):
        eng.precoders(prep2, snr_db)
    with pytest.raises(NativeError, match=r"status -2.*n_layers"):
        eng.precoders(prep, snr_db, n_layers=2)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    with pytest.raises(ValueError, match="LDS"):
        ds.compute_precoders(_dm_params(c2), snr_db=snr_db)
    ga, wt = ds.compute_precoders(_dm_params(c), snr_db=snr_db)
    assert ga.shape == (n, 1, 1) and wt.shape == (n, 1, 1, 796)


def test_public_api_numpy_and_torch_returns_and_the_definition():
    import torch
    import deepmimo_amd as dm
    n = 90
    rays, p = g._small(n, 25, (8, 1), (2, 1), 4, seed=22)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    ds.apply_fov(bs_fov=np.array([140, 120]))
    H = ds.compute_channels(p)
    snr_db = float(10 * np.log10(gs.case_snr(H)))
    bits = lambda a: (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)      # noqa: E731
    pair = ds.compute_precoders(p, snr_db=snr_db, n_layers=2)
    triple = ds.compute_precoders(p, snr_db=snr_db, n_layers=2, combiners=True)
    one = ds.compute_precoders(p, snr_db=snr_db)
    dm.config("channel_output", "torch")
    try:
        pair_t = ds.compute_precoders(p, snr_db=snr_db, n_layers=2)
        triple_t = ds.compute_precoders(p, snr_db=snr_db, n_layers=2, combiners=True)
    finally:
        dm.config("channel_output", "numpy")
    assert isinstance(pair, tuple) and len(pair) == 2 and len(triple) == 3 and len(pair_t) == 2 and len(triple_t) == 3
    assert all(isinstance(a, np.ndarray) for a in triple) and all(isinstance(a, torch.Tensor) and a.is_cuda for a in triple_t)
    assert triple[0].dtype == np.float32 and triple[0].shape == (n, 4, 2)
    assert triple[1].dtype == np.complex64 and triple[1].shape == (n, 4, 2, 8)
    assert triple[2].dtype == np.complex64 and triple[2].shape == (n, 4, 2, 2)
    for a, b in zip(pair + triple, pair_t + triple_t):
        assert np.array_equal(bits(a), bits(b)), "NumPy and torch returns differ"
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(pair, triple)), "combiners changes gamma or w_tx"
    assert np.array_equal(bits(one[0]), bits(pair[0])) and np.array_equal(bits(one[1]), bits(pair[1][:, :, :1]))
    check_precoders(*(torch.from_numpy(a) for a in triple), H, 10.0 ** (snr_db / 10.0), "public api", 2)
    assert all((a[ds.num_paths == 0] == 0).all() for a in triple)


def test_macro_dataset_fans_out():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    a, b = onp.synth_rays(31, 25, seed=1), onp.synth_rays(18, 25, seed=2)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 1])
    p.ofdm.selected_subcarriers = np.arange(0, 512, 100)
    macro = dm.MacroDataset([dm.Dataset({k: v.copy() for k, v in r.items()}) for r in (a, b)])
    assert "compute_precoders" in dm.MacroDataset.PROPAGATE_METHODS
    got = macro.compute_precoders(p, snr_db=95.0, n_layers=2, combiners=True)
    assert isinstance(got, list) and len(got) == 2
    for r, res in zip((a, b), got):
        ds = dm.Dataset({k: v.copy() for k, v in r.items()})
        alone = ds.compute_precoders(p, snr_db=95.0, n_layers=2, combiners=True)
        assert [x.shape for x in res] == [(len(r["power"]), 6, 2), (len(r["power"]), 6, 2, 8), (len(r["power"]), 6, 2, 2)]
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(res, alone))


def test_zz_report_worst_ratio():
    """Last in the file: the worst err / tol per criterion over every case that ran (DESIGN.md quotes them); nothing ran =
    nothing to report."""
    if WORST:
        for k in CRITERIA:
            have = {i: w[k] for i, w in WORST.items() if k in w}
            if have:
                i = max(have, key=have.get)
                print(f"precoders: {k} worst err / tol over {len(have)} cases = {have[i]:.4g} ({i})")
                assert have[i] <= 1.0
