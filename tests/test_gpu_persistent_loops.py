"""Parity of the persistent kernels past the first work item of a workgroup / wave.

Every launcher sizes its grid to about what is resident at once (a few times that at most), so a workgroup or wave of
k2_fd_mfma, k2b_beam_project_mfma, k2_fd_fold, k2_fd_small, k2c_beam_power and the k3_lpf_fft* kernels loops over
several items and carries LDS tables, prefetched strips and flags from one to the next.  The parity tests elsewhere use
at most a few hundred users, i.e. one item per workgroup.  Here each route (tests/_persistent_routes.py) launches more
users than 2 x the largest grid its launcher can choose (grid_upper_bound, from the launchers' own sizing rules and the
hard per-CU limits of the chip), with rays whose path counts change from item to item (0, 1, 2, 3, 8, 9, 16, 17, L-1,
L valid paths, NaN holes inside some users), and checks:
  * sub-range invariance - the same users launched again in sub-ranges of at most CU-count items, where every
                           workgroup and wave takes one item, are BIT-identical to the whole launch: per-item
                           arithmetic does not depend on where the item falls, so a difference is cross-item state;
  * oracle parity        - >= 64 users (far past the first pass of every loop, right behind empty users, empty /
                           one-path / full users, the last user) against oracle_np in complex128;
  * LoS and path counts  - all users, bit-exact;
  * 16-wave forms        - variants 10 and 11 (persistent) equal variant 8 (one workgroup per item) bit for bit.

GSRC 1 (the float gains table with matrix cores) is reached through the public API by rx_filter = 1 with more than 32
path slots (route s): lpf_table_packed needs P <= 32.
"""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

from tests import _persistent_routes as R
from tests._cases import TOL_REL, assert_channel_close
from tests.test_gpu_fd_factorised import TAIL_TOL, _flat

pytestmark = pytest.mark.gpu

FC = 3.5e9
BS_ROT = np.array([5, -10, 20])


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rays(route, seed):
    """synth_rays with every user's valid-path count drawn from {0, 1, 2, 3, 8, 9, 16, 17, L-1, L} and an interior NaN
    hole in ~15 % of the users with 4 or more paths; returns (rays, drawn counts, holed mask)"""
    from oracle import oracle_np as onp
    U, L = route.U, route.L
    max_delay = 0.9 * route.N / 10e6 if route.kind == "lpf" else 2e-6
    rays = onp.synth_rays(U, L, seed=seed, all_valid=True, max_delay=max_delay, with_doppler=route.doppler)
    rng = np.random.default_rng(seed + 1)
    pool = np.unique([c for c in (0, 1, 2, 3, 8, 9, 16, 17, L - 1, L) if 0 <= c <= L])
    counts = rng.choice(pool, U)
    holed = (counts >= 4) & (rng.uniform(size=U) < 0.15)
    hole_at = np.where(holed, 1 + (rng.uniform(size=U) * np.maximum(counts - 2, 1)).astype(int), -1)
    dead = np.arange(L)[None, :] >= counts[:, None]
    dead |= np.arange(L)[None, :] == hole_at[:, None]
    for k, v in rays.items():
        if v.ndim == 2 and v.shape == (U, L):
            v[dead] = np.nan
    if route.flat:
        rays = _flat(rays, seed)
    return rays, counts, holed


def _setup(route, seed):
    import deepmimo_amd as dm
    from deepmimo_amd.engine import ChannelEngine
    from oracle import oracle_np as onp
    gc.collect()
    torch.cuda.empty_cache()
    sel = R.selection(route)
    rays, counts, holed = _rays(route, seed)
    lpf = route.kind == "lpf"
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(route.bs), np.array(route.ue)
    p.bs_antenna.rotation = BS_ROT
    p.num_paths = route.L
    p.ofdm.subcarriers = route.N
    p.ofdm.selected_subcarriers = sel
    p.ofdm.rx_filter = int(lpf)
    p.enable_doppler = int(route.doppler)
    p.validate(route.U)
    op = onp.make_params(bs_antenna=dict(shape=list(route.bs), rotation=BS_ROT), ue_antenna=dict(shape=list(route.ue)),
                         num_paths=route.L, enable_doppler=int(route.doppler),
                         ofdm=dict(subcarriers=route.N, selected_subcarriers=sel, rx_filter=int(lpf)))
    eng = ChannelEngine(0)
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", carrier_freq=FC)
    return rays, counts, holed, op, eng, prep, onp


def _codebook(route):
    import deepmimo_amd as dm
    return np.array([dm.steering_vec(np.array(route.bs), phi=a).squeeze() for a in np.linspace(-60, 60, route.n_beams)])


def _check_loops_run(route, cu):
    """every persistent launch of the route takes >= 2 x its largest possible grid of items (per workgroup or wave);
    returns the user index from which every user is past the first pass of every loop of the route and at least two
    grids past it for the route's first (hot) kernel"""
    first = None
    far = 0
    for ln in route.launches:
        items = route.U * R.items_per_user(route, ln)
        bound = R.slot_bound(route, ln, cu)
        assert items >= 2 * bound, (route.name, ln.kernel, items, bound)
        users = -(-bound // R.items_per_user(route, ln))
        if first is None:
            first = 2 * users
        far = max(far, users)
    far = max(far, first)
    assert far < route.U - 16, (route.name, far, route.U)
    return far


def _oracle_users(counts, holed, far, L, seed):
    """>= 64 users: past `far` empty / one-path / full users, users right behind an empty one, the last user, a few
    of the first pass, the rest random past `far`"""
    U = len(counts)
    rng = np.random.default_rng(seed + 2)
    tail = np.arange(far, U)
    pick = []

    def some(mask, n):
        cand = tail[mask[far:]]
        if len(cand):
            pick.extend(rng.choice(cand, min(n, len(cand)), replace=False).tolist())
        return len(cand)

    assert some(counts == 0, 6) and some(counts == 1, 6) and some((counts == L) & ~holed, 6)
    after_empty = np.zeros(U, bool)
    after_empty[1:] = counts[:-1] == 0
    assert some(after_empty & (counts > 0), 8)
    some(after_empty & (counts == 0), 2)
    some(holed, 4)
    pick += [U - 1, 0, 1, far // 2]
    rest = np.setdiff1d(tail, pick)
    pick.extend(rng.choice(rest, max(0, 70 - len(set(pick))), replace=False).tolist())
    idx = np.unique(np.array(pick))
    assert len(idx) >= 64 and idx.max() == U - 1
    return idx


def _side_parity(prep, ref):
    np.testing.assert_array_equal(prep.side["los"].cpu().numpy(), ref["los"])
    np.testing.assert_array_equal(prep.side["num_paths"].cpu().numpy(), ref["num_paths"])


def _sub_ranges(route, cu):
    """user sub-ranges in which every workgroup and wave of every launcher takes at most one item"""
    per_user = max(R.items_per_user(route, ln) for ln in route.launches)
    c = max(1, cu // per_user)
    return [(a, min(route.U, a + c)) for a in range(0, route.U, c)]


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _assert_sub_ranges_equal(route, cu, whole, launch):
    for a, b in _sub_ranges(route, cu):
        part = launch(a, b - a)
        if isinstance(whole, tuple):
            for w, x in zip(whole, part):
                assert torch.equal(_bits(x), _bits(w[a:b])), (route.name, a, b)
        else:
            assert torch.equal(_bits(part), _bits(whole[a:b])), (route.name, a, b)
        del part


def _reference(route, rays, op, idx, onp):
    dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC) if route.doppler else None
    return onp.compute_channels(rays, op, doppler=dop, users=idx)


def _grid_note(route, cu):
    return {ln.kernel + (f"<{ln.nw}w,M{ln.mode},G{ln.gsrc}>" if ln.kind == "mfma" else ""):
            (route.U * R.items_per_user(route, ln), R.grid_upper_bound(route, ln, route.U * R.items_per_user(route, ln), cu))
            for ln in route.launches}


SINGLE = [r.name for r in R.ROUTES if not r.variants]
MULTI = [r.name for r in R.ROUTES if r.variants]


@pytest.mark.parametrize("name", SINGLE)
def test_persistent_route(name):
    route = R.ROUTES_BY_NAME[name]
    cu = _cu()
    far = _check_loops_run(route, cu)
    seed = 4000 + sum(map(ord, name))
    t0 = time.time()
    rays, counts, holed, op, eng, prep, onp = _setup(route, seed)
    if route.auto is not None:
        assert eng.lib.dmx_fd_kernel_choice(C.byref(prep.params_struct), route.L) == route.auto, name
    F = _codebook(route) if route.n_beams else None
    tol = TAIL_TOL if route.flat else TOL_REL

    if route.kind == "beam_power":
        def launch(a, c):
            return eng.beam_power(prep, F, user_begin=a, user_count=c)
    else:
        def launch(a, c):
            return eng.channels(prep, user_begin=a, user_count=c, variant=route.variant, tx_codebook=F)

    whole = launch(0, route.U)
    torch.cuda.synchronize()
    _assert_sub_ranges_equal(route, cu, whole, launch)

    idx = _oracle_users(counts, holed, far, route.L, seed)
    ref = _reference(route, rays, op, idx, onp)
    _side_parity(prep, ref)
    tidx = torch.from_numpy(idx).cuda()
    Href = ref["channel"].astype(np.complex128)
    if route.kind == "beam_power":
        amp, best = (t[tidx].cpu().numpy() for t in whole)
        want = np.abs(F @ Href).mean(axis=1).mean(axis=-1)                      # [users, beams] float64
        has = ref["los"][idx] != -1
        assert has.sum() > 0 and (~has).sum() > 0
        peak = want[has].max(axis=1, keepdims=True)
        err = np.abs(amp[has] - want[has])
        assert np.all(err <= 1e-5 * peak), (name, float(np.max(err / peak)))
        assert np.all(amp[~has] == 0)
        top2 = np.sort(want[has], axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 1e-4 * top2[:, 1]                     # no near-tie for the best beam
        np.testing.assert_array_equal(best[has][clear], np.argmax(want[has], axis=1)[clear])
        worst = float(np.max(err / peak))
    else:
        want = F @ Href if route.n_beams else Href
        worst = assert_channel_close(whole[tidx].cpu().numpy(), want, tol_rel=tol, what=f"route {name}")
    print(f"\nroute {name} ({route.what}): U={route.U} items/grid bound {_grid_note(route, cu)} worst {worst:.2e} "
          f"({time.time() - t0:.1f} s)")
    del whole, prep


@pytest.mark.parametrize("name", MULTI)
def test_persistent_variants(name):
    """variants 4, 5, 3 (their own instantiations): bit-identical sub-ranges and oracle parity; 10 and 11 (the same
    16-wave instantiation as variant 8, persistent): equal to variant 8 bit for bit; all within the tolerance of
    variant 8"""
    route = R.ROUTES_BY_NAME[name]
    cu = _cu()
    far = _check_loops_run(route, cu)
    seed = 4100 + sum(map(ord, name))
    rays, counts, holed, op, eng, prep, onp = _setup(route, seed)
    assert eng.lib.dmx_fd_kernel_choice(C.byref(prep.params_struct), route.L) == route.auto
    idx = _oracle_users(counts, holed, far, route.L, seed)
    ref = _reference(route, rays, op, idx, onp)
    _side_parity(prep, ref)
    tidx = torch.from_numpy(idx).cuda()
    H8 = eng.channels(prep, variant=8)
    assert_channel_close(H8[tidx].cpu().numpy(), ref["channel"], tol_rel=TAIL_TOL, what=f"{name} v8")
    for v in route.variants:
        H = eng.channels(prep, variant=v)
        torch.cuda.synchronize()
        if v in (10, 11):
            assert torch.equal(torch.view_as_real(H), torch.view_as_real(H8)), (name, v)
        else:
            _assert_sub_ranges_equal(route, cu, H, lambda a, c: eng.channels(prep, user_begin=a, user_count=c, variant=v))
            for a, b in _sub_ranges(route, cu):                                   # all users against variant 8
                d = (torch.view_as_real(H[a:b]) - torch.view_as_real(H8[a:b])).abs().flatten(1).amax(dim=1)
                pk = torch.view_as_real(H8[a:b]).abs().flatten(1).amax(dim=1)
                assert bool((d <= 2 * TAIL_TOL * pk).all()), (name, v, a, b, float((d / pk.clamp_min(1e-30)).max()))
        assert_channel_close(H[tidx].cpu().numpy(), ref["channel"], tol_rel=TAIL_TOL, what=f"{name} v{v}")
        del H
    del H8, prep
