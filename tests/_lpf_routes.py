"""Case table and float64 reference of tests/test_gpu_rx_filter_routes.py and tests/test_rx_filter_routes_cpu.py.

rx_filter = 1 has four gain kernels behind one dispatcher (launch_channels_fd_lpf_once, k3_lpf_gains.hip).  This module
restates the dispatcher in its default build (`lpf_route`; the tuning hooks stay at their defaults), the facts of the
three kernels the fast N = 64 / 128 / 256 / 512 / 1024 kernel leaves over (the radices, the gather form and the LDS of
k3_lpf_fft_wave; PB and the batches of k3_lpf_fft; the LDS of the direct kernel k3_lpf_gains), the table of cases that
reach each of their branches, the rays of a case and the float64 gains of every kept path.  A plain module: no torch,
no GPU.  tests/test_rx_filter_routes_cpu.py pins the restated conditions to the kernel file's text.

Users of every case (synth_rays decides the valid-path counts of the others):
  WHOLE  whole-sample delays 0, N//7, 2 (N//7) ... on its first paths (up to six): np.sinc(0) = 1 taps
  LAST   a path at N - 1 samples
  ONE / NONE / TWO   one, zero and two paths
  EQUAL  every valid path at -80 dBW: a lost path is an error of about 1 / n_paths of the user's peak
They are users 0 .. 5, so that the oracle's share of the largest case can stop at six users; users 3 .. 7 - the
sub-range the GPU test launches again - hold NONE, TWO, EQUAL and two ordinary users.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

BANDWIDTH = 10e6
FC = 28e9
BS_ROT = [0, 10, 45]
ARRAYS = {"mfma": ([8, 4], [2, 2]), "valu": ([2, 1], [1, 1])}
LIGHTSPEED = 299792458.0

WHOLE, LAST, ONE, NONE, TWO, EQUAL = range(6)
SUB_BEGIN, SUB_COUNT = 3, 5

NBIN = 8                          # k3_lpf_fft_wave: bins a lane keeps in registers
MAX_N = 4096                      # N * 16 bytes of the direct kernel's LDS within 64 KiB


# ---- the dispatcher, restated (k3_lpf_gains.hip, launch_channels_fd_lpf_once) -------------------------------------------
def lpf_route(N, K, P):
    """the gain kernel of N subcarriers, K selected ones and P path slots (P = min(num_paths, loaded paths) > 0)"""
    if N * 16 > 64 * 1024:
        return "refused"
    pow2 = N >= 2 and (N & (N - 1)) == 0
    if pow2 and 64 <= N <= 1024 and K <= N and P <= 64:
        return "fft_pow2"
    if pow2 and 64 <= N <= 2048:
        return "fft_wave"
    if pow2:
        return "fft"
    return "gains"


def mfma_preferred(M, K):
    """fd_mfma_preferred (k2_channel_fd_mfma.hip): M antenna pairs, K >= 1 selected subcarriers"""
    return K >= 1 and (M >= 9 or (M == 8 and K >= 1024))


def table_packed(N, K, P, M):
    """whether the gains table is written as packed f16 pairs: lpf_table_packed (k2_channel_fd.hip), asked by the two
    wave FFT kernels only - k3_lpf_fft and k3_lpf_gains always write floats"""
    return lpf_route(N, K, P) in ("fft_pow2", "fft_wave") and mfma_preferred(M, K) and P <= 32


def log2n(N):
    n = 0
    while (1 << n) < N:
        n += 1
    return n


def wave_radices(N):
    """radices of k3_lpf_fft_wave's Stockham passes: 8 while three or more bits are left, then one of 4 or 2"""
    left, out = log2n(N), []
    while left > 0:
        r = 3 if left >= 3 else left
        out.append(1 << r)
        left -= r
    return tuple(out)


def wave_gather(K):
    return "regs" if K <= 64 * NBIN else "buffer"


def wave_lds_bytes(N):
    return N * 8 + 4 * 2 * (N + N // 16 + 1) * 8


def fft_pb(N, P):
    """paths k3_lpf_fft transforms together"""
    return min(max(4096 // N, 1), 16, P)


def fft_batches(N, P, n):
    """batch sizes of a user with n kept paths"""
    pb = fft_pb(N, P)
    return [min(pb, n - l0) for l0 in range(0, n, pb)]


def fft_lds_bytes(N, P):
    pb = fft_pb(N, P)
    return (N // 2) * 8 + pb * N * 8 + pb * 4


def gains_lds_bytes(N):
    return N * 16


# ---- the cases --------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    N: int
    sel: tuple                    # ("range", a, b, s) | ("random", count, lo, hi, seed)
    L: int
    arrays: Tuple[str, ...]
    reaches: str
    n_ue: int = 9
    all_valid: bool = False
    delay_factor: float = 1.1     # max_delay = delay_factor * N / BANDWIDTH
    oracle_users: Optional[int] = None      # the oracle's share: the first so many users (None: all)


# Seeds: the first of 0, 1, 2 ... for which the rays of the case hold what `case_rays` asserts (the fixture users have
# the paths their names promise) and for which the equal-power user meets tests/test_rx_filter_routes_cpu.py's
# sensitivity condition with Doppler off and on.  The search is `first_good_seed` below.
CASES = (
    Case("w2048_all", 2048, ("range", 0, 2048, 1), 25, ("mfma",),
         "fft_wave 8.8.8.4, buffer gather, packed, 155,712 B of LDS", n_ue=8, oracle_users=6),
    Case("w2048_first", 2048, ("range", 0, 300, 1), 25, ("mfma", "valu"), "register bins, guarded k < K"),
    Case("w2048_512", 2048, ("range", 0, 512, 1), 25, ("valu",), "K = 64 * NBIN: the last selection in registers"),
    Case("w2048_513", 2048, ("range", 0, 513, 1), 25, ("valu",), "K = 64 * NBIN + 1: the first through the buffer"),
    Case("w2048_neg", 2048, ("random", 100, -4096, 4096, 21), 25, ("valu",), "& (N - 1) floor-mod in binreg"),
    Case("w256_wrap", 256, ("range", 0, 300, 1), 25, ("mfma", "valu"), "8.8.4 at small N, register bins", n_ue=12),
    Case("w128_wrap", 128, ("range", 0, 130, 1), 25, ("valu",), "8.8.2", n_ue=12),
    Case("w64_wrap", 64, ("range", 0, 70, 1), 25, ("valu",), "8.8", n_ue=12),
    Case("w256_p70", 256, ("range", 0, 256, 3), 70, ("mfma", "valu"),
         "P > 64: the l >= 64 branch, float table on both array sizes, accumulate passes beyond 32 slots",
         all_valid=True, delay_factor=0.9),
    Case("w512_p70", 512, ("range", 0, 200, 1), 70, ("valu",), "the same beside the 512 fast path it displaces",
         all_valid=True, delay_factor=0.9),
    Case("f32_all", 32, ("range", 0, 32, 1), 25, ("valu",), "k3_lpf_fft, PB = 16: one full batch and a ragged one", n_ue=14),
    Case("f32_off", 32, ("range", 20, 52, 1), 25, ("valu",), "the same, bins past N", n_ue=14),
    Case("f8", 8, ("range", 0, 8, 1), 9, ("valu",), "log2 N = 3", n_ue=14),
    Case("f2", 2, ("range", 0, 2, 1), 9, ("valu",), "log2 N = 1 (half_n = 1)", n_ue=14),
    Case("f4096", 4096, ("random", 64, 0, 8192, 22), 9, ("mfma", "valu"), "PB = 1, 12 stages"),
    Case("g600", 600, ("range", 0, 300, 1), 12, ("valu",), "direct kernel: three tap passes, two bin passes"),
    Case("g4000", 4000, ("random", 40, -8000, 8000, 23), 9, ("valu",), "64,000 B of LDS, step < 0"),
    Case("g1", 1, ("list", 0, 1, 5), 5, ("valu",), "N = 1", n_ue=14),
)
SEEDS = {"w2048_all": 0, "w2048_first": 0, "w2048_512": 0, "w2048_513": 0, "w2048_neg": 0, "w256_wrap": 1, "w128_wrap": 0,
         "w64_wrap": 2, "w256_p70": 2, "w512_p70": 3, "f32_all": 1, "f32_off": 1, "f8": 0, "f2": 11, "f4096": 0, "g600": 1,
         "g4000": 0, "g1": 26}
CASES_BY_ID = {c.id: c for c in CASES}
GPU_CASES = [(c.id, a) for c in CASES for a in c.arrays]


def selection(case):
    s = case.sel
    if s[0] == "range":
        return np.arange(s[1], s[2], s[3])
    if s[0] == "random":
        return np.random.default_rng(s[4]).integers(s[2], s[3], s[1])
    return np.asarray(s[1:])


def pairs(arrays):
    bs, ue = ARRAYS[arrays]
    return bs[0] * bs[1] * ue[0] * ue[1]


def route_of(case):
    return lpf_route(case.N, len(selection(case)), case.L)


def packed(case, arrays):
    return table_packed(case.N, len(selection(case)), case.L, pairs(arrays))


def case_dict(case, arrays):
    """the case description tests/_cases.oracle_params and tests/test_gpu_parity._dm_params take"""
    bs, ue = ARRAYS[arrays]
    return dict(bs_shape=bs, ue_shape=ue, bs_spacing=0.5, ue_spacing=0.5, bs_rot=BS_ROT, bs_pattern="isotropic",
                ue_pattern="isotropic", num_paths=case.L, freq_domain=1, subcarriers=case.N,
                selected=list(selection(case)), bandwidth=BANDWIDTH, rx_filter=1, bs_fov=None, ue_fov=None)


_RAYS = {}


def _path_keys(rays, L):
    return [k for k, v in rays.items() if v.ndim == 2 and v.shape[1] == L and k not in ("rx_pos", "tx_pos")]


def build_rays(case, seed):
    from oracle import oracle_np as onp
    N, L = case.N, case.L
    rays = onp.synth_rays(case.n_ue, L, seed=1000 * N + 10 * L + seed, all_valid=case.all_valid,
                          max_delay=case.delay_factor * N / BANDWIDTH, with_doppler=True)
    keys = _path_keys(rays, L)
    nw = min(6, L)
    rays["delay"][WHOLE, :nw] = (np.arange(nw) * (N // 7) / BANDWIDTH).astype(np.float32)
    rays["delay"][LAST, 0] = (N - 1) / BANDWIDTH
    for k in keys:
        rays[k][ONE, 1:] = np.nan
        rays[k][NONE, :] = np.nan
        rays[k][TWO, 2:] = np.nan
    rays["power"][EQUAL, ~np.isnan(rays["power"][EQUAL])] = -80.0
    return rays


def fixture_problems(case, rays):
    """what keeps the fixture users from being what their names say (empty when all is well)"""
    valid = np.isfinite(rays["power"]).sum(axis=1)
    bad = []
    if valid[WHOLE] < 3:                                     # delays 0, N//7 and 2 (N//7) samples at the least
        bad.append("WHOLE has fewer than three paths")
    if valid[LAST] < 1 or valid[ONE] != 1 or valid[NONE] != 0 or valid[TWO] != 2:
        bad.append("LAST / ONE / NONE / TWO")
    if valid[EQUAL] < max(3, min(8, case.L // 2)):
        bad.append("EQUAL has too few paths")
    return bad


def case_rays(case):
    """the rays of a case (shared, read-only)"""
    if case.id not in _RAYS:
        rays = build_rays(case, SEEDS[case.id])
        assert not fixture_problems(case, rays), (case.id, fixture_problems(case, rays))
        for v in rays.values():
            v.setflags(write=False)
        _RAYS[case.id] = rays
    return _RAYS[case.id]


def doppler_arg(rays, doppler):
    return dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC) if doppler else None


def oracle(case, arrays, doppler, users=None):
    """oracle_np.compute_channels of the case; users: None = the case's oracle share"""
    from oracle import oracle_np as onp
    from tests._cases import oracle_params
    rays = case_rays(case)
    op = oracle_params(case_dict(case, arrays), np.zeros(3))
    op["enable_doppler"] = int(doppler)
    if users is None and case.oracle_users is not None:
        users = np.arange(case.oracle_users)
    ref = onp.compute_channels(rays, op, doppler=doppler_arg(rays, True), users=users)
    if case.L > 64:
        assert ref["num_paths"].max() > 64, (case.id, ref["num_paths"])
    return ref


# ---- the float64 reference of the gains table ---------------------------------------------------------------------------
def path_records(rays, cd):
    """(c [n, P] complex64, dn [n, P] float32, keep [n, P] bool) in the reference's dtypes (oracle_np.ofdm_path_gains:
    channel.py:183-192): dn = delay / Ts in float32, clipped paths get zero power, c = sqrt(power / N) e^{j phase} in
    complex64.  keep = what stage 1 gives a record slot: every field finite, dn < N, a non-zero coefficient."""
    from oracle import oracle_np as onp
    from tests._cases import oracle_params
    prep = onp.prepare_paths(rays, oracle_params(cd, np.zeros(3)))
    P, N = cd["num_paths"], cd["subcarriers"]
    ts = 1 / cd["bandwidth"]
    pw = np.array(prep["_power_linear_ant_gain"][:, :P], copy=True)
    dn = rays["delay"][:, :P] / ts
    with np.errstate(invalid="ignore"):
        over = dn >= N
    pw[over] = 0
    dn[over] = N
    c = np.sqrt(pw / N) * np.exp(1j * np.deg2rad(rays["phase"][:, :P]))
    fin = np.isfinite(c) & np.isfinite(dn)
    for k in ("_aod_el_rot_fov", "_aod_az_rot_fov", "_aoa_el_rot_fov", "_aoa_az_rot_fov"):
        fin &= np.isfinite(prep[k][:, :P])
    keep = fin & (dn < N) & (c != 0)
    return c, dn, keep, prep


_DFT = {}


def dft_matrix(N, sel):
    """exp(-2j pi d sc_k / N) [N, K] with the phase index reduced in integers"""
    key = (N, tuple(int(s) for s in sel))
    if key not in _DFT:
        _DFT.clear()                                         # one at a time: 64 MB at N = K = 2048
        idx = (np.arange(N, dtype=np.int64)[:, None] * np.asarray(sel, dtype=np.int64)[None, :]) % N
        _DFT[key] = np.exp(-2j * np.pi * idx / N)
    return _DFT[key]


def tap_rows(rays, cd, doppler, users=None):
    """[user][n_keep, N] complex128 taps c_l sinc(d - dn_l) D_l(d) of the kept paths, and the kept path indices"""
    c, dn, keep, _ = path_records(rays, cd)
    N = cd["subcarriers"]
    ts = 1 / cd["bandwidth"]
    d = np.arange(N)
    users = range(len(c)) if users is None else users
    taps, kept = [], []
    for u in users:
        idx = np.flatnonzero(keep[u])
        t = c[u, idx].astype(np.complex128)[:, None] * np.sinc(d[None, :] - dn[u, idx].astype(np.float64)[:, None])
        if doppler:
            tau = ts * d[None, :]
            v = rays["doppler_vel"][u, idx].astype(np.float64)[:, None]
            a = rays["doppler_acc"][u, idx].astype(np.float64)[:, None]
            t = t * np.exp(-2j * np.pi * FC * (v * tau / LIGHTSPEED + a * tau ** 2 / (2 * LIGHTSPEED)))
        taps.append(t)
        kept.append(idx)
    return taps, kept


def lpf_gain_rows(rays, cd, doppler, users=None):
    """[user][n_keep, K] complex128: g[l, k] = c_l sum_d sinc(d - dn_l) D_l(d) exp(-2j pi d sc_k / N) of every kept path,
    in stage 1's order (the loaded order of the kept paths)"""
    W = dft_matrix(cd["subcarriers"], cd["selected"])
    return [t @ W for t in tap_rows(rays, cd, doppler, users)[0]]


def responses(rays, cd, users=None):
    """[user] (a_rx [M_rx, n_keep], a_tx [M_tx, n_keep]) float64 array responses of the kept paths"""
    from oracle import oracle_np as onp
    c, dn, keep, prep = path_records(rays, cd)
    P = cd["num_paths"]
    a_tx = onp.array_response_batch(cd["bs_shape"], cd["bs_spacing"], prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"])[..., :P]
    a_rx = onp.array_response_batch(cd["ue_shape"], cd["ue_spacing"], prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"])[..., :P]
    users = range(len(c)) if users is None else users
    return [(a_rx[u][:, keep[u]], a_tx[u][:, keep[u]]) for u in users]


def channel_from_rows(resp, rows):
    """H [M_rx, M_tx, K] complex128 of one user from its gain rows"""
    a_rx, a_tx = resp
    return np.einsum("rl,tl,lk->rtk", a_rx, a_tx, rows)


def sensitivity(resp, rows):
    """(smallest move of H over every dropped path, over every swapped pair of rows, peak |H|) of one user.  A dropped
    path l moves H by the outer product A_l (x) g_l and a swap of rows i, j by (A_i - A_j) (x) (g_j - g_i), whose largest
    element is the product of the factors' largest elements."""
    a_rx, a_tx = resp
    n = rows.shape[0]
    A = (a_rx[:, None, :] * a_tx[None, :, :]).reshape(-1, n)              # [M, n]
    peak = np.abs(channel_from_rows(resp, rows)).max()
    gmax = np.abs(rows).max(axis=1)
    drop = (np.abs(A).max(axis=0) * gmax).min() if n else np.inf
    swap = np.inf
    for i in range(n):
        for j in range(i + 1, n):
            swap = min(swap, np.abs(A[:, i] - A[:, j]).max() * np.abs(rows[i] - rows[j]).max())
    return drop, swap, peak


def first_good_seed(case, tol, limit=50):
    """the first seed whose rays pass `fixture_problems` and whose EQUAL user meets the sensitivity condition"""
    for seed in range(limit):
        rays = build_rays(case, seed)
        if fixture_problems(case, rays):
            continue
        ok = True
        for arrays in case.arrays:
            cd = case_dict(case, arrays)
            resp = responses(rays, cd, [EQUAL])[0]
            for dop in (False, True):
                rows = lpf_gain_rows(rays, cd, dop, [EQUAL])[0]
                drop, swap, peak = sensitivity(resp, rows)
                ok = ok and rows.shape[0] >= 3 and min(drop, swap) >= 2 * tol * peak
        if ok:
            return seed
    raise AssertionError(case.id)
