"""Inputs shared by tests/test_path_counts_cpu.py and tests/test_gpu_path_counts.py: every kept-path count and every K-step
tail kind of the frequency-domain kernels, on purpose.  A plain module: NumPy and the oracle only, no torch, no GPU.

* `ladder_rays`: user u keeps exactly u paths, every path within 6 dB of the strongest, so an error in ANY path - the last
  K-step's included - is an error of the channel at the bounds the kernels are held to (`sensitivity` measures that).
* `weak_tail_rays`: the worst case of the opt-in one-term rule (DMX_FLAG_ADAPTIVE_TERMS) for each number of K-steps.
* `tail_kind`: the fold kernel's `tile_kind = 2 * nsteps + last_weak`, restated.
"""
from __future__ import annotations

import copy

import numpy as np

# |H - H_ref| <= bound * max|H_ref[user]|: the project's own figures (test_precision_flag_parity's `lim`, and its
# element-wise bound of the beam amplitudes); everything else is held to tests/_cases.py TOL_REL
BOUND_MATRIX_CORE = 3e-6
BOUND_ADAPTIVE = 1e-5
BOUND_BEAM_POWER = 1e-5

K_STEP = 8                         # paths per K-step of the matrix-core contractions
MAX_KEPT = 32                      # kept paths per user, at most
WEAK_POWER_RATIO = 2.0 ** -22      # |c|^2 of a weak last K-step against the user's strongest path


def flat(rays, seed, lo=-66.0, hi=-60.0):
    """the same rays with every valid path's power drawn from [lo, hi] dB instead of [-140, -60]"""
    r = {k: v.copy() for k, v in rays.items()}
    ok = np.isfinite(r["power"])
    r["power"][ok] = np.random.default_rng(seed).uniform(lo, hi, ok.sum()).astype(np.float32)
    return r


def ray_keys(rays):
    return [k for k in rays if k not in ("rx_pos", "tx_pos")]


# ---- the ladder -------------------------------------------------------------------------------------------------------
def ladder_counts(L):
    """valid loaded paths of each user of the ladder: 0 .. min(L, 32), and for 40 loaded paths 33 and 40 as well"""
    counts = list(range(min(L, MAX_KEPT) + 1))
    if L == 40:
        counts += [33, 40]
    return counts


def ladder_rays(L, seed, holes=False, with_doppler=False, max_delay=2e-6):
    """One user per count (`ladder_counts`), powers in [-66, -60] dB, everything else from `synth_rays`.  Without holes the
    valid paths are the first ones of the row.  With holes NaNs lie between them: min(count, 32) valid paths inside the
    first 32 columns (what num_paths = 32 looks at), the rest behind, and at least one NaN in front of the last valid path,
    so the count is reached by compaction."""
    from oracle import oracle_np as onp
    counts = ladder_counts(L)
    rays = flat(onp.synth_rays(len(counts), L, seed=seed, all_valid=True, max_delay=max_delay, with_doppler=with_doppler), seed)
    rng = np.random.default_rng(seed + 1)
    W = min(L, MAX_KEPT)
    for u, cnt in enumerate(counts):
        valid = np.zeros(L, bool)
        if not holes:
            valid[:cnt] = True
        else:
            head = min(cnt, W)
            valid[rng.choice(W, size=head, replace=False)] = True
            if 0 < head < W and valid[:head].all():
                valid[head - 1], valid[head] = False, True
            if cnt > W:
                valid[W + rng.choice(L - W, size=cnt - W, replace=False)] = True
        for k in ray_keys(rays):
            rays[k][u, ~valid] = np.nan
    return rays


def kept_counts(rays, num_paths):
    """paths a user keeps: the valid ones among the first num_paths loaded (dataset.py:258-261, channel.py:260)"""
    return np.isfinite(rays["power"][:, :num_paths]).sum(axis=1)


# the runs of the ladder: loaded paths, num_paths, holes.  L40_np10 is the ladder of 40 loaded paths under num_paths = 10,
# below the count of most of its users
LADDER_RUNS = {
    "L32": dict(L=32, num_paths=32, holes=False, seed=3201),
    "L40": dict(L=40, num_paths=32, holes=False, seed=4001),
    "L32_holes": dict(L=32, num_paths=32, holes=True, seed=3202),
    "L40_holes": dict(L=40, num_paths=32, holes=True, seed=4002),
    "L40_np10": dict(L=40, num_paths=10, holes=False, seed=4003),
}
_LADDERS = {}


def ladder_run(name):
    """(rays, kept counts) of a run, built once and shared (callers do not modify them)"""
    if name not in _LADDERS:
        r = LADDER_RUNS[name]
        rays = ladder_rays(r["L"], r["seed"], holes=r["holes"])
        _LADDERS[name] = (rays, kept_counts(rays, r["num_paths"]))
    return _LADDERS[name]


def fd_case(bs, ue, sel, L, num_paths, subcarriers=512, rx_filter=0):
    """case description in the form tests/_cases.py `oracle_params` and test_gpu_parity.py `_dm_params` take"""
    return dict(bs_shape=list(bs), ue_shape=list(ue), bs_spacing=0.5, ue_spacing=0.37, bs_rot=[0, 0, 0],
                bs_pattern="isotropic", ue_pattern="isotropic", num_paths=num_paths, L=L, freq_domain=1, subcarriers=subcarriers,
                selected=[int(s) for s in sel], bandwidth=20e6, rx_filter=rx_filter, bs_fov=None, ue_fov=None)


# the smallest shapes that reach each form of the frequency-domain contraction: (BS, UE, selection, bound)
FD_SHAPES = {
    "valu": ([3, 2], [2, 1], range(0, 34, 2), None),                  # variant 1; 12 pairs, K = 17
    "mfma": ([8, 8], [2, 2], range(64), BOUND_MATRIX_CORE),            # variants 2 / 4 / 5 / 10
    "mfma_sincos": ([8, 8], [2, 2], tuple(range(63)) + (70,), BOUND_MATRIX_CORE),   # no uniform spacing: sin / cos B', nothing packed
    "small": ([4, 2], [2, 1], (5, 6, 7), None),                       # variant 9 and the single pass, K = 3
    "consumers": ([4, 2], [2, 1], range(0, 90, 10), None),            # covariance and rate, K = 9 (at K = 3 a swapped pair of
                                                                      # paths moves the rate by 1.7x its tolerance only)
    "fold_wave": ([8, 1], [1, 1], range(64), BOUND_MATRIX_CORE),       # variant 12, per-wave tables, 8 pairs
    "fold_wave_K100": ([4, 3], [1, 1], range(100), BOUND_MATRIX_CORE),  # 12 pairs: no power of two, partial last block
    "fold_shared": ([8, 4], [2, 1], range(128), BOUND_MATRIX_CORE),    # variant 12, one table set per workgroup, 64 pairs
}
BEAM_SHAPE = ([8, 8], [2, 1], range(0, 128, 2))                        # 32 beams on it, K = 64
_REFS = {}
CHANNEL_FORMS = [k for k in FD_SHAPES if k != "consumers"]


def codebooks(bs, nb=32):
    """the two codebooks of the beam tests, [nb, M_tx] complex128: steering vectors over -60 ... 60 degrees of azimuth
    (oracle_np.steering_vec, the reference's formula) and an un-normalised random one"""
    from oracle import oracle_np as onp
    m_tx = bs[0] * bs[1]
    steering = np.array([onp.steering_vec(bs, phi=a).ravel() for a in np.around(np.linspace(-60, 60, nb), 2)])
    rng = np.random.default_rng(5)
    return {"steering": steering, "random": (rng.normal(size=(nb, m_tx)) + 1j * rng.normal(size=(nb, m_tx))) * 11.0}


def beam_amplitudes(Y):
    """[..., beams] mean of |Y| over rx and subcarriers, Y [..., M_rx, beams, K]: what k2c_beam_power returns"""
    return np.abs(Y).mean(axis=-3).mean(axis=-1)


def reference(case, rays, key):
    """oracle_np.compute_channels for `case`, computed once per key and left unchanged"""
    if key not in _REFS:
        from oracle import oracle_np as onp
        from tests._cases import oracle_params
        ref = onp.compute_channels(rays, oracle_params(case, np.zeros(3)))
        ref["channel"].setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def ladder_reference(shape, run):
    """(case, rays, kept counts, oracle result) of a frequency-domain shape on a run of the ladder"""
    bs, ue, sel, _ = FD_SHAPES[shape] if shape in FD_SHAPES else BEAM_SHAPE + (None,)
    rays, kept = ladder_run(run)
    r = LADDER_RUNS[run]
    case = fd_case(bs, ue, sel, r["L"], r["num_paths"])
    return case, rays, kept, reference(case, rays, (shape, run))


# ---- rx_filter ladder -------------------------------------------------------------------------------------------------
LPF_L = 25
LPF_N = (48, 64, 128, 256, 512, 1024)
LPF_ARRAYS = {"mfma": ([8, 4], [2, 2]), "valu": ([2, 1], [1, 1])}
FC = 3.5e9


def lpf_rays():
    """the ladder for rx_filter = 1: 25 loaded paths, delays inside the shortest symbol (48 samples at 20 MHz = 2.4 us)"""
    if "lpf" not in _LADDERS:
        rays = ladder_rays(LPF_L, 2501, with_doppler=True, max_delay=2e-6)
        _LADDERS["lpf"] = (rays, kept_counts(rays, LPF_L))
    return _LADDERS["lpf"]


def lpf_reference(arrays, N, doppler):
    from oracle import oracle_np as onp
    from tests._cases import oracle_params
    bs, ue = LPF_ARRAYS[arrays]
    rays, kept = lpf_rays()
    case = fd_case(bs, ue, range(N), LPF_L, LPF_L, subcarriers=N, rx_filter=1)
    key = ("lpf", arrays, N, doppler)
    if key not in _REFS:
        op = oracle_params(case, np.zeros(3))
        op["enable_doppler"] = int(doppler)
        dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC) if doppler else None
        _REFS[key] = onp.compute_channels(rays, op, doppler=dop)
    return case, rays, kept, _REFS[key]


# ---- the one-term rule ------------------------------------------------------------------------------------------------
def tail_kind(n_keep, amplitudes, adaptive):
    """`tile_kind` of k2_fd_fold for a user: 2 * K-steps + (1 if the last K-step takes one product term).  amplitudes:
    |c_l| of the kept paths; with the flag stage 1 hands them over by falling |c|^2 (ties by path index), so the last
    K-step holds the weakest ones.  The rule (also k2_channel_fd_mfma.hip stage_item, k2c_beam_power.hip): two K-steps
    at least, and every |c|^2 of the last one at most 2^-22 of the largest.  0 for a user without paths (no tile runs)."""
    n = min(int(n_keep), MAX_KEPT)
    if n == 0:
        return 0
    a2 = np.asarray(amplitudes, np.float32)[:n] ** 2
    assert a2.shape == (n,)
    nsteps = (n + K_STEP - 1) // K_STEP
    last_weak = False
    if adaptive:
        a2 = -np.sort(-a2, kind="stable")
        l0w = ((n - 1) // K_STEP) * K_STEP
        last_weak = bool(l0w >= K_STEP and np.float32(a2[l0w:].max()) * np.float32(1 / WEAK_POWER_RATIO) <= a2.max())
    return 2 * nsteps + int(last_weak)


def mfma_flag_changes_bits(n_keep, amplitudes, factorised):
    """Whether DMX_FLAG_ADAPTIVE_TERMS changes what k2_fd_mfma computes for a user whose paths arrive strongest first: the
    rule fires (`tail_kind`), and the last K-step is not a packed one.  With a uniformly spaced selection (the factorised
    B', GSRC = 4) a last K-step of one or two paths is packed into one MFMA with all three product terms in BOTH modes
    (k2_channel_fd_mfma.hip stage_item: `pack`), so there the flag has nothing left to drop."""
    n = min(int(n_keep), MAX_KEPT)
    fires = tail_kind(n, amplitudes, True) != tail_kind(n, amplitudes, False)
    packed = factorised and n > 0 and n - ((n - 1) // K_STEP) * K_STEP <= 2
    return fires and not packed


def kept_amplitudes(rays, num_paths, subcarriers=512):
    """per user: |c_l| = sqrt(power / N) of the kept paths in path order (isotropic elements; channel.py:170-198)"""
    pw = rays["power"][:, :num_paths]
    out = []
    for u in range(pw.shape[0]):
        v = np.isfinite(pw[u])
        out.append(np.sqrt(10.0 ** (pw[u, v].astype(np.float64) / 10) / subcarriers))
    return out


def tail_kinds(rays, num_paths, adaptive):
    return np.array([tail_kind(len(a), a, adaptive) for a in kept_amplitudes(rays, num_paths)])


def weak_tail_rays(n_keep, occupancy, fires, seed=0, presorted=False, L=MAX_KEPT):
    """One user ([1, L] arrays) whose last K-step holds `occupancy` paths just under the rule's threshold (66.5 to 66.8 dB
    below the strongest path: it must fire) or just over it (64.5 to 65 dB below: it must not); the other n_keep - occupancy
    paths lie within 0.5 dB under -70 dBW.  Shuffled, so that stage 1 has to find the order, or strongest first, where
    stage 1's ranking is the identity."""
    from oracle import oracle_np as onp
    assert 9 <= n_keep <= L and occupancy == n_keep - ((n_keep - 1) // K_STEP) * K_STEP, (n_keep, occupancy)
    rays = onp.synth_rays(1, L, seed=7000 + 64 * seed + n_keep, all_valid=True)
    rng = np.random.default_rng(9000 + 64 * seed + 2 * n_keep + int(fires))
    p = np.full(L, np.nan)
    strong = n_keep - occupancy
    p[:strong] = -70.0 + rng.uniform(-0.5, 0.0, strong)
    top = np.float32(p[:strong]).max()
    p[strong:n_keep] = top - 66.5 - rng.uniform(0, 0.3, occupancy) if fires else top - 65.0 + rng.uniform(0, 0.5, occupancy)
    order = np.arange(L)
    if presorted:
        order[:n_keep] = np.argsort(-p[:n_keep], kind="stable")
    else:
        order[:n_keep] = rng.permutation(n_keep)
    keys = ray_keys(rays)
    for k in keys:
        rays[k][0, n_keep:] = np.nan
    rays["power"][0] = p.astype(np.float32)
    for k in keys:
        rays[k][0] = rays[k][0, order]
    return rays


WEAK_TAIL_CASES = [(n_keep, occ, fires, rep) for rep in range(3) for n_keep, occ in ((9, 1), (16, 8), (17, 1), (24, 8), (25, 1), (32, 8))
                   for fires in (True, False)]


def weak_tail_batch(presorted):
    """(rays of all WEAK_TAIL_CASES as one batch of 36 users, fires [36] bool, n_keep [36])"""
    key = ("weak", presorted)
    if key not in _LADDERS:
        rows = [weak_tail_rays(n, occ, f, seed=rep, presorted=presorted) for n, occ, f, rep in WEAK_TAIL_CASES]
        rays = {k: np.concatenate([r[k] for r in rows], axis=0) for k in rows[0] if k != "tx_pos"}
        rays["tx_pos"] = rows[0]["tx_pos"]
        _LADDERS[key] = (rays, np.array([f for _, _, f, _ in WEAK_TAIL_CASES]), np.array([n for n, _, _, _ in WEAK_TAIL_CASES]))
    return _LADDERS[key]


def weak_tail_reference(shape, presorted):
    bs, ue, sel, _ = FD_SHAPES[shape] if shape in FD_SHAPES else BEAM_SHAPE + (None,)
    rays, fires, n_keep = weak_tail_batch(presorted)
    case = fd_case(bs, ue, sel, MAX_KEPT, MAX_KEPT)
    return case, rays, fires, n_keep, reference(case, rays, (shape, "weak", presorted))


# ---- what a wrong path does to the reference ----------------------------------------------------------------------------
def f16_round(z):
    """real and imaginary part rounded to float16"""
    z = np.asarray(z, np.complex128)
    return z.real.astype(np.float16).astype(np.float64) + 1j * z.imag.astype(np.float16).astype(np.float64)


def path_terms(rays, params, doppler=None):
    """Per user, from the oracle's own building blocks in float64 (the steps of oracle_np.compute_channels before its sum
    over paths): (t [M_rx, M_tx, n] array-response products, c [n] path coefficients, E [n, K] with c_l E[l] the path's
    subcarrier gains) of the n kept paths.  H[u] = einsum('rtl,l,lk->rtk', t, c, E)."""
    from oracle import oracle_np as onp
    params = copy.deepcopy(params)
    np.random.seed(1001)
    prep = onp.prepare_paths(rays, params)
    P = int(params["num_paths"])
    bs, ue, ofdm = params["bs_antenna"], params["ue_antenna"], params["ofdm"]
    a_tx = onp.array_response_batch(bs["shape"], bs["spacing"], prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"])[..., :P]
    a_rx = onp.array_response_batch(ue["shape"], ue["spacing"], prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"])[..., :P]
    power = prep["_power_linear_ant_gain"][..., :P]
    delay, phase = rays["delay"][..., :P], rays["phase"][..., :P]
    out = []
    for u in range(power.shape[0]):
        v = np.isfinite(power[u])
        if not v.any():
            out.append(None)
            continue
        dop = (doppler["vel"][u, :P][v], doppler["acc"][u, :P][v], doppler["carrier_freq"]) if doppler else None
        g = onp.ofdm_path_gains(power[u, v], delay[u, v], phase[u, v], ofdm, dop).astype(np.complex128)
        c = np.sqrt(power[u, v].astype(np.float64) / ofdm["subcarriers"]) * np.exp(1j * np.deg2rad(phase[u, v].astype(np.float64)))
        t = (a_rx[u][:, None, v] * a_tx[u][None, :, v]).astype(np.complex128)
        out.append((t, c, g / c[:, None]))
    return out


def user_scale(c):
    """the power of two by which the matrix-core kernels scale a user's coefficients: the largest |Re c|, |Im c| lands in
    [512, 1024) (k2_channel_fd_fold.hip: frexpf / ldexpf(1, 10 - e))"""
    m = max(np.abs(c.real).max(), np.abs(c.imag).max())
    return 2.0 ** (10 - np.frexp(np.float32(m))[1])


def project(terms, codebook):
    """the terms of the beam-space channel F @ H: t becomes [M_rx, beams, n]"""
    t, c, E = terms
    return np.einsum("bt,rtl->rbl", np.asarray(codebook, np.complex128), t), c, E


def mutation_delta(terms, kind, l):
    """H_mutated - H of one user ([M_rx, M_tx or beams, K], complex128) for a mutation of kept path l:
    'drop'  the path is missing (a kept count one short, a masked slot);
    'swap'  its coefficient and that of path l + 1 change places (a wrong slot index);
    'f16'   its scaled coefficient on every antenna pair, c_l a_rx a_tx, keeps only its float16 part (a dropped lo term)."""
    t, c, E = terms
    if kind == "drop":
        return -np.einsum("rt,k->rtk", t[..., l] * c[l], E[l])
    if kind == "swap":
        return (c[l + 1] - c[l]) * (np.einsum("rt,k->rtk", t[..., l], E[l]) - np.einsum("rt,k->rtk", t[..., l + 1], E[l + 1]))
    if kind == "f16":
        gs = user_scale(c)
        x = t[..., l] * c[l] * gs
        return np.einsum("rt,k->rtk", (f16_round(x) - x) / gs, E[l])
    raise ValueError(kind)


def sensitivity_by(terms_all, kind, measure, codebook=None):
    """per user: the smallest over its kept paths of measure(u, H_mutated - H); inf where the mutation has no path to act
    on.  `measure` returns the change of the quantity under test over the bound it is held to."""
    out = np.full(len(terms_all), np.inf)
    for u, terms in enumerate(terms_all):
        if terms is None:
            continue
        if codebook is not None:
            terms = project(terms, codebook)
        n = len(terms[1])
        for l in (range(n - 1) if kind == "swap" else range(n)):
            out[u] = min(out[u], measure(u, mutation_delta(terms, kind, l)))
    return out


def sensitivity(terms_all, H, kind, codebook=None):
    """per user: the smallest over its kept paths of max|H_mutated - H| / max|H[u]| (inf where the mutation has no path to
    act on).  The GPU test's bound for the user has to stay below half of it."""
    H = np.asarray(H)
    out = np.full(len(terms_all), np.inf)
    for u, terms in enumerate(terms_all):
        if terms is None:
            continue
        if codebook is not None:
            terms = project(terms, codebook)
        n = len(terms[1])
        peak = np.abs(H[u]).max()
        ls = range(n - 1) if kind == "swap" else range(n)
        for l in ls:
            out[u] = min(out[u], np.abs(mutation_delta(terms, kind, l)).max() / peak)
    return out
