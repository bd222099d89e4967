"""Cases of the transmit-precoding and multi-user rate tests (tests/test_mu_rate_cpu.py, tests/test_gpu_mu_rate.py).  A
plain module: NumPy and the oracle only, nothing of deepmimo_amd, no torch.

The ray matrices are the oracle's synthetic ones with the powers raised by a shift a case names (POWER_SHIFT_DB where it
names none), chosen so that at the case's snr_db = -10, 10 or 30 the stream SNR of a typical user is some 10 dB: rates
of a few bit/s/Hz that the interference visibly lowers, and a tolerance - which grows with the SNR times the channel
criterion - that stays a small part of them (tests/test_mu_rate_cpu.py checks that).  Every case has a user without a
path and one with a single path.

VIEW_CASES: the channels of a `with_tx_precoder` view - how `beams` is given, a BS panel, a UE array, a selection of K = 1,
5, 64 or 70 subcarriers, BS rotation / field of view / pattern, where the rays live.
MU_CASES: `compute_mu_rate` - G = 1, 2, 4, 8 with ragged groups and users in no group, M_rx = 1, 2, 4, 8, K = 1, 64, 70
(a chunk tail), 130, 3 / 25 / 32 kept paths, snr_db = -10, 10, 30."""
from __future__ import annotations

import numpy as np

POWER_SHIFT_DB = 85.0

BASE = dict(bs_shape=[8, 1], ue_shape=[1, 1], bs_spacing=0.5, ue_spacing=0.5, bs_rot=[0, 0, 0], bs_pattern="isotropic",
            ue_pattern="isotropic", num_paths=8, freq_domain=1, subcarriers=64, selected=[0], bandwidth=10e6, rx_filter=0,
            bs_fov=None, ue_fov=None)
_K5 = [0, 3, 7, 20, 63]
UE_ROT = np.array([10, -20, 30])

# name -> (changes of BASE, users, loaded paths, codebook: "dft" | ("random", B), beams: "all" | "per_user" | ("table", J), rays)
VIEW_CASES = {
    "bs8x1_ue1x1_K1_all_beams_host":
        (dict(selected=[0]), 7, 8, ("random", 3), "all", "host"),
    "bs4x2_ue2x1_K5_per_user_bs_rot_fov_hbm":
        (dict(bs_shape=[4, 2], ue_shape=[2, 1], selected=_K5, bs_rot=[20, -10, 40], bs_fov=[150, 110]), 7, 8, ("random", 5),
         "per_user", "hbm"),
    "bs3x5_ue2x2_K64_table_dipole_host":
        (dict(bs_shape=[3, 5], ue_shape=[2, 2], selected=list(range(64)), bs_pattern="halfwave-dipole", bs_spacing=0.7), 7, 8,
         ("random", 4), ("table", 2), "host"),
    "bs8x8_ue2x1_K70_per_user_tr38901_hbm":
        (dict(bs_shape=[8, 8], ue_shape=[2, 1], subcarriers=128, selected=list(range(3, 73)), bs_pattern="tr38901",
              bs_rot=[0, 10, -30]), 7, 8, "dft", "per_user", "hbm"),
}

# name -> (changes of BASE, users, loaded paths, codebook, group width G, snr_db, rays, power shift in dB)
MU_CASES = {
    "G1_ue1x1_K1_P3_snr10":
        (dict(selected=[5], num_paths=3), 9, 4, ("random", 4), 1, 10.0, "host", 85.0),
    "G2_ue2x1_K64_P25_snr30":
        (dict(bs_shape=[4, 2], ue_shape=[2, 1], selected=list(range(64)), num_paths=25), 13, 25, ("random", 6), 2, 30.0, "hbm", 62.0),
    "G4_ue2x2_K70_P32_snr-10":
        (dict(bs_shape=[8, 8], ue_shape=[2, 2], subcarriers=128, selected=list(range(3, 73)), num_paths=32, bs_rot=[0, 10, -30]),
         14, 32, "dft", 4, -10.0, "host", 112.0),
    "G8_ue4x2_K130_P25_snr10":
        (dict(bs_shape=[3, 5], ue_shape=[4, 2], subcarriers=256, selected=list(range(0, 260, 2)), num_paths=25,
              bs_pattern="halfwave-dipole"), 21, 25, ("random", 12), 8, 10.0, "hbm", 95.0),
}
NO_PATH_USER, ONE_PATH_USER = 2, 4


def rays(n_ue, L, seed=11, with_doppler=False, shift=POWER_SHIFT_DB):
    """the ray matrices of a case: NO_PATH_USER without a path, ONE_PATH_USER with one, the others with 2 .. L; trailing NaN"""
    from oracle import oracle_np as onp
    r = onp.synth_rays(n_ue, L, seed=seed, all_valid=True, with_doppler=with_doppler)
    counts = np.random.default_rng(seed + 1).integers(min(2, L), L + 1, n_ue)
    counts[NO_PATH_USER], counts[ONE_PATH_USER] = 0, 1
    pad = np.arange(L)[None, :] >= counts[:, None]
    for k, v in r.items():
        if v.shape == (n_ue, L):
            v[pad] = np.nan
    r["power"] = (r["power"] + np.float32(shift)).astype(np.float32)
    return r


def codebook(kind, bs_shape):
    """complex128 [B, M_tx] of a case, rows of unit norm"""
    mh, mv = bs_shape
    m = mh * mv
    if kind == "dft":
        t = np.arange(m)
        y, z = t % mh, t // mh
        return np.exp(-2j * np.pi * (np.outer(y, y) / mh + np.outer(z, z) / mv)) / np.sqrt(m)
    rng = np.random.default_rng(300 + kind[1])
    F = rng.normal(size=(kind[1], m)) + 1j * rng.normal(size=(kind[1], m))
    return F / np.linalg.norm(F, axis=1, keepdims=True)


def view_beams(kind, n_ue, B):
    """the `beams` argument of a view case (None, int [n_ue] or int [J, n_ue]) with a -1 in it where it is an array"""
    if kind == "all":
        return None
    rng = np.random.default_rng(400 + B)
    if kind == "per_user":
        b = rng.integers(0, B, n_ue)
        b[1] = -1
        return b
    b = rng.integers(0, B, (kind[1], n_ue))
    b[1, 3] = -1
    return b


def groups_of(n_ue, G):
    """int [n_groups, G]: the users in a shuffled order, `G` to a row; the last user stays in no group, and where G > 1
    the last row is ragged (one member less, padded with -1) with a second user in no group"""
    order = np.random.default_rng(500 + G).permutation(n_ue)[:-1]
    if G > 1 and len(order) % G == 0:
        order = order[:-1]
    rows = -np.ones((-(-len(order) // G), G), np.int64)
    rows.reshape(-1)[:len(order)] = order
    return rows


def view_setup(name):
    """(case, oracle parameters, (bs_fov, ue_fov), rays, F, beams, where the rays live) of VIEW_CASES[name]"""
    from tests._cases import fov_args, oracle_params
    changes, n, L, cb, beams, place = VIEW_CASES[name]
    case = {**BASE, **changes, "num_paths": L}
    F = codebook(cb, case["bs_shape"])
    return case, oracle_params(case, UE_ROT), fov_args(case), rays(n, L), F, view_beams(beams, n, len(F)), place


def mu_setup(name):
    """(case, oracle parameters, rays, F, beams [n_ue], groups [n_groups, G], snr_db, where the rays live) of MU_CASES[name]"""
    from tests._cases import oracle_params
    changes, n, L, cb, G, snr_db, place, shift = MU_CASES[name]
    case = {**BASE, **changes}
    F = codebook(cb, case["bs_shape"])
    beams = np.random.default_rng(600 + G).integers(0, len(F), n)
    return case, oracle_params(case, UE_ROT), rays(n, L, seed=20 + G, shift=shift), F, beams, groups_of(n, G), snr_db, place
