"""Cases of the UE receive combining tests (tests/test_combiner_cpu.py, tests/test_gpu_rx_combiner.py).  A plain module:
NumPy and the oracle only, nothing of deepmimo_amd, no torch.

7 users x 8 loaded paths, BS 4 x 2, N = 64 subcarriers; user 2 has no path, user 4 a single one.  Every case names a UE
array, a subcarrier selection of K = 1, 5 or 64, a UE codebook of Q = 1, 3 (a slice that is not square) or M_rx rows, a BS
codebook of B = 1, 5 or 33 beams, how the UE is rotated, and what the GPU test runs it with: the kernel variant (or the
single pass), where the rays live, and the output type."""
from __future__ import annotations

import numpy as np

N_UE, L = 7, 8
PATH_COUNTS = (8, 5, 0, 3, 1, 8, 2)
NO_PATH_USER, ONE_PATH_USER = 2, 4

BASE = dict(bs_shape=[4, 2], ue_shape=[2, 2], bs_spacing=0.5, ue_spacing=0.5, bs_rot=[0, 0, 0], bs_pattern="isotropic",
            ue_pattern="isotropic", num_paths=L, freq_domain=1, subcarriers=64, selected=[0], bandwidth=10e6, rx_filter=0,
            bs_fov=None, ue_fov=None)
_K5 = [0, 3, 7, 20, 63]
_K64 = list(range(64))
_FIXED_ROT = np.array([10, -20, 30])
_PER_USER_ROT = np.random.default_rng(3).uniform(-60, 60, (N_UE, 3))
_ROT_RANGE = np.array([[-30, 30], [-10, 10], [0, 360]])

# name -> (changes of BASE, UE rotation, UE codebook: "dft" | "one" | ("random", Q), B, what the GPU test runs it with)
# route: "direct" the single pass (config single_pass = True), else the fd_kernel_variant of the view's channel call
CASES = {
    "ue2x2_K1_Q4_B1_fixed_rot_single_pass":
        (dict(selected=[0]), _FIXED_ROT, "dft", 1, dict(route="direct", rays="host", output="numpy")),
    "ue2x2_K64_Q3_B33_per_user_rot_folded":
        (dict(selected=_K64), _PER_USER_ROT, ("random", 3), 33, dict(route=12, rays="hbm", output="torch")),
    "ue3x1_K64_Q3_B5_rot_range_matrix_core":
        (dict(selected=_K64, ue_shape=[3, 1]), _ROT_RANGE, "dft", 5, dict(route=2, rays="host", output="numpy")),
    "ue3x1_K5_Q1_B5_ue_fov_vector":
        (dict(selected=_K5, ue_shape=[3, 1], ue_fov=[150, 100]), _FIXED_ROT, ("random", 1), 5,
         dict(route=1, rays="host", output="torch")),
    "ue1x1_K5_Q1_B33_identity":
        (dict(selected=_K5, ue_shape=[1, 1]), np.zeros(3), "one", 33, dict(route=0, rays="host", output="numpy")),
    "ue2x2_K5_Q3_B5_dipole_per_user_rot":
        (dict(selected=_K5, ue_pattern="halfwave-dipole"), _PER_USER_ROT, ("random", 3), 5,
         dict(route=0, rays="hbm", output="numpy")),
    "ue2x2_K64_Q4_B1_tr38901_ue_fov_rot_range":
        (dict(selected=_K64, ue_pattern="tr38901", ue_fov=[180, 120], ue_spacing=0.7), _ROT_RANGE, ("random", 4), 1,
         dict(route=0, rays="host", output="numpy")),
}


def rays(seed=5, with_doppler=False):
    """the ray matrices of every case: PATH_COUNTS valid paths per user, trailing NaN"""
    from oracle import oracle_np as onp
    r = onp.synth_rays(N_UE, L, seed=seed, all_valid=True, with_doppler=with_doppler)
    pad = np.arange(L)[None, :] >= np.asarray(PATH_COUNTS)[:, None]
    for k, v in r.items():
        if v.shape == (N_UE, L):
            v[pad] = np.nan
    return r


def ue_codebook(name):
    """complex128 [Q, M_rx] of a case"""
    case = {**BASE, **CASES[name][0]}
    kind = CASES[name][2]
    m_rx = int(np.prod(case["ue_shape"]))
    if kind == "one":
        return np.ones((1, 1), np.complex128)
    if kind == "dft":
        mh, mv = case["ue_shape"]
        r = np.arange(m_rx)
        y, z = r % mh, r // mh
        return np.exp(-2j * np.pi * (np.outer(y, y) / mh + np.outer(z, z) / mv)) / np.sqrt(m_rx)
    rng = np.random.default_rng(100 + kind[1])
    W = rng.normal(size=(kind[1], m_rx)) + 1j * rng.normal(size=(kind[1], m_rx))
    return W / np.linalg.norm(W, axis=1, keepdims=True)


def bs_codebook(name):
    """complex128 [B, M_tx] of a case: rows of unit norm with random phases"""
    case = {**BASE, **CASES[name][0]}
    B, m_tx = CASES[name][3], int(np.prod(case["bs_shape"]))
    rng = np.random.default_rng(200 + B)
    return np.exp(2j * np.pi * rng.uniform(size=(B, m_tx))) / np.sqrt(m_tx)


def setup(name):
    """(case, UE rotation, oracle parameters, (bs_fov, ue_fov) of the oracle, rays, W, F) of CASES[name]"""
    from tests._cases import fov_args, oracle_params
    case = {**BASE, **CASES[name][0]}
    ue_rot = CASES[name][1]
    return case, ue_rot, oracle_params(case, ue_rot), fov_args(case), rays(), ue_codebook(name), bs_codebook(name)
