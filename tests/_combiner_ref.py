"""References of the UE receive combining tests (tests/test_combiner_cpu.py, tests/test_gpu_rx_combiner.py), restated in
NumPy float64 on the NumPy oracle without a line of the package.  A plain module: NumPy only, no torch, no GPU.

    ref[u, q, t, k] = sum_r W[q, r] H_oracle[u, r, t, k]                         einsum('qr,urtk->uqtk', W, H_oracle)
    e[u, q, l]      = sum_r W[q, r] a_rx[u, r, l]                                a_rx: oracle_np.array_response_batch
    power'[u, q, l] = power[u, l] + 10 log10(max(|e|^2, 2^-100))                 the dB value a view stores, in float64

Tolerance of a channel of the view against `ref`, per user and UE beam (derived, not chosen):

    tol[u, q] = TOL_REL max|ref[u, q]| + sum_l |c_l| |e[q, l]| (2 pi 2^-24 + 2^-24 |power'_l| ln 10 / 20)

the project's parity criterion (tests/_cases.py) plus the one extra float32 rounding of the phase - at most half a float32
ulp below 180 degrees, pi 2^-24 rad, doubled as in tests/_time_series_ref.py - and of the power in dB - at most 2^-24 |power'|
dB, which is that times ln 10 / 20 of the amplitude - on a path of modulus |c_l| |e[q, l]|.  |c_l| is that of
tests/_time_series_ref.path_moduli_sum, per path.

Tolerance of a beam-pair amplitude amp[u, q, b] = mean_k |sum_t ref[u, q, t, k] F[b, t]|: the same two terms behind the BS
codebook.  | |a| - |b| | <= |a - b| and a mean of bounds that do not depend on k is the bound, so

    tol_amp[u, q, b] = TOL_REL max over b', k of |sum_t ref[u, q, t, k] F[b', t]| + sum_t |F[b, t]| (second term of tol[u, q])

The power in dBm is rounded to 0.1 dB before the best pair is taken, so the best pair can be any whose rounded power
reaches that of the reference's best pair: two amplitudes that round to the same 0.1 dB differ by at most 0.1 dB."""
from __future__ import annotations

import contextlib
import copy

import numpy as np

from tests._cases import TOL_REL

E2_FLOOR = 2.0 ** -100
ROUNDING_STEP = 10.0 ** (-0.1 / 20.0)          # amplitude ratio of the 0.1 dB the beam powers are rounded to


@contextlib.contextmanager
def oracle(params):
    """the NumPy oracle for `params`: taught the sector pattern (tests/_pattern_ref.py) where a side has it"""
    from oracle import oracle_np as onp
    pats = (params["bs_antenna"]["radiation_pattern"], params["ue_antenna"]["radiation_pattern"])
    if "tr38901" in pats:
        from tests._pattern_ref import patched_oracle
        with patched_oracle() as patched:
            yield patched
    else:
        yield onp


def prepared(rays, params, bs_fov=None, ue_fov=None):
    """`oracle_np.prepare_paths` with the seed every compute_* sets: the rotated, FoV-filtered angles, the powers and the
    resolved UE rotation [n, 3]"""
    with oracle(params) as onp:
        np.random.seed(1001)
        return onp.prepare_paths(rays, copy.deepcopy(params), bs_fov, ue_fov)


def responses(prep, params, W):
    """e [n, Q, L] complex128; 0 where the path has no arrival angle"""
    from oracle import oracle_np as onp
    ue = params["ue_antenna"]
    a_rx = onp.array_response_batch(ue["shape"], ue["spacing"], prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"])
    return np.einsum("qr,url->uql", np.asarray(W, np.complex128), a_rx)


def path_moduli(prep, params):
    """|c_l| [n, P] of the kept paths, 0 where there is none (tests/_time_series_ref.path_moduli_sum, per path)"""
    P = int(params["num_paths"])
    g = np.asarray(prep["_power_linear_ant_gain"], np.float64)[:, :P]
    g = np.where(np.isnan(prep["_aod_el_rot_fov"][:, :P]), np.nan, g)
    if params["freq_domain"]:
        g = g / params["ofdm"]["subcarriers"]
    return np.nan_to_num(np.sqrt(g), nan=0.0)


def combined_moduli_sum(prep, params, W):
    """[n, Q]: sum over the kept paths of |c_l| |e[q, l]|, the path moduli behind the combiner"""
    P = int(params["num_paths"])
    return (path_moduli(prep, params)[:, None, :] * np.abs(responses(prep, params, W))[:, :, :P]).sum(axis=2)


def rounding_term(rays, prep, params, W):
    """[n, Q]: the second term of tol"""
    P = int(params["num_paths"])
    e = np.abs(responses(prep, params, W))[:, :, :P]
    c = path_moduli(prep, params)[:, None, :]
    power = np.asarray(rays["power"], np.float64)[:, None, :P] + 10 * np.log10(np.maximum(e * e, E2_FLOOR))
    per_path = c * e * (2 * np.pi * 2.0 ** -24 + 2.0 ** -24 * np.abs(power) * np.log(10.0) / 20.0)
    return np.nansum(np.where(c > 0, per_path, 0.0), axis=2)


def reference(rays, params, W, bs_fov=None, ue_fov=None):
    """(ref [n, Q, M_tx, K] complex128, tol [n, Q], the rounding term [n, Q]) of the module docstring"""
    with oracle(params) as onp:
        H = onp.compute_channels(rays, params, bs_fov, ue_fov)["channel"]
    ref = np.einsum("qr,urtk->uqtk", np.asarray(W, np.complex128), H.astype(np.complex128))
    second = rounding_term(rays, prepared(rays, params, bs_fov, ue_fov), params, W)
    return ref, TOL_REL * np.abs(ref).max(axis=(2, 3)) + second, second


def single_antenna_channels(rays, params, prep, power, phase, bs_fov=None, ue_fov=None):
    """[n, Q, M_tx, K] complex128: the oracle's channels of the Q * n single-antenna users whose ray matrices are those of
    `rays` tiled, with `power` and `phase` [Q * n, L] in place of the tiled ones; every user keeps the orientation `prep`
    resolved for it"""
    n = rays["power"].shape[0]
    Q = power.shape[0] // n
    tiled = {k: (np.tile(v, (Q,) + (1,) * (v.ndim - 1)) if v.shape[0] == n else v) for k, v in rays.items()}
    tiled["power"], tiled["phase"] = power, phase
    one = copy.deepcopy(params)
    one["ue_antenna"]["shape"] = np.array([1, 1])
    one["ue_antenna"]["rotation"] = np.tile(prep["ue_rotation"], (Q, 1))
    with oracle(one) as onp:
        H = onp.compute_channels(tiled, one, bs_fov, ue_fov)["channel"]
    return H.reshape((Q, n) + H.shape[2:]).transpose(1, 0, 2, 3).astype(np.complex128)


def worst_ratio(X, ref, tol, what=""):
    """every entry of X [n, Q, ...] within tol [n, Q] of ref, exactly ref where tol is 0; returns the worst error / bound"""
    X, ref = np.asarray(X).astype(np.complex128), np.asarray(ref).astype(np.complex128)
    assert X.shape == ref.shape, f"{what}: shape {X.shape} vs {ref.shape}"
    assert np.isfinite(X).all() and np.isfinite(ref).all(), f"{what}: not finite"
    d = np.abs(X - ref).reshape(X.shape[0], X.shape[1], -1).max(axis=2)
    zero = tol == 0
    assert np.all(d[zero] == 0), f"{what}: a user without a path is not zero"
    ratio = float((d[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    return ratio


def pair_amplitudes(ref, F):
    """(amp [n, Q, B] float64, the beam-space peak [n, Q]) of the reference channels behind the BS codebook F [B, M_tx]"""
    Y = np.einsum("uqtk,bt->uqbk", ref, np.asarray(F, np.complex128))
    return np.abs(Y).mean(axis=3), np.abs(Y).max(axis=(2, 3))


def amplitude_tolerance(ref, second, F):
    """tol_amp [n, Q, B] of the module docstring"""
    _, peak = pair_amplitudes(ref, F)
    return TOL_REL * peak[:, :, None] + np.abs(np.asarray(F)).sum(axis=1)[None, None, :] * second[:, :, None]
