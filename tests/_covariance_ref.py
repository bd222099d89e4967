"""References of the covariance tests (tests/test_covariance_cpu.py, tests/test_gpu_covariance.py): the definition as an
einsum of the oracle's channel tensor, and the closed form in the per-path quantities that k6_covariance.hip evaluates,
restated in float64 NumPy from the oracle's own building blocks.  A plain module: no torch, no GPU."""
from __future__ import annotations

import copy

import numpy as np

SIDES = ("tx", "rx")


def cov_from_channel(H, side):
    """R[u] of the definition from H [n, M_rx, M_tx, K], in complex128"""
    H = np.asarray(H).astype(np.complex128)
    n, m_rx, m_tx, K = H.shape
    if side == "tx":
        return np.einsum("urik,urjk->uij", H, H.conj()) / (m_rx * K)
    return np.einsum("uitk,ujtk->uij", H, H.conj()) / (m_tx * K)


def cov_closed_form(rays, params, side, bs_fov=None, ue_fov=None):
    """R = A Q A^H with Q[l,l'] = c_l conj(c_l') S[l,l'] D[l,l'] per user, float64, from prepare_paths,
    array_response_batch and ofdm_path_gains (the steps of oracle_np.compute_channels before its sum over paths)."""
    from oracle import oracle_np as onp
    params = copy.deepcopy(params)
    np.random.seed(1001)
    prep = onp.prepare_paths(rays, params, bs_fov, ue_fov)
    P = int(params["num_paths"])
    bs, ue, ofdm = params["bs_antenna"], params["ue_antenna"], params["ofdm"]
    a_tx = onp.array_response_batch(bs["shape"], bs["spacing"], prep["_aod_el_rot_fov"], prep["_aod_az_rot_fov"])[..., :P]
    a_rx = onp.array_response_batch(ue["shape"], ue["spacing"], prep["_aoa_el_rot_fov"], prep["_aoa_az_rot_fov"])[..., :P]
    power = prep["_power_linear_ant_gain"][..., :P]
    delay, phase = rays["delay"][..., :P], rays["phase"][..., :P]
    a_out, a_avg = (a_tx, a_rx) if side == "tx" else (a_rx, a_tx)
    n, M = power.shape[0], a_out.shape[1]
    K = len(ofdm["selected_subcarriers"])
    R = np.zeros((n, M, M), dtype=np.complex128)
    valid = ~np.isnan(power)
    for u in range(n):
        v = valid[u]
        if not v.any():
            continue
        g = onp.ofdm_path_gains(power[u, v], delay[u, v], phase[u, v], ofdm).astype(np.complex128)      # c_l g[l,k]
        ao, aa = a_out[u][:, v].astype(np.complex128), a_avg[u][:, v].astype(np.complex128)
        ok = ~(np.isnan(ao).any(axis=0) | np.isnan(aa).any(axis=0) | np.isnan(g).any(axis=1))
        g, ao, aa = g[ok], ao[:, ok], aa[:, ok]
        D = g @ g.conj().T / K                              # c_l conj(c_l') D[l,l']
        S = aa.T @ aa.conj() / aa.shape[0]                  # S[l,l']
        R[u] = ao @ (D * S) @ ao.conj().T
    return R


def cov_err(R, Rref):
    """per user: max|R - Rref| and max|Rref|"""
    n = Rref.shape[0]
    d = np.abs(np.asarray(R).astype(np.complex128) - Rref).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    peak = np.abs(Rref).reshape(n, -1).max(axis=1) if n else np.zeros(0)
    return d, peak
