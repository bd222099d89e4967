"""References of the angle-delay representation (dmx_channels_angle_delay, k9_angle_delay.hip).  NumPy and the oracle only.

* `adp_from_channel`: the definition - codebook product and `np.fft.ifft` of a channel tensor, complex128.
* `delay_kernel` / `path_factors` / `adp_from_paths`: the closed form per path in float64, from the oracle's own building
  blocks (`oracle_np.prepare_paths`, `array_response_batch`); the per-path factors come back as well, so that a test can ask
  what one path contributes (`amplification`, `drop_delta`, `swap_delta`).
* `dft_codebook`: the orthonormal 2-D DFT codebook, restated.
"""
from __future__ import annotations

import copy

import numpy as np


def dft_codebook(shape):
    """F[by + Mh bz, y + Mh z] = exp(-2j pi (by y / Mh + bz z / Mv)) / sqrt(M), complex128 [M, M]"""
    mh, mv = int(shape[0]), int(shape[1])
    F = np.zeros((mh * mv, mh * mv), np.complex128)
    for bz in range(mv):
        for by in range(mh):
            for z in range(mv):
                for y in range(mh):
                    F[by + mh * bz, y + mh * z] = np.exp(-2j * np.pi * (by * y / mh + bz * z / mv)) / np.sqrt(mh * mv)
    return F


def adp_from_channel(H, F, n_fft, n_taps):
    """X[u, rx, r, t] = ifft(sum_tx F[r, tx] H[u, rx, tx, :], n=n_fft)[:n_taps], complex128; F None: the antenna domain"""
    H = np.asarray(H).astype(np.complex128)
    Y = H if F is None else np.einsum("bt,urtk->urbk", np.asarray(F, np.complex128), H)
    return np.fft.ifft(Y, n=int(n_fft), axis=-1)[..., :int(n_taps)]


def delay_kernel(dn, s0, d, K, N, n_fft, n_taps):
    """D[l, t] = 1/n_fft e^{-j 2pi frac(dn_l s0 / N)} e^{j pi (K-1) r} sin(pi K r) / sin(pi r), r = x - rint(x),
    x = t / n_fft - d dn_l / N; the ratio is K where r = 0.  dn: sample delays [L]; float64 throughout.  [L, n_taps]"""
    dn = np.asarray(dn, np.float64).reshape(-1, 1)
    t = np.arange(int(n_taps), dtype=np.float64).reshape(1, -1)
    x = t / n_fft - d * dn / N
    r = x - np.rint(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(r == 0, float(K), np.sin(np.pi * K * r) / np.sin(np.pi * r))
    ph = dn * s0 / N
    ph = ph - np.rint(ph)
    return np.exp(-2j * np.pi * ph) * np.exp(1j * np.pi * (K - 1) * r) * ratio / n_fft


def uniform(sel):
    """(s0, d, K) of a uniformly spaced selection (a single subcarrier has stride 1)"""
    sel = np.asarray(sel, np.int64).ravel()
    d = int(sel[1] - sel[0]) if sel.size > 1 else 1
    assert d > 0 and np.array_equal(sel, sel[0] + d * np.arange(sel.size)), "the selection is not uniformly spaced"
    return int(sel[0]), d, int(sel.size)


def path_factors(rays, params, F, n_fft, n_taps, bs_fov=None, ue_fov=None, doppler=None):
    """Per user None (no kept path) or (a_rx [M_rx, n], f [R, n], c [n], D [n, n_taps]) of the n kept paths in float64, the
    steps of oracle_np.compute_channels before its sum: X[u] = einsum('il,rl,l,lt->irt', a_rx, f, c, D).  c carries the
    Doppler factor when params['enable_doppler'] and `doppler` is given."""
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
    N, ts = ofdm["subcarriers"], 1 / ofdm["bandwidth"]
    s0, d, K = uniform(ofdm["selected_subcarriers"])
    use_dop = bool(params["enable_doppler"]) and doppler is not None
    out = []
    for u in range(power.shape[0]):
        v = ~np.isnan(power[u])
        t = a_rx[u][:, None, v] * a_tx[u][None, :, v]
        # a path outside the field of view has NaN angles and, as in the reference, an all-zero array response: no term
        v[v] = ~np.isnan(t).any(axis=(0, 1)) & (np.abs(t).max(axis=(0, 1)) > 0) & np.isfinite(delay[u, v]) & np.isfinite(phase[u, v])
        if not v.any():
            out.append(None)
            continue
        pw = np.array(power[u, v], copy=True)
        dn = (delay[u, v] / ts).astype(np.float64)                            # float32 / python float, as channel.py:183
        over = dn >= N                                                       # channel.py:187-189
        pw[over], dn[over] = 0, N
        # the coefficient in the oracle's own precision (complex64 for float32 powers, channel.py:170): what is compared
        # with the definition is the delay kernel, not the rounding of a phase in degrees
        c = (np.sqrt(pw / N) * np.exp(1j * np.deg2rad(phase[u, v]))).astype(np.complex128)
        if use_dop:
            tau = delay[u, v].astype(np.float64)
            vel, acc = doppler["vel"][u, :P][v].astype(np.float64), doppler["acc"][u, :P][v].astype(np.float64)
            c = c * np.exp(-2j * np.pi * doppler["carrier_freq"] * (vel * tau / onp.LIGHTSPEED + acc * tau ** 2 / (2 * onp.LIGHTSPEED)))
        atx = a_tx[u][:, v].astype(np.complex128)
        f = atx if F is None else np.asarray(F, np.complex128) @ atx
        out.append((a_rx[u][:, v].astype(np.complex128), f, c, delay_kernel(dn, s0, d, K, N, n_fft, n_taps)))
    return out


def adp_from_factors(fac, m_rx, n_rows, n_taps):
    if fac is None:
        return np.zeros((m_rx, n_rows, n_taps), np.complex128)
    a_rx, f, c, D = fac
    return np.einsum("il,rl,l,lt->irt", a_rx, f, c, D)


def adp_from_paths(rays, params, F, n_fft, n_taps, **kw):
    """(X [n_ue, M_rx, R, n_taps] complex128 by the closed form, the per-path factors of every user)"""
    facs = path_factors(rays, params, F, n_fft, n_taps, **kw)
    m_rx = int(np.prod(params["ue_antenna"]["shape"]))
    n_rows = int(np.prod(params["bs_antenna"]["shape"])) if F is None else len(F)
    X = np.stack([adp_from_factors(fc, m_rx, n_rows, int(n_taps)) for fc in facs]) if facs else \
        np.zeros((0, m_rx, n_rows, int(n_taps)), np.complex128)
    return X, facs


def amplification(fac, X_u):
    """A[u] = max over entries of sum_l |term_l| / max |X[u]|: how much larger the summands are than the result they leave"""
    a_rx, f, c, D = fac
    s = np.einsum("il,rl,l,lt->irt", np.abs(a_rx), np.abs(f), np.abs(c), np.abs(D))
    return float(s.max() / np.abs(X_u).max())


def drop_delta(fac, l):
    """X without path l, minus X"""
    a_rx, f, c, D = fac
    return -np.einsum("i,r,t->irt", a_rx[:, l], f[:, l], c[l] * D[l])


def swap_delta(fac, l):
    """X with the D rows of paths l and l + 1 exchanged, minus X"""
    a_rx, f, c, D = fac
    dD = D[l + 1] - D[l]
    return np.einsum("i,r,t->irt", a_rx[:, l], f[:, l], c[l] * dD) - np.einsum("i,r,t->irt", a_rx[:, l + 1], f[:, l + 1], c[l + 1] * dD)
