"""Reference and cases of the pathloss tests (tests/test_pathloss_cpu.py, tests/test_gpu_pathloss.py).

k5_pathloss (Dataset.compute_pathloss): per user g_l = 10^(p_l / 20) [* exp(j deg2rad(phase_l))], paths whose g is NaN
skipped, PL = -20 log10 |sum g|, NaN where the sum is 0.  `ref_pathloss` states that in float64 on the float32 inputs and
returns the row's condition number kappa = sum |g| / |sum g| with it: a float32 evaluation loses about kappa times its
own rounding, so the tolerance is the project's 2e-4 dB times max(1, kappa) per user.

NaN is expected only where it is exact by construction: no valid path, no path at all, or every valid path at -inf dB.
Nearly cancelling rows are pairs of equal power whose phases are 180 - delta degrees apart, delta in [0.03, 2]; no exact
zero is built from cancelling phases (the float32 sine of pi is not 0).
"""
from __future__ import annotations

import functools

import numpy as np

TOL_DB = 2e-4                                                   # the project's pathloss criterion, for a row of kappa <= 1
KAPPA_CAP = 1e4
N_UES = (1, 7, 8, 9, 17)                                        # 8 users per workgroup: one short, full, one over, two and one
PATH_COUNTS = (0, 1, 2, 31, 32, 33, 64, 65)                     # the lane loop advances by 32
ROW_KINDS = ("random", "nan_lane0", "nan_phase", "nan_second_trip", "all_nan", "neg_inf", "one_valid_last", "near_cancel")
DELTA_RANGE = (0.03, 2.0)                                       # degrees off exact cancellation


def ref_pathloss(power, phase, coherent: bool):
    """(PL in dB float64 [n], kappa float64 [n]); NaN / inf kappa where the sum is exactly 0"""
    p, ph = np.asarray(power, dtype=np.float64), np.asarray(phase, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = (10.0 ** (p / 20.0)).astype(np.complex128)
        if coherent:
            g = g * np.exp(1j * np.deg2rad(ph))
        g = np.where(np.isnan(g.real) | np.isnan(g.imag), 0.0, g)
        s = np.abs(g.sum(axis=1))
        pl = np.where(s > 0, -20.0 * np.log10(np.where(s > 0, s, 1.0)), np.nan)
        kappa = np.abs(g).sum(axis=1) / s
    return pl, kappa


def f32_pathloss(power, phase, coherent: bool):
    """The reference implementation's own formula in its own types (float32 / complex64, np.nansum), as the existing
    pathloss tests restate it"""
    power, phase = np.asarray(power, dtype=np.float32), np.asarray(phase, dtype=np.float32)
    with np.errstate(all="ignore"):
        g = np.sqrt(10 ** (power / 10)).astype(np.complex64)
        if coherent:
            g = g * np.exp(1j * np.deg2rad(phase))
        tp = np.abs(np.nansum(g, axis=1)) ** 2
        out = np.full(tp.shape, np.nan, dtype=np.float32)
        out[tp > 0] = -10 * np.log10(tp[tp > 0])
    return out


def tolerance(kappa):
    with np.errstate(all="ignore"):
        return TOL_DB * np.maximum(1.0, np.where(np.isfinite(kappa), kappa, 1.0))


def kind_applies(kind: str, L: int) -> bool:
    need = {"random": 0, "all_nan": 1, "neg_inf": 1, "nan_lane0": 1, "nan_phase": 1, "one_valid_last": 1, "near_cancel": 2,
            "nan_second_trip": 33}
    return L >= need[kind]


@functools.lru_cache(maxsize=None)
def _case(n_ue: int, L: int, turn: int):
    rng = np.random.default_rng(5000 + 100 * n_ue + L)
    power = rng.uniform(-160, -60, (n_ue, L)).astype(np.float32)
    phase = rng.uniform(-180, 180, (n_ue, L)).astype(np.float32)
    kinds = []
    for u in range(n_ue):
        kind = ROW_KINDS[(u + turn) % len(ROW_KINDS)]
        if not kind_applies(kind, L):
            kind = "random"
        kinds.append(kind)
        if kind == "nan_lane0":
            power[u, 0] = np.nan
        elif kind == "nan_phase":                               # skipped when coherent, counted when not
            phase[u, L // 2] = np.nan
        elif kind == "nan_second_trip":
            power[u, rng.integers(32, L)] = np.nan
        elif kind == "all_nan":
            power[u], phase[u] = np.nan, np.nan
        elif kind == "neg_inf":
            power[u] = -np.inf
        elif kind == "one_valid_last":
            power[u, :L - 1], phase[u, :L - 1] = np.nan, np.nan
        elif kind == "near_cancel":                             # lane 0 against the last lane of the last trip
            delta = np.exp(rng.uniform(*np.log(DELTA_RANGE)))
            first = rng.uniform(-180, 0)
            power[u], phase[u, 0], phase[u, L - 1] = -300.0, first, first + 180.0 - delta
            power[u, 0] = power[u, L - 1] = rng.uniform(-120, -60)
    power.setflags(write=False)
    phase.setflags(write=False)
    return power, phase, tuple(kinds)


def cases():
    """[dict(id, n_ue, L, power, phase, kinds)]: every n_ue x L, the row kinds starting one further on in each"""
    out = []
    for n_ue in N_UES:
        for L in PATH_COUNTS:
            power, phase, kinds = _case(n_ue, L, len(out))
            out.append(dict(id=f"n{n_ue}_L{L}", n_ue=n_ue, L=L, power=power, phase=phase, kinds=kinds))
    return out
