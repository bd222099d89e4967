"""Reference and error bounds of the angle-delay power matrix and the delay profile (DMX_FLAG_ANGLE_DELAY_POWER,
DMX_FLAG_ANGLE_DELAY_PROFILE; k9_angle_delay.hip, OUT = 1 and 2).  NumPy only.

Reference.  From X_ref [n, M_rx, R, T], the complex128 definition of tests/_angle_delay_ref.py `adp_from_channel`:

    P_ref[u, r, t] = sum_rx |X_ref[u, rx, r, t]|^2          p_ref[u, t] = sum_r P_ref[u, r, t]            (float64)

Bound on P.  The project's criterion on the complex output is per user: |X - X_ref| <= b_u = TOL_REL max |X_ref[u]| for
every entry of user u.  For one entry X = X_ref + delta with |delta| <= b_u,

    | |X|^2 - |X_ref|^2 | = | 2 Re(conj(X_ref) delta) + |delta|^2 | <= 2 |X_ref| b_u + b_u^2,

and the sum over rx adds these.  The kernel then forms the sum in float32: a square re^2 + im^2 as fmaf(im, im, re re) is two
roundings, and adding M_rx non-negative terms one after the other is M_rx - 1 more on partial sums that never exceed the
total, so the computed sum is within (M_rx + 1) u of the exact one, u = 2^-24; one more u for the terms of second order and
for the float32 store leaves (M_rx + 2) u P_ref.  Together

    tol_P[u, r, t] = sum_rx (2 |X_ref| b_u + b_u^2) + (M_rx + 2) 2^-24 P_ref.

Bound on p.  The row sum carries every tol_P through (the triangle inequality) and is a float32 sum of n_rows non-negative
terms in some fixed order - n_rows - 1 roundings, each on a partial sum below the total, whatever the order or grouping -
so with the same allowance

    tol_p[u, t] = sum_r tol_P[u, r, t] + (n_rows + 1) 2^-24 p_ref.

Both bounds come from the complex criterion and the number format alone; nothing in them is measured on the code under
test.  A value below FLT_MIN may come out as 0: FLT_MIN is added where a test compares at the rounding terms alone.

What gives the criterion its meaning is in tests/test_angle_delay_power_cpu.py: on the equal-power cases a dropped path or an
exchanged pair of delay rows moves P_ref and p_ref by at least ten times their bounds, and rounding X_ref to complex64
(what a correct complex call may return at best) stays inside tol_P.
"""
from __future__ import annotations

import numpy as np

from tests._cases import TOL_REL

U32 = 2.0 ** -24                             # unit roundoff of float32
FLT_MIN = float(np.finfo(np.float32).tiny)


def power_from_adp(X):
    """(P [n, R, T], p [n, T]) in float64 of a complex [n, M_rx, R, T] tensor: the definition"""
    X = np.asarray(X)
    a = X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2
    P = a.sum(axis=1)
    return P, P.sum(axis=1)


def power_bounds(X_ref):
    """(tol_P [n, R, T], tol_p [n, T]) of the module's derivation for the reference tensor X_ref [n, M_rx, R, T]"""
    X_ref = np.asarray(X_ref, np.complex128)
    n, m_rx, n_rows, _ = X_ref.shape
    P_ref, p_ref = power_from_adp(X_ref)
    b = TOL_REL * (np.abs(X_ref).reshape(n, -1).max(axis=1) if X_ref[0:1].size else np.zeros(n))
    b = b.reshape(n, 1, 1, 1)
    tol_P = (2 * np.abs(X_ref) * b + b ** 2).sum(axis=1) + (m_rx + 2) * U32 * P_ref
    tol_p = tol_P.sum(axis=1) + (n_rows + 1) * U32 * p_ref
    return tol_P, tol_p


_REF = {}


def case_power_ref(c):
    """(P_ref, p_ref, tol_P, tol_p) of a case of tests/_angle_delay_cases.py: computed once, shared and left unchanged"""
    if c["id"] not in _REF:
        from tests._angle_delay_cases import case_inputs
        X_ref = case_inputs(c)[3]
        out = power_from_adp(X_ref) + power_bounds(X_ref)
        for a in out:
            a.setflags(write=False)
        _REF[c["id"]] = out
    return _REF[c["id"]]


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the entries with tol > 0; entries with tol == 0 (a user without a path) have to be equal"""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    err = np.abs(got - ref)
    live = tol > 0
    assert (err[~live] == 0).all(), "an entry of a user without a path differs from the reference"
    return float((err[live] / tol[live]).max()) if live.any() else 0.0
