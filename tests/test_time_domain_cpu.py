"""CPU tests of the time-domain acceptance criterion and of the cases tests/test_gpu_time_domain.py runs.

1. `assert_taps_close` (tests/_cases.py) holds every (user, slot) to its own peak; `assert_channel_close` holds it to the
   user's peak, which in the time domain - one path per slot, path powers spread over 80 dB - lets a weak tap be wrong by
   half its amplitude.  The first test shows two such corruptions pass the old criterion and fail the new one.
2. The input condition of the GPU test: on every isotropic case the two independent CPU restatements (NumPy oracle, C twin)
   agree per slot at a tenth of the bound the kernels are held to.
3. `td_form` (tests/_td_cases.py) restates `launch_channels_td`'s choice of kernel; it is tied to the launcher's text here
   and each case's intended form is asserted, so no case can drift to another kernel unnoticed.
"""
import os
import re

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests._cases import TOL_REL, assert_channel_close, assert_taps_close, oracle_params
from tests._td_cases import (TD_BY_ID, TD_CASES, TD_TABLE_BYTES, is_isotropic, td_form, td_fov, td_rays, td_reference,
                             td_shape, td_ue_rot)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO = [c for c in TD_CASES if is_isotropic(c)]


def test_per_slot_criterion_rejects_what_the_per_user_one_accepts():
    """One user with a -60 dBW path and two paths 100 dB and more below it (ray tracers do report such paths): a 0.3 rad
    phase error on the weakest tap, and the two weak taps in each other's slots, are 3e-6 and at most 1.4e-5 of the user's
    peak - inside the per-user bound - and 0.3 and more of the taps themselves."""
    from oracle import oracle_np as onp
    c = TD_BY_ID["holes_mid"]
    rays = onp.synth_rays(c["n"], c["L"], seed=c["seed"], all_valid=True)
    u = 3
    rays["power"][u, :3] = [-60.0, -160.0, -166.0]
    rays["power"][u, 3:] = np.minimum(rays["power"][u, 3:], -70.0)
    ref = onp.compute_channels(rays, oracle_params(c, td_ue_rot(c)))["channel"]
    assert ref.dtype == np.complex64
    peak = np.abs(ref[u]).max(axis=(0, 1))
    assert int(np.argmax(peak)) == 0 and int(np.argmin(peak)) == 2 and peak[1] < 1.1e-5 * peak[0]

    assert_channel_close(ref.copy(), ref)
    assert assert_taps_close(ref.copy(), ref) == 0.0

    rotated = ref.copy()
    rotated[u, :, :, 2] *= np.complex64(np.exp(0.3j))                   # a wrong steering phase on the weakest tap
    swapped = ref.copy()
    swapped[u, :, :, 1], swapped[u, :, :, 2] = ref[u, :, :, 2], ref[u, :, :, 1]    # a wrong slot index on two weak taps
    for name, bad in (("rotated", rotated), ("swapped", swapped)):
        assert not np.array_equal(bad, ref)
        assert_channel_close(bad, ref, what=name)                       # invisible at the user's peak
        with pytest.raises(AssertionError, match=f"worst user {u} slot"):
            assert_taps_close(bad, ref, what=name)


def test_per_slot_criterion_zero_slots_shapes_and_nan():
    ref = td_reference(TD_BY_ID["fov_iso"])["channel"]
    peak = np.abs(ref).max(axis=(1, 2))
    assert (peak == 0).any() and (peak > 0).any()
    u, s = np.argwhere(peak == 0)[0]
    neg = ref.copy()
    neg[u, :, :, s] = np.complex64(complex(-0.0, -0.0))                  # either sign of zero passes
    assert_taps_close(neg, ref)
    tiny = ref.copy()
    tiny[u, 0, 0, s] = 1e-30
    with pytest.raises(AssertionError, match="all-zero reference"):
        assert_taps_close(tiny, ref)
    with pytest.raises(AssertionError, match="shape"):
        assert_taps_close(ref[:, :, :, :-1], ref)
    nan = ref.copy()
    nan[0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        assert_taps_close(nan, ref)
    # the returned figure is error / bound of the worst tap
    u, s = np.argwhere(peak > 0)[0]
    off = ref.copy()
    off[u, 0, 0, s] += np.complex64(0.5 * TOL_REL * peak[u, s])
    assert assert_taps_close(off, ref) == pytest.approx(0.5, rel=1e-2)


@pytest.mark.parametrize("c", ISO, ids=[c["id"] for c in ISO])
def test_the_two_cpu_restatements_agree_per_slot(c):
    """The reference's own error: NumPy oracle against dmx_cpu_path_prep + dmx_cpu_channels_td at TOL_REL / 10."""
    ref = td_reference(c)
    bs_fov, ue_fov = td_fov(c)
    twin = oc.compute_channels(td_rays(c), oracle_params(c, td_ue_rot(c)), bs_fov=bs_fov, ue_fov=ue_fov)
    m_rx, m_tx, P = td_shape(c)
    assert ref["channel"].shape == (c["n"], m_rx, m_tx, P) and ref["channel"].dtype == np.complex64
    worst = assert_taps_close(twin["channel"], ref["channel"], tol_rel=TOL_REL / 10, what=c["id"])
    print(f"{c['id']}: C twin against NumPy oracle, worst per-slot error / (TOL_REL / 10 * slot peak) = {worst:.3e}")
    np.testing.assert_array_equal(twin["los"], ref["los"])
    np.testing.assert_array_equal(twin["num_paths"], ref["num_paths"])


def test_cases_are_not_blind():
    """What the cases are for is in the reference tensors: weak taps, zero slots in the middle, every kept count."""
    frac = []
    for c in ISO:
        peak = np.abs(td_reference(c)["channel"]).max(axis=(1, 2))
        nz = peak > 0
        if nz.any():
            frac.append(float((peak[nz] < 1e-2 * peak.max(axis=1, keepdims=True).repeat(peak.shape[1], 1)[nz]).mean()))
    assert max(frac) > 0.1, "no case has taps far below its user's peak"
    ref = td_reference(TD_BY_ID["plain_holes_counts"])
    P = 32
    assert (np.abs(ref["channel"]).max(axis=(1, 2)) > 0).sum(axis=1).tolist() == [0, 1, P - 1, P, P, 1, 0, P - 1]
    fov = td_reference(TD_BY_ID["fov_iso"])
    peak = np.abs(fov["channel"]).max(axis=(1, 2))
    assert any((peak[u, :-1] == 0).any() and (peak[u, 1:][peak[u, :-1] == 0] > 0).any() for u in range(len(peak))), \
        "fov_iso: no masked path in front of a kept one"
    assert not fov["_fov_mask"].all(), "fov_iso: nothing is outside the FoV"
    # the dipole gain of a masked (NaN) zenith angle is 0, so the path keeps its slot there too, with a zero power
    pk = np.abs(td_reference(TD_BY_ID["fov_dipole"])["channel"]).max(axis=(1, 2))
    np.testing.assert_array_equal(pk[peak == 0], 0)


def test_td_form_rule_and_the_launchers_text():
    src = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k4_channel_td.hip")).read()
    body = src[src.index("int launch_channels_td("):]
    assert TD_TABLE_BYTES == 64 * 1024
    assert re.search(r"smem\s*=\s*\(size_t\)\(a\.m_rx \+ a\.m_tx\) \* ws\.P \* 8;", body)
    assert re.search(r"tab\s*=\s*smem <= 64 \* 1024;", body)
    assert re.search(r"pairs\s*=\s*\(\(size_t\)a\.m_rx \* a\.m_tx \* ws\.P\) % 2 == 0 && \(\(uintptr_t\)out % 16\) == 0", body)
    assert "!tab ? k4_td : (pairs ? k4_td_tab<true> : k4_td_tab<false>)" in body
    # the rule at its edges
    assert td_form(1, 255, 32) == "tab_pairs" and td_form(1, 256, 32) == "plain"
    assert td_form(1, 1, 4096) == "tab_pairs" and td_form(1, 1, 4097) == "plain"
    assert td_form(3, 35, 7) == "tab_single" and td_form(3, 35, 7, out_aligned16=False) == "tab_single"
    assert td_form(2, 40, 9) == "tab_pairs" and td_form(2, 40, 9, out_aligned16=False) == "tab_single"
    assert td_form(1, 256, 32, out_aligned16=False) == "plain"


@pytest.mark.parametrize("c", TD_CASES, ids=[c["id"] for c in TD_CASES])
def test_each_case_reaches_its_form(c):
    assert td_form(*td_shape(c)) == c["form"]


def test_every_form_and_the_table_limit_are_covered():
    assert {c["form"] for c in TD_CASES} == {"plain", "tab_pairs", "tab_single"}
    m_rx, m_tx, P = td_shape(TD_BY_ID["tab_limit_17x15_P32"])
    assert (m_rx + m_tx) * P * 8 == TD_TABLE_BYTES
    m_rx, m_tx, P = td_shape(TD_BY_ID["plain_16x16_P32"])
    assert (m_rx + m_tx) * P * 8 == TD_TABLE_BYTES + 256
