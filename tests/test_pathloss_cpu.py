"""The pathloss reference and case list (tests/_pathloss_ref.py) checked without a GPU: the float64 reference on rows whose
answer is known in closed form, what the case list reaches, the cap on the condition number, and how much of the
tolerance the reference implementation's own float32 formula uses on these cases."""
import numpy as np
import pytest

from tests._pathloss_ref import (DELTA_RANGE, KAPPA_CAP, N_UES, PATH_COUNTS, ROW_KINDS, TOL_DB, cases, f32_pathloss, kind_applies,
                                 ref_pathloss, tolerance)

CASES = cases()
IDS = [c["id"] for c in CASES]


def test_reference_on_closed_forms():
    power = np.array([[-80.0, np.nan, np.nan], [-80.0, -80.0, np.nan], [-100.0, -100.0, -100.0], [np.nan] * 3, [-np.inf] * 3,
                      [-60.0, -np.inf, np.nan]], dtype=np.float32)
    phase = np.array([[37.0, 5.0, np.nan], [10.0, 100.0, 0.0], [0.0, 120.0, -120.0], [0.0] * 3, [10.0, 20.0, 30.0],
                      [90.0, np.nan, 0.0]], dtype=np.float32)
    pl, kappa = ref_pathloss(power, phase, True)
    assert pl[0] == pytest.approx(80.0, abs=1e-12) and kappa[0] == pytest.approx(1.0)
    assert pl[1] == pytest.approx(80.0 - 10 * np.log10(2.0), abs=1e-9) and kappa[1] == pytest.approx(np.sqrt(2.0))   # 90 degrees apart
    assert np.isnan(pl[3]) and np.isnan(pl[4]) and pl[5] == pytest.approx(60.0, abs=1e-12)
    pl, kappa = ref_pathloss(power, phase, False)
    assert pl[1] == pytest.approx(80.0 - 20 * np.log10(2.0), abs=1e-9) and pl[2] == pytest.approx(100.0 - 20 * np.log10(3.0), abs=1e-9)
    assert np.all(kappa[:3] == pytest.approx(1.0)) and np.isnan(pl[3]) and np.isnan(pl[4]) and pl[5] == pytest.approx(60.0, abs=1e-12)
    # NaN only in the phase: skipped when coherent, counted when not
    p, ph = np.array([[-70.0, -70.0]], dtype=np.float32), np.array([[0.0, np.nan]], dtype=np.float32)
    assert ref_pathloss(p, ph, True)[0][0] == pytest.approx(70.0) and ref_pathloss(p, ph, False)[0][0] == pytest.approx(70.0 - 20 * np.log10(2.0))
    # no path at all, and a pair delta degrees off cancellation: |sum| = 2 A sin(delta / 2)
    assert np.isnan(ref_pathloss(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32), True)[0]).all()
    p, ph = np.array([[-80.0, -80.0]], dtype=np.float32), np.array([[-90.0, 89.5]], dtype=np.float32)
    pl, kappa = ref_pathloss(p, ph, True)
    assert kappa[0] == pytest.approx(1 / np.sin(np.deg2rad(0.25)), rel=1e-9)
    assert pl[0] == pytest.approx(80.0 - 20 * np.log10(2 * np.sin(np.deg2rad(0.25))), abs=1e-9)


def test_case_list_reaches_every_edge():
    assert [(c["n_ue"], c["L"]) for c in CASES] == [(n, L) for n in N_UES for L in PATH_COUNTS]
    assert set(N_UES) == {1, 7, 8, 9, 17} and set(PATH_COUNTS) == {0, 1, 2, 31, 32, 33, 64, 65}
    for kind in ROW_KINDS:
        with_kind = [c for c in CASES if kind in c["kinds"]]
        assert {c["L"] for c in with_kind} == {L for L in PATH_COUNTS if kind_applies(kind, L)}, kind
        assert {c["n_ue"] for c in with_kind} >= {7, 9, 17}, kind      # in a launch whose last workgroup is partly idle
    for c in CASES:
        p, ph, L = c["power"], c["phase"], c["L"]
        assert p.shape == ph.shape == (c["n_ue"], L) and p.dtype == ph.dtype == np.float32 and len(c["kinds"]) == c["n_ue"]
        finite = np.isfinite(p)
        assert np.all((p[finite] >= -160) & (p[finite] <= -60) | (p[finite] == -300))
        assert np.all(np.abs(ph[~np.isnan(ph)]) <= 180)
        for u, kind in enumerate(c["kinds"]):
            if kind == "nan_lane0":
                assert np.isnan(p[u, 0]) and not np.isnan(p[u, 1:]).any() and not np.isnan(ph[u]).any()
            elif kind == "nan_phase":
                assert np.isnan(ph[u]).sum() == 1 and not np.isnan(p[u]).any()
            elif kind == "nan_second_trip":
                assert np.isnan(p[u, 32:]).sum() == 1 and not np.isnan(p[u, :32]).any() and not np.isnan(ph[u]).any()
            elif kind == "all_nan":
                assert np.isnan(p[u]).all()
            elif kind == "neg_inf":
                assert np.all(p[u] == -np.inf) and not np.isnan(ph[u]).any()
            elif kind == "one_valid_last":
                assert np.isnan(p[u, :L - 1]).all() and np.isfinite(p[u, L - 1]) and np.isfinite(ph[u, L - 1])
            elif kind == "near_cancel":
                gap = 180.0 - abs(float(ph[u, L - 1]) - float(ph[u, 0]))
                assert p[u, 0] == p[u, L - 1] and DELTA_RANGE[0] * 0.99 <= gap <= DELTA_RANGE[1] * 1.01
                assert np.all(p[u, 1:L - 1] == -300)
            else:
                assert np.isfinite(p[u]).all() and np.isfinite(ph[u]).all()
    deltas = [180.0 - abs(float(c["phase"][u, -1]) - float(c["phase"][u, 0])) for c in CASES for u, k in enumerate(c["kinds"])
              if k == "near_cancel"]
    assert len(deltas) >= 20 and min(deltas) < 0.1 and max(deltas) > 1.0


@pytest.mark.parametrize("coherent", [True, False], ids=["coherent", "incoherent"])
def test_expected_nan_is_exact_and_kappa_is_capped(coherent):
    worst = 0.0
    for c in CASES:
        pl, kappa = ref_pathloss(c["power"], c["phase"], coherent)
        for u, kind in enumerate(c["kinds"]):
            none_valid = (c["L"] == 0 or kind in ("all_nan", "neg_inf") or (c["L"] == 1 and kind == "nan_lane0")
                          or (c["L"] == 1 and kind == "nan_phase" and coherent))
            assert np.isnan(pl[u]) == none_valid, (c["id"], u, kind)
            if not none_valid:
                assert 1.0 <= kappa[u] * (1 + 1e-12) and kappa[u] <= KAPPA_CAP, (c["id"], u, kind, kappa[u])
                worst = max(worst, kappa[u])
                if kind == "near_cancel":
                    assert (kappa[u] > 25) == coherent
    assert (worst > 1000) == coherent                            # the tolerance's scaling is exercised, not only allowed


@pytest.mark.parametrize("coherent", [True, False], ids=["coherent", "incoherent"])
def test_float32_formula_uses_a_quarter_of_the_tolerance_at_most(coherent):
    """So that the float64 reference, not the margin, is what the kernel is compared with"""
    worst = 0.0
    for c in CASES:
        pl, kappa = ref_pathloss(c["power"], c["phase"], coherent)
        f32 = f32_pathloss(c["power"], c["phase"], coherent)
        assert np.array_equal(np.isnan(f32), np.isnan(pl)), c["id"]
        ok = ~np.isnan(pl)
        ratio = np.abs(f32[ok] - pl[ok]) / tolerance(kappa[ok])
        assert np.all(ratio <= 0.25), (c["id"], ratio.max())
        worst = max(worst, ratio.max(initial=0.0))
    assert TOL_DB == 2e-4 and worst > 0
