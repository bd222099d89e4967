"""The time-domain kernels (k4_channel_td.hip: k4_td_tab<true>, k4_td_tab<false>, k4_td) on the GPU, tap by tap.

Reference: oracle_np.compute_channels in float64, stored as complex64.  Criterion: `assert_taps_close` (tests/_cases.py) -
every (user, slot) within TOL_REL = 5e-5 of that slot's own peak, all-zero slots exactly zero.  The cases (tests/_td_cases.py)
are the smallest shapes that reach each kernel form and each carry of the table kernel's incremental index advance; which
kernel a case runs is asserted with `td_form`, which tests/test_time_domain_cpu.py ties to the launcher's text.  The one case
with a half-wave dipole keeps the per-user criterion (the gain is ill-conditioned near its nulls, tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

from tests._cases import TOL_REL, assert_channel_close, assert_taps_close
from tests._td_cases import TD_BY_ID, TD_CASES, is_isotropic, td_form, td_fov, td_rays, td_reference, td_shape, td_ue_rot

pytestmark = pytest.mark.gpu

FORM_CASE = {"tab_pairs": "pairs_odd_P", "tab_single": "single_odd", "plain": "plain_32x32_ue2x2_P9"}
SENTINEL = complex(-12345.5, 54321.25)
WORST = {}                                                     # form -> (worst ratio to the bound, case)


def _dm_params(c):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(c["bs_shape"]), np.array(c["ue_shape"])
    p.bs_antenna.spacing, p.ue_antenna.spacing = c["bs_spacing"], c["ue_spacing"]
    p.bs_antenna.rotation = np.array(c["bs_rot"])
    p.ue_antenna.rotation = np.array([0, 0, 0]) if c["per_user_rot"] else np.array(c["ue_rot"])
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = c["bs_pattern"], c["ue_pattern"]
    p.num_paths, p.freq_domain = c["num_paths"], 0
    return p.validate(c["n"])


def _prepare(c, want_side="light", adaptive_terms=False):
    from deepmimo_amd.engine import ChannelEngine
    eng = ChannelEngine(0)
    bs_fov, ue_fov = td_fov(c)
    kw = dict(bs_fov=bs_fov, ue_fov=ue_fov)
    if c["per_user_rot"]:
        kw["ue_rotation_per_user"] = np.ascontiguousarray(td_ue_rot(c), dtype=np.float64)
    prep = eng.prepare(eng.upload_rays(td_rays(c)), _dm_params(c), want_side=want_side, adaptive_terms=adaptive_terms, **kw)
    return eng, prep


def _bits(t):
    import torch
    return torch.view_as_real(t).view(torch.int32)


def _guarded(c, guard):
    """(whole allocation, the [n, M_rx, M_tx, P] view `guard` elements into it), sentinel-filled"""
    import torch
    m_rx, m_tx, P = td_shape(c)
    size = c["n"] * m_rx * m_tx * P
    big = torch.full((guard + size + guard,), SENTINEL, dtype=torch.complex64, device="cuda")
    return big, big[guard:guard + size].view(c["n"], m_rx, m_tx, P)


@pytest.mark.parametrize("c", TD_CASES, ids=[c["id"] for c in TD_CASES])
def test_taps_against_the_oracle(c):
    """Each case's branch is the `reaches` text of tests/_td_cases.py"""
    import torch
    eng, prep = _prepare(c)
    H = eng.channels(prep)
    torch.cuda.synchronize()
    assert H.data_ptr() % 16 == 0 and td_form(*td_shape(c), out_aligned16=True) == c["form"]
    ref = td_reference(c)
    if is_isotropic(c):
        ratio = assert_taps_close(H.cpu().numpy(), ref["channel"], what=c["id"])
        print(f"{c['id']} ({c['form']}): worst per-slot error / (TOL_REL * slot peak) = {ratio:.3e}")
        if ratio > WORST.get(c["form"], (-1.0, ""))[0]:
            WORST[c["form"]] = (ratio, c["id"])
    else:
        err = assert_channel_close(H.cpu().numpy(), ref["channel"], what=c["id"])
        print(f"{c['id']} ({c['form']}): worst error / user peak = {err:.3e} (per-user criterion)")
    np.testing.assert_array_equal(prep.side["los"].cpu().numpy(), ref["los"])
    np.testing.assert_array_equal(prep.side["num_paths"].cpu().numpy(), ref["num_paths"])


@pytest.mark.parametrize("cid", ["pairs_odd_P", "plain_16x16_P32"])
def test_unaligned_output_takes_single_stores(cid):
    """`out` one complex64 element into an allocation: 8-byte aligned only, so the table kernel runs its single-store form
    (the table-free kernel has one form).  The same bits as the aligned launch; the element before and the guard after stay."""
    import torch
    c = TD_BY_ID[cid]
    eng, prep = _prepare(c, want_side=False)
    aligned = eng.channels(prep)
    big, out = _guarded(c, 1)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    assert td_form(*td_shape(c), out_aligned16=False) == ("plain" if c["form"] == "plain" else "tab_single")
    eng.channels(prep, out=out)
    torch.cuda.synchronize()
    assert bool(big[0] == SENTINEL) and bool(big[-1] == SENTINEL), "write outside the output tensor"
    assert torch.equal(_bits(out), _bits(aligned))


@pytest.mark.parametrize("form", sorted(FORM_CASE))
def test_guard_regions_and_user_sub_range(form):
    import torch
    c = TD_BY_ID[FORM_CASE[form]]
    assert c["form"] == form
    eng, prep = _prepare(c, want_side=False)
    whole = eng.channels(prep)
    guard = 1 << 16
    big, out = _guarded(c, guard)
    assert out.data_ptr() % 16 == 0
    eng.channels(prep, out=out)
    torch.cuda.synchronize()
    assert bool((big[:guard] == SENTINEL).all()) and bool((big[-guard:] == SENTINEL).all()), "write outside the output tensor"
    assert torch.equal(_bits(out), _bits(whole))
    big.fill_(SENTINEL)
    b, cnt = 2, c["n"] - 3
    # rows of an odd element count start 8-byte aligned at odd users: the launcher then takes the single-store form
    per_user = int(np.prod(td_shape(c)))
    assert td_form(*td_shape(c), out_aligned16=(b * per_user) % 2 == 0) == form
    eng.channels(prep, out=out[b:b + cnt], user_begin=b, user_count=cnt)
    torch.cuda.synchronize()
    assert bool((big[:guard] == SENTINEL).all()) and bool((big[-guard:] == SENTINEL).all())
    assert bool((out[:b] == SENTINEL).all()) and bool((out[b + cnt:] == SENTINEL).all()), "a user outside the range written"
    assert torch.equal(_bits(out[b:b + cnt]), _bits(whole[b:b + cnt]))


def test_adaptive_flag_keeps_path_order():
    """DMX_FLAG_ADAPTIVE_TERMS orders the records by amplitude for the frequency domain only; the time-domain slots keep the
    path order (include/deepmimo_amd.h, launch_path_prep)."""
    import torch
    c = TD_BY_ID["holes_mid"]
    eng, plain = _prepare(c, want_side=False)
    H0 = eng.channels(plain)
    eng, flagged = _prepare(c, want_side=False, adaptive_terms=True)
    assert flagged.params_struct.flags == 1
    H1 = eng.channels(flagged)
    torch.cuda.synchronize()
    assert torch.equal(_bits(H1), _bits(H0))


@pytest.mark.parametrize("form", sorted(FORM_CASE))
def test_repeat_launch_is_bit_identical(form):
    import torch
    eng, prep = _prepare(TD_BY_ID[FORM_CASE[form]], want_side=False)
    a = eng.channels(prep)
    b = eng.channels(prep)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))


def test_zz_report_worst_ratio():
    """Last in the file: the worst per-slot ratio per kernel form over the cases that ran (DESIGN.md quotes them)."""
    for form, (ratio, cid) in sorted(WORST.items()):
        print(f"time domain, {form}: worst per-slot error / (TOL_REL * slot peak) = {ratio:.3e} ({cid}); TOL_REL {TOL_REL}")
        assert ratio <= 1.0
