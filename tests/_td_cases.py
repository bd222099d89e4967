"""The time-domain cases shared by tests/test_time_domain_cpu.py (the two CPU restatements against each other) and
tests/test_gpu_time_domain.py (the kernels of k4_channel_td.hip against the NumPy oracle): the smallest shapes that reach
each kernel form and each branch of the table kernel's incremental (slot, tx, rx) advance, and `td_form`, the restated
rule by which `launch_channels_td` picks the kernel."""
from __future__ import annotations

import numpy as np

TD_TABLE_BYTES = 64 * 1024


def td_form(m_rx, m_tx, P, out_aligned16=True):
    """The kernel `launch_channels_td` runs: the table kernels while both steering tables fit 64 KiB of LDS, with 16-byte
    pair stores when a user's element count is even and `out` is 16-byte aligned; the table-free kernel beyond."""
    if (m_rx + m_tx) * P * 8 > TD_TABLE_BYTES:
        return "plain"
    return "tab_pairs" if (m_rx * m_tx * P) % 2 == 0 and out_aligned16 else "tab_single"


def _case(cid, n, L, bs, ue, form, reaches, **kw):
    d = dict(id=cid, n=n, L=L, bs_shape=bs, ue_shape=ue, form=form, reaches=reaches, num_paths=L, bs_rot=[5, -20, 60],
             ue_rot=[0, 0, 0], bs_pattern="isotropic", ue_pattern="isotropic", bs_fov=None, ue_fov=None, bs_spacing=0.5,
             ue_spacing=0.37, freq_domain=0, subcarriers=64, selected=[0], bandwidth=20e6, rx_filter=0, rays="plain",
             all_valid=False, per_user_rot=False, seed=700 + n + L)
    d.update(kw)
    return d


TD_CASES = [
    _case("plain_16x16_P32", 5, 32, [16, 16], [1, 1], "plain", "257 * 32 * 8 = 65792: first shape past the table limit", all_valid=True),
    _case("tab_limit_17x15_P32", 5, 32, [17, 15], [1, 1], "tab_pairs", "exactly 65536 bytes of dynamic LDS, the whole default",
          all_valid=True),
    _case("plain_32x32_ue2x2_P9", 4, 9, [32, 32], [2, 2], "plain", "ry / rz and ty / tz all non-trivial, UE rotation",
          ue_rot=[10, 20, 30]),
    _case("plain_holes_counts", 8, 32, [16, 16], [1, 1], "plain", "kept counts 0, 1, P - 1, P", rays="kept_counts"),
    _case("pairs_odd_P", 9, 9, [8, 5], [2, 1], "tab_pairs", "720 elements: second step, pairs straddle slot, tx and rx boundaries"),
    _case("single_odd", 9, 7, [7, 5], [3, 1], "tab_single", "735 elements, odd: three 256-steps"),
    _case("pairs_P1", 9, 1, [24, 12], [2, 1], "tab_pairs", "P = 1: every element wraps the slot counter"),
    _case("mtx1", 9, 64, [1, 1], [3, 3], "tab_pairs", "M_tx = 1, 576 elements, one user per wave in stage 1"),
    _case("mrx1_P300", 6, 300, [2, 1], [1, 1], "tab_pairs", "P = 300 > 256: step shorter than a slot row"),
    _case("P_lt_L", 12, 25, [8, 4], [2, 2], "tab_pairs", "num_paths = 10 < L: slot count is min(num_paths, L)", num_paths=10),
    _case("holes_mid", 20, 25, [6, 3], [2, 1], "tab_pairs", "NaN holes inside rows: compaction to the front, in path order",
          rays="holes"),
    _case("fov_iso", 20, 12, [4, 2], [2, 1], "tab_pairs", "a path outside the FoV keeps its slot with zeros", bs_fov=[150, 100]),
    _case("fov_dipole", 20, 12, [4, 2], [2, 1], "tab_pairs", "dipole BS: a masked path has gain 0 and keeps its slot; held to the user's peak",
          bs_fov=[150, 100], bs_pattern="halfwave-dipole"),
    _case("per_user_rot", 20, 9, [5, 3], [1, 3], "tab_single", "per-user UE rotation, 405 elements", per_user_rot=True),
]
TD_BY_ID = {c["id"]: c for c in TD_CASES}


def is_isotropic(c):
    return c["bs_pattern"] == "isotropic" and c["ue_pattern"] == "isotropic"


def td_shape(c):
    """(M_rx, M_tx, P) of a case"""
    return (c["ue_shape"][0] * c["ue_shape"][1], c["bs_shape"][0] * c["bs_shape"][1], min(c["num_paths"], c["L"]))


def td_rays(c):
    from oracle import oracle_np as onp
    rays = onp.synth_rays(c["n"], c["L"], seed=c["seed"], all_valid=c["all_valid"] or c["rays"] == "kept_counts")
    if c["rays"] == "holes":                                   # NaN in the middle of a row, the same entries of every field
        hole = np.random.default_rng(3).uniform(size=rays["power"].shape) < 0.2
        for k in onp.RAY_KEYS:
            rays[k][hole] = np.nan
    if c["rays"] == "kept_counts":                             # users with 0 / 1 / P - 1 / P kept paths
        P = min(c["num_paths"], c["L"])
        for u, cnt in enumerate([0, 1, P - 1, P, P, 1, 0, P - 1]):
            for k in onp.RAY_KEYS:
                rays[k][u, cnt:] = np.nan
    return rays


def td_ue_rot(c):
    if not c["per_user_rot"]:
        return np.array(c["ue_rot"])
    return np.random.default_rng(11).uniform(-180, 180, (c["n"], 3))


def td_fov(c):
    """(bs_fov, ue_fov) as Dataset.apply_fov stores them: both, or neither"""
    if c["bs_fov"] is None and c["ue_fov"] is None:
        return None, None
    return (np.array([360, 180]) if c["bs_fov"] is None else np.array(c["bs_fov"]),
            np.array([360, 180]) if c["ue_fov"] is None else np.array(c["ue_fov"]))


_REF = {}


def td_reference(c):
    """oracle_np.compute_channels of the case, computed once per process and shared (callers do not modify it)"""
    if c["id"] not in _REF:
        from oracle import oracle_np as onp
        from tests._cases import oracle_params
        bs_fov, ue_fov = td_fov(c)
        _REF[c["id"]] = onp.compute_channels(td_rays(c), oracle_params(c, td_ue_rot(c)), bs_fov=bs_fov, ue_fov=ue_fov)
    return _REF[c["id"]]
