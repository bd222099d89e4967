"""Reference of the radiation-pattern tests (tests/test_pattern_cpu.py, tests/test_gpu_pattern.py): the element pattern of
3GPP TR 38.901 Table 7.3-1 restated in NumPy float64, and the NumPy oracle taught the pattern without a change to it.  A
plain module: NumPy and the oracle only, nothing of deepmimo_amd.

    A_v  = min(12 ((th - pi/2) / b)^2, 30)        b = 65 degrees in radians
    A_h  = min(12 (ph / b)^2, 30)
    gain = 10^((8 - min(A_v + A_h, 30)) / 10)     0 where th or ph is NaN

th / ph are the rotated, FoV-masked zenith / azimuth of a path (`_aod_*_rot_fov`, `_aoa_*_rot_fov` of the oracle).

`patched_oracle()` swaps `oracle_np.prepare_paths` for a wrapper that runs the original with both patterns isotropic and
multiplies `_power_linear_ant_gain` by the float64 gains of the sides that are not; `oracle_np.compute_channels` then sums in
complex128 with that exact float64 power, as it does for the dipole.  No gain is rounded into a float32 dBW value."""
from __future__ import annotations

import contextlib
import copy

import numpy as np

from oracle import oracle_np as onp

BEAMWIDTH = 65.0 * np.pi / 180.0
MAX_ATT_DB = 30.0
GAIN_DBI = 8.0
CAP_ANGLE_DEG = 65.0 * np.sqrt(MAX_ATT_DB / 12.0)        # where one cut alone reaches the cap: 102.77 degrees


def tr38901_gain(th, ph):
    """Linear power gain, float64, of the module docstring"""
    th, ph = np.asarray(th, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    nan = np.isnan(th) | np.isnan(ph)
    t, p = np.where(nan, 0.0, th), np.where(nan, 0.0, ph)
    a_v = np.minimum(12.0 * np.square((t - np.pi / 2) / BEAMWIDTH), MAX_ATT_DB)
    a_h = np.minimum(12.0 * np.square(p / BEAMWIDTH), MAX_ATT_DB)
    g = np.power(10.0, (GAIN_DBI - np.minimum(a_v + a_h, MAX_ATT_DB)) / 10.0)
    return np.where(nan, 0.0, g)


def side_gain(name, th, ph):
    """The gain of one array side: 1.0, the oracle's dipole, or the sector element"""
    if name == "tr38901":
        return tr38901_gain(th, ph)
    return onp.pattern_gain(name, th)


def _prepare_paths_with_patterns(original):
    def prepare_paths(rays, params, bs_fov=None, ue_fov=None):
        pats = (params["bs_antenna"]["radiation_pattern"], params["ue_antenna"]["radiation_pattern"])
        iso = copy.deepcopy(params)
        iso["bs_antenna"]["radiation_pattern"] = iso["ue_antenna"]["radiation_pattern"] = "isotropic"
        out = original(rays, iso, bs_fov, ue_fov)
        if pats != ("isotropic", "isotropic"):
            g = (side_gain(pats[0], out["_aod_el_rot_fov"], out["_aod_az_rot_fov"]) *
                 side_gain(pats[1], out["_aoa_el_rot_fov"], out["_aoa_az_rot_fov"]))
            out["_power_linear_ant_gain"] = out["power_linear"].astype(np.float64) * g
        return out
    return prepare_paths


@contextlib.contextmanager
def patched_oracle():
    """Inside: `oracle_np.prepare_paths` / `oracle_np.compute_channels` take "tr38901" on either side"""
    original = onp.prepare_paths
    onp.prepare_paths = _prepare_paths_with_patterns(original)
    try:
        yield onp
    finally:
        onp.prepare_paths = original
