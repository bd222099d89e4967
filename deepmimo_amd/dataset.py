"""``Dataset`` / ``MacroDataset`` - the drop-in boundary of the channel-generation path.

Mirrors the parts of deepmimo/generator/dataset.py that orchestrate the hot path:

  * dict + attribute access with lazy computed attributes and the alias table
    (dataset.py:130-182, consts.py:261-322);
  * ``set_channel_params`` / ``compute_channels`` / ``apply_fov`` and the cache invalidation
    rules (dataset.py:197-268, 358-378, 423-448, 515-535);
  * the computed attributes ``los``, ``num_paths``, ``power_linear``, ``_power_linear_ant_gain``,
    rotated and FoV-filtered angles, ``_fov_mask``, ``channel`` (dataset.py:831-869);
  * ``MacroDataset`` fan-out (dataset.py:888-998).

Every number those attributes hold is produced on the GPU by the C-ABI library (engine.py ->
csrc/*.hip); this module is glue (names, caching, dtype of the returned arrays, RNG order for the
random UE rotation).  There is no NumPy implementation of the channel math in this package.

Deliberate deviation from the reference: ``compute_channels`` re-derives all
per-path side products from the current parameters on every call, so a changed radiation pattern
takes effect (the reference only invalidates its ``_power_linear_ant_gain`` cache on a rotation
or FoV change - dataset.py:213-220 - and would silently reuse the stale array).
"""
from __future__ import annotations

import inspect
import types as _types
from collections.abc import Mapping
from typing import Any, Dict, Optional

import numpy as np

from . import consts as c
from .channel import ChannelGenParameters
from .config import config
from .general_utils import DotDict

SHARED_PARAMS = [c.SCENE_PARAM_NAME, c.MATERIALS_PARAM_NAME, c.LOAD_PARAMS_PARAM_NAME, c.RT_PARAMS_PARAM_NAME]

_ROT_KEYS = (c.AOD_EL_ROT_PARAM_NAME, c.AOD_AZ_ROT_PARAM_NAME, c.AOA_EL_ROT_PARAM_NAME, c.AOA_AZ_ROT_PARAM_NAME)
_FOV_ANGLE_KEYS = (c.AOD_EL_FOV_PARAM_NAME, c.AOD_AZ_FOV_PARAM_NAME, c.AOA_EL_FOV_PARAM_NAME, c.AOA_AZ_FOV_PARAM_NAME)
_UE_ROT_RESOLVED = "_ue_rotation_resolved"     # [n_ue, 3] degrees actually used for the cached rotated angles
_PATTERNS_IN_EFFECT = "_patterns_in_effect"    # (bs, ue) radiation patterns behind the cached `_power_linear_ant_gain`

# channel time series (DESIGN.md "Channel time series")
_TIME_BLOCK_BYTES = 1 << 30                    # most the tiled ray matrices of one block of snapshots may take
_RX_VEL, _TX_VEL = "rx_vel", "tx_vel"
_TIMES, _N_TIMES, _N_UE_PER_TIME = "times", "n_times", "n_ue_per_time"
_TIME_KEYS = (_TIMES, _N_TIMES, _N_UE_PER_TIME)
_FOV_KEYS = ("bs_fov", "ue_fov")
# UE receive combining (DESIGN.md "UE receive combining")
_RX_COMBINER, _N_RX_BEAMS, _N_UE_PER_RX_BEAM = "rx_combiner", "n_rx_beams", "n_ue_per_rx_beam"
_RX_KEYS = (_RX_COMBINER, _N_RX_BEAMS, _N_UE_PER_RX_BEAM)
# transmit precoding (DESIGN.md "Transmit precoding and multi-user rates")
_TX_PRECODER, _N_TX_BEAMS, _N_UE_PER_TX_BEAM = "tx_precoder", "n_tx_beams", "n_ue_per_tx_beam"
_TX_KEYS = (_TX_PRECODER, _N_TX_BEAMS, _N_UE_PER_TX_BEAM)
_NOT_PER_USER = (_TX_VEL, c.TX_POS_PARAM_NAME) + _FOV_KEYS + _TIME_KEYS + _RX_KEYS + _TX_KEYS    # never the user axis, whatever their length
_VIEW_RESULTS = ("beam_mean_amplitude", "beam_pair_mean_amplitude")         # results kept in the dict that no view carries
# near field (DESIGN.md "Near field"): the one entry a view of `near_field` carries, its carrier frequency in Hz
_NEAR_FIELD = "near_field_carrier"
# what a block of snapshots needs to run a channel call, and nothing a caller of the view might read beside it
_BLOCK_KEYS = c.RAY_FIELDS + (c.DOPPLER_VEL_PARAM_NAME, c.DOPPLER_ACC_PARAM_NAME, c.CH_PARAMS_PARAM_NAME) + _FOV_KEYS + (_NEAR_FIELD,)

_engines: Dict[int, Any] = {}


class _DeviceSide:
    """Placeholder of a stage-1 side product that is still in HBM.  It sits in the Dataset's dict under the
    product's key (so ``in`` / ``keys()`` behave as in the reference, where the array is cached eagerly) and is
    replaced by the NumPy array the reference would hold the first time anything reads it."""
    __slots__ = ("make",)

    def __init__(self, make):
        self.make = make


def _engine():
    """Process-wide ChannelEngine for config('gpu_device_id').  Raises when use_gpu is off."""
    if not config.get("use_gpu", True):
        raise RuntimeError("deepmimo_amd has no CPU channel-generation path: set dm.config('use_gpu', True).")
    dev = int(config.get("gpu_device_id", 0))
    if dev not in _engines:
        from .engine import ChannelEngine
        _engines[dev] = ChannelEngine(dev)
    return _engines[dev]


def _tile_users(value, reps: int):
    """The per-user array `value` (NumPy or torch) `reps` times along the user axis."""
    if isinstance(value, np.ndarray):
        return np.tile(value, (reps,) + (1,) * (value.ndim - 1))
    return value.repeat(reps, *([1] * (value.dim() - 1)))


def _precoding_codebook(who: str, params, codebook):
    """The `codebook` argument of the codebook-rate methods as an array [C, L, M_tx]: "dft", [C, M_tx] or [C, L, M_tx]; anything
    else is a ValueError that starts with `who`."""
    from .geometry import dft_codebook
    bs_shape = params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE]
    m_tx = int(bs_shape[0]) * int(bs_shape[1])
    what = f"{who}: codebook must be 'dft', an array [C, {m_tx}] or an array [C, L, {m_tx}]"
    if isinstance(codebook, str):
        if codebook != "dft":
            raise ValueError(f"{what}, got {codebook!r}")
        cb = dft_codebook(bs_shape)
    elif codebook is None or isinstance(codebook, (bool, int, float, complex)):
        raise ValueError(f"{what}, got {codebook!r}")
    else:
        cb = codebook if hasattr(codebook, "shape") else np.asarray(codebook)
    if len(cb.shape) == 2:
        cb = cb[:, None, :]
    if len(cb.shape) != 3 or cb.shape[2] != m_tx or cb.shape[0] < 1:
        raise ValueError(f"{what}, got shape {tuple(codebook.shape) if hasattr(codebook, 'shape') else tuple(cb.shape)}")
    return cb


class Dataset(DotDict):
    """One (TX, RX-set) pair of ray-tracing results plus everything computed from it."""

    def __init__(self, data: Optional[Dict[str, Any]] = None):
        super().__init__(data or {})

    # -------------------------------------------------------------- lookup chain (dataset.py:130-182)
    def _host(self, key: str) -> Any:
        """self._data[key], copied out of HBM first if it is still a device-side placeholder."""
        v = self._data[key]
        if isinstance(v, _DeviceSide):
            v = v.make()
            self._data[key] = v
        return v

    def _host_all(self) -> None:
        for k in [k for k, v in self._data.items() if isinstance(v, _DeviceSide)]:
            self._host(k)

    def __getattr__(self, key: str) -> Any:
        if key == "_data" or key.startswith("__"):
            raise AttributeError(key)
        try:
            return self._host(key)
        except KeyError:
            return self._resolve_key(key)

    def __getitem__(self, key: str) -> Any:
        try:
            return self._host(key)
        except KeyError:
            return self._resolve_key(key)

    def get(self, key: str, default: Any = None) -> Any:
        return self._host(key) if key in self._data else default

    def values(self):
        self._host_all()
        return self._data.values()

    def items(self):
        self._host_all()
        return self._data.items()

    def to_dict(self) -> Dict:
        self._host_all()
        return super().to_dict()

    def deepcopy(self):
        self._host_all()
        return super().deepcopy()

    def __repr__(self) -> str:
        self._host_all()
        return super().__repr__()

    def _resolve_key(self, key: str) -> Any:
        resolved = c.DATASET_ALIASES.get(key, key)
        if resolved != key:
            key = resolved
            if key in self._data:
                return self._host(key)
        if key in self._computed_attributes:
            value = getattr(self, self._computed_attributes[key])()
            if isinstance(value, dict):
                self.update(value)
                return self._host(key)
            self[key] = value
            return value
        raise KeyError(key)

    def __dir__(self):
        return sorted(set(list(super().__dir__()) + list(self._computed_attributes.keys()) +
                          list(c.DATASET_ALIASES.keys())))

    # -------------------------------------------------------------- channel parameters
    def set_channel_params(self, params: Optional[ChannelGenParameters] = None):
        """dataset.py:197-222: validate, store a deep copy, drop rotation-dependent caches when a
        rotation changed."""
        if params is None:
            params = ChannelGenParameters()
        params.validate(self.n_ue)
        ue_shape = params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_SHAPE]
        if _N_RX_BEAMS in self._data and [int(v) for v in ue_shape] != [1, 1]:
            raise ValueError(f"this dataset is a view of with_rx_combiner: each of its users is one UE beam of a combined "
                             f"array, a single antenna, and takes ue_antenna.shape = [1, 1] only, got {list(ue_shape)}")
        bs_shape = params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE]
        if _N_TX_BEAMS in self._data and [int(v) for v in bs_shape] != [1, 1]:
            raise ValueError(f"this dataset is a view of with_tx_precoder: each of its users sees one BS beam of a precoded "
                             f"array, a single antenna, and takes bs_antenna.shape = [1, 1] only, got {list(bs_shape)}")
        old = self._data.get(c.CH_PARAMS_PARAM_NAME)
        self.ch_params = params.deepcopy()
        if old is not None:
            rot = c.PARAMSET_ANT_ROTATION
            if (not np.array_equal(old.bs_antenna[rot], params.bs_antenna[rot]) or
                    not np.array_equal(old.ue_antenna[rot], params.ue_antenna[rot])):
                self._clear_cache_rotated_angles()
        return params

    # -------------------------------------------------------------- steps every compute_* shares
    def _call_params(self, params: Optional[ChannelGenParameters]) -> ChannelGenParameters:
        """The parameters of a compute_* call, validated and stored: `params`, or the stored ones (the defaults when none
        were ever set)."""
        if params is None:
            params = ChannelGenParameters() if self._data.get(c.CH_PARAMS_PARAM_NAME) is None else self.ch_params
        return self.set_channel_params(params)

    @staticmethod
    def _required_snr(who: str, snr_db, scalar: bool = True) -> None:
        """`snr_db` is a keyword without a default that means anything: None is refused under the method's name, and a
        `scalar` one has to be a finite number."""
        if snr_db is None:
            raise ValueError(f"{who}: snr_db (dB, keyword) is required")
        if scalar:
            from .engine import snr_linear_from_db
            snr_linear_from_db(snr_db)

    def _loaded_paths(self) -> int:
        """Columns of the ray matrices: the paths every user was loaded with."""
        return int(np.shape(self[c.POWER_PARAM_NAME])[1])

    @staticmethod
    def _deliver(res):
        """What a compute_* returns for the HBM-resident result `res` - a tensor, a tuple or a dict of tensors: NumPy
        unless ``config('channel_output') == 'torch'``."""
        if config.get("channel_output", "numpy") == "torch":
            return res
        if isinstance(res, dict):
            return {k: t.cpu().numpy() for k, t in res.items()}
        return tuple(t.cpu().numpy() for t in res) if isinstance(res, tuple) else res.cpu().numpy()

    # -------------------------------------------------------------- GPU passes
    def _resolved_ue_rotation(self):
        """Per-user UE rotation in degrees or None for a constant one (dataset.py:327-338).  A (3, 2)
        array is a [lo, hi] range drawn with the global NumPy RNG, exactly as the reference draws it;
        the draw is cached with the rotated angles (and dropped with them)."""
        rot = np.asarray(self.ch_params.ue_antenna[c.PARAMSET_ANT_ROTATION])
        if rot.ndim == 1 and rot.shape[0] == 3:
            return None
        cached = self._data.get(_UE_ROT_RESOLVED)
        if cached is not None:
            return cached
        if rot.ndim == 2 and rot.shape == (3, 2):
            # a view of `at_times`, `with_rx_combiner` or `with_tx_precoder` tiles its users: a UE keeps its orientation
            # over the snapshots, the UE beams and the BS beams
            reps = self._data.get(_N_TIMES, 1) * self._data.get(_N_RX_BEAMS, 1) * self._data.get(_N_TX_BEAMS, 1)
            rot = np.tile(np.random.uniform(rot[:, 0], rot[:, 1], (self.n_ue // reps, 3)), (reps, 1))
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 3)
        self._data[_UE_ROT_RESOLVED] = rot
        return rot

    def _carrier_freq(self) -> float:
        rt = self._data.get(c.RT_PARAMS_PARAM_NAME)
        try:
            return float(rt[c.RT_PARAM_FREQUENCY]) if rt is not None else 0.0
        except Exception:
            return 0.0

    def _params_for_prep(self):
        """The parameters stage 1 runs with.  By default the current ones: a changed radiation pattern takes effect at
        once (deliberate deviation).  With ``config('strict_reference_cache', True)`` the
        reference's behaviour is reproduced instead: its `_power_linear_ant_gain` cache survives everything but a
        rotation or FoV change (dataset.py:213-220, 358-378, 515-535), so while that cache entry exists the patterns
        it was computed with stay in effect (pinned by tests/golden/aux_stale_cache.npz)."""
        params = self.ch_params
        pats = (params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_RAD_PAT], params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_RAD_PAT])
        held = self._data.get(_PATTERNS_IN_EFFECT)
        if (config.get("strict_reference_cache", False) and held is not None and held != pats
                and c.PWR_LINEAR_ANT_GAIN_PARAM_NAME in self._data):
            params = params.deepcopy()
            params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_RAD_PAT], params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_RAD_PAT] = held
            pats = held
        self._data[_PATTERNS_IN_EFFECT] = pats
        return params

    def _prep_inputs(self, wideband_fc=None, fd_variant=None):
        """(engine, parameters stage 1 runs with, uploaded rays, prepare keywords) of a GPU pass on this dataset.
        `wideband_fc`: the carrier frequency of a spatial-wideband call (`_wideband_carrier`), None for every other call.
        On a view of `near_field` the pass runs with ``near_field=True`` and the view's carrier, after the checks of
        `engine.check_near_field_call` - before any GPU work; `fd_variant`: the kernel variant of a channel call, which
        is part of those checks."""
        near_fc = self._near_field_checked(self.ch_params, wideband_fc is not None, fd_variant)
        eng = _engine()
        params = self._params_for_prep()
        rays = eng.upload_rays(self)
        kw = dict(bs_fov=self._data.get("bs_fov"), ue_fov=self._data.get("ue_fov"),
                  ue_rotation_per_user=self._resolved_ue_rotation(), carrier_freq=self._carrier_freq(),
                  adaptive_terms=bool(config.get("adaptive_precision", False)))
        if wideband_fc is not None:
            kw.update(carrier_freq=wideband_fc, spatial_wideband=True)
        if near_fc is not None:
            kw.update(carrier_freq=near_fc, near_field=True)
        return eng, params, rays, kw

    def _near_field_checked(self, params, spatial_wideband=False, fd_variant=None):
        """None on a dataset that is no view of `near_field`; on a view, its carrier frequency in Hz after the checks a call
        on it makes before any GPU work (engine.check_near_field_call)."""
        if _NEAR_FIELD not in self._data:
            return None
        from .engine import check_near_field_call
        return check_near_field_call(params, self._data[_NEAR_FIELD], fd_variant, spatial_wideband)

    def _refuse_on_near_field(self, who: str, why: str) -> None:
        if _NEAR_FIELD in self._data:
            raise ValueError(f"{who}: not covered on a near-field view ({why})")

    def _wideband_carrier(self, params, spatial_wideband, carrier_freq):
        """The checks of a channel call with ``spatial_wideband`` before any GPU work (engine.check_wideband_call): the
        carrier frequency in Hz - `carrier_freq`, else rt_params.frequency - or None when the keyword is off."""
        if not spatial_wideband:
            return None
        from .engine import check_wideband_call
        fc = self._carrier_freq() if carrier_freq is None else carrier_freq
        return check_wideband_call(params, fc, config.get("fd_kernel_variant", 0))

    def _run_prep(self, want_side=True, inputs=None, structs=None):
        """Stage 1 on the GPU; refreshes every per-path side product in the cache.  want_side="light" computes LoS,
        path counts and the FoV mask beside the records and leaves the rotated angles / powers to a second stage-1
        pass that runs only if one of them is ever read (`_store_side`)."""
        eng, params, rays, kw = inputs or self._prep_inputs()
        prep = eng.prepare(rays, params, want_side=want_side, structs=structs, **kw)
        if want_side:
            self._store_side(prep, None if want_side is True else (rays, params.deepcopy(), kw))
        return eng, prep

    def _run_single_pass(self, inputs, to_host: bool, out=None):
        """The single-pass route of `compute_channels` (engine.single_pass_route): rays -> channels in one launch, the
        light side products from the same kernel, the heavy ones deferred to a stage-1 pass on their first read.
        Returns ((channels, max delay) or None when the route does not apply and the two calls have to run, the call
        structs if they were built on the way - stage 1 then takes them instead of building them again).  `out`: the
        resident tensor to write into (not with `to_host`)."""
        from .engine import single_pass_preferred, single_pass_route
        eng, params, rays, kw = inputs
        cfg = (config.get("single_pass", "auto"), config.get("fd_kernel_variant", 0), config.get("adaptive_precision", False))
        # what needs no struct first: a call that cannot be routed pays nothing for the question
        if not params[c.PARAMSET_FD_CH] or not single_pass_route(*cfg, True, 9, True, spatial_wideband=kw.get("spatial_wideband", False),
                                                                  near_field=kw.get("near_field", False)):
            return None, None
        structs = eng._call_structs(rays, params, **kw)
        p = structs[0]
        m_rx, m_tx = p.ue_shape[0] * p.ue_shape[1], p.bs_shape[0] * p.bs_shape[1]
        if not single_pass_route(*cfg,
                                 eng.direct_supported(rays, params, structs=structs),
                                 eng.auto_fd_choice(p, rays.n_paths, structs[3]),
                                 not (to_host and eng.host_copy_chunks(rays.n_ue, m_rx * m_tx * p.n_selected)),
                                 single_pass_preferred(m_rx + m_tx, rays.n_paths, p.n_selected)):
            return None, structs
        out, side = eng.channels_direct(rays, params, out=out, structs=structs)
        prep = _types.SimpleNamespace(side=side)
        self._store_side(prep, (rays, params.deepcopy(), kw))
        return ((out.cpu().numpy() if to_host else out), eng.max_delay(prep)), structs

    def _store_side(self, prep, deferred=None) -> None:
        """Register every side product of stage 1 under the reference's cache keys.  The arrays stay in HBM
        (`_DeviceSide`) until something reads them: at 100k users x 25 paths they are ~120 MB of device-to-host
        copies that a caller who only wants the channel tensor never pays for.  With `deferred` = (device rays, params,
        prepare keywords) the rotated angles and powers are not even computed yet: the first read of any of them
        re-runs stage 1 on the SAME uploaded rays (80 MB per 100k users x 25 paths stay in HBM until then) with the same
        parameters, FoV and resolved rotations."""
        memo: Dict[str, np.ndarray] = {}
        heavy: Dict[str, Any] = {}

        def side(name):
            if name in prep.side:
                return prep.side[name]
            if not heavy:                                 # second stage-1 pass, once, for all deferred products
                heavy.update(_engine().prepare(deferred[0], deferred[1], want_side=True, **deferred[2]).side)
            return heavy[name]

        def host(name):                                   # one D2H copy per product, shared by its dependants
            if name not in memo:
                memo[name] = side(name).cpu().numpy()
            return memo[name]

        has_mask = prep.side["fov_mask"] is not None
        d = self._data
        d[c.FOV_MASK_PARAM_NAME] = _DeviceSide(lambda: host("fov_mask").astype(bool)) if has_mask else None
        for k_rot, k_fov, name in zip(_ROT_KEYS, _FOV_ANGLE_KEYS, ("aod_el_rot", "aod_az_rot", "aoa_el_rot", "aoa_az_rot")):
            d[k_rot] = _DeviceSide(lambda name=name: host(name))
            if has_mask:                                                      # dataset.py:506-511
                d[k_fov] = _DeviceSide(lambda name=name: np.where(host("fov_mask").astype(bool), host(name), np.nan))
            else:
                d[k_fov] = _DeviceSide(lambda name=name: host(name))
        d[c.PWR_LINEAR_PARAM_NAME] = _DeviceSide(lambda: host("power_linear"))
        iso = all(pat == c.PARAMSET_ANT_RAD_PAT_VALS[0] for pat in self._data[_PATTERNS_IN_EFFECT])
        # float32 * 1.0 stays float32 in the reference (ant_patterns.py:167-168)
        d[c.PWR_LINEAR_ANT_GAIN_PARAM_NAME] = _DeviceSide(
            lambda: host("power_linear_ant_gain").astype(np.float32) if iso else host("power_linear_ant_gain"))
        d[c.NUM_PATHS_PARAM_NAME] = _DeviceSide(lambda: host("num_paths").astype(np.int64))
        d[c.LOS_PARAM_NAME] = _DeviceSide(lambda: host("los").astype(np.int64))

    @staticmethod
    def _guard_host_copy(nbytes: int) -> None:
        """Refuse a device-to-host copy that cannot fit: at the headline shape the channel tensor is 1 MB per user
        (105 GB per 100k users) and `.cpu()` of it would take the process down with the host's OOM killer."""
        if not config.get("host_copy_guard", True):
            return
        avail = None
        try:
            with open("/proc/meminfo") as f:
                for line in f:
                    if line.startswith("MemAvailable:"):
                        avail = int(line.split()[1]) * 1024
                        break
        except OSError:
            pass
        if avail is not None and nbytes > 0.9 * avail:
            raise MemoryError(
                f"the channel tensor is {nbytes / 1e9:.1f} GB but only {avail / 1e9:.1f} GB of host memory are available: "
                "keep it on the GPU with dm.config('channel_output', 'torch'), or generate it in user chunks with "
                "Dataset.iter_channels(params, chunk_users=...); dm.config('host_copy_guard', False) disables this check.")

    def __getstate__(self):
        """Pickling: side products still in HBM are copied out first (their placeholders are closures)."""
        self._host_all()
        return {"_data": self._data}

    def __setstate__(self, state):
        object.__setattr__(self, "_data", state["_data"])

    def compute_channels(self, params: Optional[ChannelGenParameters] = None, *, spatial_wideband: bool = False,
                         carrier_freq=None, times=None):
        """dataset.py:224-268.  Returns complex64 [n_ue, M_rx, M_tx, K] (freq_domain) or
        [n_ue, M_rx, M_tx, num_paths]: a NumPy array by default, the HBM-resident torch tensor when
        ``config('channel_output') == 'torch'``.  Cached as ``dataset.channel``.

        ``times`` (keyword, extension): a 1-D array of T seconds gives the snapshots of ``at_times(times, carrier_freq)``
        as [T, n_ue, M_rx, M_tx, K], time-major - ``out[t]`` has the layout of one call - and a scalar the one snapshot
        without the leading axis; nothing is cached then.  A per-user [n_ue, 3] UE rotation holds for every snapshot.

        ``spatial_wideband`` (keyword, extension): the array response of every element is taken at the subcarrier's own
        frequency ``f_c + sc_k B / N`` instead of at the carrier (beam squint; include/deepmimo_amd.h
        DMX_FLAG_SPATIAL_WIDEBAND).  ``f_c``: ``carrier_freq``, else ``rt_params.frequency`` - it is then the carrier of the
        Doppler term too.  Frequency domain without rx_filter, ``config('fd_kernel_variant')`` 0 or 1 (the fp32 vector
        kernel runs either way); anything else, or no carrier frequency, raises ValueError before any GPU work.  It composes
        with ``times``, the views of ``at_times`` / ``with_rx_combiner``, ``enable_doppler`` and ``adaptive_precision``."""
        if times is not None:
            return self._channels_over_time(params, times, carrier_freq, spatial_wideband)
        params = self._call_params(params)
        wideband_fc = self._wideband_carrier(params, spatial_wideband, carrier_freq)
        np.random.seed(1001)                                                   # dataset.py:250
        to_host = config.get("channel_output", "numpy") != "torch"
        if to_host:                                                            # before any GPU work is spent on it
            self._guard_host_copy(8 * int(np.prod(self._channel_shape(params))))
        out, max_delay = self._channels_once(params, to_host, wideband_fc=wideband_fc)
        ofdm = params[c.PARAMSET_OFDM]
        if params[c.PARAMSET_FD_CH]:
            self._warn_symbol_duration(max_delay, ofdm)
        self[c.CHANNEL_PARAM_NAME] = out
        return out

    def _channel_shape(self, params):
        """(n_ue, M_rx, M_tx, K or num_paths): the tensor the host guard of `compute_channels` sizes."""
        ofdm_, n_ant = params[c.PARAMSET_OFDM], [int(np.prod(params[s_][c.PARAMSET_ANT_SHAPE])) for s_ in (c.PARAMSET_ANT_BS, c.PARAMSET_ANT_UE)]
        last = len(np.atleast_1d(ofdm_[c.PARAMSET_OFDM_SC_SAMP])) if params[c.PARAMSET_FD_CH] else int(params[c.PARAMSET_NUM_PATHS])
        return int(self.n_ue), n_ant[1], n_ant[0], last

    def _channels_once(self, params, to_host: bool, out=None, wideband_fc=None):
        """The GPU part of `compute_channels` for the stored parameters `params`: the single pass where it applies, else
        stage 1 and stage 2.  Returns (channels, the delay maximum or None in the time domain).  `out`: the resident
        tensor to write into (not with `to_host`).  `wideband_fc`: as for `_prep_inputs`."""
        inputs = self._prep_inputs(wideband_fc, fd_variant=config.get("fd_kernel_variant", 0))
        direct, structs = self._run_single_pass(inputs, to_host, out)
        if direct is not None:
            return direct
        eng, prep = self._run_prep(want_side="light", inputs=inputs, structs=structs)
        variant = int(config.get("fd_kernel_variant", 0))
        H = eng.channels_to_host(prep, variant=variant) if to_host else eng.channels(prep, out=out, variant=variant)
        return H, (eng.max_delay(prep) if params[c.PARAMSET_FD_CH] else None)

    def iter_channels(self, params: Optional[ChannelGenParameters] = None, chunk_users: int = 4096, *,
                      spatial_wideband: bool = False, carrier_freq=None, times=None):
        """Generate channels in user chunks (extension): yields ``(user_begin, H_chunk)`` with ``H_chunk`` a
        NumPy complex64 array [<= chunk_users, M_rx, M_tx, K].  For scenarios whose full tensor (1 MB per user at
        64x4 antennas x 512 subcarriers) fits neither host memory nor one NumPy array; stage 1 runs once, stage 2
        per chunk through the C-ABI's user_begin / user_count range.  Nothing is cached as ``channel``.

        With ``times`` (keyword; as in ``compute_channels``) it yields ``(t_index, user_begin, H_chunk)``, the snapshots
        in order and the users of a snapshot in order; stage 1 runs once per block of snapshots.  ``spatial_wideband``: as
        in ``compute_channels``."""
        if times is not None:
            yield from self._iter_channels_over_time(params, chunk_users, times, carrier_freq, spatial_wideband)
            return
        params = self._call_params(params)
        wideband_fc = self._wideband_carrier(params, spatial_wideband, carrier_freq)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light", inputs=self._prep_inputs(wideband_fc, config.get("fd_kernel_variant", 0)))
        n = prep.n_ue
        variant = int(config.get("fd_kernel_variant", 0))
        for b in range(0, n, max(1, int(chunk_users))):
            cnt = min(int(chunk_users), n - b)
            yield b, eng.channels_to_host(prep, variant=variant, user_begin=b, user_count=cnt)

    def compute_beam_channels(self, codebook, params: Optional[ChannelGenParameters] = None):
        """Beam-space channels ``codebook @ H`` for a TX codebook [n_beams, M_tx] (rows e.g. from
        ``dm.steering_vec``), complex64 [n_ue, M_rx, n_beams, K] - what docs/manual.ipynb cell 105 computes
        as ``F1 @ dataset.channel`` - without materialising H (extension).  Not cached."""
        self._refuse_on_near_field("compute_beam_channels", "the beam-space channel kernel builds plane-wave responses only")
        self._call_params(params)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        if config.get("channel_output", "numpy") == "torch":
            return eng.channels(prep, tx_codebook=codebook)
        cb = codebook if hasattr(codebook, "shape") else np.asarray(codebook)
        return eng.channels_to_host(prep, tx_codebook=cb)

    def compute_beam_power(self, codebook, params: Optional[ChannelGenParameters] = None, return_best: bool = False,
                           metric: str = "amplitude"):
        """Received power per beam of a TX codebook [n_beams, M_tx] - the beam sweep of docs/manual.ipynb cells
        105 / 110 / 112 in one call, with no channel tensor written anywhere (extension):

            mean_amplitude  = np.abs(codebook @ dataset.channel).mean(axis=1).mean(axis=-1)   # computed on the GPU
            recv_bf_pwr_dbm = np.around(20 * np.log10(mean_amplitude) + 30, 1), NaN where dataset.los == -1
            best_beams      = np.argmax(recv_bf_pwr_dbm, axis=1) as float, NaN where dataset.los == -1

        Returns ``recv_bf_pwr_dbm`` float64 [n_ue, n_beams] (and ``best_beams`` with ``return_best``).  The raw means stay
        available as ``dataset['beam_mean_amplitude']`` (float32 [n_ue, n_beams]).

        ``metric="power"`` averages the power instead, what 3GPP calls RSRP (an SSB sweep, an L1-RSRP report, cell selection):

            mean_power      = (np.abs(codebook @ dataset.channel) ** 2).mean(axis=1).mean(axis=-1)
            recv_bf_pwr_dbm = np.around(10 * np.log10(mean_power) + 30, 1)

        with the same NaN rule and ``best_beams``; the raw means are kept as ``dataset['beam_mean_power']``.  The two
        metrics do not always agree on the best beam.  Any other ``metric`` raises ValueError before any GPU work."""
        from .engine import check_beam_metric
        power = check_beam_metric("compute_beam_power", metric)
        self._call_params(params)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        amp, _ = eng.beam_power(prep, codebook, want_best=False, metric=metric)
        amp = amp.cpu().numpy()
        self._data["beam_mean_power" if power else "beam_mean_amplitude"] = amp
        no_paths = self[c.LOS_PARAM_NAME] == -1
        pwr = np.zeros(amp.shape) * np.nan                                      # float64, as the notebook allocates it
        with np.errstate(divide="ignore"):
            pwr[~no_paths] = np.around((10 if power else 20) * np.log10(amp[~no_paths]) + 30, 1)
        if not return_best:
            return pwr
        best = np.argmax(pwr, axis=1).astype(float) if pwr.shape[1] else np.zeros(len(pwr))
        best[np.isnan(pwr[:, 0])] = np.nan
        return pwr, best

    def compute_covariance(self, params: Optional[ChannelGenParameters] = None, side: str = "tx"):
        """Per-user spatial covariance of the frequency-domain channel, with no channel tensor written anywhere
        (extension):

            side "tx":  R[u] = np.einsum('rik,rjk->ij', H[u], H[u].conj()) / (M_rx * K)      # over the BS array
            side "rx":  R[u] = np.einsum('itk,jtk->ij', H[u], H[u].conj()) / (M_tx * K)      # over the UE array

        Returns complex64 [n_ue, M, M]: a NumPy array by default, the HBM-resident torch tensor when
        ``config('channel_output') == 'torch'``.  Every block is exactly Hermitian.  Frequency domain without
        ``rx_filter``, at most 32 used paths, tables within the LDS (include/deepmimo_amd.h has the rule): anything else
        raises ValueError before any GPU work.  Not cached."""
        from .engine import check_covariance_call
        params = self._call_params(params)
        check_covariance_call(params, self._loaded_paths(), side)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        return self._deliver(eng.covariance(prep, side=side))

    def compute_rate(self, params: Optional[ChannelGenParameters] = None, *, snr_db=None, per_subcarrier: bool = False,
                     power_allocation: str = "equal"):
        """Per-user achievable rate (spectral efficiency) in bit/s/Hz, with no channel tensor written anywhere
        (extension).  ``power_allocation="equal"`` (the default) - equal power on every BS antenna, no
        channel knowledge at the transmitter:

            s = 10 ** (snr_db / 10) / M_tx            # snr_db: total transmit power over noise power per subcarrier
            rate_k[u, k] = log2 det(I + s * H[u, :, :, k] @ H[u, :, :, k].conj().T)
            rate[u]      = rate_k[u].mean()

        ``power_allocation="waterfilling"`` - full channel knowledge at the transmitter, the same total power poured over
        the eigenmodes of each subcarrier (``compute_eigenmodes`` has them), never below the equal-power rate:

            g = 10 ** (snr_db / 10) * eigvalsh(H[u, :, :, k] @ H[u, :, :, k].conj().T)
            rate_k[u, k] = max over p >= 0, p.sum() == 1 of log2(1 + p * g).sum()

        Returns float32 [n_ue] (with ``per_subcarrier`` the pair ``(rate, rate_k)``, rate_k float32 [n_ue, K]): NumPy arrays
        by default, the HBM-resident torch tensors when ``config('channel_output') == 'torch'``.  ``snr_db`` is required
        and keyword-only.  Users without a path get 0.  Frequency domain without ``rx_filter``, at most 32 used paths, the smaller array of at most 8 elements, tables
        within the LDS (include/deepmimo_amd.h has the rule): anything else raises ValueError before any GPU work.  Not
        cached."""
        from .engine import check_rate_call, check_spectrum_call
        if power_allocation not in ("equal", "waterfilling"):
            raise ValueError(f"compute_rate: power_allocation must be 'equal' or 'waterfilling', got {power_allocation!r}")
        equal = power_allocation == "equal"
        self._required_snr("compute_rate", snr_db)
        params = self._call_params(params)
        (check_rate_call if equal else check_spectrum_call)(params, self._loaded_paths(), snr_db)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        if equal:
            return self._deliver(eng.rate(prep, snr_db, per_subcarrier=per_subcarrier))
        return self._deliver(eng.spectrum(prep, snr_db, gamma=False, rate=True, per_subcarrier=per_subcarrier))

    def compute_eigenmodes(self, params: Optional[ChannelGenParameters] = None, *, snr_db=None):
        """Eigenmodes of every user's channel per subcarrier, with no channel tensor written anywhere (extension;
        SURVEY.md 8(f)-2): the mode SNRs, sorted descending along the last axis, m = min(M_rx, M_tx):

            gamma[u, k] = 10 ** (snr_db / 10) * eigvalsh(H[u, :, :, k] @ H[u, :, :, k].conj().T)[::-1][:m]

        ``gamma / snr`` is the eigenvalue and its square root the singular value of ``H[u, :, :, k]``; the rank is the
        count of modes above a threshold and the condition number the ratio of the first to the last.  Returns float32
        [n_ue, K, m]: a NumPy array by default, the HBM-resident torch tensor when ``config('channel_output') == 'torch'``.
        ``snr_db`` (total transmit power over noise power per subcarrier) is required and keyword-only.  Users without a
        path get 0.  The shapes taken are those of ``compute_rate``; anything else raises ValueError before any GPU work.
        Not cached."""
        from .engine import check_spectrum_call
        self._required_snr("compute_eigenmodes", snr_db)
        params = self._call_params(params)
        check_spectrum_call(params, self._loaded_paths(), snr_db)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        return self._deliver(eng.spectrum(prep, snr_db))

    def compute_precoders(self, params: Optional[ChannelGenParameters] = None, *, snr_db=None, n_layers: int = 1,
                          combiners: bool = False):
        """Eigenbeam precoders (and combiners) of every user's channel per subcarrier, with no channel tensor written
        anywhere (extension).  With ``U, s, Vh = svd(H[u, :, :, k])``, strongest modes first,
        m = min(M_rx, M_tx) and L = ``n_layers`` in 1..m:

            gamma[u, k]    = 10 ** (snr_db / 10) * s[:m] ** 2           # float32   [n_ue, K, m], as compute_eigenmodes
            w_tx[u, k, i]  = Vh[i].conj()                               # complex64 [n_ue, K, L, M_tx], unit norm
            w_rx[u, k, i]  = U[:, i]                                    # complex64 [n_ue, K, L, M_rx], with ``combiners``

        so ``w_rx[u, k, i].conj() @ H[u, :, :, k] @ w_tx[u, k, i]`` is ``s[i]``, real and >= 0.  The phase of a pair is
        fixed on the smaller array: the component of largest modulus of that vector is real and positive.  A layer whose
        mode lies below the float32 resolution of the entry (about -45 dB of the sum of the modes at m = 4, -38 dB at
        m = 8; include/deepmimo_amd.h has the rule), e.g. the second layer of a one-path user, is all zeros, and so is a
        user without a path.  Returns ``(gamma, w_tx)`` or ``(gamma, w_tx, w_rx)``: NumPy arrays by default, the
        HBM-resident torch tensors when ``config('channel_output') == 'torch'``.  ``snr_db`` (total transmit power over
        noise power per subcarrier) is required and keyword-only: it puts the Gram matrix into float32 range and is the
        unit of ``gamma``; the vectors do not depend on it otherwise.  The shapes taken are those of ``compute_rate``;
        anything else raises ValueError before any GPU work.  Not cached."""
        from .engine import check_precoder_call
        self._required_snr("compute_precoders", snr_db)
        params = self._call_params(params)
        check_precoder_call(params, self._loaded_paths(), snr_db, n_layers)
        if config.get("channel_output", "numpy") != "torch":                   # before any GPU work is spent on it
            n_ant = [int(np.prod(params[k][c.PARAMSET_ANT_SHAPE])) for k in (c.PARAMSET_ANT_BS, c.PARAMSET_ANT_UE)]
            k_sel = int(np.size(params[c.PARAMSET_OFDM][c.PARAMSET_OFDM_SC_SAMP]))
            per_entry = 4 * min(n_ant) + 8 * int(n_layers) * (n_ant[0] + (n_ant[1] if combiners else 0))
            self._guard_host_copy(int(self.n_ue) * k_sel * per_entry)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        return self._deliver(eng.precoders(prep, snr_db, n_layers=int(n_layers), rx=bool(combiners)))

    def compute_angle_delay(self, params: Optional[ChannelGenParameters] = None, *, n_taps=None, n_fft=None, codebook="dft",
                            output: str = "complex"):
        """Angle-delay representation of every user's channel, with no channel tensor written anywhere (extension) - what
        CSI-feedback models train on (``output="complex"``); fingerprinting, localisation and channel-charting models train on
        its power matrix (``"power"``) and on the delay profile (``"profile"``):

            Y = codebook @ H                                         # [n_ue, M_rx, R, K], H the frequency-domain channel
            X = np.fft.ifft(Y, n=n_fft, axis=-1)[..., :n_taps]       # the first n_taps delay taps

        ``codebook``: ``"dft"`` (``dm.dft_codebook`` of the BS panel: the angular domain), a complex array [R, M_tx], or
        ``None`` (the antenna domain: R = M_tx, the delay-domain channel of every antenna pair).  ``n_taps`` is required and
        keyword-only; ``n_fft=None`` means the number of selected subcarriers.  Returns complex64 [n_ue, M_rx, R, n_taps]: a
        NumPy array by default, the HBM-resident torch tensor when ``config('channel_output') == 'torch'``.  Users without
        a path get 0.  Frequency domain without ``rx_filter``, a uniformly spaced selection, at most 32 used paths and 8 UE
        elements, K <= n_fft <= 2**20, 1 <= n_taps <= n_fft (include/deepmimo_amd.h has the rule): anything else raises
        ValueError before any GPU work.  Not cached.

        ``output``: ``"complex"`` (default) is X above.  ``"power"`` is the angle-delay channel power matrix and
        ``"profile"`` its row sum, the power-delay profile,

            P = (np.abs(X) ** 2).sum(axis=1)                         # float32 [n_ue, R, n_taps]
            p = P.sum(axis=1)                                        # float32 [n_ue, n_taps]

        raw sums (divide by M_rx, or M_rx * R, for means) formed in the kernel's registers: X is written nowhere, so the
        result is 2 M_rx, or 2 M_rx R, times smaller than X and the host-copy guard counts that size.  With an orthonormal
        codebook (``"dft"``) the profile equals the antenna-domain one (``codebook=None``) by Parseval.  ``dm.tap_delays``
        gives the delay of every tap and ``dm.delay_spread`` the mean excess delay and RMS delay spread of a profile.  On a
        view of ``with_rx_combiner`` M_rx = 1, so ``"power"`` is ``|w_q H|^2`` per UE beam q, in the angle-delay domain.
        Anything else is a ValueError."""
        from .engine import check_angle_delay_call, check_angle_delay_output
        from .geometry import dft_codebook
        check_angle_delay_output("compute_angle_delay", output)                # before the engine is needed
        if n_taps is None:
            raise ValueError("compute_angle_delay: n_taps (keyword) is required")
        params = self._call_params(params)
        bs_shape = params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE]
        m_tx = int(bs_shape[0]) * int(bs_shape[1])
        if codebook is None:
            cb = None
        elif isinstance(codebook, str):
            if codebook != "dft":
                raise ValueError(f"compute_angle_delay: codebook must be 'dft', an array [R, {m_tx}] or None, got {codebook!r}")
            cb = dft_codebook(bs_shape)
        else:
            cb = codebook if hasattr(codebook, "shape") else np.asarray(codebook)
            if len(cb.shape) != 2 or cb.shape[1] != m_tx or cb.shape[0] < 1:
                raise ValueError(f"compute_angle_delay: codebook must be [R, {m_tx}], got {tuple(cb.shape)}")
        n_rows = m_tx if cb is None else int(cb.shape[0])
        n_fft = check_angle_delay_call(params, self._loaded_paths(), n_rows, n_fft, n_taps, output)
        if config.get("channel_output", "numpy") != "torch":                   # before any GPU work is spent on it
            m_rx = int(np.prod(params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_SHAPE]))
            per_user = {"complex": 8 * m_rx * n_rows, "power": 4 * n_rows, "profile": 4}[output] * int(n_taps)
            self._guard_host_copy(int(self.n_ue) * per_user)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        return self._deliver(eng.angle_delay(prep, int(n_taps), n_fft=n_fft, tx_codebook=cb, output=output))

    def compute_codebook_rate(self, params: Optional[ChannelGenParameters] = None, *, codebook="dft", snr_db=None,
                              per_codeword: bool = False, receiver: str = "joint"):
        """Rate of every codeword of a finite precoding codebook and the best codeword per user - the precoder-matrix
        indicator (PMI) of a CSI report and the rate behind its CQI - with no channel tensor written anywhere (extension):

            s = 10 ** (snr_db / 10) / L               # snr_db: total transmit power over noise power per subcarrier
            E = H[u, :, :, k] @ W[c].T                # [M_rx, L]: codeword c, its L layers (rows of W[c]) on the BS array
            rate_c[u, c] = mean over k of log2 det(I + s * E.conj().T @ E)
            pmi[u]  = rate_c[u].argmax()              # the first maximum; -1 for a user without a path
            rate[u] = rate_c[u, pmi[u]]               # 0 for a user without a path

        ``codebook``: ``"dft"`` (``dm.dft_codebook`` of the BS panel as M_tx single-layer codewords), a complex array
        [C, M_tx] (L = 1) or [C, L, M_tx] with 1 <= L <= min(M_rx, 4).  Codewords are used as given: rows of unit norm keep the
        transmit power at ``snr_db``.  Returns ``(rate, pmi)`` - float32 [n_ue], int32 [n_ue] - and with ``per_codeword``
        ``(rate, pmi, rate_c)``, rate_c float32 [n_ue, C]: NumPy arrays by default, the HBM-resident torch tensors when
        ``config('channel_output') == 'torch'``.  ``snr_db`` is required and keyword-only.  One PMI over the whole selection;
        ``compute_subband_pmi`` adds a PMI per subband and ``compute_csi_report`` the rank.  Frequency domain without
        ``rx_filter``, at most 32 used paths and 8 UE elements (include/deepmimo_amd.h has the rule): anything else raises
        ValueError before any GPU work.  Not cached.

        ``receiver``: ``"joint"`` (default) is the log2 det above, the rate of a maximum-likelihood receiver or of MMSE with
        successive cancellation; ``"mmse"`` is what a UE with a linear MMSE receiver reports, the sum over the layers of
        log2(1 + SINR_i) after equalisation, equal power per layer:

            A = I + s * E.conj().T @ E
            rate_c[u, c] = mean over k of -np.log2(np.linalg.inv(A).diagonal().real).sum()

        It is at or below the joint rate, by more where the layers of a codeword leak into each other, so PMI (and the
        rank of ``compute_csi_report``) can differ; with one layer the two are the same bits.  Anything else is a
        ValueError."""
        return self._codebook_rate("compute_codebook_rate", params, codebook, snr_db, per_codeword, receiver=receiver)

    def _codebook_rate(self, who: str, params, codebook, snr_db, per_codeword, subbands: bool = False, subband_size=None,
                       receiver="joint"):
        """`compute_codebook_rate`, or with `subbands` `compute_subband_pmi`: the same checks and preparation, the launch
        without or with a PMI per subband.  `who`: the public method, for the messages."""
        from .engine import check_codebook_rate_call, check_subband_size
        self._required_snr(who, snr_db)
        if subbands:
            subband_size = check_subband_size(subband_size)
        params = self._call_params(params)
        cb = _precoding_codebook(who, params, codebook)
        check_codebook_rate_call(params, self._loaded_paths(), int(cb.shape[0]), int(cb.shape[1]), snr_db, receiver)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        if subbands:
            return self._deliver(eng.codebook_rate_subbands(prep, cb, snr_db, subband_size, per_codeword=bool(per_codeword),
                                                            receiver=receiver))
        return self._deliver(eng.codebook_rate(prep, cb, snr_db, per_codeword=bool(per_codeword), receiver=receiver))

    def compute_subband_pmi(self, params: Optional[ChannelGenParameters] = None, *, codebook="dft", snr_db=None,
                            subband_size=None, per_codeword: bool = False, receiver: str = "joint"):
        """``compute_codebook_rate`` with a PMI per subband from the same launch - the wideband and the subband part of a CSI
        report for the layer count of ``codebook`` (extension).  Subbands partition the selected subcarriers in their own
        order: subband s covers the positions s B .. min((s + 1) B, K) - 1 with B = ``subband_size`` (an integer >= 1; None:
        one subband), n_sb = ceil(K / B), the last one possibly short:

            rate_sb_c[u, s, c] = mean over k in subband s of log2 det(I + s * E.conj().T @ E)     # E, s as compute_codebook_rate
            pmi_sb[u, s]  = rate_sb_c[u, s].argmax()      # the first maximum; -1 for a user without a path
            rate_sb[u, s] = rate_sb_c[u, s, pmi_sb[u, s]]
            rate_c, pmi, rate: as compute_codebook_rate, the subbands added in subband order

        Returns ``(rate, pmi, rate_sb, pmi_sb)`` - float32 [n_ue], int32 [n_ue], float32 / int32 [n_ue, n_sb] - and with
        ``per_codeword`` also ``rate_c`` [n_ue, C] and ``rate_sb_c`` [n_ue, n_sb, C].  Column s equals what
        ``compute_codebook_rate`` returns for the selection ``sc[s B : (s + 1) B]`` bit for bit; with one subband all of it
        equals ``compute_codebook_rate``.  ``codebook``, ``snr_db``, the shapes taken and the return convention are those of
        ``compute_codebook_rate``; anything else raises ValueError before any GPU work.  ``receiver``: as
        ``compute_codebook_rate`` - with ``"mmse"`` every rate above is the linear MMSE receiver's.  Not cached."""
        return self._codebook_rate("compute_subband_pmi", params, codebook, snr_db, per_codeword, True, subband_size, receiver)

    def compute_csi_report(self, params: Optional[ChannelGenParameters] = None, *, codebooks=None, snr_db=None,
                           subband_size=None, receiver: str = "joint"):
        """Rank indicator, wideband PMI and a PMI per subband of every user - the three parts of a CSI report - from one
        subband launch per candidate rank on the same preparation, no channel tensor written (extension).  ``codebooks``: a
        sequence of complex arrays [C_L, L, M_tx] (2-D: L = 1) with distinct layer counts L, one per candidate rank.

            rank[u] = the L of the largest wideband rate (``compute_subband_pmi`` per codebook); on ties the smallest L;
                      0 for a user without a path

        Returns a DotDict: ``rank`` int32 [n_ue]; ``rate`` float32 [n_ue], ``pmi`` int32 [n_ue], ``rate_sb`` float32 and
        ``pmi_sb`` int32 [n_ue, n_sb], all of the chosen rank's codebook (0 / -1 without a path); ``rate_by_rank`` float32
        [n_ue, n_ranks], the wideband rate of every candidate in ascending L.  ``subband_size``, ``snr_db`` (the total
        transmit power, split over the layers of each candidate) and the return convention as ``compute_subband_pmi``; a
        duplicate L, an empty ``codebooks`` or a shape not taken raises ValueError before any GPU work.  Mapping a rate to a
        CQI index is a table lookup left to the caller.  ``receiver``: as ``compute_codebook_rate``, passed to the launch
        of every rank; with ``"mmse"`` the rank is the L of the largest linear-MMSE wideband rate (the single-layer column
        of ``rate_by_rank`` is the same bits for both receivers).  Not cached."""
        import torch
        from .engine import check_codebook_rate_call, check_subband_size
        self._required_snr("compute_csi_report", snr_db)
        subband_size = check_subband_size(subband_size)
        params = self._call_params(params)
        if codebooks is None or isinstance(codebooks, (str, bool, int, float, complex)) or hasattr(codebooks, "shape") or \
                len(codebooks) == 0:
            raise ValueError("compute_csi_report: codebooks must be a non-empty sequence of arrays [C, L, M_tx], one per rank")
        cbs = sorted((_precoding_codebook("compute_csi_report", params, cb) for cb in codebooks), key=lambda cb: int(cb.shape[1]))
        ranks = [int(cb.shape[1]) for cb in cbs]
        if len(set(ranks)) != len(ranks):
            raise ValueError(f"compute_csi_report: the codebooks must have distinct layer counts, got L = {ranks}")
        for cb in cbs:
            check_codebook_rate_call(params, self._loaded_paths(), int(cb.shape[0]), int(cb.shape[1]), snr_db, receiver)
        np.random.seed(1001)
        eng, prep = self._run_prep(want_side="light")
        per_rank = [eng.codebook_rate_subbands(prep, cb, snr_db, subband_size, receiver=receiver) for cb in cbs]
        rate, pmi, rate_sb, pmi_sb = (t.clone() for t in per_rank[0])
        rank = torch.where(pmi >= 0, ranks[0], 0).to(torch.int32)
        for L, (r, p, rs, ps) in zip(ranks[1:], per_rank[1:]):                 # a strict >: the smallest L on ties
            take = r > rate
            rank = torch.where(take, L, rank).to(torch.int32)
            rate, pmi = torch.where(take, r, rate), torch.where(take, p, pmi)
            rate_sb, pmi_sb = torch.where(take[:, None], rs, rate_sb), torch.where(take[:, None], ps, pmi_sb)
        out = dict(rank=rank, rate=rate, pmi=pmi, rate_sb=rate_sb, pmi_sb=pmi_sb,
                   rate_by_rank=torch.stack([t[0] for t in per_rank], dim=1))
        return DotDict(self._deliver(out))

    def compute_pathloss(self, coherent: bool = True) -> np.ndarray:
        """Path loss in dB assuming 0 dBm transmitted power (dataset.py:541-566); cached as ``pathloss``."""
        eng = _engine()
        pl = eng.pathloss(eng.upload_rays(self), coherent).cpu().numpy()
        self[c.PATHLOSS_PARAM_NAME] = pl
        return pl

    @staticmethod
    def _warn_symbol_duration(max_delay: float, ofdm) -> None:
        """The reference's clipping warning (channel.py:228-250), fed by the device-side max."""
        n_sc, bw = ofdm[c.PARAMSET_OFDM_SC_NUM], ofdm[c.PARAMSET_OFDM_BANDWIDTH]
        symbol = n_sc / bw
        if not (max_delay > symbol):
            return
        print("\nWarning: Some path delays exceed OFDM symbol duration")
        print("-" * 50)
        print("OFDM Configuration:")
        print(f"- Number of subcarriers (N): {n_sc}")
        print(f"- Bandwidth (B): {bw/1e6:.1f} MHz")
        print(f"- Subcarrier spacing (Δf = B/N): {bw/n_sc/1e3:.1f} kHz")
        print(f"- Symbol duration (T = 1/Δf = N/B): {symbol*1e6:.1f} μs")
        print("\nPath Information:")
        print(f"- Maximum path delay: {max_delay*1e6:.1f} μs")
        print(f"- Excess delay: {(max_delay - symbol)*1e6:.1f} μs")
        print("\nPaths arriving after the symbol duration will be clipped.")
        print("To avoid clipping, either:")
        print("1. Increase the number of subcarriers (N)")
        print("2. Decrease the bandwidth (B)")
        print(f"3. Switch to time-domain channel generation (set ch_params['{c.PARAMSET_FD_CH}'] = 0)")
        print("-" * 50)

    # -------------------------------------------------------------- lazily computed attributes
    def _side(self, key):
        """Run stage 1 if `key` is not cached yet, then return it (all side products land together)."""
        if key not in self._data:
            _ = self.ch_params                                              # resolves defaults if never set
            self._run_prep(want_side=True)
        return self._host(key)

    def _compute_rotated_angles(self) -> Dict[str, np.ndarray]:
        self._side(c.AOD_EL_ROT_PARAM_NAME)
        return {k: self._host(k) for k in _ROT_KEYS}

    def _compute_fov(self) -> Dict[str, Any]:
        self._side(c.FOV_MASK_PARAM_NAME)
        return {k: self._host(k) for k in (c.FOV_MASK_PARAM_NAME,) + _FOV_ANGLE_KEYS}

    def _compute_num_paths(self) -> np.ndarray:
        return self._side(c.NUM_PATHS_PARAM_NAME)

    def _compute_los(self) -> np.ndarray:
        return self._side(c.LOS_PARAM_NAME)

    def _compute_power_linear(self) -> np.ndarray:
        return self._side(c.PWR_LINEAR_PARAM_NAME)

    def _compute_power_linear_ant_gain(self) -> np.ndarray:
        return self._side(c.PWR_LINEAR_ANT_GAIN_PARAM_NAME)

    def _compute_array_response_product(self) -> np.ndarray:
        """complex128 [n_ue, M_rx, M_tx, L] product of the two array responses (dataset.py:398-417), from the rotated,
        FoV-filtered angles stage 1 produced on the GPU.  The channel kernels never form this tensor (10 GB at the
        headline shape, 82 GB at config 5 - they generate it per tile); it exists for callers that read the public
        attribute, on the host and for sizes that fit: above `config('array_response_max_bytes')` (default 2 GiB) a
        MemoryError names the alternatives instead of the bare KeyError an unknown attribute would raise."""
        from .geometry import _ant_indices
        p = self.ch_params
        bs, ue = p[c.PARAMSET_ANT_BS], p[c.PARAMSET_ANT_UE]
        m_tx, m_rx = int(np.prod(bs[c.PARAMSET_ANT_SHAPE])), int(np.prod(ue[c.PARAMSET_ANT_SHAPE]))
        n, L = self[c.POWER_PARAM_NAME].shape
        need = 16 * n * m_rx * m_tx * L
        limit = int(config.get("array_response_max_bytes", 2 << 30))
        if need > limit:
            raise MemoryError(
                f"array_response_product would take {need / 1e9:.1f} GB ([{n}, {m_rx}, {m_tx}, {L}] complex128); the GPU path never "
                f"materialises it - use compute_channels() / dataset.channel (or compute_beam_power), read it for a "
                f"dataset.subset(idxs) of users, or raise config('array_response_max_bytes')")
        aod_el, aod_az = self[c.AOD_EL_FOV_PARAM_NAME], self[c.AOD_AZ_FOV_PARAM_NAME]
        aoa_el, aoa_az = self[c.AOA_EL_FOV_PARAM_NAME], self[c.AOA_AZ_FOV_PARAM_NAME]

        def resp(ant, theta, phi):                                           # geometry.py:38-102
            idx = _ant_indices(ant[c.PARAMSET_ANT_SHAPE]).astype(np.float64)
            kd = 2 * np.pi * float(ant[c.PARAMSET_ANT_SPACING])
            out = np.zeros((theta.shape[0], idx.shape[0], theta.shape[1]), dtype=np.complex128)
            ok = ~np.isnan(theta)
            t, f = theta[ok], phi[ok]
            gamma = 1j * kd * np.stack([np.sin(t) * np.cos(f), np.sin(t) * np.sin(f), np.cos(t)], axis=0)   # [3, n_valid]
            ub, ul = np.nonzero(ok)
            out[ub, :, ul] = np.exp(idx @ gamma).T
            return out

        a_tx, a_rx = resp(bs, aod_el, aod_az), resp(ue, aoa_el, aoa_az)
        return a_rx[:, :, None, :] * a_tx[:, None, :, :]

    def _compute_n_ue(self) -> int:
        return self.rx_pos.shape[0]                                          # dataset.py:657-659

    def _compute_distances(self) -> np.ndarray:
        return np.linalg.norm(self.rx_pos - self.tx_pos, axis=1)             # dataset.py:661-663

    def _compute_inter_int(self) -> np.ndarray:
        v = np.array(self._inter_host(), copy=True)                          # dataset.py:629-637
        v[np.isnan(v)] = -1
        return v.astype(int)

    def _inter_host(self) -> np.ndarray:
        inter = self.inter
        if hasattr(inter, "detach"):                                         # device-resident rays (load(device=...))
            inter = inter.detach().cpu().numpy()
        return np.asarray(inter)

    def _compute_num_interactions(self) -> np.ndarray:
        """Bounces per path = decimal digits of the interaction code; 0 for LoS (code 0), NaN where there is no path
        (dataset.py:621-627)."""
        inter = self._inter_host()
        n = np.zeros_like(inter)
        n[np.isnan(inter)] = np.nan
        pos = inter > 0
        n[pos] = np.floor(np.log10(inter[pos])) + 1
        return n

    _INTER_LETTERS = {"0": "", "1": "R", "2": "D", "3": "S", "4": "T"}

    def _compute_inter_str(self) -> np.ndarray:
        """Interaction codes as letter strings: 1 reflection 'R', 2 diffraction 'D', 3 scattering 'S', 4 transmission
        'T'; LoS (0) is '', no path is 'n' (dataset.py:639-655: the code's float text without its '.0', digit by digit)."""
        inter = self._inter_host()
        table = str.maketrans(self._INTER_LETTERS)
        codes, inverse = np.unique(inter.astype(str), return_inverse=True)      # few distinct codes: translate each once
        words = np.array(["n" if s == "nan" else s[:-2].translate(table) for s in codes.tolist()])
        return words[inverse].reshape(inter.shape)

    # -------------------------------------------------------------- user grid and index helpers (dataset.py:702-795)
    def _compute_grid_info(self) -> Dict[str, np.ndarray]:
        """Distinct x / y receiver coordinates -> grid_size [nx, ny] and the mean spacing along each axis."""
        pos = np.asarray(self.rx_pos)
        xs, ys = np.unique(pos[:, 0]), np.unique(pos[:, 1])
        return {"grid_size": np.array([len(xs), len(ys)]),
                "grid_spacing": np.array([np.mean(np.diff(xs)), np.mean(np.diff(ys))])}

    def _is_valid_grid(self) -> bool:
        return np.prod(self.grid_size) == self.n_ue

    def subset(self, idxs) -> "Dataset":
        """New Dataset of the selected users (dataset.py:739-773): shared objects (scene, materials, load / ray-tracing
        parameters) by reference, every public array whose first axis is the user axis indexed by `idxs`, everything
        else as is; private (cached per-path) entries are dropped and recomputed on demand.  Device-resident rays stay
        on the device."""
        def take(value):
            if isinstance(value, np.ndarray):
                return value[idxs]
            import torch
            return value[torch.as_tensor(np.asarray(idxs), device=value.device)]
        return self._with_users(len(idxs), take, self.to_dict().items(), skip=_TIME_KEYS + _RX_KEYS + _TX_KEYS)

    def _with_users(self, n_new: int, take, items, skip=(), fixed=()) -> "Dataset":
        """New Dataset of `n_new` users from `items`, (key, value) pairs of this one: the shared objects by reference,
        every array (NumPy or torch) whose first axis is the user axis through `take`, everything else as is.  Private
        entries and the keys in `skip` are dropped; the keys in `fixed` never count as per-user arrays."""
        n_ue = self.n_ue
        init = {k: self._host(k) for k in SHARED_PARAMS if k in self._data}
        init[c.N_UE_PARAM_NAME] = n_new
        out = Dataset(init)
        for key, value in items:
            if key.startswith("_") or key in init or key in skip:
                continue
            if key not in fixed and (
                    (isinstance(value, np.ndarray) and value.ndim > 0 and value.shape[0] == n_ue) or
                    (hasattr(value, "detach") and value.dim() > 0 and value.shape[0] == n_ue)):
                value = take(value)
            out[key] = value
        return out

    # -------------------------------------------------------------- channel time series (extension)
    def set_velocities(self, rx_vel=None, tx_vel=None) -> None:
        """Per-path Doppler from the velocities of the terminals (extension).  ``rx_vel``: [3] or [n_ue, 3] in m/s, global
        x / y / z; ``tx_vel``: [3]; None is 0.  Stores them as ``rx_vel`` float64 [n_ue, 3] and ``tx_vel`` float64 [3] and
        writes the two ray matrices the Doppler model reads, float32 [n_ue, n_paths]:

            doppler_vel[u, l] = -(rx_vel[u] . k(aoa_az, aoa_el) + tx_vel . k(aod_az, aod_el))     # NaN where the path is
            doppler_acc       = 0
            k(phi, theta)     = (sin theta cos phi, sin theta sin phi, cos theta)                 # el is the zenith angle

        from the stored, unrotated angles, in float64, rounded once.  k is the vector of the array response
        ``exp(+j k p . k)``: a terminal displaced by v t sees the phase an array element at v t would see, so a path a
        terminal moves towards gets a negative ``doppler_vel`` and a positive Doppler shift (``doppler_shifts``).  Changes
        no result of a call with ``enable_doppler = 0``."""
        from .doppler import check_velocity, doppler_velocity
        rx = check_velocity("set_velocities", _RX_VEL, rx_vel, self.n_ue)
        tx = check_velocity("set_velocities", _TX_VEL, tx_vel)
        vel = doppler_velocity(self[c.AOA_AZ_PARAM_NAME], self[c.AOA_EL_PARAM_NAME], self[c.AOD_AZ_PARAM_NAME],
                               self[c.AOD_EL_PARAM_NAME], rx, tx)
        self._data[_RX_VEL], self._data[_TX_VEL] = rx, tx
        self._data[c.DOPPLER_VEL_PARAM_NAME] = vel
        self._data[c.DOPPLER_ACC_PARAM_NAME] = vel.new_zeros(vel.shape) if hasattr(vel, "detach") else np.zeros_like(vel)

    def _doppler_matrices(self, who: str):
        """(doppler_vel, doppler_acc or None) as stored - v3 data or `set_velocities`; without the first a ValueError."""
        vel = self._data.get(c.DOPPLER_VEL_PARAM_NAME)
        if vel is None:
            raise ValueError(f"{who}: the dataset has no per-path Doppler (doppler_vel): call set_velocities(rx_vel, tx_vel) "
                             "first, or load rays that carry doppler_vel / doppler_acc")
        return vel, self._data.get(c.DOPPLER_ACC_PARAM_NAME)

    def _time_carrier(self, who: str, carrier_freq) -> float:
        """`carrier_freq`, else rt_params.frequency, in Hz; neither finite and > 0 is a ValueError."""
        fc = self._carrier_freq() if carrier_freq is None else carrier_freq
        try:
            fc = float(fc)
        except (TypeError, ValueError):
            fc = float("nan")
        if not (np.isfinite(fc) and fc > 0):
            raise ValueError(f"{who}: no carrier frequency: pass carrier_freq (Hz, finite and > 0) or set rt_params.frequency")
        return fc

    def doppler_shifts(self, carrier_freq=None) -> np.ndarray:
        """Doppler shift of every path in Hz, ``-(f_c / c) * doppler_vel``: NumPy float64 [n_ue, n_paths], NaN where there
        is no path.  ``f_c``: ``carrier_freq``, else ``rt_params.frequency``."""
        from .doppler import LIGHTSPEED
        fc = self._time_carrier("doppler_shifts", carrier_freq)
        vel, _ = self._doppler_matrices("doppler_shifts")
        vel = vel.detach().cpu().numpy() if hasattr(vel, "detach") else np.asarray(vel)
        return -(fc / LIGHTSPEED) * vel.astype(np.float64)

    def at_times(self, times, carrier_freq=None) -> "Dataset":
        """The dataset at ``times`` (a scalar or a 1-D array of T finite seconds) as a plain Dataset of T * n_ue users,
        time-major: row t * n_ue + u is user u at times[t] (extension).  Every ``compute_*`` works on it unchanged.

        A snapshot turns each path's phase and nothing else:

            phase[t, u, l] = wrap(phase[u, l] - 360 (f_c / c) (doppler_vel[u, l] t + doppler_acc[u, l] t^2 / 2))

        in float64, wrapped into [-180, 180) and rounded to float32 once; where the turn is 0 the stored phase is kept bit
        for bit, NaN stays NaN.  ``f_c``: ``carrier_freq``, else ``rt_params.frequency``.  Delays, angles and powers stay
        what they are: the model holds while |v| t is small against the distances of the scene.  The kernels' own term of
        ``enable_doppler = 1`` (a phase per path from its delay) multiplies on top; its cross term a t tau is not modelled.

        Every public array whose first axis is the user axis is tiled (as ``subset`` indexes it), shared objects are held
        by reference, ``ch_params``, ``bs_fov`` and ``ue_fov`` are copied, cached results are not carried.  Rays in HBM
        are advanced there; with host rays nothing here touches the GPU.  The view also holds ``times`` [T], ``n_times``
        and ``n_ue_per_time``; ``split_times(x)`` gives a result [T * n_ue, ...] as [T, n_ue, ...].  A UE keeps its
        orientation: a (3, 2) rotation range is drawn once for the n_ue users and tiled; a per-user rotation passed to
        the view itself has to be [T * n_ue, 3].  No Doppler matrices (``set_velocities``), a ``times`` that is empty, not
        finite or more than 1-D, or no carrier frequency raise ValueError."""
        from .doppler import check_times
        t, _ = check_times("at_times", times)
        return self._time_view("at_times", t, carrier_freq)

    def _time_view(self, who: str, t: np.ndarray, carrier_freq, only=None) -> "Dataset":
        """`at_times` for the checked float64 `t` [T].  `only`: the public keys to carry (a block of the channel calls
        carries what the call reads and no more)."""
        from .doppler import advance_phase
        fc = self._time_carrier(who, carrier_freq)
        vel, acc = self._doppler_matrices(who)
        T, n_ue = len(t), int(self.n_ue)
        phase = advance_phase(self[c.PHASE_PARAM_NAME], vel, acc, t, fc)
        view = self._tiled_view(T, {c.PHASE_PARAM_NAME: phase}, only, skip=_TIME_KEYS)
        d = view._data
        d[_TIMES], d[_N_TIMES], d[_N_UE_PER_TIME] = t.copy(), T, n_ue
        return view

    def _tiled_view(self, reps: int, replaced, only=None, skip=(), users=None) -> "Dataset":
        """What the views of `at_times`, `with_rx_combiner` and `with_tx_precoder` share: a Dataset of `reps` * n_ue users,
        every public per-user array tiled, the ray matrices in `replaced` (key -> the matrix of the view) in place of the
        tiled ones, the stored parameters tiled (`_tiled_params`) with the rotations drawn for them, the fields of view
        copied, no cached result.  `only`: the public keys to carry; `skip`: keys never carried; `users`: a slice of the
        users to tile in place of all n_ue (a block of `compute_mu_rate`)."""
        cached = (set(self._computed_attributes) - {c.CH_PARAMS_PARAM_NAME}) | set(_VIEW_RESULTS) | set(replaced)
        keys = [k for k in self._data if not k.startswith("_") and k not in cached and (only is None or k in only)]
        users = slice(0, int(self.n_ue)) if users is None else users
        view = self._with_users(reps * (users.stop - users.start), lambda v: _tile_users(v[users], reps),
                                ((k, self._host(k)) for k in keys), skip=skip, fixed=_NOT_PER_USER)
        d = view._data
        d.update(replaced)
        if c.CH_PARAMS_PARAM_NAME in d:
            d[c.CH_PARAMS_PARAM_NAME] = self._tiled_params(self._data[c.CH_PARAMS_PARAM_NAME], reps, users)
            drawn = self._data.get(_UE_ROT_RESOLVED)                       # the parent's draw: the same UEs
            if drawn is not None:
                d[_UE_ROT_RESOLVED] = np.tile(drawn[users], (reps, 1))
        for k in _FOV_KEYS:
            if isinstance(d.get(k), np.ndarray):
                d[k] = d[k].copy()
        return view

    @staticmethod
    def _tiled_params(params: ChannelGenParameters, T: int, users=None) -> ChannelGenParameters:
        """A copy of `params` for T * n_ue users: a per-user UE rotation [n_ue, 3] is tiled - the rows of the slice `users`
        where one is given - everything else holds as is."""
        params = params.deepcopy()
        rot = np.asarray(params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_ROTATION])
        if rot.ndim == 2 and rot.shape != (3, 2):
            params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_ROTATION] = np.tile(rot if users is None else rot[users], (T, 1))
        return params

    def split_times(self, x):
        """A result of a ``compute_*`` on a view of ``at_times`` - an array or tensor [T * n_ue, ...], or a tuple or dict
        of them - as [T, n_ue, ...]: a view of the same memory, never a copy."""
        T, n = self._data.get(_N_TIMES), self._data.get(_N_UE_PER_TIME)
        if T is None:
            raise ValueError("split_times: this dataset is not a view of at_times")
        return self._split_users("split_times", x, T, n, "n_times * n_ue")

    @staticmethod
    def _split_users(who: str, x, outer: int, inner: int, what: str):
        """`x` - an array or tensor whose first axis holds `outer` * `inner` users (`what`), or a tuple, list or dict of
        them - as [outer, inner, ...]: a view of the same memory, never a copy."""
        if isinstance(x, Mapping):
            return type(x)({k: Dataset._split_users(who, v, outer, inner, what) for k, v in x.items()})
        if isinstance(x, (tuple, list)):
            return type(x)(Dataset._split_users(who, v, outer, inner, what) for v in x)
        shape = tuple(x.shape)
        if not shape or shape[0] != outer * inner:
            raise ValueError(f"{who}: the first axis must be {what} = {outer * inner}, got shape {shape}")
        if hasattr(x, "detach"):
            return x.view((outer, inner) + shape[1:])
        y = x.view()
        y.shape = (outer, inner) + shape[1:]                                # raises where NumPy would have to copy
        return y

    def _time_blocks(self, T: int):
        """(begin, count) of the blocks of snapshots a channel call over time runs in: the tiled ray matrices of a block
        stay under _TIME_BLOCK_BYTES."""
        per_snapshot = 4 * int(self.n_ue) * self._loaded_paths() * (len(c.RAY_FIELDS) + 2)
        step = max(1, int(_TIME_BLOCK_BYTES) // max(per_snapshot, 1))
        return [(b, min(step, T - b)) for b in range(0, T, step)]

    def _time_call(self, who: str, params, times, carrier_freq):
        """The checks every channel call with `times` makes before any GPU work: (validated parameters, float64 times [T],
        whether `times` was a scalar, the carrier frequency)."""
        from .doppler import check_times
        t, scalar = check_times(who, times)
        fc = self._time_carrier(who, carrier_freq)
        self._doppler_matrices(who)
        return self._call_params(params), t, scalar, fc

    def _in_hbm(self, keys) -> "Dataset":
        """A Dataset of the same users with `keys` of this one, its per-user NumPy arrays uploaded as they are (dtype kept):
        the source of the block views of a channel call over time.  The rays then cross PCIe once, untiled, and the tiling
        and the advance run in HBM in the same float64 steps as on the host."""
        import torch
        dev, n_ue = _engine().device, int(self.n_ue)
        src = Dataset({k: self._host(k) for k in SHARED_PARAMS if k in self._data})
        d = src._data
        d[c.N_UE_PARAM_NAME] = n_ue
        for k in keys:
            if k not in self._data:
                continue
            v = self._host(k)
            if isinstance(v, np.ndarray) and k not in _NOT_PER_USER and v.ndim > 0 and v.shape[0] == n_ue:
                v = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            d[k] = v
        if _UE_ROT_RESOLVED in self._data:
            d[_UE_ROT_RESOLVED] = self._data[_UE_ROT_RESOLVED]
        return src

    def _block_view(self, who: str, params, t: np.ndarray, fc: float) -> "Dataset":
        """The view of one block of snapshots with `params` stored for its T * n_ue users."""
        view = self._time_view(who, t, fc, only=_BLOCK_KEYS)
        view._call_params(self._tiled_params(params, len(t)))
        return view

    def _channels_over_time(self, params, times, carrier_freq, spatial_wideband=False):
        """`compute_channels(times=...)`: one stage 1 and one stage 2 (or one single pass) per block of snapshots, written
        time-major where they are returned from - no channel-sized tensor is ever transposed."""
        params, t, scalar, fc = self._time_call("compute_channels", params, times, carrier_freq)
        wideband_fc = self._wideband_carrier(params, spatial_wideband, fc)
        self._near_field_checked(params, spatial_wideband, config.get("fd_kernel_variant", 0))     # before the rays move
        to_host = config.get("channel_output", "numpy") != "torch"
        shape = self._channel_shape(params)
        if not params[c.PARAMSET_FD_CH]:
            shape = shape[:3] + (min(shape[3], self._loaded_paths()),)
        T, n_ue = len(t), shape[0]
        if to_host:                                                            # the whole series, before any GPU work
            self._guard_host_copy(8 * T * int(np.prod(shape)))
        blocks = self._time_blocks(T)
        src = self._in_hbm(_BLOCK_KEYS)
        out = None
        for b, nb in blocks:
            view = src._block_view("compute_channels", params, t[b:b + nb], fc)
            dst = None
            if len(blocks) > 1 and not to_host:
                if out is None:
                    import torch
                    out = torch.empty((T,) + shape, dtype=torch.complex64, device=_engine().device)
                dst = out[b:b + nb].view((nb * n_ue,) + shape[1:])
            np.random.seed(1001)
            H, max_delay = view._channels_once(view.ch_params, to_host, out=dst, wideband_fc=wideband_fc)
            if b == 0 and params[c.PARAMSET_FD_CH]:                            # the delays are those of every snapshot
                self._warn_symbol_duration(max_delay, params[c.PARAMSET_OFDM])
            if len(blocks) == 1:
                out = H.reshape((T,) + shape)
            elif to_host:
                if out is None:
                    out = np.empty((T,) + shape, dtype=np.complex64)
                out[b:b + nb] = H.reshape((nb,) + shape)
        return out[0] if scalar else out

    def _iter_channels_over_time(self, params, chunk_users, times, carrier_freq, spatial_wideband=False):
        """`iter_channels(times=...)`: stage 1 once per block of snapshots, stage 2 per snapshot and user chunk."""
        params, t, _, fc = self._time_call("iter_channels", params, times, carrier_freq)
        wideband_fc = self._wideband_carrier(params, spatial_wideband, fc)
        self._near_field_checked(params, spatial_wideband, config.get("fd_kernel_variant", 0))
        n_ue, step = int(self.n_ue), max(1, int(chunk_users))
        variant = int(config.get("fd_kernel_variant", 0))
        src = self._in_hbm(_BLOCK_KEYS)
        for b, nb in self._time_blocks(len(t)):
            view = src._block_view("iter_channels", params, t[b:b + nb], fc)
            np.random.seed(1001)
            eng, prep = view._run_prep(want_side="light", inputs=view._prep_inputs(wideband_fc, config.get("fd_kernel_variant", 0)))
            for i in range(nb):
                for ub in range(0, n_ue, step):
                    cnt = min(step, n_ue - ub)
                    yield b + i, ub, eng.channels_to_host(prep, variant=variant, user_begin=i * n_ue + ub, user_count=cnt)

    # -------------------------------------------------------------- near field (extension)
    def near_field(self, carrier_freq=None) -> "Dataset":
        """The dataset with spherical-wavefront array responses, as a plain Dataset of the same users that shares this one's
        arrays (extension).  Every ``compute_*`` that builds its array tables from the path records works on it unchanged
        and sees each path as a spherical wave from a point ``R = delay * f_c`` wavelengths away along the path's direction
        (the total path length), seen from element 0 of each array, in place of the plane wave:

            psi[e, l] = R_l - sqrt(R_l^2 - 2 R_l q[e, l] + d^2 (y_e^2 + z_e^2))           # revolutions
            q[e, l]   = d (y_e sin theta_l sin phi_l + z_e cos theta_l)                   # the plane-wave phase, R -> inf

        (include/deepmimo_amd.h, DMX_FLAG_NEAR_FIELD; ``dm.near_field_response``).  ``f_c``: ``carrier_freq`` in Hz, else
        ``rt_params.frequency``; it is kept as ``near_field_carrier`` and is the carrier of the Doppler term too.  The
        amplitude stays uniform over the aperture, the radius is exact for LoS and specular chains and too large for
        diffracted or scattered paths, and the two ends are curved independently.

        ``subset`` and ``at_times`` of the view are near-field views.  ValueError before any GPU work: a carrier frequency
        that is missing or not finite and > 0; in a call on the view the time domain, ``rx_filter = 1``,
        ``spatial_wideband=True``, ``config('fd_kernel_variant')`` other than 0 or 1 (channel calls run the fp32 vector
        kernel; the single pass is not taken), ``compute_beam_channels``, ``with_rx_combiner`` and
        ``compute_beam_pair_power`` (the combiner's response is still plane-wave)."""
        if _N_RX_BEAMS in self._data:
            raise ValueError("near_field: not covered on a view of with_rx_combiner (the combiner's response to a path is the "
                             "plane-wave one)")
        if _N_TX_BEAMS in self._data:
            raise ValueError("near_field: not covered on a view of with_tx_precoder (the precoder's response to a path is the "
                             "plane-wave one)")
        fc = self._time_carrier("near_field", carrier_freq)
        view = self._with_users(int(self.n_ue), lambda v: v,
                                ((k, self._host(k)) for k in list(self._data) if k not in self._computed_attributes
                                 or k == c.CH_PARAMS_PARAM_NAME), skip=_VIEW_RESULTS)
        d = view._data
        if c.CH_PARAMS_PARAM_NAME in d:
            d[c.CH_PARAMS_PARAM_NAME] = d[c.CH_PARAMS_PARAM_NAME].deepcopy()
            drawn = self._data.get(_UE_ROT_RESOLVED)
            if drawn is not None:
                d[_UE_ROT_RESOLVED] = drawn
        d[_NEAR_FIELD] = fc
        return view

    # -------------------------------------------------------------- UE receive combining (extension)
    def with_rx_combiner(self, codebook="dft", params: Optional[ChannelGenParameters] = None) -> "Dataset":
        """The dataset behind a UE combining codebook W [Q, M_rx] as a plain Dataset of Q * n_ue single-antenna users,
        combiner-major: row q * n_ue + u is user u behind row q, the UE beam q (extension).  Every ``compute_*`` works on
        it unchanged and gives what it would give for ``W[q] @ H[u]``, with no [n_ue, M_rx, ...] tensor written.  On the
        view M_rx = 1, so ``compute_angle_delay(..., output="power")`` is ``|W[q] @ H[u]|**2`` per UE beam in the angle-delay
        domain: its sum over the receive elements has one term.

        A combiner row multiplies the complex gain of each path and nothing else:

            e[u, q, l]  = sum_r W[q, r] exp(j 2 pi spacing (y_r sin theta sin phi + z_r cos theta))      # r = y + Mh z
            power[q, u, l] = power[u, l] + 10 log10(max(|e|^2, 2^-100))
            phase[q, u, l] = wrap(phase[u, l] + degrees(arg e))

        in float64, rounded to float32 once (``deepmimo_amd.combiner``); W is applied without a conjugate, as
        ``codebook @ H`` applies a BS codebook.  theta, phi are the arrival angles stage 1 gives for ``params`` (or the stored
        parameters): rotated by the UE rotation and filtered by the field of view.  The angles themselves stay what they
        are, so the UE rotation, the UE radiation pattern and ``ue_fov`` act in the view as they do in the parent; a path
        without an angle keeps its stored power and phase.  ``codebook``: ``"dft"`` (``dm.dft_codebook`` of the UE panel) or
        a finite complex array [Q, M_rx], Q >= 1; anything else raises ValueError before any GPU work.

        Every public array whose first axis is the user axis is tiled (as ``at_times`` tiles it), shared objects are held
        by reference, cached results are not carried; rays in HBM are combined there.  The view stores ``ch_params`` as a
        copy of the parameters with ``ue_antenna.shape = [1, 1]`` (a per-user rotation [n_ue, 3] tiled to [Q * n_ue, 3]; a
        (3, 2) rotation range keeps the parent's draw, tiled), ``rx_combiner`` [Q, M_rx], ``n_rx_beams`` and
        ``n_ue_per_rx_beam``; ``split_rx_beams(x)`` gives a result [Q * n_ue, ...] as [Q, n_ue, ...].  The view is bound to
        the UE array, rotation and field of view it was built with: parameters given to one of its calls have to keep
        them, and a UE shape other than [1, 1] raises ValueError.  It composes with ``at_times`` in either order; the
        outer view's split applies to the first axis."""
        from .combiner import check_rx_codebook
        self._refuse_on_near_field("with_rx_combiner", "the combiner's response to a path is the plane-wave one")
        params = self._call_params(params)
        W = check_rx_codebook("with_rx_combiner", codebook, params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_SHAPE])
        return self._rx_view(W, *self._rx_arrival_angles())

    def _rx_arrival_angles(self):
        """(theta, phi) of `with_rx_combiner` for the stored parameters: stage 1's rotated arrival zenith and azimuth in
        radians, float64 [n_ue, L], NaN where the field of view masks the path (what ``aoa_el_rot_fov`` / ``aoa_az_rot_fov``
        hold), where the rays live: NumPy arrays for host rays, tensors in HBM for rays in HBM."""
        return self._stage1_angles("aoa_el_rot", "aoa_az_rot")

    def _tx_departure_angles(self):
        """(theta, phi) of `with_tx_precoder` for the stored parameters: `_rx_arrival_angles` for the departure side, stage
        1's ``aod_el_rot`` / ``aod_az_rot`` rotated by the BS rotation, NaN where the field of view masks the path."""
        return self._stage1_angles("aod_el_rot", "aod_az_rot")

    def _stage1_angles(self, el: str, az: str):
        """The two rotated angles `el`, `az` of stage 1's side products with the field of view applied, where the rays live."""
        np.random.seed(1001)
        _, prep = self._run_prep(want_side=True)
        theta, phi, mask = prep.side[el], prep.side[az], prep.side["fov_mask"]
        if mask is not None:
            theta, phi = theta.masked_fill(mask == 0, float("nan")), phi.masked_fill(mask == 0, float("nan"))
        if not hasattr(self[c.POWER_PARAM_NAME], "detach"):
            theta, phi = theta.cpu().numpy(), phi.cpu().numpy()
        return theta, phi

    def _rx_view(self, W: np.ndarray, theta, phi, only=None) -> "Dataset":
        """`with_rx_combiner` for the checked complex128 `W` [Q, M_rx] and the arrival angles of the stored parameters.
        `only`: the public keys to carry (a block of `compute_beam_pair_power` carries what the call reads and no more)."""
        from .combiner import combine_all
        ue = self.ch_params[c.PARAMSET_ANT_UE]
        power, phase = combine_all(self[c.POWER_PARAM_NAME], self[c.PHASE_PARAM_NAME], W, ue[c.PARAMSET_ANT_SHAPE],
                                   float(ue[c.PARAMSET_ANT_SPACING]), theta, phi)
        view = self._tiled_view(len(W), {c.POWER_PARAM_NAME: power, c.PHASE_PARAM_NAME: phase}, only, skip=_RX_KEYS)
        d = view._data
        d[c.CH_PARAMS_PARAM_NAME][c.PARAMSET_ANT_UE][c.PARAMSET_ANT_SHAPE] = np.array([1, 1])
        d[_RX_COMBINER], d[_N_RX_BEAMS], d[_N_UE_PER_RX_BEAM] = W.copy(), len(W), int(self.n_ue)
        return view

    def split_rx_beams(self, x):
        """A result of a ``compute_*`` on a view of ``with_rx_combiner`` - an array or tensor [Q * n_ue, ...], or a tuple or
        dict of them - as [Q, n_ue, ...]: a view of the same memory, never a copy."""
        Q, n = self._data.get(_N_RX_BEAMS), self._data.get(_N_UE_PER_RX_BEAM)
        if Q is None:
            raise ValueError("split_rx_beams: this dataset is not a view of with_rx_combiner")
        return self._split_users("split_rx_beams", x, Q, n, "n_rx_beams * n_ue")

    # -------------------------------------------------------------- transmit precoding (extension)
    def with_tx_precoder(self, codebook="dft", beams=None, params: Optional[ChannelGenParameters] = None) -> "Dataset":
        """The dataset behind BS precoders as a plain Dataset of users served by a single-antenna base station - the mirror
        of ``with_rx_combiner`` (extension).  Every ``compute_*`` works on it unchanged and gives what it would give for
        ``H[u] @ f``, with no [n_ue, ..., M_tx, ...] tensor written.  ``codebook``: ``"dft"`` (``dm.dft_codebook`` of the BS
        panel) or a finite complex array F [B, M_tx], B >= 1.  ``beams`` says which row serves which user:

            None            all B beams: B * n_ue users, beam-major, row b * n_ue + u is user u behind F[b]
            int [n_ue]      n_ue users, row u is user u behind F[beams[u]]
            int [J, n_ue]   J * n_ue users, row j * n_ue + u is user u behind F[beams[j, u]]

        with values in -1 .. B - 1; -1 is no transmission, a row without paths (its power, delay, angles and interactions are
        NaN - ``num_paths`` 0, ``los`` -1 - and its phase the stored one).  Weights of a user's own - a zero-forcing
        precoder, say - are the case B = n_ue, ``beams = np.arange(n_ue)``.  A precoder row multiplies the complex gain of
        each path and nothing else:

            e[j, u, l]     = sum_t F[beams[j, u], t] exp(j 2 pi spacing (y_t sin theta sin phi + z_t cos theta))   # t = y + Mh z
            power[j, u, l] = power[u, l] + 10 log10(max(|e|^2, 2^-100))
            phase[j, u, l] = wrap(phase[u, l] + degrees(arg e))

        in float64, rounded to float32 once (``deepmimo_amd.combiner.precode_rays``); F is applied without a conjugate, as
        ``codebook @ H`` applies it.  theta, phi are the departure angles stage 1 gives for ``params`` (or the stored
        parameters): rotated by the BS rotation and filtered by the field of view.  The angles themselves stay what they
        are, so the BS rotation, the BS radiation pattern and ``bs_fov`` act in the view as they do in the parent; a path
        without an angle keeps its stored power and phase.

        The view is built as ``with_rx_combiner`` builds its own: per-user arrays tiled, shared objects by reference, no
        cached results, rays in HBM precoded there.  It stores ``ch_params`` with ``bs_antenna.shape = [1, 1]``,
        ``tx_precoder`` [B, M_tx], ``n_tx_beams`` (B, J, or 1 for ``beams`` [n_ue]) and ``n_ue_per_tx_beam``;
        ``split_tx_beams(x)`` gives a result as [n_tx_beams, n_ue, ...].  The view is bound to the BS array, rotation and
        field of view it was built with; a BS shape other than [1, 1] in a later call raises ValueError.  It composes with
        ``at_times`` and ``with_rx_combiner`` in either order.  A bad codebook or ``beams`` raises ValueError before any GPU
        work; a near-field view refuses the call."""
        from .combiner import check_tx_beams, check_tx_codebook
        who = "with_tx_precoder"
        self._refuse_on_near_field(who, "the precoder's response to a path is the plane-wave one")
        params = self._call_params(params)
        F = check_tx_codebook(who, codebook, params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE])
        n_ue = int(self.n_ue)
        if beams is None:
            idx = np.broadcast_to(np.arange(len(F), dtype=np.int64)[:, None], (len(F), n_ue))
        else:
            idx = check_tx_beams(who, beams, n_ue, len(F))
        return self._tx_view(F, idx, *self._tx_departure_angles())

    def _tx_view(self, F: np.ndarray, idx: np.ndarray, theta, phi, scale=None, only=None, users=None) -> "Dataset":
        """`with_tx_precoder` for the checked complex128 `F` [B, M_tx], the rows `idx` int64 [J, n] and the departure angles
        of the stored parameters.  `scale`: real [J, n] on the responses (the power split of `compute_mu_rate`); `only`:
        the public keys to carry; `users`: the slice of n users `idx` and `scale` are for, all n_ue without one."""
        from .combiner import precode_rays
        bs = self.ch_params[c.PARAMSET_ANT_BS]
        sl = slice(0, int(self.n_ue)) if users is None else users
        power, phase = precode_rays(self[c.POWER_PARAM_NAME][sl], self[c.PHASE_PARAM_NAME][sl], F, idx, bs[c.PARAMSET_ANT_SHAPE],
                                    float(bs[c.PARAMSET_ANT_SPACING]), theta[sl], phi[sl], scale)
        view = self._tiled_view(len(idx), {c.POWER_PARAM_NAME: power, c.PHASE_PARAM_NAME: phase}, only, skip=_TX_KEYS, users=users)
        d = view._data
        d[c.CH_PARAMS_PARAM_NAME][c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE] = np.array([1, 1])
        d[_TX_PRECODER], d[_N_TX_BEAMS], d[_N_UE_PER_TX_BEAM] = F.copy(), len(idx), sl.stop - sl.start
        # a row that does not transmit has no paths: `num_paths` counts arrival angles and `los` reads the interactions, so
        # the other ray matrices of the row (tiled copies of the view's own) go with its power; the phase stays as stored
        rows = np.flatnonzero(np.asarray(idx).reshape(-1) < 0)
        for k in c.RAY_FIELDS if len(rows) else ():
            v = d.get(k)
            if k in (c.POWER_PARAM_NAME, c.PHASE_PARAM_NAME) or v is None:
                continue
            if hasattr(v, "detach"):
                if v.is_floating_point():
                    import torch
                    v[torch.as_tensor(rows, device=v.device)] = float("nan")
            elif v.dtype.kind == "f":
                v[rows] = np.nan
        return view

    def split_tx_beams(self, x):
        """A result of a ``compute_*`` on a view of ``with_tx_precoder`` - an array or tensor [n_tx_beams * n_ue, ...], or a
        tuple or dict of them - as [n_tx_beams, n_ue, ...]: a view of the same memory, never a copy."""
        J, n = self._data.get(_N_TX_BEAMS), self._data.get(_N_UE_PER_TX_BEAM)
        if J is None:
            raise ValueError("split_tx_beams: this dataset is not a view of with_tx_precoder")
        return self._split_users("split_tx_beams", x, J, n, "n_tx_beams * n_ue")

    def _mu_blocks(self, G: int):
        """(begin, count) of the blocks of users `compute_mu_rate` runs in: the ray matrices of the G links of a block stay
        under _TIME_BLOCK_BYTES, the rule of the tiled ray matrices of `_time_blocks`."""
        n_ue = int(self.n_ue)
        per_user = 4 * self._loaded_paths() * (len(c.RAY_FIELDS) + 2) * G
        step = max(1, int(_TIME_BLOCK_BYTES) // max(per_user, 1))
        return [(b, min(step, n_ue - b)) for b in range(0, n_ue, step)]

    def compute_mu_rate(self, codebook, beams, groups, params: Optional[ChannelGenParameters] = None, *, snr_db=None,
                        per_subcarrier: bool = False, details: bool = False):
        """Per-user downlink rate in bit/s/Hz while the base station serves the user's group - the users co-scheduled with
        it, each on its own precoder - with no channel tensor written (extension).  ``codebook``: ``"dft"`` or F [B, M_tx] as
        in ``with_tx_precoder``; ``beams`` int [n_ue]: the row of F that serves each user; ``groups`` int [n_groups, G],
        1 <= G <= 8: the users served together, a row padded with -1.  A user is in at most one group; one in none is not
        scheduled.  With g_u the members of u's group, snr = 10 ** (snr_db / 10) and y_v = H[u, :, :, k] @ F[beams[v]]:

            N_k          = I + (snr / g_u) * sum(outer(y_v, y_v.conj()) for v in group(u) if v != u)
            rate_k[u, k] = log2 det(N_k + (snr / g_u) * outer(y_u, y_u.conj())) - log2 det(N_k)
            rate[u]      = rate_k[u].mean()

        the total power split equally over the streams of the group; the rows of F are used as given, unit-norm rows keep
        the total at snr.  ``snr_db`` (required, keyword-only): total transmit power over noise power per subcarrier.

        Returns ``rate`` float32 [n_ue], 0 for a user that is not scheduled or has no path; with ``per_subcarrier`` also
        ``rate_k`` float32 [n_ue, K]; with ``details`` also ``partners`` (int32 [n_ue, G - 1]: the other members of the group
        in the order of its row, padded with -1) and ``stream_snr`` (float32 [n_ue, G], linear: (snr / g_u) times the summed
        power of the kept paths behind the beam, the own beam first, then the partners'), in that order: NumPy arrays by
        default, the HBM-resident torch tensors when ``config('channel_output') == 'torch'``.

        The beams of a group, seen through user u's rays, are G single-antenna links to u (``with_tx_precoder``): the call
        builds them a block of users at a time and runs the multi-cell rate kernel of ``MacroDataset.compute_cell_rate`` on
        them.  ValueError before any GPU work: ``snr_db`` missing or not finite, a bad codebook, ``beams`` that is no int
        array [n_ue], a scheduled user whose beam is outside 0 .. B - 1, ``groups`` that is no 2-D int array, G outside
        1 .. 8, an index outside -1 .. n_ue - 1, a user that appears twice, the time domain, ``rx_filter = 1``, a UE array of
        more than 8 elements, a near-field view.  Not cached.

        Several streams per user: ``beams`` int [n_ue, L], row u the codebook rows of user u's streams, -1 padding a user
        with fewer (the first entry of a scheduled user must be a row of F), G * L <= 8.  Link j * L + i is then stream i
        of member j of the group - the user itself is member 0 - seen through the user's rays; the total power is split
        equally over the valid streams of the group, and the links 0 .. L - 1 that exist are the user's serving set
        (``MacroDataset.compute_cell_rate(serving_set=...)``): ``rate`` is the sum rate of the user's streams at a joint
        receiver, the partners' streams coloured noise.  ``stream_snr`` is then float32 [n_ue, G * L] in link order.
        ``beams`` [n_ue, 1] gives the bits of ``beams`` [n_ue]."""
        import torch
        from .combiner import check_tx_codebook, mu_partners
        from .engine import check_cell_rate_call
        who = "compute_mu_rate"
        self._required_snr(who, snr_db)
        self._refuse_on_near_field(who, "the precoder's response to a path is the plane-wave one")
        params = self._call_params(params)
        n_ue = int(self.n_ue)
        F = check_tx_codebook(who, codebook, params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE])
        try:
            own = np.asarray(beams.detach().cpu().numpy() if hasattr(beams, "detach") else beams)
        except (TypeError, ValueError):
            own = np.empty(0, object)
        multi = own.ndim == 2 and own.shape[0] == n_ue and own.shape[1] >= 1       # [n_ue, L]: streams per user
        if own.dtype.kind not in "iu" or not (own.shape == (n_ue,) or multi):
            raise ValueError(f"{who}: beams must be an integer array of shape ({n_ue},), the codebook row of each user, got "
                             f"{own.dtype} of shape {own.shape}")
        partners, group_size, scheduled = mu_partners(groups, n_ue, who)
        streams = np.where(scheduled[:, None], own.astype(np.int64).reshape(n_ue, -1), -1)   # [n_ue, L]; a user in no group: never read
        own, L = streams[:, 0], streams.shape[1]
        bad = scheduled & ((own < 0) | (own >= len(F)))
        if bad.any():
            u = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{who}: user {u} is scheduled on beam {int(own[u])}, outside 0 .. {len(F) - 1}")
        bad = (streams < -1) | (streams >= len(F))
        if bad.any():
            u, i = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError(f"{who}: stream {i} of user {u} is on beam {int(streams[u, i])}, outside -1 .. {len(F) - 1}")
        G = partners.shape[1] + 1
        if G * L > 8:
            raise ValueError(f"{who}: groups of {G} users with {L} streams each are {G * L} links, the call takes G * L <= 8")
        n_links = G * L
        link = params.deepcopy()
        link[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE] = np.array([1, 1])
        try:
            check_cell_rate_call([link] * n_links, [self._loaded_paths()] * n_links, snr_db)
        except ValueError as err:
            raise ValueError(f"{who}: {err}") from None
        # the link table: links 0 .. L - 1 the user's own beams, link j L + i stream i of its (j - 1)-th partner, all seen
        # through its rays; the power is split over the valid streams of the group
        idx = np.full((n_links, n_ue), -1, np.int64)
        idx[:L] = streams.T
        total = (streams >= 0).sum(axis=1)
        for j in range(1, G):
            has, mate = partners[:, j - 1] >= 0, np.maximum(partners[:, j - 1], 0)
            idx[j * L:(j + 1) * L] = np.where(has[None, :], streams[mate].T, -1)
            total = total + np.where(has, (streams[mate] >= 0).sum(axis=1), 0)
        scale = np.broadcast_to(1.0 / np.sqrt(np.maximum(total, 1).astype(np.float64)), (n_links, n_ue))
        if multi:                                                          # the links 0 .. L - 1 that exist are the user's set
            served = dict(serving_set=np.concatenate([streams >= 0, np.zeros((n_ue, n_links - L), bool)], axis=1))
        else:
            served = dict(serving=np.where(scheduled, 0, -1).astype(np.int32))
        src = self._in_hbm(_BLOCK_KEYS)                                    # the rays cross PCIe once, unprecoded
        theta, phi = src._tx_departure_angles()
        eng = _engine()
        parts = []
        for ub, nb in self._mu_blocks(n_links):
            users = slice(ub, ub + nb)
            links = [src._tx_view(F, idx[j:j + 1, users], theta, phi, scale[j:j + 1, users], only=_BLOCK_KEYS, users=users)
                     for j in range(n_links)]
            preps = []
            for view in links:
                np.random.seed(1001)
                preps.append(view._run_prep(want_side="light")[1])
            res = eng.cell_rate(preps, snr_db, per_subcarrier=per_subcarrier, details=details,
                                **{k: v[users] for k, v in served.items()})
            parts.append(res if isinstance(res, tuple) else (res,))
        got = [p[0] if len(p) == 1 else torch.cat(p) for p in zip(*parts)]
        res = got[:2] if per_subcarrier else got[:1]
        if details:
            res = res + [torch.from_numpy(partners).to(eng.device), got[-1]]
        return self._deliver(res[0] if len(res) == 1 else tuple(res))

    def compute_beam_pair_power(self, tx_codebook, rx_codebook="dft", params: Optional[ChannelGenParameters] = None,
                                return_best: bool = False, metric: str = "amplitude"):
        """Received power of every pair of a UE beam and a BS beam - the two-sided beam sweep in one call, with the semantics
        of ``compute_beam_power`` and no channel or beam-space tensor written anywhere (extension).  For a BS codebook F
        [B, M_tx] and a UE combining codebook W [Q, M_rx] (``"dft"``: ``dm.dft_codebook`` of the UE panel):

            amp[u, q, b]    = np.abs(np.einsum('qr,urtk,bt->uqbk', W, dataset.channel, F)).mean(axis=-1)  # computed on the GPU
            recv_bf_pwr_dbm = np.around(20 * np.log10(amp) + 30, 1), NaN where dataset.los == -1
            best_rx, best_tx = np.unravel_index(argmax over (q, b), (Q, B)), the first maximum, as float; NaN where
                               dataset.los == -1

        Returns ``recv_bf_pwr_dbm`` float64 [n_ue, Q, B] (and ``best_rx``, ``best_tx`` with ``return_best``): NumPy arrays,
        as ``compute_beam_power`` returns them.  The raw means stay available as ``dataset['beam_pair_mean_amplitude']``
        (float32 [n_ue, Q, B]).  W is applied without a conjugate, like F.  It runs the beam-power kernel on the
        ``with_rx_combiner`` view, a block of UE beams at a time.  A bad codebook on either side, the time domain,
        ``rx_filter = 1`` or a subcarrier index beyond the bound of the beam entry points raise ValueError before any GPU
        work.  ``metric="power"`` as in ``compute_beam_power``: the mean of ``np.abs(.) ** 2``, ``10 * np.log10``, and the raw
        means as ``dataset['beam_pair_mean_power']``; any other name raises ValueError alike."""
        import torch
        from .combiner import check_rx_codebook
        from .engine import check_beam_bound, check_beam_metric, check_selection
        who = "compute_beam_pair_power"
        power = check_beam_metric(who, metric)
        self._refuse_on_near_field(who, "the combiner's response to a path is the plane-wave one")
        params = self._call_params(params)
        bs_shape = params[c.PARAMSET_ANT_BS][c.PARAMSET_ANT_SHAPE]
        m_tx = int(bs_shape[0]) * int(bs_shape[1])
        W = check_rx_codebook(who, rx_codebook, params[c.PARAMSET_ANT_UE][c.PARAMSET_ANT_SHAPE])
        F = tx_codebook if hasattr(tx_codebook, "shape") else np.asarray(tx_codebook)
        if len(F.shape) != 2 or F.shape[1] != m_tx or F.shape[0] < 1:
            raise ValueError(f"{who}: the BS codebook must be an array [B, {m_tx}] with B >= 1, got shape {tuple(F.shape)}")
        if not params[c.PARAMSET_FD_CH]:
            raise ValueError(f"{who}: needs the frequency-domain channel (freq_domain = 1)")
        if params[c.PARAMSET_OFDM][c.PARAMSET_OFDM_LPF]:
            raise ValueError(f"{who}: ofdm.rx_filter = 1 is not covered")
        check_beam_bound(check_selection(params[c.PARAMSET_OFDM][c.PARAMSET_OFDM_SC_SAMP])[1])
        src = self._in_hbm(_BLOCK_KEYS)                                    # the rays cross PCIe once, uncombined
        theta, phi = src._rx_arrival_angles()
        no_paths = src[c.LOS_PARAM_NAME] == -1
        eng = _engine()
        F = eng._codebook(F, m_tx, min_beams=1)
        Q, n_ue, B = len(W), int(self.n_ue), int(F.shape[0])
        amp = torch.empty((n_ue, Q, B), dtype=torch.float32, device=eng.device)
        for b, nb in self._time_blocks(Q):
            view = src._rx_view(W[b:b + nb], theta, phi, only=_BLOCK_KEYS)
            np.random.seed(1001)
            _, prep = view._run_prep(want_side="light")
            # the block's small [nb, n_ue, B] result into its user-major place in HBM: a strided copy of the amplitudes alone
            amp[:, b:b + nb] = eng.beam_power(prep, F, want_best=False, metric=metric)[0].view(nb, n_ue, B).permute(1, 0, 2)
        amp = amp.cpu().numpy()
        self._data["beam_pair_mean_power" if power else "beam_pair_mean_amplitude"] = amp
        # compute_beam_power's np.around(20 * np.log10(amp) + 30, 1) in float32, then float64: the same operations per
        # element, in place on the one temporary - at 100k users x 4 x 64 pairs the passes over it are the cost of the call
        with np.errstate(divide="ignore"):
            dbm = np.log10(amp)
        dbm *= 10 if power else 20
        dbm += 30
        pwr = np.around(dbm, 1, out=dbm).astype(np.float64)
        pwr[no_paths] = np.nan
        if not return_best:
            return pwr
        best_rx, best_tx = (v.astype(float) for v in np.divmod(np.argmax(pwr.reshape(n_ue, Q * B), axis=1), B))
        best_rx[no_paths] = best_tx[no_paths] = np.nan
        return pwr, best_rx, best_tx

    def get_active_idxs(self) -> np.ndarray:
        """Users with at least one path (dataset.py:775-781)."""
        return np.where(self.num_paths > 0)[0]

    def get_uniform_idxs(self, steps) -> np.ndarray:
        """Every steps[0]-th column and steps[1]-th row of the user grid (dataset.py:783-795)."""
        from .generator_utils import get_uniform_idxs
        return get_uniform_idxs(self.n_ue, self.grid_size, steps)

    # -------------------------------------------------------------- field of view (dataset.py:423-448)
    def apply_fov(self, bs_fov: np.ndarray = np.array([360, 180]), ue_fov: np.ndarray = np.array([360, 180])) -> None:
        self._clear_cache_fov()
        self.bs_fov = bs_fov
        self.ue_fov = ue_fov

    def _clear_cache_fov(self) -> None:
        """dataset.py:515-535"""
        for k in (c.FOV_MASK_PARAM_NAME, c.NUM_PATHS_PARAM_NAME, c.LOS_PARAM_NAME, c.CHANNEL_PARAM_NAME,
                  c.PWR_LINEAR_ANT_GAIN_PARAM_NAME) + _FOV_ANGLE_KEYS:
            self._data.pop(k, None)

    def _clear_cache_rotated_angles(self) -> None:
        """dataset.py:358-378"""
        for k in _ROT_KEYS + (_UE_ROT_RESOLVED,):
            self._data.pop(k, None)
        self._clear_cache_fov()

    # -------------------------------------------------------------- orientation helpers (dataset.py:274-308)
    @property
    def tx_ori(self) -> np.ndarray:
        return self.ch_params["bs_antenna"]["rotation"] * np.pi / 180

    @property
    def bs_ori(self) -> np.ndarray:
        return self.tx_ori

    @property
    def rx_ori(self) -> np.ndarray:
        return self.ch_params["ue_antenna"]["rotation"] * np.pi / 180

    @property
    def ue_ori(self) -> np.ndarray:
        return self.rx_ori

    _computed_attributes = {
        c.N_UE_PARAM_NAME: "_compute_n_ue",
        c.NUM_PATHS_PARAM_NAME: "_compute_num_paths",
        c.DIST_PARAM_NAME: "_compute_distances",
        c.PATHLOSS_PARAM_NAME: "compute_pathloss",
        c.CHANNEL_PARAM_NAME: "compute_channels",
        c.LOS_PARAM_NAME: "_compute_los",
        c.CH_PARAMS_PARAM_NAME: "set_channel_params",
        c.PWR_LINEAR_PARAM_NAME: "_compute_power_linear",
        c.AOA_AZ_ROT_PARAM_NAME: "_compute_rotated_angles",
        c.AOA_EL_ROT_PARAM_NAME: "_compute_rotated_angles",
        c.AOD_AZ_ROT_PARAM_NAME: "_compute_rotated_angles",
        c.AOD_EL_ROT_PARAM_NAME: "_compute_rotated_angles",
        "fov": "_compute_fov",
        c.FOV_MASK_PARAM_NAME: "_compute_fov",
        c.AOA_AZ_FOV_PARAM_NAME: "_compute_fov",
        c.AOA_EL_FOV_PARAM_NAME: "_compute_fov",
        c.AOD_AZ_FOV_PARAM_NAME: "_compute_fov",
        c.AOD_EL_FOV_PARAM_NAME: "_compute_fov",
        c.PWR_LINEAR_ANT_GAIN_PARAM_NAME: "_compute_power_linear_ant_gain",
        c.NUM_INTERACTIONS_PARAM_NAME: "_compute_num_interactions",
        "grid_size": "_compute_grid_info",
        "grid_spacing": "_compute_grid_info",
        c.INTER_STR_PARAM_NAME: "_compute_inter_str",
        c.INTER_INT_PARAM_NAME: "_compute_inter_int",
        "array_response_product": "_compute_array_response_product",       # dataset.py:849
    }


class MacroDataset:
    """List of Datasets (one per TX / RX-set pair); attribute access and method calls fan out to
    every child, a single child returns its value unwrapped (dataset.py:888-998).  Methods of its own: `compute_cell_rate`
    reads all children in one launch, `compute_serving_beam` sweeps every child and picks a cell per user, `at_times`, `with_rx_combiner` and `with_tx_precoder` return a MacroDataset of the children's views."""

    SINGLE_ACCESS_METHODS = {"info"}
    PROPAGATE_METHODS = {name for name, _ in inspect.getmembers(Dataset, predicate=inspect.isfunction)
                         if not name.startswith("__")}

    def __init__(self, datasets=None):
        self.datasets = datasets if datasets is not None else []

    def _get_single(self, key):
        if not self.datasets:
            raise IndexError("MacroDataset is empty")
        return self.datasets[0][key]

    def __getattr__(self, name):
        if name in ("datasets",) or name.startswith("__"):
            raise AttributeError(name)
        if name in self.PROPAGATE_METHODS:
            if name in self.SINGLE_ACCESS_METHODS:
                return lambda *a, **k: getattr(self.datasets[0], name)(*a, **k)

            def fan_out(*a, **k):
                res = [getattr(d, name)(*a, **k) for d in self.datasets]
                return res[0] if len(res) == 1 else res
            return fan_out
        if name in SHARED_PARAMS:
            return self._get_single(name)
        res = [getattr(d, name) for d in self.datasets]
        return res[0] if len(res) == 1 else res

    def compute_cell_rate(self, params=None, *, snr_db=None, serving=None, per_subcarrier: bool = False,
                          details: bool = False, serving_set=None):
        """Per-user downlink rate in bit/s/Hz under inter-cell interference, every child one base station over the same
        users, with no channel tensor written for any of them (extension):

            rho_b = 10 ** (snr_db_b / 10) / M_tx_b      # snr_db: total transmit power over noise power per subcarrier
            N_k   = I + sum(rho_b * H_b[u, :, :, k] @ H_b[u, :, :, k].conj().T for b != s)     # s = serving[u]
            rate_k[u, k] = log2 det(N_k + rho_s * H_s[u, :, :, k] @ H_s[u, :, :, k].conj().T) - log2 det(N_k)
            rate[u]      = rate_k[u].mean()

        ``params``: one ``ChannelGenParameters`` for all children, or a list with one per child (the BS array may differ;
        the UE array and the subcarrier selection may not).  ``snr_db`` (required, keyword-only): a scalar, or one value per
        child.  ``serving``: ``None`` - each user is served by the child of largest ``link_snr`` (the first on ties) - an int
        for all users, or an int array [n_ue]; a value outside ``0 .. len(self) - 1`` means not served, rate 0.

        Returns ``rate`` float32 [n_ue]; with ``per_subcarrier`` also ``rate_k`` float32 [n_ue, K]; with ``details`` also
        ``serving`` (int32 [n_ue], -1 = not served) and ``link_snr`` (float32 [n_ue, B], linear: snr_b times the summed power
        of the child's kept paths, an RSRP-like quantity), in that order: NumPy arrays by default, the HBM-resident torch
        tensors when ``config('channel_output') == 'torch'``.  One child gives ``Dataset.compute_rate``.  At most 8
        children with equal ``n_ue``, each within the limits of ``compute_rate`` with the Gram over the UE array (at most 8
        elements; include/deepmimo_amd.h has the rule): anything else raises ValueError before any GPU work.  Not cached.

        ``serving_set`` (in place of ``serving``): joint transmission - a user served by a cluster of children at once
        (multi-TRP, CoMP, cell-free), each child an independent stream, equal power per antenna, no channel knowledge at
        the transmitters.  ``"all"``: every child serves every user, the full-cooperation bound; or a bool or integer
        array or tensor [n_ue, B], non-zero meaning member (``dm.serving_clusters`` builds one from ``link_snr``).  With
        S_u the set of user u the sum over ``b != s`` above runs over the children outside S_u, the serving term over
        those inside; a user with an empty set, or whose set reaches it on no path, gets 0.  A set of one child gives the
        bits of ``serving`` with that index.  With ``details`` the third result is the set as read, bool [n_ue, B], in
        place of the index.  Giving both ``serving`` and ``serving_set``, or a ``serving_set`` of another shape, dtype or
        string, raises ValueError before any GPU work."""
        from .engine import check_cell_rate_call, check_serving_set
        B = len(self.datasets)
        Dataset._required_snr("compute_cell_rate", snr_db, scalar=False)      # one per link: check_cell_rate_call's
        if not 1 <= B <= 8:
            raise ValueError(f"compute_cell_rate: {B} children, the call takes 1..8 base stations")
        n_ue = int(self.datasets[0].n_ue)
        if any(int(d.n_ue) != n_ue for d in self.datasets):
            raise ValueError("compute_cell_rate: the children must cover the same users (equal n_ue), got "
                             f"{[int(d.n_ue) for d in self.datasets]}")
        plist = list(params) if isinstance(params, (list, tuple)) else [params] * B
        if len(plist) != B:
            raise ValueError(f"compute_cell_rate: {len(plist)} parameter sets for {B} children")
        if serving is not None and not (isinstance(serving, (int, np.integer)) and not isinstance(serving, bool)):
            serving = np.asarray(serving)
            if serving.dtype.kind not in "iu" or serving.shape != (n_ue,):
                raise ValueError(f"compute_cell_rate: serving must be None, an int or an int array of shape ({n_ue},)")
        serving_set = check_serving_set("compute_cell_rate", serving_set, n_ue, B, serving)
        plist = [d._call_params(prm) for d, prm in zip(self.datasets, plist)]
        check_cell_rate_call(plist, [d._loaded_paths() for d in self.datasets], snr_db)
        np.random.seed(1001)
        runs = [d._run_prep(want_side="light") for d in self.datasets]
        res = runs[0][0].cell_rate([prep for _, prep in runs], snr_db, serving=serving, per_subcarrier=per_subcarrier,
                                   details=details, serving_set=serving_set)
        return Dataset._deliver(res)

    def compute_serving_beam(self, codebook, params=None, metric: str = "power"):
        """Serving cell and beam of every user from a beam sweep of every child - cell selection on RSRP - every child one
        cell over the same users (extension).  Each child runs ``compute_beam_power(codebook, params, metric=metric)``; a
        cell's value for a user is that of its best beam, and the user is served by the cell of largest value, the first on
        ties, among the cells that have a path to it.

        ``codebook``: one array [n_beams, M_tx] for all children, or a list or tuple with one per child (the BS arrays and
        the beam counts may differ); ``params`` alike.  Returns a DotDict: ``dbm_by_cell`` float64 [n_ue, n_cells], NaN where
        the cell has no path to the user; ``beam_by_cell`` int32 [n_ue, n_cells], -1 alike; ``serving`` int32 [n_ue], -1
        where no cell has a path - it goes as it is into ``compute_cell_rate(serving=...)``; ``beam`` int32 [n_ue] and
        ``dbm`` float64 [n_ue], the serving cell's beam and value, -1 and NaN alike.  Children of unequal ``n_ue``, a list of
        another length than the children or a ``metric`` other than "amplitude" / "power" raise ValueError before any GPU
        work."""
        from .engine import check_beam_metric, select_serving_beam
        who = "compute_serving_beam"
        check_beam_metric(who, metric)
        n_cells = len(self.datasets)
        if n_cells < 1:
            raise ValueError(f"{who}: the MacroDataset is empty")
        n_ue = int(self.datasets[0].n_ue)
        if any(int(d.n_ue) != n_ue for d in self.datasets):
            raise ValueError(f"{who}: the children must cover the same users (equal n_ue), got "
                             f"{[int(d.n_ue) for d in self.datasets]}")
        cbs = list(codebook) if isinstance(codebook, (list, tuple)) else [codebook] * n_cells
        plist = list(params) if isinstance(params, (list, tuple)) else [params] * n_cells
        if len(cbs) != n_cells or len(plist) != n_cells:
            raise ValueError(f"{who}: {len(cbs)} codebooks and {len(plist)} parameter sets for {n_cells} children")
        dbm_by_cell = np.full((n_ue, n_cells), np.nan)
        beam_by_cell = np.full((n_ue, n_cells), -1, np.int32)
        rows = np.arange(n_ue)
        for i, (d, cb, prm) in enumerate(zip(self.datasets, cbs, plist)):
            pwr, best = d.compute_beam_power(cb, prm, return_best=True, metric=metric)
            has = ~np.isnan(best)
            beam_by_cell[has, i] = best[has].astype(np.int32)
            dbm_by_cell[has, i] = pwr[rows[has], beam_by_cell[has, i]]
        serving, beam, dbm = select_serving_beam(dbm_by_cell, beam_by_cell)
        return DotDict({"dbm_by_cell": dbm_by_cell, "beam_by_cell": beam_by_cell, "serving": serving, "beam": beam, "dbm": dbm})

    def at_times(self, times, carrier_freq=None) -> "MacroDataset":
        """A MacroDataset of the children's ``Dataset.at_times(times, carrier_freq)`` views - T * n_ue users each, time-major
        - so ``compute_cell_rate`` runs over time (extension).  ``split_times`` gives its results as [T, n_ue, ...]."""
        return MacroDataset([d.at_times(times, carrier_freq) for d in self.datasets])

    def near_field(self, carrier_freq=None) -> "MacroDataset":
        """A MacroDataset of the children's ``Dataset.near_field(carrier_freq)`` views, so ``compute_cell_rate`` runs with
        spherical wavefronts (extension).  A MacroDataset built from views and plain children mixes the two per link."""
        return MacroDataset([d.near_field(carrier_freq) for d in self.datasets])

    def split_times(self, x):
        """``Dataset.split_times`` of the first child: the children of a view share the times and the users."""
        if not self.datasets:
            raise IndexError("MacroDataset is empty")
        return self.datasets[0].split_times(x)

    def with_rx_combiner(self, codebook="dft", params=None) -> "MacroDataset":
        """A MacroDataset of the children's ``Dataset.with_rx_combiner(codebook, params)`` views - Q * n_ue single-antenna
        users each, combiner-major - so ``compute_cell_rate`` runs per UE beam (extension).  ``params``: one
        ``ChannelGenParameters`` for all children, or a list with one per child.  ``split_rx_beams`` gives its results as
        [Q, n_ue, ...]."""
        plist = list(params) if isinstance(params, (list, tuple)) else [params] * len(self.datasets)
        if len(plist) != len(self.datasets):
            raise ValueError(f"with_rx_combiner: {len(plist)} parameter sets for {len(self.datasets)} children")
        return MacroDataset([d.with_rx_combiner(codebook, prm) for d, prm in zip(self.datasets, plist)])

    def split_rx_beams(self, x):
        """``Dataset.split_rx_beams`` of the first child: the children of a view share the UE beams and the users."""
        if not self.datasets:
            raise IndexError("MacroDataset is empty")
        return self.datasets[0].split_rx_beams(x)

    def with_tx_precoder(self, codebook="dft", beams=None, params=None) -> "MacroDataset":
        """A MacroDataset of the children's ``Dataset.with_tx_precoder(codebook, beams, params)`` views, so
        ``compute_cell_rate`` runs per BS beam (extension).  ``codebook``, ``beams`` and ``params``: one for all children, or a
        list or tuple with one per child (the BS arrays may differ).  ``split_tx_beams`` gives its results as
        [n_tx_beams, n_ue, ...]."""
        n = len(self.datasets)
        if isinstance(beams, (list, tuple)) and beams and isinstance(beams[0], (int, np.integer)):
            beams = np.asarray(beams)                                          # a plain list of beam indices: one for all
        per_child = [list(v) if isinstance(v, (list, tuple)) else [v] * n for v in (codebook, beams, params)]
        if any(len(v) != n for v in per_child):
            raise ValueError(f"with_tx_precoder: {[len(v) for v in per_child]} codebooks, beams and parameter sets for {n} children")
        return MacroDataset([d.with_tx_precoder(cb, bm, prm) for d, cb, bm, prm in zip(self.datasets, *per_child)])

    def split_tx_beams(self, x):
        """``Dataset.split_tx_beams`` of the first child: the children of a view share the BS beams and the users."""
        if not self.datasets:
            raise IndexError("MacroDataset is empty")
        return self.datasets[0].split_tx_beams(x)

    def __getitem__(self, idx):
        if isinstance(idx, (int, slice)):
            return self.datasets[idx]
        if idx in SHARED_PARAMS:
            return self._get_single(idx)
        res = [d[idx] for d in self.datasets]
        return res[0] if len(res) == 1 else res

    def __setitem__(self, key, value):
        for d in self.datasets:
            d[key] = value

    def __len__(self):
        return len(self.datasets)

    def append(self, dataset):
        self.datasets.append(dataset)
