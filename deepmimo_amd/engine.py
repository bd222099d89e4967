"""Host driver of the MI355X channel-generation kernels.

``ChannelEngine`` owns nothing but a device index: it takes the float32 ray matrices a
``Dataset`` holds (core.py:209-219 layout), keeps them as PyTorch-ROCm tensors (PyTorch is the
allocator / stream provider, not the compute path), fills the C structs of
include/deepmimo_amd.h and calls the C-ABI:

    dmx_channels_fd_direct -> complex64 [N, M_rx, M_tx, K] straight from the rays (small outputs, one launch)
    dmx_path_prep   -> per-path records + side products (LoS, path counts, FoV mask, angles, powers)
    dmx_channels_fd -> complex64 [N, M_rx, M_tx, K]     (dmx_channels_fd_lpf when rx_filter = 1)
    dmx_channels_td -> complex64 [N, M_rx, M_tx, P]
    dmx_channel_covariance -> complex64 [N, M, M]       (per-user spatial covariance, no channel tensor)
    dmx_channel_rate     -> float32 [N] (and [N, K])    (per-user achievable rate, no channel tensor)
    dmx_channel_spectrum -> float32 [N, K, m], [N], [N, K]  (eigenmode SNRs and water-filling rate, no channel tensor)
    dmx_channel_precoders -> float32 [N, K, m], complex64 [N, K, L, M_tx], [N, K, L, M_rx]  (eigenbeams, no channel tensor)
    dmx_cell_rate        -> float32 [N] (and [N, K], int32 [N], float32 [N, B])  (rate under inter-cell interference, B links)
    dmx_channels_angle_delay -> complex64 [N, M_rx, R, n_taps]  (codebook x inverse DFT, first delay taps, no channel tensor)
                                float32 [N, R, n_taps] / [N, n_taps] with output="power" / "profile" (sum over rx of |.|^2, and over rows)
    dmx_codebook_rate   -> float32 [N], int32 [N], float32 [N, C]  (rate and PMI over a precoding codebook, no channel tensor)
    dmx_codebook_rate_subbands -> the same and float32 [N, n_sb], int32 [N, n_sb], float32 [N, n_sb, C]  (a PMI per subband)

It replaces the body of Dataset.compute_channels (deepmimo/generator/dataset.py:224-268).
No CPU path exists here: without the shared library or without a GPU every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as nat
from . import consts as c


def _require_gpu(device_index: int) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("deepmimo_amd: no GPU visible (torch.cuda.is_available() is False); the channel-"
                           "generation path has no CPU fallback.")
    return torch.device("cuda", int(device_index))


@dataclass
class DeviceRays:
    """Ray matrices resident in HBM (float32 [N, L] each, contiguous)."""
    n_ue: int
    n_paths: int
    fields: Dict[str, torch.Tensor]
    doppler_vel: Optional[torch.Tensor] = None
    doppler_acc: Optional[torch.Tensor] = None


@dataclass
class PrepResult:
    workspace: torch.Tensor
    n_ue: int
    n_paths_loaded: int
    params_struct: nat.DmxParams
    keepalive: list = field(default_factory=list)
    side: Dict[str, torch.Tensor] = field(default_factory=dict)
    rays_struct: Optional[nat.DmxRays] = None
    side_struct: Optional[nat.DmxSide] = None
    workspace_bytes: int = 0
    sc_abs_max: int = 0            # largest |selected subcarrier index| (check_selection)


def is_full_fov(fov) -> bool:
    """dataset.py:450-459"""
    return fov[0] >= 360 and fov[1] >= 180


def uniform_stride(sel: np.ndarray):
    """(first, stride) when sel[k] == first + k * stride with stride > 0 for every k (dmx_params.sc_stride: lets the
    library pick the folded kernel without reading the device copy back), else (0, 0)."""
    sel = np.asarray(sel).astype(np.int64).ravel()
    if sel.size == 0 or abs(int(sel[0])) >= 2 ** 30:
        return 0, 0
    if sel.size == 1:
        return int(sel[0]), 1
    d = int(sel[1] - sel[0])
    if d <= 0 or d >= 2 ** 20 or int(sel[0]) + d * (sel.size - 1) >= 2 ** 31 or \
            not np.array_equal(sel, sel[0] + d * np.arange(sel.size)):
        return 0, 0
    return int(sel[0]), d


# include/deepmimo_amd.h DMX_SC_ABS_MAX_F32: the matrix-core and folded kernels reduce the subcarrier phase in float32,
# with an error that grows with |k|; from this |k| on only the float64-phase kernels (1 vector, 9 small-output) run
SC_ABS_MAX_F32 = 32768
F64_PHASE_VARIANTS = (1, 9)


def check_selection(sel):
    """(int64 copy of ofdm.selected_subcarriers, its largest |index|).  The device array is int32: an index outside
    int32 raises ValueError here instead of wrapping on upload."""
    sel = np.asarray(sel).astype(np.int64).ravel()
    if sel.size == 0:
        return sel, 0
    lo, hi = int(sel.min()), int(sel.max())
    if lo < -2 ** 31 or hi >= 2 ** 31:
        raise ValueError(f"selected_subcarriers holds {lo if lo < -2 ** 31 else hi}: subcarrier indices must fit int32")
    return sel, max(-lo, hi)


# Single pass against the two calls: tools/direct_bench.py --sweep --paths L on an MI355X (200k users, average ms of 50
# launches, routes alternating in one process; the same route differs by <= 0.005 ms between two passes, 0.02 at the
# largest shape), at L = 10, 16, 25 and 40 loaded paths (num_paths = 25), shapes where variant 0 runs the small-output
# kernel; profiles/r5_direct_sweep*.jsonl.  Speed-up two calls / single pass per class of table rows M_rx + M_tx:
#   rows (BS / UE)                 K    L=10          L=16          L=25          L=40
#   2..17  (1x1, 8x1, 4x4 / 1x1)   1,2  0.95-1.01     1.02-1.14     1.08-1.18     1.45-1.58
#   33, 34 (8x4 / 1x1, 2x1)        1-4  1.02-1.16     1.09-1.22     1.04-1.20     1.33-1.48
#   65, 66 (8x8 / 1x1, 2x1)        1,2  1.00-1.04     0.96-1.05     0.88-1.11     1.09-1.28
#                                  4    1.07-1.15     0.99-1.15     1.12-1.14     1.30-1.31
#   68     (8x8 / 2x2)             1,2  1.05          0.80-0.83     1.00-1.02     1.14-1.18
#                                  4,8  1.21-1.22     0.95-1.10     1.16-1.24     1.32-1.34
# The default call (8x1 / 1x1, K = 1): 0.222 | 0.223 ms at L = 10, 0.270 | 0.242 at 16, 0.314 | 0.271 at 25, 0.533 | 0.342
# at 40.  The gain is the record round trip (it grows with the path count); the cost is that up to 32 loaded paths stage 1
# packs two users into a wave and the fused kernel cannot, and that large tables leave the fused kernel's stage-1 part
# fewer waves per SIMD than it has in a launch of its own.  The automatic choice keeps a class only where every
# measured point of it is faster by more than the spread; everything else, and everything not measured (fewer than 10
# loaded paths, more than 68 table rows, more than 8 subcarriers, K > 2 on the smallest panels), stays on the two calls.
def single_pass_preferred(table_rows: int, loaded_paths: int, n_selected: int) -> bool:
    """The measured crossover above: table_rows = M_rx + M_tx, loaded_paths = columns of the ray matrices."""
    rows, L, K = int(table_rows), int(loaded_paths), int(n_selected)
    if rows > 68 or K > 8 or L < 10:
        return False
    if L >= 33:                       # stage 1 runs one user per wave there too (measured at 40)
        return True
    if rows <= 17:
        return L >= 16 and K <= 2
    if rows <= 34:
        return K <= 4
    return L >= 25 and K >= 4


def single_pass_route(single_pass, fd_kernel_variant, adaptive_precision, direct_supported, auto_choice, one_piece,
                      preferred=True, spatial_wideband=False, near_field=False) -> bool:
    """Whether ``Dataset.compute_channels`` takes the single-pass kernel (dmx_channels_fd_direct) instead of stage 1 +
    stage 2.  All of: ``config('single_pass')`` is not False; the kernel variant is the automatic one (0) and adaptive
    precision is off; the library takes the shape (dmx_fd_direct_supported == 1); variant 0 would run the small-output
    kernel there (dmx_fd_kernel_choice == 9), so the arithmetic - and every output bit - is the one the two calls give;
    the tensor leaves in one piece (resident, or a host copy `channels_to_host` would not chunk); and, for 'auto', the
    shape is on the winning side of the measured crossover (`single_pass_preferred`).  ``single_pass = True`` takes the
    route wherever it is possible, whatever the crossover says.  Never with ``spatial_wideband`` or ``near_field``: the
    single-pass kernel has no per-subcarrier array response and builds plane-wave tables only."""
    if spatial_wideband or near_field or single_pass is False or single_pass is None or single_pass in (0, "off", "false", "False"):
        return False
    if int(fd_kernel_variant) != 0 or bool(adaptive_precision):
        return False
    if not (bool(direct_supported) and int(auto_choice) == 9 and bool(one_piece)):
        return False
    return True if single_pass is True else bool(preferred)


def bounded_fd_variant(variant: int, sc_abs_max: int, small_preferred: bool) -> int:
    """The stage-2 variant to run under the float32-phase index bound: unchanged below SC_ABS_MAX_F32; from it on
    variant 0 becomes 9 where the small-output kernel is preferred and 1 elsewhere, 1 and 9 stay, and an explicit
    matrix-core or folded variant raises ValueError."""
    if sc_abs_max < SC_ABS_MAX_F32 or variant in F64_PHASE_VARIANTS:
        return variant
    if variant == 0:
        return 9 if small_preferred else 1
    raise ValueError(f"fd_kernel_variant {variant} evaluates subcarrier phases in float32 and needs every selected |index| "
                     f"below {SC_ABS_MAX_F32} (DMX_SC_ABS_MAX_F32); the selection reaches {sc_abs_max}: use variant 0, 1 "
                     f"or 9")


def check_beam_bound(sc_abs_max: int):
    """The beam entry points run the float32-phase kernels only: ValueError from SC_ABS_MAX_F32 on."""
    if sc_abs_max >= SC_ABS_MAX_F32:
        raise ValueError(f"beam-space channels / beam power need every selected subcarrier |index| below {SC_ABS_MAX_F32} "
                         f"(DMX_SC_ABS_MAX_F32); the selection reaches {sc_abs_max}")


BEAM_METRICS = ("amplitude", "power")


def check_beam_metric(who: str, metric) -> bool:
    """The `metric` of a beam sweep: False for "amplitude" (mean |F H|, the notebook's), True for "power" (mean |F H|^2,
    RSRP: DMX_FLAG_BEAM_MEAN_POWER); ValueError for anything else."""
    if not isinstance(metric, str) or metric not in BEAM_METRICS:
        raise ValueError(f"{who}: metric must be 'amplitude' or 'power', got {metric!r}")
    return metric == "power"


RECEIVERS = ("joint", "mmse")


def check_receiver(who: str, receiver) -> bool:
    """The `receiver` of a codebook-rate call: False for "joint" (log2 det: maximum likelihood, or MMSE with successive
    cancellation), True for "mmse" (the per-layer SINR of a linear MMSE receiver: DMX_FLAG_RX_LINEAR_MMSE); ValueError for
    anything else."""
    if not isinstance(receiver, str) or receiver not in RECEIVERS:
        raise ValueError(f"{who}: receiver must be 'joint' or 'mmse', got {receiver!r}")
    return receiver == "mmse"


ANGLE_DELAY_OUTPUTS = ("complex", "power", "profile")


def check_angle_delay_output(who: str, output) -> int:
    """The `output` of an angle-delay call as the flag bits of the call: 0 for "complex" (X itself), DMX_FLAG_ANGLE_DELAY_POWER
    for "power" (sum over rx of |X|^2), that | DMX_FLAG_ANGLE_DELAY_PROFILE for "profile" (summed over the rows as well);
    ValueError for anything else."""
    if not isinstance(output, str) or output not in ANGLE_DELAY_OUTPUTS:
        raise ValueError(f"{who}: output must be 'complex', 'power' or 'profile', got {output!r}")
    return {"complex": 0, "power": nat.FLAG_ANGLE_DELAY_POWER,
            "profile": nat.FLAG_ANGLE_DELAY_POWER | nat.FLAG_ANGLE_DELAY_PROFILE}[output]


def select_serving_beam(dbm_by_cell, beam_by_cell):
    """Serving cell and beam of every user from the per-cell best-beam values (pure NumPy): `dbm_by_cell` float [n_ue, n_cells],
    NaN where the cell has no path to the user, `beam_by_cell` that beam's index.  Returns (serving int32 [n_ue]: the first
    maximum over the cells that have a path, -1 where none has; beam int32 [n_ue]: the serving cell's beam, -1 alike;
    dbm float64 [n_ue]: its value, NaN alike)."""
    dbm_by_cell = np.asarray(dbm_by_cell, dtype=np.float64)
    beam_by_cell = np.asarray(beam_by_cell)
    if dbm_by_cell.ndim != 2 or beam_by_cell.shape != dbm_by_cell.shape:
        raise ValueError(f"select_serving_beam: dbm_by_cell and beam_by_cell must be [n_ue, n_cells] alike, got "
                         f"{dbm_by_cell.shape} and {beam_by_cell.shape}")
    n_ue, n_cells = dbm_by_cell.shape
    none = np.isnan(dbm_by_cell).all(axis=1) if n_cells else np.ones(n_ue, bool)
    serving = np.full(n_ue, -1, np.int32)
    beam = np.full(n_ue, -1, np.int32)
    dbm = np.full(n_ue, np.nan)
    if n_cells:
        # first maximum; a NaN cell never wins, not even against a cell whose power underflowed to 0 (-inf dBm)
        key = np.maximum(dbm_by_cell, np.finfo(np.float64).min)
        key[np.isnan(dbm_by_cell)] = -np.inf
        arg = np.argmax(key, axis=1)
        rows = np.arange(n_ue)
        serving[~none] = arg[~none]
        beam[~none] = beam_by_cell[rows, arg][~none]
        dbm[~none] = dbm_by_cell[rows, arg][~none]
    return serving, beam, dbm


WIDEBAND_VARIANTS = (0, 1)


def check_wideband_call(params, carrier_freq, fd_kernel_variant=0) -> float:
    """Everything a spatial-wideband channel call (DMX_FLAG_SPATIAL_WIDEBAND, include/deepmimo_amd.h) can refuse without a
    GPU, as ValueError: time domain, rx_filter = 1, a carrier frequency that is missing or not finite and > 0, a bandwidth
    that is not finite and > 0, and a kernel variant other than 0 or 1 (only the fp32 vector kernel forms a per-subcarrier
    array response).  `params`: validated ChannelGenParameters.  Returns the carrier frequency in Hz."""
    ofdm = params[c.PARAMSET_OFDM]
    if not params[c.PARAMSET_FD_CH]:
        raise ValueError("spatial_wideband: needs the frequency-domain channel (freq_domain = 1)")
    if ofdm[c.PARAMSET_OFDM_LPF]:
        raise ValueError("spatial_wideband: ofdm.rx_filter = 1 is not covered")
    try:
        fc = float(carrier_freq)
    except (TypeError, ValueError):
        fc = float("nan")
    if not (math.isfinite(fc) and fc > 0):
        raise ValueError("spatial_wideband: no carrier frequency: pass carrier_freq (Hz, finite and > 0) or set rt_params.frequency")
    bw = float(ofdm[c.PARAMSET_OFDM_BANDWIDTH])
    if not (math.isfinite(bw) and bw > 0):
        raise ValueError(f"spatial_wideband: ofdm.bandwidth must be finite and > 0, got {bw!r}")
    if int(fd_kernel_variant) not in WIDEBAND_VARIANTS:
        raise ValueError(f"spatial_wideband: fd_kernel_variant {int(fd_kernel_variant)} is refused, only the fp32 vector kernel "
                         f"(variant 0 or 1) forms a per-subcarrier array response")
    return fc


NEAR_FIELD_VARIANTS = (0, 1)


def check_near_field_call(params, carrier_freq, fd_kernel_variant=None, spatial_wideband=False) -> float:
    """Everything a call on a near-field view (DMX_FLAG_NEAR_FIELD, include/deepmimo_amd.h) can refuse without a GPU, as
    ValueError: time domain, rx_filter = 1, ``spatial_wideband`` on top, a carrier frequency that is missing or not finite
    and > 0, a bandwidth that is not finite and > 0 and, for a channel call (`fd_kernel_variant` given), a kernel variant
    other than 0 or 1 (of the channel kernels only the fp32 vector kernel builds spherical-wavefront tables).  `params`:
    validated ChannelGenParameters.  Returns the carrier frequency in Hz."""
    ofdm = params[c.PARAMSET_OFDM]
    if not params[c.PARAMSET_FD_CH]:
        raise ValueError("near_field: needs the frequency-domain channel (freq_domain = 1)")
    if ofdm[c.PARAMSET_OFDM_LPF]:
        raise ValueError("near_field: ofdm.rx_filter = 1 is not covered")
    if spatial_wideband:
        raise ValueError("near_field: spatial_wideband=True is not covered on a near-field view")
    try:
        fc = float(carrier_freq)
    except (TypeError, ValueError):
        fc = float("nan")
    if not (math.isfinite(fc) and fc > 0):
        raise ValueError("near_field: no carrier frequency: pass carrier_freq (Hz, finite and > 0) or set rt_params.frequency")
    bw = float(ofdm[c.PARAMSET_OFDM_BANDWIDTH])
    if not (math.isfinite(bw) and bw > 0):
        raise ValueError(f"near_field: ofdm.bandwidth must be finite and > 0, got {bw!r}")
    if fd_kernel_variant is not None and int(fd_kernel_variant) not in NEAR_FIELD_VARIANTS:
        raise ValueError(f"near_field: fd_kernel_variant {int(fd_kernel_variant)} is refused, only the fp32 vector kernel "
                         f"(variant 0 or 1) builds spherical-wavefront array tables")
    return fc


def covariance_side(side) -> int:
    """DMX_COV_TX / DMX_COV_RX for "tx" / "rx"; anything else raises ValueError."""
    if not isinstance(side, str) or side not in nat.COV_SIDES:
        raise ValueError(f"covariance: side must be 'tx' (over the BS array) or 'rx' (over the UE array), got {side!r}")
    return nat.COV_SIDES[side]


def _ptr(t: Optional[torch.Tensor]):
    """The pointer argument of a tensor a C call reads or writes; None (NULL) for one that is not there."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _fill_shape_fields(p: nat.DmxParams, params, n_selected: int):
    """The fields of dmx_params that say how large a call is: all the host-only dmx_*_supported queries read."""
    bs, ue, ofdm = params[c.PARAMSET_ANT_BS], params[c.PARAMSET_ANT_UE], params[c.PARAMSET_OFDM]
    p.bs_shape[0], p.bs_shape[1] = int(bs[c.PARAMSET_ANT_SHAPE][0]), int(bs[c.PARAMSET_ANT_SHAPE][1])
    p.ue_shape[0], p.ue_shape[1] = int(ue[c.PARAMSET_ANT_SHAPE][0]), int(ue[c.PARAMSET_ANT_SHAPE][1])
    p.num_paths = int(params[c.PARAMSET_NUM_PATHS])
    p.freq_domain = int(bool(params[c.PARAMSET_FD_CH]))
    p.n_subcarriers = int(ofdm[c.PARAMSET_OFDM_SC_NUM])
    p.n_selected = int(n_selected)
    p.bandwidth = float(ofdm[c.PARAMSET_OFDM_BANDWIDTH])


def _query_params(who: str, params, needs: Optional[str] = None, promise_stride: bool = False):
    """(dmx_params of a host-only dmx_*_supported query, the int64 selection) for validated ChannelGenParameters.  Time
    domain and rx_filter are ValueErrors under `who` (`needs`: the head of the first where it is not "`who`: needs"), an index
    outside int32 is check_selection's.  `promise_stride`: sc_first / sc_stride from `uniform_stride` of the selection."""
    ofdm = params[c.PARAMSET_OFDM]
    if not params[c.PARAMSET_FD_CH]:
        raise ValueError(f"{needs or who + ': needs'} the frequency-domain channel (freq_domain = 1)")
    if ofdm[c.PARAMSET_OFDM_LPF]:
        raise ValueError(f"{who}: ofdm.rx_filter = 1 is not covered")
    sel, _ = check_selection(ofdm[c.PARAMSET_OFDM_SC_SAMP])
    p = nat.DmxParams()
    _fill_shape_fields(p, params, sel.size)
    if promise_stride:
        p.sc_first, p.sc_stride = uniform_stride(sel)
    p._host_sel = (C.c_int32 * max(1, int(sel.size)))()       # the query reads the count, never the array; lives with p
    p.selected_subcarriers = C.addressof(p._host_sel)
    return p, sel


def _ask(who: str, query: str, *args, refusal: str = "shape not supported: "):
    """Ask the library's host-only `query`; anything but "taken" is a ValueError with the library's message, which names
    the limit."""
    lib = nat.load()
    if getattr(lib, query)(*args) != 1:
        raise ValueError(f"{who}: {refusal}" + lib.dmx_last_error().decode("utf-8", "replace"))


def _int_arg(who: str, name: str, v) -> int:
    """`v` as a C int32 argument (clipped, so the library refuses what is out of range); no integer: ValueError."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {name} must be an integer, got {v!r}")
    return int(np.clip(v, -2 ** 31, 2 ** 31 - 1))


def check_covariance_call(params, n_paths_loaded: int, side) -> int:
    """Everything `Dataset.compute_covariance` can refuse without a GPU, as ValueError: the side, time domain, rx_filter,
    and a shape dmx_covariance_supported does not take (the message is the library's and names the limit).  `params`:
    validated ChannelGenParameters.  Returns the side id."""
    sid = covariance_side(side)
    p, _ = _query_params("covariance", params)
    _ask("covariance", "dmx_covariance_supported", C.byref(p), int(n_paths_loaded), sid)
    return sid


def snr_linear_from_db(snr_db) -> float:
    """10 ** (snr_db / 10) in float64; ValueError for anything that is not a finite real number."""
    if isinstance(snr_db, bool) or not isinstance(snr_db, (int, float, np.integer, np.floating)) or not math.isfinite(float(snr_db)):
        raise ValueError(f"rate: snr_db must be a finite number (dB), got {snr_db!r}")
    return 10.0 ** (float(snr_db) / 10.0)


def _check_rate_call(who: str, query: str, params, n_paths_loaded: int, snr_db) -> float:
    snr = snr_linear_from_db(snr_db)
    p, _ = _query_params(who, params)
    _ask(who, query, C.byref(p), int(n_paths_loaded))
    return snr


def check_rate_call(params, n_paths_loaded: int, snr_db) -> float:
    """Everything `Dataset.compute_rate` can refuse without a GPU, as ValueError: time domain, rx_filter, an snr_db that is
    not finite, and a shape dmx_rate_supported does not take (the message is the library's and names the limit).  `params`:
    validated ChannelGenParameters.  Returns the linear SNR."""
    return _check_rate_call("rate", "dmx_rate_supported", params, n_paths_loaded, snr_db)


def check_spectrum_call(params, n_paths_loaded: int, snr_db) -> float:
    """`check_rate_call` for `Dataset.compute_eigenmodes` and the water-filling rate: the same refusals (the spectrum call
    takes exactly the shapes of the rate), asked of dmx_spectrum_supported.  Returns the linear SNR."""
    return _check_rate_call("spectrum", "dmx_spectrum_supported", params, n_paths_loaded, snr_db)


def check_precoder_call(params, n_paths_loaded: int, snr_db, n_layers) -> float:
    """`check_spectrum_call` for `Dataset.compute_precoders`: the same refusals, and an `n_layers` that is not an integer
    in 1..min(M_rx, M_tx), asked of dmx_precoder_supported.  Returns the linear SNR."""
    snr = snr_linear_from_db(snr_db)
    n_layers = _int_arg("precoders", "n_layers", n_layers)
    p, _ = _query_params("precoders", params)
    _ask("precoders", "dmx_precoder_supported", C.byref(p), int(n_paths_loaded), n_layers)
    return snr


def check_angle_delay_call(params, n_paths_loaded: int, n_rows, n_fft, n_taps, output="complex") -> int:
    """Everything `Dataset.compute_angle_delay` can refuse without a GPU, as ValueError: an `output` that is none of
    "complex", "power", "profile", time domain, rx_filter, a selection that is not uniformly spaced, `n_rows` / `n_fft` /
    `n_taps` that are no integers, and a shape dmx_angle_delay_supported does not take (the message is the library's and
    names the limit; the query is asked with the output's flags).  `params`: validated ChannelGenParameters; `n_fft` None =
    the number of selected subcarriers.  Returns n_fft."""
    out_flags = check_angle_delay_output("angle-delay", output)
    p, sel = _query_params("angle-delay", params, promise_stride=True)
    p.flags |= out_flags
    if p.sc_stride <= 0:
        raise ValueError("angle-delay: ofdm.selected_subcarriers must be uniformly spaced, first + k * stride with 0 < stride < 2^20 "
                         "and |first| < 2^30 (the delay transform is an inverse DFT over the selection)")
    n_fft = int(sel.size) if n_fft is None else _int_arg("angle-delay", "n_fft", n_fft)
    _ask("angle-delay", "dmx_angle_delay_supported", C.byref(p), int(n_paths_loaded), _int_arg("angle-delay", "n_rows", n_rows),
         n_fft, _int_arg("angle-delay", "n_taps", n_taps))
    return n_fft


def check_codebook_rate_call(params, n_paths_loaded: int, n_codewords, n_layers, snr_db, receiver="joint") -> float:
    """Everything `Dataset.compute_codebook_rate` can refuse without a GPU, as ValueError: a `receiver` that is neither
    "joint" nor "mmse", an snr_db that is not finite, time domain, rx_filter, `n_codewords` / `n_layers` that are no
    integers, and a shape dmx_codebook_rate_supported does not take (the message is the library's and names the limit; the
    query is asked with the receiver's flag).  `params`: validated ChannelGenParameters.  Returns the linear SNR."""
    mmse = check_receiver("codebook rate", receiver)
    snr = snr_linear_from_db(snr_db)
    n_codewords, n_layers = _int_arg("codebook rate", "n_codewords", n_codewords), _int_arg("codebook rate", "n_layers", n_layers)
    p, _ = _query_params("codebook rate", params)
    p.flags |= nat.FLAG_RX_LINEAR_MMSE if mmse else 0
    _ask("codebook rate", "dmx_codebook_rate_supported", C.byref(p), int(n_paths_loaded), n_codewords, n_layers)
    return snr


def check_subband_size(subband_size) -> Optional[int]:
    """`subband_size` of the subband calls as an int, None (one subband over the whole selection) passed through; anything
    that is not an integer >= 1 is a ValueError."""
    if subband_size is None:
        return None
    if isinstance(subband_size, bool) or not isinstance(subband_size, (int, np.integer)) or subband_size < 1:
        raise ValueError(f"codebook rate: subband_size must be an integer >= 1 or None, got {subband_size!r}")
    return int(subband_size)


def link_snrs_from_db(snr_db, n_links: int):
    """Linear SNR per link from `snr_db`: a scalar for every link, or a sequence with one entry per link."""
    if isinstance(snr_db, (list, tuple, np.ndarray)):
        vals = list(np.asarray(snr_db, dtype=object).ravel()) if isinstance(snr_db, np.ndarray) else list(snr_db)
        if len(vals) != n_links:
            raise ValueError(f"cell rate: snr_db holds {len(vals)} values for {n_links} links (one per link, or a scalar)")
        return [snr_linear_from_db(v) for v in vals]
    return [snr_linear_from_db(snr_db)] * n_links


def check_serving_set(who: str, serving_set, n_ue: int, n_links: int, serving=None):
    """The `serving_set` of a cell-rate call (DMX_FLAG_SERVING_SET, include/deepmimo_amd.h), checked without a GPU: None (no
    sets: the call without the flag), "all" (every link serves every user) or a bool or integer array / tensor
    [n_ue, n_links], non-zero meaning that the link is a member of the user's set.  ValueError for anything else, and for
    `serving` given beside it.  Returns None, "all" or the array / tensor as given."""
    if serving_set is None:
        return None
    if serving is not None:
        raise ValueError(f"{who}: serving and serving_set are two forms of the same argument, give one of them")
    if isinstance(serving_set, str):
        if serving_set != "all":
            raise ValueError(f"{who}: serving_set must be None, 'all' or a bool or integer array of shape ({n_ue}, {n_links}), "
                             f"got {serving_set!r}")
        return "all"
    if hasattr(serving_set, "detach"):
        kind = "b" if str(serving_set.dtype) == "torch.bool" else "f" if serving_set.is_floating_point() or serving_set.is_complex() else "i"
        shape, dtype, t = tuple(serving_set.shape), serving_set.dtype, serving_set
    else:
        try:
            t = np.asarray(serving_set)
        except (TypeError, ValueError):
            t = np.empty(0, object)
        kind, shape, dtype = t.dtype.kind, t.shape, t.dtype
    if kind not in "biu" or shape != (n_ue, n_links):
        raise ValueError(f"{who}: serving_set must be None, 'all' or a bool or integer array of shape ({n_ue}, {n_links}), got "
                         f"{dtype} of shape {tuple(shape)}")
    return t


def serving_clusters(link_snr, max_size: int, within_db=None):
    """Serving sets from the links' wideband receive SNR: per user the strongest link and further links in descending
    `link_snr`, as a bool array [n_ue, B] for ``MacroDataset.compute_cell_rate(serving_set=...)``.  `link_snr`: [n_ue, B],
    linear, as ``compute_cell_rate(details=True)`` returns it - it does not depend on the subcarrier selection, so a call
    with one selected subcarrier is the cheap way to get it.  A user's set starts with its strongest link (the first on
    ties) and grows in descending link_snr (index order on ties) until it holds `max_size` links or the next link is more
    than `within_db` dB below the strongest (None: no such limit).  A link with link_snr == 0 - no kept path - is never a
    member, so a user no link reaches has the empty set.  Pure NumPy."""
    ls = np.asarray(link_snr.detach().cpu().numpy() if hasattr(link_snr, "detach") else link_snr, dtype=np.float64)
    if ls.ndim != 2 or not np.isfinite(ls).all() or (ls < 0).any():
        raise ValueError(f"serving_clusters: link_snr must be a finite, non-negative array [n_ue, B], got shape {ls.shape}")
    if isinstance(max_size, bool) or not isinstance(max_size, (int, np.integer)) or max_size < 1:
        raise ValueError(f"serving_clusters: max_size must be an integer >= 1, got {max_size!r}")
    if within_db is not None and not (np.isfinite(within_db) and within_db >= 0):
        raise ValueError(f"serving_clusters: within_db must be None or finite and >= 0, got {within_db!r}")
    n_ue, B = ls.shape
    order = np.argsort(-ls, axis=1, kind="stable")                       # descending, index order on ties
    ranked = np.take_along_axis(ls, order, axis=1)
    keep = (ranked > 0) & (np.arange(B)[None, :] < int(max_size))
    if within_db is not None:
        keep &= ranked >= ranked[:, :1] * 10.0 ** (-float(within_db) / 10.0)
    member = np.zeros((n_ue, B), bool)
    np.put_along_axis(member, order, keep, axis=1)
    return member


def check_cell_rate_call(params_list, n_paths_loaded_list, snr_db):
    """Everything `MacroDataset.compute_cell_rate` can refuse without a GPU, as ValueError: the link count, an snr_db that is
    not finite (or not one per link), time domain or rx_filter on a link, and links dmx_cell_rate_supported does not take
    together (the message is the library's and names the limit).  `params_list`: validated ChannelGenParameters, one per
    link; `n_paths_loaded_list`: loaded paths per link.  Returns the linear SNRs, one per link."""
    params_list, loaded = list(params_list), list(n_paths_loaded_list)
    B = len(params_list)
    if len(loaded) != B:
        raise ValueError(f"cell rate: {B} parameter sets for {len(loaded)} links")
    if not 1 <= B <= nat.MAX_LINKS:
        raise ValueError(f"cell rate: {B} links, the call takes 1..{nat.MAX_LINKS}")
    snrs = link_snrs_from_db(snr_db, B)
    links = (nat.DmxLink * B)()
    keep, first_sel = [], None
    for b, params in enumerate(params_list):
        p, sel = _query_params(f"cell rate: link {b}", params, needs=f"cell rate: link {b} needs")
        if b and not np.array_equal(sel, first_sel):
            raise ValueError(f"cell rate: link {b} selects other subcarriers than link 0; the links must share the selection")
        first_sel = sel if b == 0 else first_sel
        keep.append(p)
        links[b].prm = C.pointer(p)
        links[b].n_paths_loaded = int(loaded[b])
        links[b].snr_linear = snrs[b]
    _ask("cell rate", "dmx_cell_rate_supported", links, B, refusal="links not supported: ")
    return snrs


class ChannelEngine:
    def __init__(self, device_index: int = 0):
        self.lib = nat.load()
        self.device = _require_gpu(device_index)

    # ------------------------------------------------------------------ uploads
    def upload_rays(self, data) -> DeviceRays:
        """data: mapping with the eight float32 [N, L] matrices (numpy or torch)."""
        fields = {}
        shape = None
        for k in c.RAY_FIELDS:
            t = self._to_dev_f32(data[k])
            if t.dim() != 2:
                raise ValueError(f"ray matrix '{k}' must be 2-D [n_ue, n_paths], got {tuple(t.shape)}")
            if shape is None:
                shape = tuple(t.shape)
            elif tuple(t.shape) != shape:
                raise ValueError(f"ray matrix '{k}' has shape {tuple(t.shape)}, expected {shape}")
            fields[k] = t
        dv = da = None
        keys = data.keys() if hasattr(data, "keys") else ()
        if c.DOPPLER_VEL_PARAM_NAME in keys and c.DOPPLER_ACC_PARAM_NAME in keys:
            dv = self._to_dev_f32(data[c.DOPPLER_VEL_PARAM_NAME])
            da = self._to_dev_f32(data[c.DOPPLER_ACC_PARAM_NAME])
        return DeviceRays(n_ue=shape[0], n_paths=shape[1], fields=fields, doppler_vel=dv, doppler_acc=da)

    def _to_dev(self, v, dtype, np_dtype=None):
        """`v` (NumPy or torch) as a contiguous device tensor of `dtype`; `np_dtype`: convert a NumPy input on the host first."""
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np_dtype))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _to_dev_f32(self, v):
        return self._to_dev(v, torch.float32, np.float32)

    # ------------------------------------------------------------------ C structs
    def _params_struct(self, params, bs_fov, ue_fov, ue_rot_per_user: Optional[torch.Tensor],
                       sel_dev: Optional[torch.Tensor], carrier_freq: float, have_doppler: bool,
                       sc_hint=(0, 0)) -> nat.DmxParams:
        bs, ue, ofdm = params[c.PARAMSET_ANT_BS], params[c.PARAMSET_ANT_UE], params[c.PARAMSET_OFDM]
        p = nat.DmxParams()
        _fill_shape_fields(p, params, 0 if sel_dev is None else sel_dev.numel())
        p.bs_spacing, p.ue_spacing = float(bs[c.PARAMSET_ANT_SPACING]), float(ue[c.PARAMSET_ANT_SPACING])
        bs_rot = np.deg2rad(np.asarray(bs[c.PARAMSET_ANT_ROTATION]))          # geometry.py:286
        for i in range(3):
            p.bs_rotation[i] = float(bs_rot[i])
        if ue_rot_per_user is None:
            ue_rot = np.deg2rad(np.asarray(ue[c.PARAMSET_ANT_ROTATION]))
            for i in range(3):
                p.ue_rotation[i] = float(ue_rot[i])
            p.ue_rotation_per_user = None
        else:
            p.ue_rotation_per_user = ue_rot_per_user.data_ptr()
        for side, key in ((bs, "bs_pattern"), (ue, "ue_pattern")):
            name = side[c.PARAMSET_ANT_RAD_PAT]
            if name not in c.PARAMSET_ANT_RAD_PAT_VALS:                      # ant_patterns.py:119-120
                raise NotImplementedError(f"The given '{name}' antenna radiation pattern is not applicable.")
            setattr(p, key, nat.PATTERN_IDS[name])
        # FoV (dataset.py:477-504); apply_fov always stores both, a lone None is the full sphere
        if bs_fov is not None and ue_fov is None:
            ue_fov = np.array([360, 180])
        if ue_fov is not None and bs_fov is None:
            bs_fov = np.array([360, 180])
        bs_full = bs_fov is not None and is_full_fov(bs_fov)
        ue_full = ue_fov is not None and is_full_fov(ue_fov)
        enabled = not ((bs_fov is None and ue_fov is None) or (bs_full and ue_full))
        p.fov_enabled = int(enabled)
        if enabled:
            p.bs_fov_restricted, p.ue_fov_restricted = int(not bs_full), int(not ue_full)
            b, u = np.deg2rad(np.asarray(bs_fov)), np.deg2rad(np.asarray(ue_fov))   # geometry.py:184
            p.bs_fov[0], p.bs_fov[1], p.ue_fov[0], p.ue_fov[1] = float(b[0]), float(b[1]), float(u[0]), float(u[1])
        p.selected_subcarriers = None if sel_dev is None or sel_dev.numel() == 0 else sel_dev.data_ptr()
        p.rx_filter = int(bool(ofdm[c.PARAMSET_OFDM_LPF]))
        p.enable_doppler = int(bool(params[c.PARAMSET_DOPPLER_EN]) and have_doppler)
        p.carrier_freq = float(carrier_freq)
        p.sc_first, p.sc_stride = sc_hint
        return p

    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch(self, nbytes: int) -> torch.Tensor:
        """uint8 view of at least `nbytes` bytes (never empty) whose data_ptr() is 256-byte aligned, as every workspace of
        the C-ABI has to be.  It may go out of scope right after the call it serves: the launch is on torch's current
        stream and the caching allocator reuses freed blocks in stream order, so the kernels still own it when they run."""
        n = max(int(nbytes), 256)
        buf = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
        off = (-buf.data_ptr()) % 256
        return buf[off:off + n]

    def _outs(self, out, wanted, torch_names: bool = False):
        """The tensors a call writes: `wanted` is a list of (shape, dtype).  `out` None: new ones; else the tensor, or the
        tuple / list of tensors in the same order, to write into - each has to be the contiguous tensor of its shape and
        dtype.  `torch_names`: the message spells the dtype "torch.float32", not "float32"."""
        given = list(out) if isinstance(out, (tuple, list)) else [out] * (out is not None)
        if out is not None and len(given) != len(wanted):
            raise ValueError(f"out must hold {len(wanted)} tensors, one per requested output")
        res = []
        for i, (shape, dt) in enumerate(wanted):
            t = given[i] if given else torch.empty(shape, dtype=dt, device=self.device)
            if t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
                raise ValueError(f"out must be a contiguous {dt if torch_names else str(dt)[6:]} tensor of shape {shape}")
            res.append(t)
        return res

    def _out(self, out: Optional[torch.Tensor], shape) -> torch.Tensor:
        """`out` when it is the contiguous complex64 tensor of `shape` a kernel writes, a new one when it is None."""
        return self._outs(out, [(shape, torch.complex64)])[0]

    def _codebook(self, tx_codebook, m_tx: int, min_beams: int = 0) -> torch.Tensor:
        """[n_beams, M_tx] beamforming matrix as a contiguous complex64 device tensor."""
        cb = self._to_dev(tx_codebook, torch.complex64)
        if cb.dim() != 2 or cb.shape[1] != m_tx or cb.shape[0] < min_beams:
            raise ValueError(f"tx_codebook must be [n_beams, {m_tx}], got {tuple(cb.shape)}")
        return cb

    def _side_tensors(self, n: int, L: int, fov_enabled, want_side):
        """Side-product tensors and the dmx_side that points at them.  "light": what is cheap beside the channel
        generation - LoS, path counts, the FoV mask when a FoV is set (stage 1 then needs the angles as numbers anyway).
        True (stage 1 only): also the four rotated-angle matrices and the powers (float64 arccos / atan2 per path: ~1 ms
        per 100k users x 25 paths, 120 MB of stores).  The delay maximum always."""
        dev, side = self.device, {}
        if want_side:
            side["fov_mask"] = torch.empty((n, L), dtype=torch.uint8, device=dev) if fov_enabled else None
            side["num_paths"] = torch.empty((n,), dtype=torch.int32, device=dev)
            side["los"] = torch.empty((n,), dtype=torch.int32, device=dev)
        if want_side is True:
            for k in ("aod_el_rot", "aod_az_rot", "aoa_el_rot", "aoa_az_rot", "power_linear_ant_gain"):
                side[k] = torch.empty((n, L), dtype=torch.float64, device=dev)
            side["power_linear"] = torch.empty((n, L), dtype=torch.float32, device=dev)
        side["max_delay_key"] = torch.zeros((1,), dtype=torch.int32, device=dev)
        s = nat.DmxSide()
        for k, t in side.items():
            if t is not None and t.numel() > 0:
                setattr(s, k, t.data_ptr())
        return side, s

    def _call_structs(self, rays: DeviceRays, params, bs_fov=None, ue_fov=None, ue_rotation_per_user=None,
                      carrier_freq: float = 0.0, adaptive_terms: bool = False, spatial_wideband: bool = False,
                      near_field: bool = False):
        """The dmx_params / dmx_rays of a call on `rays` (shared by `prepare` and `channels_direct`): checks the
        selection, uploads it and the per-user rotation.  Returns (params struct, rays struct, tensors to keep alive,
        largest |selected index|).  spatial_wideband: DMX_FLAG_SPATIAL_WIDEBAND, after `check_wideband_call`; near_field:
        DMX_FLAG_NEAR_FIELD, after `check_near_field_call`."""
        if near_field:
            check_near_field_call(params, carrier_freq, spatial_wideband=spatial_wideband)
        if spatial_wideband:
            check_wideband_call(params, carrier_freq)
        dev = self.device
        n, L = rays.n_ue, rays.n_paths
        ofdm = params[c.PARAMSET_OFDM]
        keep = []
        sel, sc_abs_max = check_selection(ofdm[c.PARAMSET_OFDM_SC_SAMP])
        sel_dev = torch.from_numpy(sel.astype(np.int32)).to(dev)
        keep.append(sel_dev)
        rot_dev = None
        if ue_rotation_per_user is not None:
            r = ue_rotation_per_user
            r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64))
            rot_dev = r.to(device=dev, dtype=torch.float64).contiguous()
            if tuple(rot_dev.shape) != (n, 3):
                raise ValueError(f"per-user UE rotation must be [n_ue, 3], got {tuple(rot_dev.shape)}")
            keep.append(rot_dev)
        have_dop = rays.doppler_vel is not None and rays.doppler_acc is not None
        p = self._params_struct(params, bs_fov, ue_fov, rot_dev, sel_dev, carrier_freq, have_dop,
                                sc_hint=uniform_stride(sel))
        p.flags = ((nat.FLAG_ADAPTIVE_TERMS if adaptive_terms else 0) | (nat.FLAG_SPATIAL_WIDEBAND if spatial_wideband else 0) |
                   (nat.FLAG_NEAR_FIELD if near_field else 0))

        r = nat.DmxRays()
        r.n_ue, r.n_paths, r.ld = n, L, L
        for k in c.RAY_FIELDS:
            setattr(r, k, rays.fields[k].data_ptr() if n * L > 0 else None)
        r.doppler_vel = rays.doppler_vel.data_ptr() if have_dop and n * L > 0 else None
        r.doppler_acc = rays.doppler_acc.data_ptr() if have_dop and n * L > 0 else None
        return p, r, keep, sc_abs_max

    # ------------------------------------------------------------------ stage 1
    def prepare(self, rays: DeviceRays, params, bs_fov=None, ue_fov=None, ue_rotation_per_user=None,
                carrier_freq: float = 0.0, want_side=True, adaptive_terms: bool = False, structs=None,
                spatial_wideband: bool = False, near_field: bool = False) -> PrepResult:
        """Run dmx_path_prep.  ue_rotation_per_user: optional [N, 3] degrees (numpy/torch).  want_side: True = every
        side product, "light" = LoS / path counts / FoV mask only, False = none.  adaptive_terms: opt into
        DMX_FLAG_ADAPTIVE_TERMS (include/deepmimo_amd.h: weak last path groups in one product term); the flag travels in
        the parameter block of the preparation, so every stage-2 call on it runs in the same mode.  structs: what
        `_call_structs` returned for the same arguments, when the caller has built them already.  spatial_wideband: opt
        into DMX_FLAG_SPATIAL_WIDEBAND (the per-subcarrier array response; `carrier_freq` is then required): it travels in
        the parameter block too, the records are the same, and `channels` on the preparation runs the wideband body.
        near_field: opt into DMX_FLAG_NEAR_FIELD (spherical-wavefront array tables from the path delay; `carrier_freq` is
        required): it travels the same way, and every call on the preparation that takes the flag runs with it."""
        n, L = rays.n_ue, rays.n_paths
        p, r, keep, sc_abs_max = structs or self._call_structs(rays, params, bs_fov, ue_fov, ue_rotation_per_user,
                                                               carrier_freq, adaptive_terms, spatial_wideband, near_field)
        keep = list(keep)

        nbytes = int(self.lib.dmx_workspace_bytes(C.byref(p), n, L))
        ws = self._scratch(nbytes)
        side, s = self._side_tensors(n, L, p.fov_enabled, want_side)
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_path_prep(C.byref(r), C.byref(p), C.c_void_p(ws.data_ptr()), nbytes, C.byref(s),
                                        self._stream_ptr())
        nat.check(rc, "dmx_path_prep")
        keep.extend(rays.fields.values())
        return PrepResult(workspace=ws, n_ue=n, n_paths_loaded=L, params_struct=p, keepalive=keep, side=side,
                          rays_struct=r, side_struct=s, workspace_bytes=nbytes, sc_abs_max=sc_abs_max)

    def fd_variant(self, prep: PrepResult, variant: int = 0) -> int:
        """The variant stage 2 runs for `variant` (bounded_fd_variant).  Beyond the bound without a spacing promise the
        library cannot see the indices, so variant 0 is resolved here.  A spatial-wideband preparation runs the fp32 vector
        kernel for variant 0 and 1 at any index; the library refuses every other variant."""
        if prep.sc_abs_max < SC_ABS_MAX_F32 or prep.params_struct.flags & (nat.FLAG_SPATIAL_WIDEBAND | nat.FLAG_NEAR_FIELD):
            return variant
        return bounded_fd_variant(int(variant), prep.sc_abs_max, self._small_preferred(prep.params_struct, prep.n_paths_loaded))

    def _small_preferred(self, p: nat.DmxParams, n_paths_loaded: int) -> bool:
        """Whether variant 0 runs the small-output kernel (9) for the shape alone, the index range left out."""
        q = nat.DmxParams.from_buffer_copy(p)
        q.sc_first, q.sc_stride = 0, 0
        return self.lib.dmx_fd_kernel_choice(C.byref(q), n_paths_loaded) == 9

    def reprepare(self, prep: PrepResult) -> PrepResult:
        """Re-issue stage 1 of an existing preparation on the current stream, reading whatever the ray tensors hold
        NOW: the delay maximum is zeroed and dmx_path_prep writes the same workspace and side tensors again.  No
        allocation, no host-device copy, no synchronisation, so a HIP graph can capture it in front of any consumer of
        the records ("new rays -> records -> rate"; tests/test_gpu_graph_capture.py)."""
        with torch.cuda.device(self.device):
            prep.side["max_delay_key"].zero_()
            nat.check(self.lib.dmx_path_prep(C.byref(prep.rays_struct), C.byref(prep.params_struct),
                                             C.c_void_p(prep.workspace.data_ptr()), prep.workspace_bytes,
                                             C.byref(prep.side_struct), self._stream_ptr()), "dmx_path_prep")
        return prep

    def relaunch(self, prep: PrepResult, out: torch.Tensor, variant: int = 0) -> torch.Tensor:
        """Re-issue stage 1 (`reprepare`) + stage 2 of an existing preparation on the current stream, reading whatever
        the ray tensors hold NOW.  No allocation, no host-device copy, no synchronisation: the two C-ABI calls only
        enqueue kernels, so this is what a HIP graph captures (tests/test_gpu_parity.py::test_hip_graph_replay)
        and what a serving loop calls per batch.  Frequency domain without rx_filter, or time domain."""
        p = prep.params_struct
        if p.freq_domain and p.rx_filter:
            raise ValueError("relaunch does not cover rx_filter = 1 (it needs a gains table per call)")
        out = self._out(out, self.channel_shape(prep))
        if p.freq_domain:
            variant = self.fd_variant(prep, variant)
        wsp = C.c_void_p(prep.workspace.data_ptr())
        self.reprepare(prep)
        stream = self._stream_ptr()
        with torch.cuda.device(self.device):
            if out.numel():
                if p.freq_domain:
                    rc = self.lib.dmx_channels_fd(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, 0, prep.n_ue,
                                                  C.c_void_p(out.data_ptr()), int(variant), stream)
                else:
                    rc = self.lib.dmx_channels_td(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, 0, prep.n_ue,
                                                  C.c_void_p(out.data_ptr()), stream)
                nat.check(rc, "stage 2")
        return out

    # ------------------------------------------------------------------ stage 2
    def channel_shape(self, prep: PrepResult, user_count: Optional[int] = None):
        p = prep.params_struct
        n = prep.n_ue if user_count is None else user_count
        m_rx, m_tx = p.ue_shape[0] * p.ue_shape[1], p.bs_shape[0] * p.bs_shape[1]
        last = p.n_selected if p.freq_domain else min(p.num_paths, prep.n_paths_loaded)
        return (n, m_rx, m_tx, last)

    def channels(self, prep: PrepResult, out: Optional[torch.Tensor] = None, user_begin: int = 0,
                 user_count: Optional[int] = None, variant: int = 0, tx_codebook=None) -> torch.Tensor:
        """Run stage 2 for users [user_begin, user_begin + user_count) into `out` (allocated if None).

        tx_codebook: optional complex [n_beams, M_tx] beamforming matrix F; the result is then the
        beam-space channel F @ H, complex64 [user_count, M_rx, n_beams, K], produced without ever writing H
        (dmx_channels_fd_beams; frequency domain without rx_filter only)."""
        p = prep.params_struct
        if user_count is None:
            user_count = prep.n_ue - user_begin
        shape = self.channel_shape(prep, user_count)
        cb = None
        if tx_codebook is not None:
            cb = self._codebook(tx_codebook, shape[2])
            if not p.freq_domain or p.rx_filter:
                raise ValueError("tx_codebook needs freq_domain = 1 and rx_filter = 0")
            check_beam_bound(prep.sc_abs_max)
            shape = (shape[0], shape[1], int(cb.shape[0]), shape[3])
        out = self._out(out, shape)
        if out.numel() == 0:
            return out
        wsp = C.c_void_p(prep.workspace.data_ptr())
        with torch.cuda.device(self.device):
            if cb is not None:
                nb = int(cb.shape[0])
                nbytes = int(self.lib.dmx_beam_workspace_bytes(C.byref(p), user_count, prep.n_paths_loaded, nb))
                bws = self._scratch(nbytes)
                rc = self.lib.dmx_channels_fd_beams(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, user_begin,
                                                    user_count, C.c_void_p(cb.data_ptr()), nb, C.c_void_p(bws.data_ptr()), nbytes,
                                                    C.c_void_p(out.data_ptr()), self._stream_ptr())
                nat.check(rc, "dmx_channels_fd_beams")
            elif p.freq_domain and p.rx_filter:
                nbytes = int(self.lib.dmx_lpf_workspace_bytes(C.byref(p), user_count, prep.n_paths_loaded))
                lws = self._scratch(nbytes)
                rc = self.lib.dmx_channels_fd_lpf(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, user_begin,
                                                  user_count, C.c_void_p(lws.data_ptr()), nbytes,
                                                  C.c_void_p(out.data_ptr()), self._stream_ptr())
                nat.check(rc, "dmx_channels_fd_lpf")
            elif p.freq_domain:
                rc = self.lib.dmx_channels_fd(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, user_begin, user_count,
                                              C.c_void_p(out.data_ptr()), self.fd_variant(prep, variant),
                                              self._stream_ptr())
                nat.check(rc, "dmx_channels_fd")
            else:
                rc = self.lib.dmx_channels_td(C.byref(p), wsp, prep.n_ue, prep.n_paths_loaded, user_begin, user_count,
                                              C.c_void_p(out.data_ptr()), self._stream_ptr())
                nat.check(rc, "dmx_channels_td")
        return out

    # ------------------------------------------------------------------ single pass
    def direct_supported(self, rays: DeviceRays, params, structs=None, **prepare_kwargs) -> bool:
        """dmx_fd_direct_supported for these rays and parameters (host-only query; `channels_direct` raises where it
        says no).  structs: what `_call_structs` returned for the same arguments, to build them once."""
        p = (structs or self._call_structs(rays, params, **prepare_kwargs))[0]
        return self._supported("dmx_fd_direct_supported", C.byref(p), rays.n_paths)

    def auto_fd_choice(self, p: nat.DmxParams, n_paths_loaded: int, sc_abs_max: int) -> int:
        """The kernel ``variant = 0`` runs for this parameter block (dmx_fd_kernel_choice, with `fd_variant`'s rule for
        selections beyond the float32-phase bound that carry no spacing promise)."""
        if sc_abs_max < SC_ABS_MAX_F32:
            return int(self.lib.dmx_fd_kernel_choice(C.byref(p), n_paths_loaded))
        return bounded_fd_variant(0, sc_abs_max, self._small_preferred(p, n_paths_loaded))

    def host_copy_chunks(self, n_users: int, per_user_elems: int) -> bool:
        """True when `channels_to_host` would move a tensor of this size in more than one chunk."""
        if n_users == 0 or per_user_elems == 0:
            return False
        return max(1, int(self.HOST_CHUNK_BYTES) // (per_user_elems * 8)) < n_users

    def channels_direct(self, rays: DeviceRays, params, out: Optional[torch.Tensor] = None, user_begin: int = 0,
                        user_count: Optional[int] = None, want_side="light", structs=None, **prepare_kwargs):
        """Ray matrices -> frequency-domain channels in one launch (dmx_channels_fd_direct), no workspace: the small-
        output shapes of variant 9, bit-identical to ``prepare(want_side="light")`` + ``channels(variant=9)``.
        want_side: "light" = LoS / path counts / FoV mask (when a FoV is set) / delay maximum, False = the delay maximum
        only; the rotated angles and powers are stage 1's (``prepare(want_side=True)``).  Returns (out, side) with
        out = complex64 [user_count, M_rx, M_tx, K] and side tensors sized for ALL users of `rays` (the kernel writes
        the rows of the users it ran).  structs: as for `direct_supported`.  Raises where the shape is not taken."""
        if want_side not in ("light", False):
            raise ValueError('channels_direct: want_side must be "light" or False (the heavy side products are stage 1\'s)')
        n, L = rays.n_ue, rays.n_paths
        p, r, keep, _ = structs or self._call_structs(rays, params, **prepare_kwargs)
        if user_count is None:
            user_count = n - user_begin
        out = self._out(out, (user_count, p.ue_shape[0] * p.ue_shape[1], p.bs_shape[0] * p.bs_shape[1], p.n_selected))
        side, s = self._side_tensors(n, L, p.fov_enabled, want_side)
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_channels_fd_direct(C.byref(r), C.byref(p), C.byref(s), int(user_begin), int(user_count),
                                                 C.c_void_p(out.data_ptr()), self._stream_ptr())
        nat.check(rc, "dmx_channels_fd_direct")
        # `keep` (selection, rotations) may go out of scope: the launch is on torch's current stream and the caching
        # allocator reuses freed blocks in stream order
        return out, side

    # ------------------------------------------------------------------ stage 2 -> NumPy
    HOST_CHUNK_BYTES = 256 << 20          # per pipeline stage; two device buffers + two pinned staging buffers of this size
    HOST_COPY_THREADS = 8                 # np.copyto releases the GIL; one thread moves ~12 GB/s, PCIe Gen5 ~57 GB/s

    def channels_to_host(self, prep: PrepResult, variant: int = 0, tx_codebook=None, chunk_bytes: Optional[int] = None,
                         user_begin: int = 0, user_count: Optional[int] = None) -> np.ndarray:
        """Stage 2 straight into a NumPy array (what ``Dataset.compute_channels`` returns by default, as the reference
        does) as a three-stage pipeline over user chunks: the kernels of chunk c + 1 run on the current stream while
        chunk c crosses PCIe into one of two pinned staging buffers on a copy stream and chunk c - 1 is moved from the
        other staging buffer into the result by a few host threads (the first touch of the result's pages happens
        there too).  47 GB/s on the pool's boxes against 14 GB/s for ``tensor.cpu().numpy()``
        (tools/host_copy_probe.py), and the device never holds more than two chunks of the tensor."""
        if user_count is None:
            user_count = prep.n_ue - user_begin
        shape = self.channel_shape(prep, user_count)
        if tx_codebook is not None:
            shape = (shape[0], shape[1], int(tx_codebook.shape[0]), shape[3])
        n, per_user = shape[0], int(np.prod(shape[1:]))
        if n == 0 or per_user == 0:
            return np.empty(shape, dtype=np.complex64)
        if tx_codebook is not None:
            tx_codebook = self._codebook(tx_codebook, self.channel_shape(prep, 0)[2])
        chunk_bytes = int(chunk_bytes or self.HOST_CHUNK_BYTES)
        cu = max(1, chunk_bytes // (per_user * 8))
        if cu >= n:                                               # one chunk: nothing to overlap
            return self.channels(prep, user_begin=user_begin, user_count=n, variant=variant, tx_codebook=tx_codebook).cpu().numpy()
        result = np.empty(shape, dtype=np.complex64)
        flat = result.reshape(n, per_user)
        stage = self._host_stage(cu * per_user)
        stage_np = [t.numpy() for t in stage]
        dev = [torch.empty((cu,) + tuple(shape[1:]), dtype=torch.complex64, device=self.device) for _ in range(2)]
        main = torch.cuda.current_stream(self.device)
        side = self._copy_stream()
        pool = self._copy_pool()
        nthr = self.HOST_COPY_THREADS

        def drain(i, b, cnt, ev):
            ev.synchronize()                                      # chunk is in stage[i]
            src = stage_np[i][:cnt * per_user].reshape(cnt, per_user)
            per = (cnt + nthr - 1) // nthr
            jobs = [pool.submit(np.copyto, flat[b + k:b + min(cnt, k + per)], src[k:min(cnt, k + per)]) for k in range(0, cnt, per)]
            for j in jobs:
                j.result()

        pending = None
        for ci, b in enumerate(range(0, n, cu)):
            i, cnt = ci & 1, min(cu, n - b)
            # dev[i] / stage[i] last held chunk ci - 2, which was drained (hence copied) before this iteration
            self.channels(prep, out=dev[i][:cnt], user_begin=user_begin + b, user_count=cnt, variant=variant, tx_codebook=tx_codebook)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                stage[i][:cnt * per_user].copy_(dev[i][:cnt].reshape(-1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            if pending is not None:
                drain(*pending)
            pending = (i, b, cnt, ev)
        drain(*pending)
        main.wait_stream(side)                                    # dev[] goes back to the allocator in stream order
        return result

    def _host_stage(self, n_elems: int):
        st = getattr(self, "_stage", None)
        if st is None or st[0].numel() < n_elems:
            st = [torch.empty(n_elems, dtype=torch.complex64, pin_memory=True) for _ in range(2)]
            self._stage = st
        return st

    def _copy_stream(self):
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        return self._side_stream

    def _copy_pool(self):
        if getattr(self, "_pool", None) is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.HOST_COPY_THREADS, thread_name_prefix="dmx-host-copy")
        return self._pool

    def beam_power(self, prep: PrepResult, tx_codebook, user_begin: int = 0, user_count: Optional[int] = None,
                   want_best: bool = True, metric: str = "amplitude"):
        """dmx_beam_power: the beam-sweep reduction of docs/manual.ipynb cell 105 without any [N, ., K] tensor.
        Returns (mean_amplitude float32 [user_count, n_beams], best_beam int32 [user_count] or None), both in HBM:
        mean_amplitude[u, b] = np.abs(F @ H[u]).mean(axis=0).mean(axis=-1).  metric "power": the power average (RSRP),
        (np.abs(F @ H[u]) ** 2).mean(axis=0).mean(axis=-1), linear, and its first maximum - DMX_FLAG_BEAM_MEAN_POWER on a copy
        of the preparation's parameter block, for this call only."""
        power = check_beam_metric("beam_power", metric)
        p = prep.params_struct
        user_count = self._users(prep.n_ue, user_begin, user_count)
        m_tx = p.bs_shape[0] * p.bs_shape[1]
        cb = self._codebook(tx_codebook, m_tx, min_beams=1)
        if not p.freq_domain or p.rx_filter:
            raise ValueError("beam_power needs freq_domain = 1 and rx_filter = 0")
        check_beam_bound(prep.sc_abs_max)
        nb = int(cb.shape[0])
        amp = torch.empty((user_count, nb), dtype=torch.float32, device=self.device)
        best = torch.empty((user_count,), dtype=torch.int32, device=self.device) if want_best else None
        if user_count == 0:
            return amp, best
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.dmx_beam_workspace_bytes(C.byref(p), user_count, prep.n_paths_loaded, nb))
            bws = self._scratch(nbytes)
            args = self._record_args(prep, user_begin, user_count)
            if power:
                call_p = nat.DmxParams.from_buffer_copy(p)       # the pointers inside stay owned by the preparation
                call_p.flags |= nat.FLAG_BEAM_MEAN_POWER
                args = (C.byref(call_p),) + args[1:]
            rc = self.lib.dmx_beam_power(*args, _ptr(cb), nb, _ptr(bws), nbytes, _ptr(amp), _ptr(best), self._stream_ptr())
            nat.check(rc, "dmx_beam_power")
        return amp, best

    # ------------------------------------------------------------------ consumers of the path records
    def _supported(self, query: str, *args) -> bool:
        """A host-only dmx_*_supported query: its yes or no; a bad argument raises."""
        rc = getattr(self.lib, query)(*args)
        if rc < 0:
            nat.check(rc, query)
        return rc == 1

    def _prep_supported(self, query: str, prep: PrepResult, *ints, call_p=None) -> bool:
        return self._supported(query, C.byref(prep.params_struct if call_p is None else call_p), prep.n_paths_loaded, *map(int, ints))

    @staticmethod
    def _receiver_params(prep: PrepResult, mmse: bool):
        """The parameter block of a codebook-rate call: the preparation's, or for the linear MMSE receiver a copy of it with
        DMX_FLAG_RX_LINEAR_MMSE (the pointers inside stay owned by the preparation) - an option of the call, as the power
        metric is of `beam_power`."""
        if not mmse:
            return None
        call_p = nat.DmxParams.from_buffer_copy(prep.params_struct)
        call_p.flags |= nat.FLAG_RX_LINEAR_MMSE
        return call_p

    @staticmethod
    def _users(n_ue: int, user_begin: int, user_count: Optional[int]) -> int:
        """`user_count` of a call: None means up to the last user."""
        return n_ue - user_begin if user_count is None else user_count

    def _record_args(self, prep: PrepResult, user_begin: int, user_count: int, call_p=None):
        """The leading arguments of every C call on a preparation's records; `call_p`: the call's own copy of the parameter
        block in place of the preparation's."""
        return (C.byref(prep.params_struct if call_p is None else call_p), C.c_void_p(prep.workspace.data_ptr()), prep.n_ue, prep.n_paths_loaded,
                int(user_begin), int(user_count))

    def covariance_supported(self, prep: PrepResult, side="tx") -> bool:
        """dmx_covariance_supported for this preparation (host-only query; `covariance` raises where it says no)."""
        return self._prep_supported("dmx_covariance_supported", prep, covariance_side(side))

    def covariance(self, prep: PrepResult, side="tx", user_begin: int = 0, user_count: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dmx_channel_covariance: per-user spatial covariance of the frequency-domain channel over the BS array
        (side "tx": R[u, i, j] = mean over rx and subcarriers of H[u, r, i, k] conj(H[u, r, j, k])) or over the UE array
        (side "rx": mean over tx and subcarriers), complex64 [user_count, M, M] in HBM, from the per-path records of
        `prep` - the channel tensor is not written.  Every block is exactly Hermitian."""
        sid = covariance_side(side)
        p = prep.params_struct
        user_count = self._users(prep.n_ue, user_begin, user_count)
        m = p.bs_shape[0] * p.bs_shape[1] if sid == 0 else p.ue_shape[0] * p.ue_shape[1]
        out = self._out(out, (user_count, m, m))
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_channel_covariance(*self._record_args(prep, user_begin, user_count), sid, _ptr(out),
                                                 self._stream_ptr())
        nat.check(rc, "dmx_channel_covariance")
        return out

    def rate_supported(self, prep: PrepResult) -> bool:
        """dmx_rate_supported for this preparation (host-only query; `rate` raises where it says no)."""
        return self._prep_supported("dmx_rate_supported", prep)

    def rate(self, prep: PrepResult, snr_db, user_begin: int = 0, user_count: Optional[int] = None,
             per_subcarrier: bool = False, out=None):
        """dmx_channel_rate: per-user achievable rate in bit/s/Hz at `snr_db` (total transmit power over noise power per
        subcarrier, equal power per BS antenna), rate[u] = mean over k of log2 det(I + snr / M_tx H_k H_k^H), float32
        [user_count] in HBM, from the per-path records of `prep` - the channel tensor is not written.  With
        `per_subcarrier` the pair (rate, rate_k), rate_k float32 [user_count, K].  `out`: the tensor (or the pair of
        tensors) to write into."""
        snr = snr_linear_from_db(snr_db)
        user_count = self._users(prep.n_ue, user_begin, user_count)
        out_r, out_k = out if isinstance(out, (tuple, list)) else (out, None)
        r, = self._outs(out_r, [((user_count,), torch.float32)])
        rk = self._outs(out_k, [((user_count, int(prep.params_struct.n_selected)), torch.float32)])[0] if per_subcarrier else None
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_channel_rate(*self._record_args(prep, user_begin, user_count), snr, _ptr(r), _ptr(rk),
                                           self._stream_ptr())
        nat.check(rc, "dmx_channel_rate")
        return (r, rk) if per_subcarrier else r

    def spectrum_supported(self, prep: PrepResult) -> bool:
        """dmx_spectrum_supported for this preparation (host-only query; `spectrum` raises where it says no)."""
        return self._prep_supported("dmx_spectrum_supported", prep)

    def _wanted_outs(self, out, outputs, torch_names: bool = False):
        """`_outs` of the wanted ones of a call's optional outputs, `outputs` = [(wanted, shape, dtype)]: (the tensors, for
        every output its pointer argument - None where it is not wanted)."""
        res = self._outs(out, [(shape, dt) for want, shape, dt in outputs if want], torch_names)
        it = iter(res)
        return res, [_ptr(next(it)) if want else None for want, _, _ in outputs]

    def spectrum(self, prep: PrepResult, snr_db, user_begin: int = 0, user_count: Optional[int] = None,
                 gamma: bool = True, rate: bool = False, per_subcarrier: bool = False, out=None):
        """dmx_channel_spectrum: the eigenmodes of every subcarrier's channel and the water-filling rate at `snr_db` (total
        transmit power over noise power per subcarrier), from the per-path records of `prep` - the channel tensor is not
        written.  `gamma`: float32 [user_count, K, m] mode SNRs snr * eig(H_k H_k^H), descending, m = min(M_rx, M_tx);
        `rate`: float32 [user_count], the mean over k of the water-filling rate in bit/s/Hz; `per_subcarrier`: float32
        [user_count, K].  Returns the requested tensors in that order, HBM-resident - a single tensor when one is asked
        for, else a tuple.  `out`: the tensor (or the tuple of tensors, in the same order) to write into."""
        snr = snr_linear_from_db(snr_db)
        if not (gamma or rate or per_subcarrier):
            raise ValueError("spectrum: at least one of gamma, rate and per_subcarrier must be asked for")
        p = prep.params_struct
        user_count = self._users(prep.n_ue, user_begin, user_count)
        K, m = int(p.n_selected), min(p.bs_shape[0] * p.bs_shape[1], p.ue_shape[0] * p.ue_shape[1])
        res, ptr = self._wanted_outs(out, [(gamma, (user_count, K, m), torch.float32), (rate, (user_count,), torch.float32),
                                           (per_subcarrier, (user_count, K), torch.float32)])
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_channel_spectrum(*self._record_args(prep, user_begin, user_count), snr, *ptr, self._stream_ptr())
        nat.check(rc, "dmx_channel_spectrum")
        return res[0] if len(res) == 1 else tuple(res)

    def precoder_supported(self, prep: PrepResult, n_layers: int = 1) -> bool:
        """dmx_precoder_supported for this preparation (host-only query; `precoders` raises where it says no)."""
        return self._prep_supported("dmx_precoder_supported", prep, n_layers)

    def precoders(self, prep: PrepResult, snr_db, n_layers: int = 1, user_begin: int = 0, user_count: Optional[int] = None,
                  gamma: bool = True, tx: bool = True, rx: bool = True, out=None):
        """dmx_channel_precoders: the eigenbeams of every subcarrier's channel at `snr_db`, from the per-path records of
        `prep` - the channel tensor is not written.  With H_k = U S V^H, strongest modes first, m = min(M_rx, M_tx) and
        L = `n_layers` in 1..m: `gamma` float32 [user_count, K, m], the mode SNRs snr * s_i^2; `tx` complex64
        [user_count, K, L, M_tx], the precoders v_i; `rx` complex64 [user_count, K, L, M_rx], the combiners u_i (unit norm,
        the gauge and the floor below which a layer is all zeros: include/deepmimo_amd.h).  Returns the requested tensors in
        that order, HBM-resident - a single tensor when one is asked for, else a tuple.  `out`: the tensor (or the tuple
        of tensors, in the same order) to write into."""
        snr = snr_linear_from_db(snr_db)
        if not (gamma or tx or rx):
            raise ValueError("precoders: at least one of gamma, tx and rx must be asked for")
        p = prep.params_struct
        user_count = self._users(prep.n_ue, user_begin, user_count)
        m_tx, m_rx = p.bs_shape[0] * p.bs_shape[1], p.ue_shape[0] * p.ue_shape[1]
        K, L = int(p.n_selected), int(n_layers)
        if not self.precoder_supported(prep, L):                    # DMX_ERR_SHAPE, before an L < 1 reaches torch.empty
            nat.check(-2, "dmx_channel_precoders")
        res, ptr = self._wanted_outs(out, [(gamma, (user_count, K, min(m_tx, m_rx)), torch.float32),
                                           (tx, (user_count, K, L, m_tx), torch.complex64),
                                           (rx, (user_count, K, L, m_rx), torch.complex64)], torch_names=True)
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_channel_precoders(*self._record_args(prep, user_begin, user_count), snr, L, *ptr, self._stream_ptr())
        nat.check(rc, "dmx_channel_precoders")
        return res[0] if len(res) == 1 else tuple(res)

    def _links(self, preps, snrs):
        links = (nat.DmxLink * len(preps))()
        for b, prep in enumerate(preps):
            links[b].prm = C.pointer(prep.params_struct)
            links[b].workspace = prep.workspace.data_ptr()
            links[b].n_paths_loaded = prep.n_paths_loaded
            links[b].snr_linear = snrs[b]
        return links

    def cell_rate_supported(self, preps) -> bool:
        """dmx_cell_rate_supported for these preparations, one per link (host-only query; `cell_rate` raises where it says
        no)."""
        preps = list(preps)
        return self._supported("dmx_cell_rate_supported", self._links(preps, [1.0] * len(preps)), len(preps))

    def cell_rate(self, preps, snr_db, serving=None, user_begin: int = 0, user_count: Optional[int] = None,
                  per_subcarrier: bool = False, details: bool = False, serving_set=None):
        """dmx_cell_rate: per-user downlink rate in bit/s/Hz under inter-cell interference.  `preps`: one preparation per
        link (base station) over the same users; `snr_db`: total transmit power over noise power per subcarrier, a scalar or
        one value per link.  With s the serving link of a user and rho_b = snr_b / M_tx,b,
        rate[u] = mean over k of log2 det(N_k + rho_s H_s,k H_s,k^H) - log2 det N_k, N_k = I + sum over b != s of
        rho_b H_b,k H_b,k^H, float32 [user_count] in HBM from the per-path records - no channel tensor is written.
        `serving`: None (the kernel serves each user by the link of largest link_snr), an int, or an int array / tensor
        [user_count]; a value outside 0..B-1 means not served (rate 0).  Returns rate; with `per_subcarrier` also rate_k
        float32 [user_count, K]; with `details` also serving (int32 [user_count], -1 = not served) and link_snr (float32
        [user_count, B], linear: snr_b times the summed power of the link's kept paths), in that order.
        `serving_set` (in place of `serving`): "all", or a bool or integer array / tensor [user_count, B], non-zero meaning
        that the link transmits to the user - DMX_FLAG_SERVING_SET on copies of the preparations' parameter blocks, for this
        call only.  The members of a user's set add into A_k, every other link into N_k; `details` then gives the set as read,
        bool [user_count, B], in place of the index."""
        preps = list(preps)
        B = len(preps)
        if not 1 <= B <= nat.MAX_LINKS:
            raise ValueError(f"cell rate: {B} links, the call takes 1..{nat.MAX_LINKS}")
        snrs = link_snrs_from_db(snr_db, B)
        n_ue = preps[0].n_ue
        if any(p.n_ue != n_ue for p in preps):
            raise ValueError("cell rate: the links must cover the same users (equal n_ue)")
        user_count = self._users(n_ue, user_begin, user_count)
        serv = None
        members = check_serving_set("cell rate", serving_set, user_count, B, serving)
        if members is not None and not isinstance(members, str):
            t = members if isinstance(members, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(members))
            link = torch.arange(B, dtype=torch.int32, device=self.device)     # device work only: the call stays capturable
            serv = ((t.to(self.device) != 0).to(torch.int32) << link).sum(dim=1, dtype=torch.int32).contiguous()
        if serving is not None:
            if isinstance(serving, (int, np.integer)) and not isinstance(serving, bool):
                serv = torch.full((user_count,), int(np.clip(serving, -1, 2 ** 31 - 1)), dtype=torch.int32, device=self.device)
            else:
                t = serving if isinstance(serving, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(serving))
                if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or tuple(t.shape) != (user_count,):
                    raise ValueError(f"cell rate: serving must be None, an int or an integer array of shape ({user_count},)")
                serv = t.clamp(-1, 2 ** 31 - 1).to(device=self.device, dtype=torch.int32).contiguous()
        K = int(preps[0].params_struct.n_selected)
        r = torch.empty((user_count,), dtype=torch.float32, device=self.device)
        rk = torch.empty((user_count, K), dtype=torch.float32, device=self.device) if per_subcarrier else None
        sv = torch.empty((user_count,), dtype=torch.int32, device=self.device) if details else None
        ls = torch.empty((user_count, B), dtype=torch.float32, device=self.device) if details else None
        links = self._links(preps, snrs)
        call_ps = []                                                        # the flagged copies live until the call returns
        if members is not None:
            for b, prep in enumerate(preps):
                call_p = nat.DmxParams.from_buffer_copy(prep.params_struct)  # the pointers inside stay owned by the preparation
                call_p.flags |= nat.FLAG_SERVING_SET
                call_ps.append(call_p)
                links[b].prm = C.pointer(call_p)
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_cell_rate(links, B, n_ue, int(user_begin), int(user_count), _ptr(serv),
                                        _ptr(r), _ptr(rk), _ptr(sv), _ptr(ls), self._stream_ptr())
        nat.check(rc, "dmx_cell_rate")
        if members is not None and details:
            sv = (sv[:, None] >> torch.arange(B, dtype=torch.int32, device=self.device)[None, :]) & 1 != 0
        res = (r,) + ((rk,) if per_subcarrier else ()) + ((sv, ls) if details else ())
        return res[0] if len(res) == 1 else res

    @staticmethod
    def _angle_delay_params(prep: PrepResult, out_flags: int):
        """The parameter block of an angle-delay call: the preparation's, or for the power and profile outputs a copy of it
        with the output's flags (the pointers inside stay owned by the preparation) - options of the call, as
        `_receiver_params`."""
        if not out_flags:
            return None
        call_p = nat.DmxParams.from_buffer_copy(prep.params_struct)
        call_p.flags |= out_flags
        return call_p

    def angle_delay_supported(self, prep: PrepResult, n_rows: int, n_fft: int, n_taps: int, output: str = "complex") -> bool:
        """dmx_angle_delay_supported for this preparation (host-only query; `angle_delay` raises where it says no)."""
        out_flags = check_angle_delay_output("angle_delay_supported", output)         # before anything else: no engine is needed to be refused
        call_p = self._angle_delay_params(prep, out_flags)
        return self._prep_supported("dmx_angle_delay_supported", prep, n_rows, n_fft, n_taps, call_p=call_p)

    def angle_delay(self, prep: PrepResult, n_taps: int, n_fft: Optional[int] = None, tx_codebook=None, user_begin: int = 0,
                    user_count: Optional[int] = None, out: Optional[torch.Tensor] = None, output: str = "complex") -> torch.Tensor:
        """dmx_channels_angle_delay: the angle-delay representation X = ifft(F @ H, n=n_fft, axis=-1)[..., :n_taps] of the
        frequency-domain channel, complex64 [user_count, M_rx, R, n_taps] in HBM, from the per-path records of `prep` - the
        channel tensor is not written.  tx_codebook: complex [R, M_tx], or None for the antenna domain (R = M_tx, the
        delay-domain channel of every antenna pair).  n_fft: None = the number of selected subcarriers.  The selection has
        to be uniformly spaced.  output "power": the angle-delay power matrix (abs(X) ** 2).sum(1), float32 [user_count, R,
        n_taps]; "profile": its row sum, the power-delay profile, float32 [user_count, n_taps] - raw sums formed in the
        kernel's registers, X is not written; the flags go on a copy of the preparation's parameter block, for this call
        only.  `out` has the shape and dtype of the chosen output."""
        out_flags = check_angle_delay_output("angle_delay", output)                   # before anything else: no engine is needed to be refused
        call_p = self._angle_delay_params(prep, out_flags)
        p = prep.params_struct
        user_count = self._users(prep.n_ue, user_begin, user_count)
        m_rx, m_tx = p.ue_shape[0] * p.ue_shape[1], p.bs_shape[0] * p.bs_shape[1]
        cb = None if tx_codebook is None else self._codebook(tx_codebook, m_tx, min_beams=1)
        rows = m_tx if cb is None else int(cb.shape[0])
        n_fft = int(p.n_selected) if n_fft is None else int(n_fft)
        taps = max(int(n_taps), 0)
        if output == "complex":
            out = self._out(out, (user_count, m_rx, rows, taps))
        else:
            out = self._outs(out, [((user_count, rows, taps) if output == "power" else (user_count, taps), torch.float32)])[0]
        with torch.cuda.device(self.device):
            nbytes, bws = 0, None
            if cb is not None and user_count > 0:
                nbytes = int(self.lib.dmx_beam_workspace_bytes(C.byref(p), user_count, prep.n_paths_loaded, rows))
                bws = self._scratch(nbytes)
            rc = self.lib.dmx_channels_angle_delay(*self._record_args(prep, user_begin, user_count, call_p), _ptr(cb), rows, _ptr(bws),
                                                   nbytes, n_fft, int(n_taps), _ptr(out), self._stream_ptr())
        nat.check(rc, "dmx_channels_angle_delay")
        return out

    CODEBOOK_WS_BYTES = 1 << 30          # beam workspace of one dmx_codebook_rate call; more users go in blocks

    def _codebook_on_device(self, prep: PrepResult, codebook):
        """(complex64 [C, L, M_tx] on the device, C, L) of the `codebook` argument of the codebook-rate calls"""
        p = prep.params_struct
        m_tx = p.bs_shape[0] * p.bs_shape[1]
        cb = self._to_dev(codebook, torch.complex64)
        if cb.dim() == 2:
            cb = cb[:, None, :]
        if cb.dim() != 3 or cb.shape[2] != m_tx or cb.shape[0] < 1 or cb.shape[1] < 1:
            raise ValueError(f"codebook must be [C, L, {m_tx}] or [C, {m_tx}], got {tuple(cb.shape)}")
        return cb, int(cb.shape[0]), int(cb.shape[1])

    def _codebook_user_blocks(self, prep: PrepResult, user_count: int, n_rows: int):
        """(first user of the block, users, beam workspace, its bytes) of the user blocks of a codebook-rate call: the beam
        workspace of a block stays within CODEBOOK_WS_BYTES"""
        p = prep.params_struct
        per_user = n_rows * max(1, min(int(p.num_paths), prep.n_paths_loaded)) * 8 + 4
        block = max(1, (int(self.CODEBOOK_WS_BYTES) - 512) // per_user)
        for b in range(0, user_count, block):
            cnt = min(block, user_count - b)
            nbytes = int(self.lib.dmx_beam_workspace_bytes(C.byref(p), cnt, prep.n_paths_loaded, n_rows))
            yield b, cnt, self._scratch(nbytes), nbytes

    def codebook_rate_supported(self, prep: PrepResult, n_codewords: int, n_layers: int = 1, receiver: str = "joint") -> bool:
        """dmx_codebook_rate_supported for this preparation (host-only query; `codebook_rate` raises where it says no)."""
        mmse = check_receiver("codebook_rate_supported", receiver)                   # before anything else: no engine is needed to be refused
        call_p = self._receiver_params(prep, mmse)
        return self._prep_supported("dmx_codebook_rate_supported", prep, n_codewords, n_layers, call_p=call_p)

    def codebook_rate(self, prep: PrepResult, codebook, snr_db, per_codeword: bool = False, user_begin: int = 0,
                      user_count: Optional[int] = None, receiver: str = "joint"):
        """dmx_codebook_rate: the rate of every codeword of a precoding codebook and the best one per user at `snr_db` (total
        transmit power over noise power per subcarrier, split equally over the layers), from the per-path records of `prep` -
        neither the channel tensor nor the beam-space tensor is written.  `codebook`: complex [C, L, M_tx], C codewords of
        L layers (a 2-D [C, M_tx] is L = 1).  With E = W[c] @ H[u, :, :, k] transposed to M_rx x L,
        rate_c[u, c] = mean over k of log2 det(I + snr / L E^H E).  Returns (rate float32 [user_count], pmi int32
        [user_count]) - pmi the first codeword of the largest rate, -1 and rate 0 for a user without a path - and with
        `per_codeword` also rate_c float32 [user_count, C], all in HBM.  Users go in blocks whose beam workspace stays within
        CODEBOOK_WS_BYTES; a block equals the same rows of one launch bit for bit.  receiver "mmse": the per-layer SINR rate of
        a linear MMSE receiver, rate_c[u, c] = mean over k of -sum_i log2 [(I + snr / L E^H E)^-1]_ii, at or below the joint
        one - DMX_FLAG_RX_LINEAR_MMSE on a copy of the preparation's parameter block, for this call only; at L = 1 the same
        bits as "joint"."""
        mmse = check_receiver("codebook_rate", receiver)                   # before anything else: no engine is needed to be refused
        call_p = self._receiver_params(prep, mmse)
        snr = snr_linear_from_db(snr_db)
        user_count = self._users(prep.n_ue, user_begin, user_count)
        cb, n_cw, n_layers = self._codebook_on_device(prep, codebook)
        if not self.codebook_rate_supported(prep, n_cw, n_layers, receiver):   # DMX_ERR_SHAPE, before anything is allocated
            nat.check(-2, "dmx_codebook_rate")
        rate = torch.empty((user_count,), dtype=torch.float32, device=self.device)
        pmi = torch.empty((user_count,), dtype=torch.int32, device=self.device)
        rate_c = torch.empty((user_count, n_cw), dtype=torch.float32, device=self.device) if per_codeword else None
        with torch.cuda.device(self.device):
            for b, cnt, bws, nbytes in self._codebook_user_blocks(prep, user_count, n_cw * n_layers):
                rc = self.lib.dmx_codebook_rate(*self._record_args(prep, int(user_begin) + b, cnt, call_p), _ptr(cb), n_cw, n_layers,
                                                _ptr(bws), nbytes, snr, _ptr(rate[b:]), _ptr(pmi[b:]),
                                                _ptr(rate_c[b:]) if per_codeword else None, self._stream_ptr())
                nat.check(rc, "dmx_codebook_rate")
        return (rate, pmi, rate_c) if per_codeword else (rate, pmi)

    def codebook_rate_subbands_supported(self, prep: PrepResult, n_codewords: int, n_layers: int = 1, subband_size: int = 1,
                                         receiver: str = "joint") -> bool:
        """dmx_codebook_rate_subbands_supported for this preparation (host-only query)."""
        mmse = check_receiver("codebook_rate_subbands_supported", receiver)                   # before anything else: no engine is needed to be refused
        call_p = self._receiver_params(prep, mmse)
        return self._prep_supported("dmx_codebook_rate_subbands_supported", prep, n_codewords, n_layers, subband_size, call_p=call_p)

    def codebook_rate_subbands(self, prep: PrepResult, codebook, snr_db, subband_size, per_codeword: bool = False,
                               user_begin: int = 0, user_count: Optional[int] = None, receiver: str = "joint"):
        """dmx_codebook_rate_subbands: `codebook_rate` with a PMI per subband in the same launch.  Subband s covers the
        selection positions s B .. min((s + 1) B, K) - 1, B = `subband_size` (an integer >= 1; None: one subband over the
        whole selection), n_sb = ceil(K / B).  Returns (rate [user_count], pmi [user_count], rate_sb [user_count, n_sb],
        pmi_sb [user_count, n_sb]) - float32 / int32 - and with `per_codeword` also rate_c [user_count, C] and rate_sb_c
        [user_count, n_sb, C], all in HBM.  Column s of the subband outputs equals `codebook_rate` on the selection
        sc[s B : (s + 1) B] bit for bit, and with one subband everything equals `codebook_rate`; with more the wideband
        outputs add the subbands in order (another summation order than `codebook_rate`).  User blocks and `receiver` as
        `codebook_rate`."""
        mmse = check_receiver("codebook_rate_subbands", receiver)                   # before anything else: no engine is needed to be refused
        call_p = self._receiver_params(prep, mmse)
        snr = snr_linear_from_db(snr_db)
        B = check_subband_size(subband_size)
        K = int(prep.params_struct.n_selected)
        B = max(1, K) if B is None else min(B, max(1, K))
        user_count = self._users(prep.n_ue, user_begin, user_count)
        cb, n_cw, n_layers = self._codebook_on_device(prep, codebook)
        if not self.codebook_rate_subbands_supported(prep, n_cw, n_layers, B, receiver):   # DMX_ERR_SHAPE, before anything is allocated
            nat.check(-2, "dmx_codebook_rate_subbands")
        n_sb = (K + B - 1) // B
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)   # noqa: E731
        rate, pmi = new((user_count,), torch.float32), new((user_count,), torch.int32)
        rate_sb, pmi_sb = new((user_count, n_sb), torch.float32), new((user_count, n_sb), torch.int32)
        rate_c = new((user_count, n_cw), torch.float32) if per_codeword else None
        rate_sb_c = new((user_count, n_sb, n_cw), torch.float32) if per_codeword else None
        ptr = lambda t, b: None if t is None else _ptr(t[b:])   # noqa: E731
        with torch.cuda.device(self.device):
            for b, cnt, bws, nbytes in self._codebook_user_blocks(prep, user_count, n_cw * n_layers):
                rc = self.lib.dmx_codebook_rate_subbands(*self._record_args(prep, int(user_begin) + b, cnt, call_p), _ptr(cb), n_cw, n_layers,
                                                         _ptr(bws), nbytes, snr, B, ptr(rate_sb, b), ptr(pmi_sb, b),
                                                         ptr(rate_sb_c, b), ptr(rate, b), ptr(pmi, b), ptr(rate_c, b),
                                                         self._stream_ptr())
                nat.check(rc, "dmx_codebook_rate_subbands")
        res = (rate, pmi, rate_sb, pmi_sb)
        return res + (rate_c, rate_sb_c) if per_codeword else res

    def pathloss(self, rays: DeviceRays, coherent: bool = True) -> torch.Tensor:
        """dmx_pathloss: float32 [n_ue] dB (dataset.py:541-566)."""
        out = torch.empty((rays.n_ue,), dtype=torch.float32, device=self.device)
        r = nat.DmxRays()
        r.n_ue, r.n_paths, r.ld = rays.n_ue, rays.n_paths, rays.n_paths
        if rays.n_ue * rays.n_paths > 0:
            r.power, r.phase = rays.fields[c.POWER_PARAM_NAME].data_ptr(), rays.fields[c.PHASE_PARAM_NAME].data_ptr()
        with torch.cuda.device(self.device):
            rc = self.lib.dmx_pathloss(C.byref(r), int(bool(coherent)), C.c_void_p(out.data_ptr()), self._stream_ptr())
        nat.check(rc, "dmx_pathloss")
        return out

    def max_delay(self, prep: PrepResult) -> float:
        """nanmax(delay[:, :P]) as the kernel saw it (channel.py:231); synchronises."""
        key = int(prep.side["max_delay_key"].cpu().numpy().astype(np.uint32)[0])
        return float(self.lib.dmx_decode_max_delay(key))
