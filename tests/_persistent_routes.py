"""Route table of tests/test_gpu_persistent_loops.py: one entry per (shape, selection, variant) that drives a persistent
kernel of deepmimo_amd/csrc/ through more work items than its grid holds, and the launchers' grid-sizing rules restated
as upper bounds.  A plain module (no torch, no GPU): tests/test_persistent_routes_cpu.py checks that every
`__global__` kernel with a gridDim-strided loop is named by at least one route.

Bounds: every launcher sizes its grid from the CU count and from how many of its workgroups fit one CU.  The bounds
below take the second from two hard limits of the MI355X (32 waves and 160 KiB of LDS per CU) and NOT from the
occupancy query, so they hold whatever the compiler does to the kernels' register counts.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

WAVES_PER_CU = 32                 # MI355X: 8 waves per SIMD x 4 SIMDs
LDS_PER_CU = 160 * 1024

# the kernels whose workgroups or waves loop over work items (gridDim-strided loops)
PERSISTENT_KERNELS = ("k2_fd_mfma", "k2b_beam_project_mfma", "k2_fd_fold", "k2_fd_small", "k2c_beam_power",
                      "k3_lpf_fft_wave", "k3_lpf_fft_pow2")


def _cdiv(a, b):
    return -(-a // b)


def _per_cu(nw, lds_bytes):
    """workgroups of `nw` waves and `lds_bytes` of LDS that one CU can hold at most"""
    n = WAVES_PER_CU // nw
    if lds_bytes:
        n = min(n, LDS_PER_CU // lds_bytes)
    return max(1, n)


# ---- LDS of the matrix-core kernel (k2_mfma_frag.h:12-15, 134-137; k2_channel_fd_mfma.hip:255-257, 428, 529) ---------
ROW_BYTES, LPAD, MAX_ROWS = 144, 32, 256
FACT_E2_BYTES, FACT_C1_BYTES = 2 * (15 * 36 + LPAD) * 4, 3 * LPAD * 4
DMA_SLOT_BYTES = 4096


def mfma_lds_bytes(rows, nw, gsrc):
    b = 2 * rows * ROW_BYTES + LPAD * (8 + 4 + 4) + 16                      # item_lds_bytes
    if gsrc == 4:
        b += FACT_E2_BYTES + nw * FACT_C1_BYTES                             # fact_lds_bytes (launch_mfma_t)
    if gsrc == 3:
        b += nw * DMA_SLOT_BYTES                                            # the static dma_slots of consume_item
    return b


@dataclass(frozen=True)
class Launch:
    """One persistent kernel launch of a route.  kind selects the sizing rule of grid_upper_bound."""
    kernel: str
    kind: str                    # mfma | beam_project | beam_power | fft_wave_per_user | fft_wave | fold | small
    nw: int = 4                  # waves per workgroup
    lds: int = 0                 # LDS bytes per workgroup (0: bounded by waves only)
    items_per_wg: int = 0        # mfma: ITEMS_PER_WG / ITEMS_PER_WG8 / 0 = resident grid
    persistent: bool = True
    shared: bool = False         # fold: one table set per workgroup (workgroup per item) instead of per wave
    wpb: int = 0                 # small: waves per workgroup (one user per wave)
    gsrc: int = 0
    mode: int = 0


@dataclass(frozen=True)
class Route:
    name: str
    what: str
    bs: Tuple[int, int]
    ue: Tuple[int, int]
    L: int
    N: int
    sel: tuple                   # ("range", a, b, s) | ("random", K, seed) | ("list", values...)
    U: int
    launches: Tuple[Launch, ...]
    kind: str = "fd"             # fd | beams | beam_power | lpf
    variant: int = 0             # dm fd_kernel_variant passed to eng.channels (fd only)
    auto: Optional[int] = None   # what dmx_fd_kernel_choice must answer for this shape (plain channel routes)
    flat: bool = False           # every valid path within 6 dB (test_gpu_fd_factorised._flat): TAIL_TOL applies
    doppler: bool = False
    n_beams: int = 0
    variants: Tuple[int, ...] = field(default=())      # h: further variants checked against variant 8


def selection(route):
    s = route.sel
    if s[0] == "range":
        return np.arange(s[1], s[2], s[3])
    if s[0] == "random":
        return np.sort(np.random.default_rng(s[2]).choice(route.N, size=s[1], replace=False))
    return np.asarray(s[1:])


def m_pairs(route):
    m_rx = route.ue[0] * route.ue[1]
    return m_rx * (route.n_beams if route.n_beams else route.bs[0] * route.bs[1])


def items_per_user(route, launch):
    """work items per user of one launch"""
    if launch.kind == "mfma":
        return _cdiv(m_pairs(route), MAX_ROWS)                                         # k2_channel_fd_mfma.hip:963
    if launch.kind == "fold":
        nblk = _cdiv(len(selection(route)), 16)                                         # k2_channel_fd_fold.hip:673-679
        return max(1, _cdiv(nblk, 64))                                                  # FOLD_SUPER: sch = 64 or >= nblk
    return 1


def grid_upper_bound(route, launch, items, cu):
    """Largest grid (workgroups) the launcher of `launch` can choose for `items` work items on `cu` CUs."""
    k = launch.kind
    if k == "mfma":
        # k2_channel_fd_mfma.hip:854-863 (resident_grid) and :871
        if not launch.persistent:
            return items
        grid = cu * _per_cu(launch.nw, launch.lds)
        if launch.items_per_wg > 0:
            g = items // launch.items_per_wg
            if g < 4 * grid:
                g = min(items, 4 * grid)
            grid = max(grid, g)
        return min(items, grid)
    if k == "beam_project":
        return min(_cdiv(items, 4), 2048)                                               # k2_channel_fd_mfma.hip:918-919
    if k == "beam_power":
        grid = cu * _per_cu(launch.nw, launch.lds)                                      # k2c_beam_power.hip:289-293
        g4 = items // 4
        if g4 > grid:
            grid = min(g4, 4 * grid)
        return min(items, grid)
    if k == "fft_wave_per_user":                                                        # k3_lpf_gains.hip:651-655 (launch_wave_fft)
        return min(cu * _per_cu(4, launch.lds), _cdiv(items, 4))
    if k == "fft_wave":
        return min(cu * _per_cu(4, launch.lds), items)                                  # k3_lpf_gains.hip:692-693
    if k == "fold":
        # k2_channel_fd_fold.hip:689 (smem >= FOLD_MIN_LDS = 160 KiB / 5 + 64: at most four per CU) and :692-694
        grid = cu * _per_cu(4, LDS_PER_CU // 5 + 64)
        return min(grid, items if launch.shared else _cdiv(items, 4))
    if k == "small":
        # k2_channel_fd_small.hip:65-70: the CU count is a constant 256 there
        per_cu = max(1, min(LDS_PER_CU // launch.lds, WAVES_PER_CU // launch.wpb))
        return min(_cdiv(items, launch.wpb), 256 * per_cu)
    raise ValueError(k)


def items_per_slot(launch):
    """work items one workgroup (1) or one wave (waves per workgroup) takes per loop iteration"""
    if launch.kind in ("beam_project", "fft_wave_per_user"):
        return 4
    if launch.kind == "fold" and not launch.shared:
        return 4
    if launch.kind == "small":
        return launch.wpb
    return 1


def slot_bound(route, launch, cu):
    """upper bound on the workgroups (or waves, for wave-per-item kernels) of the whole launch: items beyond it are
    certainly not the first of their workgroup / wave"""
    items = route.U * items_per_user(route, launch)
    return grid_upper_bound(route, launch, items, cu) * items_per_slot(launch)


# ---- the routes --------------------------------------------------------------------------------------------------
def _mfma(nw, mode, gsrc, rows, ipw, persistent=True):
    return Launch("k2_fd_mfma", "mfma", nw=nw, lds=mfma_lds_bytes(rows, nw, gsrc), items_per_wg=ipw,
                  persistent=persistent, gsrc=gsrc, mode=mode)


_FFT512 = Launch("k3_lpf_fft_pow2", "fft_wave_per_user", lds=4 * (512 + 512 // 16 + 1) * 8)        # k3_lpf_gains.hip:685-686, one path per wave
_FFT128 = Launch("k3_lpf_fft_pow2", "fft_wave_per_user", lds=4 * 4 * (128 + 128 // 16 + 1) * 8)    # the same, four paths per wave
_FFTW512 = Launch("k3_lpf_fft_wave", "fft_wave", lds=512 * 8 + 4 * 2 * (512 + 512 // 16 + 1) * 8)  # :263
_FFTW2048 = Launch("k3_lpf_fft_wave", "fft_wave", lds=2048 * 8 + 4 * 2 * (2048 + 2048 // 16 + 1) * 8)

ROUTES = (
    # GSRC 4 (factorised B', uniform selection); 8-wave workgroups with ITEMS_PER_WG8
    Route("a", "mfma GSRC 4, 8 waves, MODE 2", (8, 8), (2, 2), 25, 512, ("range", 0, 128, 1), 8192,
          (_mfma(8, 2, 4, 256, 8),), auto=2, flat=True),
    Route("b", "mfma GSRC 4, 8 waves, MODE 1", (8, 8), (2, 2), 12, 512, ("range", 0, 128, 1), 8192,
          (_mfma(8, 1, 4, 256, 8),), auto=2, flat=True),
    Route("c", "mfma GSRC 4, 8 waves, MODE 0 (64 rows, 16 strips)", (8, 4), (2, 1), 25, 512, ("range", 3, 512, 2), 12288,
          (_mfma(8, 0, 4, 64, 8),), variant=2, auto=12),
    Route("d", "mfma GSRC 4, 4 waves, resident grid", (8, 4), (1, 1), 25, 512, ("range", 5, 101, 1), 8192,
          (_mfma(4, 0, 4, 32, 0),), variant=2, auto=12),
    # the same shapes with an irregular selection: sin/cos B' (GSRC 0)
    Route("e", "mfma GSRC 0 (sin/cos), 8 waves, MODE 2", (8, 8), (2, 2), 25, 512, ("random", 128, 11), 8192,
          (_mfma(8, 2, 0, 256, 8),), auto=2, flat=True),
    Route("f", "mfma GSRC 0, 8 waves, MODE 0", (8, 4), (2, 1), 25, 512, ("random", 255, 12), 12288,
          (_mfma(8, 0, 0, 64, 8),), variant=2, auto=2),
    Route("g", "mfma GSRC 0, 4 waves, resident grid", (8, 4), (1, 1), 25, 512, ("random", 96, 13), 8192,
          (_mfma(4, 0, 0, 32, 0),), variant=2, auto=2),
    # the forced variants on the shapes of a and e (k2_channel_fd_mfma.hip:1022-1028): 4 = go4 x ITEMS_PER_WG,
    # 5 = go8, 3 = 16 waves with plain stores, 10 = go16 x ITEMS_PER_WG, 11 = go16 on the resident grid; variant 8 (go16,
    # one workgroup per item) is the loop-free instantiation 10 and 11 must equal bit for bit
    Route("h_fact", "variants 4, 5, 3, 10, 11 vs 8 on a", (8, 8), (2, 2), 25, 512, ("range", 0, 128, 1), 8192,
          (_mfma(4, 0, 4, 256, 4), _mfma(8, 2, 4, 256, 8), _mfma(16, 0, 0, 256, 4), _mfma(16, 2, 0, 256, 4),
           _mfma(16, 2, 0, 256, 0)), auto=2, flat=True, variants=(4, 5, 3, 10, 11)),
    Route("h_sincos", "variants 4, 5, 3, 10, 11 vs 8 on e", (8, 8), (2, 2), 25, 512, ("random", 128, 11), 8192,
          (_mfma(4, 0, 0, 256, 4), _mfma(8, 2, 0, 256, 8), _mfma(16, 0, 0, 256, 4), _mfma(16, 2, 0, 256, 4),
           _mfma(16, 2, 0, 256, 0)), auto=2, flat=True, variants=(4, 5, 3, 10, 11)),
    # beams: projection (wave per user, codebook staged once per workgroup) + the contraction over 2 x 32 (rx, beam)
    # rows (4 waves, resident grid); beam power: its own reduction kernel over the same rays and codebook
    Route("i", "beams: k2b_beam_project_mfma + mfma GSRC 0, 4 waves", (8, 8), (2, 1), 25, 512, ("range", 0, 512, 8), 20480,
          (Launch("k2b_beam_project_mfma", "beam_project"), _mfma(4, 0, 0, 64, 0)), kind="beams", n_beams=32),
    Route("j", "k2c_beam_power (8 waves)", (8, 8), (2, 1), 25, 512, ("range", 0, 512, 8), 20480,
          (Launch("k2b_beam_project_mfma", "beam_project"), Launch("k2c_beam_power", "beam_power", nw=8)),
          kind="beam_power", n_beams=32),
    # rx_filter: the packed f16 gains table (GSRC 2) in 8-wave workgroups, K = 200 (not a multiple of 16: no DMA), and
    # the guarded-store N = 512 FFT with the Doppler term
    Route("k", "rx_filter GSRC 2, 8 waves + k3_lpf_fft_pow2 (N = 512), Doppler", (8, 4), (2, 2), 25, 512, ("range", 0, 200, 1), 16384,
          (_mfma(8, 0, 2, 128, 8), _FFT512), kind="lpf", doppler=True),
    # GSRC 3: the LDS-DMA chain (the next item's first strip prefetched into the wave's slot), whole and ragged blocks
    Route("l256", "rx_filter GSRC 3 (DMA chain), 256 rows", (8, 8), (2, 2), 25, 512, ("range", 0, 256, 1), 4096,
          (_mfma(16, 0, 3, 256, 4),), kind="lpf"),
    Route("l320", "rx_filter GSRC 3 (DMA chain), 320 rows = 256 + 64", (10, 8), (2, 2), 25, 512, ("range", 0, 256, 1), 2048,
          (_mfma(16, 0, 3, 256, 4),), kind="lpf"),
    Route("m", "rx_filter GSRC 2 small (4 waves, resident grid) + k3_lpf_fft_pow2 (N = 128)", (4, 4), (2, 1), 25, 128,
          ("range", 0, 64, 1), 20480, (_mfma(4, 0, 2, 32, 0), _FFT128), kind="lpf"),
    Route("n", "k3_lpf_fft_pow2 (N = 512, float table) + the vector contraction, Doppler", (2, 1), (1, 1), 25, 512,
          ("range", 0, 512, 1), 20480, (_FFT512,), kind="lpf", doppler=True),
    Route("o", "k3_lpf_fft_wave (K = 600 > N = 512)", (2, 1), (1, 1), 25, 512, ("range", 0, 600, 1), 8192,
          (_FFTW512,), kind="lpf"),
    # the same kernel at N = 2048, its only route there: 155,712 B of LDS = one workgroup per CU, which reuses its twiddle
    # table and both transform buffers of every wave across 8 users of changing path counts; last pass of radix 4
    Route("o2048", "k3_lpf_fft_wave at N = 2048 (one workgroup per CU), Doppler", (2, 1), (1, 1), 25, 2048, ("random", 64, 17),
          2048, (_FFTW2048,), kind="lpf", doppler=True),
    # GSRC 1 (the float gains table with matrix cores): rx_filter with more than 32 path slots (lpf_table_packed is
    # false, k2_channel_fd.hip:308); the first 32 kept paths go through the matrix cores, the rest through the vector
    # kernel's accumulate passes
    Route("s", "rx_filter GSRC 1 (40 paths), 8 waves + k3_lpf_fft_pow2 (N = 512) float table", (4, 4), (2, 1), 40, 512,
          ("range", 0, 256, 1), 16384, (_mfma(8, 0, 1, 32, 8), _FFT512), kind="lpf"),
    # the folded kernel: one wave per item (8 pairs), and the shared-table form (64 pairs)
    Route("p", "k2_fd_fold, one wave per item", (8, 1), (1, 1), 25, 512, ("range", 0, 512, 1), 16384,
          (Launch("k2_fd_fold", "fold"),), auto=12),
    Route("q", "k2_fd_fold, shared tables (workgroup per item), variant 12", (8, 4), (2, 1), 25, 512, ("range", 0, 256, 2),
          8192, (Launch("k2_fd_fold", "fold", shared=True),), variant=12, auto=12),
    # the small-output kernel (one wave per user, four per workgroup)
    Route("r1", "k2_fd_small, K = 1", (8, 8), (1, 1), 25, 512, ("list", 0), 16384,
          (Launch("k2_fd_small", "small", wpb=4, lds=4 * (1 + 64 + 1) * 25 * 8),), variant=9, auto=9),
    Route("r3", "k2_fd_small, K = 3", (8, 8), (1, 1), 25, 512, ("list", 3, 9, 27), 16384,
          (Launch("k2_fd_small", "small", wpb=4, lds=4 * (1 + 64 + 3) * 25 * 8),), variant=9, auto=9),
)

ROUTES_BY_NAME = {r.name: r for r in ROUTES}
