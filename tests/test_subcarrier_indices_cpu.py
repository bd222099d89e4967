"""CPU tests of what the host decides about subcarrier indices (no GPU): the spacing promise uniform_stride hands the
library, the engine's selection check and its routing under DMX_SC_ABS_MAX_F32, and dmx_fd_kernel_choice with promises
of negative and large indices.  tests/test_gpu_subcarrier_indices.py runs the kernels on the same index ranges."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deepmimo_amd.engine import (SC_ABS_MAX_F32, bounded_fd_variant, check_beam_bound, check_selection,
                                 uniform_stride)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = (-2 ** 31, 2 ** 31 - 1)
F32_PHASE_VARIANTS = (2, 3, 4, 5, 8, 10, 11, 12)


def test_bound_matches_the_header():
    header = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    assert int(re.search(r"#define DMX_SC_ABS_MAX_F32 (\d+)", header).group(1)) == SC_ABS_MAX_F32 == 2 ** 15


def _selections(rng, count):
    """seeded int64 selections: arithmetic runs (any sign, strides around 0 and 2^20, starts near 0, 2^30, 2^31 and
    beyond), some with one entry moved, repeated or appended, plus unstructured draws"""
    starts = [0, 1, -1, -5, 4095, -4096, 2 ** 15, -2 ** 15, 2 ** 30 - 1, -2 ** 30 + 1, 2 ** 30, -2 ** 30,
              2 ** 31 - 1, -2 ** 31, 2 ** 31, -2 ** 31 - 1, 2 ** 40, -2 ** 40]
    for i in range(count):
        kind = i % 4
        if kind == 3:
            K = int(rng.integers(0, 40))
            yield rng.integers(-2 ** 33, 2 ** 33, K) if i % 8 == 3 else rng.integers(-50, 50, K)
            continue
        f = int(rng.choice(starts)) + int(rng.integers(-3, 4))
        s = int(rng.choice([-2, -1, 0, 1, 2, 3, 7, 2 ** 20 - 1, 2 ** 20, int(rng.integers(1, 2 ** 22))]))
        K = int(rng.choice([0, 1, 2, 3, 16, 17, int(rng.integers(1, 600))]))
        sel = f + s * np.arange(K, dtype=np.int64)
        if kind == 1 and K >= 2:
            j = int(rng.integers(0, K))
            sel[j] += int(rng.choice([-1, 1, 2 ** 32]))
        elif kind == 2 and K >= 1:
            sel = np.append(sel, sel[int(rng.integers(0, K))])
        yield sel


def test_uniform_stride_promises_only_what_holds():
    rng = np.random.default_rng(2024)
    hinted = 0
    for sel in _selections(rng, 4000):
        f, s = uniform_stride(sel)
        if s == 0:
            assert f == 0
            K = sel.size
            d = int(sel[1] - sel[0]) if K >= 2 else 1
            # a promise it could have made: a run with stride 1..2^20-1 from |first| < 2^30 that stays inside int32
            could = (K >= 1 and abs(int(sel[0])) < 2 ** 30 and 0 < d < 2 ** 20 and int(sel[0]) + d * (K - 1) <= I32[1]
                     and np.array_equal(sel, sel[0] + d * np.arange(K)))
            assert not could, sel
            continue
        hinted += 1
        assert s > 0 and I32[0] <= f <= I32[1] and s <= I32[1]
        want = f + s * np.arange(sel.size, dtype=np.int64)
        assert np.array_equal(sel, want), (f, s, sel)
        assert want.min() >= I32[0] and want.max() <= I32[1]
    assert hinted > 300
    assert uniform_stride(np.arange(-256, 256)) == (-256, 1) and uniform_stride(np.array([-5])) == (-5, 1)
    assert uniform_stride(np.arange(-63, 65, 2)) == (-63, 2) and uniform_stride(np.arange(-4146, -4046)) == (-4146, 1)


def test_selection_check():
    for sel in ([2 ** 31], [-2 ** 31 - 1], [0, 2 ** 40], np.array([3, -2 ** 63], dtype=np.int64)):
        with pytest.raises(ValueError, match="int32"):
            check_selection(sel)
    s, m = check_selection(np.array([-2 ** 31, 2 ** 31 - 1]))
    assert s.dtype == np.int64 and m == 2 ** 31
    s, m = check_selection([])
    assert s.size == 0 and m == 0
    assert check_selection(np.arange(-256, 256))[1] == 256
    assert check_selection(np.arange(2 ** 15 - 300, 2 ** 15))[1] == 2 ** 15 - 1
    assert check_selection(np.arange(-2 ** 15 + 1, -2 ** 15 + 301))[1] == 2 ** 15 - 1
    assert check_selection([-2 ** 15])[1] == 2 ** 15
    assert check_selection(np.array([[3, -9], [4, 1]]))[0].shape == (4,)


def test_bound_routing():
    below, at = SC_ABS_MAX_F32 - 1, SC_ABS_MAX_F32
    for v in (0, 1, 9) + F32_PHASE_VARIANTS:
        for small in (False, True):
            assert bounded_fd_variant(v, below, small) == v
    for m in (at, 2 ** 22, 2 ** 31):
        assert bounded_fd_variant(0, m, False) == 1 and bounded_fd_variant(0, m, True) == 9
        assert bounded_fd_variant(1, m, False) == 1 and bounded_fd_variant(9, m, True) == 9
        for v in F32_PHASE_VARIANTS:
            with pytest.raises(ValueError, match=str(SC_ABS_MAX_F32)):
                bounded_fd_variant(v, m, False)
        with pytest.raises(ValueError, match=str(SC_ABS_MAX_F32)):
            check_beam_bound(m)
    check_beam_bound(below)


def _choice(bs, ue, K, first=0, stride=0, L=25):
    from deepmimo_amd import _native as n
    lib = n.load()
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = L, 1, 512, K, 10e6
    p.sc_first, p.sc_stride = first, stride
    return lib.dmx_fd_kernel_choice(C.byref(p), L)


SHAPES = [((8, 1), (1, 1), 512), ((8, 1), (1, 1), 64), ((8, 1), (1, 1), 4), ((8, 1), (1, 1), 1), ((8, 4), (1, 1), 512),
          ((4, 4), (2, 1), 16), ((8, 4), (1, 1), 4), ((8, 6), (1, 1), 1024), ((8, 8), (1, 1), 512), ((8, 8), (2, 1), 8),
          ((8, 8), (2, 2), 512), ((8, 8), (2, 2), 16), ((16, 16), (2, 2), 2), ((64, 64), (1, 1), 1), ((4, 1), (1, 1), 1024)]


@pytest.mark.parametrize("bs,ue,K", SHAPES)
def test_kernel_choice_with_negative_and_large_promises(bs, ue, K):
    for stride in (1, 3):
        base = _choice(bs, ue, K, 0, stride)
        # a negative first index inside the bound: the same kernel as the non-negative run of that length and stride
        for first in (-1, -5, -(K * stride) // 2, -4096 - 50, -(SC_ABS_MAX_F32 - 1)):
            if abs(first + stride * (K - 1)) < SC_ABS_MAX_F32:
                assert _choice(bs, ue, K, first, stride) == base, (first, stride)
        assert _choice(bs, ue, K, SC_ABS_MAX_F32 - 1 - stride * (K - 1), stride) == base
        # reaching the bound at either end (int64 arithmetic: also where the last index would wrap int32): the
        # float64-phase kernels, 9 where the small-output kernel is the choice without a promise, else 1
        small = _choice(bs, ue, K) == 9
        for first in (SC_ABS_MAX_F32, -SC_ABS_MAX_F32, SC_ABS_MAX_F32 - stride * (K - 1), -SC_ABS_MAX_F32 - 7,
                      2 ** 22, -2 ** 30, I32[1] - 10, I32[0]):
            if K == 1 and abs(first) < SC_ABS_MAX_F32:
                continue
            assert _choice(bs, ue, K, first, stride) == (9 if small else 1), (first, stride)
    assert _choice((8, 8), (2, 2), 512, 2 ** 22, 1) == 1 and _choice((8, 1), (1, 1), 512, -2 ** 20, 7) == 1
    assert _choice((8, 1), (1, 1), 1, 2 ** 22, 1) == 9
