"""CPU-side lint of the headline instantiation of the matrix-core kernel with the factorised B' (k2_fd_mfma<true, 8, 2, 4>:
8 waves, pipelined tile body, uniformly spaced selection).  What k2_mfma_frag.h (fact_b_step) and
k2_channel_fd_mfma.hip promise for it: a packed last K-step makes a 25-path tile 10 MFMAs instead of 12, the B'
generation has no per-phasor sin/cos and no lane-pair exchange, and the kernel does not spill."""
import os
import re
import subprocess

import pytest

from tests.test_isa_lint import LIB, isa_lint, _notes

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(isa_lint.OBJDUMP)),
                                reason="needs the built library and llvm-objdump")

FACT = "k2_fd_mfma<true, 8, 2, 4>"
TWIN = "k2_fd_mfma<true, 8, 2, 0>"          # the same body with the sin/cos B'


@pytest.fixture(scope="module")
def kernels():
    ks = isa_lint.kernels_of_library(LIB)
    named = {isa_lint.short_name(k): v for k, v in ks.items()}
    assert FACT in named and TWIN in named, sorted(n for n in named if n.startswith("k2_fd_mfma"))
    return named


def _innermost_loops(insts):
    """(first, last) instruction indices of the loops that contain no other loop (backward branches)"""
    pos = {i.addr: n for n, i in enumerate(insts)}
    loops = [(pos[i.target], n) for n, i in enumerate(insts)
             if i.kind in ("branch", "cbranch") and 0 <= i.target <= i.addr and i.target in pos]
    return [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]


def _sincos(insts, a=0, b=None):
    return sum(1 for i in insts[a:b] if i.mnem.startswith(("v_sin_f32", "v_cos_f32")))


def test_tile_loop_of_a_packed_25_path_strip_has_ten_mfmas_per_tile(kernels):
    insts = kernels[FACT]
    counts = sorted(sum(1 for i in insts[a:b + 1] if i.kind == "mfma") for a, b in _innermost_loops(insts))
    # the pipelined strip walks two tiles per iteration: 4 K-steps, the last one packed = 2 x 10, all three terms = 2 x 12
    assert 20 in counts and 24 in counts, counts


def test_no_sin_cos_or_lane_exchange_in_the_tile_loops(kernels):
    insts = kernels[FACT]
    for a, b in _innermost_loops(insts):
        if any(i.kind == "mfma" for i in insts[a:b + 1]):
            body = [i.mnem for i in insts[a:b + 1]]
            assert not any(m.startswith(("v_sin", "v_cos", "ds_bpermute", "scratch_")) for m in body), (a, b)
    # per strip one sin/cos pair (E1, one lane per path) instead of eight per lane: fewer in the whole kernel than its twin
    assert _sincos(insts) < _sincos(kernels[TWIN]), (_sincos(insts), _sincos(kernels[TWIN]))


def test_headline_instantiation_does_not_spill(tmp_path):
    info = {}
    for co in isa_lint.extract_code_objects(LIB, str(tmp_path)):
        info.update(_notes(co))
    demangled = {}
    for k, v in info.items():
        d = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        demangled[re.sub(r"\(.*$", "", d).replace("void ", "").replace("dmx::", "")] = v
    v = demangled[FACT]
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v["vgpr_count"] <= 128, v
