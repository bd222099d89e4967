"""Host side of the per-user spatial covariance (dmx_covariance_supported / dmx_channel_covariance, k6_covariance.hip) -
no GPU: the symbols, the shape query against a restatement of the launcher's LDS rule, the errors of
Dataset.compute_covariance that must come before any GPU call, the pinned reference of the GPU tests (closed form against
the definition, both in float64 NumPy) and the code-object notes of the kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._covariance_ref import SIDES, cov_closed_form, cov_err, cov_from_channel
from tests.test_isa_lint import LIB, ROOT, isa_lint, _notes

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

LDS_MAX = 156 * 1024
TX, RX = 0, 1


def _params(bs=(8, 1), ue=(1, 1), K=1, num_paths=25, freq_domain=1, rx_filter=0, flags=0):
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = num_paths, freq_domain, 512, K, 10e6
    p.rx_filter, p.flags = rx_filter, flags
    sel = (C.c_int32 * max(K, 1))()
    p._keep = sel
    p.selected_subcarriers = C.addressof(sel)
    return p


def lds_rule(bs, ue, P, side):
    """(waves per workgroup, subcarrier chunk) of the launcher, restated: one wave holds both array tables, T, Q and a
    chunk of g, (M_out + M_avg + M_out + P + kc) * P * 8 bytes; 4 / 2 / 1 waves per workgroup while 4 x / 2 x fit 64 KB /
    one fits 156 KB; kc = the largest of 64, 32, 16, 8 that costs no wave against kc = 8."""
    m_tx, m_rx = bs[0] * bs[1], ue[0] * ue[1]
    rows = m_tx + m_rx + (m_tx if side == TX else m_rx) + P

    def waves(kc):
        b = (rows + kc) * P * 8
        return 4 if 4 * b <= 65536 else 2 if 2 * b <= 65536 else 1 if b <= LDS_MAX else 0
    best = waves(8)
    for kc in (64, 32, 16):
        if best and waves(kc) == best:
            return best, kc
    return best, 8


def test_header_binding_and_library_name_the_new_entry_points():
    from deepmimo_amd import _native as n
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    for sym in ("dmx_covariance_supported", "dmx_channel_covariance"):
        assert re.search(r"\b%s\(" % sym, hdr) and sym in n.EXPORTED_SYMBOLS
    flat = re.sub(r"[ \t]+", " ", hdr)
    assert "#define DMX_COV_TX 0" in flat and "#define DMX_COV_RX 1" in flat
    assert "Q[l,l']" in hdr and "S[l,l']" in hdr and "D[l,l']" in hdr           # the definition is spelled out
    assert n.ABI_VERSION == 3 and "#define DMX_ABI_VERSION 3" in flat
    assert n.COV_SIDES == {"tx": TX, "rx": RX}


@needs_lib
def test_library_exports_the_symbols_with_abi_3():
    from deepmimo_amd import _native as n
    lib = n.load()
    assert lib.dmx_version() == 3
    for sym in ("dmx_covariance_supported", "dmx_channel_covariance"):
        assert getattr(lib, sym) is not None


@needs_lib
def test_supported_shapes_without_a_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    q = lambda p, side=TX, L=25: lib.dmx_covariance_supported(C.byref(p), L, side)    # noqa: E731
    for side in (TX, RX):
        assert q(_params(), side) == 1                                        # DeepMIMO's defaults
        assert q(_params(K=512), side) == 1
        assert q(_params((8, 8), (2, 2), 512), side) == 1                     # the headline panel (64 x 4), 25 paths
        assert q(_params((64, 1), (4, 1), 74), side) == 1
        assert q(_params((32, 32), (1, 1), 2), side) == 0 and "LDS" in err()  # a too-large panel: refused on both sides
        assert q(_params(num_paths=33), side, 40) == 0 and "32" in err()      # P = 33
        assert q(_params(num_paths=32), side, 40) == 1
        assert q(_params(num_paths=40), side, 32) == 1                        # num_paths above the loaded count
        assert q(_params(freq_domain=0), side) == 0 and "freq_domain" in err()
        assert q(_params(rx_filter=1), side) == 0 and "rx_filter" in err()
        assert q(_params(K=0), side) == 0 and q(_params(), side, 0) == 0 and q(_params(num_paths=0), side) == 0
        assert q(_params(flags=n.FLAG_ADAPTIVE_TERMS), side) == 1             # either arithmetic mode
    for bad in (-1, 2, 7):
        assert q(_params(), bad) == -1 and "side" in err()
    assert q(_params(), TX, -1) == -1
    assert lib.dmx_covariance_supported(None, 25, TX) == -1 and "params is NULL" in err()
    # the edge of the byte rule at 25 paths: 2 M_out + M_avg <= 765
    assert q(_params((382, 1), (1, 1))) == 1 and q(_params((383, 1), (1, 1))) == 0
    assert "160000 bytes" in err() and str(LDS_MAX) in err()
    assert q(_params((382, 1), (1, 1)), RX) == 1 and q(_params((763, 1), (1, 1)), RX) == 1 and q(_params((764, 1), (1, 1)), RX) == 0


@needs_lib
def test_supported_equals_the_lds_rule():
    from deepmimo_amd import _native as n
    lib = n.load()
    rng = np.random.default_rng(13)
    seen = {0: 0, 1: 0, 2: 0, 4: 0}
    for _ in range(4000):
        bs = (int(rng.integers(1, 65)), int(rng.integers(1, 17)))
        ue = (int(rng.integers(1, 9)), int(rng.integers(1, 5)))
        L, num_paths, side = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(0, 2))
        P = min(L, num_paths)
        want = lds_rule(bs, ue, P, side)[0] if 1 <= P <= 32 else 0
        seen[want] += 1
        got = lib.dmx_covariance_supported(C.byref(_params(bs, ue, 3, num_paths)), L, side)
        assert got == (1 if want else 0), (bs, ue, num_paths, L, side, want, got)
    assert all(v > 50 for v in seen.values()), seen
    # the shapes the GPU tests rely on for 4 / 2 / 1 waves per workgroup and for the chunk size
    assert lds_rule((8, 1), (1, 1), 25, TX) == (4, 32) and lds_rule((8, 1), (1, 1), 25, RX) == (4, 32)
    assert lds_rule((8, 8), (2, 2), 25, TX) == (1, 64) and lds_rule((8, 8), (2, 2), 25, RX)[0] == 2
    assert lds_rule((8, 4), (2, 2), 25, TX)[0] == 2


@needs_lib
def test_argument_errors_without_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    buf = (C.c_char * 65536)()
    base = (C.addressof(buf) + 255) // 256 * 256
    ws, out = C.c_void_p(base), C.c_void_p(base + 4096)
    call = lambda p, b=0, cnt=4, side=TX, o=out, L=25: lib.dmx_channel_covariance(C.byref(p), ws, 4, L, b, cnt, side, o, None)   # noqa: E731
    assert call(_params(freq_domain=0)) == -1 and "freq_domain" in err()
    assert call(_params(rx_filter=1)) == -1 and "rx_filter" in err()
    for bad in (-1, 2):
        assert call(_params(), side=bad) == -1 and "side" in err()
    assert call(_params(), b=2, cnt=4) == -1 and "user range" in err()
    assert call(_params(), o=None) == -1 and "NULL" in err()
    assert call(_params(), o=C.c_void_p(base + 4100)) == -1 and "8-byte aligned" in err()
    assert call(_params((32, 32), (1, 1), 2)) == -2 and "LDS" in err()
    assert call(_params(num_paths=33), L=40) == -2 and "32" in err()
    assert call(_params(K=0)) == -2
    assert call(_params(), cnt=0) == 0                                        # nothing to do: success before any GPU call


def _dataset(n=5, L=25):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=2)
    return dm, dm.Dataset({k: v.copy() for k, v in rays.items()})


@needs_lib
def test_dataset_errors_come_before_any_gpu_call(monkeypatch):
    from deepmimo_amd import dataset as dsm
    dm, ds = _dataset()

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)
    for bad in ("bs", "TX", 0, None):
        with pytest.raises(ValueError, match="side"):
            ds.compute_covariance(dm.ChannelGenParameters(), side=bad)
    p = dm.ChannelGenParameters()
    p.freq_domain = 0
    with pytest.raises(ValueError, match="freq_domain"):
        ds.compute_covariance(p)
    p = dm.ChannelGenParameters()
    p.ofdm.rx_filter = 1
    with pytest.raises(ValueError, match="rx_filter"):
        ds.compute_covariance(p, side="rx")
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape = np.array([32, 32])
    with pytest.raises(ValueError, match=r"LDS"):
        ds.compute_covariance(p)
    _, ds40 = _dataset(L=40)
    p = dm.ChannelGenParameters()
    p.num_paths = 33
    with pytest.raises(ValueError, match=r"1\.\.32 paths"):
        ds40.compute_covariance(p)


@needs_lib
def test_valid_call_without_a_gpu_raises_the_usual_error(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    dm, ds = _dataset()
    for side in SIDES:
        with pytest.raises(RuntimeError, match="no GPU"):
            ds.compute_covariance(dm.ChannelGenParameters(), side=side)
    assert "compute_covariance" in dm.MacroDataset.PROPAGATE_METHODS


# the six configurations of the identity check: (bs, ue, N, selection, loaded paths)
IDENTITY_CONFIGS = {
    "defaults_K1": ([8, 1], [1, 1], 512, [0], 25),
    "defaults_K512": ([8, 1], [1, 1], 512, list(range(512)), 25),
    "panel_stride7": ([8, 8], [2, 2], 512, list(range(0, 512, 7)), 25),
    "paths7": ([4, 2], [2, 1], 64, list(range(64)), 7),
    "paths32": ([4, 4], [1, 2], 256, list(range(0, 256, 5)), 32),
    "irregular": ([4, 2], [2, 1], 512, [-3, 0, 5, 511, 512, 700, -1000, 77, 78, 300], 25),
}


@pytest.mark.parametrize("name", sorted(IDENTITY_CONFIGS))
def test_closed_form_equals_the_definition_in_float64(name):
    """The reference of the GPU tests is the einsum of the oracle's H; the kernel evaluates the closed form.  The two agree
    within 5e-7 of each user's largest |R| entry: the complex64 rounding of the oracle's H (1.1e-7 measured) with a 4x
    margin."""
    from oracle import oracle_np as onp
    bs, ue, N, sel, L = IDENTITY_CONFIGS[name]
    rays = onp.synth_rays(40, L, seed=31 + L)
    op = onp.make_params(bs_antenna=dict(shape=bs, rotation=np.array([10, -20, 30])), ue_antenna=dict(shape=ue), num_paths=L,
                         ofdm=dict(subcarriers=N, selected_subcarriers=np.array(sel)))
    H = onp.compute_channels(rays, op)["channel"]
    worst = 0.0
    for side in SIDES:
        ref = cov_from_channel(H, side)
        d, peak = cov_err(cov_closed_form(rays, op, side), ref)
        assert np.all(d[peak == 0] == 0)
        worst = max(worst, float(np.max(d / np.maximum(peak, 1e-300))))
    print(f"{name}: closed form against the definition, worst {worst:.3e} of the user's peak")
    assert worst <= 5e-7


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(isa_lint.OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_kernel_instantiations_and_no_scratch(tmp_path):
    """Both sides' instantiations are in the code object, with no scratch access, no spill and no private segment."""
    ks = {isa_lint.short_name(k): v for k, v in isa_lint.kernels_of_library(LIB).items()}
    want = ["k6_covariance<0>", "k6_covariance<1>"]
    assert sorted(k for k in ks if k.startswith("k6_covariance")) == want
    for name in want:
        assert not [i.mnem for i in ks[name] if i.mnem.startswith("scratch_")], name
    info = {}
    for co in isa_lint.extract_code_objects(LIB, str(tmp_path)):
        info.update(_notes(co))
    mine = {k: v for k, v in info.items() if "k6_covariance" in k}
    assert len(mine) == 2
    for k, v in mine.items():
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)


def test_kernel_source_has_a_flat_grid_and_shares_the_headers():
    src = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k6_covariance.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "gridDim" not in code and "__syncthreads" not in code and "atomic" not in code
    assert '#include "k2_small_body.h"' in code and '#include "dmx_common.h"' in code
    assert "wave_lds_fence" in code and "sincos_rev" in code and "launch_dyn_lds" in code and "lds_waves_per_block" in code
