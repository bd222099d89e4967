"""Angle-delay representation (dmx_channels_angle_delay, k9_angle_delay.hip): everything that can be held without a GPU - the
header and the binding, the closed form against the definition, dm.dft_codebook, the host-only shape query and the argument
checks of the engine and the Dataset, and the two conditions under which the GPU test's criterion means something: the
summation error a user's amplification admits stays within half the bound, and a wrong path moves the reference by
at least twice the bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._angle_delay_cases import BY_ID, CASES, LDS_MAX, RC, TAP_CHUNK, case_codebook, case_inputs, lds_rule, on_tap_delays
from tests._angle_delay_ref import (adp_from_channel, amplification, delay_kernel, dft_codebook, drop_delta, swap_delta,
                                    uniform)
from tests._cases import TOL_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepmimo_amd", "lib", "libdeepmimo_amd.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

SYMBOLS = ("dmx_angle_delay_supported", "dmx_channels_angle_delay")


def _params(bs=(8, 1), ue=(1, 1), K=64, num_paths=25, freq_domain=1, rx_filter=0, flags=0, first=0, stride=1):
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = num_paths, freq_domain, 512, K, 10e6
    p.rx_filter, p.flags, p.sc_first, p.sc_stride = rx_filter, flags, first, stride
    sel = (C.c_int32 * max(K, 1))()
    p._keep = sel
    p.selected_subcarriers = C.addressof(sel)
    return p


def _rows(c):
    F = case_codebook(c)
    return c["bs_shape"][0] * c["bs_shape"][1] if F is None else len(F)


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_new_entry_points():
    from deepmimo_amd import _native as n
    hdr = open(os.path.join(ROOT, "include", "deepmimo_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, hdr) and sym in n.EXPORTED_SYMBOLS
    flat = re.sub(r"[ \t]+", " ", hdr)
    assert n.ABI_VERSION == 3 and "#define DMX_ABI_VERSION 3" in flat
    assert "(M_rx + min(n_rows, 32) + tc) * P * 8" in hdr and "159744" in hdr        # the header states the LDS formula
    assert "sin(pi K r) / sin(pi r)" in hdr                                            # and the delay kernel
    assert RC == 32 and TAP_CHUNK == 64 and LDS_MAX == 159744


@needs_lib
def test_library_exports_the_symbols_with_abi_3():
    from deepmimo_amd import _native as n
    lib = n.load()
    assert lib.dmx_version() == 3
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None


def test_kernel_source_has_a_flat_grid_and_shares_the_body():
    src = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k9_angle_delay.hip")).read()
    assert '#include "k7_rate_body.h"' in src and "rows_pair<M>" in src
    body = open(os.path.join(ROOT, "deepmimo_amd", "csrc", "k7_rate_body.h")).read()
    assert src.count("fill_array_table(") == 2 and src.count("copy_rows_to_lds(") == 1 and src.count("kept_paths(") == 1
    assert "void fill_array_table(" in body and "void copy_rows_to_lds(" in body and "frac_rev" in body and "frac_rev" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())                 # comments say what it does not do
    assert "__syncthreads" not in code and "atomic" not in code.lower() and "blockIdx.y" not in code
    assert "k9_angle_delay.hip" in open(os.path.join(ROOT, "deepmimo_amd", "csrc", "Makefile")).read()


# ---- the closed form ------------------------------------------------------------------------------------------------------
def test_delay_kernel_is_the_inverse_dft_of_a_single_path():
    rng = np.random.default_rng(3)
    for s0, d, K, N, n_fft, T in ((0, 1, 512, 512, 512, 32), (3, 8, 40, 512, 64, 24), (-5, 1, 64, 512, 64, 64), (40001, 2, 65, 512, 128, 128),
                                  (7, 1, 1, 512, 1, 1)):
        dn = np.concatenate([rng.uniform(0, 60, 6), [0.0, 5.0, 31.0, 5.5, float(np.nextafter(np.float32(5), np.float32(6)))]])
        k = s0 + d * np.arange(K)
        g = np.exp(-2j * np.pi * np.outer(dn, k) / N)
        want = np.fft.ifft(g, n=n_fft, axis=-1)[:, :T]
        got = delay_kernel(dn, s0, d, K, N, n_fft, T)
        assert np.abs(got - want).max() <= 1e-12 * K / n_fft * max(1, abs(s0)), (s0, d, K, np.abs(got - want).max())
    # exactly on a tap the whole K / n_fft lands there and nowhere else on the full grid
    D = delay_kernel([5.0], 0, 1, 512, 512, 512, 512)
    assert abs(D[0, 5] - 1.0) < 1e-15 and np.abs(np.delete(D[0], 5)).max() < 1e-13


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_closed_form_equals_the_definition_on_the_oracles_tensor(c):
    """within 1e-2 of the GPU bound: the difference is the complex64 rounding of the oracle's H (measured: at most 4.8e-3 of it)"""
    _, _, _, X_ref, X_cf, facs = case_inputs(c)
    assert X_ref.shape == X_cf.shape == (c["n"], c["ue_shape"][0] * c["ue_shape"][1], _rows(c), c["n_taps"])
    peak = np.abs(X_ref).reshape(c["n"], -1).max(axis=1)
    err = np.abs(X_cf - X_ref).reshape(c["n"], -1).max(axis=1)
    dead = np.array([f is None for f in facs])
    assert (peak[dead] == 0).all() and (peak[~dead] > 0).all()
    worst = float((err[~dead] / (TOL_REL * peak[~dead])).max()) if (~dead).any() else 0.0
    print(f"{c['id']}: closed form - definition = {worst:.2e} of the bound")
    assert worst <= 1e-2


def test_case_table_reaches_the_branches_it_names():
    rule = lambda cid: lds_rule(BY_ID[cid]["ue_shape"], _rows(BY_ID[cid]), BY_ID[cid]["n_taps"],      # noqa: E731
                                min(BY_ID[cid]["num_paths"], BY_ID[cid]["L"]))
    assert rule("wpb4_users41") == 4 and rule("wpb4_users43") == 4 and rule("defaults_K512_dft") == 4
    assert rule("wpb2_users7") == 2
    # the rule has no one-wave shape: its largest tables are two waves per workgroup
    assert lds_rule([4, 2], 10 ** 6, 2 ** 20, 32) == 2 and (8 + RC + TAP_CHUNK) * 32 * 8 == 26624
    assert {_rows(BY_ID[f"rows{R}"]) for R in (1, 3, 31, 32, 33, 65)} == {1, 3, RC - 1, RC, RC + 1, 2 * RC + 1}
    assert _rows(BY_ID["ant_8x8"]) == 64 and BY_ID["taps65_dft"]["n_taps"] == TAP_CHUNK + 1
    # every M_rx the kernel is instantiated for; antenna rows of an odd panel; every kept-path count
    assert {c["ue_shape"][0] * c["ue_shape"][1] for c in CASES} == set(range(1, 9))
    assert [BY_ID[f"mrx{m}"]["ue_shape"] for m in (5, 6, 7)] == [[5, 1], [3, 2], [7, 1]] and rule("mrx7") == 4
    assert _rows(BY_ID["ant_5x3"]) == 15 and BY_ID["ant_5x3"]["rows"] == "ant" and BY_ID["ant_5x3"]["ue_shape"] == [3, 2]
    ec = BY_ID["every_count_ant"]
    assert np.isfinite(case_inputs(ec)[0]["power"]).sum(axis=1).tolist() == [u % 33 for u in range(ec["n"])] and rule("every_count_ant") == 4
    assert uniform(BY_ID["pad_K40_d8_s3_dft"]["selected"]) == (3, 8, 40) and uniform(BY_ID["taps1_ant"]["selected"]) == (7, 1, 1)
    d = on_tap_delays()
    assert d.dtype == np.float32 and d[3, 0] > 5 > d[4, 0] and float(d[3, 0]) - 5 == 2.0 ** -21 and 5 - float(d[4, 0]) == 2.0 ** -21
    # x of those two paths is 2^-30, where the kernel's limit sets in; every on-tap delay reaches the records exactly
    rays = case_inputs(BY_ID["on_tap_dft"])[0]
    assert np.array_equal(rays["delay"] / (1 / BY_ID["on_tap_dft"]["bandwidth"]), d)


# ---- dm.dft_codebook ------------------------------------------------------------------------------------------------------
def test_dft_codebook_is_unitary_and_peaks_at_the_beam_of_an_on_grid_wave():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    for shape in ([8, 1], [4, 2], [1, 4], [8, 4], [3, 5], [1, 1]):
        F = dm.dft_codebook(shape)
        M = shape[0] * shape[1]
        assert F.dtype == np.complex64 and F.shape == (M, M)
        assert np.abs(F.astype(np.complex128) @ F.astype(np.complex128).conj().T - np.eye(M)).max() < 4e-7
        assert np.abs(F - dft_codebook(shape)).max() < 1.5e-7
        # a plane wave whose phase steps are by / Mh and bz / Mv revolutions lands in beam (by, bz) alone
        mh, mv = shape
        for by, bz in ((0, 0), (mh - 1, mv - 1), (mh // 2, mv // 3)):
            m = np.arange(M)
            a = np.exp(2j * np.pi * ((m % mh) * by / mh + (m // mh) * bz / mv))
            y = np.abs(F @ a)
            assert np.argmax(y) == by + mh * bz and abs(y.max() - np.sqrt(M)) < 1e-5 and np.delete(y, by + mh * bz).max(initial=0) < 1e-5
    # broadside in the element order of the array response (geometry.py): theta = 90, phi = 0 -> every element in phase
    a = onp.array_response_batch([4, 2], 0.5, np.array([[90.0]]), np.array([[0.0]]))[0, :, 0]
    assert np.argmax(np.abs(dm.dft_codebook([4, 2]) @ a)) == 0
    with pytest.raises(ValueError):
        dm.dft_codebook([0, 2])


# ---- the host-only query --------------------------------------------------------------------------------------------------
@needs_lib
def test_supported_shapes_without_a_gpu():
    from deepmimo_amd import _native as n
    lib = n.load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    q = lambda p, R=8, n_fft=64, T=32, L=25: lib.dmx_angle_delay_supported(C.byref(p), L, R, n_fft, T)   # noqa: E731
    for c in CASES:                                                           # every listed case is taken
        s0, d, K = uniform(c["selected"])
        p = _params(c["bs_shape"], c["ue_shape"], K, c["num_paths"], first=s0, stride=d)
        assert q(p, _rows(c), c["n_fft"], c["n_taps"], c["L"]) == 1, (c["id"], err())
    assert q(_params((64, 4), (2, 2), 512), 256, 512, 32) == 1                # the headline panel, all DFT rows
    # the largest tables the rule can see, (8 + 32 + 64) * 32 * 8 = 26624 bytes, are taken; what lies beyond them is refused
    # by the limit of the array or of the path count, each named
    assert q(_params((32, 32), (4, 2), 512, 32), 1024, 2 ** 20, 2 ** 20, 32) == 1
    assert q(_params(ue=(3, 3))) == 0 and "8 UE elements" in err()            # M_rx = 9
    assert q(_params(num_paths=33), L=40) == 0 and "1..32 paths" in err()     # P = 33
    assert q(_params(num_paths=32), L=40) == 1 and q(_params(num_paths=40), L=32) == 1
    assert q(_params(K=65), n_fft=64) == 0 and "n_fft = 64" in err() and "65" in err()         # n_fft < K
    assert q(_params(), n_fft=2 ** 20 + 1) == 0 and "1048576" in err()
    assert q(_params(), n_fft=2 ** 20, T=2 ** 20) == 1
    assert q(_params(), T=65) == 0 and "n_taps = 65" in err() and "n_fft = 64" in err()         # n_taps > n_fft
    assert q(_params(), T=0) == 0 and "n_taps = 0" in err()
    assert q(_params(stride=0)) == 0 and "sc_stride > 0" in err()             # no spacing promise
    assert q(_params(K=1), n_fft=1, T=1) == 1                                 # a single subcarrier counts
    assert q(_params(), R=0) == 0 and "n_rows" in err()
    assert q(_params(K=0)) == 0 and q(_params(), L=0) == 0
    assert q(_params(freq_domain=0)) == 0 and "freq_domain" in err()
    assert q(_params(rx_filter=1)) == 0 and "rx_filter" in err()
    assert q(_params(flags=n.FLAG_ADAPTIVE_TERMS)) == 1                       # either arithmetic mode
    assert q(_params(first=-(2 ** 31))) == 1 and q(_params(first=40001, stride=8)) == 1
    assert q(_params(), L=-1) == -1
    assert lib.dmx_angle_delay_supported(None, 25, 8, 64, 32) == -1 and "params is NULL" in err()


@needs_lib
def test_supported_equals_the_restated_rule():
    lib = __import__("deepmimo_amd._native", fromlist=["load"]).load()
    rng = np.random.default_rng(17)
    seen = {0: 0, 2: 0, 4: 0}
    for _ in range(3000):
        ue = (int(rng.integers(1, 6)), int(rng.integers(1, 3)))
        L, num_paths = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        R, T = int(rng.integers(1, 80)), int(rng.integers(1, 100))
        P = min(L, num_paths)
        want = lds_rule(ue, R, T, P) if 1 <= P <= 32 and ue[0] * ue[1] <= 8 else 0
        seen[want] += 1
        got = lib.dmx_angle_delay_supported(C.byref(_params((4, 2), ue, 64, num_paths)), L, R, 128, T)
        assert got == (1 if want else 0), (ue, R, T, num_paths, L, want, got)
    assert all(v > 20 for v in seen.values()), seen


@needs_lib
def test_argument_errors_without_gpu():
    lib = __import__("deepmimo_amd._native", fromlist=["load"]).load()
    err = lambda: lib.dmx_last_error().decode()                               # noqa: E731
    buf = (C.c_char * 65536)()
    base = (C.addressof(buf) + 255) // 256 * 256
    ws, out, cb = C.c_void_p(base), C.c_void_p(base + 4096), C.c_void_p(base + 8192)

    def call(p, b=0, cnt=4, F=None, R=8, bws=None, nb=0, n_fft=64, T=32, o=out, L=25):
        return lib.dmx_channels_angle_delay(C.byref(p), ws, 4, L, b, cnt, F, R, bws, nb, n_fft, T, o, None)
    assert call(_params(freq_domain=0)) == -1 and "freq_domain" in err()
    assert call(_params(rx_filter=1)) == -1 and "rx_filter" in err()
    assert call(_params(stride=0)) == -1 and "sc_stride" in err()
    assert call(_params(), R=5) == -1 and "8 BS elements" in err()            # no codebook: the rows are the elements
    assert call(_params(), b=2, cnt=4) == -1 and "user range" in err()
    assert call(_params(), o=None) == -1 and "NULL" in err()
    assert call(_params(), o=C.c_void_p(base + 4098)) == -1 and "8-byte aligned" in err()
    assert call(_params(ue=(3, 3))) == -2 and "8 UE elements" in err()
    assert call(_params(num_paths=33), L=40) == -2 and "32" in err()
    assert call(_params(K=65)) == -2 and "n_fft" in err()
    assert call(_params(), T=65) == -2 and "n_taps" in err()
    assert call(_params(), T=0) == -2 and "n_taps" in err()
    assert call(_params(), F=cb, R=3) == -4 and "beam workspace" in err()     # a codebook needs its workspace
    assert call(_params(), cnt=0) == 0 and call(_params(), F=cb, R=3, cnt=0) == 0      # nothing to do: success before any GPU call


def _dataset(n=5, L=25):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=2)
    return dm, dm.Dataset({k: v.copy() for k, v in rays.items()})


@needs_lib
def test_check_call_and_dataset_errors_come_before_any_gpu_call(monkeypatch):
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd.engine import check_angle_delay_call
    dm, ds = _dataset()

    def no_engine():
        raise AssertionError("the GPU engine was asked for before the argument checks")
    monkeypatch.setattr(dsm, "_engine", no_engine)

    def prm(**kw):
        p = dm.ChannelGenParameters()
        p.ofdm.selected_subcarriers = np.arange(64)
        for k, v in kw.items():
            setattr(p.ofdm, k, v)
        return p
    ok = prm().validate(5)
    assert check_angle_delay_call(ok, 25, 8, None, 32) == 64 and check_angle_delay_call(ok, 25, 8, 128, 128) == 128

    def refused(p, match, n_fft=None, n_taps=32, n_rows=8, **kw):
        with pytest.raises(ValueError, match=match):
            check_angle_delay_call(p.validate(5), 25, n_rows, n_fft, n_taps)
        with pytest.raises(ValueError, match=match):
            ds.compute_angle_delay(p, n_taps=n_taps, n_fft=n_fft, **kw)
    refused(prm(selected_subcarriers=np.array([0, 1, 3])), "uniformly spaced")
    refused(prm(selected_subcarriers=np.array([5, 3, 1])), "uniformly spaced")
    refused(prm(rx_filter=1), "rx_filter")
    p = prm()
    p.freq_domain = 0
    refused(p, "freq_domain")
    refused(prm(), r"n_taps = 0", n_taps=0)
    refused(prm(), r"n_taps = 65", n_taps=65)
    refused(prm(), r"n_fft = 63", n_fft=63)
    refused(prm(), "n_taps must be an integer", n_taps=3.5)
    refused(prm(), "n_fft must be an integer", n_fft="64")
    p = prm()
    p.ue_antenna.shape = np.array([3, 3])
    refused(p, "8 UE elements")
    _, ds40 = _dataset(L=40)
    p = prm()
    p.num_paths = 33
    with pytest.raises(ValueError, match=r"1\.\.32 paths"):
        ds40.compute_angle_delay(p, n_taps=8)
    with pytest.raises(ValueError, match="n_taps"):                           # missing
        ds.compute_angle_delay(prm())
    with pytest.raises(TypeError):                                            # keyword-only
        ds.compute_angle_delay(prm(), 32)
    with pytest.raises(ValueError, match=r"\[R, 8\]"):                        # a codebook of the wrong width
        ds.compute_angle_delay(prm(), n_taps=32, codebook=np.ones((4, 7), np.complex64))
    with pytest.raises(ValueError, match="'dft'"):
        ds.compute_angle_delay(prm(), n_taps=32, codebook="hadamard")
    assert "compute_angle_delay" in dm.MacroDataset.PROPAGATE_METHODS


@needs_lib
def test_valid_call_without_a_gpu_raises_the_usual_error(monkeypatch):
    """After the host checks the call asks for the engine, which raises where no GPU is visible (no CPU fallback)."""
    import torch
    from deepmimo_amd import dataset as dsm
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dsm, "_engines", {})
    dm, ds = _dataset()
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(64)
    for cb in ("dft", None):
        with pytest.raises(RuntimeError, match="no GPU"):
            ds.compute_angle_delay(p, n_taps=32, codebook=cb)


# ---- what the GPU criterion rests on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_bound_precondition_of_every_gpu_case(c):
    """The criterion max |X - X_ref[u]| <= TOL_REL max |X_ref[u]| is valid for a user only if
        A[u] = max over entries of sum_l |term_l| / max |X_ref[u]|  <=  TOL_REL / (2 (P + 8) 2^-24):
    at that limit the fp32 summation error - P path terms, each through a handful of rounded products - is at most half the
    bound.  12.7 at 25 paths, 10.5 at 32.  Every live user of every case, none left out."""
    _, _, _, X_ref, _, facs = case_inputs(c)
    P = min(c["num_paths"], c["L"])
    limit = TOL_REL / (2 * (P + 8) * 2.0 ** -24)
    A = np.array([amplification(f, X_ref[u]) for u, f in enumerate(facs) if f is not None])
    assert len(A) >= 1
    print(f"{c['id']}: amplification <= {A.max():.2f} (limit {limit:.1f}, {len(A)} live users)")
    assert abs(TOL_REL / (2 * 33 * 2.0 ** -24) - 12.7) < 0.05 and abs(TOL_REL / (2 * 40 * 2.0 ** -24) - 10.5) < 0.05
    assert (A <= limit).all(), f"{c['id']}: amplification {A.max():.2f} above {limit:.2f}"


@pytest.mark.parametrize("cid", ["equal_power_dft", "equal_power_ant"])
def test_a_wrong_path_moves_the_reference_by_twice_the_bound(cid):
    """equal-power paths whose delays the tap window covers (d dn n_fft / N < n_taps - 2): dropping any one kept path, or
    exchanging the D rows of two neighbouring paths, moves X_ref by at least twice the user's bound"""
    c = BY_ID[cid]
    rays, _, _, X_ref, _, facs = case_inputs(c)
    s0, d, K = uniform(c["selected"])
    dn = rays["delay"].astype(np.float64) * c["bandwidth"]
    assert np.nanmax(d * dn * c["n_fft"] / c["subcarriers"]) < c["n_taps"] - 2            # the coverage condition
    pw = rays["power"][np.isfinite(rays["power"])]
    assert pw.min() >= -66 and pw.max() <= -60
    worst_drop = worst_swap = np.inf
    for u, f in enumerate(facs):
        bound = TOL_REL * np.abs(X_ref[u]).max()
        n = len(f[2])
        assert n == c["L"]
        for l in range(n):
            worst_drop = min(worst_drop, np.abs(drop_delta(f, l)).max() / bound)
        for l in range(n - 1):
            worst_swap = min(worst_swap, np.abs(swap_delta(f, l)).max() / bound)
    print(f"{cid}: a dropped path moves X_ref by >= {worst_drop:.1f} x the bound, exchanged D rows by >= {worst_swap:.1f} x")
    assert worst_drop >= 2 and worst_swap >= 2


def test_window_that_misses_the_delays_is_far_less_sensitive():
    """why the coverage condition is part of the case: with delays up to 40 samples and 32 taps of a 512-point grid a path
    behind the window leaves only its sidelobes, and dropping it moves X_ref by 11 x the bound on these inputs - two hundred
    times less than the 2239 x of the covered window"""
    c = dict(BY_ID["equal_power_dft"], id="equal_power_uncovered", max_delay=2e-6)
    rays, _, _, X_ref, _, facs = case_inputs(c)
    assert np.nanmax(rays["delay"].astype(np.float64) * c["bandwidth"]) > c["n_taps"]          # some paths lie behind the window
    worst = min(np.abs(drop_delta(f, l)).max() / (TOL_REL * np.abs(X_ref[u]).max()) for u, f in enumerate(facs)
                for l in range(len(f[2])))
    print(f"uncovered window: a dropped path moves X_ref by >= {worst:.2f} x the bound")
    assert worst < 100


def test_definition_helper_pads_and_truncates():
    rng = np.random.default_rng(1)
    H = rng.normal(size=(2, 1, 3, 5)) + 1j * rng.normal(size=(2, 1, 3, 5))
    F = rng.normal(size=(2, 3)) + 1j * rng.normal(size=(2, 3))
    X = adp_from_channel(H, F, 8, 4)
    t, k = np.arange(4)[:, None], np.arange(5)[None, :]
    want = np.einsum("bt,urtk,sk->urbs", F, H, np.exp(2j * np.pi * t * k / 8)) / 8
    assert X.shape == (2, 1, 2, 4) and np.abs(X - want).max() < 1e-14
    assert np.abs(adp_from_channel(H, None, 5, 5) - np.fft.ifft(H, axis=-1)).max() == 0
