"""The table of tests/_entry_calls.py against the header, the kernel files and the host-only launch rules (no GPU).

The two GPU files that run the table (tests/test_gpu_stream_order.py, tests/test_gpu_graph_capture.py) prove the stream and
graph contract of INTEGRATION.md section 3 only for what the table names.  Here: the table names every C-ABI function that
takes a stream and every `__global__` kernel, each case's kernel claim equals what the host-only rule of its route gives
(dmx_fd_kernel_choice, the dmx_*_supported queries, the restated launch rules of tests/_lpf_routes.py, tests/_beam_cases.py
and tests/_td_cases.py), the cases have the sizes the GPU files rely on, and every kernel launch of the library goes through
the one function that takes the caller's stream.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from tests import _beam_cases as B
from tests import _entry_calls as E
from tests import _lpf_routes as R
from tests._td_cases import td_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepmimo_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_stream_functions(text):
    """the dmx_* functions whose declaration has a `void* stream` parameter"""
    decls = re.findall(r"\b(dmx_\w+)\s*\(([^;{}()]*)\)\s*;", _no_comments(text))
    return {name for name, args in decls if re.search(r"\bvoid\s*\*\s*stream\b", args)}


def global_kernels():
    """{kernel name: file} of every `__global__` function of csrc/*.hip"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            for name in re.findall(r"__global__[^;{()]*?(?:__launch_bounds__\([^)]*\))?[^;{()]*?\bvoid\s+(\w+)\s*\(", _no_comments(f.read())):
                found[name] = os.path.basename(path)
    return found


def test_the_parsers_see_what_the_files_hold():
    fns = header_stream_functions(_read("include", "deepmimo_amd.h"))
    assert {"dmx_path_prep", "dmx_channels_fd", "dmx_pathloss", "dmx_mats_to_device", "dmx_codebook_rate_subbands"} <= fns
    assert not {"dmx_version", "dmx_fd_kernel_choice", "dmx_rate_supported", "dmx_mat5_find", "dmx_p2m_parse_paths"} & fns
    assert len(fns) == _no_comments(_read("include", "deepmimo_amd.h")).count("void* stream") == 18
    kernels = global_kernels()
    assert kernels["k2_fd_mfma"] == "k2_channel_fd_mfma.hip" and kernels["k_mat_to_rowmajor"] == "mat5_loader.hip"
    n_global = sum(_no_comments(_read("deepmimo_amd", "csrc", f)).count("__global__") for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert len(kernels) == n_global == 24


def test_the_table_names_every_function_that_takes_a_stream():
    assert {c.abi for c in E.CASES} == header_stream_functions(_read("include", "deepmimo_amd.h"))


def test_every_kernel_is_claimed_by_some_case():
    claimed = {k for c in E.CASES for k in c.kernels}
    assert claimed == set(global_kernels()), (claimed ^ set(global_kernels()))


def test_ids_are_unique_and_only_the_file_reader_is_exempt_from_capture():
    assert len(E.BY_ID) == len(E.CASES)
    exempt = [c for c in E.CASES if not c.capturable]
    assert [c.abi for c in exempt] == ["dmx_mats_to_device"] and all(c.reason for c in exempt)
    assert E.BY_ID["mat_rowmajor"].capturable
    assert all(c.rule for c in E.CASES)


# ---- the kernel claims against the host-only rules -------------------------------------------------------------------------------
def _query(cd):
    """(dmx_params of a host-only query with the spacing promise, loaded paths)"""
    from deepmimo_amd import engine
    p, _ = engine._query_params("entry calls", E.dm_params(cd), promise_stride=True)
    return p, cd["L"]


def _lib():
    from deepmimo_amd import _native as nat
    return nat.load()


def _supported(query, cd, *ints):
    p, loaded = _query(cd)
    rc = getattr(_lib(), query)(C.byref(p), loaded, *[int(i) for i in ints])
    assert rc == 1, (query, rc, _lib().dmx_last_error())


def _shape(cd):
    m_rx, m_tx = cd["ue_shape"][0] * cd["ue_shape"][1], cd["bs_shape"][0] * cd["bs_shape"][1]
    return m_rx, m_tx, len(cd["selected"]), min(cd["num_paths"], cd["L"])


def stage1_kernel(prep):
    """stage1_form (k1_path_math.h) for the table's preparations: no FoV, isotropic patterns, so the full form runs exactly
    where the rotated angles and the powers are asked for (want_side = True)"""
    cd = prep["case"]
    assert cd["bs_fov"] is None and cd["ue_fov"] is None and cd["bs_pattern"] == cd["ue_pattern"] == "isotropic"
    return "k1_path_prep_full" if prep["want_side"] is True else "k1_path_prep"


FD_KERNELS = {1: "k2_fd_valu", 2: "k2_fd_mfma", 9: "k2_fd_small", 12: "k2_fd_fold"}
CONSUMER_KERNELS = {"covariance": "k6_covariance", "rate": "k7_rate", "spectrum": "k7_rate", "precoders": "k7_rate",
                    "cell_rate": "k8_cell_rate", "angle_delay": "k9_angle_delay"}


def _projection(cd, rows):
    m_rx, m_tx, K, P = _shape(cd)
    route = B.projection_route(m_tx, rows, P)
    assert route != "error"
    return "k2b_beam_project" if route == "scalar" else "k2b_beam_project_mfma"


def expected_kernels(case, built):
    """the kernels of "reprepare every preparation, then the call" by the host-only rule of the case's route"""
    route, preps = built["route"], built["preps"]
    ks = {stage1_kernel(p) for p in preps}
    cd = preps[0]["case"] if preps else None
    tag = route[0]
    if tag == "fd":
        m_rx, m_tx, K, P = _shape(cd)
        _, variant, auto = route
        if auto:
            p, loaded = _query(cd)
            assert _lib().dmx_fd_kernel_choice(C.byref(p), loaded) == variant, case.id
        ks.add(FD_KERNELS[variant])
        if P > 32:
            ks.add("k2_fd_valu")                                            # launch_extra_path_passes
    elif tag == "direct":
        p, loaded = _query(route[1])
        assert _lib().dmx_fd_direct_supported(C.byref(p), loaded) == 1 and _lib().dmx_fd_kernel_choice(C.byref(p), loaded) == 9
        ks.add("k12_fd_direct")
    elif tag == "lpf":
        m_rx, m_tx, K, P = _shape(cd)
        r = R.lpf_route(cd["subcarriers"], K, P)
        assert r != "refused"
        ks.add("k3_lpf_" + r)
        ks.add("k2_fd_mfma" if R.mfma_preferred(m_rx * m_tx, K) else "k2_fd_valu")
        if P > 32:
            ks.add("k2_fd_valu")
    elif tag == "beams":
        ks |= {_projection(cd, route[1]), "k2_fd_mfma"}
    elif tag == "beam_power":
        m_rx = _shape(cd)[0]
        assert B.power_geometry(m_rx, route[1], len(cd["selected"]))["fits"]
        ks |= {_projection(cd, route[1]), "k2c_beam_power"}
    elif tag == "td":
        m_rx, m_tx, K, P = _shape(cd)
        ks.add("k4_td" if td_form(m_rx, m_tx, P) == "plain" else "k4_td_tab")
    elif tag == "consumer":
        name = route[1]
        if name == "covariance":
            _supported("dmx_covariance_supported", cd, {"tx": 0, "rx": 1}[route[2]])
        elif name in ("rate", "spectrum"):
            _supported(f"dmx_{name}_supported", cd)
        elif name == "precoders":
            _supported("dmx_precoder_supported", cd, route[2])
        elif name == "cell_rate":
            from deepmimo_amd import engine
            assert len(preps) == 2
            engine.check_cell_rate_call([E.dm_params(p["case"]) for p in preps], [p["case"]["L"] for p in preps], [E.SNR_DB, E.SNR_DB])
        elif name == "angle_delay":
            n_rows, n_fft, n_taps = route[2:]
            _supported("dmx_angle_delay_supported", cd, _shape(cd)[1] if n_rows is None else n_rows, n_fft, n_taps)
            if n_rows is not None:
                ks.add(_projection(cd, n_rows))
        elif name == "codebook_rate":
            n_cw, n_layers, subband = route[2:]
            if subband is None:
                _supported("dmx_codebook_rate_supported", cd, n_cw, n_layers)
            else:
                _supported("dmx_codebook_rate_subbands_supported", cd, n_cw, n_layers, subband)
            ks |= {_projection(cd, n_cw * n_layers), "k10_codebook_rate" if subband is None else "k10_codebook_rate_sb"}
        if name in CONSUMER_KERNELS:
            ks.add(CONSUMER_KERNELS[name])
    elif tag == "pathloss":
        ks.add("k5_pathloss")
    elif tag == "loader":
        ks.add("k_mat_to_rowmajor")
    else:
        raise AssertionError(tag)
    return ks


@pytest.mark.parametrize("cid", [c.id for c in E.CASES])
def test_kernel_claim_equals_the_host_rule(cid):
    case = E.BY_ID[cid]
    assert set(case.kernels) == expected_kernels(case, case.build()), cid
    assert len(set(case.kernels)) == len(case.kernels)


def test_restated_stage1_rule_is_the_one_in_the_source():
    src = _read("deepmimo_amd", "csrc", "k1_path_math.h")
    assert "const bool lean = !stage1_need_angles(prm, side) && !side.power_linear && !side.power_linear_ant_gain && !side.fov_mask;" in src
    assert "return prm.fov_enabled || prm.bs_pattern != DMX_PATTERN_ISOTROPIC || prm.ue_pattern != DMX_PATTERN_ISOTROPIC ||" in src
    eng = _read("deepmimo_amd", "engine.py")
    assert 'if want_side is True:\n            for k in ("aod_el_rot", "aod_az_rot", "aoa_el_rot", "aoa_az_rot", "power_linear_ant_gain"):' in eng
    assert 'side["fov_mask"] = torch.empty((n, L), dtype=torch.uint8, device=dev) if fov_enabled else None' in eng


# ---- the coverage the GPU files rely on ------------------------------------------------------------------------------------------
def _routes(tag):
    return [(c, c.build()) for c in E.CASES if c.build()["route"][0] == tag]


def test_coverage_of_variants_routes_and_forms():
    fd = _routes("fd")
    assert {b["route"][1] for _, b in fd} == {1, 2, 9, 12}
    fold_pairs = {int(np.prod(b["preps"][0]["case"]["bs_shape"]) * np.prod(b["preps"][0]["case"]["ue_shape"]))
                  for _, b in fd if b["route"][1] == 12}
    assert min(fold_pairs) < E.FOLD_SHARED_FROM <= max(fold_pairs) <= E.FOLD_MAX_M          # one wave per item, and shared tables
    assert _routes("direct")
    lpf = {R.lpf_route(b["preps"][0]["case"]["subcarriers"], len(b["preps"][0]["case"]["selected"]), b["L"]) for _, b in _routes("lpf")}
    assert lpf == {"fft_pow2", "fft_wave", "fft", "gains"} >= {R.route_of(c) for c in R.CASES}    # every answer of lpf_route
    # the chain "gains kernel, then matrix-core kernel" over the packed and over the float table
    chains = {(R.table_packed(b["preps"][0]["case"]["subcarriers"], len(b["preps"][0]["case"]["selected"]), b["L"],
                              _shape(b["preps"][0]["case"])[0] * _shape(b["preps"][0]["case"])[1]), "k2_fd_mfma" in c.kernels)
              for c, b in _routes("lpf")}
    assert {(True, True), (False, True), (False, False)} <= chains
    for consumer in ("k2_fd_mfma", "k2c_beam_power", "k9_angle_delay", "k10_codebook_rate"):
        assert any(consumer in c.kernels and "k2b_beam_project_mfma" in c.kernels for c in E.CASES), consumer
    for consumer in ("k2_fd_mfma", "k2c_beam_power", "k10_codebook_rate"):
        assert any(consumer in c.kernels and "k2b_beam_project" in c.kernels for c in E.CASES), consumer
    assert {k for c, _ in _routes("td") for k in c.kernels} >= {"k4_td", "k4_td_tab"}
    assert any("k9_angle_delay" in c.kernels and not any(k.startswith("k2b") for k in c.kernels) for c in E.CASES)
    assert {"k10_codebook_rate", "k10_codebook_rate_sb"} <= {k for c in E.CASES for k in c.kernels}
    assert len(E.BY_ID["cell_rate_2"].build()["preps"]) == 2


def test_sizes_and_rays_of_every_case():
    for c in E.CASES:
        b = c.build()
        if b["kind"] != "rays":
            continue
        assert b["n"] <= 64 and all(b["n"] % w for w in (2, 4, 8)), c.id
        assert b["L"] in (E.L, E.L_EXTRA) and all(p["case"]["L"] == b["L"] for p in b["preps"]), c.id
        ra, rb = E.case_rays(b, "a"), E.case_rays(b, "b")
        for r in (ra, rb):
            assert all(r[k].shape == (b["n"], b["L"]) and r[k].dtype == np.float32 for k in E.RAY_KEYS), c.id
            counts = E.valid_counts(r)
            assert counts[E.NONE_USER] == 0 and (counts > 0).sum() >= b["n"] // 2, c.id
            if b["L"] == E.L_EXTRA:                                          # more than 32 kept paths: the extra passes have work
                assert (counts > 32).sum() >= 3, (c.id, counts)
            if b["preps"] and b["preps"][0]["case"]["rx_filter"]:
                dn = r["delay"][np.isfinite(r["delay"])] * E.BANDWIDTH
                assert dn.max() < b["preps"][0]["case"]["subcarriers"], c.id
        assert not np.array_equal(ra["power"], rb["power"], equal_nan=True)
    extra = [c.id for c in E.CASES if c.build()["L"] == E.L_EXTRA and c.build()["kind"] == "rays"]
    assert {"fd_extra_mfma", "fd_extra_small", "lpf_extra"} <= set(extra)


def test_lds_cap_pairs():
    """The three launchers that pass their request as the cap of the dynamic-LDS attribute: a pair of cases of the same
    instantiation, both above 64 KiB, the captured one larger - or the reason why there is none."""
    for kernel in E.LDS_CAP_PAIRS:
        src = _read("deepmimo_amd", "csrc", global_kernels()[kernel])
        assert re.search(r'launch_dyn_lds\((?:kernel|k3_lpf_fft_wave), "%s", [^;]*?\bsmem, (?:smem|\w+_LDS_CAP), stream' % kernel, src), kernel
    big, small = (E.BY_ID[i].build()["preps"][0]["case"] for i in E.LDS_CAP_PAIRS["k3_lpf_fft_wave"])
    for cd in (big, small):
        assert R.lpf_route(cd["subcarriers"], len(cd["selected"]), cd["L"]) == "fft_wave"
    assert R.wave_lds_bytes(big["subcarriers"]) == 155712 > R.wave_lds_bytes(small["subcarriers"]) == 77888 > E.LDS_DEFAULT
    rows = []
    for i in E.LDS_CAP_PAIRS["k2c_beam_power"]:
        b = E.BY_ID[i].build()
        rows.append(_shape(b["preps"][0]["case"])[0] * b["route"][1])
    assert B.LDS_CAP_BEAM_POWER >= B.beam_pow_lds_bytes(rows[0]) > B.beam_pow_lds_bytes(rows[1]) > E.LDS_DEFAULT
    # the folded kernel: no shape it takes asks for more than the default
    assert isinstance(E.LDS_CAP_PAIRS["k2_fd_fold"], str)
    fold = _read("deepmimo_amd", "csrc", "k2_channel_fd_fold.hip")
    for text in ("FOLD_TROW = 272;", "FOLD_MAX_M = 128;", "FOLD_SHARED_FROM = 33;", "const int cand[3] = {32, 16, 8};",
                 "for (int want = 4; want >= 2; --want) {", "if (smem * want <= 160 * 1024) return c;",
                 "return (size_t)tab_rows * 12 + align_up((size_t)M * 4, 16);", "return 256 + (size_t)(M + ch) * FOLD_TROW;"):
        assert text in fold, text
    worst = max((E.fold_lds_bytes(M, nblk), M, nblk) for M in range(1, E.FOLD_MAX_M + 1) for nblk in range(1, 130))
    assert worst[0] == 54592 and worst[0] <= E.LDS_DEFAULT, worst


def test_every_launch_goes_through_the_function_that_takes_the_stream():
    """hipLaunchKernelGGL once, in launch_dyn_lds with the caller's stream; no <<< >>> launch, no memset, no copy but the
    loader's asynchronous one on the caller's stream, no synchronisation and no allocation anywhere in the library"""
    launches, copies = [], []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path) as f:
            text = _no_comments(f.read())
        name = os.path.basename(path)
        launches += [name] * (text.count("hipLaunchKernelGGL") + text.count("<<<"))
        copies += [(name, m) for m in re.findall(r"hipMemcpy\w*|hipMemset\w*", text)]
        for banned in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipFree", "hipStreamCreate"):
            assert banned not in text, (name, banned)
    assert launches == ["dmx_common.h"]
    assert "hipLaunchKernelGGL(kernel, g, b, smem, stream, args...);" in _read("deepmimo_amd", "csrc", "dmx_common.h")
    assert {c[0] for c in copies} == {"mat5_loader.hip"} and {c[1] for c in copies} == {"hipMemcpyAsync", "hipMemcpyHostToDevice"}
    assert re.search(r"hipMemcpyAsync\([^;]*hipMemcpyHostToDevice, \(hipStream_t\)stream\)", _read("deepmimo_amd", "csrc", "mat5_loader.hip"))


def test_reprepare_is_relaunchs_first_half():
    eng = _read("deepmimo_amd", "engine.py")
    body = eng[eng.index("    def relaunch("):eng.index("    # ------------------------------------------------------------------ stage 2\n")]
    assert "self.reprepare(prep)" in body and "dmx_path_prep" not in body.split('"""')[2]
    rp = eng[eng.index("    def reprepare("):eng.index("    def relaunch(")]
    assert 'prep.side["max_delay_key"].zero_()' in rp and "torch.empty" not in rp and ".to(" not in rp
