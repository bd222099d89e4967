"""The twelve A/B bench tools on tools/ab_protocol.py, each run in-process at a rehearsal size: the tool returns (its own
asserts between routes held), every line it writes parses, and every route a record names carries the protocol's per-pass
and two-pass fields.  The arguments are the smallest round ones at which the tools ran clean before they shared the module;
`--eig-users 2` keeps rate_bench.py's batched eigvalsh / svd twins (70 ms per user at K = 512) to a fraction of a second."""
import importlib
import json
import math
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

SCALED = ["--scale", "0.002", "--launches", "1", "--rounds", "1"]
NEAR_FIELD_ROUTES = {"near", "far_v1", "far_auto", "rate_near", "rate_far", "beam_power_near", "beam_power_far"}
# tool: (arguments, lines, route prefixes of the per-shape layout or route names of the per-route layout, digits)
TOOLS = {
    "direct_bench": (["--users", "2000", "--launches", "2", "--rounds", "1"], 6, {"two_calls_", "single_pass_"}, 5),
    "covariance_bench": (SCALED, 6, {"fused_", "einsum_"}, 5),
    "rate_bench": (SCALED + ["--eig-users", "2"], 2,
                   {"fused_", "slogdet_", "spectrum_", "modes_", "eigvalsh_", "beams_", "beams2_", "svd_"}, 5),
    "cell_rate_bench": (SCALED, 2, {"fused_", "single_", "twin_"}, 5),
    "angle_delay_bench": (SCALED, 4, {"fused_", "twin_"}, 5),
    "codebook_rate_bench": (SCALED, 4, {"fused_", "twin_"}, 5),
    "subband_pmi_bench": (SCALED, 3, {"subbands_", "wideband_", "loop_"}, 5),
    "pattern_bench": (SCALED, 10, {"stage1_", "both_"}, 5),
    "time_series_bench": (["--users", "500", "--times", "3", "--subcarriers", "64", "--rounds", "1"], 2,
                          {"series_", "eight_", "view_", "block_", "rate_", "rate8_"}, 4),
    "beam_pair_bench": (["--users", "512", "--unfused-users", "128", "--unfused-chunk", "64", "--subcarriers", "64", "--beams", "8",
                         "--rounds", "1"], 1, {"pair_", "unfused_", "one_sided_"}, 4),
    "wideband_bench": (SCALED, 6, {"wideband", "narrow_v1", "narrow_auto"}, 5),
    "near_field_bench": (SCALED, 14, NEAR_FIELD_ROUTES, 5),
}
PER_ROUTE_LAYOUT = {"wideband_bench", "near_field_bench"}


@pytest.fixture
def channel_output():
    import deepmimo_amd as dm
    before = dm.config("channel_output")
    yield
    dm.config("channel_output", before)


def profiles_state():
    d = os.path.join(ROOT, "profiles")
    return sorted((f, os.path.getsize(os.path.join(d, f)), os.path.getmtime(os.path.join(d, f))) for f in os.listdir(d))


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_runs_and_writes_the_protocol_fields(tool, tmp_path, capsys, monkeypatch, channel_output):
    argv, n_lines, routes, digits = TOOLS[tool]
    monkeypatch.chdir(tmp_path)                                  # a default path under profiles/ would land here, and fail below
    before = profiles_state()
    out = tmp_path / "sub" / "out.jsonl"
    mod = importlib.import_module(tool)
    mod.main(list(argv) + ([] if tool == "direct_bench" else ["--out", str(out)]))
    text = capsys.readouterr().out if tool == "direct_bench" else out.read_text()
    assert profiles_state() == before and sorted(os.listdir(tmp_path)) == ([] if tool == "direct_bench" else ["sub"])
    assert text.endswith("\n")
    recs = [json.loads(line) for line in text.splitlines()]
    assert len(recs) == n_lines
    seen = set()
    for rec in recs:
        prefixes = [m.group(1) for m in (re.fullmatch(r"(.*)avg_ms_pass0", k) for k in rec) if m]
        assert prefixes, rec
        seen |= {rec["route"]} if tool in PER_ROUTE_LAYOUT else set(prefixes)
        assert prefixes == [""] if tool in PER_ROUTE_LAYOUT else "" not in prefixes
        for p in prefixes:
            fields = {k: rec[p + k] for k in ("avg_ms_pass0", "avg_ms_pass1", "min_ms_pass0", "min_ms_pass1", "avg_ms", "spread_ms")}
            assert all(isinstance(v, float) and math.isfinite(v) for v in fields.values()), (p, fields)
            assert all(v > 0 for k, v in fields.items() if k != "spread_ms") and fields["spread_ms"] >= 0, (p, fields)
            assert fields["spread_ms"] == round(abs(fields["avg_ms_pass0"] - fields["avg_ms_pass1"]), digits), (p, fields)
            assert fields["avg_ms"] == round((fields["avg_ms_pass0"] + fields["avg_ms_pass1"]) / 2, digits), (p, fields)
            assert fields["min_ms_pass0"] <= fields["avg_ms_pass0"] and fields["min_ms_pass1"] <= fields["avg_ms_pass1"]
        for parity in ("series_equals_eight_bitwise", "subbands_equal_loop_bits"):
            assert rec.get(parity, True) is True, (parity, rec)
    assert seen == routes
