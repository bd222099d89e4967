"""tools/ab_protocol.py without a GPU: the order in which the alternation calls its routes, the fields the summary builds
from scripted readings against the expressions the bench tools carried before they shared the module, and the writer."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_protocol as ab  # noqa: E402

P0, P1 = [1.0, 2.0, 3.0], [2.5, 2.5, 4.0]          # pass averages 2.0 and 3.0, medians 2.0 and 2.5: exactly representable


class Script:
    """Fake timers that log (kind, route, launches) and hand out scripted readings; warm-ups read -1."""

    def __init__(self, readings=None):
        self.log, self.left = [], {k: list(v) for k, v in (readings or {}).items()}

    def timer(self, kind, launches=None):
        def timed(fn):
            self.log.append((kind, fn(), launches))
            return -1.0 if kind == "warm" else self.left[self.log[-1][1]].pop(0) if self.left else 0.0
        return timed

    def route(self, name, launches=None, warm=None):
        return (name, lambda: name, self.timer("time", launches), self.timer("warm", warm))


def test_two_passes_of_warm_up_then_rounds_in_route_order():
    s, hooks = Script({r: [10 * i + j for j in range(6)] for i, r in enumerate("abc")}), []
    ts = ab.alternate([s.route(r) for r in "abc"], 3, after=lambda: hooks.append(len(s.log)))
    one_pass = [("warm", r, None) for r in "abc"] + [("time", r, None) for _ in range(3) for r in "abc"]
    assert s.log == one_pass * 2
    assert hooks == list(range(1, 25))                       # once behind every reading, the warm-ups included
    assert ts == {r: ([10 * i + j for j in range(3)], [10 * i + j for j in range(3, 6)]) for i, r in enumerate("abc")}
    assert -1.0 not in itertools.chain.from_iterable(p for v in ts.values() for p in v)
    assert list(ts) == list("abc")


def test_timer_and_warm_up_per_route_as_in_pattern_bench():
    """pattern_bench.py: per form `stage1` (warm-up 5, 20 launches) and `both` (warm-up 2, 4 launches), interleaved"""
    s, forms = Script(), ("isotropic", "tr38901_bs")
    routes = [r for f in forms for r in (s.route((f, "stage1"), 20, 5), s.route((f, "both"), 4, 2))]
    ts = ab.alternate(routes, 2)
    warm = [("warm", (f, w), k) for f in forms for w, k in (("stage1", 5), ("both", 2))]
    rounds = [("time", (f, w), k) for _ in range(2) for f in forms for w, k in (("stage1", 20), ("both", 4))]
    assert s.log == (warm + rounds) * 2
    assert all(len(p) == 2 for v in ts.values() for p in v) and set(ts) == {(f, w) for f in forms for w in ("stage1", "both")}


def test_no_hook_and_no_rounds():
    s = Script()
    assert ab.alternate([s.route("a")], 0) == {"a": ([], [])}
    assert s.log == [("warm", "a", None)] * 2


def parent_fields(rn, digits, medians, raw, overall_min):
    """What the tools wrote before, their own expressions: `rec[f"{rn}_..."]` of the per-shape layout; with rn = "" the
    lines are those of the per-route layout (`rec["avg_ms"]`)."""
    rec = {}
    for ab_, v in enumerate((P0, P1)):
        if raw:
            rec[f"{rn}ms_pass{ab_}"] = [round(float(x), digits) for x in v]
        rec[f"{rn}avg_ms_pass{ab_}"] = round(float(np.mean(v)), digits)
        if medians:
            rec[f"{rn}median_ms_pass{ab_}"] = round(float(np.median(v)), digits)
        rec[f"{rn}min_ms_pass{ab_}"] = round(float(np.min(v)), digits)
    a0, a1 = rec[f"{rn}avg_ms_pass0"], rec[f"{rn}avg_ms_pass1"]
    rec[f"{rn}avg_ms"] = round((a0 + a1) / 2, digits)
    if overall_min:
        rec[f"{rn}min_ms"] = min(rec[f"{rn}min_ms_pass0"], rec[f"{rn}min_ms_pass1"])
    rec[f"{rn}spread_ms"] = round(abs(a0 - a1), digits)
    if medians:
        m0, m1 = rec[f"{rn}median_ms_pass0"], rec[f"{rn}median_ms_pass1"]
        rec[f"{rn}median_ms"] = round((m0 + m1) / 2, digits)
        rec[f"{rn}median_spread_ms"] = round(abs(m0 - m1), digits)
    return rec


@pytest.mark.parametrize("prefix,digits,medians,raw,overall_min",
                         list(itertools.product(("", "fused_"), (4, 5), (False, True), (False, True), (False, True))))
def test_summary_is_the_tools_arithmetic(prefix, digits, medians, raw, overall_min):
    got = ab.summary((P0, P1), prefix=prefix, digits=digits, medians=medians, raw=raw, overall_min=overall_min)
    want = parent_fields(prefix, digits, medians, raw, overall_min)
    assert got == want and set(got) == set(want)             # dict equality is exact: no key more, no key less
    assert got[prefix + "avg_ms"] == 2.5 and got[prefix + "spread_ms"] == 1.0 and got[prefix + "min_ms_pass1"] == 2.5


def test_summary_defaults_are_the_plain_layout():
    assert set(ab.summary((P0, P1))) == {"avg_ms_pass0", "min_ms_pass0", "avg_ms_pass1", "min_ms_pass1", "avg_ms", "spread_ms"}


def test_two_pass_fields_come_from_the_rounded_pass_averages():
    p0, p1 = [0.000014, 0.000014], [0.000026, 0.000026]     # 1e-05 and 3e-05 at 5 digits: mean 2e-05, spread 2e-05
    got = ab.summary((p0, p1))
    a0, a1 = round(float(np.mean(p0)), 5), round(float(np.mean(p1)), 5)
    assert got["avg_ms"] == round((a0 + a1) / 2, 5) and got["spread_ms"] == round(abs(a0 - a1), 5)
    assert got["spread_ms"] != round(abs(float(np.mean(p0)) - float(np.mean(p1))), 5)


def test_summaries_prefix_every_route():
    got = ab.summaries({"fused": (P0, P1), "twin": (P1, P0)}, digits=4, overall_min=True)
    want = dict(parent_fields("fused_", 4, False, False, True))
    want.update(ab.summary((P1, P0), prefix="twin_", digits=4, overall_min=True))
    assert got == want


def test_writer_replaces_appends_and_creates_the_directory(tmp_path, capsys):
    path = tmp_path / "not" / "there" / "x.jsonl"
    ab.write_lines(str(path), ['{"a": 1}', '{"b": 2}'], "w")
    assert path.read_text() == '{"a": 1}\n{"b": 2}\n' and capsys.readouterr().out == ""
    ab.write_lines(str(path), ['{"c": 3}'], "a", echo=True)
    assert path.read_text() == '{"a": 1}\n{"b": 2}\n{"c": 3}\n' and capsys.readouterr().out == '{"c": 3}\n'
    ab.write_lines(str(path), ['{"d": 4}'], "w")
    assert path.read_text() == '{"d": 4}\n'
