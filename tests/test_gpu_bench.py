"""bench.py's workloads run end to end at reduced user counts (one JSON line each, the contract's keys, the right kernel):
keeps every branch of the benchmark - headline, default arrays, beam power, time domain, rx_filter, Doppler - from
rotting between the rounds' full-size runs (with --full: every leg of the line), and a plain run stays lean and
dumps what it computed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("c3_headline", 300, "k2_fd_mfma", "hbm"), ("c5_massive", 12, "k2_fd_mfma", "hbm"), ("d8_default_arrays", 2000, "k2_fd_fold", "hbm"),
         ("d64_k256", 500, "k2_fd_fold", "hbm"), ("c3_beam_power", 300, "k2c_beam_power", "mfma"),
         ("c3_time_domain", 500, "k4_td", "hbm"), ("c3_rx_filter", 200, "k3_lpf_fft512 + k2_fd_mfma (table-fed)", "hbm")]


@pytest.mark.parametrize("workload,users,kernel,bound", CASES, ids=[c[0] for c in CASES])
def test_bench_workload_line(workload, users, kernel, bound):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--users", str(users), "--steps", "2",
                        "--warmup", "1", "--cpu-users", "0", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["metric"] == "user-channels/sec" and d["n_gpus"] == 1 and d["steps"] == 2 and d["vs_baseline"] is None
    assert d["config"]["fd_kernel"] == kernel and d["config"]["users_total"] == users
    rf = d["roofline"]
    assert rf["bound"] == bound and rf["achieved"] > 0 and rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"])
    assert d["value"] == pytest.approx(users / (d["ms_per_step"] * 1e-3), rel=1e-6)
    if workload == "c5_massive":
        assert "Doppler" in d["config"]["workload"]
    # the adaptive-precision rule's share is on the line for the kernels that have it, and only for them
    has_rule = kernel in ("k2_fd_mfma", "k2_fd_fold", "k2c_beam_power")
    assert ("kernel_ms_adaptive_terms" in rf) == has_rule
    if has_rule:
        assert rf["kernel_ms_adaptive_terms"] > 0 and rf["frac_adaptive_terms"] == pytest.approx(rf["frac"] * rf["kernel_ms"] / rf["kernel_ms_adaptive_terms"])
        assert "DMX_FLAG_ADAPTIVE_TERMS" in d["config"]["arithmetic"]


def _bench(*extra, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--warmup", "1", *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the line carries the headline figure only (no CPU baseline, no adaptive-precision launches);
    --steps sets the number of timed steps; --dump-outputs writes the last step's channel and side products as float32,
    and two runs with the same arguments write the same values."""
    import numpy as np
    runs = []
    for i, steps in enumerate((3, 1)):
        d = _bench("--steps", str(steps), "--dump-outputs", str(tmp_path / f"run{i}"))
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] == pytest.approx(512 / (d["ms_per_step"] * 1e-3), rel=1e-6)
        assert "cpu_baseline" not in d and "kernel_ms_adaptive_terms" not in d["roofline"]
        files = {f.name: np.load(f) for f in (tmp_path / f"run{i}").iterdir()}
        assert sorted(files) == ["channel.npy", "los.npy", "num_paths.npy", "users_sampled.npy"]
        assert sum(v.nbytes for v in files.values()) <= 64 << 20
        users = files.pop("users_sampled.npy")                     # 512 MB of channels: a seeded sample of users
        assert all(v.dtype == np.float32 for v in files.values())
        assert np.all(np.diff(users) > 0) and users[0] >= 0 and users[-1] < 512
        assert files["channel.npy"].shape == (len(users), 4, 64, 512, 2) and np.isfinite(files["channel.npy"]).all()
        assert np.abs(files["channel.npy"]).max(axis=(1, 2, 3, 4)).min() > 0
        assert files["num_paths.npy"].shape == (512,) and np.all(files["num_paths.npy"] == 25)
        files["users_sampled.npy"] = users
        runs.append(files)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
