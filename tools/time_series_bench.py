#!/usr/bin/env python3
"""Channel time series: what `compute_channels(times=...)` and the `at_times` view cost beside the calls they replace, in ONE
process: `python tools/time_series_bench.py [--out profiles/r13_time_series_bench.jsonl]`.

DeepMIMO's default arrays (BS 8 x 1, UE 1 x 1) with K = 512, 50k users x 25 paths, T = 8 snapshots, torch output, once with
the ray matrices on the host (NumPy) and once with them in HBM (torch):
  (a) series    ds.compute_channels(p, times=times)                    [T, n, 1, 8, K] from one call
  (b) eight     T plain compute_channels(p) calls on T datasets whose phases were advanced beforehand - what the package
                could do before `times` existed, and the yardstick
  (c) view      ds.at_times(times) alone: the only work (a) adds to (b)
  (c') block    the view (a) itself builds: one block of the ray and Doppler matrices, uploaded untiled and tiled and
                advanced in HBM wherever the rays live
  (d) rate      ds.at_times(times).compute_rate(p, snr_db=...)         [T * n]
  (e) rate8     T plain compute_rate(p, snr_db=...) calls on the datasets of (b)
Host work is part of every route (the view is host-side code), so a timing is wall-clock time around the call and the
release of its result, with a device synchronisation on both sides, not a pair of device events.  The routes alternate `--rounds` times after a warm-up; the
whole A/B runs twice (`pass` 0 and 1) and the difference between the two passes of the SAME route is the spread a
difference between the routes has to exceed.  One JSON line per placement of the rays: mean, minimum and spread of every
route (and every single timing, `*_ms_pass*`: one slow launch shows as what it is), (a)/(b), (c)/(a), (d)/(e), and whether (a) exceeds (b) by more than (b)'s spread plus (c).  Without a GPU the tool
fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd import dataset as dsm  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    del res                                          # releasing a result is part of its cost: 2 ms per 40 MB host array
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--subcarriers", type=int, default=512)
    ap.add_argument("--times", type=int, default=8, help="snapshots T")
    ap.add_argument("--step", type=float, default=1e-3, help="seconds between snapshots")
    ap.add_argument("--carrier", type=float, default=28e9)
    ap.add_argument("--snr-db", type=float, default=110.0)
    ap.add_argument("--rounds", type=int, default=5, help="timings per route and pass")
    ap.add_argument("--placements", default="host,device")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_series_bench: no GPU")
    n, L, K, T = args.users, args.paths, args.subcarriers, args.times
    times = np.arange(T) * args.step
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(K)
    rays = onp.synth_rays(n, L, seed=1234, all_valid=True, with_doppler=True)
    dm.config("channel_output", "torch")
    lines = []
    for place in args.placements.split(","):
        put = (lambda v: torch.from_numpy(v).cuda()) if place == "device" else (lambda v: v.copy())
        ds = dm.Dataset({k: put(v) for k, v in rays.items()})
        singles = [ds.at_times(float(t), carrier_freq=args.carrier) for t in times]     # advanced beforehand: not timed

        routes = [
            ("series", lambda: ds.compute_channels(p, times=times, carrier_freq=args.carrier)),
            ("eight", lambda: [s.compute_channels(p) for s in singles][-1]),
            ("view", lambda: ds.at_times(times, carrier_freq=args.carrier)),
            ("block", lambda: ds._in_hbm(dsm._BLOCK_KEYS)._block_view("compute_channels", ds._call_params(p), times, args.carrier)),
            ("rate", lambda: ds.at_times(times, carrier_freq=args.carrier).compute_rate(p, snr_db=args.snr_db)),
            ("rate8", lambda: [s.compute_rate(p, snr_db=args.snr_db) for s in singles][-1]),
        ]
        rec = dict(rays=place, bs=[8, 1], ue=[1, 1], K=K, users=n, paths=L, T=T, step_s=args.step, carrier_hz=args.carrier,
                   H_bytes=T * n * 8 * K * 8, timings_per_route=2 * args.rounds)
        # the two ways agree: (a)'s snapshots are (b)'s tensors bit for bit
        series = ds.compute_channels(p, times=times, carrier_freq=args.carrier)
        rec["series_equals_eight_bitwise"] = all(bool(torch.equal(series[i], s.compute_channels(p))) for i, s in enumerate(singles))
        del series
        for s in singles:
            s._data.pop("channel", None)
        torch.cuda.empty_cache()
        for ab in range(2):
            def run(fn):
                dt = timed(fn)
                for s in singles:                                        # (b) caches `channel` per dataset, 1.6 GB each: kept,
                    s._data.pop("channel", None)                         # its next round is served by splitting (a)'s cached
                return dt                                                # 13 GB block, and allocating that anew takes 0.4-0.8 s

            for _, fn in routes:                                         # warm-up
                run(fn)
            ts = {rn: [] for rn, _ in routes}
            for _ in range(args.rounds):
                for rn, fn in routes:
                    ts[rn].append(run(fn))
            for rn, v in ts.items():
                rec[f"{rn}_ms_pass{ab}"] = [round(float(x), 4) for x in v]
                rec[f"{rn}_avg_ms_pass{ab}"] = round(float(np.mean(v)), 4)
                rec[f"{rn}_median_ms_pass{ab}"] = round(float(np.median(v)), 4)
                rec[f"{rn}_min_ms_pass{ab}"] = round(float(np.min(v)), 4)
        for rn, _ in routes:
            a0, a1 = rec[f"{rn}_avg_ms_pass0"], rec[f"{rn}_avg_ms_pass1"]
            rec[f"{rn}_avg_ms"] = round((a0 + a1) / 2, 4)
            rec[f"{rn}_spread_ms"] = round(abs(a0 - a1), 4)
            m0, m1 = rec[f"{rn}_median_ms_pass0"], rec[f"{rn}_median_ms_pass1"]
            rec[f"{rn}_median_ms"] = round((m0 + m1) / 2, 4)
            rec[f"{rn}_median_spread_ms"] = round(abs(m0 - m1), 4)
        rec["series_over_eight"] = round(rec["series_avg_ms"] / rec["eight_avg_ms"], 4)
        rec["view_over_series"] = round(rec["view_avg_ms"] / rec["series_avg_ms"], 4)
        rec["rate_over_rate8"] = round(rec["rate_avg_ms"] / rec["rate8_avg_ms"], 4)
        rec["series_over_eight_medians"] = round(rec["series_median_ms"] / rec["eight_median_ms"], 4)
        rec["series_minus_eight_minus_block_ms"] = round(rec["series_avg_ms"] - rec["eight_avg_ms"] - rec["block_avg_ms"], 4)
        rec["series_minus_eight_ms"] = round(rec["series_avg_ms"] - rec["eight_avg_ms"], 4)
        rec["series_exceeds_eight_by_more_than_spread_plus_view"] = bool(
            rec["series_minus_eight_ms"] > rec["eight_spread_ms"] + rec["view_avg_ms"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del ds, singles, routes
        torch.cuda.empty_cache()
    dm.config("channel_output", "numpy")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
