#!/usr/bin/env python3
"""What the near-field array response costs: `python tools/near_field_bench.py --label this`.

Two shapes: the headline one (100k users, 25 paths, 8 x 8 BS / 2 x 2 UE = 64 x 4 antennas, K = 512) and DeepMIMO's default
arrays (200k users, 8 x 1 / 1 x 1, K = 512).  Seven routes on the same uploaded rays, stage 1 included in every one:

  near         dmx_path_prep + dmx_channels_fd(variant = 0) with DMX_FLAG_NEAR_FIELD: the fp32 vector kernel with
               spherical-wavefront tables (28 GHz carrier, 400 MHz of bandwidth), into a resident tensor
  far_v1       the far-field call forced to the same kernel, variant = 1: the same contraction, (near / far_v1) is what the
               (M_rx + M_tx) P float64 square roots and divisions per user cost
  far_auto     the far-field automatic route, variant = 0: (near / far_auto) is the price of the effect for channels
  rate_near, rate_far              dmx_path_prep + dmx_channel_rate, with and without the flag
  beam_power_near, beam_power_far  dmx_path_prep + dmx_beam_power with 64 beams, with and without the flag (with it the
               projection is the scalar kernel for every panel)

Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per (shape, route) with the
protocol's fields unprefixed, appended to `--out`.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402
import bench  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402

SHAPES = [dict(name="headline", bs=[8, 8], ue=[2, 2], K=512, users=100_000),
          dict(name="default_arrays", bs=[8, 1], ue=[1, 1], K=512, users=200_000)]
CARRIER, BANDWIDTH, BEAMS, SNR_DB = 28e9, 400e6, 64, 10.0
TWINS = {"near": ("far_v1", "far_auto"), "rate_near": ("rate_far",), "beam_power_near": ("beam_power_far",)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this", help="which build this is (a field of every line)")
    ap.add_argument("--out", default=os.path.join("profiles", "r16_near_field_bench.jsonl"))
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--shapes", nargs="+", default=[s["name"] for s in SHAPES], choices=[s["name"] for s in SHAPES])
    ap.add_argument("--scale", type=float, default=1.0, help="multiply both user counts (a rehearsal at a small size)")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    lib, dev, L = eng.lib, eng.device, args.paths
    stream = eng._stream_ptr()
    lines = []
    for sh in [s for s in SHAPES if s["name"] in args.shapes]:
        n = max(1, int(sh["users"] * args.scale))
        rays = eng.upload_rays(bench.synth_device_rays(n, L, 1234, dev))
        m_rx, m_tx = int(np.prod(sh["ue"])), int(np.prod(sh["bs"]))
        out = torch.empty((n, m_rx, m_tx, sh["K"]), dtype=torch.complex64, device=dev)
        outp = C.c_void_p(out.data_ptr())
        rng = np.random.default_rng(5)
        F = ((rng.standard_normal((BEAMS, m_tx)) + 1j * rng.standard_normal((BEAMS, m_tx))) / np.sqrt(2 * m_tx)).astype(np.complex64)
        F = torch.from_numpy(F).to(dev)                            # resident: no upload inside a timed launch
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(sh["bs"]), np.array(sh["ue"])
        p.num_paths = L
        p.ofdm.selected_subcarriers = np.arange(sh["K"])
        p.ofdm.bandwidth = BANDWIDTH
        p.validate(n)
        preps = {near: eng.prepare(rays, p, want_side="light", carrier_freq=CARRIER, near_field=near) for near in (True, False)}
        runs, results = [], {}

        def add(route, near, call, what, **extra):
            prep = preps[near]
            ps, wsp, stage1 = prep.params_struct, C.c_void_p(prep.workspace.data_ptr()), ab.stage1(eng, prep)

            def both():
                stage1()
                results[route] = call(prep, ps, wsp)
            runs.append((dict(build=args.label, shape=sh["name"], bs=sh["bs"], ue=sh["ue"], K=sh["K"], users=n, paths=L, route=route,
                              near_field=near, carrier_hz=CARRIER, bandwidth_hz=BANDWIDTH, calls="dmx_path_prep + " + what, **extra), both))

        def channels(variant):
            def call(prep, ps, wsp):
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, outp, variant, stream), "dmx_channels_fd")
            return call

        kernel = lambda near, v: int(lib.dmx_fd_kernel_choice(C.byref(preps[near].params_struct), L)) if v == 0 else v   # noqa: E731
        add("near", True, channels(0), "dmx_channels_fd", variant=0, kernel=kernel(True, 0))
        add("far_v1", False, channels(1), "dmx_channels_fd", variant=1, kernel=1)
        add("far_auto", False, channels(0), "dmx_channels_fd", variant=0, kernel=kernel(False, 0))
        for near in (True, False):
            tag = "near" if near else "far"
            add(f"rate_{tag}", near, lambda prep, ps, wsp: eng.rate(prep, SNR_DB), "dmx_channel_rate", snr_db=SNR_DB)
            add(f"beam_power_{tag}", near, lambda prep, ps, wsp: eng.beam_power(prep, F, want_best=False)[0], "dmx_beam_power", beams=BEAMS)
        ts = ab.alternate([(rec["route"], both, ab.device(args.launches), ab.device(1)) for rec, both in runs], args.rounds)
        by_route = {}
        for rec, _ in runs:
            rec.update(ab.summary(ts[rec["route"]]))
            by_route[rec["route"]] = rec
        for near, twins in TWINS.items():
            for twin in twins:
                by_route[near][f"over_{twin}"] = round(by_route[near]["avg_ms"] / by_route[twin]["avg_ms"], 4)
        # what was timed is the effect: the near-field channel is finite, differs from the far-field one by far more than the
        # parity criterion, and the two far-field routes agree with each other within it
        step = max(1, n // 64)
        by_name = {rec["route"]: both for rec, both in runs}
        by_name["near"]()
        near_h = out[::step].clone()
        by_name["far_v1"]()
        far_h = out[::step].clone()
        by_name["far_auto"]()
        peak = far_h.abs().amax(dim=(1, 2, 3)).clamp_min(1e-30)
        d_near = (near_h - far_h).abs().amax(dim=(1, 2, 3)) / peak
        d_far = (out[::step] - far_h).abs().amax(dim=(1, 2, 3)) / peak
        assert bool(torch.isfinite(torch.view_as_real(near_h)).all()) and float(peak.max()) > 1e-30, "bench output is not finite / all zero"
        assert float(d_far.max()) <= 5e-5 and float(d_near.max()) > 5e-3, (float(d_far.max()), float(d_near.max()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(results["rate_near"]).all()) and bool(torch.isfinite(results["beam_power_near"]).all())
        assert not torch.equal(results["rate_near"], results["rate_far"]) and not torch.equal(results["beam_power_near"], results["beam_power_far"])
        for rec, _ in runs:
            rec["check_near_minus_far_rel"], rec["check_far_routes_rel"] = round(float(d_near.max()), 5), round(float(d_far.max()), 9)
            lines.append(rec)
        del runs, out, rays, preps, results
        torch.cuda.empty_cache()
    ab.write_lines(args.out, [json.dumps(rec) for rec in lines], "a", echo=True)


if __name__ == "__main__":
    main()
