#!/usr/bin/env python3
"""What the spatial-wideband channel costs: `python tools/wideband_bench.py --label this`.

Two shapes: the headline one (100k users, 25 paths, 8 x 8 BS / 2 x 2 UE = 64 x 4 antennas, K = 512) and DeepMIMO's default
arrays (200k users, 8 x 1 / 1 x 1, K = 512).  Three routes on the same uploaded rays, stage 1 included in every one, the
channels written into a resident tensor:

  wideband    dmx_path_prep + dmx_channels_fd(variant = 0) with DMX_FLAG_SPATIAL_WIDEBAND: the per-subcarrier body of the
              fp32 vector kernel (28 GHz carrier, 400 MHz of bandwidth)
  narrow_v1   the narrowband call forced to the same kernel, variant = 1: (wideband / narrow_v1) is what the body costs
  narrow_auto the narrowband automatic route, variant = 0: (wideband / narrow_auto) is the price of the effect

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

ROUTES = [("wideband", True, 0), ("narrow_v1", False, 1), ("narrow_auto", False, 0)]
SHAPES = [dict(name="headline", bs=[8, 8], ue=[2, 2], K=512, users=100_000),
          dict(name="default_arrays", bs=[8, 1], ue=[1, 1], K=512, users=200_000)]
CARRIER, BANDWIDTH = 28e9, 400e6


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this", help="which build this is (a field of every line)")
    ap.add_argument("--out", default=os.path.join("profiles", "r15_wideband_bench.jsonl"))
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
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(sh["bs"]), np.array(sh["ue"])
        p.num_paths = L
        p.ofdm.selected_subcarriers = np.arange(sh["K"])
        p.ofdm.bandwidth = BANDWIDTH
        p.validate(n)
        runs = []
        for route, wideband, variant in ROUTES:
            prep = eng.prepare(rays, p, want_side="light", carrier_freq=CARRIER, spatial_wideband=wideband)
            ps = prep.params_struct
            rec = dict(build=args.label, shape=sh["name"], bs=sh["bs"], ue=sh["ue"], K=sh["K"], users=n, paths=L, route=route,
                       carrier_hz=CARRIER, bandwidth_hz=BANDWIDTH, variant=variant, kernel=int(lib.dmx_fd_kernel_choice(C.byref(ps), L))
                       if variant == 0 else variant, calls="dmx_path_prep + dmx_channels_fd")

            def both(ps=ps, stage1=ab.stage1(eng, prep), wsp=C.c_void_p(prep.workspace.data_ptr()), variant=variant):
                stage1()
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, outp, variant, stream), "dmx_channels_fd")
            runs.append((rec, prep, both))
        ts = ab.alternate([(rec["route"], both, ab.device(args.launches), ab.device(1)) for rec, _, both in runs], args.rounds)
        by_route = {}
        for rec, _, _ in runs:
            rec.update(ab.summary(ts[rec["route"]]))
            by_route[rec["route"]] = rec
        for rec, _, _ in runs:
            rec["wideband_over_this"] = round(by_route["wideband"]["avg_ms"] / rec["avg_ms"], 4)
            lines.append(rec)
        # what was timed is the channel: at subcarrier 0 the wideband route gives the narrowband one (5e-5 of a user's peak,
        # the parity criterion), and away from it the squint is there
        step = max(1, n // 64)
        by_name = {rec["route"]: both for rec, _, both in runs}
        by_name["wideband"]()
        wide = out[::step].clone()
        by_name["narrow_v1"]()
        narrow = out[::step]
        peak = narrow.abs().amax(dim=(1, 2, 3)).clamp_min(1e-30)
        d0 = (wide[..., 0] - narrow[..., 0]).abs().amax(dim=(1, 2)) / peak
        d_edge = (wide[..., -1] - narrow[..., -1]).abs().amax(dim=(1, 2)) / peak
        assert bool(torch.isfinite(torch.view_as_real(wide)).all()) and float(peak.max()) > 1e-30, "bench output is not finite / all zero"
        assert float(d0.max()) <= 5e-5 and float(d_edge.max()) > 5e-3, (float(d0.max()), float(d_edge.max()))
        for rec, _, _ in runs:
            rec["check_sc0_rel"], rec["check_edge_rel"] = round(float(d0.max()), 9), round(float(d_edge.max()), 5)
        del runs, out, rays
        torch.cuda.empty_cache()
    ab.write_lines(args.out, [json.dumps(rec) for rec in lines], "a", echo=True)


if __name__ == "__main__":
    main()
