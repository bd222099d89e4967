#!/usr/bin/env python3
"""Single-pass route against the two calls, alternating in ONE process: `python tools/direct_bench.py [--users 200000]`.

For each shape: stage 1 (light side products) + stage 2 (`variant = 0`, i.e. what `single_pass = False` runs) and
dmx_channels_fd_direct on the same uploaded rays, resident output, the same light side tensors, timed by the protocol of
`tools/ab_protocol.py` (device events around `--launches` launches, a warm-up of 10).  One JSON line per shape: the
protocol's fields per route, algorithmic bytes (rays read + output written) and the share of the 8 TB/s HBM peak they amount to.
`--profile` runs every route a few times only (for `rocprofv3 --kernel-trace --stats -- python tools/direct_bench.py --profile`).
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
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

HBM_PEAK = 8.0e12
# (BS panel, UE panel, K): DeepMIMO's default call first, 8 x 8 / 2 x 2 x 8 is the edge of the small-output region
SHAPES = [([8, 1], [1, 1], 1), ([8, 1], [1, 1], 16), ([8, 8], [1, 1], 1), ([8, 8], [1, 1], 4), ([32, 32], [1, 1], 2),
          ([8, 8], [2, 2], 8)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200000)
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="antenna pairs x K grid of the small-output region instead of the "
                    "shape list (the crossover table next to engine.single_pass_route)")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    lib = eng.lib
    n, L = args.users, args.paths
    rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234))
    stream = eng._stream_ptr()
    shapes = SHAPES
    if args.sweep:
        shapes = [(bs, ue, K) for bs, ue in (([1, 1], [1, 1]), ([8, 1], [1, 1]), ([4, 4], [1, 1]), ([8, 4], [1, 1]), ([8, 8], [1, 1]),
                                             ([8, 4], [2, 1]), ([8, 8], [2, 1]), ([8, 8], [2, 2])) for K in (1, 2, 4, 8, 16)]
    for bs, ue, K in shapes:
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        ps, rs, ss = prep.params_struct, prep.rays_struct, prep.side_struct
        stage1 = ab.stage1(eng, prep)
        out = torch.empty(eng.channel_shape(prep), dtype=torch.complex64, device=eng.device)
        wsp, outp = C.c_void_p(prep.workspace.data_ptr()), C.c_void_p(out.data_ptr())
        pairs = int(np.prod(bs) * np.prod(ue))
        rec = dict(bs=bs, ue=ue, K=K, users=n, paths=L, pairs=pairs,
                   auto_choice=int(lib.dmx_fd_kernel_choice(C.byref(ps), L)),
                   direct_supported=int(lib.dmx_fd_direct_supported(C.byref(ps), L)))
        rec["bytes"] = n * L * 8 * 4 + n * pairs * K * 8
        rec["floor_ms"] = rec["bytes"] / HBM_PEAK * 1e3

        def two_calls():
            stage1()
            nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, outp, 0, stream), "dmx_channels_fd")

        def single_pass():
            nat.check(lib.dmx_channels_fd_direct(C.byref(rs), C.byref(ps), C.byref(ss), 0, n, outp, stream), "dmx_channels_fd_direct")

        routes = [("two_calls", two_calls)] + ([("single_pass", single_pass)] if rec["direct_supported"] == 1 else [])
        if args.sweep and (rec["auto_choice"] != 9 or rec["direct_supported"] != 1):
            print(json.dumps(dict(bs=bs, ue=ue, K=K, pairs=pairs, auto_choice=rec["auto_choice"], direct_supported=rec["direct_supported"])), flush=True)
            continue
        if args.profile:
            for _, fn in routes:
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            continue
        ts = ab.alternate([(name, fn, ab.device(args.launches), ab.device(10)) for name, fn in routes], args.rounds)
        rec.update(ab.summaries(ts))
        for name, _ in routes:
            rec[f"{name}_share_of_peak"] = round(rec["floor_ms"] / rec[f"{name}_avg_ms"], 4)
        if "single_pass_avg_ms" in rec:
            rec["speedup"] = round(rec["two_calls_avg_ms"] / rec["single_pass_avg_ms"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
