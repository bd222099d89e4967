#!/usr/bin/env python3
"""Per-user spatial covariance: the fused route against the channel tensor + einsum, alternating in ONE process:
`python tools/covariance_bench.py [--out profiles/r6_covariance_bench.jsonl]`.

For each shape and side, on the same uploaded rays:
  (a) fused    dmx_path_prep + dmx_channel_covariance                         (no channel tensor)
  (b) einsum   dmx_path_prep + dmx_channels_fd (variant 0) + torch.einsum of the definition on the resident tensor
Device events around back-to-back launches of one route, the routes alternating `--rounds` times after a warm-up; the
whole A/B runs twice (`pass` 0 and 1) and the difference between the two passes of the SAME route is the spread a
difference between the routes has to exceed.  One JSON line per (shape, side): mean, minimum and spread of both routes,
the bytes each route has to move (rays + records + outputs; for (b) the channel tensor written and read once) and the
largest deviation between the two results relative to each user's peak.  Without a GPU the tool fails.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

# (name, BS panel, UE panel, K, users): DeepMIMO's default arrays with every subcarrier (H is 6.6 GB), the headline panel
# (64 x 4 antennas, H is 21 GB at 20k users), the headline panel with DeepMIMO's default single subcarrier
SHAPES = [("defaults_K512", [8, 1], [1, 1], 512, 200_000), ("headline_K512", [8, 8], [2, 2], 512, 20_000),
          ("headline_K1", [8, 8], [2, 2], 1, 200_000)]


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=20, help="back-to-back launches of the fused route per timing")
    ap.add_argument("--launches-einsum", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sides", default="tx,rx")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    eng = ChannelEngine(0)
    lib, L = eng.lib, args.paths
    stream = eng._stream_ptr()
    lines = []
    for name, bs, ue, K, users in SHAPES:
        n = max(1, int(users * args.scale))
        rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        ps, rs, ss = prep.params_struct, prep.rays_struct, prep.side_struct
        m_tx, m_rx = int(np.prod(bs)), int(np.prod(ue))
        H = torch.empty(eng.channel_shape(prep), dtype=torch.complex64, device=eng.device)
        wsp, Hp = C.c_void_p(prep.workspace.data_ptr()), C.c_void_p(H.data_ptr())
        for side in args.sides.split(","):
            sid, m, m_avg = nat.COV_SIDES[side], (m_tx if side == "tx" else m_rx), (m_rx if side == "tx" else m_tx)
            R = torch.empty((n, m, m), dtype=torch.complex64, device=eng.device)
            Rp = C.c_void_p(R.data_ptr())
            spec = "urik,urjk->uij" if side == "tx" else "uitk,ujtk->uij"
            res = {}

            def fused():
                nat.check(lib.dmx_path_prep(C.byref(rs), C.byref(ps), wsp, prep.workspace_bytes, C.byref(ss), stream), "dmx_path_prep")
                nat.check(lib.dmx_channel_covariance(C.byref(ps), wsp, n, L, 0, n, sid, Rp, stream), "dmx_channel_covariance")

            def einsum():
                nat.check(lib.dmx_path_prep(C.byref(rs), C.byref(ps), wsp, prep.workspace_bytes, C.byref(ss), stream), "dmx_path_prep")
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, Hp, 0, stream), "dmx_channels_fd")
                res["R"] = torch.einsum(spec, H, H.conj()) / (m_avg * K)

            routes = [("fused", fused, args.launches), ("einsum", einsum, args.launches_einsum)]
            rays_b, rec_b = n * L * 8 * 4, n * L * 52
            rec = dict(shape=name, side=side, bs=bs, ue=ue, K=K, users=n, paths=L, H_bytes=n * m_rx * m_tx * K * 8, R_bytes=n * m * m * 8)
            rec["fused_bytes"] = rays_b + 2 * rec_b + rec["R_bytes"]
            rec["einsum_bytes"] = rays_b + 2 * rec_b + 2 * rec["H_bytes"] + rec["R_bytes"]
            for ab in range(2):
                for _, fn, _cnt in routes:                                   # warm-up
                    timed(fn, 2)
                ts = {rn: [] for rn, _, _ in routes}
                for _ in range(args.rounds):
                    for rn, fn, cnt in routes:
                        ts[rn].append(timed(fn, cnt))
                for rn, v in ts.items():
                    rec[f"{rn}_avg_ms_pass{ab}"] = round(float(np.mean(v)), 5)
                    rec[f"{rn}_min_ms_pass{ab}"] = round(float(np.min(v)), 5)
            for rn, _, _ in routes:
                a0, a1 = rec[f"{rn}_avg_ms_pass0"], rec[f"{rn}_avg_ms_pass1"]
                rec[f"{rn}_avg_ms"] = round((a0 + a1) / 2, 5)
                rec[f"{rn}_spread_ms"] = round(abs(a0 - a1), 5)
            rec["speedup"] = round(rec["einsum_avg_ms"] / rec["fused_avg_ms"], 3)
            # the two results on the inputs that were timed: complex64 einsum against the fused kernel
            peak = res["R"].abs().reshape(n, -1).amax(dim=1).clamp_min(1e-30)
            rec["max_dev_of_peak"] = float(((R - res["R"]).abs().reshape(n, -1).amax(dim=1) / peak).max())
            del res["R"], R
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del H, prep, rays
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
