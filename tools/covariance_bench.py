#!/usr/bin/env python3
"""Per-user spatial covariance: the fused route against the channel tensor + einsum, alternating in ONE process:
`python tools/covariance_bench.py [--out profiles/r6_covariance_bench.jsonl]`.

For each shape and side, on the same uploaded rays:
  (a) fused    dmx_path_prep + dmx_channel_covariance                         (no channel tensor)
  (b) einsum   dmx_path_prep + dmx_channels_fd (variant 0) + torch.einsum of the definition on the resident tensor
Timed by the protocol of `tools/ab_protocol.py` (device events, a launch count per route, a warm-up of 2).  One JSON line
per (shape, side): the protocol's fields per route, the bytes each route has to move (rays + records + outputs; for (b) the channel tensor written and read once) and the
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
import ab_protocol as ab  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

# (name, BS panel, UE panel, K, users): DeepMIMO's default arrays with every subcarrier (H is 6.6 GB), the headline panel
# (64 x 4 antennas, H is 21 GB at 20k users), the headline panel with DeepMIMO's default single subcarrier
SHAPES = [("defaults_K512", [8, 1], [1, 1], 512, 200_000), ("headline_K512", [8, 8], [2, 2], 512, 20_000),
          ("headline_K1", [8, 8], [2, 2], 1, 200_000)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=20, help="back-to-back launches of the fused route per timing")
    ap.add_argument("--launches-einsum", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sides", default="tx,rx")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
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
        ps, stage1 = prep.params_struct, ab.stage1(eng, prep)
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
                stage1()
                nat.check(lib.dmx_channel_covariance(C.byref(ps), wsp, n, L, 0, n, sid, Rp, stream), "dmx_channel_covariance")

            def einsum():
                stage1()
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, Hp, 0, stream), "dmx_channels_fd")
                res["R"] = torch.einsum(spec, H, H.conj()) / (m_avg * K)

            routes = [("fused", fused, ab.device(args.launches), ab.device(2)),
                      ("einsum", einsum, ab.device(args.launches_einsum), ab.device(2))]
            rays_b, rec_b = n * L * 8 * 4, n * L * 52
            rec = dict(shape=name, side=side, bs=bs, ue=ue, K=K, users=n, paths=L, H_bytes=n * m_rx * m_tx * K * 8, R_bytes=n * m * m * 8)
            rec["fused_bytes"] = rays_b + 2 * rec_b + rec["R_bytes"]
            rec["einsum_bytes"] = rays_b + 2 * rec_b + 2 * rec["H_bytes"] + rec["R_bytes"]
            rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
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
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
