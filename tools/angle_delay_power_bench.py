#!/usr/bin/env python3
"""Angle-delay power matrix and delay profile: the two reduced outputs of dmx_channels_angle_delay against its complex output
and against the unfused route, alternating in ONE process:
`python tools/angle_delay_power_bench.py [--out profiles/r20_angle_delay_power_bench.jsonl]`.

For each shape of tools/angle_delay_bench.py, on the same uploaded rays (in HBM), stage 1 included in every route:
  (a) power    dmx_path_prep + dmx_channels_angle_delay with DMX_FLAG_ANGLE_DELAY_POWER          float32 [n, R, n_taps]
  (b) profile  ... with DMX_FLAG_ANGLE_DELAY_POWER | DMX_FLAG_ANGLE_DELAY_PROFILE                float32 [n, n_taps]
  (c) complex  ... without the bits                                                              complex64 [n, M_rx, R, n_taps]
  (d) unfused  the complex call + torch `abs() ** 2 . sum(1)` into the power matrix, in user chunks where the complex
               tensor of all users is not kept (a chunk's tensor is resident; the result is the same [n, R, n_taps])
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1, two passes; spread = the difference between
the passes of one route).  One JSON line per shape: the protocol's fields per route, the ratios (a)/(c), (b)/(c), (d)/(a),
whether (a) and (b) stay within (c) plus (c)'s spread, the output bytes of every route, and the largest deviation of (a)
from (d) and of (b) from the row sum of (a) relative to the value.  Without a GPU the tool fails.
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
from angle_delay_bench import SHAPES  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=3, help="back-to-back launches of a route per timing")
    ap.add_argument("--rounds", type=int, default=2, help="timings per route and pass: 2 passes x rounds x launches launches in all")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    lib, L = eng.lib, args.paths
    stream = eng._stream_ptr()
    lines = []
    for name, bs, ue, K, taps, rows, users, chunk in SHAPES:
        if name not in args.shapes.split(","):
            continue
        n = max(1, int(users * args.scale))
        chunk = min(chunk * 4, n)                       # the chunk tensor here is [chunk, M_rx, R, n_taps], not [.., K]
        rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234, all_valid=True))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        ps, stage1 = prep.params_struct, ab.stage1(eng, prep)
        flagged = {}
        for route, bits in (("power", nat.FLAG_ANGLE_DELAY_POWER), ("profile", nat.FLAG_ANGLE_DELAY_POWER | nat.FLAG_ANGLE_DELAY_PROFILE)):
            flagged[route] = nat.DmxParams.from_buffer_copy(ps)
            flagged[route].flags |= bits
        m_tx, m_rx = int(np.prod(bs)), int(np.prod(ue))
        cb = eng._codebook(dm.dft_codebook(bs)[:rows], m_tx, min_beams=1) if rows else None
        R = rows if rows else m_tx
        cbp = C.c_void_p(cb.data_ptr()) if rows else None
        wsp = C.c_void_p(prep.workspace.data_ptr())
        nb = int(lib.dmx_beam_workspace_bytes(C.byref(ps), n, L, R)) if rows else 0
        bws = eng._scratch(nb) if rows else None
        bwp = C.c_void_p(bws.data_ptr()) if rows else None
        out = dict(power=torch.empty((n, R, taps), dtype=torch.float32, device=eng.device),
                   profile=torch.empty((n, taps), dtype=torch.float32, device=eng.device),
                   complex=torch.empty((n, m_rx, R, taps), dtype=torch.complex64, device=eng.device),
                   unfused=torch.empty((n, R, taps), dtype=torch.float32, device=eng.device))
        x_chunk = torch.empty((chunk, m_rx, R, taps), dtype=torch.complex64, device=eng.device)

        def call(prm, begin, count, dst):
            nat.check(lib.dmx_channels_angle_delay(C.byref(prm), wsp, n, L, begin, count, cbp, R, bwp, nb, K, taps,
                                                   C.c_void_p(dst.data_ptr()), stream), "dmx_channels_angle_delay")

        def route(which):
            def run():
                stage1()
                call(flagged.get(which, ps), 0, n, out[which])
            return run

        def unfused():
            stage1()
            for b in range(0, n, chunk):
                cnt = min(chunk, n - b)
                call(ps, b, cnt, x_chunk)
                v = torch.view_as_real(x_chunk[:cnt])
                torch.sum((v * v).sum(-1), dim=1, out=out["unfused"][b:b + cnt])

        fns = [("power", route("power")), ("profile", route("profile")), ("complex", route("complex")), ("unfused", unfused)]
        routes = [(rn, fn, ab.device(args.launches), ab.device(1)) for rn, fn in fns]
        rec = dict(shape=name, bs=bs, ue=ue, K=K, n_fft=K, n_taps=taps, rows=R, codebook=bool(rows), users=n, paths=L,
                   chunk_users=chunk, launches_per_route=2 * args.rounds * args.launches,
                   out_bytes={k: int(v.numel() * v.element_size()) for k, v in out.items()})
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        c_ms, c_spread = rec["complex_avg_ms"], rec["complex_spread_ms"]
        rec["power_over_complex"] = round(rec["power_avg_ms"] / c_ms, 4)
        rec["profile_over_complex"] = round(rec["profile_avg_ms"] / c_ms, 4)
        rec["unfused_over_power"] = round(rec["unfused_avg_ms"] / rec["power_avg_ms"], 3)
        rec["power_within_complex_plus_spread"] = bool(rec["power_avg_ms"] <= c_ms + c_spread)
        rec["profile_within_complex_plus_spread"] = bool(rec["profile_avg_ms"] <= c_ms + c_spread)
        live = out["unfused"] > 0
        rec["max_rel_dev_power_vs_unfused"] = float(((out["power"] - out["unfused"]).abs()[live] / out["unfused"][live]).max())
        row_sum = out["power"].double().sum(1)
        rec["max_rel_dev_profile_vs_row_sum"] = float(((out["profile"].double() - row_sum).abs() / row_sum.clamp_min(1e-300)).max())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del out, x_chunk, prep, rays, bws
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
