#!/usr/bin/env python3
"""Angle-delay representation: the fused call against the beam-space tensor + torch.fft, alternating in ONE process:
`python tools/angle_delay_bench.py [--out profiles/r9_angle_delay_bench.jsonl]`.

For each shape, on the same uploaded rays, stage 1 included in both:
  (a) fused   dmx_path_prep + dmx_channels_angle_delay                        (no [n, M_rx, R, K] tensor)
  (b) twin    dmx_path_prep + per user chunk: dmx_channels_fd_beams (dmx_channels_fd without a codebook) into a resident
              tensor, torch.fft.ifft(..., n=n_fft, dim=-1)[..., :n_taps] copied into the result
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per shape: the protocol's
fields per route, their ratio, the largest
deviation between the two results per user peak (and in units of the 5e-5 bound of the tests), the output bytes per second
of the fused route against the HBM peak (8 TB/s), and its algorithmic flops (complex product 6, complex multiply-add 8:
n R n_taps P (6 + 8 M_rx)) as a share of the fp32 vector peak (256 CUs x 4 SIMDs x 64 flop per clock at 2.4 GHz) - both
over the time of the whole route, stage 1 and the projection included.  Without a GPU the tool fails.
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

# (name, BS panel, UE panel, K = n_fft, taps, rows of dm.dft_codebook (0: no codebook, the BS elements), users, users per
# chunk of route (b)): the headline panel with 64 and with all 256 DFT beams, DeepMIMO's default arrays
SHAPES = [("headline_R64", [64, 4], [2, 2], 512, 32, 64, 100_000, 5_000),
          ("headline_R256", [64, 4], [2, 2], 512, 32, 256, 100_000, 2_000),
          ("defaults_dft", [8, 1], [1, 1], 512, 32, 8, 200_000, 50_000),
          ("defaults_antenna", [8, 1], [1, 1], 512, 32, 0, 200_000, 50_000)]
FP32_VALU_PEAK = 256 * 4 * 64 * 2.4e9
HBM_PEAK = 8.0e12
TOL_REL = 5e-5


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
        chunk = min(chunk, n)
        rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234, all_valid=True))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        ps, stage1 = prep.params_struct, ab.stage1(eng, prep)
        m_tx, m_rx = int(np.prod(bs)), int(np.prod(ue))
        cb = eng._codebook(dm.dft_codebook(bs)[:rows], m_tx, min_beams=1) if rows else None
        R = rows if rows else m_tx
        cbp = C.c_void_p(cb.data_ptr()) if rows else None
        wsp = C.c_void_p(prep.workspace.data_ptr())
        nb_full = int(lib.dmx_beam_workspace_bytes(C.byref(ps), n, L, R)) if rows else 0
        nb_chunk = int(lib.dmx_beam_workspace_bytes(C.byref(ps), chunk, L, R)) if rows else 0
        bws_full = eng._scratch(nb_full) if rows else None
        bws_chunk = eng._scratch(nb_chunk) if rows else None
        Y = torch.empty((chunk, m_rx, R, K), dtype=torch.complex64, device=eng.device)
        x_fused = torch.empty((n, m_rx, R, taps), dtype=torch.complex64, device=eng.device)
        x_twin = torch.empty((n, m_rx, R, taps), dtype=torch.complex64, device=eng.device)

        def fused():
            stage1()
            nat.check(lib.dmx_channels_angle_delay(C.byref(ps), wsp, n, L, 0, n, cbp, R,
                                                   C.c_void_p(bws_full.data_ptr()) if rows else None, nb_full, K, taps,
                                                   C.c_void_p(x_fused.data_ptr()), stream), "dmx_channels_angle_delay")

        def twin():
            stage1()
            for b in range(0, n, chunk):
                cnt = min(chunk, n - b)
                if rows:
                    nat.check(lib.dmx_channels_fd_beams(C.byref(ps), wsp, n, L, b, cnt, cbp, R, C.c_void_p(bws_chunk.data_ptr()),
                                                        nb_chunk, C.c_void_p(Y.data_ptr()), stream), "dmx_channels_fd_beams")
                else:
                    nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, b, cnt, C.c_void_p(Y.data_ptr()), 0, stream), "dmx_channels_fd")
                x_twin[b:b + cnt] = torch.fft.ifft(Y[:cnt], n=K, dim=-1)[..., :taps]

        routes = [(rn, fn, ab.device(args.launches), ab.device(1)) for rn, fn in (("fused", fused), ("twin", twin))]
        out_bytes = n * m_rx * R * taps * 8
        rec = dict(shape=name, bs=bs, ue=ue, K=K, n_fft=K, n_taps=taps, rows=R, codebook=bool(rows), users=n, paths=L,
                   chunk_users=chunk, out_bytes=out_bytes, twin_tensor_bytes=n * m_rx * R * K * 8,
                   launches_per_route=2 * args.rounds * args.launches, fused_flops=n * R * taps * L * (6 + 8 * m_rx))
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        rec["speedup"] = round(rec["twin_avg_ms"] / rec["fused_avg_ms"], 3)
        rec["faster_by_more_than_the_spread"] = bool(rec["twin_avg_ms"] - rec["fused_avg_ms"] > rec["twin_spread_ms"] + rec["fused_spread_ms"])
        peak = x_twin.abs().reshape(n, -1).amax(dim=1).clamp_min(1e-38)
        dev = ((x_fused - x_twin).abs().reshape(n, -1).amax(dim=1) / peak).max()
        rec["max_dev_per_user_peak"] = float(dev)
        rec["max_dev_over_bound"] = round(float(dev) / TOL_REL, 4)
        sec = rec["fused_avg_ms"] * 1e-3
        rec["fused_out_bytes_per_s"] = round(out_bytes / sec, 1)
        rec["fused_out_share_of_hbm_peak"] = round(out_bytes / sec / HBM_PEAK, 5)
        rec["fused_share_of_fp32_valu_peak"] = round(rec["fused_flops"] / sec / FP32_VALU_PEAK, 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Y, x_fused, x_twin, prep, rays, bws_full, bws_chunk
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
