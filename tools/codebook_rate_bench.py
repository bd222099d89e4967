#!/usr/bin/env python3
"""Codebook-precoded rate and PMI per user: the fused route against the beam-space tensor + torch, alternating in ONE process:
`python tools/codebook_rate_bench.py [--out profiles/r10_codebook_rate_bench.jsonl]`.

For each shape, on the same uploaded rays:
  (a) fused   dmx_path_prep + dmx_codebook_rate over all users (the engine's user blocks keep the beam workspace within
              1 GiB): rate and pmi, no rate_c, no beam-space tensor
  (b) twin    dmx_path_prep + per user chunk: dmx_channels_fd_beams of the flattened codebook into a resident tensor
              [chunk, M_rx, C L, K], then log2(1 + s sum_rx |.|^2) at L = 1, or the L x L Gram by torch.einsum and
              torch.linalg.slogdet of I + s G, the mean over the subcarriers, max and argmax over the codewords.  1 MB per user
              at 64 rows x 4 x 512, so the twin runs on the first `twin users` of the shape only; `speedup_per_user` compares
              time per user - an extrapolation where the counts differ, not a like-for-like run
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per shape: the protocol's
fields per route, the algorithmic flops of
k10_codebook_rate (complex product 6, complex multiply-add 8; the projection not counted) and, from the time of the whole
fused route, their share of the fp32 vector peak (256 CUs x 4 SIMDs x 64 flop per clock at 2.4 GHz), the largest deviation
between the two rates in bit and the share of users with the same PMI.  Without a GPU the tool fails.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

# (name, BS panel, UE panel, K, codewords, layers, users, twin users, users per chunk of the twin)
SHAPES = [("headline_L1_C64", [64, 4], [2, 2], 512, 64, 1, 100_000, 4_000, 1_000),
          ("headline_L2_C32", [64, 4], [2, 2], 512, 32, 2, 100_000, 2_000, 500),
          ("defaults_K512", [8, 1], [1, 1], 512, 8, 1, 200_000, 200_000, 25_000),
          ("defaults_K1", [8, 1], [1, 1], 1, 8, 1, 200_000, 200_000, 200_000)]
FP32_VALU_PEAK = 256 * 4 * 64 * 2.4e9


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--snr-db", type=float, default=100.0)
    ap.add_argument("--launches", type=int, default=3, help="back-to-back launches of a route per timing")
    ap.add_argument("--rounds", type=int, default=2, help="timings per route and pass: 2 passes x rounds x launches launches in all")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--routes", default="fused,twin")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    L = args.paths
    snr = 10.0 ** (args.snr_db / 10.0)
    lines = []
    for name, bs, ue, K, n_cw, n_layers, users, twin_users, chunk in SHAPES:
        if name not in args.shapes.split(","):
            continue
        n = max(1, int(users * args.scale))
        n_twin = min(n, max(1, int(twin_users * args.scale)))
        chunk = min(chunk, n_twin)
        rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234, all_valid=True))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        stage1 = ab.stage1(eng, prep)
        m_tx, m_rx = int(np.prod(bs)), int(np.prod(ue))
        rows = n_cw * n_layers
        W = torch.from_numpy(dm.dft_codebook(bs)[:rows].reshape(n_cw, n_layers, m_tx)).to(eng.device)
        flat = W.reshape(rows, m_tx)
        Y = torch.empty((chunk, m_rx, rows, K), dtype=torch.complex64, device=eng.device)
        out = {}
        r_ref = torch.empty((n_twin,), dtype=torch.float32, device=eng.device)
        p_ref = torch.empty((n_twin,), dtype=torch.int64, device=eng.device)
        eye = torch.eye(n_layers, dtype=torch.complex64, device=eng.device)
        s = snr / n_layers

        def fused():
            stage1()
            out["rate"], out["pmi"] = eng.codebook_rate(prep, W, args.snr_db)

        def twin():
            stage1()
            for b in range(0, n_twin, chunk):
                cnt = min(chunk, n_twin - b)
                eng.channels(prep, out=Y[:cnt], user_begin=b, user_count=cnt, tx_codebook=flat)
                if n_layers == 1:
                    rate_c = torch.log2(1.0 + s * (Y[:cnt].real ** 2 + Y[:cnt].imag ** 2).sum(dim=1)).mean(dim=-1)
                else:
                    E = Y[:cnt].reshape(cnt, m_rx, n_cw, n_layers, K)
                    G = torch.einsum("urcik,urcjk->uckij", E.conj(), E)
                    rate_c = (torch.linalg.slogdet(eye + s * G)[1] / math.log(2.0)).mean(dim=-1)
                r_ref[b:b + cnt], p_ref[b:b + cnt] = rate_c.max(dim=1)

        want = args.routes.split(",")
        routes = [(rn, fn, ab.device(args.launches), ab.device(1)) for rn, fn in (("fused", fused), ("twin", twin)) if rn in want]
        rec = dict(shape=name, bs=bs, ue=ue, K=K, codewords=n_cw, layers=n_layers, users=n, twin_users=n_twin, paths=L,
                   snr_db=args.snr_db, chunk_users=chunk, beam_tensor_bytes_per_user=m_rx * rows * K * 8,
                   row_table_bytes_per_user=rows * L * 8, launches_per_route=2 * args.rounds * args.launches)
        # per (codeword, subcarrier): rows_pair over the layers (per path one product per row and M_rx multiply-adds), the
        # Gram's upper triangle, the elimination is not counted
        rec["fused_flops"] = n * K * n_cw * (n_layers * L * (6 + 8 * m_rx) + 8 * m_rx * n_layers * (n_layers + 1) // 2)
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        have = {r[0] for r in routes}
        if "fused" in have:
            rec["fused_share_of_fp32_valu_peak"] = round(rec["fused_flops"] / (rec["fused_avg_ms"] * 1e-3) / FP32_VALU_PEAK, 4)
            rec["mean_rate"] = float(out["rate"].double().mean())
        if {"fused", "twin"} <= have:
            rec["speedup_per_user"] = round((rec["twin_avg_ms"] / n_twin) / (rec["fused_avg_ms"] / n), 3)
            rec["like_for_like"] = n_twin == n
            rec["max_dev_bit"] = float((out["rate"][:n_twin] - r_ref).abs().max())
            rec["same_pmi_share"] = float((out["pmi"][:n_twin].long() == p_ref).double().mean())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Y, prep, rays, out, r_ref, p_ref
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
