#!/usr/bin/env python3
"""Codebook rate under the linear MMSE receiver against the joint receiver of the same build and against the unfused twin,
alternating in ONE process: `python tools/mmse_rate_bench.py [--out profiles/r19_mmse_rate_bench.jsonl]`.

For each shape, on the same uploaded rays (in HBM), stage 1 included in every route:
  (a) mmse    dmx_path_prep + dmx_codebook_rate with DMX_FLAG_RX_LINEAR_MMSE over all users: rate and pmi, no rate_c
  (b) joint   the same call without the flag
  (c) twin    dmx_path_prep + per user chunk: dmx_channels_fd_beams of the flattened codebook into a resident tensor
              [chunk, M_rx, C L, K], the L x L Gram by torch.einsum, torch.linalg.inv of I + s G, -log2 of its diagonal summed
              over the layers, the mean over the subcarriers, max and argmax over the codewords.  On the first `twin users` of
              the shape only; `speedup_per_user` compares time per user - an extrapolation, not a like-for-like run
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per shape: the protocol's
fields per route (`<route>_spread_ms` is the difference between the two passes' averages), `mmse_over_joint` = (a) / (b) from
the two-pass averages, the largest deviation between (a) and (c) in bit and the share of users with the same PMI, the mean
rate under either receiver and the share of users whose PMI differs between them.  The kernel's share of route (a) comes from a kernel trace of its own run
(`--routes mmse` under the profiler), not from this tool.  Without a GPU the tool fails.
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
SHAPES = [("headline_L2_C32", [64, 4], [2, 2], 512, 32, 2, 100_000, 2_000, 500),
          ("headline_L4_C16", [64, 4], [2, 2], 512, 16, 4, 100_000, 2_000, 500),
          ("defaults_2x1_L2_C4", [8, 1], [2, 1], 512, 4, 2, 200_000, 20_000, 5_000)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--snr-db", type=float, default=100.0)
    ap.add_argument("--launches", type=int, default=3, help="back-to-back launches of a route per timing")
    ap.add_argument("--rounds", type=int, default=2, help="timings per route and pass: 2 passes x rounds x launches launches in all")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--routes", default="mmse,joint,twin")
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

        def mmse():
            stage1()
            out["mmse"] = eng.codebook_rate(prep, W, args.snr_db, receiver="mmse")

        def joint():
            stage1()
            out["joint"] = eng.codebook_rate(prep, W, args.snr_db)

        def twin():
            stage1()
            for b in range(0, n_twin, chunk):
                cnt = min(chunk, n_twin - b)
                eng.channels(prep, out=Y[:cnt], user_begin=b, user_count=cnt, tx_codebook=flat)
                E = Y[:cnt].reshape(cnt, m_rx, n_cw, n_layers, K)
                G = torch.einsum("urcik,urcjk->uckij", E.conj(), E)
                d = torch.diagonal(torch.linalg.inv(eye + s * G), dim1=-2, dim2=-1).real
                rate_c = (-torch.log2(d).sum(dim=-1)).mean(dim=-1)
                r_ref[b:b + cnt], p_ref[b:b + cnt] = rate_c.max(dim=1)

        want = args.routes.split(",")
        routes = [(rn, fn, ab.device(args.launches), ab.device(1)) for rn, fn in (("mmse", mmse), ("joint", joint), ("twin", twin))
                  if rn in want]
        rec = dict(shape=name, bs=bs, ue=ue, K=K, codewords=n_cw, layers=n_layers, users=n, twin_users=n_twin, paths=L,
                   snr_db=args.snr_db, chunk_users=chunk, launches_per_route=2 * args.rounds * args.launches)
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        have = {r[0] for r in routes}
        if {"mmse", "joint"} <= have:
            rec["mmse_over_joint"] = round(rec["mmse_avg_ms"] / rec["joint_avg_ms"], 4)
            rec["mean_rate_mmse"] = float(out["mmse"][0].double().mean())
            rec["mean_rate_joint"] = float(out["joint"][0].double().mean())
            rec["other_pmi_share"] = float((out["mmse"][1] != out["joint"][1]).double().mean())
        if {"mmse", "twin"} <= have:
            rec["speedup_per_user"] = round((rec["twin_avg_ms"] / n_twin) / (rec["mmse_avg_ms"] / n), 3)
            rec["like_for_like"] = n_twin == n
            rec["max_dev_bit"] = float((out["mmse"][0][:n_twin] - r_ref).abs().max())
            rec["same_pmi_share"] = float((out["mmse"][1][:n_twin].long() == p_ref).double().mean())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Y, prep, rays, out, r_ref, p_ref
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
