#!/usr/bin/env python3
"""Subband PMI per user: the subband call against the wideband call (its floor) and against one wideband call per subband,
alternating in ONE process: `python tools/subband_pmi_bench.py [--out profiles/r11_subband_pmi_bench.jsonl]`.

For each shape, on the same uploaded rays and the same workspace, stage 1 included in every route:
  (a) subbands  dmx_path_prep + dmx_codebook_rate_subbands over all users: rate, pmi, rate_sb, pmi_sb (no per-codeword output)
  (b) wideband  dmx_path_prep + dmx_codebook_rate on the whole selection: rate, pmi - the same products without the subbands,
                the floor of (a)
  (c) loop      what the subband part costs without the subband call: per subband dmx_path_prep + dmx_codebook_rate on the
                sub-selection sc[s B : (s + 1) B], n_sb preparations and n_sb projections of the codebook.  The sub-selection
                is set in the parameter block of the one preparation (pointer and count) and restored afterwards, which is
                what n_sb preparations of their own compute, without n_sb workspaces
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per shape: the protocol's
fields per route, (a) / (b) and (c) / (a), whether (a)
is faster than (c) by more than the two spreads, and whether the subband outputs of (a) equal the results of (c) bit for bit.
Without a GPU the tool fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

# (name, BS panel, UE panel, K, codewords, layers, subband size, users)
SHAPES = [("headline_C64_B32", [64, 4], [2, 2], 512, 64, 1, 32, 100_000),
          ("headline_C64_B4", [64, 4], [2, 2], 512, 64, 1, 4, 100_000),
          ("defaults_C8_B32", [8, 1], [1, 1], 512, 8, 1, 32, 200_000)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--snr-db", type=float, default=100.0)
    ap.add_argument("--launches", type=int, default=3, help="back-to-back launches of a route per timing")
    ap.add_argument("--rounds", type=int, default=2, help="timings per route and pass: 2 passes x rounds x launches launches in all")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--routes", default="subbands,wideband,loop")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    L = args.paths
    lines = []
    for name, bs, ue, K, n_cw, n_layers, B, users in SHAPES:
        if name not in args.shapes.split(","):
            continue
        n = max(1, int(users * args.scale))
        rays = eng.upload_rays(onp.synth_rays(n, L, seed=1234, all_valid=True))
        p = dm.ChannelGenParameters()
        p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
        p.ofdm.selected_subcarriers = np.arange(K)
        p.validate(n)
        prep = eng.prepare(rays, p, want_side="light")
        ps, stage1 = prep.params_struct, ab.stage1(eng, prep)
        m_tx = int(np.prod(bs))
        W = torch.from_numpy(dm.dft_codebook(bs)[:n_cw * n_layers].reshape(n_cw, n_layers, m_tx)).to(eng.device)
        sel_ptr, n_sb = int(ps.selected_subcarriers), (K + B - 1) // B
        out = {}
        loop_rate = torch.empty((n, n_sb), dtype=torch.float32, device=eng.device)
        loop_pmi = torch.empty((n, n_sb), dtype=torch.int32, device=eng.device)

        def subbands():
            stage1()
            out["rate"], out["pmi"], out["rate_sb"], out["pmi_sb"] = eng.codebook_rate_subbands(prep, W, args.snr_db, B)

        def wideband():
            stage1()
            out["wide_rate"], out["wide_pmi"] = eng.codebook_rate(prep, W, args.snr_db)

        def loop():
            try:
                for s in range(n_sb):
                    ps.selected_subcarriers, ps.n_selected = sel_ptr + 4 * s * B, min(B, K - s * B)
                    stage1()
                    r, pm = eng.codebook_rate(prep, W, args.snr_db)
                    loop_rate[:, s], loop_pmi[:, s] = r, pm
            finally:
                ps.selected_subcarriers, ps.n_selected = sel_ptr, K

        want = args.routes.split(",")
        routes = [(rn, fn, ab.device(args.launches), ab.device(1))
                  for rn, fn in (("subbands", subbands), ("wideband", wideband), ("loop", loop)) if rn in want]
        rec = dict(shape=name, bs=bs, ue=ue, K=K, codewords=n_cw, layers=n_layers, subband_size=B, subbands=n_sb, users=n, paths=L,
                   snr_db=args.snr_db, launches_per_route=2 * args.rounds * args.launches)
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        have = {r[0] for r in routes}
        if "subbands" in have:
            rec["mean_rate"] = float(out["rate"].double().mean())
            rec["mean_rate_sb"] = float(out["rate_sb"].double().mean())
        if {"subbands", "wideband"} <= have:
            rec["subbands_over_wideband"] = round(rec["subbands_avg_ms"] / rec["wideband_avg_ms"], 4)
            rec["wideband_max_dev_bit"] = float((out["rate"] - out["wide_rate"]).abs().max())
            rec["same_wideband_pmi_share"] = float((out["pmi"] == out["wide_pmi"]).double().mean())
        if {"subbands", "loop"} <= have:
            rec["loop_over_subbands"] = round(rec["loop_avg_ms"] / rec["subbands_avg_ms"], 3)
            rec["subbands_faster_than_loop_beyond_spreads"] = bool(
                rec["loop_avg_ms"] - rec["subbands_avg_ms"] > rec["loop_spread_ms"] + rec["subbands_spread_ms"])
            rec["subbands_equal_loop_bits"] = bool(torch.equal(out["rate_sb"], loop_rate) and torch.equal(out["pmi_sb"], loop_pmi))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del prep, rays, out, loop_rate, loop_pmi
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
