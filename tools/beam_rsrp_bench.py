#!/usr/bin/env python3
"""Power-averaged beam sweep (RSRP): what `ChannelEngine.beam_power(metric="power")` costs beside the amplitude call it
shares a kernel with and beside the unfused way, in ONE process:
`python tools/beam_rsrp_bench.py [--out profiles/r17_beam_rsrp_bench.jsonl]`.

Two shapes, the ray matrices in HBM, 25 paths, K = 512, 100k users: the headline shape - BS 8 x 8, UE 2 x 2 - with the
first 64 beams of the BS DFT codebook, and DeepMIMO's default arrays - BS 8 x 1, UE 1 x 1 - with their 8 DFT beams.  On the
records of ONE preparation per shape:
  (a) power      eng.beam_power(prep, F, metric="power")            mean |F H|^2 [n, B] and its argmax
  (b) amplitude  eng.beam_power(prep, F)                            mean |F H|   [n, B] and its argmax: the same matrix-core
                 work plus two square roots per (row pair, subcarrier)
  (c) unfused    per chunk of users the beam-space tensor [chunk, M_rx, B, K] of dmx_channels_fd_beams, then torch
                 abs() ** 2 and the mean over rx and k - on the first `--unfused-users` users only (the tensor is
                 M_rx * B * K * 8 bytes per user).  Its time per user times n is an EXTRAPOLATION.
All three stop at a tensor in HBM, so the protocol of `tools/ab_protocol.py` runs with its device timer.  One JSON line per
shape: the protocol's fields per route, the times per user, (a)/(b), (a)/(c) per user, whether (a) - (b) exceeds the
pass-to-pass spreads of both, and how far (a) and (c) differ per user.  Without a GPU the tool fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd.dataset import _engine  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

SHAPES = {"headline": ([8, 8], [2, 2], 64), "default_arrays": ([8, 1], [1, 1], 8)}


def unfused(eng, prep, F_dev, users, chunk):
    """mean power [users, B] float32 in HBM the unfused way: the beam-space tensor per chunk of users, then torch"""
    out = torch.empty((users, F_dev.shape[0]), dtype=torch.float32, device=eng.device)
    for b in range(0, users, chunk):
        cnt = min(chunk, users - b)
        Y = eng.channels(prep, user_begin=b, user_count=cnt, tx_codebook=F_dev)          # [cnt, M_rx, B, K]
        out[b:b + cnt] = (Y.real ** 2 + Y.imag ** 2).mean(dim=(1, 3))
    return out


def measure(name, args):
    bs, ue, nb = SHAPES[name]
    n, L, K = args.users, args.paths, args.subcarriers
    B = min(nb, args.beams)
    n_c = min(args.unfused_users, n)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.ofdm.selected_subcarriers = np.arange(K)
    rays = onp.synth_rays(n, L, seed=1234, all_valid=True)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays({k: torch.from_numpy(v).cuda() for k, v in rays.items()}), p.validate(n), want_side="light")
    F_dev = eng._codebook(dm.dft_codebook(bs)[:B], bs[0] * bs[1], min_beams=1)
    m_rx = ue[0] * ue[1]
    rec = dict(shape=name, rays="device", bs=bs, ue=ue, K=K, users=n, paths=L, B=B, unfused_users=n_c,
               unfused_chunk=args.unfused_chunk, beam_space_bytes_per_user=m_rx * B * K * 8, launches_per_reading=args.launches,
               readings_per_route=2 * args.rounds)
    # the two ways agree per user: (a)'s means against (c)'s, relative to the user's largest
    P_a = eng.beam_power(prep, F_dev, metric="power")[0][:n_c].cpu().numpy()
    P_c = unfused(eng, prep, F_dev, n_c, args.unfused_chunk).cpu().numpy()
    peak = np.maximum(P_c.max(axis=1), 1e-300)
    rec["power_vs_unfused_worst_rel_err"] = float((np.abs(P_a - P_c).max(axis=1) / peak).max())
    del P_a, P_c
    torch.cuda.empty_cache()
    routes = [
        ("power", n, lambda: eng.beam_power(prep, F_dev, metric="power")),
        ("amplitude", n, lambda: eng.beam_power(prep, F_dev)),
        ("unfused", n_c, lambda: unfused(eng, prep, F_dev, n_c, args.unfused_chunk)),
    ]
    timer = ab.device(args.launches)
    ts = ab.alternate([(rn, fn, timer, timer) for rn, _, fn in routes], args.rounds)
    rec.update(ab.summaries(ts, digits=4, raw=True))
    for rn, users, _ in routes:
        rec[f"{rn}_us_per_user"] = round(1e3 * rec[f"{rn}_avg_ms"] / users, 5)
        rec[f"{rn}_spread_us_per_user"] = round(1e3 * rec[f"{rn}_spread_ms"] / users, 5)
    rec["unfused_extrapolated_ms"] = round(rec["unfused_us_per_user"] * n / 1e3, 3)
    rec["power_over_amplitude"] = round(rec["power_avg_ms"] / rec["amplitude_avg_ms"], 4)
    rec["power_over_unfused_per_user"] = round(rec["power_us_per_user"] / rec["unfused_us_per_user"], 4)
    rec["power_minus_amplitude_ms"] = round(rec["power_avg_ms"] - rec["amplitude_avg_ms"], 4)
    rec["power_slower_than_amplitude_by_more_than_the_spreads"] = bool(
        rec["power_minus_amplitude_ms"] > rec["power_spread_ms"] + rec["amplitude_spread_ms"])
    return json.dumps(rec)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--subcarriers", type=int, default=512)
    ap.add_argument("--beams", type=int, default=64, help="at most this many beams of the BS DFT codebook")
    ap.add_argument("--shapes", default="headline,default_arrays")
    ap.add_argument("--unfused-users", type=int, default=8192, help="users route (c) runs on")
    ap.add_argument("--unfused-chunk", type=int, default=2048, help="users per beam-space tensor of route (c)")
    ap.add_argument("--launches", type=int, default=3, help="back-to-back launches per reading")
    ap.add_argument("--rounds", type=int, default=5, help="readings per route and pass")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("beam_rsrp_bench: no GPU")
    lines = []
    for name in args.shapes.split(","):
        lines.append(measure(name, args))
        print(lines[-1], flush=True)
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
