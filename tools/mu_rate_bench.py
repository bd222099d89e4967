#!/usr/bin/env python3
"""Multi-user downlink rates: what `Dataset.compute_mu_rate` costs beside its unfused twin and beside the single-user call
it is built like, in ONE process: `python tools/mu_rate_bench.py [--out profiles/r18_mu_rate_bench.jsonl]`.

Two shapes, one JSON line each, the ray matrices in HBM (torch), `channel_output = 'torch'`, the DFT codebook of the BS
panel, the beam of each user from `compute_beam_power(..., metric="power", return_best=True)`, the users in groups of G in
their stored order:
  headline   BS 8 x 8, UE 2 x 2, K = 512, 25 paths, 100k users, G = 4
  default    BS 8 x 1, UE 1 x 1 (DeepMIMO's default arrays), K = 512, 25 paths, 200k users, G = 4
and per shape three routes:
  (a) mu        ds.compute_mu_rate(F, beams, groups, p, snr_db=...)       [n]: G precoded views of the users, G stage-1 passes
                and the multi-cell rate kernel per block of users
  (b) unfused   what the package could do before: stage 1, then per chunk of users the channel tensor [chunk, M_rx, M_tx, K],
                a gather of the group's codewords, torch.einsum and two torch.linalg.slogdet - on the first
                `--unfused-users` users only (the tensor is 1 MB per user at the headline shape).  Its time per user times n
                is an EXTRAPOLATION.
  (c) single    ds.with_tx_precoder(F, beams, p).compute_rate(snr_db=...)  [n]: the user alone on its beam at the full power,
                the floor of (a): one view, one stage-1 pass, the single-link rate kernel.
All three run under the host timer of `tools/ab_protocol.py` (building the views is part of (a) and (c)), warm-up included.
A line also holds the split of (a) into its parts - the departure angles (one full stage-1 pass), the view arithmetic (G
precoded ray matrices per block), the G light stage-1 passes and the rate kernel - from `--split-runs` runs of their own with
a device synchronisation around every part, and how far (a) and (b) differ per user.  Without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd import dataset as dsm  # noqa: E402
from deepmimo_amd.combiner import mu_partners  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

SHAPES = {"headline": dict(bs=[8, 8], ue=[2, 2], users=100_000), "default": dict(bs=[8, 1], ue=[1, 1], users=200_000)}


def unfused(ds, p, F, beams, groups, snr_db, chunk):
    """rate [n] float32 in HBM the unfused way: the channel tensor per chunk of users, then torch"""
    ds._call_params(p)
    np.random.seed(1001)
    eng, prep = ds._run_prep(want_side="light")
    n = prep.n_ue
    partners, size, scheduled = mu_partners(groups, n)
    idx = np.concatenate([np.where(scheduled, beams, -1)[:, None], np.where(partners >= 0, beams[np.maximum(partners, 0)], -1)], axis=1)
    amp = np.where(idx >= 0, 1.0, 0.0) * np.sqrt(10 ** (snr_db / 10) / np.maximum(size, 1))[:, None]          # [n, G]
    F_dev = torch.from_numpy(F.astype(np.complex64)).to(eng.device)
    idx_dev = torch.from_numpy(np.maximum(idx, 0)).to(eng.device)
    amp_dev = torch.from_numpy(amp.astype(np.float32)).to(eng.device)
    out = torch.empty(n, dtype=torch.float32, device=eng.device)
    for b in range(0, n, chunk):
        cnt = min(chunk, n - b)
        H = eng.channels(prep, user_begin=b, user_count=cnt)                                # [cnt, M_rx, M_tx, K]
        Wg = F_dev[idx_dev[b:b + cnt]] * amp_dev[b:b + cnt, :, None]                        # [cnt, G, M_tx]: the gather
        Y = torch.einsum("urtk,ugt->ukrg", H, Wg)                                           # [cnt, K, M_rx, G]
        eye = torch.eye(Y.shape[2], dtype=Y.dtype, device=Y.device)
        N = eye + Y[..., 1:] @ Y[..., 1:].conj().transpose(-1, -2)
        A = N + Y[..., :1] @ Y[..., :1].conj().transpose(-1, -2)
        out[b:b + cnt] = ((torch.linalg.slogdet(A)[1] - torch.linalg.slogdet(N)[1]) / np.log(2.0)).mean(dim=1)
    return out


def split_of_mu(call, runs):
    """mean milliseconds of the parts of one `compute_mu_rate` call over `runs` calls, a device synchronisation around each"""
    spent = {"angles": 0.0, "views": 0.0, "stage1": 0.0, "rate_kernel": 0.0}

    def timed(part, real):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = real(*a, **k)
            torch.cuda.synchronize()
            spent[part] += (time.perf_counter() - t0) * 1e3
            return res
        return wrapper
    saved = (dm.Dataset._tx_departure_angles, dm.Dataset._tx_view, dm.Dataset._run_prep, ChannelEngine.cell_rate)
    run_prep = timed("stage1", saved[2])
    try:
        dm.Dataset._tx_departure_angles = timed("angles", saved[0])                          # its own stage 1 runs untimed
        dm.Dataset._tx_view = timed("views", saved[1])
        dm.Dataset._run_prep = lambda self, want_side=True, **k: (run_prep if want_side == "light" else saved[2])(self, want_side=want_side, **k)
        ChannelEngine.cell_rate = timed("rate_kernel", saved[3])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(runs):
            call()
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3 / runs
    finally:
        dm.Dataset._tx_departure_angles, dm.Dataset._tx_view, dm.Dataset._run_prep, ChannelEngine.cell_rate = saved
    rec = {f"mu_split_{k}_ms": round(v / runs, 3) for k, v in spent.items()}
    rec["mu_split_total_ms"] = round(total, 3)
    rec["mu_split_rest_ms"] = round(total - sum(spent.values()) / runs, 3)
    return rec


def measure(name, args):
    shape = SHAPES[name]
    n = min(shape["users"], args.users) if args.users else shape["users"]
    L, K, G = args.paths, args.subcarriers, args.group
    n -= n % G
    n_b = min(args.unfused_users - args.unfused_users % G, n)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(shape["bs"]), np.array(shape["ue"])
    p.ofdm.selected_subcarriers = np.arange(K)
    p.num_paths = L
    F = dm.dft_codebook(shape["bs"]).astype(np.complex128)
    rays = onp.synth_rays(n, L, seed=1234, all_valid=True)
    ds = dm.Dataset({k: torch.from_numpy(v).cuda() for k, v in rays.items()})
    _, best = ds.compute_beam_power(F, p, return_best=True, metric="power")
    beams = np.nan_to_num(best, nan=0.0).astype(np.int64)
    groups = np.arange(n).reshape(-1, G)
    ds_b = ds.subset(np.arange(n_b))
    snr_db = args.snr_db
    routes = [
        ("mu", n, lambda: ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db)),
        ("unfused", n_b, lambda: unfused(ds_b, p, F, beams[:n_b], groups[:n_b // G], snr_db, args.unfused_chunk)),
        ("single", n, lambda: ds.with_tx_precoder(F, beams, p).compute_rate(snr_db=snr_db)),
    ]
    m_rx, m_tx = int(np.prod(shape["ue"])), int(np.prod(shape["bs"]))
    rec = dict(shape=name, rays="device", bs=shape["bs"], ue=shape["ue"], K=K, users=n, paths=L, G=G, B=len(F), snr_db=snr_db,
               unfused_users=n_b, unfused_chunk=args.unfused_chunk, channel_bytes_per_user=8 * m_rx * m_tx * K,
               timings_per_route=2 * args.rounds, blocks_of_users=len(ds._mu_blocks(G)), time_block_bytes=int(dsm._TIME_BLOCK_BYTES))
    # the two ways agree per user
    rate_a = routes[0][2]()[:n_b].cpu().numpy()
    rate_b = routes[1][2]().cpu().numpy()
    rec["mu_vs_unfused_worst_abs_diff_bits"] = float(np.abs(rate_a - rate_b).max())
    rec["mu_mean_rate_bits"] = float(rate_a.mean())
    torch.cuda.empty_cache()
    ts = ab.alternate([(rn, fn, ab.host_timed, ab.host_timed) for rn, _, fn in routes], args.rounds)
    rec.update(ab.summaries(ts, digits=4, raw=True))
    for rn, users, _ in routes:
        rec[f"{rn}_us_per_user"] = round(1e3 * rec[f"{rn}_avg_ms"] / users, 5)
        rec[f"{rn}_spread_us_per_user"] = round(1e3 * rec[f"{rn}_spread_ms"] / users, 5)
    rec["unfused_extrapolated_ms"] = round(rec["unfused_us_per_user"] * n / 1e3, 3)
    rec["mu_over_unfused_per_user"] = round(rec["mu_us_per_user"] / rec["unfused_us_per_user"], 4)
    rec["mu_over_single"] = round(rec["mu_avg_ms"] / rec["single_avg_ms"], 4)
    rec["mu_faster_than_unfused_by_more_than_the_spreads"] = bool(
        rec["unfused_us_per_user"] - rec["mu_us_per_user"] > rec["unfused_spread_us_per_user"] + rec["mu_spread_us_per_user"])
    rec.update(split_of_mu(routes[0][2], args.split_runs))
    return json.dumps(rec)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,default")
    ap.add_argument("--users", type=int, default=0, help="cap on the users of every shape (0: the shape's own count)")
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--subcarriers", type=int, default=512)
    ap.add_argument("--group", type=int, default=4, help="users per group, G")
    ap.add_argument("--snr-db", type=float, default=100.0, help="the synthetic path powers are -140 .. -60 dBW")
    ap.add_argument("--unfused-users", type=int, default=4096, help="users route (b) runs on")
    ap.add_argument("--unfused-chunk", type=int, default=1024, help="users per channel tensor of route (b)")
    ap.add_argument("--rounds", type=int, default=3, help="timings per route and pass")
    ap.add_argument("--split-runs", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("mu_rate_bench: no GPU")
    dm.config("channel_output", "torch")
    try:
        lines = []
        for name in args.shapes.split(","):
            lines.append(measure(name, args))
            print(lines[-1], flush=True)
    finally:
        dm.config("channel_output", "numpy")
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
