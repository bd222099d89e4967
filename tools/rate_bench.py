#!/usr/bin/env python3
"""Per-user achievable rate, channel eigenmodes and eigenbeams: the fused routes against the channel tensor + torch.linalg, alternating in
ONE process: `python tools/rate_bench.py [--out profiles/r7_precoder_bench.jsonl]`.

For each shape, on the same uploaded rays:
  (a) fused     dmx_path_prep + dmx_channel_rate                                 (no channel tensor)
  (b) slogdet   dmx_path_prep + per user chunk: dmx_channels_fd (variant 0) into a resident tensor, the Gram over the smaller
                array by torch.einsum, torch.linalg.slogdet of I + s G, the mean over the subcarriers
  (c) spectrum  dmx_path_prep + dmx_channel_spectrum, the water-filling rate only: (a)'s kernel with the Jacobi epilogue
  (d) modes     dmx_path_prep + dmx_channel_spectrum, the mode SNRs [n, K, m] only
  (e) eigvalsh  (d)'s unfused twin: (b)'s channel chunks and Gram, torch.linalg.eigvalsh of snr G, descending.  The batched
                solver takes seconds for 1e5 small matrices, so this route runs on the first `--eig-users` users only, one
                launch per timing; its time is reported for that count and `modes_speedup_per_user` compares time per user,
                an extrapolation and not a like-for-like run
  (f) beams     dmx_path_prep + dmx_channel_precoders with n_layers = 1, gamma and the smaller-side vector only (the
                rotations accumulated in registers; no second pass)
  (g) beams2    (f) with the larger-side vector as well (the second pass over the tables; at the headline shape the
                precoders of 1e5 users are as large as H itself, so this route runs on the first `--beam-users` users and
                its time is reported for that count)
  (h) svd       (g)'s unfused twin: (b)'s channel chunks and torch.linalg.svd of H_k, the first singular pair kept, on the
                first `--eig-users` users only, one launch per timing; `beams_speedup_per_user` compares time per user
Timed by the protocol of `tools/ab_protocol.py` (device events, a warm-up of 1).  One JSON line per shape: the protocol's
fields per route, the fused
kernel's algorithmic flops (complex product 6, complex multiply-add 8) and their share of the fp32 vector peak (256 CUs x
4 SIMDs x 64 flop per clock at 2.4 GHz), and the largest deviation between the two results in bit.  Without a GPU the
tool fails.
"""
import argparse
import ctypes as C
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
from deepmimo_amd import _native as nat  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

# (name, BS panel, UE panel, K, users, users per chunk of route (b)): the headline shape (H would be 105 GB) and DeepMIMO's
# defaults (one subcarrier)
SHAPES = [("headline_K512", [64, 4], [2, 2], 512, 100_000, 5_000), ("defaults_K1", [8, 1], [1, 1], 1, 200_000, 200_000)]
FP32_VALU_PEAK = 256 * 4 * 64 * 2.4e9


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--snr-db", type=float, default=110.0)
    ap.add_argument("--launches", type=int, default=5, help="back-to-back launches of a route per timing")
    ap.add_argument("--rounds", type=int, default=2, help="timings per route and pass: 2 passes x rounds x launches launches in all")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every user count (rehearsals)")
    ap.add_argument("--eig-users", type=int, default=200, help="users of route (e)")
    ap.add_argument("--beam-users", type=int, default=20000, help="users of route (g)")
    ap.add_argument("--routes", default="fused,slogdet,spectrum,modes,eigvalsh,beams,beams2,svd")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    eng = ChannelEngine(0)
    lib, L = eng.lib, args.paths
    stream = eng._stream_ptr()
    snr = 10.0 ** (args.snr_db / 10.0)
    lines = []
    for name, bs, ue, K, users, chunk in SHAPES:
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
        m, big = min(m_tx, m_rx), max(m_tx, m_rx)
        H = torch.empty((chunk, m_rx, m_tx, K), dtype=torch.complex64, device=eng.device)
        wsp = C.c_void_p(prep.workspace.data_ptr())
        r_fused = torch.empty((n,), dtype=torch.float32, device=eng.device)
        r_ref = torch.empty((n,), dtype=torch.float32, device=eng.device)
        r_wf = torch.empty((n,), dtype=torch.float32, device=eng.device)
        n_eig = min(n, max(1, args.eig_users))
        want = args.routes.split(",")
        g_fused = torch.empty((n, K, m), dtype=torch.float32, device=eng.device) if "modes" in want else None
        g_ref = torch.empty((n_eig, K, m), dtype=torch.float32, device=eng.device) if "eigvalsh" in want else None
        n_beam = min(n, max(1, args.beam_users))
        cplx = lambda *shape: torch.empty(shape, dtype=torch.complex64, device=eng.device)   # noqa: E731
        b_gamma = torch.empty((n, K, m), dtype=torch.float32, device=eng.device) if {"beams", "beams2"} & set(want) else None
        b_small = cplx(n, K, 1, m) if {"beams", "beams2"} & set(want) else None
        b_big = cplx(n_beam, K, 1, big) if "beams2" in want else None
        v_ref = cplx(n_eig, K, m_tx) if "svd" in want else None
        eye = torch.eye(m, dtype=torch.complex64, device=eng.device)
        spec = "uitk,ujtk->ukij" if m_rx <= m_tx else "urjk,urik->ukij"
        s = snr / m_tx

        def fused():
            stage1()
            nat.check(lib.dmx_channel_rate(C.byref(ps), wsp, n, L, 0, n, snr, C.c_void_p(r_fused.data_ptr()), None, stream),
                      "dmx_channel_rate")

        def slogdet():
            stage1()
            for b in range(0, n, chunk):
                cnt = min(chunk, n - b)
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, b, cnt, C.c_void_p(H.data_ptr()), 0, stream), "dmx_channels_fd")
                G = torch.einsum(spec, H[:cnt], H[:cnt].conj())
                r_ref[b:b + cnt] = (torch.linalg.slogdet(eye + s * G)[1] / math.log(2.0)).mean(dim=1)

        def spectrum():
            stage1()
            nat.check(lib.dmx_channel_spectrum(C.byref(ps), wsp, n, L, 0, n, snr, None, C.c_void_p(r_wf.data_ptr()), None, stream),
                      "dmx_channel_spectrum")

        def modes():
            stage1()
            nat.check(lib.dmx_channel_spectrum(C.byref(ps), wsp, n, L, 0, n, snr, C.c_void_p(g_fused.data_ptr()), None, None, stream),
                      "dmx_channel_spectrum")

        def eigvalsh():
            stage1()
            for b in range(0, n_eig, chunk):
                cnt = min(chunk, n_eig - b)
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, b, cnt, C.c_void_p(H.data_ptr()), 0, stream), "dmx_channels_fd")
                G = torch.einsum(spec, H[:cnt], H[:cnt].conj())
                g_ref[b:b + cnt] = torch.linalg.eigvalsh(snr * G).flip(-1).clamp_min(0)   # scaled first: raw gains are near 1e-15

        def beam_call(count, with_big):
            small, bigp = C.c_void_p(b_small.data_ptr()), C.c_void_p(b_big.data_ptr()) if with_big else None
            tx, rx = (bigp, small) if m_rx <= m_tx else (small, bigp)
            stage1()
            nat.check(lib.dmx_channel_precoders(C.byref(ps), wsp, n, L, 0, count, snr, 1, C.c_void_p(b_gamma.data_ptr()), tx, rx, stream),
                      "dmx_channel_precoders")

        def beams():
            beam_call(n, False)

        def beams2():
            beam_call(n_beam, True)

        def svd():
            stage1()
            for b in range(0, n_eig, chunk):
                cnt = min(chunk, n_eig - b)
                nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, b, cnt, C.c_void_p(H.data_ptr()), 0, stream), "dmx_channels_fd")
                _, _, vh = torch.linalg.svd(H[:cnt].permute(0, 3, 1, 2) * math.sqrt(snr), full_matrices=False)
                v_ref[b:b + cnt] = vh[..., 0, :].conj()

        routes = [(rn, fn, ab.device(1 if rn in ("eigvalsh", "svd") else args.launches), ab.device(1))
                  for rn, fn in (("fused", fused), ("slogdet", slogdet), ("spectrum", spectrum), ("modes", modes), ("eigvalsh", eigvalsh),
                                 ("beams", beams), ("beams2", beams2), ("svd", svd)) if rn in want]
        rec = dict(shape=name, bs=bs, ue=ue, K=K, users=n, paths=L, snr_db=args.snr_db, chunk_users=chunk,
                   H_bytes=n * m_rx * m_tx * K * 8, launches_per_route=2 * args.rounds * args.launches)
        rec["fused_flops"] = n * K * big * (L * (6 + 8 * m) + 8 * m * (m + 1) // 2)
        rec.update(ab.summaries(ab.alternate(routes, args.rounds)))
        have = {r[0] for r in routes}
        if {"fused", "slogdet"} <= have:
            rec["speedup"] = round(rec["slogdet_avg_ms"] / rec["fused_avg_ms"], 3)
            rec["max_dev_bit"] = float((r_fused - r_ref).abs().max())
        if "fused" in have:
            rec["fused_share_of_fp32_valu_peak"] = round(rec["fused_flops"] / (rec["fused_avg_ms"] * 1e-3) / FP32_VALU_PEAK, 4)
            rec["mean_rate"] = float(r_fused.double().mean())
        if "spectrum" in have:
            rec["mean_rate_waterfilling"] = float(r_wf.double().mean())
        if {"fused", "spectrum"} <= have:
            rec["spectrum_over_fused"] = round(rec["spectrum_avg_ms"] / rec["fused_avg_ms"], 4)
            rec["waterfilling_below_equal_max_bit"] = float((r_fused - r_wf).clamp_min(0).max())
        if {"modes", "eigvalsh"} <= have:
            rec["eigvalsh_users"] = n_eig                                 # route (e) covers these users only; (d) all of them
            rec["modes_speedup_per_user"] = round((rec["eigvalsh_avg_ms"] / n_eig) / (rec["modes_avg_ms"] / n), 3)
            top = g_ref[..., 0].clamp_min(1e-30)
            rec["modes_max_dev_rel_to_strongest"] = float(((g_fused[:n_eig] - g_ref).abs().amax(dim=-1) / top).max())
        if "beams" in have:
            rec["precoder_out_bytes_small_side"] = n * K * (4 * m + 8 * m)
        if {"beams", "modes"} <= have:
            rec["beams_over_modes"] = round(rec["beams_avg_ms"] / rec["modes_avg_ms"], 4)
        if "beams2" in have:
            rec["beams2_users"] = n_beam                                  # route (g) covers these users only
            rec["precoder_out_bytes_both_sides"] = n_beam * K * (4 * m + 8 * m + 8 * big)
        if {"beams2", "modes"} <= have:
            rec["beams2_over_modes_per_user"] = round((rec["beams2_avg_ms"] / n_beam) / (rec["modes_avg_ms"] / n), 4)
        if {"beams2", "svd"} <= have:
            rec["svd_users"] = n_eig
            rec["beams_speedup_per_user"] = round((rec["svd_avg_ms"] / n_eig) / (rec["beams2_avg_ms"] / n_beam), 3)
            k = min(n_eig, n_beam)
            v_fused = (b_big if m_rx <= m_tx else b_small)[:k, :, 0, :]
            live = b_gamma[:k, :, 0] > 0
            overlap = (v_fused.conj() * v_ref[:k]).sum(dim=-1).abs()
            rec["beams_min_overlap_with_svd"] = float(overlap[live].min()) if bool(live.any()) else None
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del H, prep, rays, b_gamma, b_small, b_big, v_ref, g_fused, g_ref
        torch.cuda.empty_cache()
    if args.out:
        ab.write_lines(args.out, lines, "w")


if __name__ == "__main__":
    main()
