#!/usr/bin/env python3
"""Stage 1 under each radiation pattern, alone and with stage 2 behind it: `python tools/pattern_bench.py --label this`.

Two shapes: the headline one (100k users, 25 paths, 8 x 8 BS / 2 x 2 UE = 64 x 4 antennas, K = 512; stage 1 in the "light"
form `compute_channels` runs, then `dmx_channels_fd(variant = 0)` into a resident tensor) and DeepMIMO's defaults (200k users,
8 x 1 / 1 x 1, K = 1; stage 1 alone, and the single-pass route `dmx_channels_fd_direct`, which is stage 1 + stage 2 there).
Forms of stage 1 on the same uploaded rays: isotropic (the lean form), half-wave dipole at the BS, a BS field of view of
[150, 110] degrees, "tr38901" at the BS, "tr38901" on both sides (the last four run the FULL form).  A form the loaded
library refuses (an older build: pattern id 2) is recorded as such and skipped.

Device events around `--launches` back-to-back launches, `--rounds` of them per form after a warm-up, the forms alternating;
the whole measurement runs twice (pass 0 and 1) and the difference between the two passes of the SAME form is the spread a
difference between forms - or between builds - has to exceed.  One JSON line per (shape, form), appended to `--out`.
Set DMX_LIB_PATH to time another build of the library with the same script on the same box; alternate the builds
(this, other, this, other) on the same `--forms` - the forms of one process share the caches, so a list of five does not
compare with a list of three - and compare `--label`s.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402

FORMS = [("isotropic", "isotropic", "isotropic", None), ("dipole_bs", "halfwave-dipole", "isotropic", None),
         ("fov_bs", "isotropic", "isotropic", [150, 110]), ("tr38901_bs", "tr38901", "isotropic", None),
         ("tr38901_both", "tr38901", "tr38901", None)]
SHAPES = [dict(name="headline", bs=[8, 8], ue=[2, 2], K=512, users=100_000, direct=False),
          dict(name="defaults", bs=[8, 1], ue=[1, 1], K=1, users=200_000, direct=True)]


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
    ap.add_argument("--label", default="this", help="which build this is (a field of every line)")
    ap.add_argument("--out", default=os.path.join("profiles", "r12_pattern_bench.jsonl"))
    ap.add_argument("--paths", type=int, default=25)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forms", nargs="+", default=[f[0] for f in FORMS], choices=[f[0] for f in FORMS],
                    help="the forms to run (two builds are compared on the same list: the forms share the caches)")
    ap.add_argument("--shapes", nargs="+", default=[s["name"] for s in SHAPES], choices=[s["name"] for s in SHAPES])
    ap.add_argument("--scale", type=float, default=1.0, help="multiply both user counts (a rehearsal at a small size)")
    args = ap.parse_args()
    eng = ChannelEngine(0)
    lib, dev, L = eng.lib, eng.device, args.paths
    stream = eng._stream_ptr()
    lines = []
    for sh in [s for s in SHAPES if s["name"] in args.shapes]:
        n = max(1, int(sh["users"] * args.scale))
        rays = eng.upload_rays(bench.synth_device_rays(n, L, 1234, dev))
        m_rx, m_tx = int(np.prod(sh["ue"])), int(np.prod(sh["bs"]))
        out = torch.empty((n, m_rx, m_tx, sh["K"]), dtype=torch.complex64, device=dev)
        outp = C.c_void_p(out.data_ptr())
        runs = []
        for form, bs_pat, ue_pat, bs_fov in [f for f in FORMS if f[0] in args.forms]:
            p = dm.ChannelGenParameters()
            p.bs_antenna.shape, p.ue_antenna.shape = np.array(sh["bs"]), np.array(sh["ue"])
            p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = bs_pat, ue_pat
            p.num_paths = L
            p.ofdm.selected_subcarriers = np.arange(sh["K"])
            p.validate(n)
            rec = dict(build=args.label, library=os.path.basename(os.path.dirname(nat.LIB_PATH)) + "/" + os.path.basename(nat.LIB_PATH),
                       shape=sh["name"], bs=sh["bs"], ue=sh["ue"], K=sh["K"], users=n, paths=L, form=form,
                       second="dmx_channels_fd_direct" if sh["direct"] else "dmx_path_prep + dmx_channels_fd(variant=0)")
            try:
                prep = eng.prepare(rays, p, want_side="light", bs_fov=None if bs_fov is None else np.array(bs_fov))
            except nat.NativeError as exc:
                rec["refused"] = str(exc)
                lines.append(rec)
                continue
            ps, rs, ss = prep.params_struct, prep.rays_struct, prep.side_struct
            wsp = C.c_void_p(prep.workspace.data_ptr())

            def stage1(rs=rs, ps=ps, ss=ss, wsp=wsp, nb=prep.workspace_bytes):
                nat.check(lib.dmx_path_prep(C.byref(rs), C.byref(ps), wsp, nb, C.byref(ss), stream), "dmx_path_prep")

            if sh["direct"]:
                assert lib.dmx_fd_direct_supported(C.byref(ps), L) == 1

                def both(rs=rs, ps=ps, ss=ss):
                    nat.check(lib.dmx_channels_fd_direct(C.byref(rs), C.byref(ps), C.byref(ss), 0, n, outp, stream), "dmx_channels_fd_direct")
            else:
                def both(rs=rs, ps=ps, ss=ss, wsp=wsp, nb=prep.workspace_bytes):
                    nat.check(lib.dmx_path_prep(C.byref(rs), C.byref(ps), wsp, nb, C.byref(ss), stream), "dmx_path_prep")
                    nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, outp, 0, stream), "dmx_channels_fd")
            runs.append((rec, prep, stage1, both))
        launches_both = args.launches if sh["direct"] else max(2, args.launches // 5)       # 105 GB of output per launch
        for ab in range(2):
            for rec, _, stage1, both in runs:                       # warm-up
                timed(stage1, 5)
                timed(both, 2)
            ts = {rec["form"]: ([], []) for rec, _, _, _ in runs}
            for _ in range(args.rounds):
                for rec, _, stage1, both in runs:
                    ts[rec["form"]][0].append(timed(stage1, args.launches))
                    ts[rec["form"]][1].append(timed(both, launches_both))
            for rec, _, _, _ in runs:
                for what, v in zip(("stage1", "both"), ts[rec["form"]]):
                    rec[f"{what}_avg_ms_pass{ab}"] = round(float(np.mean(v)), 5)
                    rec[f"{what}_min_ms_pass{ab}"] = round(float(np.min(v)), 5)
        for rec, _, _, _ in runs:
            for what in ("stage1", "both"):
                a0, a1 = rec[f"{what}_avg_ms_pass0"], rec[f"{what}_avg_ms_pass1"]
                rec[f"{what}_avg_ms"] = round((a0 + a1) / 2, 5)
                rec[f"{what}_spread_ms"] = round(abs(a0 - a1), 5)
            lines.append(rec)
        chk = torch.view_as_real(out[:: max(1, n // 64)])
        assert bool(torch.isfinite(chk).all()) and float(chk.abs().max()) > 0, "bench output is not finite / all zero"
        del runs, out, rays
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
