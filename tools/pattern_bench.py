#!/usr/bin/env python3
"""Stage 1 under each radiation pattern, alone and with stage 2 behind it: `python tools/pattern_bench.py --label this`.

Two shapes: the headline one (100k users, 25 paths, 8 x 8 BS / 2 x 2 UE = 64 x 4 antennas, K = 512; stage 1 in the "light"
form `compute_channels` runs, then `dmx_channels_fd(variant = 0)` into a resident tensor) and DeepMIMO's defaults (200k users,
8 x 1 / 1 x 1, K = 1; stage 1 alone, and the single-pass route `dmx_channels_fd_direct`, which is stage 1 + stage 2 there).
Forms of stage 1 on the same uploaded rays: isotropic (the lean form), half-wave dipole at the BS, a BS field of view of
[150, 110] degrees, "tr38901" at the BS, "tr38901" on both sides (the last four run the FULL form).  A form the loaded
library refuses (an older build: pattern id 2) is recorded as such and skipped.

Timed by the protocol of `tools/ab_protocol.py` with two routes per form, `stage1` and `both`, the forms alternating (device
events; warm-ups of 5 and 2 launches; `both` at the headline shape takes a fifth of `--launches`).  One JSON line per
(shape, form), the protocol's fields under `stage1_` and `both_`, appended to `--out`.
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
import ab_protocol as ab  # noqa: E402
import bench  # noqa: E402
import deepmimo_amd as dm  # noqa: E402
from deepmimo_amd import _native as nat  # noqa: E402
from deepmimo_amd.engine import ChannelEngine  # noqa: E402

FORMS = [("isotropic", "isotropic", "isotropic", None), ("dipole_bs", "halfwave-dipole", "isotropic", None),
         ("fov_bs", "isotropic", "isotropic", [150, 110]), ("tr38901_bs", "tr38901", "isotropic", None),
         ("tr38901_both", "tr38901", "tr38901", None)]
SHAPES = [dict(name="headline", bs=[8, 8], ue=[2, 2], K=512, users=100_000, direct=False),
          dict(name="defaults", bs=[8, 1], ue=[1, 1], K=1, users=200_000, direct=True)]


def main(argv=None):
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
    args = ap.parse_args(argv)
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
        runs, routes = [], []
        launches_both = args.launches if sh["direct"] else max(2, args.launches // 5)       # 105 GB of output per launch
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
            stage1 = ab.stage1(eng, prep)

            if sh["direct"]:
                assert lib.dmx_fd_direct_supported(C.byref(ps), L) == 1

                def both(rs=rs, ps=ps, ss=ss):
                    nat.check(lib.dmx_channels_fd_direct(C.byref(rs), C.byref(ps), C.byref(ss), 0, n, outp, stream), "dmx_channels_fd_direct")
            else:
                def both(ps=ps, stage1=stage1, wsp=C.c_void_p(prep.workspace.data_ptr())):
                    stage1()
                    nat.check(lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, outp, 0, stream), "dmx_channels_fd")
            runs.append((rec, prep))
            routes += [((form, "stage1"), stage1, ab.device(args.launches), ab.device(5)),
                       ((form, "both"), both, ab.device(launches_both), ab.device(2))]
        ts = ab.alternate(routes, args.rounds)
        for rec, _ in runs:
            for what in ("stage1", "both"):
                rec.update(ab.summary(ts[rec["form"], what], prefix=what + "_"))
            lines.append(rec)
        chk = torch.view_as_real(out[:: max(1, n // 64)])
        assert bool(torch.isfinite(chk).all()) and float(chk.abs().max()) > 0, "bench output is not finite / all zero"
        del runs, routes, out, rays
        torch.cuda.empty_cache()
    ab.write_lines(args.out, [json.dumps(rec) for rec in lines], "a", echo=True)


if __name__ == "__main__":
    main()
