"""Fidelity sweep (needs the reference package): the NumPy oracle against the imported reference on the
random configurations of tests/test_gpu_random_sweep.py (panel shapes, paths, subcarriers, rotations, FoV,
patterns, FD/TD/LPF, num_paths slicing, NaN holes).  Complements the committed goldens.  Run from a scratch
directory with the reference (DeepMIMO v4.0.0a3) and this repository on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 <repo>/oracle/crosscheck_reference.py 300

`--save FILE` also records what the reference returned on those configurations - side products whole, each channel
as a SHA-256 of its values, per-user peaks and a seeded sample of elements - which is how
tests/golden/crosscheck_reference.npz (data only) was written:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 <repo>/oracle/crosscheck_reference.py 10 \\
        --save <repo>/tests/golden/crosscheck_reference.npz

tests/test_oracle_golden.py checks the oracle against that record with check() below, no reference needed.
"""
import hashlib
import io
import os
import sys
from contextlib import redirect_stdout, redirect_stderr

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as onp  # noqa: E402
from tests._cases import random_case  # noqa: E402

SAMPLE = 4096           # channel elements kept per configuration in a record


def reference_outputs(dm, seed):
    """What the imported reference returns for sweep configuration `seed`: channel, los, num_paths, fov mask."""
    c, rays, ue_rot, op, bs_fov, ue_fov = random_case(seed)       # the configurations of tests/test_gpu_random_sweep.py
    fd = c["mode"] != "td"
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(c["bs"]), np.array(c["ue"])
    p.bs_antenna.spacing = p.ue_antenna.spacing = c["spacing"]
    p.bs_antenna.rotation, p.ue_antenna.rotation = np.array(c["bs_rot"]), np.array(ue_rot)
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = str(c["bs_pat"]), str(c["ue_pat"])
    p.num_paths, p.freq_domain = c["num_paths"], int(fd)
    p.ofdm.subcarriers, p.ofdm.selected_subcarriers = c["N"], np.asarray(c["sel"])
    p.ofdm.bandwidth, p.ofdm.rx_filter = c["bandwidth"], int(c["mode"] == "lpf")
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    if bs_fov is not None or ue_fov is not None:
        kw = {}
        if bs_fov is not None:
            kw["bs_fov"] = bs_fov
        if ue_fov is not None:
            kw["ue_fov"] = ue_fov
        ds.apply_fov(**kw)
    with redirect_stdout(io.StringIO()), redirect_stderr(io.StringIO()):
        Href = ds.compute_channels(p)
        los_ref, np_ref, mask_ref = np.asarray(ds.los), np.asarray(ds.num_paths), ds["_fov_mask"]
    return {"channel": np.asarray(Href), "los": los_ref, "num_paths": np_ref, "fov_mask": mask_ref}


def fingerprint(H):
    """SHA-256 of a channel tensor's values: dtype, shape, the finite pattern and the finite values (-0.0 as 0.0)."""
    H = np.asarray(H)
    fin = np.isfinite(H)
    h = hashlib.sha256(f"{H.dtype.str}{H.shape}".encode())
    h.update(np.packbits(fin).tobytes())
    h.update(np.ascontiguousarray(np.where(fin, H, 0) + 0).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _user_peaks(H):
    return np.nan_to_num(np.abs(np.where(np.isfinite(H), H, 0)).reshape(len(H), -1).max(axis=1, initial=0.0).astype(np.float64))


def record(ref, seed):
    """The part of reference_outputs() a record keeps (arrays only, for np.savez)."""
    H = ref["channel"]
    idx = np.sort(np.random.default_rng(31 + seed).choice(H.size, size=min(H.size, SAMPLE), replace=False))
    out = {"shape": np.array(H.shape, dtype=np.int64), "sha256": fingerprint(H), "peak": _user_peaks(H),
           "sample_idx": idx.astype(np.int64), "sample": H.reshape(-1)[idx], "los": ref["los"], "num_paths": ref["num_paths"]}
    if ref["fov_mask"] is not None:
        out["fov_mask"] = np.asarray(ref["fov_mask"])
    return out


def check(seed, ref):
    """The oracle on sweep configuration `seed` against the reference's outputs `ref` (reference_outputs(), or a
    record()): channels within 1e-7 of each configuration's peak, side products exact.  Returns (worst |dH| / peak
    over the elements `ref` holds, whether the channel is bit-identical)."""
    c, rays, ue_rot, op, bs_fov, ue_fov = random_case(seed)
    res = onp.compute_channels(rays, op, bs_fov=bs_fov, ue_fov=ue_fov)
    H = res["channel"]
    if "channel" in ref:
        Href, got = ref["channel"], H
        assert H.shape == Href.shape, f"seed {seed}: shape {H.shape} vs {Href.shape}"
        peak = float(np.max(np.abs(np.where(np.isfinite(Href), Href, 0)))) if H.size else 1.0
        same = np.array_equal(fingerprint(H), fingerprint(Href))
    else:
        assert H.shape == tuple(ref["shape"]), f"seed {seed}: shape {H.shape} vs {tuple(ref['shape'])}"
        Href, got = ref["sample"], H.reshape(-1)[ref["sample_idx"]]
        peak = float(np.max(ref["peak"])) if H.size else 1.0
        assert np.allclose(_user_peaks(H), ref["peak"], rtol=1e-7, atol=1e-12), f"seed {seed}: per-user peaks differ"
        same = np.array_equal(fingerprint(H), ref["sha256"])
    fin = np.isfinite(Href)
    assert np.array_equal(np.isfinite(got), fin), f"seed {seed}: NaN pattern differs"
    d = float(np.max(np.abs(np.where(fin, got - Href, 0)))) if got.size else 0.0
    assert d <= 1e-7 * peak + 1e-12, f"seed {seed}: channel differs by {d:.3e} (peak {peak:.3e}) cfg {c}"
    assert np.array_equal(res["los"], ref["los"]), f"seed {seed}: los"
    assert np.array_equal(res["num_paths"], ref["num_paths"]), f"seed {seed}: num_paths"
    mask_ref = ref.get("fov_mask")
    assert (mask_ref is None and res["_fov_mask"] is None) or np.array_equal(res["_fov_mask"], mask_ref), f"seed {seed}: mask"
    return d / max(peak, 1e-300), same


def main(n_cfg=None, save=None):
    import deepmimo as dm
    argv = sys.argv[1:]
    if "--save" in argv:
        i = argv.index("--save")
        save, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    if n_cfg is None:
        n_cfg = int(argv[0]) if argv else 200
    worst, kept = 0.0, {}
    for seed in range(n_cfg):
        ref = reference_outputs(dm, seed)
        worst = max(worst, check(seed, ref)[0])
        if save:
            kept.update({f"s{seed}_{k}": v for k, v in record(ref, seed).items()})
    if save:
        np.savez_compressed(save, n_cfg=np.array(n_cfg), **kept)
    print(f"oracle == reference on {n_cfg} random configurations; worst |dH|/peak = {worst:.2e}")
    return worst


if __name__ == "__main__":
    main()
