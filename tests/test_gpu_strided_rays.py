"""Ray matrices with a row stride `dmx_rays.ld > n_paths` (include/deepmimo_amd.h) on every kernel that reads them:
stage1_path (the lean k1_path_prep forms and k12_fd_direct), k1_path_prep_full and k5_pathloss.

The criterion is IDENTITY: the same rays are uploaded dense ([n, L]) and as [n, ld] tensors whose columns L .. ld - 1 hold
poison - finite, plausible and stronger than every real path (-20 dBW against at most -60).  `torch.equal` on the bits of
every side product, of the channels of both domains, of the single-pass output and of the pathloss; a read of a pad column
or of a wrong row changes nearly every user.  Three strides are live in stage 1 (ray rows `ld`, dense side-product rows
`n_paths`, workspace rows P), so one swapped for another shows here.  The dense run is also held to the oracle with the
project's existing criteria, so that identity is not two equal wrong answers.
"""
import ctypes as C

import numpy as np
import pytest

from tests._cases import assert_channel_close, assert_taps_close, oracle_params

pytestmark = pytest.mark.gpu

FC = 28e9
N_UE = 37                                                     # odd: one idle half-wave shadows the last user
POISON = dict(power=-20.0, phase=33.0, delay=1e-7, aoa_az=90.0, aoa_el=90.0, aod_az=90.0, aod_el=90.0, inter=0.0,
              doppler_vel=50.0, doppler_acc=5.0)


def _cfg(cid, L, runs, **kw):
    d = dict(id=cid, L=L, runs=runs, want_side="light", bs_rot=[5, -20, 60], ue_rot=[0, 0, 0], bs_pattern="isotropic",
             ue_pattern="isotropic", bs_fov=None, ue_fov=None, num_paths=L, doppler=False, bs_shape=[4, 2], ue_shape=[2, 1],
             bs_spacing=0.5, ue_spacing=0.37, subcarriers=64, selected=[0, 5, 63], bandwidth=20e6, rx_filter=0)
    d.update(kw)
    return d


_FULL = dict(want_side=True, bs_fov=[150, 100], ue_pattern="halfwave-dipole")
CONFIGS = [
    _cfg("lean_zrot", 25, "k1_path_prep<32, true>", bs_rot=[0, 0, 0], want_side=False),
    _cfg("lean_rot", 25, "k1_path_prep<32>"),
    _cfg("lean_64_L33", 33, "k1_path_prep<64>, one pass"),
    _cfg("lean_64_L70", 70, "k1_path_prep<64>, two passes"),
    _cfg("full_32", 25, "k1_path_prep_full<32>", **_FULL),
    _cfg("full_64", 40, "k1_path_prep_full<64>", **_FULL),
    _cfg("full_doppler", 25, "k1_path_prep_full<32> with the Doppler rays", want_side=True, doppler=True),
    _cfg("L32_edge", 32, "last shape with two users per wave"),
    _cfg("num_paths_lt_L", 25, "num_paths = 10 of 25 loaded", num_paths=10),
]


def _lds(L):
    return [L + 3, 2 * L] + ([64] if L == 25 else [])


def _rays(c):
    from oracle import oracle_np as onp
    return onp.synth_rays(N_UE, c["L"], seed=900 + c["L"], with_doppler=c["doppler"])


def _dm_params(c, freq_domain):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(c["bs_shape"]), np.array(c["ue_shape"])
    p.bs_antenna.spacing, p.ue_antenna.spacing = c["bs_spacing"], c["ue_spacing"]
    p.bs_antenna.rotation, p.ue_antenna.rotation = np.array(c["bs_rot"]), np.array(c["ue_rot"])
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = c["bs_pattern"], c["ue_pattern"]
    p.num_paths, p.freq_domain = c["num_paths"], freq_domain
    p.ofdm.subcarriers, p.ofdm.selected_subcarriers = c["subcarriers"], np.array(c["selected"], dtype=np.int64)
    p.ofdm.bandwidth, p.ofdm.rx_filter = c["bandwidth"], 0
    p.enable_doppler = int(c["doppler"])
    return p.validate(N_UE)


def _kw(c):
    return dict(bs_fov=None if c["bs_fov"] is None else np.array(c["bs_fov"]), ue_fov=None, carrier_freq=FC)


def _wide(eng, rays, L, ld):
    """DeviceRays over [n, ld] tensors: the rays in columns 0 .. L - 1, poison behind them"""
    import torch
    from deepmimo_amd import consts
    from deepmimo_amd.engine import DeviceRays

    def widen(k):
        w = np.full((N_UE, ld), POISON[k], dtype=np.float32)
        w[:, :L] = rays[k]
        return torch.from_numpy(w).to(eng.device)
    fields = {k: widen(k) for k in consts.RAY_FIELDS}
    dop = "doppler_vel" in rays
    return DeviceRays(n_ue=N_UE, n_paths=L, fields=fields, doppler_vel=widen("doppler_vel") if dop else None,
                      doppler_acc=widen("doppler_acc") if dop else None)


def _bits(t):
    import torch
    if t.is_complex():
        return torch.view_as_real(t).view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def _same(a, b, what):
    import torch
    assert (a is None) == (b is None), f"{what}: present in one run only"
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert torch.equal(_bits(a), _bits(b)), f"{what}: differs between the dense and the strided rays"


def _run(eng, dr, c, ld):
    """Everything the configuration computes on `dr`, ray rows `ld` apart: dict name -> tensor"""
    import torch
    res = {}
    for fd in (1, 0):
        p = _dm_params(c, fd)
        structs = eng._call_structs(dr, p, **_kw(c))
        structs[1].ld = ld
        prep = eng.prepare(dr, p, want_side=c["want_side"], structs=structs, **_kw(c))
        assert prep.rays_struct.ld == ld and prep.rays_struct.n_paths == c["L"]
        dom = "fd" if fd else "td"
        for k, t in prep.side.items():
            res[f"{dom} side {k}"] = t
        res[f"{dom} channel"] = eng.channels(prep, variant=1) if fd else eng.channels(prep)
    # the single pass takes 1..64 loaded and 1..32 used paths: with more loaded paths it runs on the first 32
    p = _dm_params(dict(c, num_paths=min(c["num_paths"], 32)), 1)
    structs = eng._call_structs(dr, p, **_kw(c))
    structs[1].ld = ld
    if eng.direct_supported(dr, p, structs=structs):
        H, side = eng.channels_direct(dr, p, want_side="light", structs=structs)
        res["direct channel"] = H
        for k, t in side.items():
            res[f"direct side {k}"] = t
    torch.cuda.synchronize()
    return res


def _oracle(c, rays, freq_domain):
    from oracle import oracle_np as onp
    op = oracle_params(dict(c, freq_domain=freq_domain), np.array(c["ue_rot"]))
    bs_fov = None if c["bs_fov"] is None else np.array(c["bs_fov"])
    dop = None
    if c["doppler"]:
        op["enable_doppler"] = 1
        dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC)
    return onp.compute_channels(rays, op, bs_fov=bs_fov, ue_fov=None if bs_fov is None else np.array([360, 180]), doppler=dop)


@pytest.mark.parametrize("c", CONFIGS, ids=[c["id"] for c in CONFIGS])
def test_strided_rays_give_the_dense_bits(c):
    from deepmimo_amd.engine import ChannelEngine
    eng = ChannelEngine(0)
    rays, L = _rays(c), c["L"]
    dense = _run(eng, eng.upload_rays(rays), c, L)
    assert ("direct channel" in dense) == (L <= 64), "the single pass takes up to 64 loaded paths"
    want = {"fd channel", "td channel", "fd side max_delay_key"}
    if c["want_side"]:
        want |= {"fd side los", "td side num_paths"}
    if c["want_side"] is True:
        want |= {"fd side aod_el_rot", "fd side aoa_az_rot", "fd side power_linear", "td side power_linear_ant_gain"}
    assert want <= set(dense)

    # the dense run against the oracle, the project's existing criteria
    iso = c["bs_pattern"] == "isotropic" and c["ue_pattern"] == "isotropic"
    for fd in (1, 0):
        ref = _oracle(c, rays, fd)
        dom = "fd" if fd else "td"
        H = dense[f"{dom} channel"].cpu().numpy()
        if fd or not iso:
            assert_channel_close(H, ref["channel"], what=f"{c['id']} {dom}")
        else:
            assert_taps_close(H, ref["channel"], what=f"{c['id']} td")
        if c["want_side"]:
            np.testing.assert_array_equal(dense[f"{dom} side los"].cpu().numpy(), ref["los"])
            np.testing.assert_array_equal(dense[f"{dom} side num_paths"].cpu().numpy(), ref["num_paths"])
        if dense.get(f"{dom} side fov_mask") is not None:
            np.testing.assert_array_equal(dense[f"{dom} side fov_mask"].cpu().numpy().astype(bool), ref["_fov_mask"])
        if c["want_side"] is True:
            np.testing.assert_allclose(dense[f"{dom} side power_linear"].cpu().numpy(), ref["power_linear"], rtol=1e-6, equal_nan=True)
    if "direct channel" in dense:
        ref = _oracle(dict(c, num_paths=min(c["num_paths"], 32)), rays, 1)
        assert_channel_close(dense["direct channel"].cpu().numpy(), ref["channel"], what=f"{c['id']} direct")

    for ld in _lds(L):
        strided = _run(eng, _wide(eng, rays, L, ld), c, ld)
        assert set(strided) == set(dense)
        for k in sorted(dense):
            _same(strided[k], dense[k], f"{c['id']} ld={ld}: {k}")


def _pathloss(eng, fields, L, ld, coherent):
    import torch
    from deepmimo_amd import _native as nat
    out = torch.full((N_UE,), -777.0, dtype=torch.float32, device=eng.device)
    r = nat.DmxRays()
    r.n_ue, r.n_paths, r.ld = N_UE, L, ld
    r.power, r.phase = fields["power"].data_ptr(), fields["phase"].data_ptr()
    with torch.cuda.device(eng.device):
        rc = eng.lib.dmx_pathloss(C.byref(r), int(coherent), C.c_void_p(out.data_ptr()), eng._stream_ptr())
    nat.check(rc, "dmx_pathloss")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("L", [25, 33, 70])
def test_strided_pathloss(L):
    from deepmimo_amd.engine import ChannelEngine
    from oracle import oracle_np as onp
    eng = ChannelEngine(0)
    rays = onp.synth_rays(N_UE, L, seed=900 + L)
    rays["power"][7, 3] = np.nan                                   # NaN in the middle of a row
    dr = eng.upload_rays(rays)
    for coherent in (True, False):
        dense = _pathloss(eng, dr.fields, L, L, coherent)
        _same(eng.pathloss(dr, coherent), dense, f"L={L}: the engine's own call")
        with np.errstate(invalid="ignore", divide="ignore"):       # dataset.py:541-566, as tests/test_gpu_parity.py restates it
            g = np.sqrt(10 ** (rays["power"] / 10)).astype(np.complex64)
            if coherent:
                g = g * np.exp(1j * np.deg2rad(rays["phase"]))
            tp = np.abs(np.nansum(g, axis=1)) ** 2
            want = np.full_like(tp, np.nan)
            want[tp > 0] = -10 * np.log10(tp[tp > 0])
        got = dense.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=2e-4)   # dB
        for ld in _lds(L):
            wide = _wide(eng, rays, L, ld)
            _same(_pathloss(eng, wide.fields, L, ld, coherent), dense, f"L={L} ld={ld} coherent={coherent}")
