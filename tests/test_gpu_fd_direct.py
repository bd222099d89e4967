"""Single-pass channel generation (dmx_channels_fd_direct, k12_fd_direct.hip) on the GPU.

The claim is IDENTITY with the two-call route: `torch.equal` on the channel tensor and on every light side product
against ``prepare(want_side="light")`` + ``channels(variant=9)``.  No tolerance anywhere in those comparisons.  The same
cases are also held to the project's bound against the NumPy oracle (tests/_cases.py: 5e-5 of each user's peak + 1e-12,
the existing tolerance of variant 9).  Which cases the kernel takes is decided by the host-only query
dmx_fd_direct_supported when the module is collected; nothing is skipped at run time.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests._cases import assert_channel_close, fov_args, load_golden, oracle_params

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):        # the cases are decided by a query of the library while this module is collected
    pytest.skip("needs the built library", allow_module_level=True)

FC = 28e9
GOLDENS = ["g01_plumbing", "g02_panel_order", "g03_rot_fov", "g03b_rot_fov_bs_only", "g06_dipole", "g07_delay_clip",
           "g08_num_paths_nan", "g09_random_ue_rot", "g10_doppler_v3", "g12_ula64_rot"]


def _host_supported(bs, ue, K, L, num_paths):
    """dmx_fd_direct_supported for a frequency-domain shape without rx_filter (host-only: usable at collection)"""
    import torch  # noqa: F401  (before the library, as deepmimo_amd.engine imports them: one HIP runtime per process)
    from deepmimo_amd import _native as n
    p = n.DmxParams()
    p.bs_shape[0], p.bs_shape[1], p.ue_shape[0], p.ue_shape[1] = bs[0], bs[1], ue[0], ue[1]
    p.num_paths, p.freq_domain, p.n_subcarriers, p.n_selected, p.bandwidth = num_paths, 1, 512, K, 10e6
    sel = (C.c_int32 * max(K, 1))()
    p.selected_subcarriers = C.addressof(sel)
    return n.load().dmx_fd_direct_supported(C.byref(p), L)


def _case(cid, n, L, bs, ue, N, sel, **kw):
    d = dict(id=cid, n=n, L=L, bs_shape=bs, ue_shape=ue, subcarriers=N, selected=list(sel), num_paths=kw.pop("num_paths", L),
             bs_rot=[0, 0, 0], ue_rot=[0, 0, 0], bs_pattern="isotropic", ue_pattern="isotropic", bs_fov=None, ue_fov=None,
             bs_spacing=0.5, ue_spacing=0.37, bandwidth=20e6, freq_domain=1, rx_filter=0, doppler=None, all_valid=False,
             max_delay=2e-6, rays="plain", per_user_rot=False)
    d.update(kw)
    return d


def _all_cases():
    cs = []
    # SHAPES_SMALL of tests/test_gpu_parity.py, restated
    small = [(70, 25, [8, 8], [1, 1], 512, [0], {}),
             (70, 25, [8, 8], [2, 2], 512, [0, 1], dict(bs_rot=[10, 0, -30])),
             (41, 10, [8, 1], [1, 1], 64, [3, 9, 27], dict(ue_rot=[0, 20, 40])),
             (33, 25, [4, 4], [2, 1], 512, list(range(0, 512, 103)), {}),
             (29, 32, [8, 4], [1, 2], 256, list(range(8)), dict(all_valid=True, max_delay=20e-6)),
             (260, 7, [2, 2], [1, 1], 64, list(range(64)), {})]
    for i, (n, L, bs, ue, N, sel, extra) in enumerate(small):
        cs.append(_case(f"small{i}", n, L, bs, ue, N, sel, **extra))
    for dop in (0, 1):                                                       # Doppler on and off on the same rays
        cs.append(_case(f"doppler{dop}", 37, 25, [4, 2], [2, 1], 64, [0, 5, 63], doppler=dop))
        cs.append(_case(f"doppler{dop}_rot_fov", 37, 12, [4, 2], [1, 1], 64, [1], doppler=dop, bs_rot=[5, -20, 60],
                        bs_fov=[150, 100]))
    # lean form (isotropic, no FoV) with a rotation at K = 1, 2 and 4: k12_fd_direct<1 / 2 / 4, 1>
    cs.append(_case("bs_rot_lean_K1", 51, 25, [8, 1], [1, 1], 512, [0], bs_rot=[10, 0, -30]))
    cs.append(_case("ue_rot_lean_K1", 51, 25, [4, 2], [2, 1], 512, [3], ue_rot=[0, 20, 40]))
    cs.append(_case("per_user_rot_lean_K1", 51, 25, [8, 1], [1, 1], 512, [0], per_user_rot=True))
    cs.append(_case("bs_rot_lean_K4", 51, 25, [4, 2], [2, 1], 512, [0, 1, 2, 3], bs_rot=[10, 0, -30]))
    # more than 32 loaded paths with zero rotations: stage 1 has no zero-rotation form there, the general lean one runs
    cs.append(_case("L40_zero_rot_K1", 300, 40, [8, 1], [2, 1], 512, [0], num_paths=25, all_valid=True))
    cs.append(_case("per_user_rot", 45, 25, [8, 1], [2, 2], 512, [0, 7], per_user_rot=True))
    cs.append(_case("per_user_rot_fov", 45, 9, [4, 2], [2, 1], 512, [0], per_user_rot=True, ue_fov=[120, 90]))
    for bp, up in (("halfwave-dipole", "isotropic"), ("isotropic", "halfwave-dipole"), ("halfwave-dipole", "halfwave-dipole")):
        cs.append(_case(f"pattern_{bp[:3]}_{up[:3]}", 33, 25, [4, 2], [2, 1], 128, [0, 64], bs_pattern=bp, ue_pattern=up,
                        bs_rot=[20, 10, -60]))
    cs.append(_case("fov_bs", 53, 25, [8, 1], [1, 1], 512, [0], bs_fov=[140, 120]))
    cs.append(_case("fov_ue", 53, 25, [8, 1], [1, 1], 512, [0], ue_fov=[90, 80], ue_rot=[10, 20, 30]))
    cs.append(_case("fov_both", 53, 25, [4, 2], [2, 1], 512, [0, 1, 2], bs_fov=[140, 120], ue_fov=[200, 100], bs_rot=[0, 15, 170]))
    cs.append(_case("fov_full_sphere", 21, 25, [8, 1], [1, 1], 512, [0], bs_fov=[360, 180], ue_fov=[360, 180]))
    cs.append(_case("holes", 64, 25, [8, 1], [1, 1], 512, [0, 3], rays="holes"))
    cs.append(_case("holes_fov", 64, 25, [4, 2], [1, 2], 512, [0], rays="holes", bs_fov=[180, 120]))
    cs.append(_case("kept_counts", 8, 25, [8, 1], [1, 1], 512, [0, 1], rays="kept_counts"))
    cs.append(_case("kept_counts_32", 8, 32, [4, 4], [1, 1], 512, [5], rays="kept_counts"))
    cs.append(_case("delay_clip", 40, 25, [8, 1], [1, 1], 64, [0, 1], max_delay=9e-6))     # 64 / 20 MHz = 3.2 us
    for L in (1, 25, 32, 33, 64):
        for npth in (5, 25, 32):
            cs.append(_case(f"L{L}_np{npth}", 19, L, [4, 2], [2, 1], 256, [0, 17], num_paths=npth))
    for K in (1, 2, 3, 4, 5, 8, 16):
        cs.append(_case(f"K{K}", 30, 25, [8, 1], [1, 1], 512, [(7 * k * k + 3) % 512 for k in range(K)]))
        cs.append(_case(f"K{K}_64pairs", 11, 25, [8, 4], [2, 1], 512, list(range(K))))
    cs.append(_case("sc_negative", 25, 25, [8, 1], [1, 1], 512, [-1, -200, -32768, -70000]))
    cs.append(_case("sc_large", 25, 25, [4, 2], [2, 1], 512, [32768, 40001, 2 ** 31 - 1]))
    cs.append(_case("sc_mixed", 25, 25, [8, 8], [1, 1], 512, [-(2 ** 31), 0, 2 ** 20 + 1]))
    # a 32 x 32 panel at 25 paths needs 205 KB of tables per wave: outside the LDS rule (test_fd_direct_cpu.py); at 19 paths
    # it is the one-wave-per-workgroup launch with the raised dynamic-LDS limit
    cs.append(_case("pairs1024_K2_L19", 9, 19, [32, 32], [1, 1], 512, [0, 1]))
    cs.append(_case("pairs256_K8", 9, 25, [8, 8], [2, 2], 512, list(range(8))))
    return cs


CASES = _all_cases()
SUPPORT = {c["id"]: _host_supported(c["bs_shape"], c["ue_shape"], len(c["selected"]), c["L"], c["num_paths"]) for c in CASES}
TAKEN = [c for c in CASES if SUPPORT[c["id"]] == 1]


def _rays(c):
    from oracle import oracle_np as onp
    rays = onp.synth_rays(c["n"], c["L"], seed=500 + c["n"] + c["L"], all_valid=c["all_valid"] or c["rays"] == "kept_counts",
                          max_delay=c["max_delay"], with_doppler=c["doppler"] is not None)
    keys = [k for k in rays if k not in ("rx_pos", "tx_pos")]
    if c["rays"] == "holes":                                   # NaN in the middle of a row, the same entries of every field
        rng = np.random.default_rng(3)
        hole = rng.uniform(size=rays["power"].shape) < 0.2
        hole[:, 0] |= rng.uniform(size=c["n"]) < 0.3          # the first path too: LoS then comes from a NaN slot
        for k in keys:
            rays[k][hole] = np.nan
    if c["rays"] == "kept_counts":                             # users with 0 / 1 / P - 1 / P kept paths
        P = min(c["num_paths"], c["L"])
        for u, cnt in enumerate([0, 1, P - 1, P, P, 1, 0, P - 1]):
            for k in keys:
                rays[k][u, cnt:] = np.nan
    return rays


def _ue_rot(c):
    if not c["per_user_rot"]:
        return np.array(c["ue_rot"])
    return np.random.default_rng(11).uniform(-180, 180, (c["n"], 3))


def _dm_params(c):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(c["bs_shape"]), np.array(c["ue_shape"])
    p.bs_antenna.spacing, p.ue_antenna.spacing = c["bs_spacing"], c["ue_spacing"]
    p.bs_antenna.rotation = np.array(c["bs_rot"])
    p.ue_antenna.rotation = np.array([0, 0, 0]) if c["per_user_rot"] else np.array(c["ue_rot"])
    p.bs_antenna.radiation_pattern, p.ue_antenna.radiation_pattern = c["bs_pattern"], c["ue_pattern"]
    p.num_paths, p.freq_domain = c["num_paths"], 1
    p.ofdm.subcarriers, p.ofdm.selected_subcarriers = c["subcarriers"], np.array(c["selected"], dtype=np.int64)
    p.ofdm.bandwidth, p.ofdm.rx_filter = c["bandwidth"], 0
    p.enable_doppler = int(bool(c["doppler"]))
    return p


def _kwargs(c, ue_rot):
    bs_fov, ue_fov = fov_args(c)
    kw = dict(bs_fov=bs_fov, ue_fov=ue_fov, carrier_freq=FC)
    if np.ndim(ue_rot) == 2:
        kw["ue_rotation_per_user"] = np.ascontiguousarray(ue_rot, dtype=np.float64)
    return kw


def _both_routes(eng, rays, p, kw):
    """((H, side) of the two calls, (H, side) of the single pass) on the same uploaded rays"""
    import torch
    dr = eng.upload_rays(rays)
    prep = eng.prepare(dr, p, want_side="light", **kw)
    H2 = eng.channels(prep, variant=9)
    H1, side1 = eng.channels_direct(dr, p, want_side="light", **kw)
    torch.cuda.synchronize()
    return (H2, prep.side), (H1, side1)


def _assert_identical(two, one, what):
    import torch
    (H2, s2), (H1, s1) = two, one
    assert H1.shape == H2.shape and H1.dtype == H2.dtype
    same = torch.equal(torch.view_as_real(H1).view(torch.int32), torch.view_as_real(H2).view(torch.int32))
    if not same:
        d = (torch.view_as_real(H1).view(torch.int32) != torch.view_as_real(H2).view(torch.int32))
        users = d.reshape(d.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
        worst = float((H1 - H2).abs().max())
        raise AssertionError(f"{what}: channel bits differ for {len(users)} of {d.shape[0]} users (first {users[:8]}), max |diff| {worst:.3e}")
    for k in ("los", "num_paths", "fov_mask", "max_delay_key"):
        assert (s1.get(k) is None) == (s2.get(k) is None), f"{what}: side product {k} present in one route only"
        if s1.get(k) is not None:
            assert torch.equal(s1[k], s2[k]), f"{what}: side product {k} differs"


def _oracle(c, rays, ue_rot):
    from oracle import oracle_np as onp
    op = oracle_params(c, ue_rot)
    bs_fov, ue_fov = fov_args(c)
    if bs_fov is not None or ue_fov is not None:
        bs_fov = np.array([360, 180]) if bs_fov is None else bs_fov
        ue_fov = np.array([360, 180]) if ue_fov is None else ue_fov
    dop = None
    if c["doppler"]:
        op["enable_doppler"] = 1
        dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=FC)
    return onp.compute_channels(rays, op, bs_fov=bs_fov, ue_fov=ue_fov, doppler=dop)


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def test_every_listed_shape_is_taken():
    """The scope of the kernel covers the whole list (the query is host-only, so this is decided before any launch)."""
    assert [c["id"] for c in CASES if SUPPORT[c["id"]] != 1] == []


@pytest.mark.parametrize("c", TAKEN, ids=[c["id"] for c in TAKEN])
def test_bit_identical_to_two_calls_and_within_bound_of_oracle(c):
    eng = _engine()
    rays, ue_rot = _rays(c), _ue_rot(c)
    p = _dm_params(c).validate(c["n"])
    kw = _kwargs(c, ue_rot)
    assert eng.direct_supported(eng.upload_rays(rays), p, **kw)
    two, one = _both_routes(eng, rays, p, kw)
    _assert_identical(two, one, c["id"])
    # oracle parity, the existing bound of variant 9; masks / LoS / counts exact
    ref = _oracle(c, rays, ue_rot)
    H1, s1 = one
    err = assert_channel_close(H1.cpu().numpy(), ref["channel"], what=c["id"])
    print(f"{c['id']}: worst relative error against the oracle {err:.3e}")
    np.testing.assert_array_equal(s1["los"].cpu().numpy(), ref["los"])
    np.testing.assert_array_equal(s1["num_paths"].cpu().numpy(), ref["num_paths"])
    if s1["fov_mask"] is not None:
        np.testing.assert_array_equal(s1["fov_mask"].cpu().numpy().astype(bool), ref["_fov_mask"])


GOLDEN_K = {}
for _name in GOLDENS:
    _case_, _rays_, _, _ = load_golden(_name)
    _k = min(8, len(_case_["selected"]))
    GOLDEN_K[_name] = (_k, _host_supported(_case_["bs_shape"], _case_["ue_shape"], _k, _rays_["power"].shape[1], _case_["num_paths"]))


def test_all_ten_goldens_are_taken():
    assert {k: v[1] for k, v in GOLDEN_K.items()} == {k: 1 for k in GOLDENS}


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_cut_to_eight_subcarriers(name):
    """The frequency-domain goldens without rx_filter, selection cut to its first <= 8 entries: identical to the two
    calls, and within the bound of the matching slice of the reference-made channel itself."""
    case, rays, ue_rot, ref = load_golden(name)
    k = GOLDEN_K[name][0]
    case = dict(case, selected=list(case["selected"])[:k])
    dop = name == "g10_doppler_v3"
    if np.shape(ue_rot) == (3, 2):                                      # a range: drawn as Dataset.compute_channels draws it
        np.random.seed(1001)
        ue_rot = np.random.uniform(ue_rot[:, 0], ue_rot[:, 1], (rays["power"].shape[0], 3))
    c = dict(case, per_user_rot=np.ndim(ue_rot) == 2, doppler=1 if dop else None, ue_rot=ue_rot if np.ndim(ue_rot) == 1 else [0, 0, 0])
    p = _dm_params(c).validate(rays["power"].shape[0])
    kw = _kwargs(c, ue_rot)
    kw["carrier_freq"] = 3.5e9
    if not dop:
        rays = {k_: v for k_, v in rays.items() if not k_.startswith("doppler")}
    eng = _engine()
    assert eng.direct_supported(eng.upload_rays(rays), p, **kw)
    two, one = _both_routes(eng, rays, p, kw)
    _assert_identical(two, one, name)
    want = ref["channel_doppler"] if dop else ref["channel"]
    assert_channel_close(one[0].cpu().numpy(), want[..., :k], what=name)


def test_user_sub_range_with_guard_regions():
    """user_begin > 0 and a count that is no multiple of the four waves of a workgroup, with a FoV set: the same bits as
    that slice of the full launch, sentinel-filled guard regions before and after the output untouched; and, through
    the C-ABI with caller-owned sentinel-filled side buffers, the side rows (fov_mask, num_paths, los) of the users
    outside the range untouched and those inside equal to the full launch's."""
    import torch
    from oracle import oracle_np as onp
    import deepmimo_amd as dm
    from deepmimo_amd import _native as nat
    n, L, bs, ue, K = 37, 11, [4, 2], [2, 1], 3
    M = bs[0] * bs[1] * ue[0] * ue[1]
    rays = onp.synth_rays(n, L, seed=403)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.num_paths = L
    p.ofdm.selected_subcarriers = np.arange(3, 3 + K)
    p.validate(n)
    kw = dict(bs_fov=np.array([150, 110]))
    eng = _engine()
    dr = eng.upload_rays(rays)
    full, side_full = eng.channels_direct(dr, p, **kw)
    assert side_full["fov_mask"] is not None
    guard, size = 1 << 16, n * M * K
    sentinel = complex(-12345.5, 54321.25)
    big = torch.full((guard + size + guard,), sentinel, dtype=torch.complex64, device="cuda")
    out = big[guard:guard + size].view(n, ue[0] * ue[1], bs[0] * bs[1], K)
    eng.channels_direct(dr, p, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((big[:guard] == sentinel).all()) and bool((big[guard + size:] == sentinel).all()), "write outside the output tensor"
    assert torch.equal(out, full)
    big.fill_(sentinel)
    b, cnt = 5, 15
    structs = eng._call_structs(dr, p, **kw)
    side = dict(fov_mask=torch.full((n, L), 77, dtype=torch.uint8, device="cuda"),
                num_paths=torch.full((n,), -777, dtype=torch.int32, device="cuda"),
                los=torch.full((n,), -777, dtype=torch.int32, device="cuda"),
                max_delay_key=torch.zeros((1,), dtype=torch.int32, device="cuda"))
    s = nat.DmxSide()
    for k, t in side.items():
        setattr(s, k, t.data_ptr())
    rc = eng.lib.dmx_channels_fd_direct(C.byref(structs[1]), C.byref(structs[0]), C.byref(s), b, cnt,
                                        C.c_void_p(out[b:b + cnt].data_ptr()), eng._stream_ptr())
    nat.check(rc, "dmx_channels_fd_direct")
    torch.cuda.synchronize()
    assert bool((big[:guard] == sentinel).all()) and bool((big[guard + size:] == sentinel).all())
    assert bool((out[:b] == sentinel).all()) and bool((out[b + cnt:] == sentinel).all())
    assert torch.equal(out[b:b + cnt], full[b:b + cnt])
    for k, fill in (("fov_mask", 77), ("num_paths", -777), ("los", -777)):
        assert torch.equal(side[k][b:b + cnt], side_full[k][b:b + cnt]), k
        assert bool((side[k][:b] == fill).all()) and bool((side[k][b + cnt:] == fill).all()), f"{k}: row of a user outside the range written"
    # the running maximum covers the users of the range only
    want = float(np.nanmax(rays["delay"][b:b + cnt, :L])) if np.isfinite(rays["delay"][b:b + cnt]).any() else float("nan")
    got = float(eng.lib.dmx_decode_max_delay(int(side["max_delay_key"].cpu().numpy().astype(np.uint32)[0])))
    assert got == np.float32(want)


def test_unsupported_shape_raises_and_names_the_two_calls():
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    rays = onp.synth_rays(6, 65, seed=1)
    p = dm.ChannelGenParameters()
    p.num_paths = 25
    p.validate(6)
    eng = _engine()
    dr = eng.upload_rays(rays)
    assert not eng.direct_supported(dr, p)
    with pytest.raises(NativeError, match="dmx_path_prep"):
        eng.channels_direct(dr, p)


class _Spy:
    """Counts the calls of every entry point made through a library handle"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("dmx_"):
            return f

        def wrapped(*a, **k):
            self.calls.append(name)
            return f(*a, **k)
        return wrapped


def _api_run(single_pass, variant, rays, capsys):
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    eng = dsm._engine()
    spy = _Spy(eng.lib)
    eng.lib = spy
    dm.config("single_pass", single_pass)
    dm.config("fd_kernel_variant", variant)
    dm.config("channel_output", "torch")
    try:
        ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
        capsys.readouterr()
        H = ds.compute_channels(dm.ChannelGenParameters())
        printed = capsys.readouterr().out
        before_heavy = list(spy.calls)
        light = dict(los=ds.los, num_paths=ds.num_paths)
        after_light = list(spy.calls)
        heavy = dict(aoa_az_rot=ds["_aoa_az_rot"], aod_el_rot=ds["_aod_el_rot"], power_linear=ds.power_linear)
        after_heavy = list(spy.calls)
    finally:
        eng.lib = spy._lib
        dm.config("single_pass", "auto")
        dm.config("fd_kernel_variant", 0)
        dm.config("channel_output", "numpy")
    return H, printed, light, heavy, before_heavy, after_light, after_heavy


def test_public_api_routes_and_side_products(capsys):
    """compute_channels(ChannelGenParameters()): 'auto' makes ONE dmx_channels_fd_direct call and no dmx_path_prep until
    a heavy side product is read; False and an explicit variant 9 make the two calls; tensors, light and lazily read
    heavy side products and the printed symbol-duration warning are equal."""
    import torch
    from oracle import oracle_np as onp
    rays = onp.synth_rays(300, 25, seed=21, max_delay=80e-6)                 # 512 / 10 MHz = 51.2 us: the warning prints
    auto = _api_run("auto", 0, rays, capsys)
    off = _api_run(False, 0, rays, capsys)
    v9 = _api_run("auto", 9, rays, capsys)
    assert auto[4].count("dmx_channels_fd_direct") == 1 and "dmx_path_prep" not in auto[4] and "dmx_channels_fd" not in auto[4]
    assert "dmx_path_prep" not in auto[5], "LoS / path counts must come from the fused kernel"
    assert auto[6].count("dmx_path_prep") == 1, "rotated angles and powers come from one deferred stage-1 pass"
    for other in (off, v9):
        assert "dmx_channels_fd_direct" not in other[6]
        assert other[4].count("dmx_path_prep") == 1 and other[4].count("dmx_channels_fd") == 1
        assert torch.equal(auto[0], other[0])
        assert "exceed OFDM symbol duration" in auto[1] and auto[1] == other[1]
        for k in auto[2]:
            np.testing.assert_array_equal(auto[2][k], other[2][k])
        for k in auto[3]:
            np.testing.assert_array_equal(auto[3][k], other[3][k])


def test_public_api_fov_mask_and_numpy_output():
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(90, 25, seed=22)
    res = {}
    for sp in ("auto", False):
        dm.config("single_pass", sp)
        try:
            ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
            ds.apply_fov(bs_fov=np.array([140, 120]))
            H = ds.compute_channels(dm.ChannelGenParameters())
            res[sp] = (H, ds["_fov_mask"], ds.los, ds.num_paths, ds["_aod_az_rot_fov"])
        finally:
            dm.config("single_pass", "auto")
    assert isinstance(res["auto"][0], np.ndarray)
    for a, b in zip(res["auto"], res[False]):
        np.testing.assert_array_equal(a, b)


def test_at_size_default_call_is_identical_and_repeatable():
    """200k users x 25 paths, DeepMIMO's default arrays, one subcarrier: every user bit-equal to the two calls, and a
    second launch bit-equal to the first."""
    import torch
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    n = 200_000
    rays = onp.synth_rays(n, 25, seed=5)
    p = dm.ChannelGenParameters().validate(n)
    eng = _engine()
    two, one = _both_routes(eng, rays, p, dict(carrier_freq=FC))
    _assert_identical(two, one, "200k default call")
    H_again, side_again = eng.channels_direct(eng.upload_rays(rays), p, carrier_freq=FC)
    torch.cuda.synchronize()
    _assert_identical(one, (H_again, side_again), "second launch")


def test_at_size_more_than_32_loaded_paths_zero_rotation():
    """100k users x 40 loaded paths (25 used), default arrays and rotations, one subcarrier - the shape class in which
    stage 1 runs its general lean form because the zero-rotation form exists up to 32 loaded paths only: every table
    entries of antenna phases (3e7), bit-equal to the two calls."""
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    n = 100_000
    rays = onp.synth_rays(n, 40, seed=6, all_valid=True)
    p = dm.ChannelGenParameters()
    p.ue_antenna.shape = np.array([2, 2])
    p.validate(n)
    eng = _engine()
    assert eng.direct_supported(eng.upload_rays(rays), p, carrier_freq=FC)
    two, one = _both_routes(eng, rays, p, dict(carrier_freq=FC))
    _assert_identical(two, one, "100k users x 40 loaded paths")
