"""GPU parity at negative and large subcarrier indices.  ofdm.selected_subcarriers may hold any integers: the reference
evaluates exp(-j 2pi dn k / N) in float64 for every k (channel.py:166-168, 196-197), centred grids np.arange(-N/2, N/2)
and indices far beyond N included.  Every route against the float64 oracle at the parity tolerance (tests/_cases.py),
LoS and path counts bit for bit:

- the matrix-core kernel on 256 rows (variants 0, 1, 4, 5, 10) and on 32 rows (the run-time-guarded tile body, 0, 4, 5),
  the default arrays 8x1 / 1x1 (0, 12 folded, 9 small-output); on variants 4 and 5 every uniform selection must take the
  factorised B' (k2_mfma_frag.h fact_b_step, whose strip phase E1 starts at sc_first + 16 stride strip);
- rx_filter = 1 on the FFT forms (N = 512, 1024) and the direct kernel (N = 100), Doppler with and without it;
- the beam entry points;
- DMX_SC_ABS_MAX_F32 (include/deepmimo_amd.h): beyond it variant 0 takes the float64-phase kernels and the float32-phase
  ones refuse, in the engine (ValueError) and in the C-ABI (DMX_ERR_ARG), with real device buffers.

Families whose |k| comes within 300 of 2^15 (edge+, edge-) are the largest magnitudes inside the bound; each case prints
its worst error relative to the user's peak (pytest -s) for the per-route report."""
import ctypes as C

import numpy as np
import pytest

from tests._cases import oracle_params, assert_channel_close
from tests.test_gpu_parity import _dm_params, _small_kernel_fits, check_beam_channels, check_beam_power

pytestmark = pytest.mark.gpu

N0 = 512
FAMILIES = {
    "centred": np.arange(-N0 // 2, N0 // 2),
    "neg": np.arange(-512, 0),
    "straddle": np.arange(-40, 216),                     # crosses 0 inside the strip -8..7
    "centred_s2": np.arange(-63, 65, 2),
    "single_neg": np.array([-5]),                        # K = 1: hint (-5, 1)
    "split+": np.arange(3996, 4196),                     # across the 4096 split of the phase reduction
    "split-": np.arange(-4146, -4046),
    "edge+": np.arange(2 ** 15 - 300, 2 ** 15),
    "edge-": np.arange(-2 ** 15 + 1, -2 ** 15 + 301),
    "irregular": np.sort(np.random.default_rng(15).choice(np.arange(-2 ** 15 + 1, 2 ** 15), 64, replace=False)),
}
FAM = list(FAMILIES)

# route: (BS panel, UE panel, users, paths, all paths valid, variants)
ROUTES = {
    "mfma256": ([8, 8], [2, 2], 16, 25, True, (0, 1, 4, 5, 10)),
    "mfma32": ([4, 4], [2, 1], 24, 25, False, (0, 4, 5)),
    "default8": ([8, 1], [1, 1], 32, 25, False, (0, 12, 9)),
}
SEEDS = {"mfma256": 1, "mfma32": 2, "default8": 3}


def _uniform(sel):
    from deepmimo_amd.engine import uniform_stride
    return uniform_stride(sel)[1] > 0


def _cases():
    out = []
    for r, (bs, ue, n, L, _, variants) in ROUTES.items():
        for v in variants:
            for f in FAM:
                if v == 12 and not _uniform(FAMILIES[f]):
                    continue                             # the folded kernel needs the spacing promise
                if v == 9 and not _small_kernel_fits((n, L, bs, ue, N0, FAMILIES[f], {})):
                    continue
                out.append(pytest.param(r, v, f, id=f"{r}-v{v}-{f}"))
    return out


def _case(bs, ue, L, N, sel, rx_filter=0):
    return dict(bs_shape=bs, ue_shape=ue, bs_spacing=0.5, ue_spacing=0.37, bs_rot=[0, 0, 0],
                bs_pattern="isotropic", ue_pattern="isotropic", num_paths=L, freq_domain=1, subcarriers=N,
                selected=list(np.asarray(sel)), bandwidth=20e6, rx_filter=rx_filter, bs_fov=None, ue_fov=None)


_RAYS = {}


def _rays(n, L, all_valid, seed, doppler=False):
    from oracle import oracle_np as onp
    key = (n, L, all_valid, seed, doppler)
    if key not in _RAYS:
        _RAYS[key] = onp.synth_rays(n, L, seed=seed, all_valid=all_valid, max_delay=20e-6, with_doppler=doppler)
    return _RAYS[key]


def _oracle(rays, case, doppler=False, fc=28e9):
    from oracle import oracle_np as onp
    op = oracle_params(case, np.zeros(3))
    op["enable_doppler"] = int(doppler)
    dop = dict(vel=rays["doppler_vel"], acc=rays["doppler_acc"], carrier_freq=fc) if doppler else None
    return onp.compute_channels(rays, op, doppler=dop)


def _channels(rays, case, variant=0, doppler=False, fc=28e9, hint=True, monkeypatch=None):
    """the library's channels through Dataset.compute_channels; hint=False withholds the spacing promise
    (dmx_params.sc_stride = 0), which sends a uniform selection through the sin/cos B' generation"""
    import deepmimo_amd as dm
    import deepmimo_amd.engine as eng
    if not hint:
        monkeypatch.setattr(eng, "uniform_stride", lambda sel: (0, 0))
    dm.config("fd_kernel_variant", variant)
    try:
        ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
        p = _dm_params(case, np.zeros(3))
        if doppler:
            ds["rt_params"] = {"frequency": fc}
            p.enable_doppler = 1
        H = ds.compute_channels(p)
        return H, ds
    finally:
        dm.config("fd_kernel_variant", 0)
        if not hint:
            monkeypatch.undo()


def _check(H, ds, ref, what):
    err = assert_channel_close(H, ref["channel"], what=what)
    np.testing.assert_array_equal(ds.los, ref["los"])
    np.testing.assert_array_equal(ds.num_paths, ref["num_paths"])
    print(f"subcarrier-index parity {what}: worst rel err {err:.3e}")
    return err


@pytest.mark.parametrize("route,variant,family", _cases())
def test_channels(route, variant, family, monkeypatch):
    bs, ue, n, L, all_valid, _ = ROUTES[route]
    sel = FAMILIES[family]
    rays = _rays(n, L, all_valid, seed=SEEDS[route])
    case = _case(bs, ue, L, N0, sel)
    ref = _oracle(rays, case)
    H, ds = _channels(rays, case, variant)
    _check(H, ds, ref, f"{route} v{variant} {family}")
    if variant in (4, 5) and _uniform(sel) and len(sel) > 1:
        # the factorised B' ran: the same selection without the promise (sin/cos B') rounds differently, and meets the
        # oracle too.  (K = 1 is left out: its only E2 phasor is exactly 1, so both generations may agree bit for bit.)
        Hs, dss = _channels(rays, case, variant, hint=False, monkeypatch=monkeypatch)
        _check(Hs, dss, ref, f"{route} v{variant} {family} sin/cos")
        assert not np.array_equal(H, Hs), f"{family} on variant {variant} did not take the factorised B' generation"


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("N", [512, 1024, 100])
def test_rx_filter(N, family):
    """rx_filter = 1: FFT forms at N = 512 (k3_lpf_fft_pow2, one radix-8 butterfly per lane and pass; arange(-512, 0) is
    sc[k] = k mod 512, the `ident` store of the promise) and 1024 (the same kernel, a last pass of radix 16), the direct kernel at N = 100 (floor-mod of a negative index)"""
    from deepmimo_amd.engine import uniform_stride
    sel = FAMILIES[family]
    if family == "centred":
        sel = np.arange(-(N // 2), N // 2)
    if family == "neg" and N == 512:
        first, stride = uniform_stride(sel)
        assert stride == 1 and first & 511 == 0 and len(sel) <= 512
    rays = _rays(12, 25, False, seed=N)
    case = _case([4, 4], [2, 1], 25, N, sel, rx_filter=1)
    ref = _oracle(rays, case)
    H, ds = _channels(rays, case)
    _check(H, ds, ref, f"rx_filter N={N} {family}")


@pytest.mark.parametrize("rx_filter", [0, 1])
@pytest.mark.parametrize("route", ["mfma256", "default8"])
def test_doppler_centred(route, rx_filter):
    bs, ue, n, L, all_valid, _ = ROUTES[route]
    rays = _rays(12, L, all_valid, seed=77, doppler=True)
    case = _case(bs, ue, L, N0, FAMILIES["centred"], rx_filter=rx_filter)
    ref = _oracle(rays, case, doppler=True)
    H, ds = _channels(rays, case, doppler=True)
    _check(H, ds, ref, f"{route} doppler rx_filter={rx_filter} centred")


def _beam_setup(bs, ue, L, sel, n, seed):
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(n, L, seed=seed)
    p = dm.ChannelGenParameters()
    p.bs_antenna.shape, p.ue_antenna.shape = np.array(bs), np.array(ue)
    p.num_paths = L
    p.ofdm.selected_subcarriers = sel
    op = onp.make_params(bs_antenna=dict(shape=bs), ue_antenna=dict(shape=ue), num_paths=L,
                         ofdm=dict(selected_subcarriers=sel))
    ref = onp.compute_channels(rays, op)
    m_tx = bs[0] * bs[1]
    F1 = np.array([dm.steering_vec(np.array(bs), phi=a).squeeze() for a in np.around(np.linspace(-60, 60, 16), 2)])
    rng = np.random.default_rng(seed)
    F2 = (rng.normal(size=(5, m_tx)) + 1j * rng.normal(size=(5, m_tx))) * 11.0
    return rays, p, ref, (F1.reshape(16, m_tx), F2)


@pytest.mark.parametrize("family", ["centred", "straddle", "irregular"])
@pytest.mark.parametrize("bs,ue", [([8, 8], [2, 2]), ([8, 1], [1, 1])], ids=["8x8_2x2", "8x1_1x1"])
def test_beam_channels_and_power(bs, ue, family):
    import deepmimo_amd as dm
    rays, p, ref, Fs = _beam_setup(bs, ue, 25, FAMILIES[family], 40, seed=len(family) + bs[1])
    Href = ref["channel"].astype(np.complex128)
    ds = dm.Dataset(dict(rays))
    for F in Fs:
        check_beam_channels(ds, p, F, Href)
        check_beam_power(rays, p, F, Href, ref["los"], part=(7, 20))


# ---- DMX_SC_ABS_MAX_F32 -------------------------------------------------------------------------------------------
BEYOND = {
    "2^22": np.arange(2 ** 22, 2 ** 22 + 512),
    "2^24_s7": np.arange(2 ** 24 + 3, 2 ** 24 + 3 + 7 * 256, 7),
    "irregular_2^30": np.sort(np.random.default_rng(30).choice(np.arange(2 ** 30 - 10 ** 6, 2 ** 30 + 10 ** 6), 200,
                                                               replace=False)),
}


@pytest.mark.parametrize("family", list(BEYOND))
def test_beyond_bound_auto_takes_float64_phases(family):
    """Auto routing beyond the bound meets the oracle and is the fp32 vector kernel's result bit for bit; the
    factorised path before the bound existed missed the tolerance at the first two selections"""
    bs, ue, n, L, all_valid, _ = ROUTES["mfma256"]
    rays = _rays(n, L, all_valid, seed=5)
    case = _case(bs, ue, L, N0, BEYOND[family])
    ref = _oracle(rays, case)
    H, ds = _channels(rays, case, 0)
    _check(H, ds, ref, f"beyond {family} auto")
    H1, _ = _channels(rays, case, 1)
    np.testing.assert_array_equal(H, H1)


def test_beyond_bound_few_subcarriers_take_the_small_kernel():
    bs, ue = [8, 1], [1, 1]
    rays = _rays(32, 25, False, seed=6)
    case = _case(bs, ue, 25, N0, np.arange(2 ** 22, 2 ** 22 + 8))
    ref = _oracle(rays, case)
    H, ds = _channels(rays, case, 0)
    _check(H, ds, ref, "beyond 2^22 K=8 auto")
    H9, _ = _channels(rays, case, 9)
    np.testing.assert_array_equal(H, H9)


@pytest.mark.parametrize("family", list(BEYOND))
def test_beyond_bound_float32_routes_refuse(family):
    """Engine: an explicit matrix-core / folded variant and every beam call raise ValueError.  C-ABI (the engine's
    prepared workspace and device buffers, the engine's checks bypassed): with the spacing promise the library returns
    DMX_ERR_ARG naming the bound"""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd.dataset import _engine
    bs, ue, n, L = [8, 8], [2, 2], 8, 25
    sel = BEYOND[family]
    rays = _rays(n, L, True, seed=8)
    case = _case(bs, ue, L, N0, sel)
    for v in (2, 5, 12):
        with pytest.raises(ValueError, match="32768"):
            _channels(rays, case, v)
    p = _dm_params(case, np.zeros(3))
    F = np.ones((4, 64), dtype=np.complex64)
    with pytest.raises(ValueError, match="32768"):
        dm.Dataset(dict(rays)).compute_beam_channels(F, p)
    with pytest.raises(ValueError, match="32768"):
        dm.Dataset(dict(rays)).compute_beam_power(F, p)

    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), p.validate(n))
    assert prep.sc_abs_max == int(np.abs(sel).max())
    ps = prep.params_struct
    if ps.sc_stride == 0:                                # irregular: the library cannot see the range
        return
    lib, dev = eng.lib, eng.device
    K = len(sel)
    out = torch.empty((n, 4, 64, K), dtype=torch.complex64, device=dev)
    wsp = C.c_void_p(prep.workspace.data_ptr())
    stream = eng._stream_ptr()
    for v in (2, 3, 4, 5, 8, 10, 11, 12):
        assert lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, C.c_void_p(out.data_ptr()), v, stream) == -1, v
        assert b"DMX_SC_ABS_MAX_F32" in lib.dmx_last_error()
    assert lib.dmx_fd_kernel_choice(C.byref(ps), L) == 1
    cb = torch.ones((4, 64), dtype=torch.complex64, device=dev)
    nbytes = int(lib.dmx_beam_workspace_bytes(C.byref(ps), n, L, 4))
    bws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    bptr = C.c_void_p(bws.data_ptr() + (-bws.data_ptr()) % 256)
    assert lib.dmx_channels_fd_beams(C.byref(ps), wsp, n, L, 0, n, C.c_void_p(cb.data_ptr()), 4, bptr, nbytes,
                                     C.c_void_p(out.data_ptr()), stream) == -1
    assert b"DMX_SC_ABS_MAX_F32" in lib.dmx_last_error()
    amp = torch.empty((n, 4), dtype=torch.float32, device=dev)
    assert lib.dmx_beam_power(C.byref(ps), wsp, n, L, 0, n, C.c_void_p(cb.data_ptr()), 4, bptr, nbytes,
                              C.c_void_p(amp.data_ptr()), None, stream) == -1
    assert b"DMX_SC_ABS_MAX_F32" in lib.dmx_last_error()
    # the float64-phase variants run on the same buffers and agree with the oracle
    for v in (1, 9):
        out.zero_()
        assert lib.dmx_channels_fd(C.byref(ps), wsp, n, L, 0, n, C.c_void_p(out.data_ptr()), v, stream) == 0
        torch.cuda.synchronize(dev)
        assert_channel_close(out.cpu().numpy(), _oracle(rays, case)["channel"], what=f"beyond {family} C-ABI v{v}")


def test_indices_outside_int32_raise_before_upload():
    rays = _rays(8, 25, True, seed=9)
    for sel in ([2 ** 31], [0, -2 ** 31 - 1], [5, 2 ** 40]):
        with pytest.raises(ValueError, match="int32"):
            _channels(rays, _case([8, 8], [2, 2], 25, N0, np.array(sel, dtype=np.int64)))
    # int32's own extremes are accepted (float64-phase routing) and match the oracle
    case = _case([8, 8], [2, 2], 25, N0, np.array([-2 ** 31, 2 ** 31 - 1, 7]))
    H, ds = _channels(rays, case)
    _check(H, ds, _oracle(rays, case), "int32 extremes")
