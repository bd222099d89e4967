"""Near field (DMX_FLAG_NEAR_FIELD) without a GPU: the header and the C-ABI's host-only answers, the view of
`Dataset.near_field` with every ValueError of the Python layer, the NumPy helpers, the reference of tests/_near_field_ref.py
against plain geometry (element positions and distances, not its formula), and the case table of tests/_near_field_cases.py:
every case shows the effect by far more than the tolerance, and the float32 delay moves no case by 1 % of it."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import _near_field_cases as NC
from tests import _near_field_ref as NF
from tests._cases import TOL_REL
from tests.test_wideband_cpu import _header, _lib, _params as _wb_params

FLAG, WIDEBAND = 16, 4


def _params(nat, flags=FLAG, fc=28e9, bw=4e8):
    p = _wb_params(nat, flags, fc)
    p.bandwidth = bw
    return p


# ---- 1. header and ABI, host only -----------------------------------------------------------------------------------------------
def test_header_defines_the_flag():
    nat, lib = _lib()
    header = _header()
    assert re.search(r"#define\s+DMX_FLAG_NEAR_FIELD\s+16u\b", header) and re.search(r"#define\s+DMX_ABI_VERSION\s+3\b", header)
    assert nat.FLAG_NEAR_FIELD == FLAG and nat.ABI_VERSION == 3 and lib.dmx_version() == 3
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(dmx_\w+)\s*\(", code)) == set(nat.EXPORTED_SYMBOLS)


def _entry_calls(nat, lib, p):
    """name -> (zero-user call, takes the flag) for every entry point and query of the issue's table"""
    r, s = nat.DmxRays(), nat.DmxSide()
    pp = C.byref(p)
    link = (nat.DmxLink * 1)()
    link[0].prm, link[0].n_paths_loaded, link[0].snr_linear = C.pointer(p), 5, 10.0
    cb = (C.c_float * 32)()
    raw = (C.c_char * 512)()                                                  # a 256-byte aligned beam workspace, never read
    beam_ws = C.c_void_p((C.addressof(raw) + 255) & ~255)
    taken = {
        "dmx_path_prep": lambda: lib.dmx_path_prep(C.byref(r), pp, None, 0, None, None),
        "dmx_channels_fd": lambda: lib.dmx_channels_fd(pp, None, 0, 5, 0, 0, None, 0, None),
        "dmx_channels_fd variant 1": lambda: lib.dmx_channels_fd(pp, None, 0, 5, 0, 0, None, 1, None),
        "dmx_beam_power": lambda: lib.dmx_beam_power(pp, None, 0, 5, 0, 0, cb, 1, beam_ws, 256, None, None, None),
        "dmx_channel_covariance": lambda: lib.dmx_channel_covariance(pp, None, 0, 5, 0, 0, 0, None, None),
        "dmx_channel_rate": lambda: lib.dmx_channel_rate(pp, None, 0, 5, 0, 0, 10.0, None, None, None),
        "dmx_channel_spectrum": lambda: lib.dmx_channel_spectrum(pp, None, 0, 5, 0, 0, 10.0, None, None, None, None),
        "dmx_channel_precoders": lambda: lib.dmx_channel_precoders(pp, None, 0, 5, 0, 0, 10.0, 1, None, None, None, None),
        "dmx_cell_rate": lambda: lib.dmx_cell_rate(link, 1, 0, 0, 0, None, None, None, None, None, None),
        "dmx_channels_angle_delay": lambda: lib.dmx_channels_angle_delay(pp, None, 0, 5, 0, 0, None, 8, None, 0, 8, 4, None, None),
        "dmx_codebook_rate": lambda: lib.dmx_codebook_rate(pp, None, 0, 5, 0, 0, None, 4, 1, None, 0, 10.0, None, None, None, None),
        "dmx_codebook_rate_subbands": lambda: lib.dmx_codebook_rate_subbands(pp, None, 0, 5, 0, 0, None, 4, 1, None, 0, 10.0, 4, None,
                                                                             None, None, None, None, None, None),
    }
    supported = {
        "dmx_covariance_supported": lambda: lib.dmx_covariance_supported(pp, 5, 0),
        "dmx_rate_supported": lambda: lib.dmx_rate_supported(pp, 5),
        "dmx_spectrum_supported": lambda: lib.dmx_spectrum_supported(pp, 5),
        "dmx_precoder_supported": lambda: lib.dmx_precoder_supported(pp, 5, 1),
        "dmx_cell_rate_supported": lambda: lib.dmx_cell_rate_supported(link, 1),
        "dmx_angle_delay_supported": lambda: lib.dmx_angle_delay_supported(pp, 5, 8, 8, 4),
        "dmx_codebook_rate_supported": lambda: lib.dmx_codebook_rate_supported(pp, 5, 4, 1),
        "dmx_codebook_rate_subbands_supported": lambda: lib.dmx_codebook_rate_subbands_supported(pp, 5, 4, 1, 4),
    }
    refused = {
        "dmx_channels_fd_lpf": lambda: lib.dmx_channels_fd_lpf(pp, None, 0, 5, 0, 0, None, 0, None, None),
        "dmx_channels_td": lambda: lib.dmx_channels_td(pp, None, 0, 5, 0, 0, None, None),
        "dmx_channels_fd_beams": lambda: lib.dmx_channels_fd_beams(pp, None, 0, 5, 0, 0, None, 0, None, 0, None, None),
        "dmx_channels_fd_direct": lambda: lib.dmx_channels_fd_direct(C.byref(r), pp, C.byref(s), 0, 0, None, None),
        "dmx_fd_direct_supported": lambda: lib.dmx_fd_direct_supported(pp, 5),
    }
    return taken, supported, refused, (link, cb, raw)


def test_every_entry_point_takes_or_refuses_the_flag_as_listed():
    nat, lib = _lib()
    p = _params(nat)
    taken, supported, refused, _link = _entry_calls(nat, lib, p)
    for flags in (FLAG, FLAG | nat.FLAG_ADAPTIVE_TERMS):
        p.flags = flags
        for name, call in taken.items():
            assert call() == 0, (name, flags, lib.dmx_last_error())
        for name, call in supported.items():
            p.flags = 0
            want = call()
            p.flags = flags
            assert call() == want == 1, (name, flags, lib.dmx_last_error())      # the shape limits of the far field
        for name, call in refused.items():
            assert call() == -1, (name, flags)
            assert b"DMX_FLAG_NEAR_FIELD" in lib.dmx_last_error(), (name, lib.dmx_last_error())
    p.flags = 0
    for name, call in list(taken.items()) + list(refused.items()):
        if name in ("dmx_channels_fd_lpf", "dmx_channels_td", "dmx_channels_fd_direct"):
            continue                                                             # refuse these parameters for other reasons
        assert call() in (0, 1), (name, lib.dmx_last_error())
    for flags in (FLAG, FLAG | 1):
        assert lib.dmx_fd_kernel_choice(C.byref(_params(nat, flags)), 25) == 1
    big = _params(nat)
    big.bs_shape[0], big.bs_shape[1], big.ue_shape[0], big.ue_shape[1] = 64, 4, 2, 2
    big.n_selected = 512
    assert lib.dmx_fd_kernel_choice(C.byref(big), 25) == 1
    big.flags = 0
    assert lib.dmx_fd_kernel_choice(C.byref(big), 25) != 1                      # the flag decides, not the shape


@pytest.mark.parametrize("variant", [2, 9, 12, 3, 5])
def test_other_channel_variants_are_a_shape_error(variant):
    nat, lib = _lib()
    assert lib.dmx_channels_fd(C.byref(_params(nat)), None, 0, 5, 0, 0, None, variant, None) == -2
    assert b"DMX_FLAG_NEAR_FIELD" in lib.dmx_last_error() and b"variant" in lib.dmx_last_error()
    assert lib.dmx_channels_fd(C.byref(_params(nat, flags=0)), None, 0, 5, 0, 0, None, variant, None) == 0


@pytest.mark.parametrize("field,value", [("carrier_freq", 0.0), ("carrier_freq", -28e9), ("carrier_freq", float("nan")),
                                         ("carrier_freq", float("inf")), ("bandwidth", float("inf")), ("bandwidth", float("nan")),
                                         ("bandwidth", 0.0)])
def test_a_bad_carrier_or_bandwidth_is_refused_wherever_the_flag_is_taken(field, value):
    nat, lib = _lib()
    p = _params(nat)
    taken, supported, _refused, _link = _entry_calls(nat, lib, p)
    setattr(p, field, value)
    for name, call in list(taken.items()) + list(supported.items()):
        assert call() == -1, (name, field, value)
        msg = lib.dmx_last_error()
        assert (b"DMX_FLAG_NEAR_FIELD" in msg and field.encode() in msg) or (field == "bandwidth" and b"ofdm.bandwidth" in msg), (name, msg)
    if field == "carrier_freq":
        p.flags = 0                                                              # without the flag nothing changes
        for name, call in taken.items():
            assert call() == 0, (name, lib.dmx_last_error())


def test_flag_combinations():
    nat, lib = _lib()
    p = _params(nat)
    taken, supported, refused, _link = _entry_calls(nat, lib, p)
    every = list(taken.items()) + list(supported.items()) + list(refused.items())
    p.flags = FLAG | WIDEBAND
    for name, call in every:
        assert call() == -1, name
        assert b"DMX_FLAG_NEAR_FIELD | DMX_FLAG_SPATIAL_WIDEBAND" in lib.dmx_last_error(), (name, lib.dmx_last_error())
    for flags in (2, 8, FLAG | 2, FLAG | 8, 32, FLAG | 32):
        p.flags = flags
        for name, call in every:
            assert call() == -1, (name, flags)
            assert b"unknown bits" in lib.dmx_last_error(), (name, flags, lib.dmx_last_error())
    p.flags, p.reserved0 = FLAG, 1
    for name, call in every:
        assert call() == -1 and b"unknown bits" in lib.dmx_last_error(), name


def test_cell_rate_links_may_differ_in_flag_and_carrier():
    nat, lib = _lib()
    ps = [_params(nat, FLAG, 28e9), _params(nat, 0, 0.0), _params(nat, FLAG | 1, 3.5e9)]
    links = (nat.DmxLink * 3)()
    for i, p in enumerate(ps):
        links[i].prm, links[i].n_paths_loaded, links[i].snr_linear = C.pointer(p), 5, 10.0
    assert lib.dmx_cell_rate_supported(links, 3) == 1, lib.dmx_last_error()
    assert lib.dmx_cell_rate(links, 3, 0, 0, 0, None, None, None, None, None, None) == 0, lib.dmx_last_error()
    ps[2].carrier_freq = 0.0
    assert lib.dmx_cell_rate(links, 3, 0, 0, 0, None, None, None, None, None, None) == -1
    assert b"DMX_FLAG_NEAR_FIELD" in lib.dmx_last_error() and b"carrier_freq" in lib.dmx_last_error()


# ---- 2. the view -------------------------------------------------------------------------------------------------------------------
def _dataset(with_carrier=True, n=6):
    import deepmimo_amd as dm
    ds = dm.Dataset(dict(onp.synth_rays(n, 5, seed=2, with_doppler=True)))
    if with_carrier:
        ds["rt_params"] = {"frequency": 28e9}
    return ds


def _dm_params(**ofdm):
    import deepmimo_amd as dm
    p = dm.ChannelGenParameters()
    p.ofdm.selected_subcarriers = np.arange(8)
    for k, v in ofdm.items():
        setattr(p.ofdm, k, v)
    return p


def test_view_is_a_plain_dataset_sharing_the_arrays():
    import deepmimo_amd as dm
    ds = _dataset()
    ds.set_channel_params(_dm_params())
    view = ds.near_field()
    assert type(view) is dm.Dataset and view.near_field_carrier == 28e9 and int(view.n_ue) == int(ds.n_ue)
    for k in ("power", "phase", "delay", "aoa_az", "aod_el", "inter", "doppler_vel"):
        assert view[k] is ds[k], k                                               # shared, not copied
    assert "near_field_carrier" not in ds._data
    assert ds.near_field(3.5e9).near_field_carrier == 3.5e9 and ds.near_field("6e9").near_field_carrier == 6e9
    assert view.ch_params is not ds.ch_params and view.ch_params.ofdm.subcarriers == ds.ch_params.ofdm.subcarriers
    # subset and at_times carry the entry
    assert view.subset(np.array([0, 3])).near_field_carrier == 28e9
    t = view.at_times([0.0, 1e-3])
    assert t.near_field_carrier == 28e9 and int(t.n_ue) == 2 * int(ds.n_ue)
    assert ds.at_times([0.0, 1e-3]).near_field().near_field_carrier == 28e9
    macro = dm.MacroDataset([_dataset(), _dataset()]).near_field(5e9)
    assert isinstance(macro, dm.MacroDataset) and [d.near_field_carrier for d in macro.datasets] == [5e9, 5e9]


@pytest.mark.parametrize("fc", [0.0, -1.0, float("nan"), float("inf"), "x"])
def test_view_needs_a_carrier(fc):
    with pytest.raises(ValueError, match="near_field: no carrier frequency"):
        _dataset().near_field(fc)
    with pytest.raises(ValueError, match="near_field: no carrier frequency"):
        _dataset(with_carrier=False).near_field()


def _all_calls(view, p):
    """every compute_* that runs on the view: each has to raise before it needs a GPU"""
    cb = np.ones((2, 8), np.complex64)
    return {"compute_channels": lambda: view.compute_channels(p),
            "iter_channels": lambda: next(view.iter_channels(p, 3)),
            "compute_channels times": lambda: view.compute_channels(p, times=[0.0, 1e-3]),
            "compute_covariance": lambda: view.compute_covariance(p),
            "compute_rate": lambda: view.compute_rate(p, snr_db=10.0),
            "compute_eigenmodes": lambda: view.compute_eigenmodes(p, snr_db=10.0),
            "compute_precoders": lambda: view.compute_precoders(p, snr_db=10.0),
            "compute_angle_delay": lambda: view.compute_angle_delay(p),
            "compute_codebook_rate": lambda: view.compute_codebook_rate(p, snr_db=10.0),
            "compute_subband_pmi": lambda: view.compute_subband_pmi(p, snr_db=10.0),
            "compute_beam_power": lambda: view.compute_beam_power(cb, p)}


def test_python_refusals_need_no_gpu():
    import deepmimo_amd as dm
    td = _dm_params()
    td.freq_domain = 0
    for name, call in _all_calls(_dataset().near_field(), td).items():
        with pytest.raises(ValueError):                                          # a consumer refuses the time domain by itself
            call()
    for name in ("compute_channels", "iter_channels", "compute_channels times", "compute_beam_power"):
        with pytest.raises(ValueError, match="near_field.*freq_domain"):
            _all_calls(_dataset().near_field(), td)[name]()
    for name, call in _all_calls(_dataset().near_field(), _dm_params(rx_filter=1)).items():
        with pytest.raises(ValueError):
            call()
    for name in ("compute_channels", "iter_channels", "compute_channels times", "compute_beam_power"):
        with pytest.raises(ValueError, match="near_field.*rx_filter"):
            _all_calls(_dataset().near_field(), _dm_params(rx_filter=1))[name]()
    p = _dm_params()
    view = _dataset().near_field()
    for call in (lambda: view.compute_channels(p, spatial_wideband=True), lambda: next(view.iter_channels(p, 3, spatial_wideband=True)),
                 lambda: view.compute_channels(p, spatial_wideband=True, times=[0.0])):
        with pytest.raises(ValueError, match="near_field: spatial_wideband"):
            call()
    try:
        for v in (2, 9, 12):
            dm.config("fd_kernel_variant", v)
            for name in ("compute_channels", "iter_channels", "compute_channels times"):
                with pytest.raises(ValueError, match=f"near_field: fd_kernel_variant {v}"):
                    _all_calls(_dataset().near_field(), p)[name]()
    finally:
        dm.config("fd_kernel_variant", 0)
    with pytest.raises(ValueError, match="compute_beam_channels: not covered on a near-field view"):
        view.compute_beam_channels(np.ones((2, 8), np.complex64), p)
    with pytest.raises(ValueError, match="with_rx_combiner: not covered on a near-field view"):
        view.with_rx_combiner("dft", p)
    with pytest.raises(ValueError, match="compute_beam_pair_power: not covered on a near-field view"):
        view.compute_beam_pair_power(np.ones((2, 8), np.complex64), "dft", p)
    with pytest.raises(ValueError, match="near-field view"):
        from deepmimo_amd import dist
        dist.compute_channels_sharded(view, p.validate(6))
    # a carrier spoilt after the view was made
    view._data["near_field_carrier"] = float("nan")
    with pytest.raises(ValueError, match="near_field: no carrier frequency"):
        view.compute_channels(p)


def test_engine_check_and_routes():
    from deepmimo_amd import engine
    p = _dm_params().validate(6)
    assert engine.check_near_field_call(p, 28e9) == 28e9 and engine.check_near_field_call(p, "3e9", 1) == 3e9
    with pytest.raises(ValueError):
        engine.check_near_field_call(p, None)
    with pytest.raises(ValueError):
        engine.check_near_field_call(p, 28e9, 2)
    ok = dict(single_pass="auto", fd_kernel_variant=0, adaptive_precision=False, direct_supported=True, auto_choice=9, one_piece=True)
    assert engine.single_pass_route(**ok) and not engine.single_pass_route(**ok, near_field=True)
    assert not engine.single_pass_route(**dict(ok, single_pass=True), near_field=True)


# ---- 3. the helpers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,spacing,theta,phi", [([8, 1], 0.5, 1.1, 0.4), ([4, 3], 0.37, 0.3, -2.0), ([33, 1], 0.5, np.pi / 2, 0.0),
                                                     ([1, 1], 0.5, 0.2, 0.1)])
def test_near_field_response_limits(shape, spacing, theta, phi):
    import deepmimo_amd as dm
    M = int(np.prod(shape))
    plane = dm.near_field_response(shape, spacing, theta, phi, np.inf)
    assert plane.shape == (M,) and plane.dtype == np.complex128
    sv = dm.steering_vec(np.array(shape), phi=np.degrees(theta), theta=np.degrees(phi) - 90.0, spacing=spacing)[:, 0] * np.sqrt(M)
    assert np.abs(plane - sv).max() <= 1e-9
    assert np.abs(dm.near_field_response(shape, spacing, theta, phi, 1e15) - plane).max() <= 1e-9
    assert np.all(np.abs(np.abs(dm.near_field_response(shape, spacing, theta, phi, 7.0)) - 1) < 1e-12)
    assert dm.near_field_response(shape, spacing, theta, phi, 7.0)[0] == 1.0     # element 0 is the reference
    # the helper is the reference's psi
    idx = onp.ant_indices(shape)
    q = spacing * (idx[:, 1] * np.sin(theta) * np.sin(phi) + idx[:, 2] * np.cos(theta))
    for R in (0.0, 0.3, 7.0, 1e4):
        want = NF.psi(q[:, None], NF.element_s(shape, spacing), np.array([[R]]))[:, 0]
        assert np.abs(dm.near_field_phase(shape, spacing, theta, phi, R) - want).max() <= 1e-12 * max(1.0, R)
    with pytest.raises(ValueError):
        dm.near_field_response(shape, spacing, theta, phi, -1.0)


def test_focus_codebook_and_fraunhofer_distance():
    import deepmimo_amd as dm
    cb = dm.focus_codebook([16, 2], 0.5, np.array([1.0, 1.2, np.pi / 2]), np.array([0.3, -0.3, 0.0]), np.array([20.0, 200.0, np.inf]))
    assert cb.shape == (3, 32) and cb.dtype == np.complex128
    assert np.abs(np.linalg.norm(cb, axis=1) - 1).max() <= 1e-12
    # a row collects sqrt(M) from its own focal point, less from the same direction at another distance
    a = dm.near_field_response([16, 2], 0.5, 1.0, 0.3, 20.0)
    assert abs(cb[0] @ a - np.sqrt(32)) <= 1e-9
    far = dm.focus_codebook([16, 2], 0.5, 1.0, 0.3, np.inf)[0]
    assert abs(far @ a) < 0.8 * np.sqrt(32)
    assert dm.fraunhofer_distance([64, 1], 0.5) == 2 * 31.5 ** 2
    assert dm.fraunhofer_distance([3, 5], 0.5) == 2 * 0.25 * (4 + 16) and dm.fraunhofer_distance([1, 1]) == 0.0
    # 64-element half-wavelength ULA at 28 GHz: 21 m
    assert abs(dm.fraunhofer_distance([64, 1]) * 299792458.0 / 28e9 - 21.25) < 0.05


# ---- 4. the reference against geometry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [[33, 1], [5, 3]])
@pytest.mark.parametrize("apertures", [2, 10, 1000])
def test_reference_is_the_distance_to_each_element(bs, apertures):
    H, want = los_geometry(bs, apertures, lambda rays, op, fc: NF.near_field_channels(rays, op, fc))
    assert np.abs(H[0, 0, :, :] / H[0, 0, 0, :] - want[:, None]).max() <= 1e-9


def los_geometry(bs, apertures, channels, spacing=0.5, fc=NC.CARRIER):
    """One LoS path of a single-antenna UE at `apertures` panel diagonals, angles and delay exactly representable in float32:
    (what `channels(rays, oracle params, fc)` returns, exp(-j 2pi (|x_ue - x_t| - |x_ue - x_0|)) per BS element t) with the
    element positions from the panel geometry and the UE position from the path's direction and length, in float64"""
    D = spacing * np.hypot(bs[0] - 1, bs[1] - 1)
    delay = np.float32(apertures * D / fc)
    rays = {"power": np.float32([[-70.0]]), "phase": np.float32([[45.0]]), "delay": np.array([[delay]], np.float32),
            "aoa_az": np.float32([[0.0]]), "aoa_el": np.float32([[90.0]]), "aod_az": np.float32([[60.5]]),
            "aod_el": np.float32([[71.25]]), "inter": np.float32([[0.0]])}
    op = onp.make_params(bs_antenna=dict(shape=bs, spacing=spacing), ue_antenna=dict(shape=[1, 1]), num_paths=1, freq_domain=1,
                         ofdm=dict(subcarriers=NC.N_SC, selected_subcarriers=np.array([0, 3]), bandwidth=NC.BANDWIDTH, rx_filter=0))
    prep = onp.prepare_paths(rays, op)
    theta, phi = float(prep["_aod_el_rot"][0, 0]), float(prep["_aod_az_rot"][0, 0])
    R = float(delay) * fc                                                        # wavelengths
    x_ue = R * np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])
    x_el = spacing * onp.ant_indices(bs).astype(np.float64)                      # (0, y, z) d: the panel in its y-z plane
    dist = np.linalg.norm(x_ue[None, :] - x_el, axis=1)
    return channels(rays, op, fc), np.exp(-2j * np.pi * (dist - dist[0]))


# ---- 5. teeth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in NC.CASES])
def test_case_shows_the_effect_and_the_delay_rounding_is_negligible(cid):
    case = NC.BY_ID[cid]
    nf, ff, tol = NC.references(case)
    peak = np.abs(nf).reshape(len(nf), -1).max(axis=1)
    assert 5 <= case["n"] <= 21 and np.all(nf[2] == 0) and np.all(ff[2] == 0) and (peak > 0).sum() >= 3
    diff = np.abs(nf - ff).reshape(len(nf), -1).max(axis=1)
    ok = peak > 0
    assert np.max(diff[ok] / tol[ok]) > 100, (cid, np.max(diff[ok] / tol[ok]))
    term = tol - TOL_REL * peak
    assert np.all(term[ok] >= 0) and np.any(term > 0) and np.max(term[ok] / (TOL_REL * peak[ok])) < 0.01, (cid, np.max(term[ok] / (TOL_REL * peak[ok])))


def test_table_covers_what_the_issue_lists():
    ch = NC.CHANNEL_CASES
    assert {tuple(c["bs"]) for c in ch} >= {(16, 1), (33, 1), (8, 4), (3, 5)}
    assert {tuple(c["ue"]) for c in ch} == {(1, 1), (2, 2), (3, 1)}
    assert {len(c["sel"]) for c in ch} >= {1, 5, 64, 70}
    assert any(c["sel"].min() < 0 for c in ch) and any(c["sel"].max() >= c["N"] for c in ch)
    assert {c["kept"] for c in ch if c["kept"] is not None} >= {1, 7, 32, 40}
    assert min(c["n"] for c in ch) == 5 and max(c["n"] for c in ch) == 21
    assert any(c["holes"] for c in ch)
    pairs = lambda c: int(np.prod(c["bs"]) * np.prod(c["ue"]))                  # noqa: E731
    assert any(pairs(c) <= 8 for c in ch) and any(pairs(c) > 8 for c in ch)     # one wave per user, and four
    x = NC.FULL_CASE["extras"]
    assert x["ue_rot"] == "per_user" and x["doppler"] and {x["bs_pattern"], x["ue_pattern"]} == {"tr38901", "halfwave-dipole"}
    for c in NC.CASES:
        r = NC.case_rays(c)
        assert r["delay"][0, 0] == 0.0 and np.isfinite(r["power"][0, 0])          # a path of delay 0
        R = r["delay"].astype(np.float64) * NC.CARRIER / NC.aperture(c)
        R = R[np.isfinite(R) & (R > 0)]
        assert R.min() >= 2 * (1 - 1e-6) and R.max() <= 1000 * (1 + 1e-6)
        assert np.all(r["delay"][np.isfinite(r["delay"])] * NC.BANDWIDTH < 0.5 * c["N"])     # nothing is clipped
    spans = [r for c in ch for r in [NC.case_rays(c)["delay"].astype(np.float64) * NC.CARRIER / NC.aperture(c)]]
    assert min(np.nanmin(np.where(s > 0, s, np.nan)) for s in spans) < 2.5 and max(np.nanmax(s) for s in spans) > 900
    cons = NC.CONSUMER_CASES
    assert {tuple(c["bs"]) for c in cons} == {(16, 1), (8, 4)} and {tuple(c["ue"]) for c in cons} == {(1, 1), (2, 2)}
    assert {len(c["sel"]) for c in cons} == {1, 5, 70} and {c["kept"] for c in cons} == {1, 7, 32}
