"""rx_filter = 1 on the three gain kernels the fast N = 512 / 64 / 128 / 256 / 1024 kernels leave over: the generic
wave-per-path FFT k3_lpf_fft_wave (every call at N = 2048, K > N, more than 64 path slots), the radix-2 workgroup FFT
k3_lpf_fft (N = 2 .. 32 and 4096) and the direct kernel k3_lpf_gains (any other N).  The cases, their rays and the float64
reference are those of tests/_lpf_routes.py; tests/test_rx_filter_routes_cpu.py ties the route of every case to the
dispatcher's text and holds the condition that makes the parity bound mean something (a lost or misplaced gain row of
the equal-power user moves H by at least twice the bound).  Per case, with Doppler off and on:

  parity      Dataset.compute_channels against oracle_np at the suite's TOL_REL / TOL_ABS; LoS and path counts exact;
  sub-range   eng.channels(prep, user_begin=3, user_count=5) is rows 3 .. 7 of the whole call, bit for bit (the kernels index
              the table by the user inside the call and the workspace by the user of the preparation);
  the table   where it holds floats: dmx_channels_fd_lpf through ctypes on a caller-owned workspace filled with a
              sentinel; every kept path's row within TOL_REL of that row's own peak of lpf_gain_rows, every row past a
              user's kept count and the alignment tail still the sentinel; again with user_begin = 3.

The packed f16 table is not decoded: its routes are covered by the parity check with the equal-power user.  Every case
prints its worst error / bound (pytest -s); the module prints the table BASELINE.md quotes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _lpf_routes as R
from tests._cases import TOL_ABS, TOL_REL, assert_channel_close, channel_err
from tests.test_gpu_parity import _dm_params

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1.2345e30)
WORST = {}                                   # (case, arrays) -> {"H": .., "table": ..} worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for (cid, arrays), w in WORST.items():
        c = R.CASES_BY_ID[cid]
        tab = f"{w['table']:.3f}" if "table" in w else "packed"
        print(f"rx_filter routes: {cid} {arrays} ({R.route_of(c)}): worst error / bound H {w['H']:.3f}, table rows {tab}")


def _ratio(H, Href):
    d, peak = channel_err(H, Href)
    live = peak > 0
    return float(np.max(d[live] / (TOL_REL * peak[live] + TOL_ABS))) if live.any() else 0.0


def _table(eng, prep, case, m_rx, m_tx, begin, count):
    """dmx_channels_fd_lpf on a caller-owned, 256-byte-aligned workspace filled with SENTINEL: (the [count, P, K] complex64
    table, the floats behind it up to the workspace's size, the channels)"""
    lib, dev, ps = eng.lib, eng.device, prep.params_struct
    K, P = ps.n_selected, case.L
    nbytes = int(lib.dmx_lpf_workspace_bytes(C.byref(ps), count, case.L))
    assert nbytes >= count * P * K * 8 and nbytes % 256 == 0
    buf = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    off = ((-buf.data_ptr()) % 256) // 4
    ws = buf[off:off + nbytes // 4]
    assert ws.data_ptr() % 256 == 0
    buf.fill_(float(SENTINEL))
    out = torch.empty((count, m_rx, m_tx, K), dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dmx_channels_fd_lpf(C.byref(ps), C.c_void_p(prep.workspace.data_ptr()), prep.n_ue, case.L, begin, count,
                                     C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(out.data_ptr()), eng._stream_ptr())
    assert rc == 0, lib.dmx_last_error()
    torch.cuda.synchronize(dev)
    host = buf.cpu().numpy()
    assert np.all(host[:off] == SENTINEL) and np.all(host[off + nbytes // 4:] == SENTINEL), "wrote outside the workspace"
    flat = host[off:off + nbytes // 4]
    n = count * P * K * 2
    return flat[:n].view(np.complex64).reshape(count, P, K), flat[n:], out


def _check_table(tab, tail, rows, what):
    """every kept row within TOL_REL of its own peak, everything else untouched; returns the worst error / bound"""
    assert np.all(tail == SENTINEL), f"{what}: wrote behind the table"
    worst = 0.0
    for ul, g in enumerate(rows):
        n = g.shape[0]
        rest = tab[ul, n:]
        assert np.all(rest.real == SENTINEL) and np.all(rest.imag == SENTINEL), f"{what}: user {ul} wrote past its {n} kept paths"
        if n == 0:
            continue
        got = tab[ul, :n].astype(np.complex128)
        assert np.isfinite(got).all(), f"{what}: user {ul} has NaN, inf or untouched entries in a kept row"
        peak = np.abs(g).max(axis=1)
        assert np.all(peak > 0)
        r = np.abs(got - g).max(axis=1) / (TOL_REL * peak)
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, (f"{what}: user {ul} path {int(np.argmax(r))} of {n}: row error {r.max() * TOL_REL:.3e} of the "
                                f"row's peak (tol {TOL_REL})")
    return worst


@pytest.mark.parametrize("cid,arrays", R.GPU_CASES, ids=[f"{c}-{a}" for c, a in R.GPU_CASES])
def test_route(cid, arrays):
    import deepmimo_amd as dm
    from deepmimo_amd.dataset import _engine
    case = R.CASES_BY_ID[cid]
    rays = R.case_rays(case)
    cd = R.case_dict(case, arrays)
    n, nu = case.n_ue, case.oracle_users or case.n_ue
    bs, ue = R.ARRAYS[arrays]
    m_rx, m_tx = ue[0] * ue[1], bs[0] * bs[1]
    float_table = not R.packed(case, arrays)
    eng = _engine()
    worst = WORST.setdefault((cid, arrays), {"H": 0.0})
    for dop in (0, 1):
        what = f"{cid} {arrays} ({R.route_of(case)}) doppler={dop}"
        ref = R.oracle(case, arrays, dop)
        p = _dm_params(cd, np.zeros(3))
        p.enable_doppler = dop
        ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
        ds["rt_params"] = {"frequency": R.FC}
        H = ds.compute_channels(p)
        assert H.shape[0] == n and ref["channel"].shape[0] == nu
        r = _ratio(H[:nu], ref["channel"])
        print(f"\nrx_filter routes {what}: H worst error / bound {r:.3f}")
        worst["H"] = max(worst["H"], r)
        assert_channel_close(H[:nu], ref["channel"], what=what)
        np.testing.assert_array_equal(ds.los, ref["los"])
        np.testing.assert_array_equal(ds.num_paths, ref["num_paths"])

        # the engine on one preparation: the whole call, a sub-range, and the table itself
        prep = eng.prepare(eng.upload_rays({k: v.copy() for k, v in rays.items()}), p.validate(n), want_side="light",
                           carrier_freq=R.FC)
        assert prep.params_struct.enable_doppler == dop and prep.params_struct.rx_filter == 1
        full = eng.channels(prep)
        part = eng.channels(prep, user_begin=R.SUB_BEGIN, user_count=R.SUB_COUNT)
        torch.cuda.synchronize()
        assert_channel_close(full[:nu].cpu().numpy(), ref["channel"], what=what + " engine")
        assert torch.equal(torch.view_as_real(part), torch.view_as_real(full[R.SUB_BEGIN:R.SUB_BEGIN + R.SUB_COUNT])), \
            f"{what}: users {R.SUB_BEGIN} .. {R.SUB_BEGIN + R.SUB_COUNT - 1} differ when launched on their own"
        if not float_table:
            continue
        rows = R.lpf_gain_rows(rays, cd, bool(dop))
        for begin, count in ((0, n), (R.SUB_BEGIN, R.SUB_COUNT)):
            tab, tail, out = _table(eng, prep, case, m_rx, m_tx, begin, count)
            assert torch.equal(torch.view_as_real(out), torch.view_as_real(full[begin:begin + count])), (what, begin)
            rt = _check_table(tab, tail, rows[begin:begin + count], f"{what} table of users {begin} .. {begin + count - 1}")
            print(f"rx_filter routes {what}: table rows of users {begin} .. {begin + count - 1} worst error / bound {rt:.3f}")
            worst["table"] = max(worst.get("table", 0.0), rt)
        del prep, full, part


def test_more_than_4096_subcarriers_are_refused():
    """N = 4100: the direct kernel's taps and roots would need 65,600 B of LDS; the library says so"""
    import deepmimo_amd as dm
    from deepmimo_amd._native import NativeError
    from oracle import oracle_np as onp
    assert R.lpf_route(4100, 4, 9) == "refused" and R.lpf_route(4096, 4, 9) == "fft" and R.lpf_route(4095, 4, 9) == "gains"
    rays = onp.synth_rays(8, 9, seed=4100, max_delay=1e-4)
    cd = dict(R.case_dict(R.CASES_BY_ID["g4000"], "valu"), subcarriers=4100, selected=[0, 1, 5, 4099])
    ds = dm.Dataset(dict(rays))
    with pytest.raises(NativeError, match=r"at most 4096 subcarriers \(got 4100\)"):
        ds.compute_channels(_dm_params(cd, np.zeros(3)))
