"""k5_pathloss at its edges: the user tail of the last workgroup (8 users per workgroup), path counts around the lane
loop's step of 32 (L = 0 included), NaN in the power or only in the phase, in the first lane or only in the second trip,
rows with no valid path, rows at -inf dB, and nearly cancelling rows.

Through the direct ABI, with `out` inside a sentinel-filled buffer, and through ChannelEngine.pathloss; coherent and
incoherent.  The NaN mask is the float64 reference's (tests/_pathloss_ref.py) and every other user is within
2e-4 dB * max(1, kappa) of it, kappa = sum |g| / |sum g| being the row's condition number.

Measured on an MI355X over all cases: worst error 0.12 of the tolerance (incoherent, kappa 1; 0.08 coherent), largest
kappa 3.5e3.
"""
import ctypes as C

import numpy as np
import pytest

from tests._pathloss_ref import cases, ref_pathloss, tolerance

pytestmark = pytest.mark.gpu

CASES = cases()
GUARD = 64
SENTINEL = -777.25


def _direct(eng, power, phase, n_ue, L, coherent):
    """dmx_pathloss on device tensors, `out` in the middle of a sentinel buffer: the whole buffer on the host"""
    import torch
    from deepmimo_amd import _native as nat
    buf = torch.full((GUARD + n_ue + GUARD,), SENTINEL, dtype=torch.float32, device=eng.device)
    out = buf[GUARD: GUARD + n_ue]
    r = nat.DmxRays()
    r.n_ue, r.n_paths, r.ld = n_ue, L, L
    if n_ue * L > 0:
        r.power, r.phase = power.data_ptr(), phase.data_ptr()
    with torch.cuda.device(eng.device):
        rc = eng.lib.dmx_pathloss(C.byref(r), int(coherent), C.c_void_p(out.data_ptr()), eng._stream_ptr())
    nat.check(rc, "dmx_pathloss")
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("coherent", [True, False], ids=["coherent", "incoherent"])
def test_pathloss_edges_against_the_float64_reference(coherent):
    import torch
    from deepmimo_amd import consts
    from deepmimo_amd.engine import ChannelEngine, DeviceRays
    eng = ChannelEngine(0)
    worst, worst_kappa, worst_at = 0.0, 0.0, None
    for c in CASES:
        n_ue, L = c["n_ue"], c["L"]
        power = torch.from_numpy(c["power"].copy()).to(eng.device)
        phase = torch.from_numpy(c["phase"].copy()).to(eng.device)
        host = _direct(eng, power, phase, n_ue, L, coherent)
        assert np.all(host[:GUARD] == np.float32(SENTINEL)), f"{c['id']}: wrote in front of out"
        assert np.all(host[GUARD + n_ue:] == np.float32(SENTINEL)), f"{c['id']}: wrote behind out (the idle users of the last workgroup)"
        got = host[GUARD: GUARD + n_ue]
        want, kappa = ref_pathloss(c["power"], c["phase"], coherent)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (c["id"], c["kinds"], got, want)
        if L == 0:
            assert np.isnan(got).all()
        ok = ~np.isnan(want)
        ratio = np.abs(got[ok].astype(np.float64) - want[ok]) / tolerance(kappa[ok])
        if ratio.size:
            print(f"{c['id']} coherent={coherent}: worst error / tolerance {ratio.max():.3f}, largest kappa {kappa[ok].max():.3g}")
            if ratio.max() > worst:
                worst, worst_at = float(ratio.max()), (c["id"], np.array(c["kinds"])[ok][int(ratio.argmax())])
            worst_kappa = max(worst_kappa, float(kappa[ok].max()))
        assert np.all(ratio <= 1.0), (c["id"], c["kinds"], got, want, kappa)
        # the engine's own call: the same bits
        fields = {consts.POWER_PARAM_NAME: power, consts.PHASE_PARAM_NAME: phase}
        via = eng.pathloss(DeviceRays(n_ue=n_ue, n_paths=L, fields=fields), coherent)
        assert via.shape == (n_ue,) and via.dtype == torch.float32
        assert np.array_equal(via.cpu().numpy().view(np.int32), got.view(np.int32)), c["id"]
    print(f"pathloss coherent={coherent}: worst error / tolerance {worst:.3f} at {worst_at}; largest kappa {worst_kappa:.4g}")


def test_pathloss_of_no_user_is_ok():
    import torch
    from deepmimo_amd.engine import ChannelEngine
    eng = ChannelEngine(0)
    some = torch.zeros((4, 3), dtype=torch.float32, device=eng.device)
    for L in (0, 3):
        host = _direct(eng, some, some, 0, L, True)
        assert np.all(host == np.float32(SENTINEL))
