"""Transmit precoding and multi-user rates on the GPU: the channels of the `with_tx_precoder` view against H @ f of the
NumPy oracle, `compute_mu_rate` against the definition (tests/_mu_ref.py) at its derived tolerance, the cross-checks against
`compute_codebook_rate` and `MacroDataset.compute_cell_rate`, determinism (two calls, a forced block split, host and HBM
rays, NumPy and torch output, the order of the groups), and the view under `at_times` and behind `with_rx_combiner`.

The cases are those of tests/_mu_cases.py - at most 21 users, one without a path and one with a single path in each.

Worst error / tolerance measured on the MI355X: see the README paragraph "Transmit precoding and multi-user rates"."""
import os

import numpy as np
import pytest

from tests import _mu_cases as CS
from tests import _mu_ref as MR
from tests._cases import TOL_REL

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_parity import _dm_params  # noqa: E402

R = MR.R


def _dataset(rays, case, place="host"):
    import torch
    import deepmimo_amd as dm
    put = (lambda v: torch.from_numpy(v.copy()).cuda()) if place == "hbm" else (lambda v: v.copy())
    ds = dm.Dataset({k: put(v) for k, v in rays.items()})
    if case["bs_fov"] is not None:
        ds.apply_fov(bs_fov=np.array(case["bs_fov"]))
    return ds


def _np(x):
    return x.cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


_refs = {}


def _mu_reference(name):
    """the reference of a multi-user case, computed once and left unchanged"""
    if name not in _refs:
        case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
        _refs[name] = MR.mu_reference(rays, op, F, beams, groups, snr_db)
        for a in _refs[name].values():
            a.setflags(write=False)
    return _refs[name]


def _mu_call(name, place=None, **kw):
    case, op, rays, F, beams, groups, snr_db, where = CS.mu_setup(name)
    ds = _dataset(rays, case, place or where)
    return ds.compute_mu_rate(F, beams, groups, _dm_params(case, CS.UE_ROT), snr_db=snr_db, **kw)


# ---------------------------------------------------------------------------------------------- 1. the channels of the view
@pytest.mark.parametrize("name", list(CS.VIEW_CASES))
def test_view_channels_match_the_precoded_oracle_channels(name):
    case, op, fov, rays, F, beams, place = CS.view_setup(name)
    n, B = rays["power"].shape[0], len(F)
    ds = _dataset(rays, case, place)
    view = ds.with_tx_precoder(F, beams, _dm_params(case, CS.UE_ROT))
    idx = np.broadcast_to(np.arange(B)[:, None], (B, n)) if beams is None else np.asarray(beams).reshape(-1, n)
    J = len(idx)
    ref, tol = MR.view_reference(rays, op, F, idx, *fov)                              # [J, n, M_rx, K], [J, n]
    assert view.n_ue == J * n and view.n_tx_beams == J and list(view.ch_params.bs_antenna.shape) == [1, 1]
    assert hasattr(view.power, "detach") == (place == "hbm")                           # precoded where the rays live
    H = view.compute_channels()
    assert H.shape == (J * n, ref.shape[2], 1, ref.shape[3]) and H.dtype == np.complex64
    got = view.split_tx_beams(H)
    assert np.shares_memory(got, H)
    assert R.worst_ratio(got[:, :, :, 0], ref, tol, what=name) <= 1.0
    assert (tol > 0).sum() >= J * 3 and np.all(got[:, CS.NO_PATH_USER] == 0)
    off = idx < 0
    assert off.any() == (beams is not None)
    paths = view.split_tx_beams(np.asarray(view.num_paths))
    assert np.all(got[off] == 0) and np.all(paths[off] == 0) and np.all(paths[~off] == np.asarray(ds.num_paths)[np.nonzero(~off)[1]])


# ---------------------------------------------------------------------------------------------- 2. the multi-user rate
@pytest.mark.parametrize("name", list(CS.MU_CASES))
def test_mu_rate_matches_the_definition(name):
    case, op, rays, F, beams, groups, snr_db, place = CS.mu_setup(name)
    ref = _mu_reference(name)
    n, G, K = len(beams), groups.shape[1], len(case["selected"])
    rate, rate_k, partners, stream = _mu_call(name, per_subcarrier=True, details=True)
    assert rate.shape == (n,) and rate_k.shape == (n, K) and partners.shape == (n, G - 1) and stream.shape == (n, G)
    assert rate.dtype == rate_k.dtype == stream.dtype == np.float32 and partners.dtype == np.int32
    assert MR.worst(rate, ref["rate"], ref["tol"], what=f"{name}: rate") <= 1.0
    assert MR.worst(rate_k, ref["rate_k"], ref["tol_k"], what=f"{name}: rate_k") <= 1.0
    assert np.array_equal(partners, ref["partners"])
    assert MR.worst(stream, ref["stream_snr"], ref["stream_tol"], what=f"{name}: stream_snr") <= 1.0
    idle = ref["size"] == 0
    assert idle.any() and np.all(rate[idle] == 0) and np.all(rate_k[idle] == 0) and np.all(stream[idle] == 0)
    assert rate[CS.NO_PATH_USER] == 0 and rate[~idle].max() > 0.5
    # the rate alone is the same rate
    assert _mu_call(name).tobytes() == rate.tobytes()


# ---------------------------------------------------------------------------------------------- 3. cross-checks
def test_single_user_groups_against_the_codebook_rate_and_the_cell_rate():
    import deepmimo_amd as dm
    from tests._codebook_rate_ref import codebook_rate_tolerance
    name = "G2_ue2x1_K64_P25_snr30"
    case, op, rays, F, beams, _, snr_db, _ = CS.mu_setup(name)
    n = len(beams)
    alone = np.arange(n)[:, None]
    p = _dm_params(case, CS.UE_ROT)
    ds = _dataset(rays, case, "hbm")
    rate = ds.compute_mu_rate(F, beams, alone, p, snr_db=snr_db)
    ref = MR.mu_reference(rays, op, F, beams, alone, snr_db)
    assert MR.worst(rate, ref["rate"], ref["tol"], what="groups of one") <= 1.0
    # the codeword of each user in the per-codeword rates of the codebook call
    _, _, rate_c = ds.compute_codebook_rate(p, codebook=F, snr_db=snr_db, per_codeword=True)
    tol_c = codebook_rate_tolerance(ref["H"], F[:, None, :], 10 ** (snr_db / 10))[0]
    rows = np.arange(n)
    assert MR.worst(rate, rate_c[rows, beams], ref["tol"] + tol_c[rows, beams], what="against compute_codebook_rate") <= 1.0
    assert rate.max() > 3.0
    # the multi-cell call on the same view, one link: bit for bit
    view = ds.with_tx_precoder(F, beams, p)
    cell = dm.MacroDataset([view]).compute_cell_rate(snr_db=snr_db)
    assert cell.tobytes() == rate.tobytes()


def test_a_partner_never_raises_the_rate():
    name = "G2_ue2x1_K64_P25_snr30"
    case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
    ref, n = _mu_reference(name), len(beams)
    p = _dm_params(case, CS.UE_ROT)
    ds = _dataset(rays, case)
    paired = ds.compute_mu_rate(F, beams, groups, p, snr_db=snr_db)
    members = groups[groups >= 0]
    alone = ds.compute_mu_rate(F, beams, members[:, None], p, snr_db=snr_db)
    tol_alone = MR.mu_reference(rays, op, F, beams, members[:, None], snr_db, H=ref["H"])["tol"]
    assert np.all(paired <= alone + ref["tol"] + tol_alone)
    assert ((alone - paired) > 10 * (ref["tol"] + tol_alone))[ref["size"] == 2].sum() >= (ref["size"] == 2).sum() // 2


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_same_bits_from_every_way_to_run_it(monkeypatch):
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd import dataset as dsm
    from deepmimo_amd.engine import ChannelEngine
    name = "G4_ue2x2_K70_P32_snr-10"
    case, op, rays, F, beams, groups, snr_db, _ = CS.mu_setup(name)
    n, L, G = len(beams), rays["power"].shape[1], groups.shape[1]
    kw = dict(per_subcarrier=True, details=True)
    first = _mu_call(name, "host", **kw)
    for what, again in (("a second call", _mu_call(name, "host", **kw)), ("rays in HBM", _mu_call(name, "hbm", **kw))):
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), what
    # torch output: the same bits, in HBM
    dm.config("channel_output", "torch")
    try:
        as_torch = _mu_call(name, "host", **kw)
    finally:
        dm.config("channel_output", "numpy")
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in as_torch)
    for a, b in zip(first, as_torch):
        assert a.tobytes() == b.cpu().numpy().tobytes() and a.dtype == b.cpu().numpy().dtype
    # a forced split into blocks of five users
    launches = []
    real = ChannelEngine.cell_rate
    monkeypatch.setattr(ChannelEngine, "cell_rate", lambda self, preps, *a, **k: (launches.append(preps[0].n_ue), real(self, preps, *a, **k))[1])
    monkeypatch.setattr(dsm, "_TIME_BLOCK_BYTES", 5 * 4 * L * 10 * G)
    split = _mu_call(name, "host", **kw)
    assert launches == [5, 5, n - 10]
    for a, b in zip(first, split):
        assert a.tobytes() == b.tobytes()
    monkeypatch.undo()
    # the order of the groups' rows changes nothing
    ds = _dataset(rays, case)
    shuffled = ds.compute_mu_rate(F, beams, groups[::-1].copy(), _dm_params(case, CS.UE_ROT), snr_db=snr_db, **kw)
    for a, b in zip(first, shuffled):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- 5. composition
_PLAIN = {**CS.BASE, "bs_shape": [4, 2], "ue_shape": [2, 2], "selected": list(range(64))}


def test_the_view_over_time_in_either_order():
    """Against the time-series reference (tests/_time_series_ref.py) precoded with F[beams]; the tolerance adds the float32
    rounding of the advanced phase, 2 pi 2^-24 on the path moduli behind the precoder."""
    from tests import _time_series_ref as TS
    from tests._cases import oracle_params
    times, fc = (0.0, 1e-4, 0.7), 28e9
    n, L, T = 7, 8, 3
    rays = CS.rays(n, L, with_doppler=True)
    op, p = oracle_params(_PLAIN, CS.UE_ROT), _dm_params(_PLAIN, CS.UE_ROT)
    F = CS.codebook(("random", 5), [4, 2])
    beams = CS.view_beams("per_user", n, 5)
    idx = beams[None]
    H_t = TS.reference_channels(rays, op, times, fc).astype(np.complex128)             # [T, n, M_rx, M_tx, K]
    prep = R.prepared(rays, op)
    a, _ = MR._moduli(rays, prep, op, F, idx, None)
    extra = 2 * np.pi * 2.0 ** -24 * a.sum(axis=2) + MR.rounding_term(rays, prep, op, F, idx)          # [1, n]
    ds = _dataset(rays, _PLAIN)
    views = {"at_times first": ds.at_times(times, carrier_freq=fc).with_tx_precoder(F, np.tile(beams, T), p),
             "precoder first": ds.with_tx_precoder(F, beams, p).at_times(times, carrier_freq=fc)}
    for what, view in views.items():
        assert view.n_ue == T * n
        H = view.compute_channels().reshape(T, n, 4, 1, 64)
        for t in range(T):
            ref = MR.precoded(H_t[t], F, idx)
            tol = TOL_REL * np.abs(ref).max(axis=(2, 3)) + extra
            assert R.worst_ratio(H[t][None, :, :, 0], ref, tol, what=f"{what}, snapshot {t}") <= 1.0
    moved = np.abs(MR.precoded(H_t[2] - H_t[0], F, idx)).max(axis=(2, 3))
    assert (moved > 100 * tol).sum() >= n // 2                                         # the snapshots differ: it can fail


def test_the_view_behind_a_receive_combiner_in_either_order():
    """y[u, q, k] = W[q] @ H[u, :, :, k] @ F[beams[u]]: the tolerance carries the roundings of both views on the path
    moduli |c_l| |e_tx| |e_rx|."""
    from tests._cases import oracle_params
    n, L, Q = 7, 8, 3
    rays = CS.rays(n, L)
    op, p = oracle_params(_PLAIN, CS.UE_ROT), _dm_params(_PLAIN, CS.UE_ROT)
    F, W = CS.codebook(("random", 5), [4, 2]), CS.codebook(("random", Q), [2, 2])
    beams = CS.view_beams("per_user", n, 5)
    Y = MR.precoded(MR.oracle_channels(rays, op), F, beams[None])[0]                   # [n, M_rx, K]
    ref = np.einsum("qr,urk->quk", W, Y)[:, :, None, :]                                # [Q, n, 1, K]
    prep = R.prepared(rays, op)
    e_tx = np.abs(MR.tx_responses(prep, op, F, beams[None]))[0][:, None, :L]            # [n, 1, L]
    e_rx = np.abs(R.responses(prep, op, W))[:, :, :L]                                   # [n, Q, L]
    c = R.path_moduli(prep, op)[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        db = np.asarray(rays["power"], np.float64)[:, None, :]
        p_tx, p_rx = db + 20 * np.log10(e_tx), db + 20 * np.log10(e_rx)
        both = np.abs(np.nan_to_num(p_tx + 20 * np.log10(e_rx), neginf=0.0)) + np.maximum(np.abs(np.nan_to_num(p_tx, neginf=0.0)),
                                                                                         np.abs(np.nan_to_num(p_rx, neginf=0.0)))
    per_path = c * e_tx * e_rx * (2 * 2 * np.pi * 2.0 ** -24 + 2.0 ** -24 * both * np.log(10.0) / 20.0)
    tol = TOL_REL * np.abs(ref).max(axis=(2, 3)) + np.where(c > 0, per_path, 0.0).sum(axis=2).T
    ds = _dataset(rays, _PLAIN)
    views = {"precoder first": ds.with_tx_precoder(F, beams, p).with_rx_combiner(W),
             "combiner first": ds.with_rx_combiner(W, p).with_tx_precoder(F, np.tile(beams, Q))}
    for what, view in views.items():
        assert view.n_ue == Q * n and view.n_rx_beams == Q
        H = view.compute_channels()
        assert H.shape == (Q * n, 1, 1, 64)
        assert R.worst_ratio(H.reshape(Q, n, 1, 64), ref, tol, what=what) <= 1.0
    assert (tol > 0).sum() >= Q * 4
