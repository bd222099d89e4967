"""Every kept-path count and every K-step tail kind on each frequency-domain kernel, against the NumPy oracle in float64.

The inputs are those of tests/_path_count_cases.py: the ladder (user u keeps u paths, all within 6 dB) and the weak-tail
cases of the opt-in one-term rule.  tests/test_path_counts_cpu.py holds the condition that makes the bounds below mean
something: on these inputs a dropped path, two paths in each other's slots or a coefficient without its lo term moves the
reference by at least twice the bound.  The bounds are the project's own: 3e-6 of a user's peak for the matrix-core and
folded kernels in default mode, 1e-5 with DMX_FLAG_ADAPTIVE_TERMS (`lim` of test_precision_flag_parity), 1e-5 for the beam
amplitudes, TOL_REL everywhere else.  LoS and path counts bit-exact; a user without paths exactly zero.
"""
import os

import numpy as np
import pytest

from tests import _path_count_cases as P
from tests._cases import TOL_ABS, TOL_REL, channel_err

pytestmark = pytest.mark.gpu

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "lib", "libdeepmimo_amd.so")
if not os.path.exists(_LIB):
    pytest.skip("needs the built library", allow_module_level=True)

from tests.test_gpu_covariance import check_covariance  # noqa: E402
from tests.test_gpu_parity import _dm_params, check_beam_channels, check_beam_power  # noqa: E402
from tests.test_gpu_rate import check_rate  # noqa: E402
from tests._rate_ref import median_snr  # noqa: E402

WORST = {}                                   # what -> worst error / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module: the worst error / bound per form over what ran (BASELINE.md quotes them; every figure was asserted
    where it was measured)"""
    yield
    groups = {}
    for what, r in WORST.items():
        key = " ".join(what.split(" ")[:2]) if what.startswith("rx_filter") else what.split(" ")[0]
        groups[key] = max(groups.get(key, 0.0), r)
    for key in sorted(groups):
        print(f"path counts: {key}: worst error / bound {groups[key]:.3f}")


RUNS = list(P.LADDER_RUNS)

# form -> (shape of tests/_path_count_cases.py FD_SHAPES, fd_kernel_variant or "direct" for the single pass)
FORMS = {
    "v1_valu": ("valu", 1), "v2_mfma": ("mfma", 2), "v2_mfma_sincos": ("mfma_sincos", 2), "v4_mfma": ("mfma", 4),
    "v5_mfma": ("mfma", 5), "v10_mfma": ("mfma", 10),
    "v9_small": ("small", 9), "v12_wave": ("fold_wave", 12), "v12_wave_K100": ("fold_wave_K100", 12),
    "v12_shared": ("fold_shared", 12), "single_pass": ("small", "direct"),
}


def _engine():
    from deepmimo_amd.engine import ChannelEngine
    return ChannelEngine(0)


def _params(case, n):
    return _dm_params(case, np.zeros(3)).validate(n)


def _hold(H, Href, bound, what, dead=None):
    """max|dH| <= bound * max|Href[u]| per user (plus TOL_ABS where the bound is TOL_REL, as tests/_cases.py has it);
    users in `dead` exactly zero.  Prints and records the worst error / bound."""
    H = np.asarray(H)
    assert H.shape == Href.shape and H.dtype == Href.dtype, (what, H.shape, Href.shape)
    assert np.isfinite(H.astype(np.complex128)).all(), f"{what}: NaN or inf"
    d, peak = channel_err(H, Href)
    if dead is not None:
        assert np.all(peak[dead] == 0) and np.all(peak[~dead] > 0)
        assert np.all(np.abs(H[dead]) == 0), f"{what}: a user without paths is not exactly zero"
    lim = bound * peak + (TOL_ABS if bound == TOL_REL else 0.0)
    live = peak > 0
    ratio = d[live] / lim[live]
    u = int(np.flatnonzero(live)[np.argmax(ratio)])
    print(f"{what}: worst error / peak {d[u] / peak[u]:.3e} (user {u}), bound {bound:.1e}, ratio {ratio.max():.3f}")
    WORST[what] = float(ratio.max())
    assert np.all(d <= lim), f"{what}: {(d > lim).sum()} users out of bound, worst user {u} at {d[u] / peak[u]:.3e} of its peak (bound {bound:.1e})"


def _side_exact(side, ref, what):
    np.testing.assert_array_equal(side["los"].cpu().numpy(), ref["los"], err_msg=what)
    np.testing.assert_array_equal(side["num_paths"].cpu().numpy(), ref["num_paths"], err_msg=what)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("form", list(FORMS))
def test_fd_contraction_on_the_ladder(form, run):
    shape, variant = FORMS[form]
    case, rays, kept, ref = P.ladder_reference(shape, run)
    n = len(kept)
    bound = P.FD_SHAPES[shape][3] or TOL_REL
    eng = _engine()
    dr = eng.upload_rays(rays)
    p = _params(case, n)
    if variant == "direct":
        assert eng.direct_supported(dr, p), "the single pass does not take this shape"
        H, side = eng.channels_direct(dr, p, want_side="light")
    else:
        prep = eng.prepare(dr, p, want_side="light")
        H, side = eng.channels(prep, variant=variant), prep.side
    _hold(H.cpu().numpy(), ref["channel"], bound, f"{form} {run}", dead=kept == 0)
    _side_exact(side, ref, f"{form} {run}")


@pytest.mark.parametrize("codebook", ["steering", "random"])
@pytest.mark.parametrize("run", RUNS)
def test_beam_consumers_on_the_ladder(run, codebook):
    """compute_beam_channels and compute_beam_power (k2c_beam_power loops to n_keep) with the suite's own checks"""
    import deepmimo_amd as dm
    case, rays, kept, ref = P.ladder_reference("beam", run)
    p = _dm_params(case, np.zeros(3))
    F = P.codebooks(case["bs_shape"])[codebook]
    Href = ref["channel"].astype(np.complex128)
    ds = dm.Dataset({k: v.copy() for k, v in rays.items()})
    Y = check_beam_channels(ds, p, F, Href)
    assert np.all(Y[kept == 0] == 0)
    ds = check_beam_power({k: v.copy() for k, v in rays.items()}, p, F, Href, ref["los"], part=(7, 20))
    amp = ds["beam_mean_amplitude"]
    want = np.abs(F @ Href).mean(axis=1).mean(axis=-1)
    live = kept > 0
    ratio = (np.abs(amp - want)[live] / (P.BOUND_BEAM_POWER * want[live].max(axis=1, keepdims=True))).max()
    print(f"beam power {run} {codebook}: worst amplitude error / bound {ratio:.3f}")
    WORST[f"beam_power {run} {codebook}"] = float(ratio)
    assert ratio <= 1.0 and np.all(amp[~live] == 0)
    np.testing.assert_array_equal(ds.num_paths, ref["num_paths"])


@pytest.mark.parametrize("run", RUNS)
def test_covariance_and_rate_on_the_ladder(run):
    """k6_covariance and k7_rate loop to n_keep: both sides of the covariance and the rate, with the helpers and the
    tolerances of their own tests, against the oracle's channel of the ladder"""
    import torch
    case, rays, kept, ref = P.ladder_reference("consumers", run)
    eng = _engine()
    prep = eng.prepare(eng.upload_rays(rays), _params(case, len(kept)), want_side="light")
    assert eng.covariance_supported(prep, "tx") and eng.covariance_supported(prep, "rx") and eng.rate_supported(prep)
    H = ref["channel"]
    R = [eng.covariance(prep, side=s) for s in ("tx", "rx")]
    snr = median_snr(H)
    snr_db = 10 * np.log10(snr)
    rate, rate_k = eng.rate(prep, snr_db, per_subcarrier=True)
    torch.cuda.synchronize()
    WORST[f"covariance {run}"] = check_covariance(R[0], R[1], H, f"ladder {run}") / TOL_REL
    WORST[f"rate {run}"] = check_rate(rate, rate_k, H, 10.0 ** (snr_db / 10.0), f"ladder {run}")
    _side_exact(prep.side, ref, run)


@pytest.mark.parametrize("doppler", [0, 1])
@pytest.mark.parametrize("arrays", list(P.LPF_ARRAYS))
@pytest.mark.parametrize("N", P.LPF_N)
def test_rx_filter_on_the_ladder(N, arrays, doppler):
    """rx_filter = 1 (k3_lpf_fft*: 8, 4 or 2 paths per wave): 0 ... 25 kept paths at every OFDM size class"""
    case, rays, kept, ref = P.lpf_reference(arrays, N, bool(doppler))
    eng = _engine()
    p = _dm_params(case, np.zeros(3))
    p.enable_doppler = doppler
    p = p.validate(len(kept))
    prep = eng.prepare(eng.upload_rays(rays), p, want_side="light", carrier_freq=P.FC)
    assert prep.params_struct.rx_filter == 1 and prep.params_struct.enable_doppler == doppler
    H = eng.channels(prep)
    _hold(H.cpu().numpy(), ref["channel"], TOL_REL, f"rx_filter {arrays} N={N} doppler={doppler}", dead=kept == 0)
    _side_exact(prep.side, ref, f"rx_filter {arrays} N={N}")
    if doppler:
        assert not np.array_equal(ref["channel"], P.lpf_reference(arrays, N, False)[3]["channel"]), "the Doppler term changed nothing"


# ---- the one-term rule: fold tile kinds 4 ... 9 on purpose -------------------------------------------------------------
ADAPTIVE_FORMS = {"v12_wave": ("fold_wave", 12), "v12_shared": ("fold_shared", 12), "v2_mfma": ("mfma", 2), "v2_mfma_sincos": ("mfma_sincos", 2),
                  "beam_power": ("beam", None)}


def _weak_tail_result(eng, form, presorted, adaptive):
    """(result [n, ...] as NumPy, reference of the same form in float64, bound) of a form on the weak-tail batch"""
    shape, variant = ADAPTIVE_FORMS[form]
    case, rays, fires, n_keep, ref = P.weak_tail_reference(shape, presorted)
    prep = eng.prepare(eng.upload_rays(rays), _params(case, len(fires)), want_side="light", adaptive_terms=adaptive)
    assert prep.params_struct.flags == (1 if adaptive else 0)
    np.testing.assert_array_equal(prep.side["num_paths"].cpu().numpy(), n_keep)
    if form == "beam_power":
        F = P.codebooks(case["bs_shape"])["steering"]
        amp = eng.beam_power(prep, F)[0].cpu().numpy()
        want = np.abs(F @ ref["channel"].astype(np.complex128)).mean(axis=1).mean(axis=-1)
        return amp, want, P.BOUND_BEAM_POWER
    return eng.channels(prep, variant=variant).cpu().numpy(), ref["channel"], (P.BOUND_ADAPTIVE if adaptive else P.BOUND_MATRIX_CORE)


def _hold_any(X, want, bound, what):
    if X.ndim == 2:                                                     # beam amplitudes [n, beams]: element-wise, of the strongest beam
        ratio = (np.abs(X - want) / (bound * want.max(axis=1, keepdims=True))).max()
        print(f"{what}: worst amplitude error / bound {ratio:.3f}")
        WORST[what] = float(ratio)
        assert ratio <= 1.0, (what, ratio)
    else:
        _hold(X, want, bound, what)


@pytest.mark.parametrize("form", list(ADAPTIVE_FORMS))
def test_adaptive_tail_kinds(form):
    """Weak last K-steps of 1 and 8 paths behind one, two and three strong K-steps, just under the rule's threshold and
    just over it.  Shuffled rays: the error stays inside the flag's bound (and the default's without it).  Rays already in
    stage 1's order: the flagged result differs in bits from the default one exactly for the users `tail_kind` says the
    rule fires on - which shows it fired, there and nowhere else."""
    eng = _engine()
    for presorted in (False, True):
        for adaptive in (False, True):
            X, want, bound = _weak_tail_result(eng, form, presorted, adaptive)
            _hold_any(X, want, bound, f"{form} weak tail {'sorted' if presorted else 'shuffled'} {'flag' if adaptive else 'default'}")
    rays, fires, n_keep = P.weak_tail_batch(True)
    flagged_kind, default_kind = P.tail_kinds(rays, P.MAX_KEPT, True), P.tail_kinds(rays, P.MAX_KEPT, False)
    expect = flagged_kind != default_kind
    np.testing.assert_array_equal(expect, fires)
    assert set(flagged_kind.tolist()) == {4, 5, 6, 7, 8, 9}
    if form == "v2_mfma":
        # uniformly spaced selection: a last K-step of one or two paths is packed with all three terms in both modes
        # (tests/_path_count_cases.py mfma_flag_changes_bits); v2_mfma_sincos runs the same cases with nothing packed
        amps = P.kept_amplitudes(rays, P.MAX_KEPT)
        expect = np.array([P.mfma_flag_changes_bits(n_keep[u], amps[u], True) for u in range(len(fires))])
    S3 = _weak_tail_result(eng, form, True, False)[0]
    S1 = _weak_tail_result(eng, form, True, True)[0]
    bits = np.uint32 if S1.dtype == np.float32 else np.uint64
    differ = np.array([not np.array_equal(S1[u].view(bits), S3[u].view(bits)) for u in range(len(fires))])
    assert differ[expect].all(), f"{form}: the rule did not fire for users {np.flatnonzero(expect & ~differ).tolist()} (kinds {flagged_kind[expect & ~differ].tolist()})"
    assert not differ[~expect].any(), f"{form}: the flag changed users {np.flatnonzero(~expect & differ).tolist()} the rule does not fire on"
