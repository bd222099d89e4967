"""The device loader (deepmimo_amd/csrc/mat5_loader.hip, deepmimo_amd/matio.py) on every stored type and tile edge.

Three layers, each against the layer below and against the NumPy statement `ref_rowmajor` (tests/_mat5_cases.py):
the layout kernel through dmx_mat_to_rowmajor_f32 on payload tensors, over the type x shape table, the output inside a
sentinel-filled buffer; the reader pipeline dmx_mats_to_device over raw binary files, at payload sizes that give one
slice, a one-byte last slice and ten slices, with every thread count and unaligned file and staging offsets; and
matio / dm.load(device='cuda') over a scenario whose files the tests' own MAT writer made with mixed storage.

Comparison is by bits (float32 viewed as int32), except that a NaN converted from a stored double is compared as NaN.
"""
import ctypes as C
import json

import numpy as np
import pytest

from tests import _mat5_cases as m5
from tests._mat5_cases import (MI_DOUBLE, MI_NAMES, PIPELINE_FILE_OFFSETS, PIPELINE_PAYLOADS, PIPELINE_THREADS, STORED_TYPES,
                               case_values, kernel_cases, ref_rowmajor, selection)

pytestmark = pytest.mark.gpu

GUARD = 96                                                      # float32 words of sentinel on either side of an output
SENTINEL = -777.25


def _lib():
    from deepmimo_amd import _native as nat
    return nat.load()


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guarded(n):
    """(whole buffer, the n words in its middle)"""
    import torch
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD: GUARD + n]


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to("cuda")   # a copy: payload views of bytes are read-only


def _payload_dev(payload: bytes):
    return _to_dev(np.frombuffer(payload, dtype=np.uint8)) if payload else None


def _check_guards(buf, n, what):
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == np.float32(SENTINEL)), f"{what}: wrote in front of the output"
    assert np.all(host[GUARD + n:] == np.float32(SENTINEL)), f"{what}: wrote behind the output"
    return host[GUARD: GUARD + n]


def _assert_same(got, want, mi, what):
    """Bits; for a stored double the NaNs as NaN (their sign and payload are the converter's business)"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    if mi == MI_DOUBLE:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions"
        got, want = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} of {want.size} differ, first at {tuple(int(b[0]) for b in bad)}: "
                              f"got {got[bad][0]!r} want {want[bad][0]!r}")


def _launch_kernel(lib, d_payload, mi, rows, cols, d_idx, n_sel, keep):
    """dmx_mat_to_rowmajor_f32 into a guarded buffer; returns the buffer (not synchronised)"""
    from deepmimo_amd import _native as nat
    buf, out = _guarded(n_sel * keep)
    rc = lib.dmx_mat_to_rowmajor_f32(_ptr(d_payload), mi, rows, cols, _ptr(d_idx), n_sel, keep, _ptr(out), _stream_ptr())
    nat.check(rc, "dmx_mat_to_rowmajor_f32")
    return buf


@pytest.mark.parametrize("mi", STORED_TYPES, ids=[MI_NAMES[t] for t in STORED_TYPES])
def test_layout_kernel_on_the_type_and_shape_table(mi):
    import torch
    lib = _lib()
    cases = [c[1:] for c in kernel_cases() if c[0] == mi]
    payloads, runs = {}, []
    for rows, cols, keep, kind in cases:
        if (rows, cols) not in payloads:
            raw = case_values(mi, rows, cols).tobytes(order="F")
            payloads[rows, cols] = (raw, _payload_dev(raw))
        raw, d_payload = payloads[rows, cols]
        idx, n_sel = selection(kind, rows)
        d_idx = None if idx is None else _to_dev(idx)
        runs.append((rows, cols, keep, kind, idx, n_sel, d_idx, _launch_kernel(lib, d_payload, mi, rows, cols, d_idx, n_sel, keep)))
    torch.cuda.synchronize()
    compared = 0
    for rows, cols, keep, kind, idx, n_sel, _, buf in runs:
        what = f"{MI_NAMES[mi]} {rows}x{cols} keep {keep} {kind}"
        got = _check_guards(buf, n_sel * keep, what).reshape(n_sel, keep)
        _assert_same(got, ref_rowmajor(payloads[rows, cols][0], mi, rows, cols, idx, n_sel, keep), mi, what)
        compared += 1
    print(f"layout kernel, {MI_NAMES[mi]}: {compared} cases compared bit for bit")
    assert compared == len(cases) >= 6


def test_layout_kernel_empty_outputs_write_nothing():
    """n_sel == 0 and cols_keep == 0 return OK without a launch, with and without an index list"""
    import torch
    lib = _lib()
    raw = case_values(m5.MI_INT16, 33, 5).tobytes(order="F")
    d_payload, d_idx = _payload_dev(raw), _to_dev(np.array([4, 0, 32], dtype=np.int64))
    buf, out = _guarded(64)
    for idx, n_sel, keep in ((None, 0, 5), (d_idx, 0, 5), (None, 33, 0), (d_idx, 3, 0), (None, 0, 0)):
        assert lib.dmx_mat_to_rowmajor_f32(_ptr(d_payload), m5.MI_INT16, 33, 5, _ptr(idx), n_sel, keep, _ptr(out), _stream_ptr()) == 0
        assert lib.dmx_mat_to_rowmajor_f32(None, m5.MI_INT16, 33, 5, _ptr(idx), n_sel, keep, None, _stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.all(buf == SENTINEL)
    assert lib.dmx_mat_to_rowmajor_f32(_ptr(d_payload), m5.MI_INT16, 33, 5, None, 34, 5, _ptr(out), _stream_ptr()) != 0   # n_sel > rows
    assert lib.dmx_mat_to_rowmajor_f32(_ptr(d_payload), m5.MI_INT16, 33, 5, None, 3, 6, _ptr(out), _stream_ptr()) != 0    # keep > cols


# ---- pipeline -------------------------------------------------------------------------------------------------------

def _pinned(nbytes):
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)           # as matio._staging makes it


def _junk(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _pipeline(lib, specs, stage, d_idx, n_idx, n_threads):
    """One dmx_mats_to_device call.  specs: dicts with mi, rows, cols, keep, raw, path (None: staged here), file_offset,
    stage_offset.  Returns the guarded output buffers after the stream has been synchronised."""
    import torch
    from deepmimo_amd import _native as nat
    stage.fill_(0xA5)
    stage_np = stage.numpy()
    jobs = (nat.DmxMatJob * len(specs))()
    bufs, keepalive = [], []
    for j, s in zip(jobs, specs):
        nbytes = len(s["raw"])
        n_sel = s["rows"] if d_idx is None else n_idx
        d_payload = torch.full((max(nbytes, 1),), 0x5A, dtype=torch.uint8, device="cuda")
        buf, out = _guarded(n_sel * s["keep"])
        if s["path"] is None and nbytes:
            stage_np[s["stage_offset"]: s["stage_offset"] + nbytes] = np.frombuffer(s["raw"], dtype=np.uint8)
        j.path = None if s["path"] is None else str(s["path"]).encode()
        j.file_offset, j.nbytes, j.stage_offset = s["file_offset"], nbytes, s["stage_offset"]
        j.d_payload, j.d_out = d_payload.data_ptr(), out.data_ptr()
        j.data_type, j.cols_keep, j.rows, j.cols = s["mi"], s["keep"], s["rows"], s["cols"]
        keepalive.append(d_payload)
        bufs.append(buf)
    rc = lib.dmx_mats_to_device(jobs, len(specs), _ptr(stage), _ptr(d_idx), 0 if d_idx is None else n_idx, n_threads, _stream_ptr())
    torch.cuda.synchronize()
    nat.check(rc, "dmx_mats_to_device")
    return bufs


def _alone(lib, s, idx, d_idx):
    """The same job through dmx_mat_to_rowmajor_f32 on a payload torch uploaded, and ref_rowmajor: (kernel, reference)"""
    import torch
    n_sel = s["rows"] if idx is None else idx.size
    buf = _launch_kernel(lib, _payload_dev(s["raw"]), s["mi"], s["rows"], s["cols"], d_idx, n_sel, s["keep"])
    torch.cuda.synchronize()
    got = _check_guards(buf, n_sel * s["keep"], "alone").reshape(n_sel, s["keep"])
    return got, ref_rowmajor(s["raw"], s["mi"], s["rows"], s["cols"], idx, n_sel, s["keep"])


def _pipeline_selection(rows):
    """Descending stride 3 with a few duplicates in front"""
    return np.concatenate([np.array([rows - 1, 0, rows - 1, rows // 2], dtype=np.int64), np.arange(rows - 1, -1, -3, dtype=np.int64)])


def test_pipeline_slices_threads_and_offsets(tmp_path):
    """One job per call: 65,536 bytes (one slice), 65,537 bytes (a one-byte second slice), 614,528 bytes (ten slices at 32
    threads) x n_threads 0 / 1 / 2 / 3 / 32 / 100 x file offsets 0 / 3 / 184, staged at an offset that is no multiple of
    256, with and without an index list"""
    lib = _lib()
    stage = _pinned(1 << 20)
    compared = 0
    for p, (mi, rows, cols) in enumerate(PIPELINE_PAYLOADS):
        raw = case_values(mi, rows, cols).tobytes(order="F")
        keep = cols if p != 2 else 10
        idx = _pipeline_selection(rows)
        d_idx = _to_dev(idx)
        base = dict(mi=mi, rows=rows, cols=cols, keep=keep, raw=raw)
        want = {False: _alone(lib, base, None, None), True: _alone(lib, base, idx, d_idx)}
        for use_idx in (False, True):
            _assert_same(want[use_idx][0], want[use_idx][1], mi, f"payload {p} alone, index list {use_idx}")
        paths = {}
        for off in PIPELINE_FILE_OFFSETS:
            paths[off] = tmp_path / f"payload{p}_at{off}.bin"
            paths[off].write_bytes(_junk(off, 10 + off) + raw + _junk(777, 5))
        for t, n_threads in enumerate(PIPELINE_THREADS):
            for off in PIPELINE_FILE_OFFSETS:
                spec = dict(base, path=paths[off], file_offset=off, stage_offset=1001 + 3 * t)
                for use_idx in (False, True):
                    what = f"{MI_NAMES[mi]} {len(raw)} bytes, {n_threads} threads, file offset {off}, index list {use_idx}"
                    buf, = _pipeline(lib, [spec], stage, d_idx if use_idx else None, idx.size, n_threads)
                    n_sel = idx.size if use_idx else rows
                    got = _check_guards(buf, n_sel * keep, what).reshape(n_sel, keep)
                    _assert_same(got, want[use_idx][0], mi, what + " against the kernel alone")
                    _assert_same(got, want[use_idx][1], mi, what + " against the reference")
                    compared += 1
    print(f"pipeline, one job per call: {compared} results compared bit for bit")
    assert compared == 3 * 6 * 3 * 2


def test_pipeline_five_unequal_jobs_in_one_call(tmp_path):
    """Different types and sizes, one job staged by the caller (path = NULL) and one job of zero bytes, in one call.
    Without an index list the zero-byte job is a matrix of zero rows.  With one, every index must lie inside every job's
    rows (matio checks that before the call), so the zero-byte job there is a matrix of zero columns."""
    lib = _lib()
    stage = _pinned(1 << 20)
    shapes = [(MI_DOUBLE, 129, 33, 31, 184), (m5.MI_UINT32, 64, 3, 2, None),                  # (type, rows, cols, keep, file offset)
              (m5.MI_SINGLE, 4801, 32, 10, 0), (m5.MI_UINT8, 65537, 1, 1, 3)]
    idx = np.array([63, 0, 31, 32, 63, 5] + list(range(62, -1, -3)), dtype=np.int64)      # inside the smallest job's 64 rows
    d_idx = _to_dev(idx)
    compared = 0
    for use_idx, zero in ((False, (m5.MI_INT64, 0, 4, 4, None)), (True, (m5.MI_INT64, 70, 0, 0, 3))):
        specs, at = [], 13
        for n, (mi, rows, cols, keep, off) in enumerate(shapes[:2] + [zero] + shapes[2:]):        # five jobs
            raw = case_values(mi, rows, cols).tobytes(order="F")
            path = None
            if off is not None:
                path = tmp_path / f"job{n}_{int(use_idx)}.bin"
                path.write_bytes(_junk(off, 20 + n) + raw + _junk(100, 6))
            specs.append(dict(mi=mi, rows=rows, cols=cols, keep=keep, raw=raw, path=path, file_offset=off or 0, stage_offset=at))
            at += len(raw) + 5
        assert at < stage.numel() and sorted({len(s["raw"]) for s in specs})[0] == 0 and len({len(s["raw"]) for s in specs}) == 5
        for n_threads in (3, 32):
            bufs = _pipeline(lib, specs, stage, d_idx if use_idx else None, idx.size, n_threads)
            for n, (s, buf) in enumerate(zip(specs, bufs)):
                what = f"job {n} ({MI_NAMES[s['mi']]} {s['rows']}x{s['cols']}), {n_threads} threads, index list {use_idx}"
                n_sel = idx.size if use_idx else s["rows"]
                got = _check_guards(buf, n_sel * s["keep"], what).reshape(n_sel, s["keep"])
                alone, ref = _alone(lib, s, idx if use_idx else None, d_idx if use_idx else None)
                _assert_same(got, alone, s["mi"], what + " against the kernel alone")
                _assert_same(got, ref, s["mi"], what + " against the reference")
                compared += 1
    print(f"pipeline, five jobs per call: {compared} results compared bit for bit")
    assert compared == 2 * 2 * 5


# ---- matio and dm.load ------------------------------------------------------------------------------------------------

N_RX, N_COLS = 70, 40


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    """A scenario folder whose ray files hold: class double stored as int16; class double stored as uint8, compressed;
    single; double; single behind two other variables; the rest single or double, compressed or not"""
    import deepmimo_amd as dm
    from oracle import oracle_np as onp
    rays = onp.synth_rays(N_RX, N_COLS, seed=33, all_valid=True)
    rays["aoa_az"] = np.round(rays["aoa_az"])                                  # integer-valued, as MATLAB stores in int16
    rays["phase"][5:, 30:] = np.nan
    rays["delay"] = rays["delay"].astype(np.float64) * (1 + 2.0 ** -30)        # doubles that float32 has to round
    storage = {"aoa_az": (m5.MI_INT16, m5.MX_DOUBLE, False), "inter": (m5.MI_UINT8, m5.MX_DOUBLE, True),
               "phase": (m5.MI_SINGLE, None, False), "delay": (MI_DOUBLE, None, False), "power": (m5.MI_SINGLE, None, False),
               "aoa_el": (m5.MI_SINGLE, None, True), "aod_az": (MI_DOUBLE, None, True), "aod_el": (MI_DOUBLE, m5.MX_SINGLE, False),
               "rx_pos": (m5.MI_SINGLE, None, False), "tx_pos": (MI_DOUBLE, None, True)}
    folder = tmp_path_factory.mktemp("scen")
    params = {"rt_params": {"frequency": 3.5e9}, "scene": {"num_scenes": 1}, "materials": {},
              "txrx_sets": {"txrx_set_0": {"id": 0, "is_tx": True, "is_rx": False, "num_points": 1, "name": "bs"},
                            "txrx_set_1": {"id": 1, "is_tx": False, "is_rx": True, "num_points": N_RX, "name": "ue"}}}
    (folder / "params.json").write_text(json.dumps(params))
    for k, v in rays.items():
        mi, mx, comp = storage[k]
        lead = [m5.numeric_element("note", np.arange(6).reshape(2, 3), m5.MI_INT32), m5.char_element("who", "set 1")] if k == "power" else []
        (folder / dm.core.get_mat_filename(k, 0, 0, 1)).write_bytes(m5.write_mat(k, v, mi, mx, comp, leading=lead))
    return folder, rays


SELECTIONS = {"strided": np.arange(N_RX - 1, -1, -3)[::-1].copy(), "reversed": np.arange(N_RX - 1, -1, -1),
              "duplicated": np.array([3, 3, 69, 0, 3, 69, 41, 41] * 5)}


@pytest.mark.parametrize("max_paths", [33, N_COLS, 50], ids=["below", "equal", "above"])
@pytest.mark.parametrize("sel", list(SELECTIONS), ids=list(SELECTIONS))
def test_device_load_of_mixed_storage_matches_the_host_load(scenario, sel, max_paths):
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd import matio
    folder, rays = scenario
    idx = SELECTIONS[sel]
    host = dm.load(str(folder), max_paths=max_paths, rx_sets={1: idx})
    devd = dm.load(str(folder), max_paths=max_paths, rx_sets={1: idx}, device="cuda")
    cap = matio.STAGING_CAP_BYTES
    try:
        matio.STAGING_CAP_BYTES = 1                                            # every file a pipeline run of its own
        dev1 = dm.load(str(folder), max_paths=max_paths, rx_sets={1: idx}, device="cuda")
    finally:
        matio.STAGING_CAP_BYTES = cap
    keep = min(max_paths, N_COLS)
    for k in dm.consts.RAY_FIELDS:
        assert isinstance(devd[k], torch.Tensor) and devd[k].is_cuda and devd[k].dtype == torch.float32
        got = devd[k].cpu().numpy()
        with np.errstate(all="ignore"):
            want = np.asarray(host[k]).astype(np.float32)
            written = rays[k][idx][:, :keep].astype(np.float32)
        assert got.shape == (idx.size, keep)
        assert np.array_equal(got, want, equal_nan=True), f"{k}: device load differs from the host load"
        assert np.array_equal(got, written, equal_nan=True), f"{k}: device load differs from what was written"
        assert torch.equal(dev1[k].view(torch.int32), devd[k].view(torch.int32)), f"{k}: file-by-file load differs"
    assert np.isnan(devd["phase"].cpu().numpy()).sum() == np.isnan(rays["phase"][idx][:, :keep]).sum() > 0
    np.testing.assert_array_equal(np.asarray(devd.rx_pos), np.asarray(host.rx_pos))
    np.testing.assert_array_equal(np.asarray(devd.rx_pos), rays["rx_pos"][idx])


def _items(folder):
    import deepmimo_amd as dm
    return [(str(folder / dm.core.get_mat_filename(k, 0, 0, 1)), k) for k in dm.consts.RAY_FIELDS]


@pytest.mark.parametrize("max_paths", [10, None, 50])
def test_empty_integer_selection_gives_empty_tensors(scenario, max_paths):
    """m[rx_idxs][:, :max_paths] of the host path is an empty matrix; an empty index tensor has a null pointer, which
    dmx_mats_to_device reads as 'every row'"""
    import torch
    import deepmimo_amd as dm
    from deepmimo_amd import matio
    folder, _ = scenario
    keep = N_COLS if max_paths is None else min(max_paths, N_COLS)
    for empty in (np.array([], dtype=np.int64), np.zeros((0,), dtype=np.int32), []):
        out = matio.load_matrices_to_device(_items(folder), "cuda", rx_idxs=empty, max_paths=max_paths)
        assert set(out) == {k for _, k in _items(folder)}
        for k, t in out.items():
            assert t.shape == (0, keep) and t.dtype == torch.float32 and t.is_cuda, k
    one = matio.load_matrix_to_device(*_items(folder)[0], "cuda", rx_idxs=np.array([], dtype=np.int64), max_paths=max_paths)
    assert one.shape == (0, keep)
    if max_paths is not None:                                                  # and through dm.load, as on the host
        none = np.array([], dtype=np.int64)
        host = dm.load(str(folder), max_paths=max_paths, rx_sets={1: none})
        devd = dm.load(str(folder), max_paths=max_paths, rx_sets={1: none}, device="cuda")
        for k in dm.consts.RAY_FIELDS:
            assert isinstance(devd[k], torch.Tensor) and devd[k].is_cuda and tuple(devd[k].shape) == np.asarray(host[k]).shape == (0, keep)
        assert np.asarray(devd.rx_pos).shape == np.asarray(host.rx_pos).shape == (0, 3)
    # no selection at all still means every row
    full = matio.load_matrix_to_device(*_items(folder)[0], "cuda", rx_idxs=None, max_paths=max_paths)
    assert full.shape == (N_RX, keep)


def test_bad_requests_raise_before_any_launch(scenario, tmp_path):
    import torch
    from deepmimo_amd import matio
    folder, _ = scenario
    torch.cuda.synchronize()
    for bad in ([0, N_RX], [-1, 2], np.array([N_RX + 5])):
        with pytest.raises(IndexError, match="out of range"):
            matio.load_matrices_to_device(_items(folder), "cuda", rx_idxs=bad, max_paths=10)
    path = tmp_path / "cube.mat"
    path.write_bytes(m5.write_mat("inter_pos", np.zeros((4, 3, 2), dtype=np.float32), m5.MI_SINGLE))
    with pytest.raises(ValueError, match="3 dimensions"):
        matio.load_matrix_to_device(str(path), "inter_pos", "cuda")
    with pytest.raises(ValueError, match="GPU device"):
        matio.load_matrices_to_device(_items(folder), "cpu")
    torch.cuda.synchronize()


def test_two_loading_threads_take_turns_at_the_staging_buffer(tmp_path, monkeypatch):
    """The page-locked staging buffer is one per process and dmx_mats_to_device runs with the GIL released: matio holds a
    lock from `_staging` until the stream has drained.  The first thread, once it has the buffer, gives the second 0.2 s to
    enter `_staging`: with the lock it cannot, it waits in front of it until the first load is complete."""
    import threading
    import torch
    from deepmimo_amd import matio
    rng = np.random.default_rng(77)
    groups = {"first": ("power", rng.uniform(-140, -60, (50, 10)).astype(np.float32), m5.MI_SINGLE),
              "second": ("delay", rng.uniform(1e-8, 2e-6, (64, 12)), MI_DOUBLE)}
    items = {}
    for who, (key, values, mi) in groups.items():
        path = tmp_path / f"{who}.mat"
        path.write_bytes(m5.write_mat(key, values, mi))
        items[who] = [(str(path), key)]
    torch.cuda.synchronize()
    real = matio._staging
    first_has_buffer, second_started, second_entered = threading.Event(), threading.Event(), threading.Event()
    seen, results, errors = {}, {}, []

    def staging(nbytes):
        who = threading.current_thread().name
        if who == "second":
            second_entered.set()
        buf = real(nbytes)
        if who == "first":
            first_has_buffer.set()
            seen["entered_while_first_held_the_buffer"] = second_entered.wait(0.2)
            seen["second_had_started"] = second_started.is_set()
        return buf

    def load(who):
        try:
            if who == "second":
                assert first_has_buffer.wait(30)
                second_started.set()
            results[who] = matio.load_matrices_to_device(items[who], "cuda")
        except BaseException as e:                                             # noqa: BLE001 - reported by the main thread
            errors.append((who, repr(e)))
            first_has_buffer.set()

    monkeypatch.setattr(matio, "_staging", staging)
    threads = [threading.Thread(target=load, args=(who,), name=who) for who in ("first", "second")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and not any(t.is_alive() for t in threads), errors
    assert seen == {"entered_while_first_held_the_buffer": False, "second_had_started": True}, seen
    assert second_entered.is_set()                                             # it did get its turn afterwards
    torch.cuda.synchronize()
    for who, (key, values, mi) in groups.items():
        host = matio.read_matrix_host(items[who][0][0], key)
        assert np.array_equal(host, values)
        _assert_same(results[who][key].cpu().numpy(), host.astype(np.float32), mi, f"{who} thread, {key}")
