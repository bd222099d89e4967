"""Inputs of the device-loader tests (tests/test_mat_loader_cpu.py, tests/test_gpu_mat_loader.py): a writer of MATLAB
level-5 MAT files, the NumPy statement of the layout kernel, value sets per stored type and the shape table.

The writer follows the published MAT-File Format description (header, data-element tags, small data elements, miMATRIX
sub-elements, miCOMPRESSED) and nothing else; tests/test_mat_loader_cpu.py ties it to scipy.io.loadmat as an independent
reader.  Unlike scipy.io.savemat it can store an array of one class in another numeric type - MATLAB itself stores
integer-valued doubles in the narrowest integer type - and it can put other variables ahead of the target.

`ref_rowmajor` is what k_mat_to_rowmajor computes: reinterpret the payload, reshape column-major, gather rows, trim
columns, convert to float32 (round to nearest even, as NumPy's astype does; a bit copy for miSINGLE).
"""
from __future__ import annotations

import functools
import struct
import zlib

import numpy as np

# miTYPE of a stored payload -> NumPy dtype (MAT-File Format, table 1-1)
MI_INT8, MI_UINT8, MI_INT16, MI_UINT16, MI_INT32, MI_UINT32, MI_SINGLE, MI_DOUBLE, MI_INT64, MI_UINT64 = 1, 2, 3, 4, 5, 6, 7, 9, 12, 13
MI_MATRIX, MI_COMPRESSED = 14, 15
MI_DTYPES = {MI_INT8: np.int8, MI_UINT8: np.uint8, MI_INT16: np.int16, MI_UINT16: np.uint16, MI_INT32: np.int32,
             MI_UINT32: np.uint32, MI_SINGLE: np.float32, MI_DOUBLE: np.float64, MI_INT64: np.int64, MI_UINT64: np.uint64}
MI_NAMES = {MI_INT8: "int8", MI_UINT8: "uint8", MI_INT16: "int16", MI_UINT16: "uint16", MI_INT32: "int32", MI_UINT32: "uint32",
            MI_SINGLE: "single", MI_DOUBLE: "double", MI_INT64: "int64", MI_UINT64: "uint64"}
STORED_TYPES = tuple(MI_DTYPES)
# mxCLASS of an array -> NumPy dtype (table 1-3), and the class an array of a stored type has when nothing says otherwise
MX_CHAR, MX_DOUBLE, MX_SINGLE = 4, 6, 7
MX_DTYPES = {6: np.float64, 7: np.float32, 8: np.int8, 9: np.uint8, 10: np.int16, 11: np.uint16, 12: np.int32, 13: np.uint32,
             14: np.int64, 15: np.uint64}
MX_OF_MI = {MI_INT8: 8, MI_UINT8: 9, MI_INT16: 10, MI_UINT16: 11, MI_INT32: 12, MI_UINT32: 13, MI_SINGLE: 7, MI_DOUBLE: 6,
            MI_INT64: 14, MI_UINT64: 15}


# ---- writer ---------------------------------------------------------------------------------------------------------

def _element(mi: int, raw: bytes) -> bytes:
    """One data element: 1..4 bytes in the small form (type and size in 16 bits each, data in the tag's second word),
    anything else as an 8-byte tag and the data padded to 8 bytes"""
    n = len(raw)
    if 0 < n <= 4:
        return struct.pack("<HH", mi, n) + raw + bytes(4 - n)
    return struct.pack("<II", mi, n) + raw + bytes(-n % 8)


def _matrix(name: str, mx_class: int, dims, real: bytes) -> bytes:
    body = (_element(MI_UINT32, struct.pack("<II", mx_class, 0))             # array flags: class in the low byte, no flag set
            + _element(MI_INT32, struct.pack(f"<{len(dims)}i", *dims))
            + _element(MI_INT8, name.encode("ascii"))
            + real)
    return struct.pack("<II", MI_MATRIX, len(body)) + body


def numeric_element(name: str, values, mi: int, mx_class: int | None = None, compress: bool = False) -> bytes:
    """The miMATRIX element of one real numeric array of any dimension count: `values` stored as type `mi` (column-major),
    announced as class `mx_class` (default: the class of the stored type); compress: wrapped in miCOMPRESSED"""
    a = np.asarray(values)
    if a.dtype != MI_DTYPES[mi]:
        a = a.astype(MI_DTYPES[mi])
    el = _matrix(name, MX_OF_MI[mi] if mx_class is None else mx_class, a.shape, _element(mi, a.tobytes(order="F")))
    return _compressed(el) if compress else el


def char_element(name: str, text: str) -> bytes:
    """A 1 x n char array (a non-numeric variable), 16-bit code units"""
    return _matrix(name, MX_CHAR, (1, len(text)), _element(MI_UINT16, np.array([ord(ch) for ch in text], dtype=np.uint16).tobytes()))


def _compressed(element: bytes) -> bytes:
    z = zlib.compress(element)
    return struct.pack("<II", MI_COMPRESSED, len(z)) + z                     # compressed elements carry no padding


def mat_file(*elements: bytes) -> bytes:
    """A level-5 MAT-file image: 116 bytes of text, no subsystem offset, version 0x0100, the little-endian mark"""
    text = b"MATLAB 5.0 MAT-file, written by tests/_mat5_cases.py"
    return text + b" " * (116 - len(text)) + bytes(8) + struct.pack("<H", 0x0100) + b"IM" + b"".join(elements)


def write_mat(name: str, values, mi: int, mx_class: int | None = None, compress: bool = False, leading=()) -> bytes:
    """File image with the target array behind the elements of `leading` (numeric_element / char_element results)"""
    return mat_file(*leading, numeric_element(name, values, mi, mx_class, compress))


# ---- the layout kernel, in NumPy ------------------------------------------------------------------------------------

def ref_rowmajor(payload: bytes, data_type: int, rows: int, cols: int, row_idx, n_sel: int, keep: int) -> np.ndarray:
    """float32 [n_sel, keep]: rows row_idx[:n_sel] (None: the first n_sel) and the first `keep` columns of the
    column-major [rows, cols] payload of stored type `data_type`"""
    a = np.frombuffer(payload, dtype=MI_DTYPES[data_type], count=rows * cols).reshape((rows, cols), order="F")
    idx = np.arange(n_sel) if row_idx is None else np.asarray(row_idx, dtype=np.int64)[:n_sel]
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(a[idx][:, :keep]).astype(np.float32)


# ---- values that break a wrong conversion -----------------------------------------------------------------------------

F32_BITS = [0x7fc00000, 0x7fc00001, 0xffc12345, 0x7fe00000, 0xffffffff,     # quiet NaNs, distinct payloads and signs
            0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000,     # -0.0, smallest / largest denormal, +-inf
            0x3f800000, 0x00800000, 0x7f7fffff]                             # 1.0, smallest normal, largest finite
F64_DENORMAL_IN_F32 = 1e-40                                                   # float32: the denormal 71362 * 2^-149


@functools.lru_cache(maxsize=None)
def special_values(mi: int) -> np.ndarray:
    """1-D array of dtype MI_DTYPES[mi]"""
    dt = MI_DTYPES[mi]
    if mi == MI_SINGLE:
        return np.array(F32_BITS, dtype=np.uint32).view(np.float32)
    if mi == MI_DOUBLE:
        return np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50,   # ties to even; just above a tie
                         -(1 + 2.0 ** -24), 1e300, -1e300, 3.4028235677973366e38,           # -> inf (the last: the first such double)
                         F64_DENORMAL_IN_F32, -F64_DENORMAL_IN_F32, 2.0 ** -150, 1e-46,      # denormal; tie to 0; below it
                         2.0 ** -126 * (1 - 2.0 ** -25),                                     # rounds up to the smallest normal
                         -0.0, 0.0, np.inf, -np.inf, np.nan, 5e-324, 1.0], dtype=dt)
    if mi in (MI_INT8, MI_INT16):
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        return np.array([lo, lo + 1, -1, 0, 1, hi, -(hi // 2) - 7], dtype=dt)
    if mi in (MI_UINT8, MI_UINT16):
        hi = np.iinfo(dt).max
        return np.array([0, hi // 2, hi // 2 + 1, hi // 2 + 2, hi - 1, hi], dtype=dt)
    if mi == MI_INT32:
        t = 2 ** 24
        return np.array([t + 1, -(t + 1), t + 3, -(t + 3), -2 ** 31, 2 ** 31 - 1, -1, 0, 2 ** 30 + 64, 2 ** 30 + 192], dtype=dt)
    if mi == MI_UINT32:
        return np.array([2 ** 31, 2 ** 31 + 128, 2 ** 31 + 384, 2 ** 31 + 129, 2 ** 32 - 1, 2 ** 32 - 128, 2 ** 32 - 129,
                         2 ** 24 + 1, 2 ** 24 + 3, 0, 3000000000], dtype=dt)
    # 64-bit integers.  float32 spacing: 2 at 2^24, 2^30 at 2^53, 2^40 at 2^63.  v + 1 behind a tie at 2^53 scale is also a
    # tie of int64 -> float64, so a conversion that goes through double rounds it down twice
    t24, t53 = 2 ** 24, 2 ** 53
    ties = [t24 + 1, t24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, t53 + 2 ** 29, t53 + 3 * 2 ** 29, t53 + 2 ** 29 + 1, t53 + 2 ** 29 - 1,
            t53 + 1, 2 ** 62 + 2 ** 38, 2 ** 62 + 2 ** 38 + 1]
    if mi == MI_INT64:
        return np.array(ties + [-v for v in ties] + [2 ** 63 - 1, -(2 ** 63 - 1), -2 ** 63, 2 ** 63 - 2 ** 38, -1, 0], dtype=dt)
    return np.array(ties + [2 ** 63, 2 ** 63 + 2 ** 39, 2 ** 63 + 2 ** 39 + 1, 2 ** 63 + 3 * 2 ** 39, 2 ** 64 - 1, 2 ** 64 - 2 ** 39,
                            2 ** 64 - 2 ** 39 - 1, 2 ** 63 - 1, 0], dtype=dt)


def case_values(mi: int, rows: int, cols: int, seed: int = 0) -> np.ndarray:
    """[rows, cols] of the stored dtype: two of every three elements (column-major order) walk the special values, the
    third is random over the type's whole range"""
    dt, n = MI_DTYPES[mi], rows * cols
    rng = np.random.default_rng(seed + 1000 * mi + 17 * rows + cols)
    if np.issubdtype(dt, np.integer):
        ii = np.iinfo(dt)
        flat = rng.integers(ii.min, ii.max, size=n, dtype=dt, endpoint=True)
    else:
        flat = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, size=n)).astype(dt)
    sp = special_values(mi)
    i = np.arange(n)
    walk = (i - i // 3) % sp.size
    flat = np.where(i % 3 != 2, sp[walk], flat).astype(dt)
    return flat.reshape((rows, cols), order="F")


# ---- shapes ---------------------------------------------------------------------------------------------------------

ROWS = (1, 31, 32, 33, 65)
COLS = (1, 32, 33, 65)
KEEPS = (1, 31, 32, 33)                                        # and keep = cols
SELECTIONS = ("none_all", "none_head", "identity", "reversed", "repeat40", "dups", "last")
FULL_TABLE_TYPES = (MI_SINGLE, MI_DOUBLE, MI_INT8, MI_UINT16)


def selection(kind: str, rows: int):
    """(row_idx as int64 array or None, n_sel)"""
    if kind == "none_all":
        return None, rows
    if kind == "none_head":
        return None, rows - 1                                   # n_sel < rows without an index list (0 for one row)
    if kind == "identity":
        return np.arange(rows, dtype=np.int64), rows
    if kind == "reversed":
        return np.arange(rows - 1, -1, -1, dtype=np.int64), rows
    if kind == "repeat40":
        return np.full(40, rows // 2, dtype=np.int64), 40
    if kind == "dups":
        n = 2 * rows + 1                                        # more selected rows than stored ones
        return (np.arange(n, dtype=np.int64) * 7 + 3) % rows, n
    if kind == "last":
        return np.array([rows - 1], dtype=np.int64), 1
    raise ValueError(kind)


def _col_keeps():
    return [(c, k) for c in COLS for k in sorted({k for k in KEEPS if k <= c} | {c})]


def _shape_table():
    """Every rows x (cols, keep) with the selection kinds taking turns, then every rows x selection kind with the
    (cols, keep) pairs taking turns"""
    ck = _col_keeps()
    out, t = [], 0
    for r in ROWS:
        for c, k in ck:
            out.append((r, c, k, SELECTIONS[t % len(SELECTIONS)]))
            t += 1
    for r in ROWS:
        for s in SELECTIONS:
            c, k = ck[t % len(ck)]
            out.append((r, c, k, s))
            t += 1
    return list(dict.fromkeys(out))


SHAPE_TABLE = _shape_table()
# one tile edge crossed in each axis, below / at / over a tile, every index-list form once
REDUCED_TABLE = [(33, 33, 33, "reversed"), (65, 65, 33, "dups"), (31, 32, 31, "none_head"), (1, 1, 1, "none_all"),
                 (32, 65, 65, "identity"), (33, 33, 32, "repeat40")]


def kernel_cases():
    """[(mi, rows, cols, keep, selection kind)] of the direct-ABI kernel test"""
    out = []
    for mi in STORED_TYPES:
        out += [(mi,) + s for s in (SHAPE_TABLE if mi in FULL_TABLE_TYPES else REDUCED_TABLE)]
    return out


def tile_class(n: int) -> str:
    """Where a count sits against the 32-wide tile"""
    return "below" if n < 32 else "at" if n == 32 else "over" if n == 33 else "two_plus" if n > 64 else "inside"


# ---- read slices of the pipeline --------------------------------------------------------------------------------------

def slice_plan(nbytes: int, n_threads: int):
    """[(lo, hi)] byte ranges dmx_mats_to_device hands to its reader threads for one payload"""
    n_threads = min(32, max(1, n_threads))
    step = -(-nbytes // n_threads)
    step = -(-step // 4096) * 4096
    step = max(step, 65536)
    return [(lo, min(lo + step, nbytes)) for lo in range(0, nbytes, step)]


# (stored type, rows, cols): 65,536 bytes, 65,537 bytes (a prime), 614,528 bytes
PIPELINE_PAYLOADS = [(MI_INT16, 1024, 32), (MI_UINT8, 65537, 1), (MI_SINGLE, 4801, 32)]
PIPELINE_THREADS = (0, 1, 2, 3, 32, 100)
PIPELINE_FILE_OFFSETS = (0, 3, 184)
