"""CPU guard of tests/test_gpu_persistent_loops.py: every `__global__` kernel of deepmimo_amd/csrc/*.hip whose
workgroups or waves loop over work items (a gridDim-strided loop) is named by at least one route of
tests/_persistent_routes.py, so that a new persistent kernel cannot land without a parity test past its first item.
Also checks the route table itself: each launch names a kernel that exists and is persistent, and each route keeps
at least two grids' worth of items for every one of its launches on a 256-CU MI355X."""
import glob
import os
import re

from tests import _persistent_routes as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimo_amd", "csrc")


def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def kernels_with_strided_loops(sources):
    """{kernel name: file} for every __global__ function whose body reads gridDim (the only use of it in this library
    is the stride of a persistent loop)"""
    found = {}
    for path, text in sources:
        src = _strip_comments(text)
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src):
            i = src.index("{", m.end())
            depth, j = 0, i
            while True:
                if src[j] == "{":
                    depth += 1
                elif src[j] == "}":
                    depth -= 1
                    if depth == 0:
                        break
                j += 1
            body = src[i:j]
            if re.search(r"\bgridDim\b", body):
                found[m.group(1)] = os.path.basename(path)
    return found


def _sources():
    out = []
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(p) as f:
            out.append((p, f.read()))
    return out


def _routed():
    return {ln.kernel for r in R.ROUTES for ln in r.launches}


def test_every_persistent_kernel_has_a_route():
    found = kernels_with_strided_loops(_sources())
    assert len(found) >= 7, found                   # the scan itself works (seven such kernels; the set is pinned below)
    missing = sorted(k for k in found if k not in _routed())
    assert not missing, f"persistent kernels without a route in tests/_persistent_routes.py: {missing}"
    assert set(found) == set(R.PERSISTENT_KERNELS), (sorted(found), R.PERSISTENT_KERNELS)


def test_routes_name_existing_persistent_kernels():
    found = kernels_with_strided_loops(_sources())
    for name in _routed():
        assert name in found, f"route names {name}, which is not a persistent kernel of deepmimo_amd/csrc"


def test_scanner_on_a_known_source():
    src = """
    template <int NW> __global__ __launch_bounds__(256) void k_loop(int n) {
        for (int i = blockIdx.x; i < n; i += gridDim.x) { if (i) { } }
    }
    __global__ void k_flat(int n) { /* gridDim */ int i = blockIdx.x; // gridDim.x
    }
    __device__ void helper() { int g = gridDim.x; }
    """
    assert kernels_with_strided_loops([("x.hip", src)]) == {"k_loop": "x.hip"}


def test_every_route_loops_on_256_cus():
    for r in R.ROUTES:
        for ln in r.launches:
            items = r.U * R.items_per_user(r, ln)
            assert items >= 2 * R.slot_bound(r, ln, 256), (r.name, ln.kernel)
