"""Case table of the one-wave-per-user consumers (k6_covariance, k7_rate with its three epilogues, k8_cell_rate,
k9_angle_delay, k10_codebook_rate wideband and per subband) at the shapes the other tables leave out: Gram orders 3, 5, 6
and 7 in both orientations, odd arrays on either side, a first panel dimension that is neither 1 nor the element count,
every kept-path count 0 .. 32, every (M, L) pair of k10.  A plain module: NumPy and the oracle only, no torch, no GPU.

The dictionaries have the form of tests/test_gpu_fd_direct.py `_case` (restated here, as tests/_angle_delay_cases.py does:
this module has to import without the library).  The existing tables import the lists below, the way
tests/test_gpu_spectrum.py adds EXTRA; the criteria stay where they are.

The functions of the first section restate the launch rules of deepmimo_amd/csrc/ in plain Python, so that a case can say
which template instantiation and which slice, tail and store form it reaches; tests/test_consumer_shapes_cpu.py ties each
of them to the source lines it restates and holds the ledger: every instantiation the dispatch switches can launch is
reached by a case of the union of the tables.

* `gram_order`, `rate_slices`, `phase3_two`, `second_pass_two`, `vec16`: launch_rate_epi / launch_cell_rate / k7_rate
* `cb_launch`: launch_cb (k10_codebook_rate.hip);  `ad_launch`: launch_angle_delay (k9_angle_delay.hip)
* `tri_pair`, `tri_pairs`: k6_covariance's walk over an upper triangle
"""
from __future__ import annotations

import numpy as np

CB_ROWS = 32            # rows of the row table per LDS chunk (k10_codebook_rate.hip)
MAX_ORDER = 8           # the consumers are templated on 1 .. 8
MAX_LAYERS = 4          # k10: L = 1 .. 4, L <= M


# ---- the launch rules, restated -----------------------------------------------------------------------------------------
def _prod(shape):
    return int(shape[0]) * int(shape[1])


def gram_order(bs, ue):
    """(m, small_is_rx, small_mh, M_big, big_mh) of launch_rate_epi: the Gram runs over the smaller array, the UE's on a tie"""
    m_tx, m_rx = _prod(bs), _prod(ue)
    rx_small = m_rx <= m_tx
    if rx_small:
        return m_rx, 1, int(ue[0]), m_tx, int(bs[0])
    return m_tx, 0, int(bs[0]), m_rx, int(ue[0])


def rate_slices(K, M_big):
    """(S, log2_S) of launch_rate_epi and, per link, of launch_cell_rate: the largest power of two with K S <= 64, S <= M_big"""
    log2_s = 0
    while K * (2 << log2_s) <= 64 and (2 << log2_s) <= M_big:
        log2_s += 1
    return 1 << log2_s, log2_s


def phase3_two(M_big, S):
    """the values `two = t + S < Mb` takes over every slice sl < S and trip t = sl, sl + 2 S, ... of phase 3"""
    return {t + S < M_big for sl in range(S) for t in range(sl, M_big, 2 * S)}


def second_pass_two(M_big, S):
    """the values `two = t + 1 < Mb` takes over every slice and trip t = 2 sl, 2 sl + 2 S, ... of the precoders' second pass"""
    return {t + 1 < M_big for sl in range(S) for t in range(2 * sl, M_big, 2 * S)}


def vec16(M_big):
    """launch_precoders: the large-side rows take 16-byte stores (the output base is 16-byte aligned in every test)"""
    return M_big % 2 == 0


def slice_class(S, M_big):
    return "S1" if S == 1 else ("full" if S == M_big else "partial")


def cb_launch(K, layers, B=None):
    """dict(kc, kcp, S, cpc) of launch_cb; B: the subband size of the subband form"""
    kc = min(K, 64)
    if B is not None:
        kc = min(min(B, K), kc)
    log2_kcp = 0
    while (1 << log2_kcp) < kc:
        log2_kcp += 1
    return dict(kc=kc, kcp=1 << log2_kcp, S=1 << (6 - log2_kcp), cpc=CB_ROWS // layers)


def ad_launch(n_taps):
    """dict(tc, tcp, S) of launch_angle_delay"""
    tc = min(n_taps, 64)
    log2_tcp = 0
    while (1 << log2_tcp) < tc:
        log2_tcp += 1
    return dict(tc=tc, tcp=1 << log2_tcp, S=64 // (1 << log2_tcp))


def tri_pair(e, n):
    """k6_covariance `tri_pair`: (ok, i, j) of pair number e of an n x n upper triangle"""
    r, c = divmod(e, n + 1)
    if c < n - r:
        return True, r, r + c
    i = n - 1 - r
    return i != r, i, i + (c - (n - r))


def tri_pairs(n):
    """the (i, j) the kernel's loop `for e < ((n + 1) >> 1) * (n + 1)` visits, in order, skipped entries left out"""
    out = []
    for e in range(((n + 1) >> 1) * (n + 1)):
        ok, i, j = tri_pair(e, n)
        if ok:
            out.append((i, j))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _case(cid, n, L, bs, ue, N, sel, **kw):
    """tests/test_gpu_fd_direct.py `_case`, with the `adaptive` key the consumer tables add"""
    d = dict(id=cid, n=n, L=L, bs_shape=bs, ue_shape=ue, subcarriers=N, selected=list(sel), num_paths=kw.pop("num_paths", L),
             bs_rot=[0, 0, 0], ue_rot=[0, 0, 0], bs_pattern="isotropic", ue_pattern="isotropic", bs_fov=None, ue_fov=None,
             bs_spacing=0.5, ue_spacing=0.37, bandwidth=20e6, freq_domain=1, rx_filter=0, doppler=None, all_valid=False,
             max_delay=2e-6, rays="plain", per_user_rot=False, adaptive=False)
    d.update(kw)
    return d


K1 = [0]
K3 = [0, 17, 34]                                  # uniformly spaced: k9 takes it too
K70 = list(range(0, 512, 7))[:70]                 # two chunks, the second 6 wide
K33 = list(range(3, 36))
EVERY_COUNT_L = 32

# (bs, ue) of each order and orientation.  small_mh is neither 1 nor m on [5,3]/[3,2] (UE-small) and [3,2]/[7,1] (BS-small);
# M_big is odd on [3,3]/[5,1] (9), [5,3]/[3,2] (15), [5,3]/[7,1] (15), [3,2]/[7,1] (7) and [3,1]/[5,1] (5)
UE_SMALL = {3: ([4, 2], [3, 1]), 5: ([3, 3], [5, 1]), 6: ([5, 3], [3, 2]), 7: ([4, 2], [7, 1])}
BS_SMALL = {3: ([3, 1], [5, 1]), 5: ([5, 1], [3, 2]), 6: ([3, 2], [7, 1]), 7: ([7, 1], [4, 2])}


def _rate_cases():
    cs = []
    # m = 3
    cs.append(_case("m3_ue_K1", 23, 25, *UE_SMALL[3], 512, K1))                          # S = 8 = M_big
    cs.append(_case("m3_ue_K70", 23, 25, *UE_SMALL[3], 512, K70))
    cs.append(_case("m3_bs_K3", 23, 25, *BS_SMALL[3], 512, K3))                          # M_big = 5, S = 4
    cs.append(_case("m3_bs_2x2_K70", 23, 25, [3, 1], [2, 2], 512, K70))                  # M_big = 4 on two rows
    # m = 5
    cs.append(_case("m5_ue_K1", 33, 25, *UE_SMALL[5], 512, K1))                          # M_big = 9, S = 8: only slice 0 has a second t
    cs.append(_case("m5_ue_K70", 23, 25, *UE_SMALL[5], 512, K70))                        # S = 1, the last t alone
    cs.append(_case("m5_bs_K3", 23, 25, *BS_SMALL[5], 512, K3))                          # M_big = 6, S = 4
    # m = 6
    cs.append(_case("m6_ue_K3", 33, 25, *UE_SMALL[6], 512, K3))                          # M_big = 15, S = 8, small_mh = 3
    cs.append(_case("m6_ue_K70", 23, 25, *UE_SMALL[6], 512, K70))
    cs.append(_case("m6_bs_K1", 23, 25, *BS_SMALL[6], 512, K1))                          # M_big = 7, S = 4, small_mh = 3
    cs.append(_case("m6_bs_K70", 23, 25, *BS_SMALL[6], 512, K70))
    # m = 7.  27 users where the UE is the smaller array: with the rays of 23 users one user of 22 is rank-deficient far
    # above the median SNR and the tolerance share of tests/test_rate_cpu.py is 0.045 (K = 1, 3) and 0.072 / 0.062
    # ([4,2] / [5,3] at K = 70), over its cap of 0.05; with those of 27 it is 0.002 at most
    cs.append(_case("m7_ue_K1", 27, 25, *UE_SMALL[7], 512, K1))
    cs.append(_case("m7_ue_K3", 27, 25, *UE_SMALL[7], 512, K3))
    cs.append(_case("m7_ue_5x3_K70", 27, 25, [5, 3], [7, 1], 512, K70))                  # M_big = 15
    cs.append(_case("m7_bs_K3", 23, 25, *BS_SMALL[7], 512, K3))
    cs.append(_case("m7_bs_K70", 23, 25, *BS_SMALL[7], 512, K70))
    return cs


RATE_CASES = _rate_cases()

# user u keeps exactly u % 33 of 32 loaded paths; 37 users: 33 counts and a launch residue of one
EVERY_COUNT = _case("every_count", 37, EVERY_COUNT_L, [4, 2], [2, 1], 512, K3, num_paths=EVERY_COUNT_L, rays="every_count")

# rank 1 and rank 2 at odd order: Jacobi meets exact zeros, the sort meets ties, absent layers are +0.0
RANK_CASES = [_case(f"L{L}_m{m}", 50, L, *UE_SMALL[m], 64, [0, 9, 63]) for m in (3, 5) for L in (1, 2)]

# the order / orientation shapes, one selection each, and K = 33: one above k6's chunk of 32 at these shapes
COVARIANCE_CASES = [c for c in RATE_CASES if c["id"] in ("m3_ue_K1", "m3_bs_K3", "m5_ue_K1", "m5_bs_K3", "m6_ue_K3", "m6_bs_K1",
                                                         "m7_ue_K3", "m7_bs_K3", "m7_ue_5x3_K70")]
COVARIANCE_CASES = COVARIANCE_CASES + [_case("m5_ue_K33", 23, 25, *UE_SMALL[5], 512, K33), EVERY_COUNT]
# k6 has no limit of 8 elements: 9 and 15 on the UE side too
COVARIANCE_CASES += [_case("ue_3x3", 23, 25, [2, 1], [3, 3], 512, K3), _case("ue_5x3", 23, 25, [4, 2], [5, 3], 512, K1)]

UE_OF_ORDER = {1: [1, 1], 2: [2, 1], 3: [3, 1], 4: [2, 2], 5: [5, 1], 6: [3, 2], 7: [7, 1], 8: [4, 2]}
ML_PAIRS = [(M, L) for M in range(1, MAX_ORDER + 1) for L in range(1, min(M, MAX_LAYERS) + 1)]
ML_CODEWORDS = 5
ML_SUBBAND = 2                                    # K = 3: a subband of two and a short last one


def _codebook_cases():
    cs = [_case(f"ml_{M}_{L}", 19, 25, [4, 2], UE_OF_ORDER[M], 512, K3, layers=L, C=ML_CODEWORDS) for M, L in ML_PAIRS]
    # L = 3: 10 codewords fill a row chunk, the 11th starts a second one
    cs.append(_case("ml_3_3_C11", 19, 25, [4, 2], UE_OF_ORDER[3], 512, K3, layers=3, C=11))
    cs.append(dict(EVERY_COUNT, layers=2, C=ML_CODEWORDS))
    return cs


CODEBOOK_CASES = _codebook_cases()
SUBBAND_CASES = [(c["id"], ML_SUBBAND) for c in CODEBOOK_CASES]


def _cell(cid, links, serving_db=20.0, inr_db=10.0):
    """tests/test_gpu_cell_rate.py `_cell`"""
    links = [dict(c, id=f"{cid}_b{b}", selected=list(c["selected"])) for b, c in enumerate(links)]
    return dict(id=cid, links=links, serving_db=serving_db, inr_db=inr_db)


def _cell_cases():
    cs = []
    cs.append(_cell("ue3", [_case("", 23, 25, *UE_SMALL[3], 512, K3)] * 2))
    # links of 9, 16 and 15 BS elements: S = 8, 16, 8 inside one launch, the first and the last with a t of their own
    cs.append(_cell("ue5_mixed", [_case("", 23, 25, [3, 3], [5, 1], 512, K3), _case("", 23, 25, [4, 4], [5, 1], 512, K3),
                                  _case("", 23, 25, [5, 3], [5, 1], 512, K3)], serving_db=10.0))
    cs.append(_cell("ue5_bs3", [_case("", 23, 25, [3, 1], [5, 1], 512, K1)] * 2, serving_db=10.0, inr_db=0.0))
    cs.append(_cell("ue6", [_case("", 23, 25, *UE_SMALL[6], 512, K3)] * 2, serving_db=10.0))
    cs.append(_cell("ue7", [_case("", 23, 25, *UE_SMALL[7], 512, K1)] * 2, serving_db=10.0))
    return cs


CELL_CASES = _cell_cases()
ONE_LINK_CELLS = {3: "ue3", 5: "ue5_mixed", 6: "ue6", 7: "ue7"}     # the cell whose link 0 is the UE-small shape of order m

# k9: the UE shapes the `mrx` loop of tests/_angle_delay_cases.py gains, and the odd-M_tx antenna-row case
ANGLE_DELAY_UE = ([5, 1], [3, 2], [7, 1])
ANGLE_DELAY_ODD_TX = "ant_5x3"
ANGLE_DELAY_EVERY_COUNT = "every_count_ant"


def every_count_rays(c):
    """user u keeps exactly u % (L + 1) paths: NaN from that slot on, in every field (the holes of tests/test_gpu_rate.py
    `_case_rays`).  Every power lies in [-66, -60] dB (tests/_path_count_cases.py `flat`): with the generator's 80 dB of
    spread the last kept path is too weak for its loss to show in any output"""
    from oracle import oracle_np as onp
    from tests._path_count_cases import flat
    rays = flat(onp.synth_rays(c["n"], c["L"], seed=900 + c["n"], all_valid=True, max_delay=c["max_delay"]), 31)
    keys = [k for k in rays if k not in ("rx_pos", "tx_pos")]
    for u in range(c["n"]):
        for k in keys:
            rays[k][u, every_count_kept(c, u):] = np.nan
    return rays


def every_count_kept(c, u):
    return u % (c["L"] + 1)


def drop_last_path(rays):
    """mutation (c): the last kept path of every user removed"""
    out = {k: np.array(v, copy=True) for k, v in rays.items()}
    keys = [k for k in out if k not in ("rx_pos", "tx_pos")]
    valid = np.isfinite(out["power"])
    for u in range(valid.shape[0]):
        idx = np.flatnonzero(valid[u])
        if len(idx):
            for k in keys:
                out[k][u, idx[-1]] = np.nan
    return out


# ---- what a wrong index does to the reference ---------------------------------------------------------------------------
# mutation -> what it stands for; the sensitivity tests of tests/test_consumer_shapes_cpu.py apply no other, and a failure
# there prints the line
MUTATIONS = {
    "last_big": "the last element of the larger array missing (the `two`/S tail, a store that stops one short)",
    "last_small": "the last element of the smaller array missing (an order-templated loop that stops one short)",
    "transpose_small": "the smaller array's elements in transposed order, t = y + mh z <-> z + mv y",
    "swap_small_shape": "the smaller array's panel taken as [mv, mh] (a wrong small_mh in the t % mh, t / mh split)",
    "drop_last_path": "the last kept path of every user missing (the path loop's tail)",
    "last_codeword": "k10: the last codeword missing",
    "last_layer": "k10: the last layer of every codeword missing",
    # k8, k9, k10 are templated on M_rx whichever array is larger: the same faults named by the side
    "last_tx": "k8: the last BS element of every link missing (the `two`/S tail of that link's t loop)",
    "last_rx": "k8, k9, k10: the last UE element missing (an M_rx-templated loop that stops one short)",
    "last_row": "k9: the last row (BS element or codebook row) missing",
    "transpose_rx": "k9: the UE elements in transposed order",
    "swap_ue_shape": "k8, k10: the UE panel taken as [mv, mh] (a wrong ue_mh in the t % mh, t / mh split)",
}


def small_axis(H):
    """axis of H [n, M_rx, M_tx, K] the Gram runs over"""
    return 1 if H.shape[1] <= H.shape[2] else 2


def transposed_order(mh, mv):
    """element t = y + mh z of an [mh, mv] panel -> the element at z + mv y"""
    return np.array([(t // mh) + mv * (t % mh) for t in range(mh * mv)])


def mutate_channel(kind, H, c):
    """H [n, M_rx, M_tx, K] of the oracle with one index wrong (the tensor-level mutations)"""
    H = np.array(H, copy=True)
    ax = small_axis(H)
    big = 3 - ax
    if kind == "last_big":
        H[(slice(None),) * big + (-1,)] = 0
    elif kind == "last_small":
        H[(slice(None),) * ax + (-1,)] = 0
    elif kind == "transpose_small":
        shape = c["ue_shape"] if ax == 1 else c["bs_shape"]
        H = np.take(H, transposed_order(int(shape[0]), int(shape[1])), axis=ax)
    else:
        raise ValueError(kind)
    return H


def mutation_void(kind, c):
    """the reason a mutation leaves nothing to detect on a case by construction, or None"""
    m, small_is_rx, small_mh, M_big, _ = gram_order(c["bs_shape"], c["ue_shape"])
    if kind in ("transpose_small", "swap_small_shape") and small_mh in (1, m):
        return "the smaller array is a single row or column: both orders and both splits are the same elements"
    if kind == "swap_small_shape" and small_mh * small_mh == m:
        return "the smaller array is a square panel: [mv, mh] is the same panel"
    if kind == "last_big" and M_big == 1:
        return "one element on either side"
    return None


# outputs that do not change when an array's elements are permuted: a determinant, the eigenvalues, the sum over rx
PERMUTATION_INVARIANT = ("rate", "spectrum", "cell", "codebook")
PERMUTATIONS = ("transpose_small", "transpose_rx")


def sees(consumer, kind):
    """whether an output of `consumer` ("rate", "spectrum", "precoders", "covariance", "cell", "codebook", "subband",
    "angle_delay") can change under mutation `kind` at all"""
    assert kind in MUTATIONS, kind
    return not (kind in PERMUTATIONS and consumer in PERMUTATION_INVARIANT + ("subband",))


def panel_void(shape):
    """the reason taking an [mh, mv] panel as [mv, mh] is the same panel, or None"""
    mh, mv = int(shape[0]), int(shape[1])
    if mh in (1, mh * mv):
        return "a single row or column: both splits are the same elements"
    if mh == mv:
        return "a square panel: [mv, mh] is the same panel"
    return None
