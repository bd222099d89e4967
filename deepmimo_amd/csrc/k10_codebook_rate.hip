// Fused consumer of the per-path records: the rate of every codeword of a finite precoding codebook and the best codeword per
// user (the PMI and the rate behind a CQI of a CSI report), without the channel tensor.  W [C, L, M_tx]: C codewords of L
// layers, row W[c, i, :] multiplying the BS array as a row of F does in k2b_beam_project:
//   E[c, rx, i, k] = sum_tx W[c, i, tx] H[rx, tx, k] = sum_l a_rx[rx, l] f[c L + i, l] c_l g[l, k],   g[l, k] = exp(-j 2pi dn_l sc_k / N)
//   rate_c[u, c]   = 1/K sum_k log2 det(I_L + (snr / L) E_{c,k}^H E_{c,k}),   pmi[u] = argmax_c rate_c[u, c] (the first maximum)
//   rate[u]        = rate_c[u, pmi[u]]
// f is the row table k2b_beam_project wrote for the flattened codebook [C L, M_tx].  The Gram runs over the LAYERS (L x L,
// L <= M_rx: the Gram of the columns of E, positive semidefinite by construction), never over the UE array: for L < M_rx the
// M_rx x M_rx matrix I + s E E^H is rank-deficient beyond the identity and loses its last pivots to cancellation in fp32
// (k7_rate.hip says the same of its smaller-array rule).  The registers hold conj(E^H E), whose determinant is the same.
// One WAVE per user as k7_rate / k9_angle_delay: no workgroup barrier, the wave's tables in its own LDS slice, a flat grid.
//   1  as[M_rx][P]: the a_rx table (k7_rate's phase 1)
//   2  per chunk of kc = min(K, 64) subcarriers: w[l][k] = sqrt(snr / L) c_l g[l, k] PATH-MAJOR in LDS, the phase reduced in
//      float64 as the exact product (k7_rate's phase 2: any int32 subcarrier index)
//   3  ab[rc][P]: a chunk of WHOLE codewords of the row table, rc = L floor(32 / L) rows, copied as k9's phase 2'.  The row
//      chunks are the outer loop and the subcarrier chunks the inner one: w is rebuilt per pair (P kc sincos against the
//      rc M_rx P kc products it feeds), and a lane needs one accumulator instead of one per codeword.
//   4  lane = s kcp + k, kcp the power of two >= kc, S = 64 / kcp slices; slice s takes the codewords s, s + S, ... of the
//      chunk.  Per (codeword, subcarrier): rows_pair<M_rx> once per pair of layers (the third of three with its own row
//      again as the dummy, whose unused products the compiler drops), E in registers, the upper triangle of the L x L Gram,
//      epilogue_logdet<L>.  L = 1: the two rows of a call are two codewords of the slice, which share the reads of w and
//      a_rx; every row keeps its own chain of operations, so which rows share a call changes no bit.
//   5  the subcarriers of a chunk are added in a fixed xor tree over the log2(kcp) low lane bits (inactive lanes add +0.0),
//      which leaves the same bits in every lane of the slice; trip `it` of the codeword loop is kept by the lane whose
//      subcarrier index is `it` (at most 32 kcp / 64 <= kcp trips), chunk after chunk in chunk order, then times 1/K.  So
//      the value of a codeword depends on its rows and the user alone: not on its index, the other codewords or the launch.
//   6  the chunk's rates move to lanes 0 .. nc-1 in codeword order (one coalesced store of rate_c), a fixed xor tree picks
//      the largest, the lower index on ties, and the chunks are compared in order with a strict >: the first maximum.
// A user without a kept path: rate +0.0, pmi -1, rate_c +0.0.  LDS of one wave: (M_rx + min(C L, rc) + kc) * P * 8 bytes.
// Bound: fp32 VALU issue of rows_pair, C L rows of P (1 + M_rx) complex products per subcarrier; the row table is read once,
// C L P 8 bytes per user.
//
// Subband form (k10_codebook_rate_sb, dmx_codebook_rate_subbands): the same body with SB = true.  Subband s covers the
// selection positions s B .. min((s + 1) B, K) - 1, n_sb = ceil(K / B), and is processed exactly as the wideband kernel
// processes a selection that is that subband alone: kc = min(B, K, 64) and kcp for every subband of the launch, chunks from
// the subband's first subcarrier, the same xor tree, the chunks added in chunk order, then times (float)(1.0 / len_s) (a
// short last subband adds +0.0 in the idle tree lanes, which is exact).  The nest: row chunks outside as before (the row
// table is still read once), subbands next, a subband's chunks inside.  The lane that keeps a codeword is the same for
// every subband, so one more register there adds the subbands' sums in subband order: the wideband rate_c, times 1 / K.
// After each subband phase 6 runs on the subband's sums (one coalesced store into rate_sb_c, the xor argmax); where the
// codebook spans more than one row chunk lane 0 compares with the rate_sb entry it wrote itself on the earlier row chunks
// with a strict >, the first maximum again - no LDS, so n_sb has no limit but K.  Bit for bit rate_sb_c[:, s, :],
// rate_sb[:, s], pmi_sb[:, s] are what the wideband kernel gives for the selection sc[s B : (s + 1) B], and with one
// subband all six outputs are the wideband kernel's; with more than one the wideband outputs are another summation order of
// the same terms (held to the oracle tolerance only).  LDS of one wave: (M_rx + min(C L, rc) + min(B, K, 64)) * P * 8 bytes.
//
// Linear MMSE receiver (DMX_FLAG_RX_LINEAR_MMSE, the template parameter MMSE): phase 4 ends in epilogue_mmse<L> on the same Gram
// registers, sum_i log2(1 + sinr_i) = -sum_i log2 [(I + s G)^-1]_ii from L eliminations of L x L (k7_rate_body.h), in place of
// epilogue_logdet<L>.  Nothing else differs, so every statement above on bits and order holds with the flag on both sides.
// Instantiated for L >= 2 only: one layer is its own MMSE rate and the launcher takes the instantiation without the flag.
#include "dmx_common.h"
#include "k2_small_body.h"
#include "k7_rate_body.h"
#include <math.h>

namespace dmx {

static constexpr int CB_ROWS = 32;           // rows of the row table per LDS chunk, at most (whole codewords only)

struct CbArgs {
    int64_t user_begin, user_count;
    int ue_mh;
    int C;                   // codewords
    int cpc;                 // codewords per row chunk: floor(32 / L)
    int K, kc;               // selected subcarriers, subcarriers per chunk = w row stride
    int kcp, log2_kcp;       // power of two >= kc
    int S, log2_S;           // codeword slices = 64 / kcp
    const int32_t* sc;
    double inv_n;
    float scale;             // sqrt(snr / L)
    float inv_k;
    const float2* ftab;      // [user_count, C L, P] from k2b_beam_project
    int ld;                  // table row stride in path slots (= P)
    NearField nf;            // DMX_FLAG_NEAR_FIELD (array_phase.h): the UE table here, the BS side inside ftab's rows
};

struct SbArgs {              // the subband form only
    int B, n_sb;             // subcarriers per subband (<= K), subbands = ceil(K / B)
    float inv_full, inv_last;        // (float)(1.0 / B) and the same of the last subband's length
    float* rate_sb;          // [user_count, n_sb]
    int32_t* pmi_sb;         // [user_count, n_sb] or NULL
    float* rate_sb_c;        // [user_count, n_sb, C] or NULL
};

// 6  the sums of a row chunk's codewords (codeword j of the chunk in lane src_lane of lane j) times `inv` move to lanes
// 0 .. nc-1 in codeword order and are stored to out[at ..] (out NULL: not stored); a fixed xor tree leaves the largest and its index
// in the chunk, the lower index on ties, in every lane
__device__ __forceinline__ void chunk_best(float acc, float inv, int src_lane, int lane, int nc, float* out, size_t at, float& v, int& vi) {
    v = __shfl(acc, src_lane, 64) * inv;
    vi = lane;
    const bool mine = lane < nc;
    if (mine && out) out[at + lane] = v;
    v = mine ? v : -1.f;
    for (int d = 1; d < CB_ROWS; d <<= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(vi, d, 64);
        const bool take = ov > v || (ov == v && oi < vi);
        v = take ? ov : v; vi = take ? oi : vi;
    }
    v = __shfl(v, 0, 64); vi = __shfl(vi, 0, 64);
}

// SB = false: the wideband kernel (sb unused, out_rate not NULL); SB = true: the subband form, every wideband output optional.
// MMSE: the receiver of DMX_FLAG_RX_LINEAR_MMSE, epilogue_mmse<L> on the Gram in place of epilogue_logdet<L> (L > 1 only)
template <int M, int L, bool SB, bool MMSE>
__device__ __forceinline__ void codebook_rate_body(const WsView& ws, const CbArgs& a, const SbArgs& sb, float* __restrict__ out_rate,
                                                   int32_t* __restrict__ out_pmi, float* __restrict__ out_rate_c) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                          // waves never talk to each other
    const int ld = a.ld, C = a.C, K = a.K, kc = a.kc, S = a.S, cpc = a.cpc;
    const int rows_all = C * L, rc = rows_all < cpc * L ? rows_all : cpc * L;
    const size_t per_wave = (size_t)(M + rc + kc) * ld;
    float2* as = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * per_wave;     // [M][ld]
    float2* ab = as + (size_t)M * ld;                                                // [rc][ld]
    float2* w = ab + (size_t)rc * ld;                                                // [ld][kc]
    const int64_t u = a.user_begin + ul;
    float* oc = out_rate_c ? out_rate_c + (size_t)ul * C : nullptr;
    const int n = kept_paths(ws, u);
    const int n_sb = SB ? sb.n_sb : 1;
    if (n <= 0) {                                                            // no kept path
        if (oc) for (int i = lane; i < C; i += 64) oc[i] = 0.f;
        if constexpr (SB) {
            for (int i = lane; i < n_sb; i += 64) {
                sb.rate_sb[(size_t)ul * n_sb + i] = 0.f;
                if (sb.pmi_sb) sb.pmi_sb[(size_t)ul * n_sb + i] = -1;
            }
            if (sb.rate_sb_c) {
                float* o = sb.rate_sb_c + (size_t)ul * n_sb * C;
                for (size_t i = lane; i < (size_t)n_sb * C; i += 64) o[i] = 0.f;
            }
        }
        if (lane == 0) {
            if (!SB || out_rate) out_rate[ul] = 0.f;
            if (out_pmi) out_pmi[ul] = -1;
        }
        return;
    }
    const WsRecords rec{ws, (size_t)u * ws.P, a.nf};

    // 1  the a_rx table
    fill_array_table(as, rec, true, 0, M, a.ue_mh, n, ld, lane);

    const int kl = lane & (a.kcp - 1), sl = lane >> a.log2_kcp;              // this lane's subcarrier of the chunk and slice
    // where lane j finds codeword j of a chunk after phase 5: slice j mod S, trip j / S
    const int src_lane = ((lane & (S - 1)) << a.log2_kcp) + (lane >> a.log2_S);
    float best = -1.f;                                                       // every rate is >= 0: the first codeword wins
    int best_c = -1;
    for (int c0 = 0; c0 < C; c0 += cpc) {
        const int nc = C - c0 < cpc ? C - c0 : cpc;
        // 3  rows c0 L .. (c0 + nc) L of the row table: one contiguous block on both sides
        wave_lds_fence();                                                    // the last chunk's reads before this chunk's writes
        copy_rows_to_lds(ab, a.ftab, ((size_t)ul * rows_all + (size_t)c0 * L) * ld, nc * L * ld, lane);

        float wide = 0.f;                                                    // SB: the subbands' sums of this lane's codeword, in subband order
        for (int b = 0; b < n_sb; ++b) {
            const int ks = SB ? b * sb.B : 0;                                // the subband's positions ks .. ke - 1
            const int ke = SB ? (K - ks < sb.B ? K : ks + sb.B) : K;
            float acc = 0.f;                                                 // of codeword c0 + kl S + sl
            for (int k0 = ks; k0 < ke; k0 += kc) {
                const int kn = ke - k0 < kc ? ke - k0 : kc;
                // 2  w of the chunk
                wave_lds_fence();
                fill_w_chunk(w, rec, a.sc, k0, a.inv_n, a.scale, n, kn, kc, lane);
                wave_lds_fence();

                // 4, 5  one codeword per slice and trip
                const float2* wk = w + (kl < kn ? kl : 0);
                int it = 0;
                if constexpr (L == 1) {
                    // one layer: the two rows of a call are the codewords of trips `it` and `it + 1`
                    for (int cb = 0; cb < nc; cb += 2 * S, it += 2) {
                        const int ca = cb + sl, cc = cb + S + sl;
                        float lg0 = 0.f, lg1 = 0.f;
                        if (kl < kn && ca < nc) {
                            const bool two = cc < nc;
                            float2 e0[M], e1[M];
                            rows_pair<M>(as, ab + (size_t)ca * ld, ab + (size_t)(two ? cc : ca) * ld, wk, ld, kc, n, e0, e1);
                            float g0[1] = {0.f}, g1[1] = {0.f}, z0[1] = {0.f}, z1[1] = {0.f};
#pragma unroll
                            for (int i = 0; i < M; ++i) {                        // rx in index order
                                g0[0] = fmaf(e0[i].x, e0[i].x, fmaf(e0[i].y, e0[i].y, g0[0]));
                                g1[0] = fmaf(e1[i].x, e1[i].x, fmaf(e1[i].y, e1[i].y, g1[0]));
                            }
                            lg0 = epilogue_logdet<1>(g0, z0);
                            lg1 = two ? epilogue_logdet<1>(g1, z1) : 0.f;
                        }
                        for (int d = 1; d < a.kcp; d <<= 1) {
                            lg0 += __shfl_xor(lg0, d, 64);
                            lg1 += __shfl_xor(lg1, d, 64);
                        }
                        acc += kl == it ? lg0 : (kl == it + 1 ? lg1 : 0.f);
                    }
                } else {
                    for (int cb = 0; cb < nc; cb += S, ++it) {
                        const int ci = cb + sl;
                        float lg = 0.f;
                        if (kl < kn && ci < nc) {
                            const float2* rows = ab + (size_t)ci * L * ld;
                            float2 e[L + (L & 1)][M];                            // an odd L: the last row is the dummy's
                            rows_pair<M>(as, rows, rows + ld, wk, ld, kc, n, e[0], e[1]);
                            if constexpr (L > 2) {
                                rows_pair<M>(as, rows + (size_t)2 * ld, rows + (size_t)(L > 3 ? 3 : 2) * ld, wk, ld, kc, n, e[2], e[3]);
                            }
                            float gr[L * L], gi[L * L];
#pragma unroll
                            for (int p = 0; p < L; ++p) {
#pragma unroll
                                for (int q = p; q < L; ++q) {                    // G_pq = sum_rx e_p conj(e_q), rx in index order
                                    float r = 0.f, im = 0.f;
#pragma unroll
                                    for (int i = 0; i < M; ++i) {
                                        r = fmaf(e[p][i].x, e[q][i].x, fmaf(e[p][i].y, e[q][i].y, r));
                                        if (q > p) im = fmaf(e[p][i].y, e[q][i].x, fmaf(-e[p][i].x, e[q][i].y, im));
                                    }
                                    gr[p * L + q] = r; gi[p * L + q] = im;
                                    if (q > p) { gr[q * L + p] = 0.f; gi[q * L + p] = 0.f; }
                                }
                            }
                            if constexpr (MMSE) lg = epilogue_mmse<L>(gr, gi);
                            else lg = epilogue_logdet<L>(gr, gi);
                        }
                        for (int d = 1; d < a.kcp; d <<= 1) lg += __shfl_xor(lg, d, 64);
                        acc += kl == it ? lg : 0.f;
                    }
                }
            }

            // 6  codeword c0 + j in lane j, stored, and the chunk's first maximum
            float v;
            int vi;
            if constexpr (SB) {
                const size_t us = (size_t)ul * n_sb + b;
                chunk_best(acc, ke - ks == sb.B ? sb.inv_full : sb.inv_last, src_lane, lane, nc,
                           sb.rate_sb_c, us * C + c0, v, vi);
                // the subband's best over the row chunks so far is what this lane stored itself: a strict >, the first maximum
                if (lane == 0 && (c0 == 0 || v > sb.rate_sb[us])) {
                    sb.rate_sb[us] = v;
                    if (sb.pmi_sb) sb.pmi_sb[us] = c0 + vi;
                }
                wide += acc;
            } else {
                chunk_best(acc, a.inv_k, src_lane, lane, nc, oc, c0, v, vi);
                if (v > best) { best = v; best_c = c0 + vi; }
            }
        }
        if constexpr (SB) {                                                  // the wideband trio from the subbands' sums
            float v;
            int vi;
            chunk_best(wide, a.inv_k, src_lane, lane, nc, oc, c0, v, vi);
            if (v > best) { best = v; best_c = c0 + vi; }
        }
    }
    if (lane == 0) {
        if (!SB || out_rate) out_rate[ul] = best;
        if (out_pmi) out_pmi[ul] = best_c;
    }
}

template <int M, int L, bool MMSE = false>
__global__ __launch_bounds__(256) void k10_codebook_rate(WsView ws, CbArgs a, float* __restrict__ out_rate,
                                                         int32_t* __restrict__ out_pmi, float* __restrict__ out_rate_c) {
    codebook_rate_body<M, L, false, MMSE>(ws, a, SbArgs{}, out_rate, out_pmi, out_rate_c);
}

template <int M, int L, bool MMSE = false>
__global__ __launch_bounds__(256) void k10_codebook_rate_sb(WsView ws, CbArgs a, SbArgs sb, float* __restrict__ out_rate,
                                                            int32_t* __restrict__ out_pmi, float* __restrict__ out_rate_c) {
    codebook_rate_body<M, L, true, MMSE>(ws, a, sb, out_rate, out_pmi, out_rate_c);
}

// LDS bytes of one wave for P path slots (0: the shape is not taken): the a_rx table, one chunk of whole codewords of the
// row table and one chunk of w,
//   (M_rx + min(C * L, rc) + kc) * P * 8,   M_rx <= 8,  rc = L * floor(32 / L),  kc = min(n_selected, 64)
// lds_waves_per_block turns that into 4 / 2 waves per workgroup (at most 26,624 bytes per wave).  The subband form has
// kc = min(subband_size, n_selected, 64) and nothing else in the LDS, so it never needs more.
static size_t cb_lds_bytes(const dmx_params& prm, int P, int n_codewords, int n_layers, size_t kc) {
    if (P < 1 || P > 32 || n_codewords < 1 || n_layers < 1 || n_layers > 4 || prm.n_selected < 1 || kc < 1) return 0;
    const size_t m_rx = (size_t)prm.ue_shape[0] * prm.ue_shape[1];
    if (m_rx > 8 || (size_t)n_layers > m_rx) return 0;
    const size_t rows = (size_t)n_codewords * n_layers, rcm = (size_t)n_layers * (CB_ROWS / n_layers);
    const size_t rc = rows < rcm ? rows : rcm;
    return (m_rx + rc + kc) * (size_t)P * sizeof(float2);
}

size_t codebook_rate_lds_bytes(const dmx_params& prm, int P, int n_codewords, int n_layers) {
    return cb_lds_bytes(prm, P, n_codewords, n_layers, prm.n_selected < 64 ? prm.n_selected : 64);
}

int codebook_rate_waves_per_block(const dmx_params& prm, int P, int n_codewords, int n_layers) {
    return lds_waves_per_block(codebook_rate_lds_bytes(prm, P, n_codewords, n_layers));
}

size_t codebook_rate_subbands_lds_bytes(const dmx_params& prm, int P, int n_codewords, int n_layers, int subband_size) {
    if (subband_size < 1) return 0;
    const int kc = prm.n_selected < 64 ? prm.n_selected : 64;
    return cb_lds_bytes(prm, P, n_codewords, n_layers, subband_size < kc ? subband_size : kc);
}

int codebook_rate_subbands_waves_per_block(const dmx_params& prm, int P, int n_codewords, int n_layers, int subband_size) {
    return lds_waves_per_block(codebook_rate_subbands_lds_bytes(prm, P, n_codewords, n_layers, subband_size));
}

namespace {

struct CbLaunch {
    dim3 g, b;
    size_t smem;
    hipStream_t stream;
    const WsView* ws;
    const CbArgs* a;
    const SbArgs* sb;        // NULL: the wideband kernel
    bool mmse;               // DMX_FLAG_RX_LINEAR_MMSE
    float* out_rate;
    int32_t* out_pmi;
    float* out_rate_c;
};

// the linear MMSE receiver's instantiations, two layers or more
template <int M, int L>
int launch_cb_mmse(const CbLaunch& l) {
    if (l.sb) {
        return launch_dyn_lds(k10_codebook_rate_sb<M, L, true>, "k10_codebook_rate_sb", l.g, l.b, l.smem, WAVE_LDS_MAX, l.stream,
                              *l.ws, *l.a, *l.sb, l.out_rate, l.out_pmi, l.out_rate_c);
    }
    return launch_dyn_lds(k10_codebook_rate<M, L, true>, "k10_codebook_rate", l.g, l.b, l.smem, WAVE_LDS_MAX, l.stream, *l.ws, *l.a,
                          l.out_rate, l.out_pmi, l.out_rate_c);
}

template <int M, int L>
int launch_cb_ml(const CbLaunch& l) {
    if constexpr (L <= M) {
        // one layer is its own linear MMSE rate: the flag picks the instantiation below, the same bits
        if constexpr (L > 1) {
            if (l.mmse) return launch_cb_mmse<M, L>(l);
        }
        if (l.sb) {
            return launch_dyn_lds(k10_codebook_rate_sb<M, L>, "k10_codebook_rate_sb", l.g, l.b, l.smem, WAVE_LDS_MAX, l.stream, *l.ws,
                                  *l.a, *l.sb, l.out_rate, l.out_pmi, l.out_rate_c);
        }
        return launch_dyn_lds(k10_codebook_rate<M, L>, "k10_codebook_rate", l.g, l.b, l.smem, WAVE_LDS_MAX, l.stream, *l.ws, *l.a,
                              l.out_rate, l.out_pmi, l.out_rate_c);
    } else {
        set_error("codebook rate: n_layers = %d exceeds M_rx = %d", L, M);
        return DMX_ERR_SHAPE;
    }
}

template <int M>
int launch_cb_m(const CbLaunch& l, int n_layers) {
    switch (n_layers) {
        case 1: return launch_cb_ml<M, 1>(l);
        case 2: return launch_cb_ml<M, 2>(l);
        case 3: return launch_cb_ml<M, 3>(l);
        default: return launch_cb_ml<M, 4>(l);
    }
}

}  // namespace

// the projection of the flattened codebook [C L, M_tx] into beam_ws (beam_workspace_bytes), then the kernel; sb: the subband
// form's outputs with B = the subband size (any value >= 1), the rest filled in here, or NULL
static int launch_cb(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, const float2* codebook,
                     int n_codewords, int n_layers, void* beam_ws, double snr_linear, SbArgs* sb, float* out_rate, int32_t* out_pmi,
                     float* out_rate_c, hipStream_t stream) {
    if (user_count == 0) return DMX_OK;
    const size_t lds = sb ? codebook_rate_subbands_lds_bytes(prm, ws.P, n_codewords, n_layers, sb->B)
                          : codebook_rate_lds_bytes(prm, ws.P, n_codewords, n_layers);
    const int wpb = lds_waves_per_block(lds);
    if (!wpb) { set_error("codebook rate kernel: tables of one user do not fit the LDS"); return DMX_ERR_SHAPE; }
    BeamTabs t;
    int rc = launch_beam_project(prm, ws, user_begin, user_count, codebook, n_codewords * n_layers, beam_ws, stream, &t);
    if (rc) return rc;
    CbArgs a;
    a.user_begin = user_begin; a.user_count = user_count;
    a.ue_mh = prm.ue_shape[0];
    a.nf = near_field_of(prm);
    a.C = n_codewords; a.cpc = CB_ROWS / n_layers;
    a.K = prm.n_selected; a.kc = a.K < 64 ? a.K : 64;
    if (sb) {
        sb->B = sb->B < a.K ? sb->B : a.K;
        sb->n_sb = (a.K + sb->B - 1) / sb->B;
        sb->inv_full = (float)(1.0 / (double)sb->B);
        sb->inv_last = (float)(1.0 / (double)(a.K - (sb->n_sb - 1) * sb->B));
        a.kc = sb->B < a.kc ? sb->B : a.kc;          // a subband is a selection of its own: kc = min(B, K, 64)
    }
    a.log2_kcp = 0;
    while ((1 << a.log2_kcp) < a.kc) ++a.log2_kcp;
    a.kcp = 1 << a.log2_kcp;
    a.log2_S = 6 - a.log2_kcp; a.S = 1 << a.log2_S;
    a.sc = prm.selected_subcarriers;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.scale = (float)sqrt(snr_linear / (double)n_layers);
    a.inv_k = (float)(1.0 / (double)a.K);
    a.ftab = t.ftab;
    a.ld = ws.P;
    const int m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    CbLaunch l;
    l.smem = (size_t)wpb * lds;
    l.g = dim3((unsigned)((user_count + wpb - 1) / wpb)); l.b = dim3(64 * wpb);      // flat: one wave per user
    l.stream = stream; l.ws = &ws; l.a = &a; l.sb = sb;
    l.mmse = (prm.flags & DMX_FLAG_RX_LINEAR_MMSE) != 0;
    l.out_rate = out_rate; l.out_pmi = out_pmi; l.out_rate_c = out_rate_c;
    switch (m_rx) {
        case 1: return launch_cb_m<1>(l, n_layers);
        case 2: return launch_cb_m<2>(l, n_layers);
        case 3: return launch_cb_m<3>(l, n_layers);
        case 4: return launch_cb_m<4>(l, n_layers);
        case 5: return launch_cb_m<5>(l, n_layers);
        case 6: return launch_cb_m<6>(l, n_layers);
        case 7: return launch_cb_m<7>(l, n_layers);
        default: return launch_cb_m<8>(l, n_layers);
    }
}

int launch_codebook_rate(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, const float2* codebook,
                         int n_codewords, int n_layers, void* beam_ws, double snr_linear, float* out_rate, int32_t* out_pmi,
                         float* out_rate_c, hipStream_t stream) {
    return launch_cb(prm, ws, user_begin, user_count, codebook, n_codewords, n_layers, beam_ws, snr_linear, nullptr, out_rate,
                     out_pmi, out_rate_c, stream);
}

int launch_codebook_rate_subbands(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                                  const float2* codebook, int n_codewords, int n_layers, void* beam_ws, double snr_linear,
                                  int subband_size, float* out_rate_sb, int32_t* out_pmi_sb, float* out_rate_sb_c, float* out_rate,
                                  int32_t* out_pmi, float* out_rate_c, hipStream_t stream) {
    SbArgs sb{};
    sb.B = subband_size;
    sb.rate_sb = out_rate_sb; sb.pmi_sb = out_pmi_sb; sb.rate_sb_c = out_rate_sb_c;
    return launch_cb(prm, ws, user_begin, user_count, codebook, n_codewords, n_layers, beam_ws, snr_linear, &sb, out_rate, out_pmi,
                     out_rate_c, stream);
}

}  // namespace dmx
