// Fused consumer of the per-path records of SEVERAL links over the same users (one base station each, B <= DMX_MAX_LINKS):
// the downlink rate of every user on its serving link while the other links transmit, without any channel tensor.
//   N_k         = I + sum_{b != s} rho_b H_{b,k} H_{b,k}^H,      rho_b = snr_b / M_tx,b           (M_rx x M_rx)
//   A_k         = N_k + rho_s H_{s,k} H_{s,k}^H
//   rate_k[u,k] = log2 det A_k - log2 det N_k  (>= 0),           rate[u] = 1/K sum_k rate_k[u,k]
//   link_snr[u,b] = snr_b sum_{l kept} |c_{b,l}|^2,              s = serving[u] or the first argmax_b link_snr[u,b]
// The arithmetic is k7_rate's with one more loop: the interference covariance lives on the UE array (at most 8 x 8), so the
// links add into it one after the other and a wave needs the LDS tables of ONE link at a time - its slice is sized by the
// largest link, whatever B is.  The Gram always runs over the UE array (M = M_rx <= 8), t over the link's BS array, also
// where M_tx < M_rx: all links have to meet in the same M_rx x M_rx matrix.
// One WAVE per user, a flat grid, no workgroup barrier.
//   0  per link, before anything else: lane l squares c_l, a fixed xor tree adds the lanes, link_snr = snr_b * sum; the
//      automatic serving link is the first strict maximum in link order (-1 if no link of the user has a kept path)
//   per chunk of kc = min(K, 64) subcarriers and per link with kept paths, in link order, on that link's records:
//   1  array tables a_rx[M][l], a_tx[M_tx,b][l] (k7_rate's phase 1).  They are REBUILT per (chunk, link) when B > 1 - the
//      slice holds one link - and built once when B = 1; (M + M_tx) P / 64 sincos per lane against M_tx P (1 + M) complex
//      products in phase 3, below 1 % of it
//   2  w[l][k] path-major, carrying sqrt(rho_b) (k7_rate's phase 2)
//   3  k7_rate's phase 3 on rows_pair (k7_rate_body.h) with the slice rule S of THIS link: lane = k S_b + s.  Links differ
//      in S_b, so the reduced Gram is then moved to lane k (one __shfl per entry; nothing moves where S_b = 1)
//      The interferers add into G_int in link order; the serving link's Gram is kept aside.
//   4  A = G_int + G_s on those same floats, so an interferer's rounding error enters both determinants alike; both
//      determinants by epilogue_logdet on copies, the difference clamped to 0 .. FLT_MAX.  The lane sums its chunks in chunk
//      order, the wave adds the lanes in a fixed xor tree.
// B = 1: G_int = 0, log2 det N = 0 exactly and the steps above are k7_rate<M, EPI_LOGDET>'s for M_rx <= M_tx - the same bits.
// fp32 vector arithmetic, no atomics, every sum in a fixed order that does not depend on where the user sits in the launch.
// LDS of one wave: max_b (M_rx + M_tx,b + kc) * P_b * 8 bytes; cell_rate_lds_bytes has the rule.
// SET (DMX_FLAG_SERVING_SET on every link): serving[u] is a set of links, bit b = link b transmits to the user.  The same
// steps with another destination of the adds: the members' Grams add into the serving Gram in link order (the first one is
// copied, as the one serving link is without the flag), everything else into G_int.  A set of one bit runs the steps of that
// index bit for bit; the full set leaves G_int = 0 and gives log2 det(I + sum_b G_b).
#include "dmx_common.h"
#include "k2_small_body.h"
#include "k7_rate_body.h"
#include <math.h>

namespace dmx {

struct CellLink {
    WsView ws;
    int m_tx, tx_mh;
    int S, log2_S;       // slices of the BS array per subcarrier (1 unless K < 64)
    float scale;         // sqrt(snr_b / M_tx,b)
    double snr;
    NearField nf;        // DMX_FLAG_NEAR_FIELD of this link's parameters (array_phase.h)
};

struct CellArgs {
    int64_t user_begin, user_count;
    int n_links, rx_mh;
    int K, kc;           // selected subcarriers, subcarriers per chunk = w row stride
    const int32_t* sc;   // the selection of link 0
    double inv_n;
    float inv_k;
    unsigned per_wave;   // float2 slots of one wave's slice: the largest link's tables
    CellLink link[DMX_MAX_LINKS];
};

// 1, 2, 4  the table fills, rows_pair of phase 3 and epilogue_logdet: k7_rate_body.h, shared with k7_rate.hip

// 3  slice sl of S of the large array (t = sl, sl + S, ...) for this lane's subcarrier, added to the upper triangle in gr, gi
template <int M>
__device__ __forceinline__ void gram_accumulate(const float2* as, const float2* ab, const float2* wk, const int ld, const int kc,
                                                const int n, const int Mb, const int sl, const int S, float (&gr)[M * M],
                                                float (&gi)[M * M]) {
    for (int t = sl; t < Mb; t += 2 * S) {
        const bool two = t + S < Mb;
        const float2* b0 = ab + (size_t)t * ld;
        const float2* b1 = ab + (size_t)(two ? t + S : t) * ld;
        float2 h0[M], h1[M];
        rows_pair<M>(as, b0, b1, wk, ld, kc, n, h0, h1);
        if (!two) {
#pragma unroll
            for (int i = 0; i < M; ++i) h1[i] = make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = i; j < M; ++j) {                            // G_ij += h_i conj(h_j), first t then t + S
                float r = gr[i * M + j], im = gi[i * M + j];
                r = fmaf(h0[i].x, h0[j].x, fmaf(h0[i].y, h0[j].y, r));
                r = fmaf(h1[i].x, h1[j].x, fmaf(h1[i].y, h1[j].y, r));
                if (j > i) {
                    im = fmaf(h0[i].y, h0[j].x, fmaf(-h0[i].x, h0[j].y, im));
                    im = fmaf(h1[i].y, h1[j].x, fmaf(-h1[i].x, h1[j].y, im));
                }
                gr[i * M + j] = r; gi[i * M + j] = im;
            }
        }
    }
}

// the slices of a subcarrier sit in S neighbouring lanes: a fixed xor tree leaves the sum in each of them
template <int M>
__device__ __forceinline__ void gram_reduce(const int S, float (&gr)[M * M], float (&gi)[M * M]) {
    for (int d = 1; d < S; d <<= 1) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = i; j < M; ++j) {
                gr[i * M + j] += __shfl_xor(gr[i * M + j], d, 64);
                if (j > i) gi[i * M + j] += __shfl_xor(gi[i * M + j], d, 64);
            }
        }
    }
}

template <int M, bool SET>
__global__ __launch_bounds__(256) void k8_cell_rate(CellArgs a, const int32_t* __restrict__ serving, float* __restrict__ out_rate,
                                                    float* __restrict__ out_rate_k, int32_t* __restrict__ out_serving,
                                                    float* __restrict__ out_link_snr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                          // waves never talk to each other
    const int B = a.n_links, K = a.K, kc = a.kc;
    float2* as = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * a.per_wave;    // [M][ld] of the link at hand
    const int64_t u = a.user_begin + ul;
    float* ok = out_rate_k ? out_rate_k + (size_t)ul * K : nullptr;

    // 0  wideband receive SNR per link and the serving link
    int s = 0;
    float best = -1.f;
    bool any = false;
    int reach = 0;                                                           // bit b: link b has a kept path to the user
    for (int b = 0; b < B; ++b) {
        const WsView& ws = a.link[b].ws;
        const int n = kept_paths(ws, u);
        float p = 0.f;
        if (lane < n) {                                                      // P <= 32: a lane per path
            const float cr = ws.c_re[(size_t)u * ws.P + lane], ci = ws.c_im[(size_t)u * ws.P + lane];
            p = fmaf(cr, cr, ci * ci);
        }
        for (int d = 1; d < 64; d <<= 1) p += __shfl_xor(p, d, 64);
        const float ls = (float)fmin((double)p * a.link[b].snr, 3.402823466e38);
        if (out_link_snr && lane == 0) out_link_snr[(size_t)ul * B + b] = ls;
        any = any || n > 0;
        if (n > 0) reach |= 1 << b;
        if (ls > best) { best = ls; s = b; }                                 // strictly: the first of equal values
    }
    int n_s = 0;
    if constexpr (SET) {                                                     // s: the set, bit b = link b serves
        s = serving ? serving[ul] : -1;                                      // NULL: every link
        if (serving && s < 0) s = 0;                                         // a negative entry: nobody
        s = __builtin_amdgcn_readfirstlane(s) & ((1 << B) - 1);              // B <= DMX_MAX_LINKS = 8
        if (out_serving && lane == 0) out_serving[ul] = s;
        n_s = (s & reach) != 0;                                              // a member reaches the user
    } else {
        if (serving) s = serving[ul]; else if (!any) s = -1;
        s = __builtin_amdgcn_readfirstlane(s);
        if (s < 0 || s >= B) s = -1;
        if (out_serving && lane == 0) out_serving[ul] = s;
        if (s >= 0) n_s = kept_paths(a.link[s].ws, u);
    }
    if (n_s <= 0) {                                                          // not served, or no kept path to be served by
        if (ok) for (int i = lane; i < K; i += 64) ok[i] = 0.f;
        if (lane == 0) out_rate[ul] = 0.f;
        return;
    }

    float rate_sum = 0.f;
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc;
        float ir[M * M], ii[M * M], sr[M * M], si[M * M];                    // G_int and the serving link's Gram, lane = k
#pragma unroll
        for (int i = 0; i < M * M; ++i) ir[i] = ii[i] = sr[i] = si[i] = 0.f;
        bool first = true;                                                   // SET: no member's Gram is in sr, si yet
        for (int b = 0; b < B; ++b) {
            const CellLink& lk = a.link[b];
            const int ld = lk.ws.P, Mb = lk.m_tx;
            const int n = kept_paths(lk.ws, u);
            if (n <= 0) continue;                                            // this link does not reach the user
            const WsRecords rec{lk.ws, (size_t)u * ld, lk.nf};
            float2* ab = as + (size_t)M * ld;                                // [Mb][ld]
            float2* w = ab + (size_t)Mb * ld;                                // [ld][kc]
            wave_lds_fence();                                                // the last link's reads before this link's writes
            // 1  array tables of this link
            if (B > 1 || k0 == 0) {
                fill_array_table(as, rec, true, 0, M, a.rx_mh, n, ld, lane);
                fill_array_table(ab, rec, false, 0, Mb, lk.tx_mh, n, ld, lane);
            }
            // 2  w of the chunk
            fill_w_chunk(w, rec, a.sc, k0, a.inv_n, lk.scale, n, kn, kc, lane);
            wave_lds_fence();

            // 3  this lane's share of the upper triangle of the link's Gram, lane = k S + slice
            float gr[M * M], gi[M * M];
#pragma unroll
            for (int i = 0; i < M * M; ++i) gr[i] = gi[i] = 0.f;
            const int kl = lane >> lk.log2_S, sl = lane & (lk.S - 1);
            if (kl < kn) gram_accumulate<M>(as, ab, w + kl, ld, kc, n, Mb, sl, lk.S, gr, gi);
            gram_reduce<M>(lk.S, gr, gi);
            if (lk.log2_S) {                                                 // subcarrier k from lane k S to lane k
                const int src = (lane << lk.log2_S) & 63;
#pragma unroll
                for (int i = 0; i < M; ++i) {
#pragma unroll
                    for (int j = i; j < M; ++j) {
                        gr[i * M + j] = __shfl(gr[i * M + j], src, 64);
                        if (j > i) gi[i * M + j] = __shfl(gi[i * M + j], src, 64);
                    }
                }
            }
            const bool mine = SET ? ((s >> b) & 1) != 0 : b == s;
            if (mine && (!SET || first)) {
#pragma unroll
                for (int i = 0; i < M * M; ++i) { sr[i] = gr[i]; si[i] = gi[i]; }
                first = false;
            } else if (mine) {
#pragma unroll
                for (int i = 0; i < M * M; ++i) { sr[i] += gr[i]; si[i] += gi[i]; }
            } else {
#pragma unroll
                for (int i = 0; i < M * M; ++i) { ir[i] += gr[i]; ii[i] += gi[i]; }
            }
        }

        // 4  log2 det(I + G_int + G_s) - log2 det(I + G_int)
#pragma unroll
        for (int i = 0; i < M * M; ++i) { sr[i] += ir[i]; si[i] += ii[i]; }
        const float lg_a = epilogue_logdet<M>(sr, si), lg_n = epilogue_logdet<M>(ir, ii);
        const float lg = fminf(fmaxf(lg_a - lg_n, 0.f), 3.402823466e38f);
        if (lane < kn) {
            if (ok) ok[k0 + lane] = lg;
            rate_sum += lg;
        }
    }
    for (int d = 1; d < 64; d <<= 1) rate_sum += __shfl_xor(rate_sum, d, 64);
    if (lane == 0) out_rate[ul] = rate_sum * a.inv_k;
}

static inline int link_paths(const dmx_link& l) { return l.prm->num_paths < l.n_paths_loaded ? l.prm->num_paths : l.n_paths_loaded; }

// LDS bytes of one wave (0: a link's shape is not taken): the tables of the largest link and one chunk of w,
//   max_b (M_rx + M_tx,b + kc) * P_b * 8,   M_rx <= 8,  P_b = min(num_paths, loaded paths) in 1..32,  kc = min(n_selected, 64)
// lds_waves_per_block turns that into 4 / 2 / 1 waves per workgroup (16 KB / 32 KB / 156 KB per wave).
size_t cell_rate_lds_bytes(const dmx_link* links, int n_links) {
    size_t most = 0;
    for (int b = 0; b < n_links; ++b) {
        const dmx_params& prm = *links[b].prm;
        const int P = link_paths(links[b]);
        const size_t m_tx = (size_t)prm.bs_shape[0] * prm.bs_shape[1], m_rx = (size_t)prm.ue_shape[0] * prm.ue_shape[1];
        if (P < 1 || P > 32 || prm.n_selected < 1 || m_rx > 8) return 0;
        const size_t kc = prm.n_selected < 64 ? prm.n_selected : 64;
        const size_t bytes = (m_rx + m_tx + kc) * (size_t)P * sizeof(float2);
        most = bytes > most ? bytes : most;
    }
    return most;
}

template <int M>
static int launch_cell_m(const bool set, const dim3 g, const dim3 b, size_t smem, hipStream_t stream, const CellArgs& a,
                         const int32_t* serving, float* out_rate, float* out_rate_k, int32_t* out_serving, float* out_link_snr) {
    if (set)
        return launch_dyn_lds(k8_cell_rate<M, true>, "k8_cell_rate", g, b, smem, WAVE_LDS_MAX, stream, a, serving, out_rate,
                              out_rate_k, out_serving, out_link_snr);
    return launch_dyn_lds(k8_cell_rate<M, false>, "k8_cell_rate", g, b, smem, WAVE_LDS_MAX, stream, a, serving, out_rate,
                          out_rate_k, out_serving, out_link_snr);
}

// links: checked by the caller (dmx_abi.hip, cell_rate_shape): equal ue_shape, n_subcarriers and n_selected, M_rx <= 8,
// DMX_FLAG_SERVING_SET on every link or on none - link 0 picks the instantiation
int launch_cell_rate(const dmx_link* links, int n_links, int64_t n_ue, int64_t user_begin, int64_t user_count,
                     const int32_t* serving, float* out_rate, float* out_rate_k, int32_t* out_serving, float* out_link_snr,
                     hipStream_t stream) {
    const size_t bytes = cell_rate_lds_bytes(links, n_links);
    const int wpb = lds_waves_per_block(bytes);
    if (!wpb) { set_error("cell rate kernel: tables of one link do not fit the LDS"); return DMX_ERR_SHAPE; }
    const dmx_params& p0 = *links[0].prm;
    CellArgs a;
    a.user_begin = user_begin; a.user_count = user_count;
    a.n_links = n_links;
    a.rx_mh = p0.ue_shape[0];
    a.K = p0.n_selected; a.kc = a.K < 64 ? a.K : 64;
    a.sc = p0.selected_subcarriers;
    a.inv_n = 1.0 / (double)p0.n_subcarriers;
    a.inv_k = (float)(1.0 / (double)a.K);
    a.per_wave = (unsigned)(bytes / sizeof(float2));
    for (int b = 0; b < DMX_MAX_LINKS; ++b) {
        CellLink& lk = a.link[b];
        const dmx_link& src = links[b < n_links ? b : 0];                    // the unused entries: a copy, never read
        const dmx_params& prm = *src.prm;
        ws_carve(const_cast<void*>(src.workspace), n_ue, link_paths(src), &lk.ws);
        lk.m_tx = prm.bs_shape[0] * prm.bs_shape[1];
        lk.tx_mh = prm.bs_shape[0];
        lk.log2_S = gram_slices_log2(a.K, lk.m_tx);
        lk.S = 1 << lk.log2_S;
        lk.scale = (float)sqrt(src.snr_linear / (double)lk.m_tx);
        lk.snr = src.snr_linear;
        lk.nf = near_field_of(prm);
    }
    const int m_rx = p0.ue_shape[0] * p0.ue_shape[1];
    const bool set = (p0.flags & DMX_FLAG_SERVING_SET) != 0;
    const size_t smem = (size_t)wpb * bytes;
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), blk(64 * wpb);  // flat: one wave per user
    switch (m_rx) {
        case 1: return launch_cell_m<1>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 2: return launch_cell_m<2>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 3: return launch_cell_m<3>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 4: return launch_cell_m<4>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 5: return launch_cell_m<5>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 6: return launch_cell_m<6>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        case 7: return launch_cell_m<7>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
        default: return launch_cell_m<8>(set, g, blk, smem, stream, a, serving, out_rate, out_rate_k, out_serving, out_link_snr);
    }
}

}  // namespace dmx
