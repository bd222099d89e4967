// Fused consumer of the per-path records: the per-user achievable rate of the frequency-domain channel
// with equal power on every transmit antenna and no channel knowledge at the transmitter, without the channel tensor:
//   H_k[r,t]     = sum_l c_l a_rx[r,l] a_tx[t,l] g[l,k],            g[l,k] = exp(-j 2pi dn_l sc_k / N)
//   rate_k[u,k]  = log2 det(I + (snr / M_tx) H_k H_k^H) = log2 det(I + G_k),   rate[u] = 1/K sum_k rate_k[u,k]
//   G_k[i,j]     = sum_t h_i[t] conj(h_j[t]),   h_i[t] = sum_l a_small[i,l] a_big[t,l] w[l,k],   w[l,k] = sqrt(snr / M_tx) c_l g[l,k]
// det(I + s H H^H) = det(I + s H^H H): the Gram matrix is formed over the SMALLER array (m = min(M_rx, M_tx) <= 8 elements,
// the UE side on a tie), t runs over the larger one.  G is the Gram of the rows h_i and so positive semidefinite by
// construction, whatever fp32 does to the rows; the P x P path-coupling route (G = V T V^H) is cheaper but loses that, and a
// rank-1 user at high SNR then shows a spurious second eigenvalue of either sign.
// One WAVE per user as k6_covariance: no workgroup barrier, the wave's tables in its own LDS slice, a flat grid.
//   1  array tables a_small[m][l], a_big[M_big][l]: float64 phase reduction + sincos_rev
//   2  per chunk of kc = min(K, 64) subcarriers: w[l][k] PATH-MAJOR in LDS (phase = fma(x, k, -rint(x k)) in float64, any
//      int32 index), so lanes that own consecutive subcarriers read consecutive words and a_small / a_big reads broadcast
//   3  a lane owns a subcarrier - or, for K < 64, a (subcarrier, slice s of S) pair, lane = k S + s, S a power of two, slice s
//      taking t = s, s + S, ... - and adds the upper triangle of G in registers, two t per trip of the path loop; the slices
//      of a subcarrier are added in a fixed xor tree across the lanes
//   4  unrolled elimination of I + G (the kernel is templated on m): every pivot is >= 1 in exact arithmetic and is clamped
//      to that, rate_k = sum log2(pivot); rate_k is stored coalesced if wanted; the lane sums its chunks in chunk order, the
//      wave adds the lanes in a fixed xor tree
//   4' the second epilogue on the same body (the kernel is templated on it; dmx_channel_spectrum): w carries sqrt(snr), so G
//      holds mode SNRs (order 1 .. 1e6, not raw gains near 1e-15); a cyclic complex Jacobi iteration on the upper triangle
//      in registers leaves the eigenvalues gamma_i = snr lambda_i(H_k H_k^H) on the diagonal - pair (p, q): phase of G_pq,
//      tau = (G_qq - G_pp) / (2 |G_pq|), t = sign(tau) / (|tau| + sqrt(1 + tau^2)), branch-free with t = 0 where
//      |G_pq| = 0, no eigenvectors - clamped to >= 0, sorted descending by a compile-time odd-even transposition network,
//      then the water-filling rate in closed form (at most m steps).  gamma is stored m consecutive floats per lane.
//      The sweep count is fixed per m, the same for every lane, with no data-dependent exit:
//          m       1  2  3  4  5  6  7  8
//          needed  0  1  4  5  5  6  7  7
//          SWEEPS  0  2  5  6  6  7  8  8
//      "needed": the smallest count after which a float32 NumPy restatement of jacobi_sweep (tests/_spectrum_ref.py,
//      jacobi_f32) leaves the off-diagonal Frobenius norm <= 2^-24 |G|_F on 2403 hard synthetic matrices per m (rank one,
//      two equal eigenvalues, clustered values, a 1e6 spread, diagonal, equal diagonals, Wishart) and on the Grams of every
//      GPU test case; SWEEPS is that plus one sweep of margin.  tests/test_spectrum_cpu.py holds the table to the model.
//      A non-zero eigenvalue repeated three times or more stalls that norm at about 40 * 2^-24 |G|_F (the diagonal
//      differences inside the cluster sit at the float32 spacing of the eigenvalue); the eigenvalues do not move.
//   4" the third epilogue (EPI_VECTORS; dmx_channel_precoders): the same iteration with the rotations accumulated in an
//      m x m matrix X in registers (X starts as I and takes, on all m rows, the column update of G), so that the columns of
//      X are the eigenvectors of G, i.e. the singular vectors of H_k on the SMALLER array: u_i where that is the UE array,
//      conj(v_i) where it is the BS array (the Gram of the rows h_i is then the conjugate of H^H H).  Here a pair is rotated
//      only where |G_pq| >= 2^-50: below that the squares behind |G_pq| leave the normal float32 range, the phase
//      e = G_pq / |G_pq| loses its unit modulus and would rescale a column of X (the eigenvalues do not care).  The sorting
//      network swaps the columns of X with d; the gauge makes the component of largest modulus (first on ties) of every
//      small-side vector real and positive, its imaginary part exactly +0.  Layer i is present iff
//      gamma_i > max(c_J 2^-24 sum_j gamma_j, 1e-30), c_J = 13 SWEEPS[m] m (m - 1) / 2: below that an eigenvalue cannot be
//      told from the iteration's own rounding; an absent layer is +0.0 in both vectors.  The large-side vector needs a
//      second pass over the tables in LDS (only when it is asked for): the t loop of phase 3 again, two ADJACENT t per trip,
//      h_j[t] recomputed, y_i[t] = sum_j conj(h_j[t]) x_i[j] / sqrt(gamma_i) (w carries sqrt(snr), so no norm pass), the
//      conjugate of that where the BS array is the smaller one.  A lane walks its own output row, 16 bytes per layer and
//      trip; for K < 64 every slice lane writes its own t and nothing is reduced.
// fp32 vector arithmetic, no atomics, every sum in a fixed order that does not depend on where the user sits in the launch.
// LDS of one wave: (m + M_big + kc) * P * 8 bytes, P = min(num_paths, loaded paths) <= 32; rate_lds_bytes has the rule.
// Bound: fp32 VALU issue of phase 3 (M_big * P * (1 + m) complex products per subcarrier), far below HBM.  The Jacobi
// epilogue adds SWEEPS * m (m - 1) / 2 rotations of about 16 (m - 2) + 40 flops per subcarrier (3e4 at m = 8), a few per
// cent of phase 3 by flops unless M_big is tiny; measured on an MI355X it is 24 % at the headline shape (m = 4, M_big = 256),
// the divisions and square roots of a rotation being dependent chains with one wave per SIMD to hide them.
#include "dmx_common.h"
#include "k2_small_body.h"
#include "k7_rate_body.h"
#include <math.h>

namespace dmx {

struct RateArgs {
    int64_t user_begin, user_count;
    int m_big, big_mh, small_mh;
    int small_is_rx;     // the Gram runs over the UE array (M_rx <= M_tx), else over the BS array
    int K, kc;           // selected subcarriers, subcarriers per chunk = w row stride
    int S, log2_S;       // slices of the large array per subcarrier (1 unless K < 64)
    const int32_t* sc;
    double inv_n;
    float scale;         // sqrt(snr / M_tx), or sqrt(snr) for the spectrum
    float inv_k;
    int ld;              // table row stride in path slots (= P)
    NearField nf;        // DMX_FLAG_NEAR_FIELD (array_phase.h)
};

// 2 .. 4  the w chunk, rows_pair of phase 3, epilogue_logdet and the kept-path count: k7_rate_body.h, shared with the other
//          consumers.  The array tables of phase 1 are this file's own statement of fill_array_table's body.

// sweeps of the Jacobi iteration per m (index 0 unused)
constexpr int SWEEPS[9] = {0, 0, 2, 5, 6, 6, 7, 8, 8};

// One cyclic sweep of the complex Jacobi iteration on the upper triangle (G_kp with k > p is conj of the stored G_pk): the
// pair (p, q) is rotated to G_pq = 0 by the phase e of G_pq and the angle of t.  Branch-free: t = 0 where |G_pq| = 0, and
// the NaN of 0 * inf on that path is dropped by the selects.  VEC: the pair is rotated only where |G_pq| >= 2^-50 (else
// t = 0, e = 1), and every row of X[M][M] (vr, vi; not read otherwise) takes the column update of G.
template <int M, bool VEC>
__device__ __forceinline__ void jacobi_sweep(float (&gr)[M * M], float (&gi)[M * M], float* vr, float* vi) {
#pragma unroll
    for (int p = 0; p < M - 1; ++p) {
#pragma unroll
        for (int q = p + 1; q < M; ++q) {
            const float ga = gr[p * M + q], gb = gi[p * M + q];
            const float ag = sqrtf(fmaf(ga, ga, gb * gb));
            const bool nz = VEC ? ag >= 0x1p-50f : ag > 0.f;
            const float inv = 1.f / ag;
            const float er = nz ? ga * inv : 1.f, ei = nz ? gb * inv : 0.f;
            const float dp = gr[p * M + p], dq = gr[q * M + q];
            const float tau = (dq - dp) * (0.5f * inv);
            float t = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(fmaf(tau, tau, 1.f)));
            t = nz ? t : 0.f;
            const float c = 1.f / sqrtf(fmaf(t, t, 1.f)), s = t * c;
            gr[p * M + p] = fmaf(-t, ag, dp);
            gr[q * M + q] = fmaf(t, ag, dq);
            gr[p * M + q] = 0.f; gi[p * M + q] = 0.f;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                if (k == p || k == q) continue;
                const int ip = k < p ? k * M + p : p * M + k, iq = k < q ? k * M + q : q * M + k;
                const float sp = k < p ? 1.f : -1.f, sq = k < q ? 1.f : -1.f;
                const float xr = gr[ip], xi = sp * gi[ip], zr = gr[iq], zi = sq * gi[iq];
                const float yr = fmaf(zr, er, zi * ei), yi = fmaf(zi, er, -(zr * ei));      // y = G_kq conj(e)
                gr[ip] = fmaf(c, xr, -(s * yr)); gi[ip] = sp * fmaf(c, xi, -(s * yi));      // G_kp = c x - s y
                gr[iq] = fmaf(s, xr, c * yr);    gi[iq] = sq * fmaf(s, xi, c * yi);         // G_kq = s x + c y
            }
            if constexpr (VEC) {
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const float ar = vr[k * M + p], ai = vi[k * M + p], zr = vr[k * M + q], zi = vi[k * M + q];
                    const float yr = fmaf(zr, er, zi * ei), yi = fmaf(zi, er, -(zr * ei));  // y = X_kq conj(e)
                    vr[k * M + p] = fmaf(c, ar, -(s * yr)); vi[k * M + p] = fmaf(c, ai, -(s * yi));
                    vr[k * M + q] = fmaf(s, ar, c * yr);    vi[k * M + q] = fmaf(s, ai, c * yi);
                }
            }
        }
    }
}

// 4' eigenvalues of G (mode SNRs: w carries sqrt(snr)) by SWEEPS[M] cyclic Jacobi sweeps, clamped to 0 .. FLT_MAX and sorted
//    descending into d, and the water-filling rate under unit total power from them:
//      rate_k = sum_{i < a} log2(mu d_i),  mu = (1 + sum_{i < a} 1 / d_i) / a,  a the largest count with mu > 1 / d_{a-1}
//    Modes <= 1e-30 take no power (1 / d stays finite); mu d_i is >= 1 in exact arithmetic and clamped to 1 .. FLT_MAX.
template <int M>
__device__ __forceinline__ float epilogue_spectrum(float (&gr)[M * M], float (&gi)[M * M], float (&d)[M]) {
#pragma unroll 1
    for (int sw = 0; sw < SWEEPS[M]; ++sw) jacobi_sweep<M, false>(gr, gi, nullptr, nullptr);
#pragma unroll
    for (int i = 0; i < M; ++i) d[i] = fminf(fmaxf(gr[i * M + i], 0.f), 3.402823466e38f);
#pragma unroll
    for (int r = 0; r < M; ++r) {                                            // odd-even transposition network
#pragma unroll
        for (int i = r & 1; i + 1 < M; i += 2) {
            const float hi = fmaxf(d[i], d[i + 1]), lo = fminf(d[i], d[i + 1]);
            d[i] = hi; d[i + 1] = lo;
        }
    }
    float sinv = 0.f, mu = 1.f;
    int cnt = 0;
    bool alive = true;
#pragma unroll
    for (int a = 1; a <= M; ++a) {
        const float g = d[a - 1];
        const bool pos = g > 1e-30f;
        const float inv = 1.f / (pos ? g : 1.f);
        const float sa = sinv + inv, mua = (1.f + sa) / (float)a;
        alive = alive && pos && mua > inv;
        sinv = alive ? sa : sinv; mu = alive ? mua : mu; cnt += alive ? 1 : 0;
    }
    float rk = 0.f;
#pragma unroll
    for (int i = 0; i < M; ++i) rk += i < cnt ? log2f(fminf(fmaxf(mu * d[i], 1.f), 3.402823466e38f)) : 0.f;
    return rk;
}

// 4" eigenvalues as in 4' (d, descending) with the eigenvectors of G in the columns of X (xr, xi), sorted with d: the small-side
//    singular vectors of H_k, x_i or (cs = -1: the BS array is the smaller one) its conjugate, in the gauge of the header
template <int M>
__device__ __forceinline__ void epilogue_vectors(float (&gr)[M * M], float (&gi)[M * M], float (&d)[M], float (&xr)[M * M],
                                                 float (&xi)[M * M], const float cs) {
#pragma unroll
    for (int i = 0; i < M * M; ++i) { xr[i] = i / M == i % M ? 1.f : 0.f; xi[i] = 0.f; }
#pragma unroll 1
    for (int sw = 0; sw < SWEEPS[M]; ++sw) jacobi_sweep<M, true>(gr, gi, xr, xi);
#pragma unroll
    for (int i = 0; i < M; ++i) d[i] = fminf(fmaxf(gr[i * M + i], 0.f), 3.402823466e38f);
#pragma unroll
    for (int r = 0; r < M; ++r) {                                            // odd-even transposition network, columns with d
#pragma unroll
        for (int i = r & 1; i + 1 < M; i += 2) {
            const bool sw = d[i + 1] > d[i];
            const float hi = fmaxf(d[i], d[i + 1]), lo = fminf(d[i], d[i + 1]);
            d[i] = hi; d[i + 1] = lo;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const float ar = xr[k * M + i], ai = xi[k * M + i], br = xr[k * M + i + 1], bi = xi[k * M + i + 1];
                xr[k * M + i] = sw ? br : ar; xi[k * M + i] = sw ? bi : ai;
                xr[k * M + i + 1] = sw ? ar : br; xi[k * M + i + 1] = sw ? ai : bi;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {                                            // the gauge, column by column
        float best = -1.f, br = 1.f, bi = 0.f;
        int jb = 0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const float re = xr[j * M + i], im = cs * xi[j * M + i];
            xi[j * M + i] = im;
            const float a2 = fmaf(re, re, im * im);
            const bool up = a2 > best;                                       // strictly: the first of equal moduli
            best = up ? a2 : best; br = up ? re : br; bi = up ? im : bi; jb = up ? j : jb;
        }
        const float ab = sqrtf(best), inv = 1.f / ab, pr = br * inv, pi = bi * inv;
#pragma unroll
        for (int j = 0; j < M; ++j) {                                        // x_j conj(p), the pivot component (|x|, +0) itself
            const float re = xr[j * M + i], im = xi[j * M + i];
            xr[j * M + i] = j == jb ? ab : fmaf(re, pr, im * pi);
            xi[j * M + i] = j == jb ? 0.f : fmaf(im, pr, -(re * pi));
        }
    }
}

enum { EPI_LOGDET = 0, EPI_SPECTRUM = 1, EPI_VECTORS = 2 };

// outputs of EPI_VECTORS: the small-side vectors [user_count, K, L, m], the large-side ones [user_count, K, L, M_big], each
// may be NULL; vec16: rows of `big` take 16-byte stores (M_big even, the base 16-byte aligned)
struct VecOut {
    float2* small_side;
    float2* big;
    int L, vec16;
};

// EPI_LOGDET: out_rate is written, out_rate_k may be NULL, out_gamma is not used.  EPI_SPECTRUM: each output may be NULL.
// EPI_VECTORS: out_gamma and the two of `vo`, each may be NULL; no rate.
template <int M, int EPI>
__global__ __launch_bounds__(256) void k7_rate(WsView ws, RateArgs a, float* __restrict__ out_rate, float* __restrict__ out_rate_k,
                                               float* __restrict__ out_gamma, VecOut vo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                          // waves never talk to each other
    const int ld = a.ld, Mb = a.m_big, K = a.K, kc = a.kc, S = a.S;
    const size_t per_wave = (size_t)(M + Mb + kc) * ld;
    float2* as = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * per_wave;     // [M][ld]
    float2* ab = as + (size_t)M * ld;                                                // [Mb][ld]
    float2* w = ab + (size_t)Mb * ld;                                                // [ld][kc]
    const int64_t u = a.user_begin + ul;
    float* ok = out_rate_k ? out_rate_k + (size_t)ul * K : nullptr;
    float* og = EPI != EPI_LOGDET && out_gamma ? out_gamma + (size_t)ul * K * M : nullptr;     // [K][M]
    const int L = vo.L;
    float2* os = EPI == EPI_VECTORS && vo.small_side ? vo.small_side + (size_t)ul * K * L * M : nullptr;   // [K][L][M]
    float2* ob = EPI == EPI_VECTORS && vo.big ? vo.big + (size_t)ul * K * L * Mb : nullptr;                // [K][L][Mb]
    const int n = kept_paths(ws, u);
    if (n <= 0) {                                                            // no kept path: +0.0 everywhere
        if (ok) for (int i = lane; i < K; i += 64) ok[i] = 0.f;
        if (og) for (int i = lane; i < K * M; i += 64) og[i] = 0.f;
        if (os) for (size_t i = lane; i < (size_t)K * L * M; i += 64) os[i] = make_float2(0.f, 0.f);
        if (ob) for (size_t i = lane; i < (size_t)K * L * Mb; i += 64) ob[i] = make_float2(0.f, 0.f);
        if (lane == 0 && out_rate) out_rate[ul] = 0.f;
        return;
    }
    const WsRecords rec{ws, (size_t)u * ws.P};

    // 1  array tables
    for (int i = lane; i < M * n; i += 64) {
        const int t = i / n, l = i - t * n;
        const double sy = a.small_is_rx ? rec.rx_y(l) : rec.tx_y(l), sz = a.small_is_rx ? rec.rx_z(l) : rec.tx_z(l);
        float s, c;
        if (a.nf.on) near_field_sincos(t % a.small_mh, t / a.small_mh, sy, sz, rec.dn(l), a.nf.end(a.small_is_rx), s, c);
        else
            sincos_rev(frac_rev(__builtin_fma((double)(t % a.small_mh), sy, (double)(t / a.small_mh) * sz)), s, c);
        as[t * ld + l] = make_float2(c, s);
    }
    for (int i = lane; i < Mb * n; i += 64) {
        const int t = i / n, l = i - t * n;
        const double sy = a.small_is_rx ? rec.tx_y(l) : rec.rx_y(l), sz = a.small_is_rx ? rec.tx_z(l) : rec.rx_z(l);
        float s, c;
        if (a.nf.on) near_field_sincos(t % a.big_mh, t / a.big_mh, sy, sz, rec.dn(l), a.nf.end(!a.small_is_rx), s, c);
        else
            sincos_rev(frac_rev(__builtin_fma((double)(t % a.big_mh), sy, (double)(t / a.big_mh) * sz)), s, c);
        ab[t * ld + l] = make_float2(c, s);
    }

    const int kl = lane >> a.log2_S, sl = lane & (S - 1);                    // this lane's subcarrier of the chunk and slice
    float rate_sum = 0.f;
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc;
        // 2  w of the chunk
        wave_lds_fence();                                                    // the last chunk's reads before this chunk's writes
        fill_w_chunk(w, rec, a.sc, k0, a.inv_n, a.scale, n, kn, kc, lane);
        wave_lds_fence();

        // 3  this lane's share of the upper triangle of G
        float gr[M * M], gi[M * M];
#pragma unroll
        for (int i = 0; i < M * M; ++i) gr[i] = gi[i] = 0.f;
        const bool active = kl < kn;
        if (active) {
            const float2* wk = w + kl;
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

        // 4  the epilogue on the upper triangle: log2 det(I + G), or the eigenvalues of G and the water-filling rate
        float lg;
        if constexpr (EPI == EPI_LOGDET) {
            lg = epilogue_logdet<M>(gr, gi);
        } else if constexpr (EPI == EPI_VECTORS) {
            float d[M], xr[M * M], xi[M * M], isg[M];
            epilogue_vectors<M>(gr, gi, d, xr, xi, a.small_is_rx ? 1.f : -1.f);
            lg = 0.f;
            constexpr float CJ_U24 = (float)(13 * SWEEPS[M] * (M * (M - 1) / 2)) * 0x1p-24f;
            float tot = 0.f;
#pragma unroll
            for (int i = 0; i < M; ++i) tot += d[i];
            const float floor_g = fmaxf(CJ_U24 * tot, 1e-30f);
#pragma unroll
            for (int i = 0; i < M; ++i) {                                    // an absent layer: +0.0 in both vectors
                const bool present = d[i] > floor_g;
                isg[i] = present ? 1.f / sqrtf(d[i]) : 0.f;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    xr[j * M + i] = present ? xr[j * M + i] : 0.f;
                    xi[j * M + i] = present ? xi[j * M + i] : 0.f;
                }
            }
            if (active && sl == 0) {
                if (og) {
#pragma unroll
                    for (int i = 0; i < M; ++i) og[(size_t)(k0 + kl) * M + i] = d[i];
                }
                if (os) {                                                    // L * M consecutive complex values per lane
                    float2* row = os + (size_t)(k0 + kl) * L * M;
#pragma unroll
                    for (int i = 0; i < M; ++i) {
                        if (i < L) {
#pragma unroll
                            for (int j = 0; j < M; ++j) row[i * M + j] = make_float2(xr[j * M + i], xi[j * M + i]);
                        }
                    }
                }
            }
            if (ob && active) {
                // the second pass: y_i[t] = sum_j conj(h_j[t]) x_i[j] / sqrt(gamma_i) with the stored small-side vector x_i, h
                // itself where the BS array is the smaller one; this slice's t in adjacent pairs
                const float hs = a.small_is_rx ? -1.f : 1.f;
                const float2* wk = w + kl;
                float2* rows = ob + (size_t)(k0 + kl) * L * Mb;
                for (int t = 2 * sl; t < Mb; t += 2 * S) {
                    const bool two = t + 1 < Mb;
                    const float2* b0 = ab + (size_t)t * ld;
                    const float2* b1 = ab + (size_t)(two ? t + 1 : t) * ld;
                    float2 h0[M], h1[M];
                    rows_pair<M>(as, b0, b1, wk, ld, kc, n, h0, h1);
#pragma unroll
                    for (int i = 0; i < M; ++i) {
                        if (i < L) {
                            float2 y0 = make_float2(0.f, 0.f), y1 = y0;
#pragma unroll
                            for (int j = 0; j < M; ++j) {
                                const float sr = xr[j * M + i], si = xi[j * M + i];
                                const float i0 = hs * h0[j].y, i1 = hs * h1[j].y;
                                y0.x = fmaf(h0[j].x, sr, fmaf(-i0, si, y0.x));
                                y0.y = fmaf(h0[j].x, si, fmaf(i0, sr, y0.y));
                                y1.x = fmaf(h1[j].x, sr, fmaf(-i1, si, y1.x));
                                y1.y = fmaf(h1[j].x, si, fmaf(i1, sr, y1.y));
                            }
                            const bool present = isg[i] > 0.f;
                            y0.x = present ? y0.x * isg[i] : 0.f; y0.y = present ? y0.y * isg[i] : 0.f;
                            y1.x = present ? y1.x * isg[i] : 0.f; y1.y = present ? y1.y * isg[i] : 0.f;
                            float2* dst = rows + (size_t)i * Mb + t;
                            if (two && vo.vec16) {
                                *reinterpret_cast<float4*>(dst) = make_float4(y0.x, y0.y, y1.x, y1.y);
                            } else {
                                dst[0] = y0;
                                if (two) dst[1] = y1;
                            }
                        }
                    }
                }
            }
        } else {
            float d[M];
            lg = epilogue_spectrum<M>(gr, gi, d);
            if (og && active && sl == 0) {                                   // M consecutive floats per lane, lanes in k order
#pragma unroll
                for (int i = 0; i < M; ++i) og[(size_t)(k0 + kl) * M + i] = d[i];
            }
        }
        if (active && sl == 0) {
            if (ok) ok[k0 + kl] = lg;
            rate_sum += lg;
        }
    }
    for (int d = 1; d < 64; d <<= 1) rate_sum += __shfl_xor(rate_sum, d, 64);
    if (lane == 0 && out_rate) out_rate[ul] = rate_sum * a.inv_k;
}

// LDS bytes of one wave for P path slots (0: the shape is not taken): both array tables and one chunk of w,
//   (m + M_big + kc) * P * 8,   m = min(M_rx, M_tx) <= 8,  M_big = max(M_rx, M_tx),  kc = min(n_selected, 64)
// lds_waves_per_block turns that into 4 / 2 / 1 waves per workgroup (16 KB / 32 KB / 156 KB per wave).
size_t rate_lds_bytes(const dmx_params& prm, int P) {
    if (P < 1 || P > 32 || prm.n_selected < 1) return 0;
    const size_t m_tx = (size_t)prm.bs_shape[0] * prm.bs_shape[1], m_rx = (size_t)prm.ue_shape[0] * prm.ue_shape[1];
    const size_t m = m_rx <= m_tx ? m_rx : m_tx, big = m_rx <= m_tx ? m_tx : m_rx;
    if (m > 8) return 0;
    const size_t kc = prm.n_selected < 64 ? prm.n_selected : 64;
    return (m + big + kc) * (size_t)P * sizeof(float2);
}

int rate_waves_per_block(const dmx_params& prm, int P) { return lds_waves_per_block(rate_lds_bytes(prm, P)); }

template <int M, int EPI>
static int launch_rate_m(const dim3 g, const dim3 b, size_t smem, hipStream_t stream, const WsView& ws, const RateArgs& a,
                         float* out_rate, float* out_rate_k, float* out_gamma, const VecOut& vo) {
    return launch_dyn_lds(k7_rate<M, EPI>, EPI == EPI_LOGDET ? "k7_rate" : EPI == EPI_SPECTRUM ? "k7_rate (spectrum)" : "k7_rate (vectors)",
                          g, b, smem, WAVE_LDS_MAX, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
}

// scale: what the path coefficients are multiplied by, sqrt(snr / M_tx) for the determinant and sqrt(snr) for the spectrum
template <int EPI>
static int launch_rate_epi(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, float scale,
                           float* out_rate, float* out_rate_k, float* out_gamma, hipStream_t stream,
                           const VecOut& vo = VecOut{nullptr, nullptr, 0, 0}) {
    const int wpb = rate_waves_per_block(prm, ws.P);
    if (!wpb) { set_error("rate kernel: tables of one user do not fit the LDS"); return DMX_ERR_SHAPE; }
    const int m_tx = prm.bs_shape[0] * prm.bs_shape[1], m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    const bool rx_small = m_rx <= m_tx;
    const int m = rx_small ? m_rx : m_tx;
    RateArgs a;
    a.user_begin = user_begin; a.user_count = user_count;
    a.m_big = rx_small ? m_tx : m_rx;
    a.big_mh = rx_small ? prm.bs_shape[0] : prm.ue_shape[0];
    a.small_mh = rx_small ? prm.ue_shape[0] : prm.bs_shape[0];
    a.nf = near_field_of(prm);
    a.small_is_rx = rx_small ? 1 : 0;
    a.K = prm.n_selected; a.kc = a.K < 64 ? a.K : 64;
    a.log2_S = gram_slices_log2(a.K, a.m_big);
    a.S = 1 << a.log2_S;
    a.sc = prm.selected_subcarriers;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.scale = scale;
    a.inv_k = (float)(1.0 / (double)a.K);
    a.ld = ws.P;
    const size_t smem = (size_t)wpb * rate_lds_bytes(prm, ws.P);
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), b(64 * wpb);    // flat: one wave per user
    switch (m) {
        case 1: return launch_rate_m<1, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 2: return launch_rate_m<2, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 3: return launch_rate_m<3, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 4: return launch_rate_m<4, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 5: return launch_rate_m<5, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 6: return launch_rate_m<6, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        case 7: return launch_rate_m<7, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
        default: return launch_rate_m<8, EPI>(g, b, smem, stream, ws, a, out_rate, out_rate_k, out_gamma, vo);
    }
}

int launch_rate(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                float* out_rate, float* out_rate_k, hipStream_t stream) {
    const int m_tx = prm.bs_shape[0] * prm.bs_shape[1];
    return launch_rate_epi<EPI_LOGDET>(prm, ws, user_begin, user_count, (float)sqrt(snr_linear / (double)m_tx), out_rate,
                                       out_rate_k, nullptr, stream);
}

int launch_spectrum(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                    float* out_gamma, float* out_rate, float* out_rate_k, hipStream_t stream) {
    return launch_rate_epi<EPI_SPECTRUM>(prm, ws, user_begin, user_count, (float)sqrt(snr_linear), out_rate, out_rate_k,
                                         out_gamma, stream);
}

// out_tx [user_count, K, L, M_tx], out_rx [user_count, K, L, M_rx]: the small-side one comes from the rotations, the other
// from the second pass
int launch_precoders(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                     int n_layers, float* out_gamma, float2* out_tx, float2* out_rx, hipStream_t stream) {
    const int m_tx = prm.bs_shape[0] * prm.bs_shape[1], m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    const bool rx_small = m_rx <= m_tx;
    VecOut vo;
    vo.small_side = rx_small ? out_rx : out_tx;
    vo.big = rx_small ? out_tx : out_rx;
    vo.L = n_layers;
    vo.vec16 = (rx_small ? m_tx : m_rx) % 2 == 0 && ((uintptr_t)vo.big & 15u) == 0;
    return launch_rate_epi<EPI_VECTORS>(prm, ws, user_begin, user_count, (float)sqrt(snr_linear), nullptr, nullptr, out_gamma,
                                        stream, vo);
}

}  // namespace dmx
