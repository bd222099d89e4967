// Bodies the one-wave-per-user consumers of the path records share: k7_rate.hip, k8_cell_rate.hip, k9_angle_delay.hip and
// k10_codebook_rate.hip run the same table fills, products and elimination on one wave's LDS tables,
// so that one link gives the same bits through k7_rate and k8_cell_rate, and a single subband the bits of the wideband
// codebook rate.  By phase, as the kernels' headers number them (k7_rate.hip's numbers; where another kernel's differ
// they follow in brackets):
//   kept_paths        0  the user's kept-path count, wave-uniform, at most P
//   fill_array_table  1  rows of an array's steering table, a[t][l] = exp(j 2pi ((t % mh) y_l + (t / mh) z_l))   [k9: 1, 2']
//                        (k8, k9, k10; k7_rate.hip keeps its own two loops of the same expression)
//   fill_w_chunk      2  a chunk of w[l][k] = scale c_l exp(-j 2pi dn_l sc_k / N), path-major
//   copy_rows_to_lds  -  a chunk of rows of k2b_beam_project's row table, HBM to LDS                              [k9: 2', k10: 3]
//   rows_pair         3  h_i[t] of two large-array elements for a lane's subcarrier                               [k10: 4]
//   epilogue_logdet   4  log2 det(I + G) from the pivots of an elimination on the upper triangle
// Host: gram_slices_log2, the slice rule of phase 3.
// Tables of one wave (k7_rate.hip has the layout): as [M][ld] the Gram side, ab [Mb][ld] the other array, w [ld][kc]
// path-major.  fp32, every sum in the order written here.  The callers fence the wave's LDS (wave_lds_fence) between a
// fill and the reads of it; nothing here does.
#pragma once
#include "dmx_common.h"
#include "array_phase.h"
#include "k2_small_body.h"
#include <hip/hip_runtime.h>

namespace dmx {

// 3  log2 of the slices of the large array per subcarrier: the largest power of two S with K S <= 64 and S <= M_big
__host__ inline int gram_slices_log2(const int K, const int m_big) {
    int log2_S = 0;
    while (K * (2 << log2_S) <= 64 && (2 << log2_S) <= m_big) ++log2_S;
    return log2_S;
}

// 0  kept paths of user u: one scalar for the wave, at most the P slots of a record row
__device__ __forceinline__ int kept_paths(const WsView& ws, const int64_t u) {
    const int n = __builtin_amdgcn_readfirstlane(ws.n_keep[u]);
    return n < ws.P ? n : ws.P;
}

// 1  rows row0 .. row0 + rows of the steering table of the UE (rx) or the BS array, first panel dimension mh, for the first
//    n paths: tab[t][l], t from 0.  float64 phase - the plane wave, or with rec.nf.on the spherical one of array_phase.h -
//    reduced to a revolution before the float32 sincos.
__device__ __forceinline__ void fill_array_table(float2* tab, const WsRecords& rec, const bool rx, const int row0, const int rows,
                                                 const int mh, const int n, const int ld, const int lane) {
    const NearFieldEnd nf = rec.nf.end(rx);
    for (int i = lane; i < rows * n; i += 64) {
        const int t = i / n, l = i - t * n, e = row0 + t;
        const double sy = rx ? rec.rx_y(l) : rec.tx_y(l), sz = rx ? rec.rx_z(l) : rec.tx_z(l);
        float s, c;
        if (nf.on) near_field_sincos(e % mh, e / mh, sy, sz, rec.dn(l), nf, s, c);
        else
            sincos_rev(frac_rev(__builtin_fma((double)(e % mh), sy, (double)(e / mh) * sz)), s, c);
        tab[t * ld + l] = make_float2(c, s);
    }
}

// 2  w[l][k] = scale c_l exp(-j 2pi dn_l sc[k0 + k] / N) for the first n paths and the kn subcarriers from position k0, row
//    stride kc
__device__ __forceinline__ void fill_w_chunk(float2* w, const WsRecords& rec, const int32_t* sc, const int k0, const double inv_n,
                                             const float scale, const int n, const int kn, const int kc, const int lane) {
    for (int i = lane; i < n * kn; i += 64) {
        const int l = i / kn, k = i - l * kn;
        float s, c;
        // the fractional part of the EXACT product x * k (k2_small_body.h)
        const double x = (double)rec.dn(l) * inv_n, kd = (double)sc[k0 + k];
        sincos_rev((float)__builtin_fma(x, kd, -rint(x * kd)), s, c);
        const float cr = rec.c_re(l) * scale, ci = rec.c_im(l) * scale;
        w[l * kc + k] = make_float2(fmaf(cr, c, ci * s), fmaf(ci, c, -(cr * s)));     // c_l (cos - j sin)
    }
}

// cnt values from src + off to dst, one contiguous block on both sides; by 16 bytes where the offset is even (src is 16-byte
// aligned)
__device__ __forceinline__ void copy_rows_to_lds(float2* dst, const float2* src, const size_t off, const int cnt, const int lane) {
    src += off;
    if ((off & 1) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (int i = lane; i < cnt / 2; i += 64) {
            const float4 v = s4[i];
            dst[2 * i] = make_float2(v.x, v.y); dst[2 * i + 1] = make_float2(v.z, v.w);
        }
        if ((cnt & 1) && lane == 0) dst[cnt - 1] = src[cnt - 1];
    } else {
        for (int i = lane; i < cnt; i += 64) dst[i] = src[i];
    }
}

// 4  pivots of I + G by elimination on the upper triangle, each clamped to >= 1: log2 det(I + G).  LAST: log2 of the last
//    pivot alone, the Schur complement of I + G at its last row and column
template <int M, bool LAST = false>
__device__ __forceinline__ float epilogue_logdet(float (&gr)[M * M], float (&gi)[M * M]) {
    float lg = 0.f;
#pragma unroll
    for (int p = 0; p < M; ++p) {
        const float d = fmaxf(gr[p * M + p] + (p == 0 ? 1.f : 0.f), 1.f);
        if (!LAST || p == M - 1) lg += log2f(d);
        const float inv = 1.f / d;
#pragma unroll
        for (int i = p + 1; i < M; ++i) {
            const float er = gr[p * M + i] * inv, ei = -gi[p * M + i] * inv;         // conj(A_pi) / d
#pragma unroll
            for (int j = i; j < M; ++j) {
                const float xr = gr[p * M + j], xi = gi[p * M + j];
                gr[i * M + j] -= fmaf(er, xr, -(ei * xi));
                if (j > i) gi[i * M + j] -= fmaf(er, xi, ei * xr);
            }
            if (p == 0) gr[i * M + i] += 1.f;                            // the identity, once per diagonal entry
        }
    }
    return lg;
}

// 4' the linear MMSE receiver on the same Gram (upper triangle, as epilogue_logdet takes it): sum over the layers t of
//    log2(1 + sinr_t), 1 + sinr_t = 1 / [(I + G)^-1]_tt, which is the Schur complement of I + G at layer t: the last pivot
//    of the elimination above run with the rows and columns t and M - 1 exchanged, on a register copy.  No difference of
//    two logarithms, and with every pivot clamped to >= 1 no term below zero.
template <int M>
__device__ __forceinline__ float epilogue_mmse(const float (&gr)[M * M], const float (&gi)[M * M]) {
    float lg = 0.f;
#pragma unroll
    for (int t = 0; t < M; ++t) {
        float ar[M * M], ai[M * M];
#pragma unroll
        for (int p = 0; p < M; ++p) {
#pragma unroll
            for (int q = 0; q < M; ++q) {
                const int a = p == t ? M - 1 : (p == M - 1 ? t : p), b = q == t ? M - 1 : (q == M - 1 ? t : q);
                const bool up = a <= b;                                  // below the diagonal of G: the conjugate
                ar[p * M + q] = q < p ? 0.f : (up ? gr[a * M + b] : gr[b * M + a]);
                ai[p * M + q] = q <= p ? 0.f : (up ? gi[a * M + b] : -gi[b * M + a]);
            }
        }
        lg += epilogue_logdet<M, true>(ar, ai);
    }
    return lg;
}

// h_i[t] of the two large-array elements whose table rows are b0 and b1, for this lane's subcarrier (wk = w + k)
template <int M>
__device__ __forceinline__ void rows_pair(const float2* as, const float2* b0, const float2* b1, const float2* wk, const int ld,
                                          const int kc, const int n, float2 (&h0)[M], float2 (&h1)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) h0[i] = h1[i] = make_float2(0.f, 0.f);
#pragma unroll 2
    for (int l = 0; l < n; ++l) {
        const float2 x = wk[l * kc], p0 = b0[l], p1 = b1[l];
        const float2 q0 = make_float2(fmaf(x.x, p0.x, -(x.y * p0.y)), fmaf(x.x, p0.y, x.y * p0.x));
        const float2 q1 = make_float2(fmaf(x.x, p1.x, -(x.y * p1.y)), fmaf(x.x, p1.y, x.y * p1.x));
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float2 v = as[i * ld + l];
            h0[i].x = fmaf(v.x, q0.x, fmaf(-v.y, q0.y, h0[i].x));
            h0[i].y = fmaf(v.x, q0.y, fmaf(v.y, q0.x, h0[i].y));
            h1[i].x = fmaf(v.x, q1.x, fmaf(-v.y, q1.y, h1[i].x));
            h1[i].y = fmaf(v.x, q1.y, fmaf(v.y, q1.x, h1[i].y));
        }
    }
}

}  // namespace dmx
