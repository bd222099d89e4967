// Bodies the rate kernels share: k7_rate.hip (one link, white noise) and k8_cell_rate.hip (several links, the other cells'
// signals as coloured noise) run the same products and the same elimination on one wave's LDS tables, so that a single link
// gives the same bits through either kernel.
//   rows_pair         3  h_i[t] of two large-array elements for a lane's subcarrier
//   epilogue_logdet   4  log2 det(I + G) from the pivots of an elimination on the upper triangle
// Tables of one wave (k7_rate.hip has the layout): as [M][ld] the Gram side, ab [Mb][ld] the other array, w [ld][kc]
// path-major.  fp32, every sum in the order written here.
#pragma once
#include <hip/hip_runtime.h>

namespace dmx {

// 4  pivots of I + G by elimination on the upper triangle, each clamped to >= 1: log2 det(I + G)
template <int M>
__device__ __forceinline__ float epilogue_logdet(float (&gr)[M * M], float (&gi)[M * M]) {
    float lg = 0.f;
#pragma unroll
    for (int p = 0; p < M; ++p) {
        const float d = fmaxf(gr[p * M + p] + (p == 0 ? 1.f : 0.f), 1.f);
        lg += log2f(d);
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
