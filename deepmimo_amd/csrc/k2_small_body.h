// One user's tables and output block of the small-output kernels: k2_fd_small (k2_channel_fd_small.hip, records from the
// HBM workspace) and the single-pass kernel k12_fd_direct (k12_fd_direct.hip, records the same wave has just put into
// LDS) call this one body, so their bits agree by construction (tests/test_gpu_fd_direct.py holds torch.equal).
//   tables   b_rx[rx][l] = c_l * a_rx[rx,l],  a_tx[tx][l],  g[l][k] = exp(-j 2pi dn_l sc_k / N)   in the wave's LDS slice
//   outputs  lane = (antenna pair p, chunk of KC subcarriers): w_l = b_rx[rx][l] * a_tx[tx][l] once per path,
//            KC complex FMAs with it; lanes walk the user's block linearly -> coalesced stores.
// The two including files are compiled with different -ffp-contract settings, so nothing here is left to contraction:
// the body switches it off and every fused operation is an explicit fma ("Bit identity", has the forms).
#pragma once
#include "dmx_common.h"
#include "array_phase.h"

namespace dmx {

struct SmallArgs {
    int64_t user_begin, user_count;
    int m_rx, m_tx, ue_mh, bs_mh;
    int K;
    const int32_t* sc;
    double inv_n;
    int ld;          // table row stride in path slots
};
__host__ inline SmallArgs small_args(const dmx_params& prm, int64_t user_begin, int64_t user_count, int ld) {
    SmallArgs a;
    a.user_begin = user_begin; a.user_count = user_count;
    a.m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    a.m_tx = prm.bs_shape[0] * prm.bs_shape[1];
    a.ue_mh = prm.ue_shape[0];
    a.bs_mh = prm.bs_shape[0];
    a.K = prm.n_selected;
    a.sc = prm.selected_subcarriers;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.ld = ld;
    return a;
}
// bytes of one wave's three tables
__host__ inline size_t small_table_bytes(const dmx_params& prm, int ld) {
    return ((size_t)prm.ue_shape[0] * prm.ue_shape[1] + (size_t)prm.bs_shape[0] * prm.bs_shape[1] + (size_t)prm.n_selected) * ld * sizeof(float2);
}

// a user's compacted records in the HBM workspace; the LDS counterpart is LdsRecords (k12_fd_direct.hip)
struct WsRecords {
    const WsView& ws;
    size_t rb;                                                               // first record of the user's row
    NearField nf{};                                                          // how the array phases of these records are read
                                                                             // (array_phase.h): off unless the kernel sets it
    __device__ float c_re(int l) const { return ws.c_re[rb + l]; }
    __device__ float c_im(int l) const { return ws.c_im[rb + l]; }
    __device__ float dn(int l) const { return ws.dn[rb + l]; }
    __device__ double tx_y(int l) const { return ws.tx_y[rb + l]; }
    __device__ double tx_z(int l) const { return ws.tx_z[rb + l]; }
    __device__ double rx_y(int l) const { return ws.rx_y[rb + l]; }
    __device__ double rx_z(int l) const { return ws.rx_z[rb + l]; }
};

// Tables brx [m_rx][ld], atx [m_tx][ld], g [ld][K] of this wave from the first n_act records of `rec`, then the user's
// block o [m_rx * m_tx][K].  The first fence orders what the wave did in LDS before (the previous user's table reads,
// the record writes) against the table writes.  UL = paths per trip of the output loop's sum, which the unroller would
// otherwise pick by the size of the surrounding kernel: each kernel names what it was measured with.
template <int KC, int UL, class Rec>
__device__ __forceinline__ void small_user_block(const SmallArgs& a, const Rec& rec, int n_act, const int lane, float2* brx,
                                                 float2* atx, float2* g, float2* o) {
#pragma clang fp contract(off)
    const int ld = a.ld, K = a.K, M = a.m_rx * a.m_tx;
    n_act = n_act < ld ? n_act : ld;
    if (n_act == 0) {                                                       // channel.py:270-271
        for (int i = lane; i < M * K; i += 64) o[i] = make_float2(0.f, 0.f);
        return;
    }
    wave_lds_fence();
    for (int i = lane; i < a.m_rx * n_act; i += 64) {
        const int r = i / n_act, l = i - r * n_act;
        float s, c;
        const double t = __builtin_fma((double)(r % a.ue_mh), rec.rx_y(l), (double)(r / a.ue_mh) * rec.rx_z(l));
        sincos_rev((float)(t - rint(t)), s, c);
        const float cr = rec.c_re(l), ci = rec.c_im(l);
        brx[r * ld + l] = make_float2(fmaf(cr, c, -(ci * s)), fmaf(cr, s, ci * c));
    }
    for (int i = lane; i < a.m_tx * n_act; i += 64) {
        const int t = i / n_act, l = i - t * n_act;
        float s, c;
        const double x = __builtin_fma((double)(t % a.bs_mh), rec.tx_y(l), (double)(t / a.bs_mh) * rec.tx_z(l));
        sincos_rev((float)(x - rint(x)), s, c);
        atx[t * ld + l] = make_float2(c, s);
    }
    for (int i = lane; i < n_act * K; i += 64) {
        const int l = i / K, k = i - l * K;
        float s, c;
        // the fractional part of the EXACT product x * k, which matters once dn / N * k needs more than 53 bits (|k|
        // towards 2^31)
        const double x = (double)rec.dn(l) * a.inv_n, kd = (double)a.sc[k];
        sincos_rev((float)__builtin_fma(x, kd, -rint(x * kd)), s, c);
        g[l * K + k] = make_float2(c, -s);                                  // exp(-j 2pi x) = cos - j sin
    }
    wave_lds_fence();

    const int nchunk = (K + KC - 1) / KC;
    const int total = M * nchunk;
    for (int e = lane; e < total; e += 64) {
        const int p = e / nchunk, k0 = (e - p * nchunk) * KC;
        const int rx = p / a.m_tx, tx = p - rx * a.m_tx;
        const float2* br = brx + rx * ld;
        const float2* at = atx + tx * ld;
        int kj[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) kj[j] = (k0 + j) < K ? (k0 + j) : (K - 1);
        float2 acc[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) acc[j] = make_float2(0.f, 0.f);
#pragma unroll UL
        for (int l = 0; l < n_act; ++l) {
            const float2 b = br[l], t = at[l];
            const float wr = b.x * t.x - b.y * t.y, wi = b.x * t.y + b.y * t.x;      // four rounded products
            const float nwi = -wi;                                                   // the sign once per path, not per product
            const float2* gl = g + l * K;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const float2 v = gl[kj[j]];
                acc[j].x += fmaf(wr, v.x, nwi * v.y);
                acc[j].y += fmaf(wr, v.y, wi * v.x);
            }
        }
        float2* dst = o + (size_t)p * K + k0;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (k0 + j < K) dst[j] = acc[j];
    }
}

}  // namespace dmx
