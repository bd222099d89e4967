// Stage 2, frequency domain - small-output kernel (variant 9): one WAVE per user, no workgroup barrier.
//
// DeepMIMO's default selects ONE subcarrier (channel.py:57) and dataset-building scripts rarely take more than a
// few dozen, so a user's block [M_rx, M_tx, K] is often a few KB.  The matrix-core kernel spends ~5 us of fixed
// latency per user in that regime (A' tiles through LDS, three workgroup barriers, 1024 threads for 64 outputs), the
// fp32 vector kernel puts one subcarrier on a lane and leaves 63 lanes idle at K = 1.  Here a wave owns a user:
//   tables   b_rx[rx][l] = c_l * a_rx[rx,l],  a_tx[tx][l],  g[l][k] = exp(-j 2pi dn_l sc_k / N)   in the wave's LDS slice
//            ((M_rx + M_tx + K) * L sin/cos per user instead of M_rx * M_tx * L + L * K)
//   outputs  lane = (antenna pair p, chunk of KC subcarriers): w_l = b_rx[rx][l] * a_tx[tx][l] once per path,
//            KC complex FMAs with it; lanes walk the user's block linearly -> coalesced stores.
// Waves of a workgroup never talk to each other; LDS traffic of one wave is ordered by the hardware, the fences only
// stop the compiler from moving reads over writes.  fp32 arithmetic with the float64 phase reduction of the other
// kernels (dataset.py:398-417 + channel.py:264-284; same record layout, first 32 kept paths, the rest through
// launch_extra_path_passes).  Bound: VALU / LDS issue (tables), far below HBM: the regime is latency, not bandwidth.
#include "dmx_common.h"
#include "k2_small_body.h"

namespace dmx {

// the tables and the output loop are small_user_block (k2_small_body.h), shared with the single-pass kernel
template <int KC>
__global__ __launch_bounds__(256) void k2_fd_small(WsView ws, SmallArgs a, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int per_wave = (a.m_rx + a.m_tx + a.K) * a.ld;
    float2* brx = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * per_wave;   // [m_rx][ld]
    float2* atx = brx + (size_t)a.m_rx * a.ld;                                      // [m_tx][ld]
    float2* g = atx + (size_t)a.m_tx * a.ld;                                        // [ld][K]
    for (int64_t ul = (int64_t)blockIdx.x * wpb + wave; ul < a.user_count; ul += (int64_t)gridDim.x * wpb) {
        const int64_t u = a.user_begin + ul;
        small_user_block<KC, 1>(a, WsRecords{ws, (size_t)u * ws.P}, ws.n_keep[u], lane, brx, atx, g,
                             out + (size_t)ul * a.m_rx * a.m_tx * a.K);
    }
}

static int small_ld(const WsView& ws) { return ws.P < 32 ? ws.P : 32; }      // first 32 kept paths, the rest through launch_extra_path_passes
static int small_waves_per_block(const dmx_params& prm, const WsView& ws) {
    return lds_waves_per_block(small_table_bytes(prm, small_ld(ws)));
}

bool fd_small_supported(const dmx_params& prm, const WsView& ws) { return small_waves_per_block(prm, ws) > 0; }

// Automatic choice, from tools/small_k_sweep.sh (200k users, 25 paths, ms for matrix-core | vector | this kernel):
//   64 pairs x K=1   2.08 | 2.98 | 0.14      64 pairs x K=8    3.71 | 5.09 | 1.08     1024 pairs x K=2  16.1 | 78.6 | 2.6
//   256 pairs x K=8  5.32 | 34.7 | 7.15      256 pairs x K=16  6.56 | 23.3 | 9.6
//   8 pairs x K=1    1.90 | 0.44 | 0.10      8 pairs x K=16    3.50 | 0.96 | 0.53     8 pairs x K=64    4.02 | 1.32 | 1.91
// i.e. up to ~8 subcarriers this kernel wins unless the tables push it to one wave per workgroup; below 24 antenna
// pairs (where the matrix cores are not used) it wins up to 16 subcarriers, the subcarrier-per-lane kernel beyond.
bool fd_small_preferred(const dmx_params& prm, const WsView& ws) {
    const int wpb = small_waves_per_block(prm, ws);
    if (!wpb) return false;
    const int K = prm.n_selected;
    const int64_t M = (int64_t)prm.ue_shape[0] * prm.ue_shape[1] * prm.bs_shape[0] * prm.bs_shape[1];
    if (M < 24) return K <= 16;
    if (K <= 4) return true;
    return K <= 8 && wpb >= 2 && M * K <= 2048;
}

int launch_channels_fd_small(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                             float2* out, hipStream_t stream) {
    const int wpb = small_waves_per_block(prm, ws);
    if (!wpb) { set_error("small-output kernel: tables of one user do not fit the LDS"); return DMX_ERR_SHAPE; }
    const SmallArgs a = small_args(prm, user_begin, user_count, small_ld(ws));
    const size_t smem = (size_t)wpb * small_table_bytes(prm, a.ld);
    // persistent: as many workgroups as the LDS lets be resident (160 KB per CU), at most 8 waves per SIMD
    int per_cu = (int)((size_t)160 * 1024 / smem);
    if (per_cu * wpb > 32) per_cu = 32 / wpb;
    if (per_cu < 1) per_cu = 1;
    int64_t grid = (user_count + wpb - 1) / wpb;
    if (grid > (int64_t)256 * per_cu) grid = (int64_t)256 * per_cu;
    const dim3 g((unsigned)grid), b(64 * wpb);
    if (a.K >= 4) return launch_dyn_lds(k2_fd_small<4>, "k2_fd_small", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
    if (a.K >= 2) return launch_dyn_lds(k2_fd_small<2>, "k2_fd_small", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
    return launch_dyn_lds(k2_fd_small<1>, "k2_fd_small", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
}

}  // namespace dmx
