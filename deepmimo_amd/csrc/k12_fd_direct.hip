// Single-pass frequency-domain channels for small outputs: ray matrices -> H in ONE launch, no HBM workspace.
//
// The two-call route (k1_path_prep -> 60 B/path records in HBM -> k2_fd_small) moves 4.3 x the bytes of the rays
// themselves when a user's block is a few dozen bytes (DeepMIMO's default: 8 antenna pairs, one subcarrier).  Here one
// WAVE owns one user from its ray row to its output block:
//   phase A   lane = loaded path: stage1_path (k1_path_math.h, the body k1_path_prep runs), ballot / popcount
//             compaction of the kept paths into the wave's LDS record slice, and the light side products (path count,
//             LoS, FoV mask, running delay maximum) through stage1_user_out;
//   phase B/C small_user_block (k2_small_body.h, the body k2_fd_small runs): tables b_rx / a_tx / g built from the LDS
//             records, then the output loop.
// Waves of a workgroup never talk to each other, no workgroup barrier anywhere.  Flat grid of ceil(user_count / waves
// per workgroup) workgroups, as k1_path_prep.
//
// Bit identity with the two calls is the contract (tests/test_gpu_fd_direct.py) and follows from the source: both bodies
// are shared, this file is compiled without FMA contraction like k1_path_prep.hip, and small_user_block leaves nothing
// to contraction.  MODE selects which of stage 1's three arithmetic forms runs: stage1_form (k1_path_math.h) is the one
// rule of both launchers - the zero-rotation form only up to 32 loaded paths, where stage 1 has it - so the same
// inputs take the same form.
//
// Scope (fd_direct_waves_per_block): frequency domain, rx_filter = 0, flags = 0, loaded paths <= 64 (one pass of the
// wave), used paths <= 32, tables + records of a wave within the LDS.  Everything else: DMX_ERR_SHAPE, never wrong
// numbers.  The record slice drops dop_v / dop_a of the HBM layout: only the rx_filter kernels read them.
#include "dmx_common.h"
#include "k1_path_math.h"
#include "k2_small_body.h"

namespace dmx {

struct DirectArgs {
    dmx_rays rays;
    // light side products, indexed by absolute user (nullptr = not wanted)
    uint8_t* fov_mask;
    int32_t* num_paths;
    int32_t* los;
    uint32_t* max_delay_key;
    Stage1Params s1;
    SmallArgs s2;
};

// one wave's compacted records in LDS (the WsView fields k2_fd_small reads), 8-byte fields first
static constexpr int DIRECT_SLOTS = 32;
struct DirectRecords {
    double tx_y[DIRECT_SLOTS], tx_z[DIRECT_SLOTS], rx_y[DIRECT_SLOTS], rx_z[DIRECT_SLOTS];
    float c_re[DIRECT_SLOTS], c_im[DIRECT_SLOTS], dn[DIRECT_SLOTS];
};
static constexpr size_t DIRECT_REC_BYTES = sizeof(DirectRecords);          // 1408
static_assert(DIRECT_REC_BYTES % 8 == 0, "the float2 tables behind the records stay 8-byte aligned");
// small_user_block's view of them (WsRecords is the workspace's)
struct LdsRecords {
    const DirectRecords* r;
    __device__ float c_re(int l) const { return r->c_re[l]; }
    __device__ float c_im(int l) const { return r->c_im[l]; }
    __device__ float dn(int l) const { return r->dn[l]; }
    __device__ double tx_y(int l) const { return r->tx_y[l]; }
    __device__ double tx_z(int l) const { return r->tx_z[l]; }
    __device__ double rx_y(int l) const { return r->rx_y[l]; }
    __device__ double rx_z(int l) const { return r->rx_z[l]; }
};

// MODE = Stage1Form: 0 = angles as numbers (FoV, dipole or sector pattern), 1 = lean, 2 = lean with exactly zero rotations (<= 32 loaded paths)
template <int KC, int MODE>
__global__ __launch_bounds__(256) void k12_fd_direct(DirectArgs a, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.s2.user_count) return;                                      // wave-uniform
    const int64_t u = a.s2.user_begin + ul;
    const int ld = a.s2.ld;
    const size_t per_wave = DIRECT_REC_BYTES + (size_t)(a.s2.m_rx + a.s2.m_tx + a.s2.K) * ld * sizeof(float2);
    unsigned char* base = smem_raw + (size_t)wave * per_wave;
    DirectRecords* rec = reinterpret_cast<DirectRecords*>(base);
    float2* brx = reinterpret_cast<float2*>(base + DIRECT_REC_BYTES);       // [m_rx][ld]
    float2* atx = brx + (size_t)a.s2.m_rx * ld;                             // [m_tx][ld]
    float2* g = atx + (size_t)a.s2.m_tx * ld;                               // [ld][K]

    // Phase A: the one pass of k1_path_prep<64, LEAN, ZROT> a user with <= 64 loaded paths needs - frequency domain,
    // rx_filter = 0, none of the angle / power side outputs (need_angles of launch_path_prep without them)
    dmx_side side = {};
    side.fov_mask = a.fov_mask; side.num_paths = a.num_paths; side.los = a.los; side.max_delay_key = a.max_delay_key;
    const int need_angles = a.s1.fov_enabled || a.s1.bs_pat != DMX_PATTERN_ISOTROPIC || a.s1.ue_pat != DMX_PATTERN_ISOTROPIC;
    double usx, ucx, usy, ucy, urz;
    stage1_ue_rotation(a.s1, u, usx, ucx, usy, ucy, urz);
    constexpr int freq_domain = 1, rx_filter = 0, grp = 0;                  // constants: stage 1's other branches are compiled out
    constexpr bool first_pass = true;
    const bool in = lane < a.rays.n_paths;
    Stage1User us;
    const Stage1Path p = stage1_path<64, MODE != 0, MODE == 2>(a.s1, a.rays, side, freq_domain, rx_filter, need_angles, usx, ucx,
                                                               usy, ucy, urz, u, lane, in, grp, first_pass, us);
    const unsigned long long kb = __ballot(p.keep);
    if (p.keep) {                                                 // keep => lane < P <= DIRECT_SLOTS, so slot < DIRECT_SLOTS
        const int slot = __popcll(kb & ((1ull << lane) - 1ull));
        rec->c_re[slot] = p.c_re; rec->c_im[slot] = p.c_im; rec->dn[slot] = p.dn;
        rec->tx_y[slot] = p.ty; rec->tx_z[slot] = p.tz;
        rec->rx_y[slot] = p.ry; rec->rx_z[slot] = p.rz;
    }
    float maxd = us.maxd;
    for (int off = 32; off > 0; off >>= 1) maxd = fmaxf(maxd, __shfl_xor(maxd, off, 64));
    const bool anyd = __ballot(us.any_delay) != 0ull;
    if (lane == 0) stage1_user_out(side, a.s1.fov_enabled, u, us, maxd, anyd);

    small_user_block<KC, (KC == 4 ? 2 : 4)>(a.s2, LdsRecords{rec}, __popcll(kb), lane, brx, atx, g, out + (size_t)ul * a.s2.m_rx * a.s2.m_tx * a.s2.K);
}

static int direct_used_paths(const dmx_params& prm, int32_t n_paths_loaded) {
    return prm.num_paths < n_paths_loaded ? prm.num_paths : n_paths_loaded;
}
// Waves per workgroup by k2_fd_small's rule with the record slice added.  0 = outside the kernel's scope.
int fd_direct_waves_per_block(const dmx_params& prm, int32_t n_paths_loaded) {
    if (!prm.freq_domain || prm.rx_filter || prm.flags != 0) return 0;
    if (n_paths_loaded < 1 || n_paths_loaded > 64 || prm.n_selected < 1) return 0;
    const int P = direct_used_paths(prm, n_paths_loaded);
    if (P < 1 || P > DIRECT_SLOTS) return 0;
    return lds_waves_per_block(DIRECT_REC_BYTES + small_table_bytes(prm, P));
}

template <int MODE>
static int launch_direct_m(const DirectArgs& a, dim3 g, dim3 b, size_t smem, float2* out, hipStream_t stream) {
    if (a.s2.K >= 4) return launch_dyn_lds(k12_fd_direct<4, MODE>, "k12_fd_direct", g, b, smem, WAVE_LDS_MAX, stream, a, out);
    if (a.s2.K >= 2) return launch_dyn_lds(k12_fd_direct<2, MODE>, "k12_fd_direct", g, b, smem, WAVE_LDS_MAX, stream, a, out);
    return launch_dyn_lds(k12_fd_direct<1, MODE>, "k12_fd_direct", g, b, smem, WAVE_LDS_MAX, stream, a, out);
}

int launch_channels_fd_direct(const dmx_rays& rays, const dmx_params& prm, const dmx_side& side, int64_t user_begin,
                              int64_t user_count, float2* out, hipStream_t stream) {
    const int wpb = fd_direct_waves_per_block(prm, rays.n_paths);
    if (!wpb) {
        set_error("dmx_channels_fd_direct does not take this shape (frequency domain, rx_filter = 0, flags = 0, <= 64 loaded and "
                  "<= 32 used paths, tables within the LDS): call dmx_path_prep + dmx_channels_fd");
        return DMX_ERR_SHAPE;
    }
    if (user_count == 0) return DMX_OK;
    DirectArgs a;
    a.rays = rays;
    a.fov_mask = side.fov_mask; a.num_paths = side.num_paths; a.los = side.los; a.max_delay_key = side.max_delay_key;
    const int P = direct_used_paths(prm, rays.n_paths);
    a.s1 = stage1_params(prm, P);
    a.s2 = small_args(prm, user_begin, user_count, P);
    // the arithmetic form launch_path_prep picks for the same parameters, side pointers and path count
    const Stage1Form form = stage1_form(prm, side, rays.n_paths);
    const size_t smem = (size_t)wpb * (DIRECT_REC_BYTES + small_table_bytes(prm, P));
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), b(64 * wpb);
    if (form == STAGE1_LEAN_ZROT) return launch_direct_m<2>(a, g, b, smem, out, stream);
    if (form == STAGE1_LEAN) return launch_direct_m<1>(a, g, b, smem, out, stream);
    return launch_direct_m<0>(a, g, b, smem, out, stream);
}

}  // namespace dmx
