// Single-pass frequency-domain channels for small outputs: ray matrices -> H in ONE launch, no HBM workspace.
//
// The two-call route (k1_path_prep -> 60 B/path records in HBM -> k2_fd_small) moves 4.3 x the bytes of the rays
// themselves when a user's block is a few dozen bytes (DeepMIMO's default: 8 antenna pairs, one subcarrier).  Here one
// WAVE owns one user from its ray row to its output block:
//   phase A   lane = loaded path: stage 1's per-path arithmetic (k1_path_math.h, the very functions k1_path_prep
//             calls), ballot / popcount compaction of the kept paths into the wave's LDS record slice, and the light
//             side products (path count, LoS, FoV mask, running delay maximum);
//   phase B   k2_fd_small's tables b_rx / a_tx / g built from the LDS records;
//   phase C   k2_fd_small's output loop (lane = antenna pair x chunk of KC subcarriers, coalesced stores).
// Waves of a workgroup never talk to each other: direct_lds_fence orders a wave's own LDS traffic for the compiler, no
// workgroup barrier anywhere.  Flat grid of ceil(user_count / waves per workgroup) workgroups, as k1_path_prep.
//
// Bit identity with the two calls is the contract (tests/test_gpu_fd_direct.py): phase A is written operation for
// operation like k1_path_prep's loop body and, like that file, compiled without FMA contraction; phases B / C are
// k2_fd_small's statements with the contraction that file is compiled with (the pragma below).  MODE selects which of
// stage 1's three arithmetic forms runs: stage1_form (k1_path_math.h) is the one rule of both launchers - the zero-rotation
// form only up to 32 loaded paths, where stage 1 has it - so the same inputs take the same form.
//
// Scope (fd_direct_waves_per_block): frequency domain, rx_filter = 0, flags = 0, loaded paths <= 64 (one pass of the
// wave), used paths <= 32, tables + records of a wave within the LDS.  Everything else: DMX_ERR_SHAPE, never wrong
// numbers.  The record slice drops dop_v / dop_a of the HBM layout: only the rx_filter kernels read them.
#include "dmx_common.h"
#include "k1_path_math.h"

namespace dmx {

struct DirectArgs {
    dmx_rays rays;
    // light side products, indexed by absolute user (nullptr = not wanted)
    uint8_t* fov_mask;
    int32_t* num_paths;
    int32_t* los;
    uint32_t* max_delay_key;
    // stage 1 (PrepArgs of k1_path_prep.hip)
    double bsx, csx, bsy, csy, brz;
    double usx, ucx, usy, ucy, urz;
    const double* ue_rot_pu;
    int fov_enabled, bs_restricted, ue_restricted;
    double bs_fh, bs_fv, ue_fh, ue_fv;
    int bs_pat, ue_pat;
    double bs_spacing, ue_spacing;
    int P;
    int n_sc;
    float ts32;
    int doppler;
    double fc;
    // stage 2 (SmallArgs of k2_channel_fd_small.hip)
    int64_t user_begin, user_count;
    int m_rx, m_tx, ue_mh, bs_mh;
    int K;
    const int32_t* sc;
    double inv_n;
    int ld;
};

// one wave's compacted records in LDS (the WsView fields k2_fd_small reads), 8-byte fields first
static constexpr int DIRECT_SLOTS = 32;
struct DirectRecords {
    double tx_y[DIRECT_SLOTS], tx_z[DIRECT_SLOTS], rx_y[DIRECT_SLOTS], rx_z[DIRECT_SLOTS];
    float c_re[DIRECT_SLOTS], c_im[DIRECT_SLOTS], dn[DIRECT_SLOTS];
};
static constexpr size_t DIRECT_REC_BYTES = sizeof(DirectRecords);          // 1408
static_assert(DIRECT_REC_BYTES % 8 == 0, "the float2 tables behind the records stay 8-byte aligned");

__device__ __forceinline__ void direct_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Phase A: k1_path_prep<64, LEAN, ZROT>'s loop body for the one pass a user with <= 64 loaded paths needs, flags = 0,
// frequency domain, rx_filter = 0; records go to `rec` instead of the workspace.  Returns the kept-path count.
template <bool LEAN, bool ZROT>
__device__ __forceinline__ int direct_phase_a(const DirectArgs& a, const int64_t u, const int lane, DirectRecords* rec) {
    const dmx_rays& r = a.rays;
    const int L = r.n_paths;
    const size_t row = (size_t)u * (size_t)r.ld;
    const size_t srow = (size_t)u * (size_t)L;

    double usx = a.usx, ucx = a.ucx, usy = a.usy, ucy = a.ucy, urz = a.urz;
    if (a.ue_rot_pu) {
        const double rx = a.ue_rot_pu[3 * u + 0] * D2R_D, ry = a.ue_rot_pu[3 * u + 1] * D2R_D;
        urz = a.ue_rot_pu[3 * u + 2] * D2R_D;
        sincos(rx, &usx, &ucx);
        sincos(ry, &usy, &ucy);
    }
    const bool iso = (a.bs_pat == DMX_PATTERN_ISOTROPIC) && (a.ue_pat == DMX_PATTERN_ISOTROPIC);
    const float nan32 = __int_as_float(0x7fc00000);
    const double nan64 = (double)nan32;

    const int j = lane;
    const bool in = j < L;
    // the eight (ten) loads together, from an index every lane may read, masked afterwards (k1_path_prep.hip)
    const size_t jc = row + (size_t)(j < L ? j : L - 1);
    const float power_r = r.power[jc], phase_r = r.phase[jc], delay_r = r.delay[jc], aoa_az_r = r.aoa_az[jc];
    const float aoa_el_r = r.aoa_el[jc], aod_az_r = r.aod_az[jc], aod_el_r = r.aod_el[jc], inter_r = r.inter[jc];
    const bool dop_rays = a.doppler && r.doppler_vel && r.doppler_acc;
    float dvel_r = 0.f, dacc_r = 0.f;
    if (dop_rays) { dvel_r = r.doppler_vel[jc]; dacc_r = r.doppler_acc[jc]; }
    const float power = in ? power_r : nan32;
    const float phase = in ? phase_r : nan32;
    const float delay = in ? delay_r : nan32;
    const float aoa_az = in ? aoa_az_r : nan32;
    const float aoa_el = in ? aoa_el_r : nan32;
    const float aod_az = in ? aod_az_r : nan32;
    const float aod_el = in ? aod_el_r : nan32;
    const float inter = in ? inter_r : nan32;

    double zc_t, re_t, im_t, zc_r, re_r, im_r, sphi_t = 0.0, sphi_r = 0.0;
    if constexpr (ZROT) {
        rotate_dir_zero(aod_el, aod_az, zc_t, re_t, im_t, sphi_t);
        rotate_dir_zero(aoa_el, aoa_az, zc_r, re_r, im_r, sphi_r);
    } else {
        rotate_dir<LEAN>(aod_el, aod_az, a.bsx, a.csx, a.bsy, a.csy, a.brz, zc_t, re_t, im_t);
        rotate_dir<LEAN>(aoa_el, aoa_az, usx, ucx, usy, ucy, urz, zc_r, re_r, im_r);
    }
    double th_t = (isnan(zc_t) || fabs(zc_t) > 1.0) ? nan64 : 0.0, ph_t = (isnan(re_t) || isnan(im_t)) ? nan64 : 0.0;
    double th_r = (isnan(zc_r) || fabs(zc_r) > 1.0) ? nan64 : 0.0, ph_r = (isnan(re_r) || isnan(im_r)) ? nan64 : 0.0;
    if constexpr (!LEAN) {
        // need_angles of launch_path_prep without the angle outputs this kernel does not have
        if (a.fov_enabled || !iso) {
            th_t = acos(zc_t); ph_t = atan2(im_t, re_t);
            th_r = acos(zc_r); ph_r = atan2(im_r, re_r);
        }
    }

    bool mask = true;
    bool has_fov_path = false;
    float first_inter;
    if (!LEAN && a.fov_enabled) {
        if (a.bs_restricted) mask = mask && in_fov(th_t, ph_t, a.bs_fh, a.bs_fv);
        if (a.ue_restricted) mask = mask && in_fov(th_r, ph_r, a.ue_fh, a.ue_fv);
        mask = mask && in;
        if (in && a.fov_mask) a.fov_mask[srow + j] = mask ? 1 : 0;
        if (!mask) { th_t = nan64; ph_t = nan64; th_r = nan64; ph_r = nan64; }
        const unsigned long long mb = __ballot(mask);
        const int src = mb != 0ull ? __ffsll((long long)mb) - 1 : 0;
        const float cand = __shfl(inter, src, 64);
        first_inter = nan32;
        if (mb != 0ull) { has_fov_path = true; first_inter = cand; }
    } else {
        first_inter = __shfl(inter, 0, 64);
    }
    const int count_paths = __popcll(__ballot(in && !isnan(ph_r)));

    const float p10 = power / 10.0f;
    const float pl = exp10f(p10);
    double pw;
    if (LEAN || iso) {
        pw = (double)pl;
    } else {
        const double gt = a.bs_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_t) : 1.0;
        const double gr = a.ue_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_r) : 1.0;
        pw = (double)pl * (gt * gr);
    }

    const bool used = in && j < a.P;
    float maxd = -INFINITY;
    bool any_delay = false;
    if (used && !isnan(delay)) { maxd = fmaxf(maxd, delay); any_delay = true; }
    const bool valid = used && !isnan(pw);
    const float ph32 = phase * D2R_F;
    float e_re, e_im;
    np_sincosf(ph32, e_im, e_re);
    const bool ang_ok = !isnan(th_t) && !isnan(th_r);
    float c_re, c_im;
    float dn = delay / a.ts32;
    double pwc = pw;
    if (dn >= (float)a.n_sc) { pwc = 0.0; dn = (float)a.n_sc; }
    if (LEAN || iso) {
        const float amp = sqrtf((float)pwc / (float)a.n_sc);
        c_re = amp * e_re; c_im = amp * e_im;
    } else {
        const double amp = sqrt(pwc / (double)a.n_sc);
        c_re = (float)(amp * (double)e_re); c_im = (float)(amp * (double)e_im);
    }
    if (dop_rays) {
        const double v = in ? (double)dvel_r : 0.0;
        const double ac = in ? (double)dacc_r : 0.0;
        const double tau = (double)delay;
        const double arg = -TWO_PI * a.fc * (v * tau / LIGHTSPEED + ac * (tau * tau) / (2.0 * LIGHTSPEED));
        double sd, cd;
        sincos(arg, &sd, &cd);
        const float nr = (float)((double)c_re * cd - (double)c_im * sd);
        const float ni = (float)((double)c_re * sd + (double)c_im * cd);
        c_re = nr; c_im = ni;
    }
    const bool keep = valid && ang_ok && !isnan(ph_t) && !isnan(ph_r) && !isnan(c_re) && !isnan(c_im) && !isnan(dn) &&
                      (c_re != 0.0f || c_im != 0.0f);
    double ty = 0.0, tz = 0.0, ry = 0.0, rz = 0.0;
    if (ang_ok && ZROT) {
        ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * sphi_t); tz = a.bs_spacing * zc_t;
        ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * sphi_r); rz = a.ue_spacing * zc_r;
    } else if (ang_ok) {
        const double rho_t = sqrt(re_t * re_t + im_t * im_t), rho_r = sqrt(re_r * re_r + im_r * im_r);
        ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * (rho_t > 0.0 ? im_t / rho_t : 0.0)); tz = a.bs_spacing * zc_t;
        ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * (rho_r > 0.0 ? im_r / rho_r : 0.0)); rz = a.ue_spacing * zc_r;
    }
    const unsigned long long kb = __ballot(keep);
    if (keep) {                                                   // keep => j < P <= DIRECT_SLOTS, so slot < DIRECT_SLOTS
        const int slot = __popcll(kb & ((1ull << lane) - 1ull));
        rec->c_re[slot] = c_re; rec->c_im[slot] = c_im; rec->dn[slot] = dn;
        rec->tx_y[slot] = ty; rec->tx_z[slot] = tz;
        rec->rx_y[slot] = ry; rec->rx_z[slot] = rz;
    }

    for (int off = 32; off > 0; off >>= 1) maxd = fmaxf(maxd, __shfl_xor(maxd, off, 64));
    const bool anyd = __ballot(any_delay) != 0ull;
    if (lane == 0) {
        if (a.num_paths) a.num_paths[u] = count_paths;
        if (a.los) {
            const bool has = a.fov_enabled ? has_fov_path : (count_paths > 0);
            a.los[u] = has ? ((first_inter == 0.0f) ? 1 : 0) : -1;
        }
        // look first, update only when this user raises the launch's maximum (k1_path_prep.hip)
        if (a.max_delay_key && anyd) {
            const uint32_t key = float_order_key(maxd);
            if (key > __hip_atomic_load(a.max_delay_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(a.max_delay_key, key);
        }
    }
    return __popcll(kb);
}

// the file is compiled without FMA contraction for phase A; from here on the statements are k2_fd_small's and contract
// as they do in k2_channel_fd_small.hip
#pragma clang fp contract(fast)

// MODE = Stage1Form: 0 = angles as numbers (FoV, dipole pattern), 1 = lean, 2 = lean with exactly zero rotations (<= 32 loaded paths)
template <int KC, int MODE>
__global__ __launch_bounds__(256) void k12_fd_direct(DirectArgs a, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                         // wave-uniform
    const int64_t u = a.user_begin + ul;
    const int ld = a.ld, K = a.K, M = a.m_rx * a.m_tx;
    const size_t per_wave = DIRECT_REC_BYTES + (size_t)(a.m_rx + a.m_tx + K) * ld * sizeof(float2);
    unsigned char* base = smem_raw + (size_t)wave * per_wave;
    DirectRecords* rec = reinterpret_cast<DirectRecords*>(base);
    float2* brx = reinterpret_cast<float2*>(base + DIRECT_REC_BYTES);       // [m_rx][ld]
    float2* atx = brx + (size_t)a.m_rx * ld;                                // [m_tx][ld]
    float2* g = atx + (size_t)a.m_tx * ld;                                  // [ld][K]

    int n_act = direct_phase_a<MODE != 0, MODE == 2>(a, u, lane, rec);
    n_act = n_act < ld ? n_act : ld;
    float2* o = out + (size_t)ul * M * K;
    if (n_act == 0) {                                                       // channel.py:270-271
        for (int i = lane; i < M * K; i += 64) o[i] = make_float2(0.f, 0.f);
        return;
    }
    direct_lds_fence();                                                     // records are written

    for (int i = lane; i < a.m_rx * n_act; i += 64) {
        const int r = i / n_act, l = i - r * n_act;
        float s, c;
        sincos_rev(frac_rev((double)(r % a.ue_mh) * rec->rx_y[l] + (double)(r / a.ue_mh) * rec->rx_z[l]), s, c);
        const float cr = rec->c_re[l], ci = rec->c_im[l];
        // k2_fd_small's `cr * c - ci * s, cr * s + ci * c` as the compiler contracts it there: which product of a sum
        // goes into the FMA is its choice, and it chose differently in this kernel.  Written out, it cannot
        brx[r * ld + l] = make_float2(fmaf(cr, c, -(ci * s)), fmaf(cr, s, ci * c));
    }
    for (int i = lane; i < a.m_tx * n_act; i += 64) {
        const int t = i / n_act, l = i - t * n_act;
        float s, c;
        sincos_rev(frac_rev((double)(t % a.bs_mh) * rec->tx_y[l] + (double)(t / a.bs_mh) * rec->tx_z[l]), s, c);
        atx[t * ld + l] = make_float2(c, s);
    }
    for (int i = lane; i < n_act * K; i += 64) {
        const int l = i / K, k = i - l * K;
        float s, c;
        // k2_fd_small contracts frac_rev's `t - rint(t)` with the product that makes t: the fractional part of the EXACT
        // product x * k, which matters once dn / N * k needs more than 53 bits (|k| towards 2^31).  Written out likewise
        const double x = (double)rec->dn[l] * a.inv_n, kd = (double)a.sc[k];
        sincos_rev((float)__builtin_fma(x, kd, -rint(x * kd)), s, c);
        g[l * K + k] = make_float2(c, -s);                                  // exp(-j 2pi x) = cos - j sin
    }
    direct_lds_fence();

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
        for (int l = 0; l < n_act; ++l) {
            const float2 b = br[l], t = at[l];
            const float wr = b.x * t.x - b.y * t.y, wi = b.x * t.y + b.y * t.x;
            const float2* gl = g + l * K;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const float2 v = gl[kj[j]];
                acc[j].x += wr * v.x - wi * v.y;
                acc[j].y += wr * v.y + wi * v.x;
            }
        }
        float2* dst = o + (size_t)p * K + k0;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (k0 + j < K) dst[j] = acc[j];
    }
}

// Waves per workgroup by k2_fd_small's rule with the record slice added: four while 4 x (records + tables) fit the
// 64 KB a workgroup gets by default, then two, then one wave with up to 156 KB.  0 = outside the kernel's scope.
static constexpr size_t DIRECT_LDS_MAX = 156 * 1024;
int fd_direct_waves_per_block(const dmx_params& prm, int32_t n_paths_loaded) {
    if (!prm.freq_domain || prm.rx_filter || prm.flags != 0) return 0;
    if (n_paths_loaded < 1 || n_paths_loaded > 64 || prm.n_selected < 1) return 0;
    const int P = prm.num_paths < n_paths_loaded ? prm.num_paths : n_paths_loaded;
    if (P < 1 || P > DIRECT_SLOTS) return 0;
    const size_t bytes = DIRECT_REC_BYTES + ((size_t)prm.ue_shape[0] * prm.ue_shape[1] + (size_t)prm.bs_shape[0] * prm.bs_shape[1] +
                                             (size_t)prm.n_selected) * P * 8;
    if (bytes * 4 <= 64 * 1024) return 4;
    if (bytes * 2 <= 64 * 1024) return 2;
    if (bytes <= DIRECT_LDS_MAX) return 1;
    return 0;
}

template <int KC, int MODE>
static int launch_direct_t(const DirectArgs& a, dim3 g, dim3 b, size_t smem, float2* out, hipStream_t stream) {
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k12_fd_direct<KC, MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)DIRECT_LDS_MAX);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return DMX_ERR_LAUNCH; }
    }
    hipLaunchKernelGGL((k12_fd_direct<KC, MODE>), g, b, smem, stream, a, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("k12_fd_direct launch failed: %s", hipGetErrorString(e)); return DMX_ERR_LAUNCH; }
    return DMX_OK;
}

template <int MODE>
static int launch_direct_m(const DirectArgs& a, dim3 g, dim3 b, size_t smem, float2* out, hipStream_t stream) {
    if (a.K >= 4) return launch_direct_t<4, MODE>(a, g, b, smem, out, stream);
    if (a.K >= 2) return launch_direct_t<2, MODE>(a, g, b, smem, out, stream);
    return launch_direct_t<1, MODE>(a, g, b, smem, out, stream);
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
    a.bsx = sin(prm.bs_rotation[0]); a.csx = cos(prm.bs_rotation[0]);
    a.bsy = sin(prm.bs_rotation[1]); a.csy = cos(prm.bs_rotation[1]);
    a.brz = prm.bs_rotation[2];
    a.usx = sin(prm.ue_rotation[0]); a.ucx = cos(prm.ue_rotation[0]);
    a.usy = sin(prm.ue_rotation[1]); a.ucy = cos(prm.ue_rotation[1]);
    a.urz = prm.ue_rotation[2];
    a.ue_rot_pu = prm.ue_rotation_per_user;
    a.fov_enabled = prm.fov_enabled; a.bs_restricted = prm.bs_fov_restricted; a.ue_restricted = prm.ue_fov_restricted;
    a.bs_fh = prm.bs_fov[0]; a.bs_fv = prm.bs_fov[1]; a.ue_fh = prm.ue_fov[0]; a.ue_fv = prm.ue_fov[1];
    a.bs_pat = prm.bs_pattern; a.ue_pat = prm.ue_pattern;
    a.bs_spacing = prm.bs_spacing; a.ue_spacing = prm.ue_spacing;
    a.P = prm.num_paths < rays.n_paths ? prm.num_paths : rays.n_paths;
    a.n_sc = prm.n_subcarriers;
    a.ts32 = (float)(1.0 / prm.bandwidth);
    a.doppler = prm.enable_doppler; a.fc = prm.carrier_freq;
    a.user_begin = user_begin; a.user_count = user_count;
    a.m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    a.m_tx = prm.bs_shape[0] * prm.bs_shape[1];
    a.ue_mh = prm.ue_shape[0];
    a.bs_mh = prm.bs_shape[0];
    a.K = prm.n_selected;
    a.sc = prm.selected_subcarriers;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.ld = a.P;
    // the arithmetic form launch_path_prep picks for the same parameters, side pointers and path count (stage1_form is
    // the launchers' one rule: the zero-rotation form only up to 32 loaded paths, as stage 1 has it)
    const Stage1Form form = stage1_form(prm, side, rays.n_paths);
    const size_t smem = (size_t)wpb * (DIRECT_REC_BYTES + (size_t)(a.m_rx + a.m_tx + a.K) * a.ld * 8);
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), b(64 * wpb);
    if (form == STAGE1_LEAN_ZROT) return launch_direct_m<2>(a, g, b, smem, out, stream);
    if (form == STAGE1_LEAN) return launch_direct_m<1>(a, g, b, smem, out, stream);
    return launch_direct_m<0>(a, g, b, smem, out, stream);
}

}  // namespace dmx
