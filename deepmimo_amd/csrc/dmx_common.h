// Shared definitions of the HIP side: the per-path record layout that stage 1 (k1_path_prep)
// writes and stage 2 (k2_channel_fd / k4_channel_td) reads, and small device helpers.
//
// Record layout in the caller-provided workspace (SoA, one array per field, [n_ue, P] row-major,
// P = min(params.num_paths, loaded paths)).  Paths that take part in a user's sum are COMPACTED to
// the front of the user's row; n_keep[u] says how many.  Phase steps are kept in REVOLUTIONS
// (phase / 2pi) in float64 so that element-index multiples stay exact before range reduction:
//   a_tx[m = y + Mh*z, l] = exp(j 2pi (y*tx_y[l] + z*tx_z[l]))      geometry.py:85-102
// (kd = 2pi*spacing, so kd*sin(theta)sin(phi)/2pi = spacing*sin(theta)sin(phi)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/deepmimo_amd.h"

namespace dmx {

struct WsView {
    float*   c_re;    // [n, P]  path coefficient: FD sqrt(p/N) e^{j phase} (x Doppler), TD sqrt(p) e^{j phase}
    float*   c_im;    // [n, P]
    float*   dn;      // [n, P]  normalised delay tau/Ts after the ">= N" clip (channel.py:183-189)
    double*  tx_y;    // [n, P]  revolutions per y-step of the BS panel
    double*  tx_z;    // [n, P]
    double*  rx_y;    // [n, P]
    double*  rx_z;    // [n, P]
    float*   dop_v;   // [n, P]  Doppler velocity / acceleration of the kept path (used by the rx_filter
    float*   dop_a;   //         variant only, where the Doppler phase depends on the tap index)
    int32_t* n_keep;  // [n]     compacted paths per user
    int64_t  n;
    int32_t  P;
    float    neg_one; // -1.0f as a kernel-argument SGPR the compiler cannot fold: the multiplier of the f16 split's
                      // residual fma, so that it is selected as v_fma_mix_f32 (k2_mfma_frag.h, split2_f16)
};

// Largest |selected index| the sc_first / sc_stride promise implies (int64: no wrap), or -1 without a promise
__host__ inline int64_t sc_hint_abs_max(const dmx_params& p) {
    if (p.sc_stride <= 0 || p.n_selected < 1) return -1;
    const int64_t a = p.sc_first, b = a + (int64_t)p.sc_stride * (p.n_selected - 1);
    const int64_t ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
    return ma > mb ? ma : mb;
}
// the promise shows an index the float32-phase kernels cannot take (include/deepmimo_amd.h DMX_SC_ABS_MAX_F32)
__host__ inline bool sc_beyond_f32(const dmx_params& p) { return sc_hint_abs_max(p) >= DMX_SC_ABS_MAX_F32; }

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carve the workspace.  Returns total bytes; fills `v` when base != nullptr.
__host__ inline size_t ws_carve(void* base, int64_t n, int32_t P, WsView* v) {
    size_t off = 0;
    const size_t np = (size_t)n * (size_t)P;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    size_t o_cre = take(np * 4), o_cim = take(np * 4), o_dn = take(np * 4);
    size_t o_txy = take(np * 8), o_txz = take(np * 8), o_rxy = take(np * 8), o_rxz = take(np * 8);
    size_t o_dv = take(np * 4), o_da = take(np * 4);
    size_t o_keep = take((size_t)n * 4);
    if (v) {
        char* b = (char*)base;
        v->c_re = (float*)(b + o_cre); v->c_im = (float*)(b + o_cim); v->dn = (float*)(b + o_dn);
        v->tx_y = (double*)(b + o_txy); v->tx_z = (double*)(b + o_txz);
        v->rx_y = (double*)(b + o_rxy); v->rx_z = (double*)(b + o_rxz);
        v->dop_v = (float*)(b + o_dv); v->dop_a = (float*)(b + o_da);
        v->n_keep = (int32_t*)(b + o_keep);
        v->n = n; v->P = P;
        v->neg_one = -1.0f;
    }
    return off;
}

// sin/cos of 2*pi*r for r already reduced to [-0.5, 0.5] revolutions.  v_sin_f32 / v_cos_f32 take
// their argument in revolutions, i.e. exactly this representation; measured max abs error on the
// reduced range (tools/sincos_acc.hip, MI355X): 1.25e-7, against 5.2e-8 for sincospif at ~15x the
// instructions.  All phase accuracy in this library lives in the float64 range reduction before.
__device__ __forceinline__ void sincos_rev(float r, float& s, float& c) {
    s = __builtin_amdgcn_sinf(r);
    c = __builtin_amdgcn_cosf(r);
}

// fractional part in [-0.5, 0.5] of a float64 phase given in revolutions
__device__ __forceinline__ float frac_rev(double t) {
    return (float)(t - rint(t));
}

// One wave's own LDS traffic is ordered by the hardware; this only stops the compiler from moving reads over writes
// (the one-wave-per-user kernels k2_fd_small and k12_fd_direct have no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

void set_error(const char* fmt, ...);

// Waves per workgroup of the one-wave-per-user kernels from the LDS bytes one wave needs: four while 4 x fit the 64 KB a
// workgroup gets by default, then two, then one; a single wave may take up to 156 KB (of the CU's 160 KB) with the
// dynamic-LDS attribute raised.  0 = does not fit.
static constexpr size_t WAVE_LDS_MAX = 156 * 1024;
__host__ inline int lds_waves_per_block(size_t bytes_per_wave) {
    if (bytes_per_wave == 0) return 0;
    if (bytes_per_wave * 4 <= 64 * 1024) return 4;
    if (bytes_per_wave * 2 <= 64 * 1024) return 2;
    if (bytes_per_wave <= WAVE_LDS_MAX) return 1;
    return 0;
}

// compute units of the current device (persistent grids are sized from it)
int device_cu_count();

// ---- launch layer: every kernel launch of the library goes through these two ----
// Workgroups of `kernel` the device holds at once, CUs x workgroups per CU as registers and LDS allow (1 where the
// runtime cannot say).  A persistent launcher turns it into its grid by its own, measured rule.
template <class... Params>
int64_t resident_workgroups(void (*kernel)(Params...), int threads, size_t smem) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), threads, smem) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    return (int64_t)device_cu_count() * per_cu;
}

// Launch, check, set the error string.  A request beyond the 64 KiB a workgroup gets by default first raises the
// kernel's dynamic-LDS attribute to `lds_cap` (per device and cheap: no cached flag, so every GPU of a process gets it);
// LDS_NO_RAISE is for kernels whose shape limits keep them within the default.
static constexpr size_t LDS_NO_RAISE = 0;
template <class... Params, class... Args>
int launch_dyn_lds(void (*kernel)(Params...), const char* name, dim3 g, dim3 b, size_t smem, size_t lds_cap, hipStream_t stream,
                   const Args&... args) {
    if (smem > 64 * 1024 && lds_cap != LDS_NO_RAISE) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute failed: %s", hipGetErrorString(e)); return DMX_ERR_LAUNCH; }
    }
    hipLaunchKernelGGL(kernel, g, b, smem, stream, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch failed: %s", name, hipGetErrorString(e)); return DMX_ERR_LAUNCH; }
    return DMX_OK;
}

// stage launchers (defined next to their kernels)
int launch_path_prep(const dmx_rays& rays, const dmx_params& prm, const WsView& ws, const dmx_side& side,
                     hipStream_t stream);
int launch_channels_fd(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                       float2* out, int variant, hipStream_t stream);
int fd_auto_choice(const dmx_params& prm, const WsView& ws);
int fd_direct_waves_per_block(const dmx_params& prm, int32_t n_paths_loaded);
int launch_channels_fd_direct(const dmx_rays& rays, const dmx_params& prm, const dmx_side& side, int64_t user_begin,
                              int64_t user_count, float2* out, hipStream_t stream);
int launch_channels_fd_lpf(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                           float2* gtab, float2* out, hipStream_t stream);
int launch_channels_fd_beams(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                             const float2* codebook, int n_beams, void* beam_ws, float2* out, hipStream_t stream);
size_t beam_workspace_bytes(int64_t user_count, int n_beams, int P);
int launch_beam_power(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                      const float2* codebook, int n_beams, void* beam_ws, float* out_amp, int32_t* out_best, hipStream_t stream);
bool fd_mfma_supported(const dmx_params& prm, const WsView& ws);
int launch_channels_td(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                       float2* out, hipStream_t stream);
int cov_waves_per_block(const dmx_params& prm, int P, int side, int* kc_out);
int launch_covariance(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, int side,
                      float2* out, hipStream_t stream);
size_t rate_lds_bytes(const dmx_params& prm, int P);
int rate_waves_per_block(const dmx_params& prm, int P);
int launch_rate(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                float* out_rate, float* out_rate_k, hipStream_t stream);
int launch_spectrum(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                    float* out_gamma, float* out_rate, float* out_rate_k, hipStream_t stream);
int launch_precoders(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, double snr_linear,
                     int n_layers, float* out_gamma, float2* out_tx, float2* out_rx, hipStream_t stream);
size_t cell_rate_lds_bytes(const dmx_link* links, int n_links);
int launch_cell_rate(const dmx_link* links, int n_links, int64_t n_ue, int64_t user_begin, int64_t user_count,
                     const int32_t* serving, float* out_rate, float* out_rate_k, int32_t* out_serving, float* out_link_snr,
                     hipStream_t stream);

size_t angle_delay_lds_bytes(const dmx_params& prm, int P, int n_rows, int n_taps);
int angle_delay_waves_per_block(const dmx_params& prm, int P, int n_rows, int n_taps);
int launch_angle_delay(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, const float2* codebook,
                       int n_rows, void* beam_ws, int n_fft, int n_taps, float2* out, hipStream_t stream);

size_t codebook_rate_lds_bytes(const dmx_params& prm, int P, int n_codewords, int n_layers);
int codebook_rate_waves_per_block(const dmx_params& prm, int P, int n_codewords, int n_layers);
int launch_codebook_rate(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, const float2* codebook,
                         int n_codewords, int n_layers, void* beam_ws, double snr_linear, float* out_rate, int32_t* out_pmi,
                         float* out_rate_c, hipStream_t stream);
size_t codebook_rate_subbands_lds_bytes(const dmx_params& prm, int P, int n_codewords, int n_layers, int subband_size);
int codebook_rate_subbands_waves_per_block(const dmx_params& prm, int P, int n_codewords, int n_layers, int subband_size);
int launch_codebook_rate_subbands(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                                  const float2* codebook, int n_codewords, int n_layers, void* beam_ws, double snr_linear,
                                  int subband_size, float* out_rate_sb, int32_t* out_pmi_sb, float* out_rate_sb_c, float* out_rate,
                                  int32_t* out_pmi, float* out_rate_c, hipStream_t stream);

// between the stage-2 files: the kernels variant 0 chooses from (k2_channel_fd.hip), their predicates and launchers
bool fd_mfma_preferred(const dmx_params& prm, const WsView& ws);
bool fd_small_preferred(const dmx_params& prm, const WsView& ws);
bool fd_fold_preferred(const dmx_params& prm, const WsView& ws);
int launch_channels_fd_mfma(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                            float2* out, int config, hipStream_t stream);
int launch_channels_fd_small(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                             float2* out, hipStream_t stream);
int launch_channels_fd_fold(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, float2* out,
                            int chunk_blocks, hipStream_t stream);
// rx_filter: the contraction over a gains table (float, or packed f16 where lpf_table_packed says the matrix-core
// kernel is its only reader)
bool lpf_table_packed(const dmx_params& prm, const WsView& ws);
int launch_channels_fd_mfma_gload(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                                  const float2* gtab, float2* out, hipStream_t stream, bool packed);
int launch_channels_fd_lpf_contract(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                                    const float2* gtab, float2* out, hipStream_t stream, bool packed);
// k2b_beam_project's output inside the beam workspace, read by the beam-space contraction and by k2c_beam_power
struct BeamTabs {
    const float2* ftab;      // [user_count, n_beams, P]  f[b,l] = sum_tx F[b,tx] a_tx[tx,l]
    const int32_t* fexp;     // [user_count]              exponent of max |f| per user
};
int launch_beam_project(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count,
                        const float2* codebook, int n_beams, void* beam_ws, hipStream_t stream, BeamTabs* tabs);

}  // namespace dmx
