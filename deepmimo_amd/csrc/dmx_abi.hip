// C-ABI entry points (include/deepmimo_amd.h): argument validation, workspace carving, error
// string.  No allocation, no synchronisation, no global state besides the thread-local message.
#include "dmx_common.h"
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace dmx {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int device_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
        (void)hipGetLastError();
        cus = 256;                                        // MI355X
    }
    return cus;
}

static int check_patterns(const dmx_params* p) {
    if (p->bs_pattern < 0 || p->bs_pattern > DMX_PATTERN_TR38901 || p->ue_pattern < 0 || p->ue_pattern > DMX_PATTERN_TR38901) {
        set_error("unknown radiation pattern id"); return DMX_ERR_ARG;
    }
    return DMX_OK;
}

// `takes`: which of DMX_FLAG_SPATIAL_WIDEBAND (dmx_path_prep and dmx_channels_fd only), DMX_FLAG_NEAR_FIELD (those two, the
// consumers, dmx_beam_power and their dmx_*_supported queries), DMX_FLAG_BEAM_MEAN_POWER (dmx_beam_power only) and
// DMX_FLAG_RX_LINEAR_MMSE (dmx_codebook_rate, dmx_codebook_rate_subbands and their two queries only) the caller takes; a flag
// it does not take is refused here.  DMX_FLAG_ANGLE_DELAY_POWER and DMX_FLAG_ANGLE_DELAY_PROFILE (dmx_channels_angle_delay and
// its query only; the second only beside the first) are asked after those, so that the refusals above keep their order, and
// DMX_FLAG_SERVING_SET (dmx_cell_rate and its query only) after them.
static constexpr uint32_t ANGLE_DELAY_OUTPUT_FLAGS = DMX_FLAG_ANGLE_DELAY_POWER | DMX_FLAG_ANGLE_DELAY_PROFILE;

static int check_params(const dmx_params* p, uint32_t takes = 0) {
    if (!p) { set_error("params is NULL"); return DMX_ERR_ARG; }
    for (int i = 0; i < 2; ++i) {
        if (p->bs_shape[i] < 1 || p->ue_shape[i] < 1) { set_error("antenna shape entries must be >= 1"); return DMX_ERR_SHAPE; }
    }
    if ((int64_t)p->bs_shape[0] * p->bs_shape[1] > 65536 || (int64_t)p->ue_shape[0] * p->ue_shape[1] > 65536) {
        set_error("antenna panel larger than 65536 elements"); return DMX_ERR_SHAPE;
    }
    if (check_patterns(p)) return DMX_ERR_ARG;
    if (p->num_paths < 0) { set_error("num_paths must be >= 0"); return DMX_ERR_ARG; }
    if ((p->flags & ~(DMX_FLAG_ADAPTIVE_TERMS | DMX_FLAG_SPATIAL_WIDEBAND | DMX_FLAG_NEAR_FIELD | DMX_FLAG_BEAM_MEAN_POWER |
                      DMX_FLAG_RX_LINEAR_MMSE | ANGLE_DELAY_OUTPUT_FLAGS | DMX_FLAG_SERVING_SET)) != 0 ||
        p->reserved0 != 0) { set_error("unknown bits in dmx_params.flags / reserved0"); return DMX_ERR_ARG; }
    if ((p->flags & DMX_FLAG_BEAM_MEAN_POWER) && !(takes & DMX_FLAG_BEAM_MEAN_POWER)) {
        set_error("DMX_FLAG_BEAM_MEAN_POWER is an option of the dmx_beam_power call alone: no other entry point takes it, "
                  "dmx_path_prep included");
        return DMX_ERR_ARG;
    }
    if ((p->flags & DMX_FLAG_RX_LINEAR_MMSE) && !(takes & DMX_FLAG_RX_LINEAR_MMSE)) {
        set_error("DMX_FLAG_RX_LINEAR_MMSE is an option of the dmx_codebook_rate and dmx_codebook_rate_subbands calls and their "
                  "dmx_*_supported queries alone: no other entry point takes it, dmx_path_prep included");
        return DMX_ERR_ARG;
    }
    if ((p->flags & DMX_FLAG_NEAR_FIELD) && (p->flags & DMX_FLAG_SPATIAL_WIDEBAND)) {
        set_error("DMX_FLAG_NEAR_FIELD | DMX_FLAG_SPATIAL_WIDEBAND: the two are not covered together");
        return DMX_ERR_ARG;
    }
    if (p->flags & DMX_FLAG_NEAR_FIELD) {
        if (!(takes & DMX_FLAG_NEAR_FIELD)) {
            set_error("DMX_FLAG_NEAR_FIELD is not taken here: the rx_filter, time-domain, beam-space channel and single-pass kernels "
                      "build plane-wave array responses only");
            return DMX_ERR_ARG;
        }
        if (!(p->carrier_freq > 0) || !std::isfinite(p->carrier_freq)) {
            set_error("DMX_FLAG_NEAR_FIELD needs carrier_freq finite and > 0, got carrier_freq = %g", p->carrier_freq);
            return DMX_ERR_ARG;
        }
        if (!(p->bandwidth > 0) || !std::isfinite(p->bandwidth)) {
            set_error("DMX_FLAG_NEAR_FIELD needs bandwidth finite and > 0, got bandwidth = %g", p->bandwidth);
            return DMX_ERR_ARG;
        }
    }
    if ((p->flags & DMX_FLAG_SPATIAL_WIDEBAND) && !(takes & DMX_FLAG_SPATIAL_WIDEBAND)) {
        set_error("DMX_FLAG_SPATIAL_WIDEBAND is taken by dmx_path_prep and dmx_channels_fd only: no other kernel forms a per-subcarrier "
                  "array response");
        return DMX_ERR_ARG;
    }
    if ((p->flags & ANGLE_DELAY_OUTPUT_FLAGS) && !(takes & DMX_FLAG_ANGLE_DELAY_POWER)) {
        set_error("%s is an option of the dmx_channels_angle_delay call and its dmx_angle_delay_supported query alone: no other "
                  "entry point takes it, dmx_path_prep included",
                  (p->flags & ANGLE_DELAY_OUTPUT_FLAGS) == ANGLE_DELAY_OUTPUT_FLAGS ? "DMX_FLAG_ANGLE_DELAY_POWER | DMX_FLAG_ANGLE_DELAY_PROFILE"
                  : (p->flags & DMX_FLAG_ANGLE_DELAY_POWER)                       ? "DMX_FLAG_ANGLE_DELAY_POWER"
                                                                                  : "DMX_FLAG_ANGLE_DELAY_PROFILE");
        return DMX_ERR_ARG;
    }
    if ((p->flags & ANGLE_DELAY_OUTPUT_FLAGS) == DMX_FLAG_ANGLE_DELAY_PROFILE) {
        set_error("DMX_FLAG_ANGLE_DELAY_PROFILE is valid only together with DMX_FLAG_ANGLE_DELAY_POWER: the profile is the row sum "
                  "of the power matrix");
        return DMX_ERR_ARG;
    }
    if ((p->flags & DMX_FLAG_SERVING_SET) && !(takes & DMX_FLAG_SERVING_SET)) {
        set_error("DMX_FLAG_SERVING_SET is an option of the dmx_cell_rate call and its dmx_cell_rate_supported query alone: no other "
                  "entry point takes it, dmx_path_prep included");
        return DMX_ERR_ARG;
    }
    if (p->freq_domain) {
        if (p->n_subcarriers < 1) { set_error("ofdm.subcarriers must be >= 1"); return DMX_ERR_ARG; }
        if (p->n_selected < 0 || (p->n_selected > 0 && !p->selected_subcarriers)) {
            set_error("selected_subcarriers missing"); return DMX_ERR_ARG;
        }
        if (!(p->bandwidth > 0)) { set_error("ofdm.bandwidth must be > 0"); return DMX_ERR_ARG; }
        if (p->sc_stride < 0) { set_error("sc_stride must be >= 0"); return DMX_ERR_ARG; }
    }
    return DMX_OK;
}

// the float32-phase kernels refuse a promised selection that reaches DMX_SC_ABS_MAX_F32 (their error grows with |k|)
static int check_sc_bound_f32(const dmx_params* p, const char* what) {
    if (!sc_beyond_f32(*p)) return DMX_OK;
    set_error("%s: selected subcarrier |index| %lld reaches DMX_SC_ABS_MAX_F32 = %d, beyond which its float32 phase "
              "misses the error bound; use variant 0, 1 or 9", what, (long long)sc_hint_abs_max(*p), DMX_SC_ABS_MAX_F32);
    return DMX_ERR_ARG;
}

static inline int used_paths(const dmx_params* p, int32_t loaded) { return p->num_paths < loaded ? p->num_paths : loaded; }

// Checks shared by the entry points.  Which of several faults is reported is part of the behaviour: each entry point keeps
// its order of calls (tests/test_host_cpu.py pins return code and message of single and paired faults).
static int check_rays(const dmx_rays* rays) {
    if (!rays) { set_error("rays is NULL"); return DMX_ERR_ARG; }
    if (rays->n_ue < 0 || rays->n_paths < 0 || rays->ld < rays->n_paths) { set_error("bad ray matrix shape"); return DMX_ERR_ARG; }
    if (rays->n_ue > 0 && rays->n_paths > 0 &&
        (!rays->power || !rays->phase || !rays->delay || !rays->aoa_az || !rays->aoa_el || !rays->aod_az ||
         !rays->aod_el || !rays->inter)) {
        set_error("a required ray field pointer is NULL"); return DMX_ERR_ARG;
    }
    return DMX_OK;
}

static int check_user_range(int64_t n_ue, int64_t user_begin, int64_t user_count) {
    if (n_ue < 0 || user_begin < 0 || user_count < 0 || user_begin + user_count > n_ue) {
        set_error("user range [%lld, %lld) outside [0, %lld)", (long long)user_begin, (long long)(user_begin + user_count), (long long)n_ue);
        return DMX_ERR_ARG;
    }
    if (user_count > 0x7fffffffLL) { set_error("too many users for one call"); return DMX_ERR_SHAPE; }
    return DMX_OK;
}

static int check_workspace_aligned(const void* workspace) {
    if (((uintptr_t)workspace & 255u) == 0) return DMX_OK;
    set_error("workspace must be 256-byte aligned"); return DMX_ERR_WORKSPACE;
}
static int check_out_aligned(const void* out) {
    if (((uintptr_t)out & 7u) == 0) return DMX_OK;
    set_error("out must be 8-byte aligned"); return DMX_ERR_ARG;
}

// the beam-space entry points: plain frequency domain within the float32-phase bound, a codebook of at least `min_beams`
static int check_beam_call(const dmx_params* p, const char* entry, const void* codebook, int32_t n_beams, int32_t min_beams) {
    if (!p->freq_domain || p->rx_filter) { set_error("%s needs freq_domain = 1 and rx_filter = 0", entry); return DMX_ERR_ARG; }
    if (int rc = check_sc_bound_f32(p, entry)) return rc;
    if (n_beams < min_beams || (n_beams > 0 && !codebook)) { set_error("codebook missing"); return DMX_ERR_ARG; }
    return DMX_OK;
}

static int check_beam_workspace(int64_t user_count, int32_t n_beams, int P, const void* beam_ws, size_t beam_ws_bytes) {
    const size_t need = beam_workspace_bytes(user_count, n_beams, P);
    if (!beam_ws || beam_ws_bytes < need || ((uintptr_t)beam_ws & 255u)) {
        set_error("beam workspace too small or misaligned: need %zu bytes, 256-byte aligned", need);
        return DMX_ERR_WORKSPACE;
    }
    return DMX_OK;
}

static dmx_side side_or_none(const dmx_side* side) {
    dmx_side s;
    if (side) s = *side; else memset(&s, 0, sizeof(s));
    return s;
}

// ---- the consumers of the per-path records (covariance, rate, spectrum, precoders, cell rate, angle-delay, codebook rate) ----
// An entry point is: consumer_args, its own argument checks, check_snr where it takes one, shape_status of its shape rule, the
// early return without users, carve, launch.  A dmx_*_supported query is `supported` over the same shape rule.

// Before the shape rule: the parameter block, the user range, what the entry point found `missing` (counted only with users
// to run) or `misaligned` among its pointers - the message, or nullptr - around the workspace alignment, and plain frequency
// domain under the entry point's name `fn`.  `takes`: check_params' mask.
static int consumer_args(const char* fn, const dmx_params* prm, const void* workspace, int64_t n_ue, int64_t user_begin,
                         int64_t user_count, const char* missing, const char* misaligned, uint32_t takes = DMX_FLAG_NEAR_FIELD) {
    int rc = check_params(prm, takes);
    if (rc || (rc = check_user_range(n_ue, user_begin, user_count))) return rc;
    if (user_count > 0 && missing) { set_error("%s", missing); return DMX_ERR_ARG; }
    if ((rc = check_workspace_aligned(workspace))) return rc;
    if (misaligned) { set_error("%s", misaligned); return DMX_ERR_ARG; }
    if (!prm->freq_domain) { set_error("%s called with freq_domain = 0", fn); return DMX_ERR_ARG; }
    if (prm->rx_filter) { set_error("%s does not cover rx_filter = 1", fn); return DMX_ERR_ARG; }
    return DMX_OK;
}
static const char* const WS_OUT_NULL = "workspace/out is NULL";

// finite and > 0, and so is its square root in float32 (the kernel's scale of the path coefficients); `what` names the value
static int check_snr(const char* what, double snr_linear) {
    if (snr_linear >= 1e-70 && snr_linear <= 1e70) return DMX_OK;
    set_error("%s must be finite and > 0 (1e-70 .. 1e70), got %g", what, snr_linear);
    return DMX_ERR_ARG;
}

// A shape rule answers 1: taken; 0: not taken, with the limit in the error string; negative: bad argument.
// What a launching entry point returns for that answer:
static int shape_status(int shape) { return shape < 0 ? shape : shape == 0 ? DMX_ERR_SHAPE : DMX_OK; }

// a dmx_*_supported query: the parameter block (`takes`: check_params' mask), then the shape rule
template <class Shape>
static int supported(const dmx_params* prm, Shape shape, uint32_t takes = DMX_FLAG_NEAR_FIELD) {
    const int rc = check_params(prm, takes);
    return rc ? rc : shape();
}

// Steps the shape rules share, each with the words of its feature; 1: passed, 0: not taken.  `who` + " needs ...":
static int shape_plain_fd(const char* who, const dmx_params* p) {
    if (p->freq_domain && !p->rx_filter) return 1;
    set_error("%s needs freq_domain = 1 and rx_filter = 0", who);
    return 0;
}
// *P = min(num_paths, loaded paths), which has to be in 1..32
static int shape_used_paths(const char* feature, const dmx_params* p, int32_t n_paths_loaded, int* P) {
    *P = used_paths(p, n_paths_loaded);
    if (*P >= 1 && *P <= 32) return 1;
    set_error("%s: min(num_paths, loaded paths) = %d is outside the 1..32 paths the kernel supports", feature, *P);
    return 0;
}
static int shape_selected(const char* feature, const dmx_params* p) {
    if (p->n_selected >= 1) return 1;
    set_error("%s: at least one selected subcarrier is needed", feature);
    return 0;
}
// the head of a one-link shape rule: a loaded-path count, plain frequency domain, 1..32 used paths, a subcarrier
static int shape_head(const char* feature, const char* who_fd, const dmx_params* p, int32_t n_paths_loaded, int* P) {
    if (n_paths_loaded < 0) { set_error("n_paths_loaded must be >= 0"); return DMX_ERR_ARG; }
    return shape_plain_fd(who_fd, p) && shape_used_paths(feature, p, n_paths_loaded, P) && shape_selected(feature, p);
}

// the view of the records, carved once the checks have passed
static WsView carve(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded) {
    WsView ws;
    ws_carve(const_cast<void*>(workspace), n_ue, used_paths(prm, n_paths_loaded), &ws);
    return ws;
}

}  // namespace dmx

using namespace dmx;

extern "C" {

int dmx_version(void) { return DMX_ABI_VERSION; }

const char* dmx_last_error(void) { return g_err; }

size_t dmx_workspace_bytes(const dmx_params* prm, int64_t n_ue, int32_t n_paths_loaded) {
    if (!prm || n_ue < 0 || n_paths_loaded < 0) return 0;
    return ws_carve(nullptr, n_ue, used_paths(prm, n_paths_loaded), nullptr);
}

float dmx_decode_max_delay(uint32_t key) {
    if (key == 0) { uint32_t q = 0x7fc00000u; float f; memcpy(&f, &q, 4); return f; }
    uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

int dmx_path_prep(const dmx_rays* rays, const dmx_params* prm, void* workspace, size_t workspace_bytes,
                  const dmx_side* side, void* stream) {
    int rc = check_params(prm, DMX_FLAG_SPATIAL_WIDEBAND | DMX_FLAG_NEAR_FIELD);
    if (rc || (rc = check_rays(rays))) return rc;
    if (rays->n_ue > 0x7fffffffLL * 4) { set_error("too many users for one call"); return DMX_ERR_SHAPE; }
    const int P = used_paths(prm, rays->n_paths);
    const size_t need = ws_carve(nullptr, rays->n_ue, P, nullptr);
    if (need > 0 && (!workspace || workspace_bytes < need)) { set_error("workspace too small: need %zu bytes", need); return DMX_ERR_WORKSPACE; }
    if ((rc = check_workspace_aligned(workspace))) return rc;
    WsView ws;
    ws_carve(workspace, rays->n_ue, P, &ws);
    return launch_path_prep(*rays, *prm, ws, side_or_none(side), (hipStream_t)stream);
}

static int stage2_common(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                         int64_t user_begin, int64_t user_count, void* out, WsView* ws, uint32_t takes = 0) {
    int rc = check_params(prm, takes);
    if (rc || (rc = check_user_range(n_ue, user_begin, user_count))) return rc;
    if (user_count > 0 && (!workspace || !out)) { set_error("workspace/out is NULL"); return DMX_ERR_ARG; }
    if ((rc = check_workspace_aligned(workspace)) || (rc = check_out_aligned(out))) return rc;
    ws_carve(const_cast<void*>(workspace), n_ue, used_paths(prm, n_paths_loaded), ws);
    return DMX_OK;
}

int dmx_channels_fd(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                    int64_t user_begin, int64_t user_count, void* out_c64, int32_t variant, void* stream) {
    WsView ws;
    int rc = stage2_common(prm, workspace, n_ue, n_paths_loaded, user_begin, user_count, out_c64, &ws,
                           DMX_FLAG_SPATIAL_WIDEBAND | DMX_FLAG_NEAR_FIELD);
    if (rc) return rc;
    if (!prm->freq_domain) { set_error("dmx_channels_fd called with freq_domain = 0"); return DMX_ERR_ARG; }
    if (prm->rx_filter) { set_error("rx_filter = 1 is handled by dmx_channels_fd_lpf"); return DMX_ERR_ARG; }
    if (variant < 0 || variant > 12) { set_error("unknown variant %d", variant); return DMX_ERR_ARG; }
    if (prm->flags & DMX_FLAG_SPATIAL_WIDEBAND) {
        if (!(prm->carrier_freq > 0) || !std::isfinite(prm->carrier_freq) || !std::isfinite(prm->bandwidth)) {   // bandwidth > 0: check_params
            set_error("DMX_FLAG_SPATIAL_WIDEBAND needs carrier_freq and bandwidth finite and > 0, got carrier_freq = %g, bandwidth = %g",
                      prm->carrier_freq, prm->bandwidth);
            return DMX_ERR_ARG;
        }
        if (variant > 1) {
            set_error("DMX_FLAG_SPATIAL_WIDEBAND: variant %d refused, only the fp32 vector kernel (variant 0 or 1) forms a "
                      "per-subcarrier array response", variant);
            return DMX_ERR_SHAPE;
        }
    }
    if ((prm->flags & DMX_FLAG_NEAR_FIELD) && variant > 1) {
        set_error("DMX_FLAG_NEAR_FIELD: variant %d refused, only the fp32 vector kernel (variant 0 or 1) builds spherical-wavefront "
                  "array tables", variant);
        return DMX_ERR_SHAPE;
    }
    if (variant >= 2 && variant != 9 && (rc = check_sc_bound_f32(prm, "matrix-core / folded variant"))) return rc;
    if (prm->n_selected == 0) return DMX_OK;
    return launch_channels_fd(*prm, ws, user_begin, user_count, (float2*)out_c64, variant, (hipStream_t)stream);
}

int dmx_fd_kernel_choice(const dmx_params* prm, int32_t n_paths_loaded) {
    if (!prm) { set_error("params is NULL"); return DMX_ERR_ARG; }
    if (n_paths_loaded < 0 || prm->n_selected < 0 || prm->bs_shape[0] < 1 || prm->bs_shape[1] < 1 || prm->ue_shape[0] < 1 ||
        prm->ue_shape[1] < 1) { set_error("bad shape"); return DMX_ERR_SHAPE; }
    if (check_patterns(prm)) return DMX_ERR_ARG;
    if (prm->flags & DMX_FLAG_BEAM_MEAN_POWER) { set_error("DMX_FLAG_BEAM_MEAN_POWER is an option of the dmx_beam_power call alone"); return DMX_ERR_ARG; }
    if (prm->flags & DMX_FLAG_RX_LINEAR_MMSE) {
        set_error("DMX_FLAG_RX_LINEAR_MMSE is an option of the dmx_codebook_rate and dmx_codebook_rate_subbands calls alone");
        return DMX_ERR_ARG;
    }
    if (prm->flags & ANGLE_DELAY_OUTPUT_FLAGS) {
        set_error("DMX_FLAG_ANGLE_DELAY_POWER and DMX_FLAG_ANGLE_DELAY_PROFILE are options of the dmx_channels_angle_delay call alone");
        return DMX_ERR_ARG;
    }
    if (prm->flags & DMX_FLAG_SERVING_SET) { set_error("DMX_FLAG_SERVING_SET is an option of the dmx_cell_rate call alone"); return DMX_ERR_ARG; }
    if (prm->flags & (DMX_FLAG_SPATIAL_WIDEBAND | DMX_FLAG_NEAR_FIELD)) return 1;
    WsView ws{};
    ws.P = used_paths(prm, n_paths_loaded);
    return fd_auto_choice(*prm, ws);
}

int dmx_fd_direct_supported(const dmx_params* prm, int32_t n_paths_loaded) {
    int rc = check_params(prm);
    if (rc) return rc;
    if (n_paths_loaded < 0) { set_error("n_paths_loaded must be >= 0"); return DMX_ERR_ARG; }
    return fd_direct_waves_per_block(*prm, n_paths_loaded) > 0 ? 1 : 0;
}

int dmx_channels_fd_direct(const dmx_rays* rays, const dmx_params* prm, const dmx_side* side,
                           int64_t user_begin, int64_t user_count, void* out_c64, void* stream) {
    int rc = check_params(prm);
    if (rc || (rc = check_rays(rays)) || (rc = check_user_range(rays->n_ue, user_begin, user_count))) return rc;
    if (side && (side->aod_el_rot || side->aod_az_rot || side->aoa_el_rot || side->aoa_az_rot || side->power_linear ||
                 side->power_linear_ant_gain)) {
        set_error("dmx_channels_fd_direct writes fov_mask, num_paths, los and max_delay_key only: rotated angles and powers come "
                  "from dmx_path_prep");
        return DMX_ERR_ARG;
    }
    if (!prm->freq_domain) { set_error("dmx_channels_fd_direct called with freq_domain = 0: call dmx_path_prep + dmx_channels_td"); return DMX_ERR_SHAPE; }
    if (fd_direct_waves_per_block(*prm, rays->n_paths) == 0) {
        set_error("dmx_channels_fd_direct does not take this shape (frequency domain, rx_filter = 0, flags = 0, 1..64 loaded and "
                  "1..32 used paths, at least one subcarrier, tables within the LDS): call dmx_path_prep + dmx_channels_fd");
        return DMX_ERR_SHAPE;
    }
    if (user_count > 0 && !out_c64) { set_error("out is NULL"); return DMX_ERR_ARG; }
    if ((rc = check_out_aligned(out_c64))) return rc;
    return launch_channels_fd_direct(*rays, *prm, side_or_none(side), user_begin, user_count, (float2*)out_c64, (hipStream_t)stream);
}

size_t dmx_lpf_workspace_bytes(const dmx_params* prm, int64_t user_count, int32_t n_paths_loaded) {
    if (!prm || user_count < 0 || n_paths_loaded < 0 || prm->n_selected < 0) return 0;
    return align_up((size_t)user_count * (size_t)used_paths(prm, n_paths_loaded) * (size_t)prm->n_selected * 8, 256);
}

int dmx_channels_fd_lpf(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                        int64_t user_begin, int64_t user_count, void* lpf_workspace, size_t lpf_workspace_bytes,
                        void* out_c64, void* stream) {
    WsView ws;
    int rc = stage2_common(prm, workspace, n_ue, n_paths_loaded, user_begin, user_count, out_c64, &ws);
    if (rc) return rc;
    if (!prm->freq_domain || !prm->rx_filter) { set_error("dmx_channels_fd_lpf needs freq_domain = 1 and rx_filter = 1"); return DMX_ERR_ARG; }
    if (prm->n_selected == 0) return DMX_OK;
    const size_t need = dmx_lpf_workspace_bytes(prm, user_count, n_paths_loaded);
    if (need > 0 && (!lpf_workspace || lpf_workspace_bytes < need || ((uintptr_t)lpf_workspace & 255u))) {
        set_error("lpf workspace too small or misaligned: need %zu bytes, 256-byte aligned", need);
        return DMX_ERR_WORKSPACE;
    }
    return launch_channels_fd_lpf(*prm, ws, user_begin, user_count, (float2*)lpf_workspace, (float2*)out_c64, (hipStream_t)stream);
}

size_t dmx_beam_workspace_bytes(const dmx_params* prm, int64_t user_count, int32_t n_paths_loaded, int32_t n_beams) {
    if (!prm || user_count < 0 || n_paths_loaded < 0 || n_beams < 0) return 0;
    return beam_workspace_bytes(user_count, n_beams, used_paths(prm, n_paths_loaded));
}

int dmx_channels_fd_beams(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                          int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_beams,
                          void* beam_workspace, size_t beam_workspace_bytes_, void* out_c64, void* stream) {
    WsView ws;
    int rc = stage2_common(prm, workspace, n_ue, n_paths_loaded, user_begin, user_count, out_c64, &ws);
    if (rc) return rc;
    if ((rc = check_beam_call(prm, "dmx_channels_fd_beams", codebook_c64, n_beams, 0))) return rc;
    if (prm->n_selected == 0 || n_beams == 0) return DMX_OK;
    if (ws.P > 32) { set_error("num_paths = %d exceeds the 32 paths the beam-space kernel supports", ws.P); return DMX_ERR_SHAPE; }
    if ((rc = check_beam_workspace(user_count, n_beams, ws.P, beam_workspace, beam_workspace_bytes_))) return rc;
    return launch_channels_fd_beams(*prm, ws, user_begin, user_count, (const float2*)codebook_c64, n_beams, beam_workspace,
                                    (float2*)out_c64, (hipStream_t)stream);
}

int dmx_beam_power(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                   int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_beams,
                   void* beam_workspace, size_t beam_workspace_bytes_, float* out_mean_amp, int32_t* out_best_beam,
                   void* stream) {
    WsView ws;
    int rc = stage2_common(prm, workspace, n_ue, n_paths_loaded, user_begin, user_count, out_mean_amp, &ws,
                           DMX_FLAG_NEAR_FIELD | DMX_FLAG_BEAM_MEAN_POWER);
    if (rc) return rc;
    if ((rc = check_beam_call(prm, "dmx_beam_power", codebook_c64, n_beams, 1))) return rc;
    if (prm->n_selected < 1) { set_error("dmx_beam_power needs at least one selected subcarrier"); return DMX_ERR_ARG; }
    if (ws.P > 32) { set_error("num_paths = %d exceeds the 32 paths the beam-space kernels support", ws.P); return DMX_ERR_SHAPE; }
    if ((rc = check_beam_workspace(user_count, n_beams, ws.P, beam_workspace, beam_workspace_bytes_))) return rc;
    return launch_beam_power(*prm, ws, user_begin, user_count, (const float2*)codebook_c64, n_beams, beam_workspace,
                             out_mean_amp, out_best_beam, (hipStream_t)stream);
}

static int covariance_shape(const dmx_params* prm, int32_t n_paths_loaded, int32_t side) {
    if (side != DMX_COV_TX && side != DMX_COV_RX) { set_error("side must be DMX_COV_TX (0) or DMX_COV_RX (1), got %d", side); return DMX_ERR_ARG; }
    int P;
    const int rc = shape_head("covariance", "the covariance", prm, n_paths_loaded, &P);
    if (rc != 1) return rc;
    if (cov_waves_per_block(*prm, P, side, nullptr) == 0) {
        const long long m_tx = (long long)prm->bs_shape[0] * prm->bs_shape[1], m_rx = (long long)prm->ue_shape[0] * prm->ue_shape[1];
        set_error("covariance: one user's tables, (%lld + %lld + %lld + %d + 8) * %d * 8 = %lld bytes, exceed the %zu bytes of LDS "
                  "a wave can get", m_tx, m_rx, side == DMX_COV_TX ? m_tx : m_rx, P, P,
                  (m_tx + m_rx + (side == DMX_COV_TX ? m_tx : m_rx) + P + 8) * P * 8, WAVE_LDS_MAX);
        return 0;
    }
    return 1;
}

int dmx_covariance_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t side) {
    return supported(prm, [&] { return covariance_shape(prm, n_paths_loaded, side); });
}

int dmx_channel_covariance(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                           int64_t user_begin, int64_t user_count, int32_t side, void* out_c64, void* stream) {
    int rc = consumer_args("dmx_channel_covariance", prm, workspace, n_ue, user_begin, user_count,
                           !workspace || !out_c64 ? WS_OUT_NULL : nullptr, (uintptr_t)out_c64 & 7u ? "out must be 8-byte aligned" : nullptr);
    if (rc || (rc = shape_status(covariance_shape(prm, n_paths_loaded, side)))) return rc;
    if (user_count == 0) return DMX_OK;
    return launch_covariance(*prm, carve(prm, workspace, n_ue, n_paths_loaded), user_begin, user_count, side, (float2*)out_c64,
                             (hipStream_t)stream);
}

static int rate_shape(const dmx_params* prm, int32_t n_paths_loaded) {
    int P;
    const int rc = shape_head("rate", "the rate", prm, n_paths_loaded, &P);
    if (rc != 1) return rc;
    const long long m_tx = (long long)prm->bs_shape[0] * prm->bs_shape[1], m_rx = (long long)prm->ue_shape[0] * prm->ue_shape[1];
    const long long m = m_rx <= m_tx ? m_rx : m_tx, big = m_rx <= m_tx ? m_tx : m_rx;
    if (m > 8) {
        set_error("rate: min(M_rx, M_tx) = %lld exceeds the 8 elements of the smaller array the kernel supports", m);
        return 0;
    }
    if (rate_waves_per_block(*prm, P) == 0) {
        const int kc = prm->n_selected < 64 ? prm->n_selected : 64;
        set_error("rate: one user's tables, (%lld + %lld + %d) * %d * 8 = %lld bytes, exceed the %zu bytes of LDS a wave can get",
                  m, big, kc, P, (m + big + kc) * P * 8, WAVE_LDS_MAX);
        return 0;
    }
    return 1;
}

int dmx_rate_supported(const dmx_params* prm, int32_t n_paths_loaded) {
    return supported(prm, [&] { return rate_shape(prm, n_paths_loaded); });
}

int dmx_channel_rate(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                     int64_t user_begin, int64_t user_count, double snr_linear, float* out_rate, float* out_rate_k,
                     void* stream) {
    // float outputs: rows of a float32 tensor are 4-byte aligned
    int rc = consumer_args("dmx_channel_rate", prm, workspace, n_ue, user_begin, user_count,
                           !workspace || !out_rate ? WS_OUT_NULL : nullptr,
                           ((uintptr_t)out_rate | (uintptr_t)out_rate_k) & 3u ? "out_rate / out_rate_k must be 4-byte aligned" : nullptr);
    if (rc || (rc = check_snr("dmx_channel_rate: snr_linear", snr_linear)) || (rc = shape_status(rate_shape(prm, n_paths_loaded)))) return rc;
    if (user_count == 0) return DMX_OK;
    return launch_rate(*prm, carve(prm, workspace, n_ue, n_paths_loaded), user_begin, user_count, snr_linear, out_rate, out_rate_k,
                       (hipStream_t)stream);
}

int dmx_spectrum_supported(const dmx_params* prm, int32_t n_paths_loaded) {
    return dmx_rate_supported(prm, n_paths_loaded);                          // the same kernel body, the same rule
}

int dmx_channel_spectrum(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                         int64_t user_begin, int64_t user_count, double snr_linear, float* out_gamma, float* out_rate,
                         float* out_rate_k, void* stream) {
    int rc = consumer_args("dmx_channel_spectrum", prm, workspace, n_ue, user_begin, user_count,
                           !workspace ? "workspace is NULL" :
                           !out_gamma && !out_rate && !out_rate_k ? "dmx_channel_spectrum: out_gamma, out_rate and out_rate_k are all NULL" : nullptr,
                           ((uintptr_t)out_gamma | (uintptr_t)out_rate | (uintptr_t)out_rate_k) & 3u ?
                               "out_gamma / out_rate / out_rate_k must be 4-byte aligned" : nullptr);
    if (rc || (rc = check_snr("dmx_channel_spectrum: snr_linear", snr_linear)) || (rc = shape_status(rate_shape(prm, n_paths_loaded)))) return rc;
    if (user_count == 0) return DMX_OK;
    return launch_spectrum(*prm, carve(prm, workspace, n_ue, n_paths_loaded), user_begin, user_count, snr_linear, out_gamma, out_rate,
                           out_rate_k, (hipStream_t)stream);
}

// rate_shape and 1 <= n_layers <= min(M_rx, M_tx)
static int precoder_shape(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_layers) {
    const int rc = rate_shape(prm, n_paths_loaded);
    if (rc != 1) return rc;
    const int m_tx = prm->bs_shape[0] * prm->bs_shape[1], m_rx = prm->ue_shape[0] * prm->ue_shape[1];
    const int m = m_rx <= m_tx ? m_rx : m_tx;
    if (n_layers < 1 || n_layers > m) {
        set_error("precoders: n_layers = %d is outside 1..min(M_rx, M_tx) = 1..%d", n_layers, m);
        return 0;
    }
    return 1;
}

int dmx_precoder_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_layers) {
    return supported(prm, [&] { return precoder_shape(prm, n_paths_loaded, n_layers); });
}

int dmx_channel_precoders(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                          int64_t user_begin, int64_t user_count, double snr_linear, int32_t n_layers, float* out_gamma,
                          void* out_tx_c64, void* out_rx_c64, void* stream) {
    int rc = consumer_args("dmx_channel_precoders", prm, workspace, n_ue, user_begin, user_count,
                           !workspace ? "workspace is NULL" :
                           !out_gamma && !out_tx_c64 && !out_rx_c64 ? "dmx_channel_precoders: out_gamma, out_tx_c64 and out_rx_c64 are all NULL" : nullptr,
                           ((uintptr_t)out_gamma & 3u) || (((uintptr_t)out_tx_c64 | (uintptr_t)out_rx_c64) & 7u) ?
                               "out_gamma must be 4-byte aligned, out_tx_c64 / out_rx_c64 8-byte aligned" : nullptr);
    if (rc || (rc = check_snr("dmx_channel_precoders: snr_linear", snr_linear)) ||
        (rc = shape_status(precoder_shape(prm, n_paths_loaded, n_layers)))) return rc;
    if (user_count == 0) return DMX_OK;
    return launch_precoders(*prm, carve(prm, workspace, n_ue, n_paths_loaded), user_begin, user_count, snr_linear, n_layers, out_gamma,
                            (float2*)out_tx_c64, (float2*)out_rx_c64, (hipStream_t)stream);
}

// the links in range of `n_links` (none when the count is not one the kernel takes: the shape rule refuses it)
static int links_in_range(int32_t n_links) { return n_links >= 1 && n_links <= DMX_MAX_LINKS ? n_links : 0; }

// what a link's parameter block may carry: DMX_FLAG_NEAR_FIELD per link, DMX_FLAG_SERVING_SET on every link or on none
static constexpr uint32_t CELL_RATE_TAKES = DMX_FLAG_NEAR_FIELD | DMX_FLAG_SERVING_SET;

// links whose blocks passed check_params
static int check_serving_set_uniform(const dmx_link* links, int n_links) {
    for (int b = 1; b < n_links; ++b) {
        if ((links[b].prm->flags ^ links[0].prm->flags) & DMX_FLAG_SERVING_SET) {
            set_error("DMX_FLAG_SERVING_SET is set on every link of a call or on none: link %d %s it, link 0 %s", b,
                      links[b].prm->flags & DMX_FLAG_SERVING_SET ? "has" : "lacks",
                      links[0].prm->flags & DMX_FLAG_SERVING_SET ? "has it" : "does not");
            return DMX_ERR_ARG;
        }
    }
    return DMX_OK;
}

// every link's parameter block
static int check_link_params(const dmx_link* links, int32_t n_links) {
    if (!links) { set_error("links is NULL"); return DMX_ERR_ARG; }
    for (int b = 0; b < links_in_range(n_links); ++b) {
        if (int rc = check_params(links[b].prm, CELL_RATE_TAKES)) return rc;
    }
    return check_serving_set_uniform(links, links_in_range(n_links));
}

// Every link's params are checked.
static int cell_rate_shape(const dmx_link* links, int32_t n_links) {
    if (!links) { set_error("links is NULL"); return DMX_ERR_ARG; }
    if (!links_in_range(n_links)) {
        set_error("cell rate: n_links = %d is outside the 1..%d links (DMX_MAX_LINKS) the kernel supports", n_links, DMX_MAX_LINKS);
        return 0;
    }
    for (int b = 0; b < n_links; ++b) {
        if (int rc = check_params(links[b].prm, CELL_RATE_TAKES)) return rc;
        if (links[b].n_paths_loaded < 0) { set_error("link %d: n_paths_loaded must be >= 0", b); return DMX_ERR_ARG; }
    }
    if (int rc = check_serving_set_uniform(links, n_links)) return rc;
    const dmx_params* p0 = links[0].prm;
    const long long m_rx = (long long)p0->ue_shape[0] * p0->ue_shape[1];
    for (int b = 0; b < n_links; ++b) {
        const dmx_params* p = links[b].prm;
        char link[48], who[64];
        snprintf(link, sizeof(link), "cell rate: link %d", b);
        snprintf(who, sizeof(who), "%s: the rate", link);
        int P;
        if (!shape_plain_fd(who, p) || !shape_used_paths(link, p, links[b].n_paths_loaded, &P)) return 0;
        if (p->ue_shape[0] != p0->ue_shape[0] || p->ue_shape[1] != p0->ue_shape[1]) {
            set_error("cell rate: link %d has ue_shape %d x %d, link 0 %d x %d: the links must share the UE array", b,
                      p->ue_shape[0], p->ue_shape[1], p0->ue_shape[0], p0->ue_shape[1]);
            return 0;
        }
        if (p->n_subcarriers != p0->n_subcarriers || p->n_selected != p0->n_selected) {
            set_error("cell rate: link %d has %d of %d subcarriers selected, link 0 %d of %d: the links must share n_subcarriers "
                      "and the selection", b, p->n_selected, p->n_subcarriers, p0->n_selected, p0->n_subcarriers);
            return 0;
        }
    }
    if (!shape_selected("cell rate", p0)) return 0;
    if (m_rx > 8) {
        set_error("cell rate: M_rx = %lld exceeds the 8 elements of the UE array the kernel supports", m_rx);
        return 0;
    }
    const int kc = p0->n_selected < 64 ? p0->n_selected : 64;
    for (int b = 0; b < n_links; ++b) {
        const dmx_params* p = links[b].prm;
        const long long m_tx = (long long)p->bs_shape[0] * p->bs_shape[1], P = used_paths(p, links[b].n_paths_loaded);
        if ((unsigned long long)((m_rx + m_tx + kc) * P * 8) > WAVE_LDS_MAX) {
            set_error("cell rate: link %d: one user's tables, (%lld + %lld + %d) * %lld * 8 = %lld bytes, exceed the %zu bytes of LDS "
                      "a wave can get", b, m_rx, m_tx, kc, P, (m_rx + m_tx + kc) * P * 8, WAVE_LDS_MAX);
            return 0;
        }
    }
    return 1;
}

int dmx_cell_rate_supported(const dmx_link* links, int32_t n_links) { return cell_rate_shape(links, n_links); }

int dmx_cell_rate(const dmx_link* links, int32_t n_links, int64_t n_ue, int64_t user_begin, int64_t user_count,
                  const int32_t* serving, float* out_rate, float* out_rate_k, int32_t* out_serving, float* out_link_snr,
                  void* stream) {
    // consumer_args per link: the steps of one kind for every link before the next kind
    int rc = check_link_params(links, n_links);
    if (rc || (rc = check_user_range(n_ue, user_begin, user_count))) return rc;
    if (user_count > 0 && !out_rate) { set_error("%s", WS_OUT_NULL); return DMX_ERR_ARG; }
    const int nb = links_in_range(n_links);
    for (int b = 0; b < nb; ++b) {
        if (user_count > 0 && !links[b].workspace) { set_error("%s", WS_OUT_NULL); return DMX_ERR_ARG; }
        if ((rc = check_workspace_aligned(links[b].workspace))) return rc;
    }
    if (((uintptr_t)serving | (uintptr_t)out_rate | (uintptr_t)out_rate_k | (uintptr_t)out_serving | (uintptr_t)out_link_snr) & 3u) {
        set_error("serving / out_rate / out_rate_k / out_serving / out_link_snr must be 4-byte aligned"); return DMX_ERR_ARG;
    }
    for (int b = 0; b < nb; ++b) {
        if (!links[b].prm->freq_domain) { set_error("dmx_cell_rate called with freq_domain = 0 on link %d", b); return DMX_ERR_ARG; }
        if (links[b].prm->rx_filter) { set_error("dmx_cell_rate does not cover rx_filter = 1 (link %d)", b); return DMX_ERR_ARG; }
        char what[64];
        snprintf(what, sizeof(what), "dmx_cell_rate: snr_linear of link %d", b);
        if ((rc = check_snr(what, links[b].snr_linear))) return rc;
    }
    if ((rc = shape_status(cell_rate_shape(links, n_links)))) return rc;
    if (user_count == 0) return DMX_OK;
    return launch_cell_rate(links, n_links, n_ue, user_begin, user_count, serving, out_rate, out_rate_k, out_serving,
                            out_link_snr, (hipStream_t)stream);
}

static int angle_delay_shape(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_rows, int32_t n_fft, int32_t n_taps) {
    if (n_paths_loaded < 0) { set_error("n_paths_loaded must be >= 0"); return DMX_ERR_ARG; }
    if (!shape_plain_fd("angle-delay:", prm)) return 0;
    if (prm->sc_stride < 1) {                                                // between the steps of shape_head
        set_error("angle-delay: needs a uniformly spaced selection promised by sc_stride > 0 (sc_k = sc_first + k * sc_stride), got "
                  "sc_stride = %d", prm->sc_stride);
        return 0;
    }
    int P;
    if (!shape_used_paths("angle-delay", prm, n_paths_loaded, &P) || !shape_selected("angle-delay", prm)) return 0;
    const long long m_rx = (long long)prm->ue_shape[0] * prm->ue_shape[1];
    if (m_rx > 8) { set_error("angle-delay: M_rx = %lld exceeds the 8 UE elements the kernel supports", m_rx); return 0; }
    if (n_fft < prm->n_selected || n_fft > (1 << 20)) {
        set_error("angle-delay: n_fft = %d is outside n_selected = %d .. 2^20 = 1048576", n_fft, prm->n_selected);
        return 0;
    }
    if (n_taps < 1 || n_taps > n_fft) { set_error("angle-delay: n_taps = %d is outside 1 .. n_fft = %d", n_taps, n_fft); return 0; }
    if (n_rows < 1) { set_error("angle-delay: n_rows = %d, at least one row is needed", n_rows); return 0; }
    if (angle_delay_waves_per_block(*prm, P, n_rows, n_taps) == 0) {
        const int rc = n_rows < 32 ? n_rows : 32, tc = n_taps < 64 ? n_taps : 64;
        set_error("angle-delay: one user's tables, (%lld + %d + %d) * %d * 8 = %lld bytes, exceed the %zu bytes of LDS a wave can get",
                  m_rx, rc, tc, P, (m_rx + rc + tc) * P * 8, WAVE_LDS_MAX);
        return 0;
    }
    return 1;
}

// the angle-delay call and its query take the two output options beside the near field
static constexpr uint32_t ANGLE_DELAY_TAKES = DMX_FLAG_NEAR_FIELD | ANGLE_DELAY_OUTPUT_FLAGS;

int dmx_angle_delay_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_rows, int32_t n_fft, int32_t n_taps) {
    return supported(prm, [&] { return angle_delay_shape(prm, n_paths_loaded, n_rows, n_fft, n_taps); }, ANGLE_DELAY_TAKES);
}

int dmx_channels_angle_delay(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                             int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_rows,
                             void* beam_workspace, size_t beam_workspace_bytes_, int32_t n_fft, int32_t n_taps, void* out_c64,
                             void* stream) {
    int rc = consumer_args("dmx_channels_angle_delay", prm, workspace, n_ue, user_begin, user_count,
                           !workspace || !out_c64 ? WS_OUT_NULL : nullptr,
                           prm && (prm->flags & DMX_FLAG_ANGLE_DELAY_POWER)                          // float32 out
                               ? ((uintptr_t)out_c64 & 3u ? "out must be 4-byte aligned" : nullptr)
                               : ((uintptr_t)out_c64 & 7u ? "out must be 8-byte aligned" : nullptr),
                           ANGLE_DELAY_TAKES);
    if (rc) return rc;
    if (prm->sc_stride < 1) {
        set_error("dmx_channels_angle_delay needs a uniformly spaced selection promised by sc_stride > 0"); return DMX_ERR_ARG;
    }
    const int m_tx = prm->bs_shape[0] * prm->bs_shape[1];
    if (!codebook_c64 && n_rows != m_tx) {
        set_error("dmx_channels_angle_delay: without a codebook the rows are the %d BS elements, got n_rows = %d", m_tx, n_rows);
        return DMX_ERR_ARG;
    }
    if ((rc = shape_status(angle_delay_shape(prm, n_paths_loaded, n_rows, n_fft, n_taps)))) return rc;
    if (user_count == 0) return DMX_OK;
    const WsView ws = carve(prm, workspace, n_ue, n_paths_loaded);
    if (codebook_c64 && (rc = check_beam_workspace(user_count, n_rows, ws.P, beam_workspace, beam_workspace_bytes_))) return rc;
    return launch_angle_delay(*prm, ws, user_begin, user_count, (const float2*)codebook_c64, n_rows, beam_workspace, n_fft, n_taps,
                              (float2*)out_c64, (hipStream_t)stream);
}

static int codebook_rate_shape(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers) {
    int P;
    const int head = shape_head("codebook rate", "codebook rate:", prm, n_paths_loaded, &P);
    if (head != 1) return head;
    const long long m_rx = (long long)prm->ue_shape[0] * prm->ue_shape[1];
    if (m_rx > 8) { set_error("codebook rate: M_rx = %lld exceeds the 8 UE elements the kernel supports", m_rx); return 0; }
    const int l_max = m_rx < 4 ? (int)m_rx : 4;
    if (n_layers < 1 || n_layers > l_max) {
        set_error("codebook rate: n_layers = %d is outside 1..min(M_rx, 4) = 1..%d", n_layers, l_max);
        return 0;
    }
    if (n_codewords < 1 || (long long)n_codewords * n_layers > 65536) {
        set_error("codebook rate: n_codewords = %d with %d layers is outside 1 <= n_codewords, n_codewords * n_layers <= 65536",
                  n_codewords, n_layers);
        return 0;
    }
    if (codebook_rate_waves_per_block(*prm, P, n_codewords, n_layers) == 0) {
        const long long rows = (long long)n_codewords * n_layers, rcm = (long long)n_layers * (32 / n_layers);
        const long long rc = rows < rcm ? rows : rcm, kc = prm->n_selected < 64 ? prm->n_selected : 64;
        set_error("codebook rate: one user's tables, (%lld + %lld + %lld) * %d * 8 = %lld bytes, exceed the %zu bytes of LDS a wave "
                  "can get", m_rx, rc, kc, P, (m_rx + rc + kc) * P * 8, WAVE_LDS_MAX);
        return 0;
    }
    return 1;
}

// the codebook-rate calls and their queries take the receiver option beside the near field
static constexpr uint32_t CODEBOOK_RATE_TAKES = DMX_FLAG_NEAR_FIELD | DMX_FLAG_RX_LINEAR_MMSE;

int dmx_codebook_rate_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers) {
    return supported(prm, [&] { return codebook_rate_shape(prm, n_paths_loaded, n_codewords, n_layers); }, CODEBOOK_RATE_TAKES);
}

// the checks dmx_codebook_rate and dmx_codebook_rate_subbands share, up to the shape; `out` is the output that must not be NULL,
// `out_misaligned` the message when one of the outputs is not 4-byte aligned
static int codebook_rate_args(const char* fn, const dmx_params* prm, const void* workspace, int64_t n_ue, int64_t user_begin,
                              int64_t user_count, const void* codebook_c64, double snr_linear, const void* out,
                              const char* out_misaligned) {
    char snr_name[64];
    snprintf(snr_name, sizeof(snr_name), "%s: snr_linear", fn);
    const int rc = consumer_args(fn, prm, workspace, n_ue, user_begin, user_count,
                                 !workspace || !out ? WS_OUT_NULL : !codebook_c64 ? "codebook missing" : nullptr,
                                 out_misaligned ? out_misaligned : (uintptr_t)codebook_c64 & 7u ? "codebook must be 8-byte aligned" : nullptr,
                                 CODEBOOK_RATE_TAKES);
    return rc ? rc : check_snr(snr_name, snr_linear);
}

int dmx_codebook_rate(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                      int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_codewords, int32_t n_layers,
                      void* beam_workspace, size_t beam_workspace_bytes_, double snr_linear, float* out_rate, int32_t* out_pmi,
                      float* out_rate_c, void* stream) {
    int rc = codebook_rate_args("dmx_codebook_rate", prm, workspace, n_ue, user_begin, user_count,
                                codebook_c64, snr_linear, out_rate,
                                ((uintptr_t)out_rate | (uintptr_t)out_pmi | (uintptr_t)out_rate_c) & 3u ?
                                    "out_rate / out_pmi / out_rate_c must be 4-byte aligned" : nullptr);
    if (rc || (rc = shape_status(codebook_rate_shape(prm, n_paths_loaded, n_codewords, n_layers)))) return rc;
    if (user_count == 0) return DMX_OK;
    const WsView ws = carve(prm, workspace, n_ue, n_paths_loaded);
    if ((rc = check_beam_workspace(user_count, n_codewords * n_layers, ws.P, beam_workspace, beam_workspace_bytes_))) return rc;
    return launch_codebook_rate(*prm, ws, user_begin, user_count, (const float2*)codebook_c64, n_codewords, n_layers,
                                beam_workspace, snr_linear, out_rate, out_pmi, out_rate_c, (hipStream_t)stream);
}

// the shape of dmx_codebook_rate and a subband size >= 1; the subband form keeps min(subband_size, n_selected, 64) subcarriers
// of w in the LDS where the wideband one keeps min(n_selected, 64), so the LDS rule refuses nothing more
static int codebook_rate_subbands_shape(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers,
                                        int32_t subband_size) {
    if (subband_size < 1) { set_error("codebook rate: subband_size = %d must be >= 1", subband_size); return DMX_ERR_ARG; }
    const int rc = codebook_rate_shape(prm, n_paths_loaded, n_codewords, n_layers);
    if (rc != 1) return rc;
    if (codebook_rate_subbands_waves_per_block(*prm, used_paths(prm, n_paths_loaded), n_codewords, n_layers, subband_size) == 0) {
        set_error("codebook rate: one user's tables of the subband form exceed the %zu bytes of LDS a wave can get", WAVE_LDS_MAX);
        return 0;
    }
    return 1;
}

int dmx_codebook_rate_subbands_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers,
                                         int32_t subband_size) {
    return supported(prm, [&] { return codebook_rate_subbands_shape(prm, n_paths_loaded, n_codewords, n_layers, subband_size); },
                     CODEBOOK_RATE_TAKES);
}

int dmx_codebook_rate_subbands(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                               int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_codewords,
                               int32_t n_layers, void* beam_workspace, size_t beam_workspace_bytes_, double snr_linear,
                               int32_t subband_size, float* out_rate_sb, int32_t* out_pmi_sb, float* out_rate_sb_c, float* out_rate,
                               int32_t* out_pmi, float* out_rate_c, void* stream) {
    int rc = codebook_rate_args("dmx_codebook_rate_subbands", prm, workspace, n_ue, user_begin,
                                user_count, codebook_c64, snr_linear, out_rate_sb,
                                ((uintptr_t)out_rate_sb | (uintptr_t)out_pmi_sb | (uintptr_t)out_rate_sb_c | (uintptr_t)out_rate |
                                 (uintptr_t)out_pmi | (uintptr_t)out_rate_c) & 3u ? "the outputs must be 4-byte aligned" : nullptr);
    if (rc || (rc = shape_status(codebook_rate_subbands_shape(prm, n_paths_loaded, n_codewords, n_layers, subband_size)))) return rc;
    if (user_count == 0) return DMX_OK;
    const WsView ws = carve(prm, workspace, n_ue, n_paths_loaded);
    if ((rc = check_beam_workspace(user_count, n_codewords * n_layers, ws.P, beam_workspace, beam_workspace_bytes_))) return rc;
    return launch_codebook_rate_subbands(*prm, ws, user_begin, user_count, (const float2*)codebook_c64, n_codewords, n_layers,
                                         beam_workspace, snr_linear, subband_size, out_rate_sb, out_pmi_sb, out_rate_sb_c, out_rate,
                                         out_pmi, out_rate_c, (hipStream_t)stream);
}

int dmx_channels_td(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                    int64_t user_begin, int64_t user_count, void* out_c64, void* stream) {
    WsView ws;
    int rc = stage2_common(prm, workspace, n_ue, n_paths_loaded, user_begin, user_count, out_c64, &ws);
    if (rc) return rc;
    if (prm->freq_domain) { set_error("dmx_channels_td called with freq_domain = 1"); return DMX_ERR_ARG; }
    return launch_channels_td(*prm, ws, user_begin, user_count, (float2*)out_c64, (hipStream_t)stream);
}

}  // extern "C"
