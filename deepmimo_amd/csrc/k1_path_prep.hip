// Stage 1 - path prep: one lane per path; a wavefront serves two users (32 lanes each) when the
// scenario has at most 32 loaded paths (DeepMIMO's MAX_PATHS is 25), one user otherwise.
//
// Replaces, for all users at once, the vectorised NumPy prologue of Dataset.compute_channels:
//   _rotate_angles_batch        geometry.py:244-319   (via dataset.py:310-356)
//   _apply_FoV_batch            geometry.py:162-195   (via dataset.py:461-512)
//   dbw2watt + AntennaPattern   generator_utils.py:35, ant_patterns.py:21-71, 145-168
//   _compute_num_paths / _los   dataset.py:569-619
//   the k-independent part of OFDM_PathGenerator.generate   channel.py:182-192
//   the array-response phase    geometry.py:85-102
// and emits per-path records (dmx_common.h) with the contributing paths compacted to the front
// of each user's row (wave ballot + prefix popcount), so stage 2 never touches a dead path.
// The per-path arithmetic itself is stage1_path in k1_path_math.h, which the single-pass kernel (k12_fd_direct.hip) runs too.
//
// Numerics follow the reference's dtype flow on purpose (DESIGN.md "numerics"): deg2rad in
// float32, sin/cos of the zenith angle rounded to float32, everything touching the rotation in
// float64, tau/Ts as a float32 division.  This file is compiled with -ffp-contract=off so the
// float64 expressions associate exactly as NumPy evaluates them.  HBM traffic is ~40 B read and
// ~50 B written per path: noise next to stage 2's output stream, so no tuning beyond coalescing
// (lane = path => each field is one contiguous row segment per wave).
#include "dmx_common.h"
#include "k1_path_math.h"
#include <math.h>

namespace dmx {

struct PrepArgs {
    dmx_rays rays;
    dmx_side side;
    WsView ws;
    Stage1Params s1;                       // k1_path_math.h: what the single-pass kernel takes too
    int freq_domain;
    int rx_filter;
    int need_angles;                       // angles wanted as numbers (side outputs, FoV, dipole), not just directions
    int sort_paths;                        // frequency domain: kept paths ordered by falling amplitude (the sum does not care;
                                           // stage 2 drops product terms of a weak last K-step, k2_channel_fd_mfma.hip)
};

// The LEAN forms: nothing needs the angles as numbers (no FoV, isotropic patterns, no angle / power side outputs - what
// compute_channels and bench.py run), so the arccos / atan2 / FoV / dipole code of stage1_path is compiled out, which
// takes the kernel from 228 to far fewer registers, i.e. from 2 to 3-4 waves per SIMD on a kernel that waits on its loads
// and stores.  LPU = lanes per user (32: two users share a wave; 64: one user per wave, any path count).  ZROT: both
// rotations are exactly zero and the same for every user.  The per-path arithmetic is stage1_path (k1_path_math.h); here
// are the passes over a user's paths, the record slots, the workspace writes and the reductions.  The form that does
// need the angles is k1_path_prep_full below.
#ifndef K1_WAVES
#define K1_WAVES 4                                          // waves per workgroup (every wave works alone)
#endif
template <int LPU, bool ZROT = false>
__global__ __launch_bounds__(64 * K1_WAVES, 16 / K1_WAVES) void k1_path_prep(PrepArgs a) {
    constexpr int UPW = 64 / LPU;                           // users per wave
    const int lane = threadIdx.x & (LPU - 1);               // lane inside the user's group
    const int grp = (threadIdx.x & 63) / LPU;               // which group of the wave
    const int64_t u_raw = ((int64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6)) * UPW + grp;
    const bool u_ok = u_raw < a.rays.n_ue;
    if (__ballot(u_ok) == 0ull) return;                     // whole wave past the end
    const int64_t u = u_ok ? u_raw : a.rays.n_ue - 1;       // idle group shadows the last user, writes nothing
    const int L = a.rays.n_paths;
    const size_t wrow = (size_t)u * (size_t)a.s1.P;

    double usx, ucx, usy, ucy, urz;
    stage1_ue_rotation(a.s1, u, usx, ucx, usy, ucy, urz);

    int keep_base = 0;
    Stage1User us;

    for (int j0 = 0; j0 < L; j0 += LPU) {
        const int j = j0 + lane;
        const Stage1Path p = stage1_path<LPU, true, ZROT>(a.s1, a.rays, a.side, a.freq_domain, a.rx_filter, a.need_angles,
                                                          usx, ucx, usy, ucy, urz, u, j, u_ok && j < L, grp, j0 == 0, us);
        const unsigned long long kb = group_mask<LPU>(__ballot(p.keep), grp);
        int rank = 0;
        const bool sorted = a.sort_paths && L <= LPU;          // kernel-uniform; the whole user is in this one pass
        if (sorted) {
            // rank among the kept paths by |c|^2, ties by path index: 0 = strongest.  Lanes that keep nothing carry -1.
            const float key = p.keep ? p.c_re * p.c_re + p.c_im * p.c_im : -1.0f;
            for (int jj = 0; jj < L; ++jj) {
                const float kj = __shfl(key, jj, LPU);
                rank += (kj > key || (kj == key && jj < lane)) ? 1 : 0;
            }
        }
        if (p.keep) {
            const int slot = sorted ? rank : keep_base + __popcll(kb & ((1ull << lane) - 1ull));
            a.ws.c_re[wrow + slot] = p.c_re; a.ws.c_im[wrow + slot] = p.c_im; a.ws.dn[wrow + slot] = p.dn;
            a.ws.tx_y[wrow + slot] = p.ty; a.ws.tx_z[wrow + slot] = p.tz;
            a.ws.rx_y[wrow + slot] = p.ry; a.ws.rx_z[wrow + slot] = p.rz;
            a.ws.dop_v[wrow + slot] = p.dvel;                                    // 0 without Doppler; `keep` lanes are `in` lanes
            a.ws.dop_a[wrow + slot] = p.dacc;
        }
        keep_base += __popcll(kb);
    }

    // wave reductions
    float maxd = us.maxd;
    for (int off = LPU / 2; off > 0; off >>= 1) maxd = fmaxf(maxd, __shfl_xor(maxd, off, LPU));
    const bool anyd = group_mask<LPU>(__ballot(us.any_delay), grp) != 0ull;
    if (lane == 0 && u_ok) {
        a.ws.n_keep[u] = keep_base;
        stage1_user_out(a.side, a.s1.fov_enabled, u, us, maxd, anyd);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The FULL form (something needs the angles as numbers) is deliberately NOT on the shared body: on stage1_path its two
// instantiations ran 1.4 - 1.9 % longer than before at the same occupancy, beyond the spread, and
// the cause was not found in the disassembly.  It keeps its own argument struct and the inline loop body it had; whatever
// changes in stage1_path (k1_path_math.h) has to be made here too, and tests/test_gpu_fd_direct.py (the FoV and dipole
// cases run k12_fd_direct's MODE 0 = stage1_path against this kernel, torch.equal) notices if it is not.
struct PrepArgsFull {
    dmx_rays rays;
    dmx_side side;
    WsView ws;
    // rotation
    double bsx, csx, bsy, csy, brz;       // sin/cos of BS rotation about x, y; rotation about z (rad)
    double usx, ucx, usy, ucy, urz;       // same for a constant UE rotation
    const double* ue_rot_pu;              // [n,3] degrees or nullptr
    // fov
    int fov_enabled, bs_restricted, ue_restricted;
    double bs_fh, bs_fv, ue_fh, ue_fv;    // radians
    int bs_pat, ue_pat;
    double bs_spacing, ue_spacing;
    int P;                                 // paths used for the channel
    int freq_domain;
    int n_sc;
    float ts32;                            // float32(1/bandwidth)
    int doppler;
    int rx_filter;
    int need_angles;                       // angles wanted as numbers (side outputs, FoV, dipole), not just directions
    int sort_paths;                        // frequency domain: kept paths ordered by falling amplitude (the sum does not care;
                                           // stage 2 drops product terms of a weak last K-step, k2_channel_fd_mfma.hip)
    double fc;
};

// SECTOR: a side has the TR 38.901 sector element (DMX_PATTERN_TR38901).  An instantiation of its own, because with the
// branch in the one body the dipole and FoV launches ran 1.6 - 2.2 % longer at 200k users (222 instead of 202 registers,
// the same two waves per SIMD; profiles/README.md, r12): without it the body compiles to the instructions it had.
template <int LPU, bool SECTOR = false>
__global__ __launch_bounds__(64 * K1_WAVES, 8 / K1_WAVES) void k1_path_prep_full(PrepArgsFull a) {
    constexpr bool LEAN = false, ZROT = false;
    constexpr int UPW = 64 / LPU;                           // users per wave
    const int lane = threadIdx.x & (LPU - 1);               // lane inside the user's group
    const int grp = (threadIdx.x & 63) / LPU;               // which group of the wave
    const int64_t u_raw = ((int64_t)blockIdx.x * K1_WAVES + (threadIdx.x >> 6)) * UPW + grp;
    const bool u_ok = u_raw < a.rays.n_ue;
    if (__ballot(u_ok) == 0ull) return;                     // whole wave past the end
    const int64_t u = u_ok ? u_raw : a.rays.n_ue - 1;       // idle group shadows the last user, writes nothing
    const dmx_rays& r = a.rays;
    const int L = r.n_paths;
    const size_t row = (size_t)u * (size_t)r.ld;
    const size_t srow = (size_t)u * (size_t)L;              // dense side-product rows
    const size_t wrow = (size_t)u * (size_t)a.P;

    double usx = a.usx, ucx = a.ucx, usy = a.usy, ucy = a.ucy, urz = a.urz;
    if (a.ue_rot_pu) {                                      // per-user rotation in degrees (dataset.py:329-338)
        const double rx = a.ue_rot_pu[3 * u + 0] * D2R_D, ry = a.ue_rot_pu[3 * u + 1] * D2R_D;
        urz = a.ue_rot_pu[3 * u + 2] * D2R_D;
        sincos(rx, &usx, &ucx);
        sincos(ry, &usy, &ucy);
    }
    const bool iso = (a.bs_pat == DMX_PATTERN_ISOTROPIC) && (a.ue_pat == DMX_PATTERN_ISOTROPIC);
    const float nan32 = __int_as_float(0x7fc00000);
    const double nan64 = (double)nan32;

    int keep_base = 0, count_paths = 0;
    bool has_fov_path = false;
    float first_inter = nan32;
    float maxd = -INFINITY;
    bool any_delay = false;

    for (int j0 = 0; j0 < L; j0 += LPU) {
        const int j = j0 + lane;
        const bool in = u_ok && j < L;
        // Eight loads issued TOGETHER, from an index every lane may read (idle lanes: the user's last path), masked
        // afterwards.  Written as `in ? array[row + j] : nan`, each load sat alone in a branch of its own with an
        // `s_waitcnt vmcnt(0)` behind it: eight memory round trips in a row were the 8 us a wave lived (SQ_WAVE_CYCLES /
        // SQ_WAVES, profiles/r3_d8_summary.txt) and 0.20-0.28 ms of stage 1 per 200k users.
        const size_t jc = row + (size_t)(j < L ? j : L - 1);
        const float power_r = r.power[jc], phase_r = r.phase[jc], delay_r = r.delay[jc], aoa_az_r = r.aoa_az[jc];
        const float aoa_el_r = r.aoa_el[jc], aod_az_r = r.aod_az[jc], aod_el_r = r.aod_el[jc], inter_r = r.inter[jc];
        const bool dop_rays = a.doppler && r.doppler_vel && r.doppler_acc;       // kernel-uniform
        float dvel_r = 0.f, dacc_r = 0.f;
        if (dop_rays) { dvel_r = r.doppler_vel[jc]; dacc_r = r.doppler_acc[jc]; }    // in the same batch
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
        // arccos is NaN outside [-1, 1]; np.angle is NaN only for NaN input
        double th_t = (isnan(zc_t) || fabs(zc_t) > 1.0) ? nan64 : 0.0, ph_t = (isnan(re_t) || isnan(im_t)) ? nan64 : 0.0;
        double th_r = (isnan(zc_r) || fabs(zc_r) > 1.0) ? nan64 : 0.0, ph_r = (isnan(re_r) || isnan(im_r)) ? nan64 : 0.0;
        if constexpr (!LEAN) {
            if (a.need_angles) {                             // wave-uniform
                th_t = acos(zc_t); ph_t = np_angle(re_t, im_t);
                th_r = acos(zc_r); ph_r = np_angle(re_r, im_r);
            }
            if (in) {
                if (a.side.aod_el_rot) a.side.aod_el_rot[srow + j] = th_t;
                if (a.side.aod_az_rot) a.side.aod_az_rot[srow + j] = ph_t;
                if (a.side.aoa_el_rot) a.side.aoa_el_rot[srow + j] = th_r;
                if (a.side.aoa_az_rot) a.side.aoa_az_rot[srow + j] = ph_r;
            }
        }

        // field of view (dataset.py:493-511): outside -> angles become NaN
        bool mask = true;
        if (!LEAN && a.fov_enabled) {
            if (a.bs_restricted) mask = mask && in_fov(th_t, ph_t, a.bs_fh, a.bs_fv);
            if (a.ue_restricted) mask = mask && in_fov(th_r, ph_r, a.ue_fh, a.ue_fv);
            mask = mask && in;
            if (in && a.side.fov_mask) a.side.fov_mask[srow + j] = mask ? 1 : 0;
            if (!mask) { th_t = nan64; ph_t = nan64; th_r = nan64; ph_r = nan64; }
            const unsigned long long mb = group_mask<LPU>(__ballot(mask), grp);
            // first in-FoV path (dataset.py:594-598); the shuffle is executed by every lane, the
            // result is kept only by groups that had no in-FoV path yet
            const int src = mb != 0ull ? __ffsll((long long)mb) - 1 : 0;
            const float cand = __shfl(inter, src, LPU);
            if (!has_fov_path && mb != 0ull) { has_fov_path = true; first_inter = cand; }
        } else if (j0 == 0) {
            first_inter = __shfl(inter, 0, LPU);             // dataset.py:602
        }
        count_paths += __popcll(group_mask<LPU>(__ballot(in && !isnan(ph_r)), grp));   // dataset.py:616-619

        // powers (generator_utils.py:35, ant_patterns.py:167-168)
        const float p10 = power / 10.0f;
        const float pl = exp10f(p10);                        // float32 pow, as NumPy evaluates 10**float32
        double pw;
        if (LEAN || iso) {
            pw = (double)pl;
        } else {
            const double gt = a.bs_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_t)
                              : ((SECTOR && a.bs_pat == DMX_PATTERN_TR38901) ? tr38901_gain(th_t, ph_t) : 1.0);
            const double gr = a.ue_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_r)
                              : ((SECTOR && a.ue_pat == DMX_PATTERN_TR38901) ? tr38901_gain(th_r, ph_r) : 1.0);
            pw = (double)pl * (gt * gr);
        }
        if constexpr (!LEAN) {
            if (in) {
                if (a.side.power_linear) a.side.power_linear[srow + j] = pl;
                if (a.side.power_linear_ant_gain) a.side.power_linear_ant_gain[srow + j] = pw;
            }
        }

        // per-path record for the first P paths (dataset.py:258-261)
        const bool used = in && j < a.P;
        if (used && !isnan(delay)) { maxd = fmaxf(maxd, delay); any_delay = true; }
        const bool valid = used && !isnan(pw);               // channel.py:260
        const float ph32 = phase * D2R_F;                    // np.deg2rad(float32)
        float e_re, e_im;
        np_sincosf(ph32, e_im, e_re);                        // complex64 exp: NumPy's float32 cos / sin (and NaN-cheap, see there)
        const bool ang_ok = !isnan(th_t) && !isnan(th_r);    // geometry.py:65 zeroes NaN-zenith columns
        float c_re, c_im, dn = 0.0f;
        bool keep;
        if (a.freq_domain) {
            dn = delay / a.ts32;                             // float32 / float32 (channel.py:183)
            double pwc = pw;
            if (dn >= (float)a.n_sc) { pwc = 0.0; dn = (float)a.n_sc; }   // channel.py:187-189
            if (LEAN || iso) {
                const float amp = sqrtf((float)pwc / (float)a.n_sc);      // float32 (channel.py:192)
                c_re = amp * e_re; c_im = amp * e_im;
            } else {
                const double amp = sqrt(pwc / (double)a.n_sc);
                c_re = (float)(amp * (double)e_re); c_im = (float)(amp * (double)e_im);
            }
            if (dop_rays && !a.rx_filter) {                                      // construct_deepmimo.py:267-280
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
            // nansum (channel.py:283): a path with any NaN factor contributes nothing
            keep = valid && ang_ok && !isnan(ph_t) && !isnan(ph_r) && !isnan(c_re) && !isnan(c_im) && !isnan(dn) &&
                   (c_re != 0.0f || c_im != 0.0f);          // clipped / zero-gain paths add exactly 0
        } else {
            if (LEAN || iso) {
                const float amp = sqrtf((float)pw);                        // channel.py:286
                c_re = amp * e_re; c_im = amp * e_im;
            } else {
                const double amp = sqrt(pw);
                c_re = (float)(amp * (double)e_re); c_im = (float)(amp * (double)e_im);
            }
            if (!ang_ok) { c_re *= 0.0f; c_im *= 0.0f; }                   // zero array response, NaN stays NaN
            keep = valid;                                                  // slot even if coefficient is 0
        }
        double ty = 0.0, tz = 0.0, ry = 0.0, rz = 0.0;
        if (ang_ok && ZROT) {
            ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * sphi_t); tz = a.bs_spacing * zc_t;
            ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * sphi_r); rz = a.ue_spacing * zc_r;
        } else if (ang_ok) {                                 // geometry.py:99-101 in revolutions (kd / 2pi = spacing)
            const double rho_t = sqrt(re_t * re_t + im_t * im_t), rho_r = sqrt(re_r * re_r + im_r * im_r);
            ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * (rho_t > 0.0 ? im_t / rho_t : 0.0)); tz = a.bs_spacing * zc_t;
            ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * (rho_r > 0.0 ? im_r / rho_r : 0.0)); rz = a.ue_spacing * zc_r;
        }
        const unsigned long long kb = group_mask<LPU>(__ballot(keep), grp);
        int rank = 0;
        const bool sorted = a.sort_paths && L <= LPU;          // kernel-uniform; the whole user is in this one pass
        if (sorted) {
            // rank among the kept paths by |c|^2, ties by path index: 0 = strongest.  Lanes that keep nothing carry -1.
            const float key = keep ? c_re * c_re + c_im * c_im : -1.0f;
            for (int jj = 0; jj < L; ++jj) {
                const float kj = __shfl(key, jj, LPU);
                rank += (kj > key || (kj == key && jj < lane)) ? 1 : 0;
            }
        }
        if (keep) {
            const int slot = sorted ? rank : keep_base + __popcll(kb & ((1ull << lane) - 1ull));
            a.ws.c_re[wrow + slot] = c_re; a.ws.c_im[wrow + slot] = c_im; a.ws.dn[wrow + slot] = dn;
            a.ws.tx_y[wrow + slot] = ty; a.ws.tx_z[wrow + slot] = tz;
            a.ws.rx_y[wrow + slot] = ry; a.ws.rx_z[wrow + slot] = rz;
            a.ws.dop_v[wrow + slot] = dvel_r;                                    // 0 without Doppler; `keep` lanes are `in` lanes
            a.ws.dop_a[wrow + slot] = dacc_r;
        }
        keep_base += __popcll(kb);
    }

    // wave reductions
    for (int off = LPU / 2; off > 0; off >>= 1) maxd = fmaxf(maxd, __shfl_xor(maxd, off, LPU));
    const bool anyd = group_mask<LPU>(__ballot(any_delay), grp) != 0ull;
    if (lane == 0 && u_ok) {
        a.ws.n_keep[u] = keep_base;
        if (a.side.num_paths) a.side.num_paths[u] = count_paths;
        if (a.side.los) {
            const bool has = a.fov_enabled ? has_fov_path : (count_paths > 0);
            a.side.los[u] = has ? ((first_inter == 0.0f) ? 1 : 0) : -1;    // dataset.py:604-609
        }
        // one running maximum for the whole launch: a returning atomic per user would serialise 1e5 updates on
        // one L2 word (~88 per us), so look first (relaxed, L2-served) and only update when this user raises it
        if (a.side.max_delay_key && anyd) {
            const uint32_t key = float_order_key(maxd);
            if (key > __hip_atomic_load(a.side.max_delay_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(a.side.max_delay_key, key);
        }
    }
}

int launch_path_prep(const dmx_rays& rays, const dmx_params& prm, const WsView& ws, const dmx_side& side,
                     hipStream_t stream) {
    if (rays.n_ue == 0) return DMX_OK;
    const Stage1Params s1 = stage1_params(prm, ws.P);
    const int rx_filter = prm.rx_filter && prm.freq_domain;
    // amplitude order only where something uses it: the opt-in adaptive precision of stage 2 (frequency domain; the
    // time-domain slots keep the path order, channel.py:285-287).  25 lane shuffles per user otherwise saved.
    const int sort_paths = (prm.freq_domain && (prm.flags & DMX_FLAG_ADAPTIVE_TERMS)) ? 1 : 0;
    const int need_angles = stage1_need_angles(prm, side);
    const Stage1Form form = stage1_form(prm, side, rays.n_paths);            // k1_path_math.h: shared with the single pass
    const bool two = rays.n_paths <= 32;                                     // two users per wave
    const int upb = (two ? 2 : 1) * K1_WAVES;
    const dim3 grid((unsigned)((rays.n_ue + upb - 1) / upb)), block(64 * K1_WAVES);
    if (form == STAGE1_FULL) {
        PrepArgsFull a;
        a.rays = rays; a.side = side; a.ws = ws;
        a.bsx = s1.bsx; a.csx = s1.csx; a.bsy = s1.bsy; a.csy = s1.csy; a.brz = s1.brz;
        a.usx = s1.usx; a.ucx = s1.ucx; a.usy = s1.usy; a.ucy = s1.ucy; a.urz = s1.urz;
        a.ue_rot_pu = s1.ue_rot_pu;
        a.fov_enabled = s1.fov_enabled; a.bs_restricted = s1.bs_restricted; a.ue_restricted = s1.ue_restricted;
        a.bs_fh = s1.bs_fh; a.bs_fv = s1.bs_fv; a.ue_fh = s1.ue_fh; a.ue_fv = s1.ue_fv;
        a.bs_pat = s1.bs_pat; a.ue_pat = s1.ue_pat;
        a.bs_spacing = s1.bs_spacing; a.ue_spacing = s1.ue_spacing;
        a.P = s1.P; a.freq_domain = prm.freq_domain; a.n_sc = s1.n_sc; a.ts32 = s1.ts32;
        a.doppler = s1.doppler; a.rx_filter = rx_filter; a.need_angles = need_angles; a.sort_paths = sort_paths; a.fc = s1.fc;
        if (s1.bs_pat == DMX_PATTERN_TR38901 || s1.ue_pat == DMX_PATTERN_TR38901)
            return launch_dyn_lds(two ? k1_path_prep_full<32, true> : k1_path_prep_full<64, true>, "k1_path_prep", grid, block, 0, LDS_NO_RAISE, stream, a);
        return launch_dyn_lds(two ? k1_path_prep_full<32> : k1_path_prep_full<64>, "k1_path_prep", grid, block, 0, LDS_NO_RAISE, stream, a);
    }
    PrepArgs a;
    a.rays = rays; a.side = side; a.ws = ws; a.s1 = s1;
    a.freq_domain = prm.freq_domain; a.rx_filter = rx_filter; a.need_angles = need_angles; a.sort_paths = sort_paths;
    const auto lean = !two ? k1_path_prep<64> : (form == STAGE1_LEAN_ZROT ? k1_path_prep<32, true> : k1_path_prep<32>);
    return launch_dyn_lds(lean, "k1_path_prep", grid, block, 0, LDS_NO_RAISE, stream, a);
}

}  // namespace dmx
