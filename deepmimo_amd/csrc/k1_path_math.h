// Per-path arithmetic of stage 1, shared by k1_path_prep.hip and the single-pass kernel k12_fd_direct.hip: the
// constants, NumPy's float32 sin / cos, the float64 rotation, the field-of-view test, the dipole and sector-element gains, the small
// ballot helpers, and on top of them stage1_path - the whole per-path body from the ray loads to the record values -
// with the lane-0 epilogue stage1_user_out.  Every function is __forceinline__ and follows the reference's dtype flow;
// the including file decides the FMA contraction: both k1_path_prep.hip and k12_fd_direct.hip are compiled with
// -ffp-contract=off (Makefile), so both kernels evaluate the very same operations.  Stage1Params / stage1_params and
// stage1_form are what both launchers pass and pick.
#pragma once
#include "dmx_common.h"
#include <math.h>

namespace dmx {

static constexpr float D2R_F = 0.017453292519943295f;       // float32(pi/180): np.deg2rad on float32
static constexpr double D2R_D = 0.017453292519943295;       // np.deg2rad on float64
static constexpr double TWO_PI = 6.283185307179586;
static constexpr double HALF_PI = 1.5707963267948966;
static constexpr double LIGHTSPEED = 299792458.0;           // deepmimo_v3/consts.py:112

// NumPy's float32 sin / cos (the SIMD loops np.sin / np.cos dispatch to for float32 arrays on x86
// with FMA): Cody-Waite reduction by pi/2 in three float32 constants, degree-9 / degree-8 minimax
// polynomials, all in float32 FMAs.  The zenith sin/cos feed arccos / atan2, which amplify a
// 1-ulp float32 difference by 1/sin(zenith) towards the rotated poles, so K1 reproduces that
// routine operation for operation; validated bit-for-bit against np.sin / np.cos on 2e6 inputs
// (tests/test_oracle_golden.py::test_numpy_f32_sincos_model).  |x| beyond the routine's range
// (7e4) falls back to sinf / cosf like NumPy falls back to libm.
__device__ __forceinline__ void np_sincosf(float x, float& s_out, float& c_out) {
    // NaN - "no path": the padding lanes of every wave and most paths of a ray-traced user - must take the polynomial (it
    // propagates NaN like np.sin does), not this branch: the wave would execute libm's large-argument sinf AND cosf for it
    if (fabsf(x) > 71476.0625f) { s_out = sinf(x); c_out = cosf(x); return; }
    float q = x * 0x1.45f306p-1f;
    q = (q + 0x1.8p+23f) - 0x1.8p+23f;                       // round to nearest integer
    float r = fmaf(q, -0x1.921fb0p+00f, x);
    r = fmaf(q, -0x1.5110b4p-22f, r);
    r = fmaf(q, -0x1.846988p-48f, r);
    const float r2 = r * r;
    float sp = fmaf(0x1.7d3bbcp-19f, r2, -0x1.a06bbap-13f);
    sp = fmaf(sp, r2, 0x1.11119ap-07f);
    sp = fmaf(sp, r2, -0x1.555556p-03f);
    sp = fmaf(sp, r2, 0.0f);
    sp = fmaf(sp, r, r);
    float cp = fmaf(0x1.98e616p-16f, r2, -0x1.6c06dcp-10f);
    cp = fmaf(cp, r2, 0x1.55553cp-05f);
    cp = fmaf(cp, r2, -0.5f);
    cp = fmaf(cp, r2, 1.0f);
    const int iq = (int)q;
    const int iqc = iq + 1;
    float sv = (iq & 1) ? cp : sp;
    float cv = (iqc & 1) ? cp : sp;
    s_out = (iq & 2) ? -sv : sv;
    c_out = (iqc & 2) ? -cv : cv;
}

// float64 sin / cos for the LEAN instantiations (nothing but the channel depends on them: no angle output, no FoV
// compare, no dipole gain - those keep the library call, whose last-bit behaviour the FoV masks were validated with).
// Cody-Waite reduction by pi/2 in two constants (exact for |k| < 2^20) and the fdlibm kernels: 2.2e-16 against long
// double on 2e7 arguments.  |x| >= 1e5 (never an angle in degrees times pi/180) takes the library call; NaN - the padding
// lanes of every wave - must NOT: a first version sent NaN there too and every wave executed both forms.
__device__ __forceinline__ void sincos_lean(double x, double& s_out, double& c_out) {
    if (fabs(x) >= 1.0e5) { sincos(x, &s_out, &c_out); return; }
    const double k = rint(x * 6.36619772367581382433e-01);
    double r = __builtin_fma(-k, 1.57079632673412561417e+00, x);
    r = __builtin_fma(-k, 6.07710050650619224932e-11, r);
    const double z = r * r;
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    const double sn = __builtin_fma(r * z, ps, r);
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double cs = __builtin_fma(z * z, pc, __builtin_fma(z, -0.5, 1.0));
    const int q = (int)k;                                    // NaN -> 0: the NaN of sn / cs goes through
    const double sv = (q & 1) ? cs : sn, cv = (q & 1) ? sn : cs;
    s_out = (q & 2) ? -sv : sv;
    c_out = ((q + 1) & 2) ? -cv : cv;
}

// geometry.py:284-310 for one path: the rotated direction as (cos zenith', re, im) with
//   zenith' = arccos(zc)  (geometry.py:305-306),  azimuth' = angle(re + j im)  (geometry.py:308-310).
// The angles themselves are only materialised when something needs them (side outputs, FoV, dipole
// pattern); the array-response steps use sin(zenith') = sqrt(1 - zc^2), sin(azimuth') = im / |re + j im|
// and cos(zenith') = zc, which are the same numbers without three float64 trig calls per array side.
template <bool LEAN>
__device__ __forceinline__ void rotate_dir(float el_deg, float az_deg, double sx, double cx, double sy,
                                           double cy, double rz, double& zc, double& re, double& im) {
    const float th32 = el_deg * D2R_F;
    const float ph32 = az_deg * D2R_F;
    float st32, ct32;
    np_sincosf(th32, st32, ct32);                           // np.sin / np.cos of float32 stay float32
    const double st = (double)st32, ct = (double)ct32;
    const double d = (double)ph32 - rz;
    double sd, cd;
    if constexpr (LEAN) {
        sincos_lean(d, sd, cd);
    } else {
        // the library call on a finite stand-in for NaN ("no path": padding lanes, most paths of a ray-traced user), so that
        // no wave walks its large-argument reduction for them; finite arguments get the very same bits as before
        const bool bad = isnan(d);
        sincos(bad ? 0.0 : d, &sd, &cd);
        if (bad) { sd = d; cd = d; }
    }
    zc = cy * cx * ct + st * (sy * cx * cd - sx * sd);
    re = cy * st * cd - sy * ct;
    im = cy * sx * ct + st * (sy * sx * cd + cx * sd);
}

// The same for an EXACTLY zero rotation (DeepMIMO's default, channel.py:36-46): with sin = 0 and cos = 1 every product of
// geometry.py:294-310 that carries a rotation term is an exact zero and the sums are exact, so
//   zc = cos(zenith),  re = sin(zenith) cos(azimuth),  im = sin(zenith) sin(azimuth)
// are the very numbers the general expressions give (NaN inputs propagate the same way) - 4 float64 operations instead
// of 20.  sphi = sin(azimuth') = im / |re + j im| is sign(sin zenith) sin(azimuth) up to the 1e-16 by which the float64
// sin / cos pair misses the unit circle (the general path divides by that norm): no square root, no division.
__device__ __forceinline__ void rotate_dir_zero(float el_deg, float az_deg, double& zc, double& re, double& im, double& sphi) {
    const float th32 = el_deg * D2R_F;
    const float ph32 = az_deg * D2R_F;
    float st32, ct32;
    np_sincosf(th32, st32, ct32);
    const double st = (double)st32, ct = (double)ct32;
    double sd, cd;
    sincos_lean((double)ph32, sd, cd);
    zc = isnan(sd) ? sd : ct;
    re = st * cd;
    im = st * sd;
    sphi = st > 0.0 ? sd : (st < 0.0 ? -sd : 0.0);
}

// np.angle(re + 1j * im) (geometry.py:308-310), zeros included.  Building the complex number is arithmetic: 1j * im has the
// real part 0 * im - 1 * 0, which is -0 for a negative (or -0) im and +0 otherwise, and the imaginary part 0 + im, so an
// im of -0 becomes +0 and a re of -0 becomes +0 unless im carries a sign.  Plain atan2(im, re) differs exactly there: on
// the branch cut (im = -0, re < 0: -pi instead of +pi, e.g. zero rotation, azimuth 0, elevation 180) and at a pole (re = -0,
// im = +0: pi instead of 0, e.g. elevation 0 with cos(azimuth) < 0), where the FoV test then sees another azimuth.
__device__ __forceinline__ double np_angle(double re, double im) {
    return atan2(im + 0.0, signbit(im) ? re : re + 0.0);
}

// np.mod(x, 2pi): result takes the sign of the divisor
__device__ __forceinline__ double pymod_2pi(double x) {
    double m = fmod(x, TWO_PI);
    if (m != 0.0) { if (m < 0.0) m += TWO_PI; } else { m = 0.0; }
    return m;
}

// geometry.py:180-193
__device__ __forceinline__ bool in_fov(double th, double ph, double fh, double fv) {
    const double t = pymod_2pi(th), p = pymod_2pi(ph);
    const bool az = (p <= 0 + fh / 2) || (p >= TWO_PI - fh / 2);
    const bool el = (t <= HALF_PI + fv / 2) && (t >= HALF_PI - fv / 2);
    return az && el;
}

// ant_patterns.py:34-71 (NaN -> 0)
__device__ __forceinline__ double dipole_gain(double th) {
    const double s = sin(th);
    if (!(fabs(s) > 1e-10)) return 0.0;
    const double c = cos(HALF_PI * cos(th));
    return 1.643 * (c * c / s);
}

// The sector element of 3GPP TR 38.901 Table 7.3-1 (DMX_PATTERN_TR38901) on the rotated, FoV-masked angles: boresight at
// zenith pi/2, azimuth 0, 65 degree beamwidths, 8 dBi, each cut and their sum capped at 30 dB.  Linear power gain in
// float64; NaN (no path, or masked by the FoV) -> 0 like the dipole's - fmin would drop the NaN, so it is tested.
static constexpr double TR38901_BW = 65.0 * D2R_D;
__device__ __forceinline__ double tr38901_gain(double th, double ph) {
    if (isnan(th) || isnan(ph)) return 0.0;
    const double v = (th - HALF_PI) / TR38901_BW, h = ph / TR38901_BW;
    const double av = fmin(12.0 * (v * v), 30.0), ah = fmin(12.0 * (h * h), 30.0);
    return exp10((8.0 - fmin(av + ah, 30.0)) / 10.0);
}

// the bits of a 64-lane ballot that belong to group `grp` of LPU lanes, shifted down to bit 0
template <int LPU>
__device__ __forceinline__ unsigned long long group_mask(unsigned long long b, int grp) {
    if constexpr (LPU == 64) return b;
    else return (b >> (grp * LPU)) & ((1ull << LPU) - 1ull);
}

__device__ __forceinline__ uint32_t float_order_key(float f) {
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Stage 1's parameters as both kernels take them (PrepArgs of k1_path_prep.hip and DirectArgs of k12_fd_direct.hip embed it)
struct Stage1Params {
    double bsx, csx, bsy, csy, brz;       // sin/cos of BS rotation about x, y; rotation about z (rad)
    double usx, ucx, usy, ucy, urz;       // same for a constant UE rotation
    const double* ue_rot_pu;              // [n,3] degrees or nullptr
    int fov_enabled, bs_restricted, ue_restricted;
    double bs_fh, bs_fv, ue_fh, ue_fv;    // radians
    int bs_pat, ue_pat;
    double bs_spacing, ue_spacing;
    int P;                                // paths used for the channel
    int n_sc;
    float ts32;                           // float32(1/bandwidth)
    int doppler;
    double fc;
};
__host__ inline Stage1Params stage1_params(const dmx_params& prm, int P) {
    Stage1Params s;
    s.bsx = sin(prm.bs_rotation[0]); s.csx = cos(prm.bs_rotation[0]);
    s.bsy = sin(prm.bs_rotation[1]); s.csy = cos(prm.bs_rotation[1]);
    s.brz = prm.bs_rotation[2];
    s.usx = sin(prm.ue_rotation[0]); s.ucx = cos(prm.ue_rotation[0]);
    s.usy = sin(prm.ue_rotation[1]); s.ucy = cos(prm.ue_rotation[1]);
    s.urz = prm.ue_rotation[2];
    s.ue_rot_pu = prm.ue_rotation_per_user;
    s.fov_enabled = prm.fov_enabled; s.bs_restricted = prm.bs_fov_restricted; s.ue_restricted = prm.ue_fov_restricted;
    s.bs_fh = prm.bs_fov[0]; s.bs_fv = prm.bs_fov[1]; s.ue_fh = prm.ue_fov[0]; s.ue_fv = prm.ue_fov[1];
    s.bs_pat = prm.bs_pattern; s.ue_pat = prm.ue_pattern;
    s.bs_spacing = prm.bs_spacing; s.ue_spacing = prm.ue_spacing;
    s.P = P; s.n_sc = prm.n_subcarriers;
    s.ts32 = (float)(1.0 / prm.bandwidth);
    s.doppler = prm.enable_doppler; s.fc = prm.carrier_freq;
    return s;
}

// the UE rotation of user u: the launch's constant one, or the user's own in degrees (dataset.py:329-338)
__device__ __forceinline__ void stage1_ue_rotation(const Stage1Params& a, int64_t u, double& usx, double& ucx, double& usy,
                                                   double& ucy, double& urz) {
    usx = a.usx; ucx = a.ucx; usy = a.usy; ucy = a.ucy; urz = a.urz;
    if (a.ue_rot_pu) {
        const double rx = a.ue_rot_pu[3 * u + 0] * D2R_D, ry = a.ue_rot_pu[3 * u + 1] * D2R_D;
        urz = a.ue_rot_pu[3 * u + 2] * D2R_D;
        sincos(rx, &usx, &ucx);
        sincos(ry, &usy, &ucy);
    }
}

// What stage1_path yields for one lane's path: the record values, and whether the path takes a record slot
struct Stage1Path {
    float c_re, c_im, dn;                 // dn = 0 in the time domain
    double ty, tz, ry, rz;
    float dvel, dacc;                     // the rays' Doppler terms as loaded (0 without Doppler)
    bool keep;
};
// A user's light side products as they build up over the passes of its lanes; every pass of stage1_path adds its share.
// count_paths / has_fov_path / first_inter are the same in every lane of the user's group, maxd / any_delay are per lane
// and reduced by stage1_user_out's caller.
struct Stage1User {
    int count_paths = 0;                  // dataset.py:616-619
    bool has_fov_path = false;            // FoV on: some path so far is inside
    float first_inter = __int_as_float(0x7fc00000);   // interaction code of the first path (FoV on: the first inside)
    float maxd = -INFINITY;               // largest delay of a used path
    bool any_delay = false;
};

// Path j of user u - k1_path_prep's loop body and k12_fd_direct's phase A.  LPU = lanes per user, `in` = the lane has a
// path of a real user, grp = the user's group in the wave, first_pass = j is among the user's first LPU paths; the
// pass's share of the per-user side products goes into `us` (updated in place for the register count).  The
// side outputs that are per path (angles, powers, FoV mask) are written here; a kernel that does not have one passes a
// constant nullptr in `side` and that code is compiled out, as it is for freq_domain / rx_filter given as constants.
template <int LPU, bool LEAN, bool ZROT>
__device__ __forceinline__ Stage1Path stage1_path(const Stage1Params& a, const dmx_rays& r, const dmx_side& side,
                                                  const int freq_domain, const int rx_filter, const int need_angles,
                                                  const double usx, const double ucx, const double usy, const double ucy,
                                                  const double urz, const int64_t u, const int j, const bool in, const int grp,
                                                  const bool first_pass, Stage1User& us) {
    const int L = r.n_paths;
    const size_t row = (size_t)u * (size_t)r.ld;
    const size_t srow = (size_t)u * (size_t)L;              // dense side-product rows
    const bool iso = (a.bs_pat == DMX_PATTERN_ISOTROPIC) && (a.ue_pat == DMX_PATTERN_ISOTROPIC);
    const float nan32 = __int_as_float(0x7fc00000);
    const double nan64 = (double)nan32;
    Stage1Path o;

    // Eight loads issued TOGETHER, from an index every lane may read (idle lanes: the user's last path), masked
    // afterwards.  Written as `in ? array[row + j] : nan`, each load sat alone in a branch of its own with an
    // `s_waitcnt vmcnt(0)` behind it: eight memory round trips in a row were the 8 us a wave lived (SQ_WAVE_CYCLES /
    // SQ_WAVES, profiles/r3_d8_summary.txt) and 0.20-0.28 ms of stage 1 per 200k users.
    const size_t jc = row + (size_t)(j < L ? j : L - 1);
    const float power_r = r.power[jc], phase_r = r.phase[jc], delay_r = r.delay[jc], aoa_az_r = r.aoa_az[jc];
    const float aoa_el_r = r.aoa_el[jc], aod_az_r = r.aod_az[jc], aod_el_r = r.aod_el[jc], inter_r = r.inter[jc];
    const bool dop_rays = a.doppler && r.doppler_vel && r.doppler_acc;       // kernel-uniform
    o.dvel = 0.f; o.dacc = 0.f;
    if (dop_rays) { o.dvel = r.doppler_vel[jc]; o.dacc = r.doppler_acc[jc]; }    // in the same batch
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
        if (need_angles) {                               // wave-uniform
            th_t = acos(zc_t); ph_t = np_angle(re_t, im_t);
            th_r = acos(zc_r); ph_r = np_angle(re_r, im_r);
        }
        if (in) {
            if (side.aod_el_rot) side.aod_el_rot[srow + j] = th_t;
            if (side.aod_az_rot) side.aod_az_rot[srow + j] = ph_t;
            if (side.aoa_el_rot) side.aoa_el_rot[srow + j] = th_r;
            if (side.aoa_az_rot) side.aoa_az_rot[srow + j] = ph_r;
        }
    }

    // field of view (dataset.py:493-511): outside -> angles become NaN
    bool mask = true;
    if (!LEAN && a.fov_enabled) {
        if (a.bs_restricted) mask = mask && in_fov(th_t, ph_t, a.bs_fh, a.bs_fv);
        if (a.ue_restricted) mask = mask && in_fov(th_r, ph_r, a.ue_fh, a.ue_fv);
        mask = mask && in;
        if (in && side.fov_mask) side.fov_mask[srow + j] = mask ? 1 : 0;
        if (!mask) { th_t = nan64; ph_t = nan64; th_r = nan64; ph_r = nan64; }
        const unsigned long long mb = group_mask<LPU>(__ballot(mask), grp);
        // first in-FoV path (dataset.py:594-598); the shuffle is executed by every lane, the
        // result is kept only by groups that had no in-FoV path yet
        const int src = mb != 0ull ? __ffsll((long long)mb) - 1 : 0;
        const float cand = __shfl(inter, src, LPU);
        if (!us.has_fov_path && mb != 0ull) { us.has_fov_path = true; us.first_inter = cand; }
    } else if (first_pass) {
        us.first_inter = __shfl(inter, 0, LPU);          // dataset.py:602
    }
    us.count_paths += __popcll(group_mask<LPU>(__ballot(in && !isnan(ph_r)), grp));   // dataset.py:616-619

    // powers (generator_utils.py:35, ant_patterns.py:167-168)
    const float p10 = power / 10.0f;
    const float pl = exp10f(p10);                        // float32 pow, as NumPy evaluates 10**float32
    double pw;
    if (LEAN || iso) {
        pw = (double)pl;
    } else {
        const double gt = a.bs_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_t)
                                                                  : (a.bs_pat == DMX_PATTERN_TR38901 ? tr38901_gain(th_t, ph_t) : 1.0);
        const double gr = a.ue_pat == DMX_PATTERN_HALFWAVE_DIPOLE ? dipole_gain(th_r)
                                                                  : (a.ue_pat == DMX_PATTERN_TR38901 ? tr38901_gain(th_r, ph_r) : 1.0);
        pw = (double)pl * (gt * gr);
    }
    if constexpr (!LEAN) {
        if (in) {
            if (side.power_linear) side.power_linear[srow + j] = pl;
            if (side.power_linear_ant_gain) side.power_linear_ant_gain[srow + j] = pw;
        }
    }

    // per-path record for the first P paths (dataset.py:258-261)
    const bool used = in && j < a.P;
    if (used && !isnan(delay)) { us.maxd = fmaxf(us.maxd, delay); us.any_delay = true; }
    const bool valid = used && !isnan(pw);               // channel.py:260
    const float ph32 = phase * D2R_F;                    // np.deg2rad(float32)
    float e_re, e_im;
    np_sincosf(ph32, e_im, e_re);                        // complex64 exp: NumPy's float32 cos / sin (and NaN-cheap, see there)
    const bool ang_ok = !isnan(th_t) && !isnan(th_r);    // geometry.py:65 zeroes NaN-zenith columns
    float c_re, c_im, dn = 0.0f;
    if (freq_domain) {
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
        if (dop_rays && !rx_filter) {                                        // construct_deepmimo.py:267-280
            const double v = in ? (double)o.dvel : 0.0;
            const double ac = in ? (double)o.dacc : 0.0;
            const double tau = (double)delay;
            const double arg = -TWO_PI * a.fc * (v * tau / LIGHTSPEED + ac * (tau * tau) / (2.0 * LIGHTSPEED));
            double sd, cd;
            sincos(arg, &sd, &cd);
            const float nr = (float)((double)c_re * cd - (double)c_im * sd);
            const float ni = (float)((double)c_re * sd + (double)c_im * cd);
            c_re = nr; c_im = ni;
        }
        // nansum (channel.py:283): a path with any NaN factor contributes nothing
        o.keep = valid && ang_ok && !isnan(ph_t) && !isnan(ph_r) && !isnan(c_re) && !isnan(c_im) && !isnan(dn) &&
                 (c_re != 0.0f || c_im != 0.0f);        // clipped / zero-gain paths add exactly 0
    } else {
        if (LEAN || iso) {
            const float amp = sqrtf((float)pw);                        // channel.py:286
            c_re = amp * e_re; c_im = amp * e_im;
        } else {
            const double amp = sqrt(pw);
            c_re = (float)(amp * (double)e_re); c_im = (float)(amp * (double)e_im);
        }
        if (!ang_ok) { c_re *= 0.0f; c_im *= 0.0f; }                   // zero array response, NaN stays NaN
        o.keep = valid;                                                // slot even if coefficient is 0
    }
    o.c_re = c_re; o.c_im = c_im; o.dn = dn;
    o.ty = 0.0; o.tz = 0.0; o.ry = 0.0; o.rz = 0.0;
    if (ang_ok && ZROT) {
        o.ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * sphi_t); o.tz = a.bs_spacing * zc_t;
        o.ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * sphi_r); o.rz = a.ue_spacing * zc_r;
    } else if (ang_ok) {                                 // geometry.py:99-101 in revolutions (kd / 2pi = spacing)
        const double rho_t = sqrt(re_t * re_t + im_t * im_t), rho_r = sqrt(re_r * re_r + im_r * im_r);
        o.ty = a.bs_spacing * (sqrt(1.0 - zc_t * zc_t) * (rho_t > 0.0 ? im_t / rho_t : 0.0)); o.tz = a.bs_spacing * zc_t;
        o.ry = a.ue_spacing * (sqrt(1.0 - zc_r * zc_r) * (rho_r > 0.0 ? im_r / rho_r : 0.0)); o.rz = a.ue_spacing * zc_r;
    }
    return o;
}

// A user's light side products, by lane 0 of the user's group once its passes are done; maxd = us.maxd reduced over the
// group's lanes, anyd = any of them had a delay
__device__ __forceinline__ void stage1_user_out(const dmx_side& side, const int fov_enabled, const int64_t u,
                                                const Stage1User& us, const float maxd, const bool anyd) {
    if (side.num_paths) side.num_paths[u] = us.count_paths;
    if (side.los) {
        const bool has = fov_enabled ? us.has_fov_path : (us.count_paths > 0);
        side.los[u] = has ? ((us.first_inter == 0.0f) ? 1 : 0) : -1;    // dataset.py:604-609
    }
    // one running maximum for the whole launch: a returning atomic per user would serialise 1e5 updates on
    // one L2 word (~88 per us), so look first (relaxed, L2-served) and only update when this user raises it
    if (side.max_delay_key && anyd) {
        const uint32_t key = float_order_key(maxd);
        if (key > __hip_atomic_load(side.max_delay_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(side.max_delay_key, key);
    }
}

// The arithmetic form of stage 1 for a launch - ONE rule for launch_path_prep and launch_channels_fd_direct, whose
// results are bit-identical by contract:
//   STAGE1_FULL       something needs the angles as numbers (FoV, dipole or sector pattern, angle / power / mask side outputs)
//   STAGE1_LEAN       nothing does: arccos / atan2 / FoV / dipole compiled out, sincos_lean
//   STAGE1_LEAN_ZROT  lean, both rotations exactly zero and the same for every user, AND at most 32 loaded paths: the
//                     zero-rotation form exists for the two-users-per-wave instantiation only, and it differs from the
//                     general lean form in the last float64 bits of the y steps (rotate_dir_zero above)
enum Stage1Form { STAGE1_FULL = 0, STAGE1_LEAN = 1, STAGE1_LEAN_ZROT = 2 };
__host__ inline bool stage1_need_angles(const dmx_params& prm, const dmx_side& side) {
    return prm.fov_enabled || prm.bs_pattern != DMX_PATTERN_ISOTROPIC || prm.ue_pattern != DMX_PATTERN_ISOTROPIC ||
           side.aod_el_rot || side.aod_az_rot || side.aoa_el_rot || side.aoa_az_rot;
}
__host__ inline Stage1Form stage1_form(const dmx_params& prm, const dmx_side& side, int32_t n_paths_loaded) {
    const bool lean = !stage1_need_angles(prm, side) && !side.power_linear && !side.power_linear_ant_gain && !side.fov_mask;
    if (!lean) return STAGE1_FULL;
    bool zrot = !prm.ue_rotation_per_user && n_paths_loaded <= 32;
    for (int i = 0; i < 3; ++i) zrot = zrot && prm.bs_rotation[i] == 0.0 && prm.ue_rotation[i] == 0.0;
    return zrot ? STAGE1_LEAN_ZROT : STAGE1_LEAN;
}

}  // namespace dmx
