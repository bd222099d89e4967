// Per-path arithmetic of stage 1, shared by k1_path_prep.hip and the single-pass kernel k12_fd_direct.hip: the
// constants, NumPy's float32 sin / cos, the float64 rotation, the field-of-view test, the dipole gain and the small
// ballot helpers.  Every function is __forceinline__ and follows the reference's dtype flow; the including file
// decides the FMA contraction: both k1_path_prep.hip and k12_fd_direct.hip are compiled with -ffp-contract=off (Makefile;
// the single-pass kernel switches contraction back ON with a pragma after its stage-1 part), so both kernels evaluate
// the very same operations.  stage1_form is the one rule by which both launchers pick the arithmetic form.
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

// The arithmetic form of stage 1 for a launch - ONE rule for launch_path_prep and launch_channels_fd_direct, whose
// results are bit-identical by contract:
//   STAGE1_FULL       something needs the angles as numbers (FoV, dipole pattern, angle / power / mask side outputs)
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
