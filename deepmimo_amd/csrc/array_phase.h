// The phase of one array element for one path, in revolutions (float64): the one statement of it that every kernel which
// builds its array tables from the path records goes through (k2_fd_valu, k6_covariance, k7_rate, fill_array_table of
// k7_rate_body.h and with it k8 / k9 / k10, k2b_beam_project's scalar form, k2c_beam_power's receive side).
//
// Far field (plane wave): q = y sy + z sz, with sy = d sin(th) sin(ph), sz = d cos(th) what stage 1 wrote for the path and
// the end, in the order of operations the call site had before this header existed (`FMA`), so that every far-field bit
// stays what it was.
//
// Near field (DMX_FLAG_NEAR_FIELD, include/deepmimo_amd.h): the path is a spherical wave from a point R wavelengths away
// along its direction as seen from element 0, R = dn * carrier_freq / bandwidth from the record's float32 dn (the path
// length tau f_c).  Element (y, z) sits at d (0, y, z), s = d^2 (y^2 + z^2), and its phase is the path-length difference
//   psi = R - sqrt(R^2 - 2 R q + s) = (2 R q - s) / (R + sqrt(R^2 - 2 R q + s))
// evaluated in the second form, which does not cancel, and 0 where the numerator is 0 (element 0; also 0 / 0 at R = 0).
// |q| <= sqrt(s), so the argument of the root is (R - sqrt(s))^2 at the least: a squared distance, clamped against its
// own rounding.  R -> infinity gives q.
#pragma once
#include "dmx_common.h"

namespace dmx {

// near-field arguments of one end of the link
struct NearFieldEnd {
    int on;
    double r_scale;   // carrier_freq / bandwidth: R = dn * r_scale
    double d2;        // element spacing of this end, squared (wavelengths^2)
};
// ... of both ends, as the launchers put it into a kernel's argument block
struct NearField {
    int on;
    double r_scale, d2_rx, d2_tx;
    __host__ __device__ NearFieldEnd end(const bool rx) const { return NearFieldEnd{on, r_scale, rx ? d2_rx : d2_tx}; }
    __host__ __device__ NearFieldEnd rx() const { return end(true); }
    __host__ __device__ NearFieldEnd tx() const { return end(false); }
};

__host__ inline NearField near_field_of(const dmx_params& prm) {
    NearField nf;
    nf.on = (prm.flags & DMX_FLAG_NEAR_FIELD) ? 1 : 0;
    nf.r_scale = nf.on ? prm.carrier_freq / prm.bandwidth : 0.0;
    nf.d2_rx = prm.ue_spacing * prm.ue_spacing;
    nf.d2_tx = prm.bs_spacing * prm.bs_spacing;
    return nf;
}

// psi of the header for the plane-wave phase q.  Not inlined: the callers are the table fills in front of register-heavy
// bodies, and a call keeps their far-field register allocation within a few VGPRs of what it was without this branch
__device__ __noinline__ inline double near_field_phase(const double q, const int y, const int z, const double R, const double d2) {
    const double s = d2 * (double)(y * y + z * z);
    const double num = 2.0 * R * q - s;
    if (num == 0.0) return 0.0;
    const double arg = R * R - num;
    return num / (R + sqrt(arg > 0.0 ? arg : 0.0));
}

// FMA: the far-field form is __builtin_fma((double)y, sy, (double)z * sz); else (double)y * sy + (double)z * sz, which the
// compiler contracts as it did at the call site.  `dn`: the record's normalised delay (read only with nf.on)
template <bool FMA = true>
__device__ __forceinline__ double array_phase(const int y, const int z, const double sy, const double sz, const float dn,
                                              const NearFieldEnd& nf) {
    double q;
    if constexpr (FMA) q = __builtin_fma((double)y, sy, (double)z * sz);
    else q = (double)y * sy + (double)z * sz;
    if (nf.on) return near_field_phase(q, y, z, (double)dn * nf.r_scale, nf.d2);
    return q;
}

// sin and cos of an element's near-field phase: what a table fill whose far-field statement stays at the call site stores
// under the flag (k7_rate.hip, fill_array_table of k7_rate_body.h)
__device__ __forceinline__ void near_field_sincos(const int y, const int z, const double sy, const double sz, const float dn,
                                                  const NearFieldEnd& nf, float& s, float& c) {
    sincos_rev(frac_rev(array_phase(y, z, sy, sz, dn, nf)), s, c);
}

}  // namespace dmx
