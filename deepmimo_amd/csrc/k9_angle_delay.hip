// Fused consumer of the per-path records: the angle-delay representation of the frequency-domain channel - a TX codebook (or
// none: the antenna domain) over the BS array, an inverse DFT of n_fft points over the K uniformly spaced subcarriers
// sc_k = s0 + d k, cut to the first n_taps delay taps - without the channel tensor:
//   Y[u,rx,r,k] = sum_tx F[r,tx] H[u,rx,tx,k]
//   X[u,rx,r,t] = 1/n_fft sum_{k<K} Y[u,rx,r,k] e^{+j 2pi k t / n_fft},   t = 0 .. n_taps-1
//               = sum_l a_rx[rx,l] f[r,l] c_l D[l,t],      f[r,l] = sum_tx F[r,tx] a_tx[tx,l]   (a_tx itself without F)
//   D[l,t]      = 1/n_fft e^{-j 2pi frac(dn_l s0 / N)} e^{j pi (K-1) x} sin(pi K x) / sin(pi x),   x = t/n_fft - d dn_l / N
// (x and r = x - rint(x) give the same D: the signs of the three factors cancel), sin(pi K x) / sin(pi x) -> +-K at a tap.
// One WAVE per user as k7_rate: no workgroup barrier, no atomics, the wave's tables in its own LDS slice, a flat grid.
//   1  as[M_rx][P]: the a_rx table (k7_rate's phase 1)
//   D  per path, once per user, in lane l: e^{j pi b}, e^{j pi K b} in float64 (b = d dn / N; K b reduced mod 2 as the exact
//      product minus an even integer) and q_l = c_l / n_fft e^{-j 2pi frac(dn s0 / N)} e^{j pi b} e^{-j pi K b} in float32;
//      per tap, once per tap chunk, in the lane that owns the tap: e^{j pi a}, e^{j pi K a} in float64 (a = t / n_fft,
//      K t reduced mod 2 n_fft in integers) and their quotient e^{j pi (K-1) a} in float32.  That is P + tc float64 sincospi
//      per user instead of P tc; numerator and denominator then come by angle addition,
//          sin(pi K x) = Im(e^{j pi K a} conj(e^{j pi K b})),   sin(pi x) = Im(e^{j pi a} conj(e^{j pi b})),
//      two float64 products each, so that a path 1 float32 ulp off a tap (|x| = 2^-30 at 512 points) keeps 7 digits of
//      both; the hardware sine's 1.25e-7 absolute error would leave the ratio none.  |sin(pi x)| < pi 2^-30: the limit K,
//      with the sign of cos(pi K x) cos(pi x).
//   2  w[l][t] = q_l e^{j pi (K-1) a_t} ratio PATH-MAJOR in LDS for a chunk of tc = min(n_taps, 64) taps; lane = (slice, tap)
//      as in phase 3, so a lane's tap values stay in registers and the path values come by lane shuffle
//   2' ab[RC][P]: a chunk of at most RC = 32 rows of the row table - copied from k2b_beam_project's f table with a codebook,
//      computed as k7_rate's a_big without one.  Not the whole [R][P] table: 256 rows would leave two waves per CU.
//   3  lane = s tc' + t, tc' the power of two >= tc, S = 64 / tc' row slices (1 above 32 taps): per trip rows_pair<M_rx> of
//      k7_rate_body.h on rows base + s and base + S + s of the chunk, the products stored instead of Gram'd - each store
//      instruction writes S n_taps 8 contiguous bytes of one (rx, row .. row + S) block
// n_taps > 64: the tap chunks rebuild w and stream the rows again.  fp32 vector arithmetic, every sum in a fixed order that
// does not depend on where the user sits in the launch.  LDS of one wave: (M_rx + min(R, 32) + tc) * P * 8 bytes.
#include "dmx_common.h"
#include "k2_small_body.h"
#include "k7_rate_body.h"
#include <math.h>

namespace dmx {

static constexpr int AD_RC = 32;             // rows of the row table per LDS chunk

struct AdArgs {
    int64_t user_begin, user_count;
    int ue_mh, bs_mh;
    int R;                   // rows: codebook rows, or M_tx
    int n_taps, tc;          // taps, taps per chunk = w row stride
    int tcp, log2_tcp, S;    // power of two >= tc, row slices per trip
    int K, s0, d, n_fft;     // the selection s0 + d k, k < K, and the inverse DFT's length
    double inv_n, inv_nfft;
    const float2* ftab;      // [user_count, R, P] from k2b_beam_project, or nullptr: rows are the BS elements
    int ld;                  // table row stride in path slots (= P)
    NearField nf;            // DMX_FLAG_NEAR_FIELD (array_phase.h); with ftab the BS side of it is inside the rows
};

struct cd { double x, y; };                                                  // float64 complex: cos, sin
__device__ __forceinline__ cd expjpi(double v) { cd r; sincospi(v, &r.y, &r.x); return r; }
__device__ __forceinline__ cd mul_conj(cd a, cd b) {                         // a conj(b)
    return cd{__builtin_fma(a.x, b.x, a.y * b.y), __builtin_fma(a.y, b.x, -(a.x * b.y))};
}

// OUT: what phase 3 stores.  0: X, complex [M][R][T] per user.  1: the angle-delay power P[r][t] = sum_rx |X[rx][r][t]|^2, one
// float per (row, tap) - a lane holds all M entries of its (row, tap) in registers after rows_pair<M>, so the sum is
// |h[0]|^2 + ... + |h[M-1]|^2 in ascending rx, each term fmaf(im, im, re re).  2: the delay profile p[t] = sum_r P[r][t]: a lane
// adds its rows in the order it meets them (r0 ascending, base ascending, row ra before rb), the S row slices of a tap are then
// added in ascending slice order by lane shuffle and slice 0 stores.  `out` is float [R][T] / [T] per user for 1 / 2.
template <int M>
__device__ __forceinline__ float row_power(const float2 (&h)[M]) {
    float p = fmaf(h[0].y, h[0].y, h[0].x * h[0].x);
#pragma unroll
    for (int i = 1; i < M; ++i) p += fmaf(h[i].y, h[i].y, h[i].x * h[i].x);
    return p;
}

// The float pointers of OUT 1 and 2 are formed inside their `if constexpr` branches: a pointer formed beside `o`, dead in OUT 0,
// changed the register allocation of the OUT 0 instantiations, which are to stay the instruction streams they were.
template <int M, int OUT>
__global__ __launch_bounds__(256) void k9_angle_delay(WsView ws, AdArgs a, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                          // waves never talk to each other
    const int ld = a.ld, R = a.R, T = a.n_taps, tc = a.tc, S = a.S;
    const int rc = R < AD_RC ? R : AD_RC;
    const size_t per_wave = (size_t)(M + rc + tc) * ld;
    float2* as = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * per_wave;     // [M][ld]
    float2* ab = as + (size_t)M * ld;                                                // [rc][ld]
    float2* w = ab + (size_t)rc * ld;                                                // [ld][tc]
    const int64_t u = a.user_begin + ul;
    float2* o = out + (size_t)ul * M * R * T;                                        // [M][R][T]
    const int n = kept_paths(ws, u);
    if (n <= 0) {                                                            // no kept path: +0.0 everywhere
        if constexpr (OUT == 0) {
            for (size_t i = lane; i < (size_t)M * R * T; i += 64) o[i] = make_float2(0.f, 0.f);
        } else {
            const size_t per_user = (size_t)(OUT == 2 ? 1 : R) * T;         // [R][T], or [T]
            float* of = reinterpret_cast<float*>(out) + (size_t)ul * per_user;
            for (size_t i = lane; i < per_user; i += 64) of[i] = 0.f;
        }
        return;
    }
    const WsRecords rec{ws, (size_t)u * ws.P, a.nf};

    // 1  the a_rx table
    fill_array_table(as, rec, true, 0, M, a.ue_mh, n, ld, lane);

    // D  this lane's path (lanes >= n hold path n - 1 again and are never asked)
    cd e1b, ekb;
    float2 q;
    {
        const int l = lane < n ? lane : n - 1;
        const double dn = (double)rec.dn(l);
        const double x = dn * a.inv_n;
        const double b = ((double)a.d * dn) * a.inv_n, kd = (double)a.K;     // d dn is exact: 20 + 24 bits
        e1b = expjpi(b);
        ekb = expjpi(__builtin_fma(b, kd, -2.0 * rint(0.5 * (b * kd))));     // the EXACT product b K less an even integer
        float s, c;
        const double s0 = (double)a.s0;
        sincos_rev((float)__builtin_fma(x, s0, -rint(x * s0)), s, c);        // k7_rate's phase 2
        const float sc = (float)a.inv_nfft;
        const float cr = rec.c_re(l) * sc, ci = rec.c_im(l) * sc;
        const float pr = fmaf(cr, c, ci * s), pi = fmaf(ci, c, -(cr * s));   // c_l / n_fft (cos - j sin)
        const cd g = mul_conj(e1b, ekb);                                     // e^{j pi b} e^{-j pi K b}
        const float gr = (float)g.x, gi = (float)g.y;
        q = make_float2(fmaf(pr, gr, -(pi * gi)), fmaf(pr, gi, pi * gr));
    }

    const int tl = lane & (a.tcp - 1), sl = lane >> a.log2_tcp;             // this lane's tap of the chunk and row slice
    for (int t0 = 0; t0 < T; t0 += tc) {
        const int tn = T - t0 < tc ? T - t0 : tc;
        const bool active = tl < tn;
        // 2  w of the tap chunk
        wave_lds_fence();                                                    // the last chunk's reads before this chunk's writes
        {
            const int t = t0 + (active ? tl : 0);
            const cd e1a = expjpi((double)t * a.inv_nfft);
            const int64_t kt = ((int64_t)a.K * t) % (2 * (int64_t)a.n_fft);
            const cd eka = expjpi((double)kt * a.inv_nfft);
            const cd ga = mul_conj(eka, e1a);                                // e^{j pi (K-1) a}
            const float gar = (float)ga.x, gai = (float)ga.y;
            for (int l0 = 0; l0 < n; l0 += S) {
                const int l = l0 + sl < n ? l0 + sl : n - 1;
                const cd b1{__shfl(e1b.x, l, 64), __shfl(e1b.y, l, 64)}, bk{__shfl(ekb.x, l, 64), __shfl(ekb.y, l, 64)};
                const float2 ql = make_float2(__shfl(q.x, l, 64), __shfl(q.y, l, 64));
                const cd v1 = mul_conj(e1a, b1), vk = mul_conj(eka, bk);     // e^{j pi x}, e^{j pi K x}
                const bool at_tap = fabs(v1.y) < 0x1.921fb54442d18p-29;      // pi 2^-30
                const float lim = (vk.x < 0.0) != (v1.x < 0.0) ? -(float)a.K : (float)a.K;
                const float ratio = at_tap ? lim : (float)vk.y / (float)(at_tap ? 1.0 : v1.y);
                const float hr = fmaf(ql.x, gar, -(ql.y * gai)) * ratio, hi = fmaf(ql.x, gai, ql.y * gar) * ratio;
                if (active && l0 + sl < n) w[l * tc + tl] = make_float2(hr, hi);
            }
        }

        float acc = 0.f;                  // OUT 2: this lane's rows of tap t0 + tl; unused and removed in OUT 0 and 1
        for (int r0 = 0; r0 < R; r0 += rc) {
            const int nr = R - r0 < rc ? R - r0 : rc;
            // 2' rows r0 .. r0 + nr of the row table
            wave_lds_fence();
            if (a.ftab) {                                                    // [nr][P] is one contiguous block on both sides
                copy_rows_to_lds(ab, a.ftab, ((size_t)ul * R + r0) * ld, nr * ld, lane);
            } else {
                fill_array_table(ab, rec, false, r0, nr, a.bs_mh, n, ld, lane);
            }
            wave_lds_fence();

            // 3  two rows per lane and trip, stored
            if (active) {
                const float2* wk = w + tl;
                for (int base = 0; base < nr; base += 2 * S) {
                    const int ra = base + sl, rb = base + S + sl;
                    const bool va = ra < nr, vb = rb < nr;
                    const float2* b0 = ab + (size_t)(va ? ra : 0) * ld;
                    const float2* b1 = ab + (size_t)(vb ? rb : 0) * ld;
                    float2 h0[M], h1[M];
                    rows_pair<M>(as, b0, b1, wk, ld, tc, n, h0, h1);
                    if constexpr (OUT == 0) {
#pragma unroll
                        for (int i = 0; i < M; ++i) {
                            float2* row = o + ((size_t)i * R + r0) * T + t0 + tl;
                            if (va) row[(size_t)ra * T] = h0[i];
                            if (vb) row[(size_t)rb * T] = h1[i];
                        }
                    } else if constexpr (OUT == 1) {
                        float* row = reinterpret_cast<float*>(out) + ((size_t)ul * R + r0) * T + t0 + tl;
                        if (va) row[(size_t)ra * T] = row_power<M>(h0);
                        if (vb) row[(size_t)rb * T] = row_power<M>(h1);
                    } else {
                        if (va) acc += row_power<M>(h0);
                        if (vb) acc += row_power<M>(h1);
                    }
                }
            }
        }
        if constexpr (OUT == 2) {                                            // every lane shuffles: a source lane shares tl
            float sum = 0.f;
            for (int s = 0; s < S; ++s) sum += __shfl(acc, (s << a.log2_tcp) + tl, 64);
            if (active && sl == 0) reinterpret_cast<float*>(out)[(size_t)ul * T + t0 + tl] = sum;
        }
    }
}

// LDS bytes of one wave for P path slots (0: the shape is not taken): the a_rx table, one chunk of the row table and one
// chunk of w,
//   (M_rx + min(R, 32) + tc) * P * 8,   M_rx <= 8,  R = n_rows,  tc = min(n_taps, 64)
// lds_waves_per_block turns that into 4 / 2 / 1 waves per workgroup (16 KB / 32 KB / 156 KB per wave).
size_t angle_delay_lds_bytes(const dmx_params& prm, int P, int n_rows, int n_taps) {
    if (P < 1 || P > 32 || n_rows < 1 || n_taps < 1) return 0;
    const size_t m_rx = (size_t)prm.ue_shape[0] * prm.ue_shape[1];
    if (m_rx > 8) return 0;
    const size_t rc = n_rows < AD_RC ? n_rows : AD_RC, tc = n_taps < 64 ? n_taps : 64;
    return (m_rx + rc + tc) * (size_t)P * sizeof(float2);
}

int angle_delay_waves_per_block(const dmx_params& prm, int P, int n_rows, int n_taps) {
    return lds_waves_per_block(angle_delay_lds_bytes(prm, P, n_rows, n_taps));
}

template <int M>
static int launch_ad_m(int output, const dim3 g, const dim3 b, size_t smem, hipStream_t stream, const WsView& ws, const AdArgs& a,
                       float2* out) {
    switch (output) {
        case 0: return launch_dyn_lds(k9_angle_delay<M, 0>, "k9_angle_delay", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
        case 1: return launch_dyn_lds(k9_angle_delay<M, 1>, "k9_angle_delay", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
        default: return launch_dyn_lds(k9_angle_delay<M, 2>, "k9_angle_delay", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
    }
}

// out complex [user_count, M_rx, n_rows, n_taps], or by the call's flags float [user_count, n_rows, n_taps]
// (DMX_FLAG_ANGLE_DELAY_POWER) or float [user_count, n_taps] (with DMX_FLAG_ANGLE_DELAY_PROFILE beside it); with a codebook the
// projection runs first into beam_ws (beam_workspace_bytes), as in launch_beam_power
int launch_angle_delay(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, const float2* codebook,
                       int n_rows, void* beam_ws, int n_fft, int n_taps, float2* out, hipStream_t stream) {
    if (user_count == 0) return DMX_OK;
    const int wpb = angle_delay_waves_per_block(prm, ws.P, n_rows, n_taps);
    if (!wpb) { set_error("angle-delay kernel: tables of one user do not fit the LDS"); return DMX_ERR_SHAPE; }
    AdArgs a;
    a.ftab = nullptr;
    if (codebook) {
        BeamTabs t;
        int rc = launch_beam_project(prm, ws, user_begin, user_count, codebook, n_rows, beam_ws, stream, &t);
        if (rc) return rc;
        a.ftab = t.ftab;
    }
    a.user_begin = user_begin; a.user_count = user_count;
    a.ue_mh = prm.ue_shape[0]; a.bs_mh = prm.bs_shape[0];
    a.nf = near_field_of(prm);
    a.R = n_rows;
    a.n_taps = n_taps; a.tc = n_taps < 64 ? n_taps : 64;
    a.log2_tcp = 0;
    while ((1 << a.log2_tcp) < a.tc) ++a.log2_tcp;
    a.tcp = 1 << a.log2_tcp;
    a.S = 64 / a.tcp;
    a.K = prm.n_selected; a.s0 = prm.sc_first; a.d = prm.sc_stride; a.n_fft = n_fft;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.inv_nfft = 1.0 / (double)n_fft;
    a.ld = ws.P;
    const int m_rx = prm.ue_shape[0] * prm.ue_shape[1];
    const size_t smem = (size_t)wpb * angle_delay_lds_bytes(prm, ws.P, n_rows, n_taps);
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), b(64 * wpb);    // flat: one wave per user
    const int output = !(prm.flags & DMX_FLAG_ANGLE_DELAY_POWER) ? 0 : (prm.flags & DMX_FLAG_ANGLE_DELAY_PROFILE) ? 2 : 1;
    switch (m_rx) {
        case 1: return launch_ad_m<1>(output, g, b, smem, stream, ws, a, out);
        case 2: return launch_ad_m<2>(output, g, b, smem, stream, ws, a, out);
        case 3: return launch_ad_m<3>(output, g, b, smem, stream, ws, a, out);
        case 4: return launch_ad_m<4>(output, g, b, smem, stream, ws, a, out);
        case 5: return launch_ad_m<5>(output, g, b, smem, stream, ws, a, out);
        case 6: return launch_ad_m<6>(output, g, b, smem, stream, ws, a, out);
        case 7: return launch_ad_m<7>(output, g, b, smem, stream, ws, a, out);
        default: return launch_ad_m<8>(output, g, b, smem, stream, ws, a, out);
    }
}

}  // namespace dmx
