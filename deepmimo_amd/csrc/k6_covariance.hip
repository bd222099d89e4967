// Fused consumer of the per-path records: the per-user spatial covariance of the frequency-domain
// channel over one array, averaged over the other array and the selected subcarriers, without the channel tensor:
//   H[r,t,k]  = sum_l c_l a_rx[r,l] a_tx[t,l] g[l,k],            g[l,k] = exp(-j 2pi dn_l sc_k / N)
//   R_tx[i,j] = 1 / (M_rx K) sum_r sum_k H[r,i,k] conj(H[r,j,k]) = sum_l sum_l' a_tx[i,l] Q[l,l'] conj(a_tx[j,l'])
//   Q[l,l']   = c_l conj(c_l') S[l,l'] D[l,l'],   S = 1/M_rx sum_r a_rx[r,l] conj(a_rx[r,l']),   D = 1/K sum_k g[l,k] conj(g[l',k])
// (R_rx: the two arrays exchanged).  One WAVE per user from its records to its M x M block, as k2_fd_small: no
// workgroup barrier, the wave's tables in its own LDS slice, a flat grid of ceil(users / waves) workgroups.
//   1  array tables  ao[m][l] (the side R is over), aa[m][l] (the averaged side): float64 phase reduction + sincos_rev
//   2  delay coupling D for l <= l': chunks of kc subcarriers of g in LDS (phase = fma(x, k, -rint(x k)) in float64, any
//      int32 index), a lane owns (l, l') pairs and adds g conj(g') over the chunk in index order, chunk sums are added
//      to the pair's slot of Q in chunk order
//   3  path coupling S from aa, Q = c conj(c') S D / (M_avg K), mirrored to the full Hermitian P x P matrix
//   4  T = ao Q (M x P), R[i,j] = sum_l' T[i,l'] conj(ao[j,l']) for i <= j; [j,i] gets the conjugate, the diagonal an
//      imaginary part of +0 and a real part clamped at 0 (it is a mean of |H|^2)
// fp32 vector arithmetic, no atomics, every sum in a fixed order that does not depend on where the user sits in the
// launch.  LDS of one wave: (M_out + M_avg + M_out + P + kc) * P * 8 bytes (ao, aa, T, Q, g chunk), P = min(num_paths,
// loaded paths) <= 32; cov_waves_per_block has the rule.  Bound: VALU / LDS issue of phases 2 and 4, far below HBM.
#include "dmx_common.h"
#include "array_phase.h"
#include "k2_small_body.h"

namespace dmx {

struct CovArgs {
    int64_t user_begin, user_count;
    int m_out, out_mh;   // elements / first panel dimension of the array R is over
    int m_avg, avg_mh;   // ... of the array that is averaged over
    int K, kc;           // selected subcarriers, subcarriers per chunk
    const int32_t* sc;
    double inv_n;
    float scale;         // 1 / (m_avg * K)
    int ld;              // table row stride in path slots (= P)
    NearField nf;        // DMX_FLAG_NEAR_FIELD (array_phase.h)
};

// Pair (i <= j) number e of an n x n upper triangle, rows i and n - 1 - i folded into one row of n + 1 entries
// (e < ((n + 1) / 2) * (n + 1)); false for the second half of the middle row of an odd n, which is that row again
__device__ __forceinline__ bool tri_pair(int e, int n, int& i, int& j) {
    const int r = e / (n + 1), c = e - r * (n + 1);
    if (c < n - r) { i = r; j = r + c; return true; }
    i = n - 1 - r; j = i + (c - (n - r));
    return i != r;
}

// acc += p * conj(q)
__device__ __forceinline__ void cmac_conj(float& ar, float& ai, const float2 p, const float2 q) {
    ar = fmaf(p.x, q.x, fmaf(p.y, q.y, ar));
    ai = fmaf(p.y, q.x, fmaf(-p.x, q.y, ai));
}

template <int SIDE>
__global__ __launch_bounds__(256) void k6_covariance(WsView ws, CovArgs a, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int64_t ul = (int64_t)blockIdx.x * wpb + wave;
    if (ul >= a.user_count) return;                                          // waves never talk to each other
    const int ld = a.ld, M = a.m_out, K = a.K;
    const size_t per_wave = (size_t)(2 * M + a.m_avg + ld + a.kc) * ld;
    float2* ao = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * per_wave;     // [M][ld]
    float2* aa = ao + (size_t)M * ld;                                                // [m_avg][ld]
    float2* T = aa + (size_t)a.m_avg * ld;                                           // [M][ld]
    float2* Q = T + (size_t)M * ld;                                                  // [ld][ld]
    float2* g = Q + (size_t)ld * ld;                                                 // [kc][ld]
    const int64_t u = a.user_begin + ul;
    float2* o = out + (size_t)ul * M * M;
    int n = __builtin_amdgcn_readfirstlane(ws.n_keep[u]);
    n = n < ld ? n : ld;
    if (n <= 0) {                                                            // no kept path: an all-zero block
        for (int i = lane; i < M * M; i += 64) o[i] = make_float2(0.f, 0.f);
        return;
    }
    const WsRecords rec{ws, (size_t)u * ws.P};

    // 1  array tables, and the pair sums of phase 2 start at zero
    for (int i = lane; i < M * n; i += 64) {
        const int t = i / n, l = i - t * n;
        const double sy = SIDE == DMX_COV_TX ? rec.tx_y(l) : rec.rx_y(l), sz = SIDE == DMX_COV_TX ? rec.tx_z(l) : rec.rx_z(l);
        float s, c;
        sincos_rev(frac_rev(array_phase(t % a.out_mh, t / a.out_mh, sy, sz, a.nf.on ? rec.dn(l) : 0.f, a.nf.end(SIDE != DMX_COV_TX))), s, c);
        ao[t * ld + l] = make_float2(c, s);
    }
    for (int i = lane; i < a.m_avg * n; i += 64) {
        const int t = i / n, l = i - t * n;
        const double sy = SIDE == DMX_COV_TX ? rec.rx_y(l) : rec.tx_y(l), sz = SIDE == DMX_COV_TX ? rec.rx_z(l) : rec.tx_z(l);
        float s, c;
        sincos_rev(frac_rev(array_phase(t % a.avg_mh, t / a.avg_mh, sy, sz, a.nf.on ? rec.dn(l) : 0.f, a.nf.end(SIDE == DMX_COV_TX))), s, c);
        aa[t * ld + l] = make_float2(c, s);
    }
    for (int i = lane; i < n * ld; i += 64) Q[i] = make_float2(0.f, 0.f);

    // 2  D[l,l'] (not yet divided by K) for l <= l' into Q[l][l']
    const int npair = ((n + 1) >> 1) * (n + 1);
    for (int k0 = 0; k0 < K; k0 += a.kc) {
        const int kn = K - k0 < a.kc ? K - k0 : a.kc;
        wave_lds_fence();                                                    // the last chunk's reads before this chunk's writes
        for (int i = lane; i < n * kn; i += 64) {
            const int k = i / n, l = i - k * n;
            float s, c;
            // the fractional part of the EXACT product x * k (k2_small_body.h)
            const double x = (double)rec.dn(l) * a.inv_n, kd = (double)a.sc[k0 + k];
            sincos_rev((float)__builtin_fma(x, kd, -rint(x * kd)), s, c);
            g[k * ld + l] = make_float2(c, -s);
        }
        wave_lds_fence();
        for (int e = lane; e < npair; e += 64) {
            int l, m;
            if (!tri_pair(e, n, l, m)) continue;
            float sr = 0.f, si = 0.f;
            for (int k = 0; k < kn; ++k) cmac_conj(sr, si, g[k * ld + l], g[k * ld + m]);
            float2 d = Q[l * ld + m];                                        // the pair's slot is this lane's alone
            d.x += sr; d.y += si;
            Q[l * ld + m] = d;
        }
    }

    // 3  S from the averaged side's table; Q = c conj(c') S D / (M_avg K), both triangles
    wave_lds_fence();
    for (int e = lane; e < npair; e += 64) {
        int l, m;
        if (!tri_pair(e, n, l, m)) continue;
        float sr = 0.f, si = 0.f;
        for (int r = 0; r < a.m_avg; ++r) cmac_conj(sr, si, aa[r * ld + l], aa[r * ld + m]);
        const float2 d = Q[l * ld + m];
        const float pr = (sr * d.x - si * d.y) * a.scale, pi = (sr * d.y + si * d.x) * a.scale;
        float wr = 0.f, wi = 0.f;
        cmac_conj(wr, wi, make_float2(rec.c_re(l), rec.c_im(l)), make_float2(rec.c_re(m), rec.c_im(m)));
        const float qr = wr * pr - wi * pi, qi = l == m ? 0.f : wr * pi + wi * pr;
        Q[l * ld + m] = make_float2(qr, qi);
        Q[m * ld + l] = make_float2(qr, -qi);
    }

    // 4  T = ao Q, then the upper triangle of R = T ao^H and its mirror image
    wave_lds_fence();
    for (int e = lane; e < M * n; e += 64) {
        const int i = e / n, m = e - i * n;
        float tr = 0.f, ti = 0.f;
        for (int l = 0; l < n; ++l) {
            const float2 x = ao[i * ld + l], q = Q[l * ld + m];
            tr = fmaf(x.x, q.x, fmaf(-x.y, q.y, tr));
            ti = fmaf(x.x, q.y, fmaf(x.y, q.x, ti));
        }
        T[i * ld + m] = make_float2(tr, ti);
    }
    wave_lds_fence();
    const int nout = ((M + 1) >> 1) * (M + 1);
    for (int e = lane; e < nout; e += 64) {
        int i, j;
        if (!tri_pair(e, M, i, j)) continue;
        float rr = 0.f, ri = 0.f;
        for (int m = 0; m < n; ++m) cmac_conj(rr, ri, T[i * ld + m], ao[j * ld + m]);
        if (i == j) {
            o[(size_t)i * M + i] = make_float2(fmaxf(rr, 0.f), 0.f);
        } else {
            o[(size_t)i * M + j] = make_float2(rr, ri);
            o[(size_t)j * M + i] = make_float2(rr, -ri);
        }
    }
}

// Waves per workgroup (0: the shape is not taken) and the subcarrier chunk for P path slots.  One wave needs
//   (M_out + M_avg + M_out + P + kc) * P * 8 bytes
// and lds_waves_per_block turns that into 4 / 2 / 1 waves (16 KB / 32 KB / 156 KB per wave).  kc is 64, 32, 16 or 8: the
// largest with which a workgroup still has as many waves as kc = 8 gives it, so the chunk shrinks before waves are
// given up and the shape is refused only when kc = 8 does not fit 156 KB.
int cov_waves_per_block(const dmx_params& prm, int P, int side, int* kc_out) {
    if (P < 1 || P > 32) return 0;
    const size_t m_tx = (size_t)prm.bs_shape[0] * prm.bs_shape[1], m_rx = (size_t)prm.ue_shape[0] * prm.ue_shape[1];
    const size_t rows = m_tx + m_rx + (side == DMX_COV_TX ? m_tx : m_rx) + (size_t)P;
    auto waves = [&](int kc) { return lds_waves_per_block((rows + (size_t)kc) * (size_t)P * sizeof(float2)); };
    const int best = waves(8);
    int kc = 8;
    for (int c : {64, 32, 16})
        if (best && waves(c) == best) { kc = c; break; }
    if (kc_out) *kc_out = kc;
    return best;
}

int launch_covariance(const dmx_params& prm, const WsView& ws, int64_t user_begin, int64_t user_count, int side,
                      float2* out, hipStream_t stream) {
    int kc = 8;
    const int wpb = cov_waves_per_block(prm, ws.P, side, &kc);
    if (!wpb) { set_error("covariance kernel: tables of one user do not fit the LDS"); return DMX_ERR_SHAPE; }
    const bool tx = side == DMX_COV_TX;
    CovArgs a;
    a.user_begin = user_begin; a.user_count = user_count;
    a.m_out = tx ? prm.bs_shape[0] * prm.bs_shape[1] : prm.ue_shape[0] * prm.ue_shape[1];
    a.out_mh = tx ? prm.bs_shape[0] : prm.ue_shape[0];
    a.m_avg = tx ? prm.ue_shape[0] * prm.ue_shape[1] : prm.bs_shape[0] * prm.bs_shape[1];
    a.avg_mh = tx ? prm.ue_shape[0] : prm.bs_shape[0];
    a.K = prm.n_selected; a.kc = kc;
    a.sc = prm.selected_subcarriers;
    a.inv_n = 1.0 / (double)prm.n_subcarriers;
    a.scale = (float)(1.0 / ((double)a.m_avg * (double)a.K));
    a.ld = ws.P;
    a.nf = near_field_of(prm);
    const size_t smem = (size_t)wpb * (size_t)(2 * a.m_out + a.m_avg + a.ld + a.kc) * a.ld * sizeof(float2);
    const dim3 g((unsigned)((user_count + wpb - 1) / wpb)), b(64 * wpb);    // flat: one wave per user
    if (tx) return launch_dyn_lds(k6_covariance<DMX_COV_TX>, "k6_covariance", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
    return launch_dyn_lds(k6_covariance<DMX_COV_RX>, "k6_covariance", g, b, smem, WAVE_LDS_MAX, stream, ws, a, out);
}

}  // namespace dmx
