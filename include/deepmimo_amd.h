/*
 * deepmimo_amd.h - C-ABI of the MI355X-native DeepMIMO channel-generation path.
 *
 * The reference (jmoraispk/DeepMIMO v4.0.0a3) is pure Python and has no FFI: the seam this
 * library sits behind is the method  Dataset.compute_channels(params)
 * (deepmimo/generator/dataset.py:224-268) and the lazy attributes it feeds (`channel`, `los`,
 * `num_paths`, `_fov_mask`, rotated angles, powers; dataset.py:831-869).  A maintainer binds
 * these entry points with ctypes (INTEGRATION.md shows the stub).  Everything is plain C:
 * borrowed DEVICE pointers + sizes in, caller-allocated DEVICE buffers out, a hipStream_t passed
 * as void*.  The library allocates nothing, keeps no global state except a thread-local error
 * string (in particular it reads no environment variable), launches asynchronously on the given stream and never
 * synchronises.  One entry point does I/O: dmx_mats_to_device (the loader) opens the files it is given and runs reader
 * threads for the duration of the call; nothing of either outlives it.
 *
 * Layouts: ray fields are float32 row-major [n_ue, ld] (ld >= n_paths), NaN = "no path", exactly
 * the arrays Dataset holds after core.py:209-219.  The channel tensor is complex64 interleaved
 * (re, im), C-contiguous [n_ue, M_rx, M_tx, K] (frequency domain) or [n_ue, M_rx, M_tx, P]
 * (time domain), last index fastest, as channel.py:257 allocates it.
 */
#ifndef DEEPMIMO_AMD_H
#define DEEPMIMO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMX_ABI_VERSION 3

/* status codes (0 = ok).  dmx_last_error() holds the message of the last failure on this thread. */
#define DMX_OK               0
#define DMX_ERR_ARG         -1   /* NULL / inconsistent argument */
#define DMX_ERR_SHAPE       -2   /* shape outside what the kernels support */
#define DMX_ERR_LAUNCH      -3   /* hipLaunch / runtime failure */
#define DMX_ERR_WORKSPACE   -4   /* workspace too small or misaligned */

/* radiation patterns: deepmimo/consts.py:254, deepmimo/generator/ant_patterns.py:21-71 */
#define DMX_PATTERN_ISOTROPIC        0
#define DMX_PATTERN_HALFWAVE_DIPOLE  1
/* The sector element of 3GPP TR 38.901 Table 7.3-1 (Sionna's "tr38901"; not in the reference).  On a path's rotated,
 * FoV-masked angles - zenith th in [0, pi], azimuth ph in (-pi, pi], boresight th = pi/2, ph = 0: the panel lies in the
 * y-z plane and faces +x, where the FoV test is centred - in float64, with b = 65 degrees in radians:
 *   A_v = min(12 ((th - pi/2) / b)^2, 30),  A_h = min(12 (ph / b)^2, 30),  A = min(A_v + A_h, 30),
 *   gain = 10^((8 - A) / 10)     linear power gain, 8 dBi at boresight, floor -22 dBi; 0 where th or ph is NaN
 * It multiplies the path power like the dipole's gain.  Either side takes any of the three, independently. */
#define DMX_PATTERN_TR38901          2

/* Ray-path records of one (TX, RX-set) pair: the float32 matrices of core.py:209-219. */
typedef struct dmx_rays {
    int64_t n_ue;          /* users (rows) */
    int32_t n_paths;       /* loaded paths per user (columns) */
    int32_t ld;            /* row stride in elements, >= n_paths */
    const float* power;    /* dBW                        consts.py:188 */
    const float* phase;    /* degrees                    consts.py:189 */
    const float* delay;    /* seconds                    consts.py:190 */
    const float* aoa_az;   /* degrees                    consts.py:191 */
    const float* aoa_el;   /* degrees, zenith            consts.py:192 */
    const float* aod_az;   /* degrees                    consts.py:193 */
    const float* aod_el;   /* degrees, zenith            consts.py:194 */
    const float* inter;    /* interaction code, 0 = LoS  consts.py:197 */
    const float* doppler_vel;  /* m/s, optional (NULL)   deepmimo_v3/consts.py:63 */
    const float* doppler_acc;  /* m/s^2, optional (NULL) deepmimo_v3/consts.py:64 */
} dmx_rays;

/* Channel parameters: ChannelGenParameters (channel.py:33-63) after validate() (:78-139), plus
 * the FoV pair Dataset.apply_fov stored (dataset.py:423-448).  Angles in RADIANS as the host's
 * np.deg2rad produced them (float64), so the device sees the reference's exact doubles. */
typedef struct dmx_params {
    int32_t bs_shape[2];          /* [Mh, Mv]; element m = y + Mh*z   geometry.py:105-120 */
    int32_t ue_shape[2];
    double  bs_spacing;           /* wavelengths */
    double  ue_spacing;
    double  bs_rotation[3];       /* radians about x, y, z            geometry.py:286-291 */
    double  ue_rotation[3];       /* radians; used when ue_rotation_per_user == NULL */
    const double* ue_rotation_per_user; /* device [n_ue, 3] DEGREES (dataset.py:329-338) or NULL */
    int32_t bs_pattern;           /* DMX_PATTERN_* */
    int32_t ue_pattern;
    int32_t fov_enabled;          /* 0: Dataset._compute_fov returns mask None (dataset.py:484) */
    int32_t bs_fov_restricted;    /* dataset.py:497 */
    int32_t ue_fov_restricted;    /* dataset.py:502 */
    double  bs_fov[2];            /* radians [horizontal, vertical]   geometry.py:184 */
    double  ue_fov[2];
    int32_t num_paths;            /* params.num_paths; min(num_paths, rays.n_paths) paths are used */
    int32_t freq_domain;          /* 1: OFDM channel, 0: time-domain taps   channel.py:54 */
    int32_t n_subcarriers;        /* ofdm.subcarriers (N) */
    int32_t n_selected;           /* K = len(ofdm.selected_subcarriers) */
    const int32_t* selected_subcarriers; /* device [K]; any int32 values (negative, >= N), see DMX_SC_ABS_MAX_F32 */
    double  bandwidth;            /* Hz; Ts = 1/bandwidth             channel.py:223 */
    int32_t rx_filter;            /* ofdm.rx_filter (LPF / sinc interpolation)  channel.py:193-194 */
    int32_t enable_doppler;       /* apply the v3 Doppler term (construct_deepmimo.py:267-280) */
    double  carrier_freq;         /* Hz, for Doppler */
    /* Host-side promise about the DEVICE array above (ABI 2): when sc_stride > 0 the caller guarantees
     * selected_subcarriers[k] == sc_first + k * sc_stride for every k (np.arange(N), np.arange(0, N, s), [0] ...:
     * what channel.py:57 and the reference's own scripts select).  It lets dmx_channels_fd pick the folded kernel for
     * few antenna pairs without reading the device array back.  sc_stride = 0 makes no promise (any selection).
     * With a promise the library also sees the largest |index|, max(|sc_first|, |sc_first + (K-1) sc_stride|), and
     * enforces DMX_SC_ABS_MAX_F32 with it; without one, keeping within that bound is the caller's job. */
    int32_t sc_first;
    int32_t sc_stride;
    /* Arithmetic mode of the matrix-core kernels (ABI 3).  The reference multiplies and sums every path in complex128
     * (channel.py:283-284); the kernels form every product from three f16 x f16 terms with fp32 accumulation, which
     * keeps |error| <= ~2e-6 of a user's strongest path.  0 = that, for every path (default).
     * DMX_FLAG_ADAPTIVE_TERMS: opt-in - stage 1 writes a user's kept paths in order of falling amplitude and a last
     * 8-path group whose paths are all >= 66 dB below the strongest one is multiplied out in ONE term (worst case 7.6e-6
     * of the strongest path; 3-5 % less time at 25 paths).  The flag must be the same in dmx_path_prep and in the
     * stage-2 call that reads its workspace. */
    uint32_t flags;
    uint32_t reserved0;          /* must be 0 */
} dmx_params;

#define DMX_FLAG_ADAPTIVE_TERMS 1u

/* Spatial-wideband channel (beam squint): the array response of every element is taken at the subcarrier's own frequency
 * f_c + sc_k B / N instead of at the carrier.  With c_l, dn_l as in dmx_channels_fd, psi_rx[r,l] = y_r rx_y[l] + z_r rx_z[l]
 * and psi_tx[t,l] alike the element's steering phase in unreduced revolutions (spacing sin(th) sin(ph) per y step,
 * spacing cos(th) per z step: what stage 1 writes), beta = bandwidth / carrier_freq and s_k = 1 + beta sc_k / N:
 *   H_wb[u, r, t, k] = sum_l c_l exp(j 2pi (psi_rx[r,l] + psi_tx[t,l]) s_k) exp(-j 2pi dn_l sc_k / N)
 * Equivalently element (r, t) sees path l with its own true delay tau_l - (psi_rx + psi_tx) / f_c: delays are referred to
 * element 0 of each array, where the narrowband array response has zero phase.  sc_k = 0, or carrier_freq -> infinity,
 * gives the narrowband channel.  Everything that acts per path is decided on the centre delay tau_l as without the flag:
 * the clip at dn >= N, the field of view and the patterns, the Doppler term inside c_l, num_paths, compaction, LoS.
 * The flag (value 4; 2 stays an unknown bit):
 *   dmx_path_prep         accepts it; the records are the same bits as without it.
 *   dmx_channels_fd       needs carrier_freq and bandwidth finite and > 0 (else DMX_ERR_ARG) and runs the fp32 vector
 *                         kernel's per-subcarrier body for variant 0 and 1, the accumulate passes beyond 32 path slots
 *                         included; any other explicit variant is DMX_ERR_SHAPE (the matrix-core, folded and small-output
 *                         kernels rest on the separable form H = A G, which the squint removes).  Phases are reduced in
 *                         float64: any int32 subcarrier index is valid.  May be combined with DMX_FLAG_ADAPTIVE_TERMS,
 *                         which changes the order of a user's records only.
 *   dmx_fd_kernel_choice  answers 1.
 *   every other entry point that takes dmx_params (dmx_channels_fd_lpf, dmx_channels_td, dmx_channels_fd_beams,
 *   dmx_beam_power, dmx_channels_fd_direct, every consumer) and every dmx_*_supported query: DMX_ERR_ARG, with the flag
 *   named in dmx_last_error().  Not covered either: frequency-dependent element patterns and path gains, the squint together
 *   with the near field (DMX_FLAG_NEAR_FIELD below is refused beside this flag). */
#define DMX_FLAG_SPATIAL_WIDEBAND 4u

/* Near field: a spherical-wavefront array response per path, in place of the plane wave.  An array is a panel in its local
 * y-z plane, element e = (y, z) at d (0, y, z) wavelengths, d the spacing; stage 1 writes sy = d sin(th) sin(ph) and
 * sz = d cos(th), revolutions per step, per path l and end, on the rotated, FoV-filtered angles.  With the flag the path is
 * a spherical wave from a point at distance R_l wavelengths along its direction, seen from element 0:
 *   R_l     = dn_l carrier_freq / bandwidth     (= tau_l f_c, the path length in wavelengths, from the record's float32 dn)
 *   q_e     = y sy_l + z sz_l                   (the plane-wave phase)
 *   s_e     = d^2 (y^2 + z^2)
 *   psi_e,l = R_l - sqrt(R_l^2 - 2 R_l q_e + s_e)  revolutions
 *           = (2 R_l q_e - s_e) / (R_l + sqrt(R_l^2 - 2 R_l q_e + s_e))    (evaluated this way)
 *           = 0 where the numerator is 0        (element 0 always, where R_l = 0 would make it 0 / 0)
 *   H_nf[u, r, t, k] = sum_l c_l exp(j 2pi (psi_rx[r,l] + psi_tx[t,l])) exp(-j 2pi dn_l sc_k / N)
 * psi is float64, reduced to a revolution before the float32 sin / cos as every array table is; the argument of the root
 * is a squared distance and never negative; R -> infinity gives q_e, the response without the flag; a 1 x 1 array has
 * psi = 0.  The sum stays separable (H = A G), only the array tables change.  Limits of the model: the amplitude is
 * uniform over the aperture (no 1/r taper); the radius is the TOTAL path length - exact for LoS and for chains of specular
 * reflections (the image source), too large for a path through a diffraction or scattering point, which comes out less
 * curved than it is; the two ends are curved independently, so the cross term between two large arrays (LoS MIMO rank
 * from sphericity) is not covered.  Everything else per path - the clip at dn >= N, FoV, patterns, Doppler, num_paths,
 * compaction, LoS - is unchanged, and c_l and dn_l are the same bits as without the flag.
 * The flag (value 16; 2 and 8 stay unknown bits) needs carrier_freq and bandwidth finite and > 0 wherever it is taken
 * (else DMX_ERR_ARG, naming the flag and the field), combines with DMX_FLAG_ADAPTIVE_TERMS and is DMX_ERR_ARG together
 * with DMX_FLAG_SPATIAL_WIDEBAND everywhere:
 *   dmx_path_prep         accepts it; the records are the same bits.
 *   dmx_channels_fd       variants 0 and 1 run the fp32 vector kernel with near-field tables; any other explicit variant is
 *                         DMX_ERR_SHAPE.  dmx_fd_kernel_choice answers 1.
 *   dmx_channel_covariance, dmx_channel_rate, dmx_channel_spectrum, dmx_channel_precoders, dmx_channels_angle_delay,
 *   dmx_codebook_rate, dmx_codebook_rate_subbands, dmx_beam_power (scalar projection for every panel) and their
 *   dmx_*_supported queries accept it with the shape limits of the far field; dmx_cell_rate accepts it per link (links may
 *   differ in flag and carrier).
 *   dmx_channels_fd_lpf, dmx_channels_td, dmx_channels_fd_beams, dmx_channels_fd_direct, dmx_fd_direct_supported:
 *   DMX_ERR_ARG / not taken, with DMX_FLAG_NEAR_FIELD in dmx_last_error(). */
#define DMX_FLAG_NEAR_FIELD 16u

/* Power-averaged beam sweep (RSRP): dmx_beam_power reports mean |F H|^2 in place of mean |F H|.  The flag (value 64; 2, 8
 * and 32 stay unknown bits) is an option of that one call, not of the preparation: the workspace is that of dmx_path_prep
 * WITHOUT the flag, and dmx_beam_power is the only entry point that takes it.  It combines with DMX_FLAG_ADAPTIVE_TERMS and
 * with DMX_FLAG_NEAR_FIELD.  Every other entry point that takes a dmx_params block - dmx_path_prep, dmx_channels_fd,
 * dmx_channels_fd_lpf, dmx_channels_td, dmx_channels_fd_beams, dmx_channels_fd_direct, dmx_fd_kernel_choice, every consumer,
 * every link of dmx_cell_rate - and every dmx_*_supported query: DMX_ERR_ARG, with DMX_FLAG_BEAM_MEAN_POWER in dmx_last_error().  The
 * values are defined at dmx_beam_power below. */
#define DMX_FLAG_BEAM_MEAN_POWER 64u

/* Linear MMSE receiver in the codebook rate: dmx_codebook_rate and dmx_codebook_rate_subbands score a codeword by the
 * post-equalisation SINR of each layer, what a UE that separates its layers with a linear MMSE receiver forms CQI, PMI and
 * rank from, in place of log2 det (the rate of a joint receiver: maximum likelihood, or MMSE with successive cancellation).
 * With E, L, snr_linear, W and the subband partition as defined at those two calls, s = snr_linear / L and
 * A_ck = I_L + s E_ck^H E_ck:
 *   sinr[u, c, i, k] = 1 / [A_ck^-1]_ii - 1                                 (linear MMSE, equal power per layer)
 *   rate_c[u, c]     = 1 / K sum_k sum_i log2(1 + sinr[u, c, i, k]) = -1 / K sum_k sum_i log2 [A_ck^-1]_ii
 * pmi, rate, rate_sb_c, pmi_sb and rate_sb follow from this rate_c exactly as without the flag: the first maximum,
 * rate == rate_c[u, pmi] bit for bit, +0.0 / -1 / +0.0 for a user without a kept path, no output NaN, infinite or negative;
 * launches repeat bit for bit, a user sub-range equals the rows of a whole launch, subband s equals the wideband call on
 * selected_subcarriers[s B : (s + 1) B] and one subband equals the wideband call, all with the flag set on both sides.  The
 * value is at or below the one without the flag (Hadamard's inequality on A^-1), up to rounding.  1 + sinr_i is the Schur
 * complement of A_ck at layer i: the last pivot of the elimination of the rate without the flag, run once per layer with
 * that layer ordered last, every pivot clamped to >= 1 as there.  At L = 1 the two receivers are the same number: the flag
 * then runs the same kernel and every output is bit-equal to the call without it.
 * The flag (value 256; 2, 8, 32 and 128 stay unknown bits) is, like the power option of the beam sweep above, an option of
 * the call and not of the preparation: the workspace is that of dmx_path_prep WITHOUT the flag.  It combines with
 * DMX_FLAG_ADAPTIVE_TERMS and with DMX_FLAG_NEAR_FIELD, and the shape limits are unchanged:
 *   dmx_codebook_rate, dmx_codebook_rate_subbands, dmx_codebook_rate_supported, dmx_codebook_rate_subbands_supported
 *                         take it.
 *   every other entry point that takes a dmx_params block - dmx_path_prep, dmx_channels_fd, dmx_channels_fd_lpf,
 *   dmx_channels_td, dmx_channels_fd_beams, dmx_beam_power, dmx_channels_fd_direct, dmx_fd_kernel_choice, every other
 *   consumer, every link of dmx_cell_rate - and every other dmx_*_supported query: DMX_ERR_ARG, with
 *   DMX_FLAG_RX_LINEAR_MMSE in dmx_last_error().
 * Not covered: the per-layer SINRs as an output, zero-forcing and maximum-ratio receivers, unequal power per layer, the
 * linear receiver in dmx_channel_rate and dmx_cell_rate, L > 4. */
#define DMX_FLAG_RX_LINEAR_MMSE 256u

/* Angle-delay power matrix and delay profile: dmx_channels_angle_delay writes, in place of the complex tensor X it defines
 * below, the two reduced quantities that fingerprinting, localisation and channel-charting models train on.  With X, F,
 * n_rows, n_fft and n_taps as at that call:
 *   P[u, r, t] = sum_{rx < M_rx} |X[u, rx, r, t]|^2      float32 [user_count, n_rows, n_taps]     DMX_FLAG_ANGLE_DELAY_POWER
 *   p[u, t]    = sum_{r < n_rows} P[u, r, t]             float32 [user_count, n_taps]             ... | DMX_FLAG_ANGLE_DELAY_PROFILE
 * raw sums, no division: the angle-delay channel power matrix (ADCPM) and its row sum, the power-delay profile.  With rows
 * that are orthonormal (a unitary DFT codebook) p equals the profile of the antenna domain (Parseval).  The output goes
 * through the unchanged out_c64 parameter, C-contiguous, taps fastest, 4-byte aligned; X is not written
 * anywhere, and nothing beyond the smaller extent is touched.  |X|^2 of one (rx, r, t) is fmaf(im, im, re re) of the fp32
 * value the complex call would store; P adds them in ascending rx, p adds P over the rows in an order fixed by (n_rows,
 * n_taps) alone, all in fp32 without atomics: launches repeat bit for bit, a user sub-range equals the same rows of a whole
 * launch, P is within (M_rx + 2) 2^-24 P + FLT_MIN of the float64 sum over the complex call's own output and p within
 * (n_rows + 1) 2^-24 p + FLT_MIN of the float64 row sum of P (to first order M_rx + 1 and n_rows - 1 roundings; the rest covers
 * the terms of second order and the float32 store).  A user without kept paths gets +0.0 in every element; no output is NaN, infinite or
 * negative; a value below FLT_MIN may come out as 0.
 * The flags (values 1024 and 4096; 2, 8, 32, 128, 512 and 2048 stay unknown bits) are options of the call and not of the
 * preparation, like the options of the beam sweep and of the codebook rate above: the workspace is that of dmx_path_prep
 * WITHOUT them.  DMX_FLAG_ANGLE_DELAY_PROFILE is valid only together with DMX_FLAG_ANGLE_DELAY_POWER; alone it is DMX_ERR_ARG,
 * with both names in dmx_last_error().  They combine with DMX_FLAG_ADAPTIVE_TERMS and with DMX_FLAG_NEAR_FIELD, and the shape
 * limits are unchanged:
 *   dmx_channels_angle_delay, dmx_angle_delay_supported
 *                         take them.
 *   every other entry point that takes a dmx_params block - dmx_path_prep, dmx_channels_fd, dmx_channels_fd_lpf,
 *   dmx_channels_td, dmx_channels_fd_beams, dmx_beam_power, dmx_channels_fd_direct, dmx_fd_kernel_choice, every other
 *   consumer, every link of dmx_cell_rate - and every other dmx_*_supported query: DMX_ERR_ARG, with the flag's name in
 *   dmx_last_error().
 * Not covered: the power per receive element or its maximum over elements, a Doppler axis, the delay spread inside the
 * kernel (it is array code on p), the rx_filter and time-domain forms, the spatial-wideband flag. */
#define DMX_FLAG_ANGLE_DELAY_POWER 1024u
#define DMX_FLAG_ANGLE_DELAY_PROFILE 4096u

/* Serving sets in the cell rate: dmx_cell_rate reads `serving` as a SET of links per user in place of one index, so a user
 * may be served by several links at once - joint transmission from a cluster of base stations (multi-TRP, CoMP, cell-free),
 * several streams to one user in a multi-user group, or, with every link serving, the full-cooperation bound.  The model is
 * the one of dmx_cell_rate: equal power per antenna, no channel knowledge at the transmitters, every link an independent
 * Gaussian codebook.  The values are defined at dmx_cell_rate below.
 * The flag (value 16384; 2, 8, 32, 128, 512, 2048 and 8192 stay unknown bits) is an option of the call and not of the
 * preparation, like the options of the beam sweep, the codebook rate and the angle-delay call above: the workspaces are
 * those of dmx_path_prep WITHOUT it.  It is set on every link of a call or on none: a mix is DMX_ERR_ARG, with
 * DMX_FLAG_SERVING_SET and the first link that differs from link 0 in dmx_last_error().  Per link it combines with
 * DMX_FLAG_ADAPTIVE_TERMS and with DMX_FLAG_NEAR_FIELD as without it; shape limits, the LDS rule and the argument checks
 * are unchanged:
 *   dmx_cell_rate, dmx_cell_rate_supported
 *                         take it.
 *   every other entry point that takes a dmx_params block - dmx_path_prep, dmx_channels_fd, dmx_channels_fd_lpf,
 *   dmx_channels_td, dmx_channels_fd_beams, dmx_beam_power, dmx_channels_fd_direct, dmx_fd_kernel_choice, every other
 *   consumer - and every other dmx_*_supported query: DMX_ERR_ARG, with DMX_FLAG_SERVING_SET in dmx_last_error().
 * Not covered: precoders computed in the library, the uplink, coherent joint precoding with channel knowledge at the
 * transmitters, more than DMX_MAX_LINKS links. */
#define DMX_FLAG_SERVING_SET 16384u

/* Subcarrier index bound of the float32-phase kernels.  The matrix-core and folded kernels (variants 2-5, 8, 10-12, the
 * beam entry points) reduce the phase dn k / N in float32 as qh (k mod 4096) + ql k, whose error grows linearly with
 * |k|: they meet the error claim above (~2e-6 of a user's peak) only while every selected |k| is below this bound.  The
 * fp32 vector kernel (1) and the small-output kernel (9) evaluate the phase in float64 and take any int32 index; the
 * rx_filter path reduces k mod N exactly and is not bounded either.  When the caller promises a uniform spacing
 * (sc_stride > 0) and an index reaches the bound, variant 0 picks 1 (or 9 where the small-output kernel is preferred),
 * and an explicit matrix-core or folded variant, dmx_channels_fd_beams and dmx_beam_power return DMX_ERR_ARG.  Without
 * the promise the library cannot see the indices: the caller keeps them below the bound or passes variant 1 or 9. */
#define DMX_SC_ABS_MAX_F32 32768

/* Optional side products of the path-prep stage (any pointer may be NULL = not wanted).
 * All device pointers; [n_ue, n_paths] arrays are dense row-major with row stride n_paths. */
typedef struct dmx_side {
    uint8_t*  fov_mask;              /* [n_ue, n_paths] 0/1                 dataset.py:494-504 */
    int32_t*  num_paths;             /* [n_ue]                              dataset.py:613-619 */
    int32_t*  los;                   /* [n_ue] in {-1, 0, 1}                dataset.py:569-611 */
    double*   aod_el_rot;            /* [n_ue, n_paths] radians, before FoV masking  dataset.py:341-349 */
    double*   aod_az_rot;
    double*   aoa_el_rot;
    double*   aoa_az_rot;
    float*    power_linear;          /* [n_ue, n_paths] W                   dataset.py:694-696 */
    double*   power_linear_ant_gain; /* [n_ue, n_paths] W                   dataset.py:665-691 */
    uint32_t* max_delay_key;         /* [1], caller zeroes it; order-preserving key of
                                        nanmax(delay[:, :P]) (channel.py:231), see dmx_decode_max_delay */
} dmx_side;

/* ABI version of the loaded library (== DMX_ABI_VERSION of the header it was built from). */
int dmx_version(void);

/* Message of the last failing call on the calling thread ("" if none). */
const char* dmx_last_error(void);

/* Bytes of device workspace dmx_path_prep needs for n_ue users (256-byte aligned base required). */
size_t dmx_workspace_bytes(const dmx_params* prm, int64_t n_ue, int32_t n_paths_loaded);

/* Decode *max_delay_key (copied back to the host) into seconds; NaN when no finite delay was seen. */
float dmx_decode_max_delay(uint32_t key);

/*
 * Stage 1 (replaces dataset.py:310-356 rotate, :461-512 FoV, :665-696 powers/patterns, :569-619
 * LoS/path counts, and the per-path part of channel.py:170-198): one pass over the ray matrices
 * that fills the compact per-path records in `workspace` and the requested side products.
 */
int dmx_path_prep(const dmx_rays* rays, const dmx_params* prm, void* workspace, size_t workspace_bytes,
                  const dmx_side* side, void* stream);

/*
 * Stage 2, frequency domain (replaces dataset.py:398-417 array-response product and the user loop
 * channel.py:264-284): out[u, rx, tx, k] = sum_l a_rx[rx,l] a_tx[tx,l] c_l exp(-j 2pi dn_l sc_k / N)
 * for users [user_begin, user_begin + user_count) of the prepared workspace; `out` points at the
 * first of those users (complex64 [user_count, M_rx, M_tx, K]).
 * variant: 0 = automatic; 1 = fp32 vector kernel; 2 = split-precision MFMA kernel (persistent workgroups of 8
 *          waves, two per CU, or of 4 waves up to 128 subcarriers; non-temporal output stores); 9 = small-output
 *          kernel (one wave per user; automatic when few subcarriers are selected); 12 = folded matrix-core kernel
 *          for at most 128 antenna pairs (needs prm->sc_stride > 0; automatic for every such selection up to 32 pairs and
 *          up to 128 pairs while few subcarriers are selected).
 *          Tuning knobs kept for A/B measurements (all parity-tested): 3 = MFMA with plain stores (16 waves),
 *          4 / 5 / 10 = 4- / 8- / 16-wave workgroups whatever the subcarrier count, 8 = one 16-wave workgroup per
 *          (user, row block) instead of persistent workgroups, 11 = exactly the resident number of persistent
 *          16-wave workgroups.
 */
int dmx_channels_fd(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                    int64_t user_begin, int64_t user_count, void* out_c64, int32_t variant, void* stream);

/* Host-only: the kernel `variant = 0` selects for this shape (1, 2, 9 or 12 above), from measured crossovers; 1 or 9
 * when sc_stride > 0 and an index reaches DMX_SC_ABS_MAX_F32; negative on a bad argument.  No GPU involved. */
int dmx_fd_kernel_choice(const dmx_params* prm, int32_t n_paths_loaded);

/*
 * Single pass for small outputs: ray matrices -> frequency-domain channels in ONE launch, without a workspace (one
 * wave per user keeps its compacted per-path records in LDS; k12_fd_direct.hip).  Meant for the shapes where variant 9
 * runs (DeepMIMO's default call: 8 antenna pairs, one subcarrier), where the records' round trip through HBM is most
 * of the two-call route's traffic.
 *
 * dmx_fd_direct_supported - host-only: 1 if dmx_channels_fd_direct takes this shape, 0 if not (call dmx_path_prep +
 * dmx_channels_fd), negative on a bad argument.  No GPU involved.  Taken: freq_domain = 1, rx_filter = 0, flags = 0,
 * 1 <= n_paths_loaded <= 64, 1 <= min(num_paths, n_paths_loaded) <= 32, n_selected >= 1, and one wave's records and
 * tables (1408 + (M_rx + M_tx + K) * P * 8 bytes) within 156 KB.
 */
int dmx_fd_direct_supported(const dmx_params* prm, int32_t n_paths_loaded);

/*
 * Users [user_begin, user_begin + user_count) of `rays`; out = complex64 [user_count, M_rx, M_tx, K] of the first of
 * them.  side: only fov_mask, num_paths, los, max_delay_key may be non-NULL (indexed by absolute user, as dmx_path_prep
 * writes them; max_delay_key zeroed by the caller); any other non-NULL member is DMX_ERR_ARG.  Unsupported shape:
 * DMX_ERR_SHAPE with a message that names the two-call route.
 * Result: bit-identical to dmx_path_prep + dmx_channels_fd(variant = 9) on the same inputs and side pointers.
 */
int dmx_channels_fd_direct(const dmx_rays* rays, const dmx_params* prm, const dmx_side* side,
                           int64_t user_begin, int64_t user_count, void* out_c64, void* stream);

/*
 * Stage 2, frequency domain with the receive low-pass filter (ofdm.rx_filter = 1; replaces
 * channel.py:166-168, 193-194): g[l,k] = sum_d c_l sinc(d - dn_l) exp(-j 2pi d sc_k / N) is first
 * written to `lpf_workspace` (dmx_lpf_workspace_bytes(prm, user_count, n_paths_loaded) bytes,
 * 256-byte aligned, device), then contracted as in dmx_channels_fd.
 */
size_t dmx_lpf_workspace_bytes(const dmx_params* prm, int64_t user_count, int32_t n_paths_loaded);
int dmx_channels_fd_lpf(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                        int64_t user_begin, int64_t user_count, void* lpf_workspace, size_t lpf_workspace_bytes,
                        void* out_c64, void* stream);

/*
 * Stage 2 with a fused consumer: beam-space channel for a TX codebook F [n_beams, M_tx]
 * (complex64, row-major, device), out[u, rx, b, k] = sum_tx F[b,tx] H[u, rx, tx, k]  - what
 * docs/manual.ipynb cell 105 computes as `F1 @ dataset.channel` after materialising H.  H itself is never
 * written: the projection is folded into the transmit array response before the contraction, so the output
 * (complex64 [user_count, M_rx, n_beams, K]) and the HBM traffic shrink by M_tx / n_beams.
 */
size_t dmx_beam_workspace_bytes(const dmx_params* prm, int64_t user_count, int32_t n_paths_loaded, int32_t n_beams);
int dmx_channels_fd_beams(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                          int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_beams,
                          void* beam_workspace, size_t beam_workspace_bytes, void* out_c64, void* stream);

/*
 * Fused consumer that writes no [N, ., K] tensor at all: the beam-sweep reduction of
 * docs/manual.ipynb cell 105, `np.abs(F1 @ dataset.channel).mean(axis=1).mean(axis=-1)`:
 *   out_mean_amp[u, b] = 1 / (M_rx K) * sum_rx sum_k | sum_tx F[b,tx] H[u, rx, tx, k] |        float32 [user_count, n_beams]
 *   out_best_beam[u]   = argmax_b out_mean_amp[u, b] (first maximum; -1 for a user without paths)   int32 [user_count], may be NULL
 * (cells 110 / 112 take argmax / max of the rounded dBm values 20 log10(.) + 30: the host does that on the small
 * [N, n_beams] result).  Frequency domain without rx_filter; same workspace as dmx_channels_fd_beams.
 * With DMX_FLAG_BEAM_MEAN_POWER in prm->flags (for this call only: the records were prepared without it) the two outputs are
 * the power average, what 3GPP calls RSRP, from the same matrix-core products one instruction before the square root:
 *   out_mean_amp[u, b] = 1 / (M_rx K) * sum_rx sum_k | sum_tx F[b,tx] H[u, rx, tx, k] |^2      linear, the channel's 1/sqrt(N) included
 *   out_best_beam[u]   = its first maximum (-1 and zeros for a user without paths)
 * Both forms sum in a fixed order (no atomics): a launch repeats bit for bit, and a sub-range of users gives the same rows
 * as a whole launch.  The power form is scaled once at the end in float32: a mean below FLT_MIN may come out as 0.
 */
int dmx_beam_power(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                   int64_t user_begin, int64_t user_count, const void* codebook_c64, int32_t n_beams,
                   void* beam_workspace, size_t beam_workspace_bytes, float* out_mean_amp, int32_t* out_best_beam,
                   void* stream);

/*
 * Fused consumer: the per-user spatial covariance of the frequency-domain channel over one array,
 * averaged over the other array and the selected subcarriers, from the workspace of dmx_path_prep - H is never written.
 * With c_l the path coefficient, a_tx[t,l] / a_rx[r,l] the array responses and g[l,k] = exp(-j 2pi dn_l sc_k / N):
 *   H[r,t,k]  = sum_l c_l a_rx[r,l] a_tx[t,l] g[l,k]
 *   R_tx[i,j] = 1 / (M_rx K) sum_r sum_k H[r,i,k] conj(H[r,j,k])                      side = DMX_COV_TX
 *             = sum_l sum_l' a_tx[i,l] Q[l,l'] conj(a_tx[j,l'])
 *   Q[l,l']   = c_l conj(c_l') S[l,l'] D[l,l']
 *   S[l,l']   = 1 / M_rx sum_r a_rx[r,l] conj(a_rx[r,l'])
 *   D[l,l']   = 1 / K sum_k g[l,k] conj(g[l',k])
 *   R_rx[i,j] = 1 / (M_tx K) sum_t sum_k H[i,t,k] conj(H[j,t,k])                      side = DMX_COV_RX (arrays exchanged)
 * out: complex64 interleaved, C-contiguous [user_count, M, M] of users [user_begin, user_begin + user_count), M = M_tx
 * or M_rx.  Every block equals its conjugate transpose exactly, with diagonal imaginary parts 0 and real parts >= 0; a
 * user without kept paths gets zeros.  fp32 arithmetic in a fixed order: launches repeat bit for bit and a user sub-range
 * equals the same rows of a whole launch.  Subcarrier phases are reduced in float64: any int32 index is valid
 * (DMX_SC_ABS_MAX_F32 does not apply).  prm->flags changes the order of a user's records and so the summation order only;
 * the workspace of either arithmetic mode is accepted.
 *
 * dmx_covariance_supported - host-only: 1 if dmx_channel_covariance takes this shape, 0 if not (dmx_last_error() then
 * names the limit), negative on a bad argument (a `side` other than the two above is DMX_ERR_ARG).  No GPU involved.
 * Taken: freq_domain = 1, rx_filter = 0, P = min(num_paths, n_paths_loaded) in 1..32, n_selected >= 1, and one wave's
 * tables within the LDS: (M_out + M_avg + M_out + P + 8) * P * 8 bytes <= 156 KB (159744), M_out the array R is over and
 * M_avg the other one (the kernel takes subcarriers in chunks of 64, 32, 16 or 8, the largest that costs no wave of the
 * workgroup, so 8 decides).  At 25 paths: 2 M_out + M_avg <= 765, e.g. a 64 x 4 BS panel with a 2 x 2 UE on either side;
 * a 32 x 32 BS panel is refused on both sides.
 *
 * dmx_channel_covariance - time domain, rx_filter = 1 or a bad side: DMX_ERR_ARG; an unsupported shape: DMX_ERR_SHAPE with
 * the limit in the message.
 */
#define DMX_COV_TX 0   /* R over the BS array: [user_count, M_tx, M_tx], mean over rx and k */
#define DMX_COV_RX 1   /* R over the UE array: [user_count, M_rx, M_rx], mean over tx and k */
int dmx_covariance_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t side);
int dmx_channel_covariance(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                           int64_t user_begin, int64_t user_count, int32_t side, void* out_c64, void* stream);

/*
 * Fused consumer: the per-user achievable rate (spectral efficiency) of the frequency-domain channel,
 * equal power on every transmit antenna and no channel knowledge at the transmitter, from the workspace of dmx_path_prep -
 * H is never written.  With H_k = H[u, :, :, k] (M_rx x M_tx, including the 1/sqrt(N) factor of the channel tensor) and
 * snr_linear the ratio of the total transmit power to the noise power per subcarrier:
 *   rate_k[u, k] = log2 det(I + (snr_linear / M_tx) H_k H_k^H)       bit/s/Hz   out_rate_k float32 [user_count, K], may be NULL
 *   rate[u]      = 1 / K sum_k rate_k[u, k]                                     out_rate   float32 [user_count]
 * for users [user_begin, user_begin + user_count).  det(I + s H H^H) = det(I + s H^H H): the kernel forms the Gram matrix
 * over the smaller array, m = min(M_rx, M_tx), as the Gram of the channel's rows (positive semidefinite by construction),
 * and takes log2 of the pivots of I + G, each clamped to >= 1 (its lower bound in exact arithmetic).  No output is NaN or
 * negative; a user without kept paths gets +0.0 in both outputs.  fp32 arithmetic in a fixed order, no atomics: launches
 * repeat bit for bit and a user sub-range equals the same rows of a whole launch.  Subcarrier phases are reduced in
 * float64: any int32 index is valid (DMX_SC_ABS_MAX_F32 does not apply).  prm->flags changes the order of a user's records
 * and so the summation order only; the workspace of either arithmetic mode is accepted.
 *
 * dmx_rate_supported - host-only: 1 if dmx_channel_rate takes this shape, 0 if not (dmx_last_error() then names the limit),
 * negative on a bad argument.  No GPU involved.  Taken: freq_domain = 1, rx_filter = 0, P = min(num_paths, n_paths_loaded)
 * in 1..32, n_selected >= 1, m = min(M_rx, M_tx) <= 8, and one wave's tables within the LDS:
 *   (m + M_big + kc) * P * 8 bytes <= 156 KB (159744),   M_big = max(M_rx, M_tx),   kc = min(n_selected, 64)
 * At 25 paths: m + M_big + kc <= 798, e.g. a 64 x 4 BS panel with a 2 x 2 UE at 512 subcarriers (324), DeepMIMO's defaults
 * (8 x 1 / 1 x 1), or a 2 x 1 BS with a 4 x 4 UE (the Gram then runs over the BS side); a 32 x 32 BS panel is refused.
 *
 * dmx_channel_rate - time domain, rx_filter = 1, or an snr_linear that is not finite and > 0 (taken: 1e-70 .. 1e70):
 * DMX_ERR_ARG; an unsupported shape: DMX_ERR_SHAPE with the limit in the message; user_count = 0: DMX_OK, nothing done.
 * out_rate / out_rate_k: 4-byte aligned device pointers.
 */
int dmx_rate_supported(const dmx_params* prm, int32_t n_paths_loaded);
int dmx_channel_rate(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                     int64_t user_begin, int64_t user_count, double snr_linear, float* out_rate, float* out_rate_k,
                     void* stream);

/*
 * Fused consumer, the closed-loop view of the same Gram: the eigenmodes of every subcarrier's channel and the rate with full
 * channel knowledge at the transmitter (water-filling over the modes of a subcarrier), H never written.  H_k and snr_linear
 * as in dmx_channel_rate, m = min(M_rx, M_tx):
 *   gamma[u, k, i] = snr_linear * lambda_i(H_k H_k^H),  i = 0 .. m-1, sorted descending     out_gamma  float32 [user_count, K, m]
 *                    (the mode SNRs: gamma / snr_linear is the eigenvalue, its square root the singular value of H_k)
 *   rate_k[u, k]   = max over p_i >= 0, sum_i p_i = 1 of sum_i log2(1 + p_i gamma_i)         out_rate_k float32 [user_count, K]
 *                  = sum_{i < a} log2(mu gamma_i),  mu = (1 + sum_{i < a} 1 / gamma_i) / a,
 *                    a the largest count of strongest modes with mu > 1 / gamma_{a-1}; modes with gamma_i = 0 take no power
 *   rate[u]        = 1 / K sum_k rate_k[u, k]                                                out_rate   float32 [user_count]
 * Each of the three outputs may be NULL (not all of them).  Both rates spend the same total power ((snr / M_tx) I has trace
 * snr), so this rate_k is never below dmx_channel_rate's, and for m = 1 it is log2(1 + gamma_0).  Every value is finite and
 * >= 0 (gamma is clamped to 0 .. FLT_MAX; modes below 1e-30 count as zero); a user without kept paths gets +0.0 everywhere.
 * The kernel is dmx_channel_rate's with another epilogue: the path coefficients are scaled by sqrt(snr_linear), so the Gram
 * holds mode SNRs, and a cyclic complex Jacobi iteration with a fixed sweep count (m = 1 .. 8: 0, 2, 5, 6, 6, 7, 8, 8; no
 * data-dependent exit) diagonalises it in registers.  Launches repeat bit for bit, a user sub-range equals the same rows of
 * a whole launch, and a launch with fewer outputs writes the same bits.
 * Accuracy: the sweep counts leave the off-diagonal Frobenius norm <= 2^-24 |G|_F except where a non-zero eigenvalue is
 * repeated three times or more; there only the eigenvalue bound holds (every gamma within c_J 2^-24 |G|_F, c_J = 13 * sweeps *
 * m (m - 1) / 2), the off-diagonal one does not.  Usable range: the rotation squares the off-diagonal entries in float32,
 * so mode SNRs (entries of snr_linear * H_k H_k^H) are diagonalised between about 3e-23 and 1.8e19; smaller off-diagonal
 * entries are treated as zero, larger ones overflow and gamma, still finite and >= 0, is then meaningless.
 *
 * dmx_spectrum_supported - the rule of dmx_rate_supported, unchanged.
 * dmx_channel_spectrum - the argument rules of dmx_channel_rate; all three outputs NULL with user_count > 0: DMX_ERR_ARG.
 */
int dmx_spectrum_supported(const dmx_params* prm, int32_t n_paths_loaded);
int dmx_channel_spectrum(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                         int64_t user_begin, int64_t user_count, double snr_linear,
                         float* out_gamma   /* [user_count, K, m] or NULL */,
                         float* out_rate    /* [user_count]       or NULL */,
                         float* out_rate_k  /* [user_count, K]    or NULL */, void* stream);

/*
 * Fused consumer, the third view of the same Gram: what the transmitter and the receiver apply to reach the water-filling
 * rate - the singular vectors of every subcarrier's channel, H never written.  H_k, snr_linear and gamma as in
 * dmx_channel_spectrum, m = min(M_rx, M_tx), L = n_layers in 1..m, H_k = U Sigma V^H with the strongest modes first:
 *   gamma[u, k, i]   = snr_linear * sigma_i^2                          out_gamma  float32   [user_count, K, m]
 *   w_tx[u, k, i, :] = v_i  (precoder, unit norm)                       out_tx_c64 complex64 [user_count, K, L, M_tx]
 *   w_rx[u, k, i, :] = u_i  (combiner, unit norm)                       out_rx_c64 complex64 [user_count, K, L, M_rx]
 *   H_k v_i = sigma_i u_i,   H_k^H u_i = sigma_i v_i,   sigma_i = sqrt(gamma_i / snr_linear)
 * so u_i^H H_k v_i = sigma_i, real and >= 0.  Each of the three outputs may be NULL (not all of them).
 * Gauge: the component of largest modulus (the first on ties) of the SMALLER-side vector of each pair (u_i if M_rx <= M_tx,
 * else v_i) is real and positive, its imaginary part stored as exactly +0; the other vector follows from the relation above.
 * Resolved modes: layer i of an entry (u, k) is present iff
 *   gamma_i > max(c_J * 2^-24 * sum_j gamma_j, 1e-30),   c_J = 13 * sweeps * m (m - 1) / 2  (0 for m = 1)
 * evaluated in float32 as one constant per m times the sum of the sorted gamma in index order.  Below that floor - about
 * -45 dB of the entry's total mode SNR at m = 4, -38 dB at m = 8 - an eigenvalue cannot be told from the rounding of the
 * iteration itself (the accuracy statement of dmx_channel_spectrum).  An absent layer gets +0.0 in every component of both
 * vectors; a user without kept paths gets +0.0 everywhere.
 * The kernel is dmx_channel_spectrum's with a third epilogue: the Jacobi rotations (the same sweep counts) are accumulated in
 * an m x m matrix in registers, whose columns are the smaller-side vectors; the larger-side vectors take a second pass over
 * the tables in LDS, y_i = B x_i / sqrt(gamma_i), and only when that output is asked for.  A pair (p, q) is rotated only
 * where |G_pq| >= 2^-50: below that the float32 squares behind |G_pq| leave the normal range and the rotation's phase would
 * lose its unit modulus.  Usable range therefore: off-diagonal mode-SNR entries below 2^-50 (about 8.9e-16) count as zero;
 * the upper end is dmx_channel_spectrum's.  Because of this gate gamma is held to dmx_channel_spectrum's accuracy statement
 * but is not promised bit-equal to its gamma.
 * Accuracy (float32 model of the iteration on the hard and the repeated-eigenvalue matrices of tests/_spectrum_ref.py): the
 * smaller-side vectors of an entry are orthonormal to |X^H X - I|_F <= 69 * 2^-24 at m = 8 (7 * 2^-24 at m = 2), and each
 * satisfies |G x_i - gamma_i x_i|_2 <= 7.5 * 2^-24 |G|_F, G = snr_linear times the Gram of H_k over the smaller array - a
 * statement about the residual, free of eigenvalue gaps: inside a cluster of equal gamma the vectors span the right subspace
 * and the choice within it is arbitrary.  The larger-side vector is unit to |gamma|_2 / gamma_i times that residual bound.
 * Launches repeat bit for bit, a user sub-range equals the same rows of a whole launch, a launch with fewer outputs writes
 * the same bits, and n_layers = L' writes the first L' layers of n_layers = m.
 *
 * dmx_precoder_supported - the rule of dmx_rate_supported, and 1 <= n_layers <= m (else 0, the limit in dmx_last_error()).
 * dmx_channel_precoders - the argument rules of dmx_channel_spectrum; all three outputs NULL with user_count > 0:
 * DMX_ERR_ARG; n_layers outside 1..m: DMX_ERR_SHAPE; user_count = 0: DMX_OK.  out_gamma: 4-byte aligned, out_tx_c64 /
 * out_rx_c64: 8-byte aligned device pointers.
 */
int dmx_precoder_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_layers);
int dmx_channel_precoders(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                          int64_t user_begin, int64_t user_count, double snr_linear, int32_t n_layers,
                          float* out_gamma   /* [user_count, K, m]       or NULL */,
                          void* out_tx_c64   /* [user_count, K, L, M_tx] or NULL */,
                          void* out_rx_c64   /* [user_count, K, L, M_rx] or NULL */, void* stream);

/*
 * Fused consumer of SEVERAL links at once: the downlink rate of every user under inter-cell interference, no channel tensor
 * written for any link.  Link b = 0 .. n_links-1 stands for one base station: its own dmx_path_prep workspace over the same
 * n_ue users, its own dmx_params (the BS shape may differ from link to link) and snr_b = snr_linear, the total transmit
 * power of that base station over the noise power per subcarrier.  With H_{b,k} = H_b[u, :, :, k] and rho_b = snr_b / M_tx,b
 * (equal power on every antenna, no channel knowledge at the transmitters, as in dmx_channel_rate), for user u with serving
 * link s = s[u]:
 *   N_k            = I + sum_{b != s} rho_b H_{b,k} H_{b,k}^H                    (M_rx x M_rx: the other cells as coloured noise)
 *   A_k            = N_k + rho_s H_{s,k} H_{s,k}^H
 *   rate_k[u, k]   = log2 det A_k - log2 det N_k                  bit/s/Hz   out_rate_k   float32 [user_count, K], may be NULL
 *   rate[u]        = 1 / K sum_k rate_k[u, k]                                out_rate     float32 [user_count]
 *   link_snr[u, b] = snr_b * sum over the kept paths l of |c_{b,l}|^2        out_link_snr float32 [user_count, n_links], may be NULL
 * c_{b,l} are the coefficients of link b's records, the frequency-domain sqrt(p / N) e^{j phase} with the antenna gains, so
 * link_snr is the non-coherent wideband receive SNR of an antenna pair (an RSRP-like quantity), linear, clamped to FLT_MAX.
 * serving: a device int32 [user_count] (entry i belongs to user user_begin + i), any value outside 0 .. n_links-1 meaning "not
 * served"; or NULL, and the kernel serves every user by argmax_b link_snr[u, b], the first on ties, -1 if no link of the user
 * has a kept path.  out_serving (int32 [user_count], may be NULL) receives the link each user was served by: the chosen one,
 * or the given one with every value outside the range replaced by -1.
 * A user who is not served, or whose serving link has no kept path, gets +0.0 in rate and rate_k.  No value is NaN, infinite
 * or negative (the difference of the logarithms is clamped to 0 .. FLT_MAX).  n_links = 1 is dmx_channel_rate: where
 * M_rx <= M_tx the same bits.  The Gram always runs over the UE array, also where M_tx < M_rx.
 * The kernel is dmx_channel_rate's with one more loop: per chunk of 64 subcarriers the links are taken in link order, each
 * in the wave's one LDS slice; the interferers add into one register Gram and A_k is formed by adding the serving link's
 * Gram to those same floats, so an interferer's rounding enters both determinants alike.  fp32 arithmetic in a fixed order,
 * no atomics: launches repeat bit for bit, a user sub-range equals the same rows of a whole launch, a launch with fewer
 * outputs writes the same bits, and links whose users have no kept path change nothing.  Subcarrier phases are reduced in
 * float64: any int32 index is valid.
 *
 * With DMX_FLAG_SERVING_SET in the flags of EVERY link (for this call only: the records were prepared without it) serving[i]
 * is a set of links: bit b (1 << b, b < n_links) means that link b transmits to the user, bits at or above n_links are
 * ignored, a negative entry is the empty set, and serving == NULL means that every link serves every user.  With S_u the
 * set of user u:
 *   N_k            = I + sum_{b not in S_u} rho_b H_{b,k} H_{b,k}^H
 *   A_k            = N_k + sum_{b in S_u} rho_b H_{b,k} H_{b,k}^H
 *   rate_k[u, k]   = log2 det A_k - log2 det N_k,      rate[u] = 1 / K sum_k rate_k[u, k]
 * the sum rate of the set's independent streams at a joint receiver (non-coherent joint transmission); with every link in
 * the set N_k = I and the value is the full-cooperation rate log2 det(I + sum_b rho_b H_b H_b^H).  link_snr is unchanged.
 * out_serving receives the set as read: the bits below n_links, 0 for a negative entry, all n_links bits for NULL.  A user
 * whose set is empty, or none of whose set's links has a kept path, gets +0.0 in rate and rate_k; a link without a kept path
 * contributes nothing on either side; no value is NaN, infinite or negative.  The members add into the serving Gram in link
 * order, everything else into the interference Gram, and A_k is formed on those same floats by the same epilogue, with the
 * same repeatability: launches repeat bit for bit, a user sub-range equals the rows of a whole launch, fewer outputs write
 * the same bits.  A set of exactly one bit, 1 << s, writes rate, rate_k and link_snr bit-equal to the call without the flag
 * and serving = s.  Without the flag every output bit is what it was.
 *
 * dmx_cell_rate_supported - host-only: 1 if dmx_cell_rate takes these links, 0 if not (dmx_last_error() then names the
 * limit), negative on a bad argument; workspace may be NULL.  Taken: 1 <= n_links <= DMX_MAX_LINKS; every link with
 * freq_domain = 1, rx_filter = 0 and P_b = min(num_paths, n_paths_loaded) in 1..32; all links with the same ue_shape,
 * n_subcarriers and n_selected >= 1 - the selection array of link 0 is the one read, the others must hold the same values;
 * M_rx <= 8; and one wave's tables of the largest link within the LDS:
 *   max_b (M_rx + M_tx,b + kc) * P_b * 8 bytes <= 156 KB (159744),   kc = min(n_selected, 64)
 * which does not depend on n_links: the headline shape (64 x 4 BS panel, 2 x 2 UE, 25 paths, 512 subcarriers) is taken for
 * any number of cells, a 32 x 32 panel on a single link refuses the call.
 *
 * dmx_cell_rate - links NULL, a link without params, time domain or rx_filter = 1 on a link, an snr_linear that is not
 * finite and > 0 (taken: 1e-70 .. 1e70), a NULL workspace or out_rate with user_count > 0: DMX_ERR_ARG; an unsupported
 * shape or link count: DMX_ERR_SHAPE with the limit in the message; user_count = 0: DMX_OK, nothing done.  Workspaces:
 * 256-byte aligned; serving and the four outputs: 4-byte aligned device pointers.
 */
#define DMX_MAX_LINKS 8
typedef struct dmx_link {
    const dmx_params* prm;
    const void*       workspace;       /* of dmx_path_prep with prm, over the n_ue users of the call */
    int32_t           n_paths_loaded;
    double            snr_linear;      /* total transmit power of this link over the noise power per subcarrier */
} dmx_link;
int dmx_cell_rate_supported(const dmx_link* links, int32_t n_links);
int dmx_cell_rate(const dmx_link* links, int32_t n_links, int64_t n_ue, int64_t user_begin, int64_t user_count,
                  const int32_t* serving     /* device [user_count] or NULL */,
                  float* out_rate            /* [user_count] */,
                  float* out_rate_k          /* [user_count, K]       or NULL */,
                  int32_t* out_serving       /* [user_count]          or NULL */,
                  float* out_link_snr        /* [user_count, n_links] or NULL */, void* stream);

/*
 * Fused consumer: the angle-delay representation of the frequency-domain channel - a TX codebook over the BS array and an
 * inverse DFT over the subcarriers, cut to the first delay taps - what CSI-feedback, fingerprinting and positioning models
 * train on, from the workspace of dmx_path_prep; H is never written.  H[u, rx, tx, k] is the channel tensor of
 * dmx_channels_fd (rx_filter = 0) on a uniformly spaced selection sc_k = sc_first + k * sc_stride, k = 0 .. K-1, and F a
 * codebook [n_rows, M_tx] (complex64, row-major, device) or NULL, the antenna domain: n_rows = M_tx and F = I.
 *   Y[u, rx, r, k] = sum_tx F[r, tx] H[u, rx, tx, k]
 *   X[u, rx, r, t] = np.fft.ifft(Y, n=n_fft, axis=-1)[..., :n_taps]
 *                  = (1 / n_fft) sum_{k<K} Y[u, rx, r, k] e^{+j 2 pi k t / n_fft},   t = 0 .. n_taps-1
 * out: complex64 interleaved, C-contiguous [user_count, M_rx, n_rows, n_taps], taps fastest - the channel layout with
 * M_tx -> n_rows and K -> n_taps.  Per path, with c_l the path coefficient (Doppler included), dn_l the clipped sample delay,
 * a_rx / a_tx the array responses, N = n_subcarriers, d = sc_stride, s0 = sc_first:
 *   X[u, rx, r, t] = sum_l a_rx[rx, l] f[r, l] c_l D[l, t]
 *   f[r, l] = sum_tx F[r, tx] a_tx[tx, l]          (the projection of dmx_channels_fd_beams; a_tx itself without a codebook)
 *   D[l, t] = (1 / n_fft) e^{-j 2 pi frac(dn_l s0 / N)} e^{j pi (K-1) r} sin(pi K r) / sin(pi r)
 *   r = x - rint(x),   x = t / n_fft - d dn_l / N,   sin(pi K r) / sin(pi r) -> K as r -> 0
 * D is formed in float64: numerator and denominator by angle addition from per-tap values (t / n_fft, K t / n_fft reduced
 * in integers) and per-path values (d dn / N, K d dn / N reduced as the exact product), the limit K where |sin(pi r)| <
 * pi 2^-30 - a path one float32 ulp off a tap keeps 7 digits of the ratio; sc_first may be any int32 (its phase is reduced in
 * float64, DMX_SC_ABS_MAX_F32 does not apply).  The sums run in fp32 in a fixed order, no atomics: launches repeat bit for
 * bit and a user sub-range equals the same rows of a whole launch; a user without kept paths gets +0.0 everywhere.
 * prm->flags changes the order of a user's records and so the summation order only; the workspace of either arithmetic mode
 * is accepted.  With a codebook the projection runs first into `beam_workspace` (dmx_beam_workspace_bytes(prm, user_count,
 * n_paths_loaded, n_rows) bytes, 256-byte aligned, device; unused and may be NULL without a codebook); a BS panel the
 * projection cannot take is DMX_ERR_SHAPE from the call.  With DMX_FLAG_ANGLE_DELAY_POWER in prm->flags (for this call
 * only: the records were prepared without it) out is float32 [user_count, n_rows, n_taps], the sum of |X|^2 over rx, and with
 * DMX_FLAG_ANGLE_DELAY_PROFILE beside it float32 [user_count, n_taps], that summed over the rows as well; both are defined at
 * the flags above.
 *
 * dmx_angle_delay_supported - host-only: 1 if dmx_channels_angle_delay takes this shape, 0 if not (dmx_last_error() then
 * names the limit), negative on a bad argument.  No GPU involved.  Taken: freq_domain = 1, rx_filter = 0, sc_stride > 0 (a
 * single subcarrier counts, stride 1), P = min(num_paths, n_paths_loaded) in 1..32, M_rx <= 8,
 * 1 <= n_selected <= n_fft <= 2^20, 1 <= n_taps <= n_fft, n_rows >= 1, and one wave's tables within the LDS:
 *   (M_rx + min(n_rows, 32) + tc) * P * 8 bytes <= 156 KB (159744),   tc = min(n_taps, 64)
 * (the row table goes through the LDS in chunks of 32 rows, the taps in chunks of 64).  With both chunks bounded the rule
 * refuses nothing the other limits admit: the largest tables, M_rx = 8, n_rows >= 32, n_taps >= 64 at 32 paths, are
 * (8 + 32 + 64) * 32 * 8 = 26624 bytes, two waves per workgroup; it is what the launcher sizes the workgroup by.
 *
 * dmx_channels_angle_delay - time domain, rx_filter = 1, sc_stride = 0 (no spacing promise), or n_rows != M_tx with a NULL
 * codebook: DMX_ERR_ARG; an unsupported shape: DMX_ERR_SHAPE with the limit in the message; a missing, short or misaligned
 * beam workspace with a codebook: DMX_ERR_WORKSPACE; user_count = 0: DMX_OK, nothing done.
 */
int dmx_angle_delay_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_rows, int32_t n_fft, int32_t n_taps);
int dmx_channels_angle_delay(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                             int64_t user_begin, int64_t user_count,
                             const void* codebook_c64 /* [n_rows, M_tx] device, or NULL: antenna domain, n_rows = M_tx */,
                             int32_t n_rows, void* beam_workspace, size_t beam_workspace_bytes /* dmx_beam_workspace_bytes; unused with NULL */,
                             int32_t n_fft, int32_t n_taps, void* out_c64, void* stream);

/*
 * Fused consumer: the rate of every codeword of a finite precoding codebook and the best codeword per user - the precoder-
 * matrix indicator (PMI) of a CSI report and the rate behind its channel-quality indicator - from the workspace of
 * dmx_path_prep; H is never written.  W is a codebook [n_codewords, n_layers, M_tx] (complex64, row-major, device) of C
 * codewords with L layers each; row W[c, i, :] multiplies the BS array as a row of F does in dmx_channels_fd_beams, and
 * H[u, rx, tx, k] is the channel tensor of dmx_channels_fd (rx_filter = 0):
 *   E[u, c, rx, i, k] = sum_tx W[c, i, tx] H[u, rx, tx, k]                          (M_rx x L per codeword and subcarrier)
 *   rate_c[u, c]      = 1 / K sum_k log2 det(I_L + (snr_linear / L) E_{c,k}^H E_{c,k})   out_rate_c float32 [user_count, C], may be NULL
 *   pmi[u]            = argmax_c rate_c[u, c], the first maximum                    out_pmi    int32   [user_count], may be NULL
 *   rate[u]           = rate_c[u, pmi[u]]                                           out_rate   float32 [user_count]
 * snr_linear, the total transmit power over the noise power per subcarrier, is split equally over the L layers.  Codewords are
 * used as given: rows of unit norm keep the transmit power at snr_linear, and that is the caller's business.  The Gram is
 * formed over the layers (L x L, L <= M_rx, positive semidefinite by construction), never over the UE array, whose
 * I + s E E^H is rank-deficient beyond the identity for L < M_rx; the pivots of the elimination are clamped to >= 1 as in
 * dmx_channel_rate.  A user without kept paths gets rate +0.0, pmi -1 and +0.0 in every rate_c.  No output is NaN, infinite
 * or negative.  The projection of the flattened codebook [C * L, M_tx] runs first into `beam_workspace`
 * (dmx_beam_workspace_bytes(prm, user_count, n_paths_loaded, C * L) bytes, 256-byte aligned, device); the kernel then streams
 * that table through the LDS in chunks of whole codewords, L * floor(32 / L) rows.  fp32 arithmetic in a fixed order, no
 * atomics: launches repeat bit for bit, a user sub-range equals the same rows of a whole launch, a launch with fewer outputs
 * writes the same bits, and the rate of a codeword depends on neither its index nor the other codewords (a repeated codeword
 * repeats its bits; the PMI is then the first).  Subcarrier phases are reduced in float64: any int32 index is valid,
 * DMX_SC_ABS_MAX_F32 does not apply.  prm->flags changes the order of a user's records and so the summation order only; the
 * workspace of either arithmetic mode is accepted.
 * A PMI per subband, and with it one call per L for rank adaptation: dmx_codebook_rate_subbands below.  Not covered: L > 4 or
 * L > M_rx, the time domain and rx_filter = 1.
 *
 * dmx_codebook_rate_supported - host-only: 1 if dmx_codebook_rate takes this shape, 0 if not (dmx_last_error() then names the
 * limit), negative on a bad argument.  No GPU involved.  Taken: freq_domain = 1, rx_filter = 0,
 * P = min(num_paths, n_paths_loaded) in 1..32, n_selected >= 1, M_rx <= 8, 1 <= n_layers <= min(M_rx, 4), n_codewords >= 1,
 * n_codewords * n_layers <= 65536, and one wave's tables within the LDS:
 *   (M_rx + min(C * L, rc) + kc) * P * 8 bytes <= 156 KB (159744),   rc = L * floor(32 / L),  kc = min(n_selected, 64)
 * With both chunks bounded the rule refuses nothing the other limits admit: the largest tables, M_rx = 8, 32 rows and 64
 * subcarriers at 32 paths, are (8 + 32 + 64) * 32 * 8 = 26624 bytes, two waves per workgroup; it is what the launcher sizes
 * the workgroup by.
 *
 * dmx_codebook_rate - time domain, rx_filter = 1, a NULL codebook or out_rate with user_count > 0, an snr_linear that is not
 * finite and > 0 (taken: 1e-70 .. 1e70): DMX_ERR_ARG; an unsupported shape, or a BS panel the projection cannot take:
 * DMX_ERR_SHAPE with the limit in the message; a missing, short or misaligned beam workspace: DMX_ERR_WORKSPACE;
 * user_count = 0: DMX_OK, nothing done.  workspace: 256-byte aligned; codebook: 8-byte, the outputs: 4-byte aligned device
 * pointers.
 */
int dmx_codebook_rate_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers);
int dmx_codebook_rate(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                      int64_t user_begin, int64_t user_count,
                      const void* codebook_c64 /* [n_codewords, n_layers, M_tx] device */, int32_t n_codewords, int32_t n_layers,
                      void* beam_workspace, size_t beam_workspace_bytes /* dmx_beam_workspace_bytes(prm, user_count, n_paths_loaded, C * L) */,
                      double snr_linear, float* out_rate /* [user_count] */, int32_t* out_pmi /* [user_count] or NULL */,
                      float* out_rate_c /* [user_count, C] or NULL */, void* stream);

/*
 * The subband form of dmx_codebook_rate: the three parts of a CSI report for one layer count - a PMI and its rate per subband
 * and the wideband pair - in one launch; the projection of the codebook, which does not depend on the subcarriers, runs once.
 * Subbands partition the selection in its own order: with B = subband_size >= 1 and K = n_selected, subband s covers the
 * selection positions s B .. min((s + 1) B, K) - 1, n_sb = ceil(K / B) subbands, the last possibly short; B >= K is one
 * subband.  With E, snr_linear and L as above:
 *   rate_sb_c[u, s, c] = mean over k in subband s of log2 det(I_L + (snr_linear / L) E_{c,k}^H E_{c,k})
 *                                                                    out_rate_sb_c float32 [user_count, n_sb, C], may be NULL
 *   pmi_sb[u, s]       = argmax_c rate_sb_c[u, s, c], the first maximum            out_pmi_sb int32 [user_count, n_sb], may be NULL
 *   rate_sb[u, s]      = rate_sb_c[u, s, pmi_sb[u, s]]                             out_rate_sb float32 [user_count, n_sb]
 *   rate_c[u, c]       = 1 / K sum_s (sum over the subband s), the subbands added in subband order
 *   pmi[u], rate[u]    as in dmx_codebook_rate, from this rate_c; out_rate_c, out_pmi, out_rate as there, each may be NULL
 * A subband is processed exactly as dmx_codebook_rate processes a selection that consists of that subband alone (chunks of
 * min(B, K, 64) subcarriers from the subband's first one, the same summation tree, the chunks in order, times
 * (float)(1.0 / length)).  So rate_sb_c[:, s, :], rate_sb[:, s] and pmi_sb[:, s] equal bit for bit what dmx_codebook_rate returns
 * for the selection selected_subcarriers[s B : (s + 1) B], and with one subband all six outputs equal dmx_codebook_rate bit for
 * bit.  With more than one subband the wideband outputs add the same terms in another order: they agree with dmx_codebook_rate
 * within rounding, not bit for bit.  A user without kept paths gets +0.0 in every rate and -1 in every PMI.  No output is NaN,
 * infinite or negative.  As above: launches repeat bit for bit, a user sub-range equals the same rows of a whole launch, and
 * leaving out optional outputs changes no bit of the others.  n_sb is bounded by K alone: where the codebook spans several
 * chunks of rows a subband's running best lives in out_rate_sb / out_pmi_sb themselves, not in the LDS.
 *
 * dmx_codebook_rate_subbands_supported - host-only, as dmx_codebook_rate_supported with subband_size: a subband_size < 1 is a bad
 * argument (DMX_ERR_ARG); else the limits of dmx_codebook_rate_supported with the LDS rule
 *   (M_rx + min(C * L, rc) + kc_sb) * P * 8 bytes <= 156 KB (159744),   kc_sb = min(subband_size, n_selected, 64)
 * which is never more than the wideband call needs (26624 bytes at most).
 *
 * dmx_codebook_rate_subbands - the argument checks, error codes and alignments of dmx_codebook_rate, with out_rate_sb the output
 * that must not be NULL when user_count > 0; subband_size < 1: DMX_ERR_ARG.  The beam workspace is that of dmx_codebook_rate.
 */
int dmx_codebook_rate_subbands_supported(const dmx_params* prm, int32_t n_paths_loaded, int32_t n_codewords, int32_t n_layers,
                                         int32_t subband_size);
int dmx_codebook_rate_subbands(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                               int64_t user_begin, int64_t user_count,
                               const void* codebook_c64 /* [n_codewords, n_layers, M_tx] device */, int32_t n_codewords, int32_t n_layers,
                               void* beam_workspace, size_t beam_workspace_bytes /* as dmx_codebook_rate */,
                               double snr_linear, int32_t subband_size,
                               float* out_rate_sb /* [user_count, n_sb] */, int32_t* out_pmi_sb /* [user_count, n_sb] or NULL */,
                               float* out_rate_sb_c /* [user_count, n_sb, C] or NULL */, float* out_rate /* [user_count] or NULL */,
                               int32_t* out_pmi /* [user_count] or NULL */, float* out_rate_c /* [user_count, C] or NULL */,
                               void* stream);

/*
 * Stage 2, time domain (replaces channel.py:285-287): out[u, rx, tx, s] = a_rx a_tx sqrt(p) e^{j phase}
 * of the s-th valid path (valid paths compacted to the front, remaining slots zero),
 * complex64 [user_count, M_rx, M_tx, P], P = min(num_paths, n_paths_loaded).
 */
int dmx_channels_td(const dmx_params* prm, const void* workspace, int64_t n_ue, int32_t n_paths_loaded,
                    int64_t user_begin, int64_t user_count, void* out_c64, void* stream);

/*
 * Consumer of the ray records: Dataset.compute_pathloss (dataset.py:541-566).  out: device float32 [n_ue], dB;
 * coherent != 0 sums complex gains, 0 sums amplitudes; NaN where the summed power is not positive.
 */
int dmx_pathloss(const dmx_rays* rays, int32_t coherent, float* out, void* stream);

/* ---- loader step before the path: reference .mat files -> device SoA ------------ */

/* Where one numeric array lives inside a MATLAB level-5 MAT-file image, as written by scipy.io.savemat
 * in the DeepMIMO converter (deepmimo/converter/converter_utils.py:59-85). */
typedef struct dmx_mat_info {
    int32_t class_id;      /* mxCLASS of the array (7 = single, 6 = double, 12 = int32, ...) */
    int32_t data_type;     /* miTYPE of the stored payload (7 = miSINGLE, 9 = miDOUBLE, 5 = miINT32, ...) */
    int32_t elem_bytes;
    int32_t ndim;
    int64_t dims[4];       /* MATLAB order; payload is column-major */
    int64_t data_offset;   /* byte offset of the payload in the file image */
    int64_t data_bytes;
    int32_t compressed;    /* 1: the element is zlib-compressed (miCOMPRESSED) at [comp_offset, +comp_bytes):   */
    int32_t reserved;      /*    inflate it and call dmx_mat5_find again on the inflated element              */
    int64_t comp_offset;
    int64_t comp_bytes;
} dmx_mat_info;

/* Host-side: locate variable `var_name` (NULL = first array) in a MAT-file image.  Replaces the parsing
 * half of scipy.io.loadmat at deepmimo/generator/core.py:241.  No GPU involved. */
int dmx_mat5_find(const void* file_image, size_t len, const char* var_name, dmx_mat_info* info);

/* Device: raw column-major [rows, cols] payload (copied to HBM as stored) -> row-major float32
 * [n_sel, cols_keep], gathering rows d_row_idx (device int64 [n_sel], NULL = the first n_sel rows) and
 * keeping the first cols_keep columns.  Replaces core.py:250 (rx_idxs select) and :254 (max_paths trim). */
int dmx_mat_to_rowmajor_f32(const void* d_payload, int32_t data_type, int64_t rows, int64_t cols,
                            const int64_t* d_row_idx, int64_t n_sel, int32_t cols_keep, float* d_out, void* stream);

/* All ray matrices of a TX/RX pair in one pipeline (core.py:241-254 loads them one `scipy.io.loadmat` at a time): reader
 * threads of the library `pread` the payloads - every file in slices by all threads, file after file - into `staging`
 * (host memory the caller page-locked, e.g. hipHostMalloc; job i's bytes at stage_offset), while the calling thread, as
 * each file completes, queues its asynchronous H2D copy into d_payload and dmx_mat_to_rowmajor_f32 on `stream`.  Returns
 * when everything is QUEUED: `staging`, every d_payload and d_row_idx must stay untouched until the stream has been
 * synchronised.  path == NULL: the job's bytes are in `staging` already (an inflated miCOMPRESSED element). */
typedef struct dmx_mat_job {
    const char* path;        /* file holding the payload, or NULL */
    uint64_t file_offset;    /* dmx_mat_info.data_offset */
    uint64_t nbytes;         /* dmx_mat_info.data_bytes */
    uint64_t stage_offset;   /* where the payload goes inside `staging` */
    void*    d_payload;      /* device, nbytes */
    int32_t  data_type;      /* dmx_mat_info.data_type */
    int32_t  cols_keep;
    int64_t  rows, cols;
    float*   d_out;          /* device float32 [n_sel, cols_keep] */
} dmx_mat_job;
int dmx_mats_to_device(const dmx_mat_job* jobs, int32_t n_jobs, void* staging, const int64_t* d_row_idx, int64_t n_sel,
                       int32_t n_threads, void* stream);

/* ---- two steps before the path: Wireless InSite paths.p2m text -> ray matrices ----- */

/* Receiver count announced on line 22 of a `*.paths.*.p2m` file image (p2m_parser.py:36, 80); -1 on error. */
int64_t dmx_p2m_count_rx(const char* text, size_t len);

/* Host-side parse of a `*.paths.*.p2m` file image into NaN-padded float32 matrices [n_rx, max_paths]
 * (inter_pos: [n_rx, max_paths, max_inter, 3], may be NULL).  Replaces paths_parser,
 * deepmimo/converter/wireless_insite/p2m_parser.py:48-145, before its compress_path_data step. */
int dmx_p2m_parse_paths(const char* text, size_t len, int32_t max_paths, int32_t max_inter, int64_t n_rx,
                        float* aoa_az, float* aoa_el, float* aod_az, float* aod_el, float* delay, float* power,
                        float* phase, float* inter, float* inter_pos);

#ifdef __cplusplus
}
#endif
#endif /* DEEPMIMO_AMD_H */
