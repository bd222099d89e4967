"""Host-side geometry utilities of the public API (deepmimo/generator/geometry.py).

The per-path geometry of the hot path (rotation, FoV, array response) runs on the GPU
(csrc/k1_path_prep.hip, csrc/k2_channel_fd*.hip).  What stays on the host is the one-vector
utility ``steering_vec`` (geometry.py:322-339, exported at deepmimo/__init__.py:36-38) that users
call to build beam codebooks, the orthonormal DFT codebook ``dft_codebook`` (extension: the angular side of
``Dataset.compute_angle_delay``), the element-index helper they need, and ``pattern_gain`` (extension): the element gain
stage 1 applies for each ``radiation_pattern``, restated in NumPy for plotting and checking."""
from __future__ import annotations

import numpy as np


def _ant_indices(panel_size) -> np.ndarray:
    """[M, 3] element indices of an [Mh, Mv] panel: x = 0, y fastest, z slowest (geometry.py:105-120)."""
    mh, mv = int(panel_size[0]), int(panel_size[1])
    m = np.arange(mh * mv)
    return np.stack([np.zeros_like(m), m % mh, m // mh], axis=1)


def steering_vec(array, phi: float = 0, theta: float = 0, spacing: float = 0.5) -> np.ndarray:
    """Normalised array response [M, 1] for a beam towards (phi, theta) degrees.

    Same argument convention as the reference, including its swap: the response is evaluated at
    zenith = phi and azimuth = theta + 90 deg (geometry.py:338)."""
    idx = _ant_indices(array)
    kd = 2 * np.pi * spacing
    zen, az = phi * np.pi / 180, theta * np.pi / 180 + np.pi / 2
    gamma = 1j * kd * np.array([np.sin(zen) * np.cos(az), np.sin(zen) * np.sin(az), np.cos(zen)])
    resp = np.exp(idx @ gamma).reshape(-1, 1)
    return resp / np.linalg.norm(resp)


def wideband_array_response(shape, spacing: float = 0.5, theta: float = 0, phi: float = 0, freq_ratio=1.0) -> np.ndarray:
    """``steering_vec(shape, phi, theta, spacing)`` at another frequency (extension): the same expression with the element
    spacing measured in wavelengths of ``freq_ratio * f_c``, i.e. ``spacing * freq_ratio``.  ``freq_ratio`` is
    ``s_k = 1 + (bandwidth / carrier_freq) * sc_k / N`` for subcarrier ``sc_k`` of a spatial-wideband channel
    (``compute_channels(spatial_wideband=True)``): a beam steered with ``steering_vec`` at the carrier meets this response
    at the band edges, which is beam squint.  A scalar gives [M, 1] - with ``freq_ratio = 1`` exactly ``steering_vec`` - and
    a 1-D array of K ratios [M, K], every column normalised."""
    idx = _ant_indices(shape)
    zen, az = phi * np.pi / 180, theta * np.pi / 180 + np.pi / 2
    ratios = np.asarray(freq_ratio, dtype=np.float64)
    if ratios.ndim > 1 or not np.all(np.isfinite(ratios)):
        raise ValueError("wideband_array_response: freq_ratio must be a finite scalar or 1-D array")
    cols = []
    for f in ratios.reshape(-1):
        kd = 2 * np.pi * (spacing * float(f))
        gamma = 1j * kd * np.array([np.sin(zen) * np.cos(az), np.sin(zen) * np.sin(az), np.cos(zen)])
        resp = np.exp(idx @ gamma).reshape(-1, 1)
        cols.append(resp / np.linalg.norm(resp))
    return np.concatenate(cols, axis=1) if cols else np.zeros((len(idx), 0), dtype=np.complex128)


def near_field_phase(shape, spacing, theta, phi, distance) -> np.ndarray:
    """The phase of every element of an [Mh, Mv] panel for a spherical wave, in revolutions (extension): NumPy float64
    [..., M] over the broadcast shape of ``theta`` (zenith), ``phi`` (azimuth) - radians, in the panel's own frame, what
    stage 1's rotated angles are - and ``distance`` (wavelengths, >= 0, ``np.inf`` allowed).  Element e = (y, z) sits at
    ``spacing * (0, y, z)`` wavelengths and the source ``distance`` wavelengths from element 0 along (theta, phi):

        q   = spacing * (y sin(theta) sin(phi) + z cos(theta))                    # the plane-wave phase
        s   = spacing^2 (y^2 + z^2)
        psi = R - sqrt(R^2 - 2 R q + s) = (2 R q - s) / (R + sqrt(R^2 - 2 R q + s)),   0 where 2 R q = s

    the definition of DMX_FLAG_NEAR_FIELD (include/deepmimo_amd.h), evaluated in its second form; R = inf gives q."""
    idx = _ant_indices(shape).astype(np.float64)
    y, z = idx[:, 1], idx[:, 2]
    theta, phi, R = np.broadcast_arrays(np.asarray(theta, np.float64), np.asarray(phi, np.float64), np.asarray(distance, np.float64))
    if np.any(np.isnan(R)) or np.any(R < 0):
        raise ValueError("near_field_phase: distance must be >= 0 wavelengths (np.inf for the plane wave)")
    theta, phi, R = theta[..., None], phi[..., None], R[..., None]
    d = float(spacing)
    q = d * (y * np.sin(theta) * np.sin(phi) + z * np.cos(theta))
    s = d * d * (y * y + z * z)
    far = np.isinf(R)
    Rf = np.where(far, 0.0, R)
    num = 2.0 * Rf * q - s
    arg = np.maximum(Rf * Rf - num, 0.0)
    den = Rf + np.sqrt(arg)
    psi = np.where(num == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
    return np.where(far, q, psi)


def near_field_response(shape, spacing: float = 0.5, theta=np.pi / 2, phi=0.0, distance=np.inf) -> np.ndarray:
    """``exp(j 2 pi psi)`` of ``near_field_phase``: the array response of an [Mh, Mv] panel to a spherical wave from
    ``distance`` wavelengths along zenith ``theta`` / azimuth ``phi`` (radians, the panel's frame), complex128 [..., M],
    not normalised (extension).  ``distance = np.inf`` is the phase law of ``steering_vec``: ``sqrt(M) *
    steering_vec(shape, phi=degrees(theta), theta=degrees(phi) - 90, spacing)[:, 0]``.  The amplitude is uniform over the
    aperture (no 1/r taper), as in the kernels."""
    return np.exp(2j * np.pi * near_field_phase(shape, spacing, theta, phi, distance))


def focus_codebook(shape, spacing: float = 0.5, theta=np.pi / 2, phi=0.0, distance=np.inf) -> np.ndarray:
    """A polar-domain (beam-focusing) codebook (extension): for arrays of B focal points - ``theta``, ``phi`` in radians,
    ``distance`` in wavelengths, broadcast against each other - the rows ``conj(near_field_response) / sqrt(M)``,
    complex128 [B, M], each of unit norm.  Usable as the ``codebook`` of every call that takes one (it is applied without a
    conjugate): on a near-field view the row at a LoS user's own (theta, phi, R) collects ``sqrt(M) * sum |c|``, which the
    plane-wave row ``distance = np.inf`` at the same angle no longer does inside the Fraunhofer distance."""
    resp = near_field_response(shape, spacing, theta, phi, distance)
    resp = resp.reshape(-1, resp.shape[-1])
    return np.conj(resp) / np.sqrt(resp.shape[-1])


def fraunhofer_distance(shape, spacing: float = 0.5) -> float:
    """``2 D^2`` in wavelengths, ``D = spacing * sqrt((Mh - 1)^2 + (Mv - 1)^2)`` the panel diagonal (extension): beyond it
    a spherical wavefront deviates from the plane wave by less than 1/16 wavelength over the aperture."""
    mh, mv = int(shape[0]), int(shape[1])
    return 2.0 * float(spacing) ** 2 * float((mh - 1) ** 2 + (mv - 1) ** 2)


def pattern_gain(name: str, theta, phi=None):
    """Linear power gain of one antenna element with the radiation pattern `name`, as stage 1 applies it to a path
    (``power_linear_ant_gain = power_linear * g_tx * g_rx``): NumPy float64, angles in RADIANS in the panel's own frame
    (after ``rotation``): zenith `theta` in [0, pi], azimuth `phi` in (-pi, pi], boresight theta = pi/2, phi = 0.

    * ``"isotropic"``: the float 1.0.
    * ``"halfwave-dipole"``: 1.643 cos^2(pi/2 cos theta) / sin theta where |sin theta| > 1e-10, else 0 (`phi` unused).
    * ``"tr38901"`` (extension): the sector element of 3GPP TR 38.901 Table 7.3-1, with b = 65 degrees,

          A_v = min(12 ((theta - pi/2) / b)^2, 30),  A_h = min(12 (phi / b)^2, 30),  A = min(A_v + A_h, 30)
          gain = 10^((8 - A) / 10)            8 dBi at boresight, floor -22 dBi

    A NaN angle (no path, or a path the field of view masks) gives 0."""
    if name == "isotropic":
        return 1.0
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if name == "halfwave-dipole":
            s = np.sin(theta)
            ok = np.abs(s) > 1e-10                               # False for NaN
            return np.where(ok, 1.643 * (np.cos(np.pi / 2 * np.cos(theta)) ** 2 / np.where(ok, s, 1.0)), 0.0)
        if name == "tr38901":
            if phi is None:
                raise ValueError("pattern_gain: 'tr38901' depends on the azimuth, give phi")
            phi = np.asarray(phi, dtype=np.float64)
            b = np.deg2rad(65.0)
            a_v = np.minimum(12.0 * ((theta - np.pi / 2) / b) ** 2, 30.0)
            a_h = np.minimum(12.0 * (phi / b) ** 2, 30.0)
            gain = 10.0 ** ((8.0 - np.minimum(a_v + a_h, 30.0)) / 10.0)
            return np.where(np.isnan(theta) | np.isnan(phi), 0.0, gain)
    raise NotImplementedError(f"The given '{name}' antenna radiation pattern is not applicable.")


def dft_codebook(shape) -> np.ndarray:
    """Orthonormal 2-D DFT codebook of an [Mh, Mv] panel, complex64 [M, M] with M = Mh * Mv (extension):

        F[by + Mh * bz, y + Mh * z] = exp(-2j * pi * (by * y / Mh + bz * z / Mv)) / sqrt(M)

    in the element order of `_ant_indices` (y fastest).  Rows are beams: ``F @ H`` is the channel in the angular domain,
    and ``F @ F.conj().T`` is the identity."""
    mh, mv = int(shape[0]), int(shape[1])
    if mh < 1 or mv < 1:
        raise ValueError(f"dft_codebook: panel shape entries must be >= 1, got {tuple(shape)}")
    idx = _ant_indices((mh, mv))
    y, z = idx[:, 1], idx[:, 2]
    phase = np.outer(y, y) / mh + np.outer(z, z) / mv
    return (np.exp(-2j * np.pi * phase) / np.sqrt(mh * mv)).astype(np.complex64)
