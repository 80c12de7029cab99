"""
The restoring step in numpy: the statement of include/cip_restore.h that the
tests compare the library against - the shape formulas, the beam fit on a
window, the support radius, the tap expression and the restore loop itself.
"""
import math

import numpy as np

MAX_RADIUS = 32


def shape(a, b, c):
    """(fwhm_major, fwhm_minor, pa) of the form a da^2 + 2 b da db + c db^2."""
    tr, d = a + c, math.hypot(a - c, 2.0 * b)
    lmin, lmax = (tr - d) / 2.0, (tr + d) / 2.0
    pa = -0.5 * math.atan2(2.0 * b, a - c)
    if pa <= -math.pi / 2.0:
        pa += math.pi
    return 2.0 * math.sqrt(math.log(2.0) / lmin), 2.0 * math.sqrt(math.log(2.0) / lmax), pa


def from_fwhm(major, minor, pa):
    """(a, b, c) of the beam with these FWHMs (pixels) and position angle."""
    lmin, lmax = 4.0 * math.log(2.0) / major ** 2, 4.0 * math.log(2.0) / minor ** 2
    s, k = math.sin(pa), math.cos(pa)
    return lmin * s * s + lmax * k * k, (lmin - lmax) * s * k, lmin * k * k + lmax * s * s


def gaussian(a, b, c, radius):
    """exp(-(a da^2 + 2 b da db + c db^2)) on a (2 r + 1)^2 window."""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    da, db = d[:, None], d[None, :]
    return np.exp(-(a * da * da + 2.0 * b * da * db + c * db * db))


def fit_set(window, cut):
    """The (da, db, y) of the fit set of `window` at `cut`."""
    window = np.asarray(window, dtype=np.float64)
    r = window.shape[0] // 2
    p0 = window[r, r]
    assert window.shape == (2 * r + 1, 2 * r + 1) and np.isfinite(p0) and p0 > 0
    with np.errstate(invalid="ignore"):
        take = window >= cut * p0  # NaN fails
    take[r, r] = False
    ia, ib = np.nonzero(take)
    return (ia - r).astype(np.float64), (ib - r).astype(np.float64), -np.log(window[ia, ib] / p0)


def fit_window(window, cut):
    """(a, b, c, n_fit) minimising sum (y - (a da^2 + b 2 da db + c db^2))^2 over the
    fit set; raises np.linalg.LinAlgError on a singular normal matrix."""
    da, db, y = fit_set(window, cut)
    X = np.stack([da * da, 2.0 * da * db, db * db], axis=1)
    N, rhs = X.T @ X, X.T @ y
    if np.linalg.matrix_rank(N) < 3:
        raise np.linalg.LinAlgError("singular normal matrix")
    a, b, c = np.linalg.solve(N, rhs)
    return float(a), float(b), float(c), len(y)


def radius(a, b, c, tol):
    """The least R >= 0 with exp(-lmin R^2) <= tol."""
    lmin = ((a + c) - math.hypot(a - c, 2.0 * b)) / 2.0
    return math.ceil(math.sqrt(math.log(1.0 / tol) / lmin))


def taps(a, b, c, R):
    """The tap expression, every operation rounded, in the header's order."""
    d = np.arange(-R, R + 1, dtype=np.float64)
    da, db = d[:, None], d[None, :]
    return np.exp(-((a * (da * da) + (2.0 * b) * (da * db)) + c * (db * db)))


def dft_psf(uvw, freq, wgt, pix, half, u_scale=1.0, v_scale=1.0):
    """The (2 half + 1)^2 patch around the centre of the normalised PSF of a
    w = 0 scene, by direct DFT: sum w cos(2 pi f / c (u l + v m)) / sum w."""
    k = 2.0 * np.pi * np.asarray(freq)[None, :] / 299792458.0
    ku = (uvw[:, 0:1] * u_scale * k).ravel()
    kv = (uvw[:, 1:2] * v_scale * k).ravel()
    w = np.asarray(wgt, dtype=np.float64).ravel()
    d = np.arange(-half, half + 1) * pix
    phase = ku[:, None, None] * d[None, :, None] + kv[:, None, None] * d[None, None, :]
    return np.tensordot(w, np.cos(phase), axes=1) / w.sum()


def restore(model, residual, taps_table):
    """out = residual (or +0.0); then, for every non-zero model pixel in
    ascending flat index, out[win] += model.flat[idx] * taps[win']."""
    model = np.asarray(model, dtype=np.float64)
    nx, ny = model.shape
    R = taps_table.shape[0] // 2
    assert taps_table.shape == (2 * R + 1, 2 * R + 1)
    out = np.zeros((nx, ny)) if residual is None else np.array(residual, dtype=np.float64)
    flat = model.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in np.flatnonzero(flat):  # NaN counts as non-zero, -0.0 and +0.0 do not
            i, j = divmod(int(idx), ny)
            i_lo, i_hi = max(i - R, 0), min(i + R + 1, nx)
            j_lo, j_hi = max(j - R, 0), min(j + R + 1, ny)
            # out[i2, j2] takes taps[i2 - i + R][j2 - j + R]
            out[i_lo:i_hi, j_lo:j_hi] += flat[idx] * taps_table[i_lo - i + R:i_hi - i + R, j_lo - j + R:j_hi - j + R]
    return out
