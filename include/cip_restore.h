/*
 * cip_restore.h - the restoring step of libcip_hip.so: the clean beam fitted
 * to the PSF's main lobe and the restored image (model convolved with that
 * beam, plus the residual). Second header of the C ABI; the conventions are
 * those of cip.h (extern "C", 0 or a negative CIP_E* code, the message through
 * cip_last_error(), device pointers on the current device). The reference has
 * no counterpart: it stops at the dirty image.
 *
 * Axes. An image is (nx, ny) row-major fp64, axis 0 <-> l, axis 1 <-> m, as
 * everywhere here. Offsets from a centre are da along axis 0 and db along
 * axis 1, in pixels.
 *
 * The beam is the Gaussian
 *   G(da, db) = exp(-(a da^2 + 2 b da db + c db^2))
 * with a positive definite form: a > 0, c > 0, a c - b^2 > 0.
 *
 * Shape <-> quadratic form. With tr = a + c and d = hypot(a - c, 2 b) the
 * eigenvalues are lmin = (tr - d) / 2 and lmax = (tr + d) / 2, and
 *   fwhm_major = 2 sqrt(ln 2 / lmin)      fwhm_minor = 2 sqrt(ln 2 / lmax)
 *   pa = -0.5 atan2(2 b, a - c), plus pi when that is <= -pi / 2
 * (pa: the major axis from +axis 1 (+m, north) towards +axis 0 (+l, east), in
 * (-pi/2, pi/2]; a circular beam has pa = 0). The inverse, cip_beam_from_fwhm:
 *   lmin = 4 ln 2 / major^2, lmax = 4 ln 2 / minor^2, s = sin pa, k = cos pa
 *   a = lmin s^2 + lmax k^2    b = (lmin - lmax) s k    c = lmin k^2 + lmax s^2
 * G is 0.5 at half the major FWHM along the major axis.
 *
 * Fit (cip_beam_fit_window). `window` is (2 r + 1)^2 row-major HOST fp64 with
 * the PSF's centre pixel at [r][r]; NaN marks a position outside the PSF.
 * p0 = window[r][r] must be finite and > 0. The fit set is every
 * (da, db) != (0, 0) with window[da + r][db + r] >= cut p0 (NaN fails the
 * comparison and drops out). Over it
 *   sum (y - (a da^2 + b (2 da db) + c db^2))^2,   y = -log(window / p0),
 * is minimised: 3 x 3 normal equations in fp64, solved on the host. n_fit is
 * the size of the set.
 *
 * Taps (cip_beam_taps). For a radius R the table is (2 R + 1)^2 row-major,
 *   taps[(da + R) (2 R + 1) + (db + R)]
 *       = exp(-((a (da da) + (2.0 b) (da db)) + c (db db)))
 * computed on the host in fp64 with da, db as doubles, every operation
 * rounded (no FMA). cip_restore uploads exactly this table, so a caller that
 * reads it can restate the restore to the bit without sharing an exp.
 *
 * Restore (cip_restore), rounding included:
 *   out[i, j] = residual ? residual[i, j] : +0.0
 *   for every model pixel (i', j') with model[i', j'] != 0 (so +0.0 and -0.0
 *       are skipped; NaN is not), |i - i'| <= R and |j - j'| <= R, in
 *       ascending flat index i' ny + j':
 *     out[i, j] = out[i, j] + (model[i', j'] taps[i - i' + R][j - j' + R])
 * The product and the add are each one rounded fp64 operation (no FMA) and
 * the order of the adds is the one stated, so the result is bit-identical to
 * the numpy loop
 *   for idx in np.flatnonzero(model): out[win] += model.flat[idx] * taps[win']
 * No atomics: identical calls give identical bits. R = 0 gives
 * out = residual + model taps[0], and taps[0] = 1.
 */
#ifndef CIP_RESTORE_H
#define CIP_RESTORE_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cip_beam { /* HOST memory; pixel units */
  double a, b, c;                /* G(da, db) = exp(-(a da^2 + 2 b da db + c db^2)) */
  double fwhm_major, fwhm_minor; /* pixels */
  double pa;                     /* radians, in (-pi/2, pi/2] */
  int64_t n_fit;                 /* pixels that entered the fit (0: beam given, not fitted) */
} cip_beam;
#define CIP_RESTORE_MAX_RADIUS 32
#define CIP_BEAM_FIT_RADIUS 8 /* default fit-window half width */
#define CIP_BEAM_FIT_CUT 0.35 /* default cut, relative to the PSF's centre pixel */

/* Host-only. Fills every field (n_fit = 0). CIP_EINVAL unless both FWHMs are
 * finite and fwhm_major >= fwhm_minor > 0, with pa finite; out NULL. */
int cip_beam_from_fwhm(double fwhm_major, double fwhm_minor, double pa,
                       cip_beam* out);

/* Host-only: the fit defined above. CIP_EINVAL: window or out NULL,
 * 0 < cut < 1 violated, radius outside 1 .. 64, a centre pixel that is not
 * finite or not > 0. CIP_ERANGE, with a message that says to lower cut or to
 * pass a beam: the normal matrix is singular or the solution not finite (a PSF
 * narrower than about 2.4 pixels at cut 0.5 leaves only the four axis
 * neighbours, whose determinant is exactly zero), or the fitted form is not
 * positive definite. */
int cip_beam_fit_window(const double* window, int64_t radius, double cut,
                        cip_beam* out);

/* The fit on a DEVICE PSF (psf_nx, psf_ny) whose centre pixel is
 * (psf_cx, psf_cy); -1 for a centre means psf_n / 2, as for cip_hogbom_clean.
 * The (2 radius + 1)^2 window around the centre is copied to the host (one
 * 2-D copy of the part inside the PSF, positions outside it are NaN; one wait
 * on hip_stream) and handed to cip_beam_fit_window: same code, same result.
 * No kernel. CIP_EINVAL also for a NULL psf, a dimension < 1 and a centre
 * outside the PSF. */
int cip_beam_fit(const double* psf, int64_t psf_nx, int64_t psf_ny,
                 int64_t psf_cx, int64_t psf_cy, double cut, int64_t radius,
                 void* hip_stream, cip_beam* out);

/* Host-only. The least R >= 0 with exp(-lmin R^2) <= tol:
 * ceil(sqrt(log(1 / tol) / lmin)), from the beam's a, b, c alone. Returns R
 * (>= 0) or a CIP_E* code. CIP_EINVAL: beam NULL or not positive definite,
 * 0 < tol < 1 violated. CIP_ERANGE: R > CIP_RESTORE_MAX_RADIUS (at tol = 1e-8
 * a major FWHM up to 12.5 pixels fits). */
int cip_beam_radius(const cip_beam* beam, double tol);

/* Host-only. taps_out: HOST (2 radius + 1)^2 doubles, the table defined
 * above. CIP_EINVAL: NULL pointers, a beam that is not positive definite,
 * radius outside 0 .. CIP_RESTORE_MAX_RADIUS. */
int cip_beam_taps(const cip_beam* beam, int64_t radius, double* taps_out);

/* The restore defined above. model, residual (may be NULL) and out are DEVICE
 * (nx, ny) fp64 images. out may be residual (in place); it must not be model.
 * Only a, b, c of the beam are read. radius < 0 means
 * cip_beam_radius(beam, 1e-8), with its CIP_ERANGE. Stream-ordered on
 * hip_stream: the call returns once its work is queued and never waits for
 * the device; the images must stay valid until the stream reaches that work.
 * CIP_EINVAL: NULL model / out / beam, out == model, a dimension < 1,
 * radius > CIP_RESTORE_MAX_RADIUS, a beam that is not positive definite. */
int cip_restore(const double* model, const double* residual, int64_t nx,
                int64_t ny, const cip_beam* beam, int64_t radius,
                void* hip_stream, double* out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_RESTORE_H */
