/*
 * cip_mosaic.h - facet mosaicking in libcip_hip.so: facet images, each on the
 * tangent plane at its own centre (cip_facet_rephase + cip_ms2dirty), are
 * resampled onto one wide-field plane at the phase centre.
 * Eighth header of the C ABI; the conventions are those of cip.h (extern "C",
 * 0 or a negative CIP_E* code, the message through cip_last_error(), device
 * pointers on the current device unless marked HOST). The reference has no
 * counterpart: it makes one image on one plane.
 *
 * Images are row-major float64. The output plane is (nx, ny) with pixel sizes
 * (px, py), its pixel (nx/2, ny/2) at the phase centre. A facet is (fnx, fny)
 * with pixel sizes (fpx, fpy) on the tangent plane at (l0, m0), its pixel
 * (fnx/2, fny/2) at the facet centre (integer division throughout).
 *
 * Geometry. For the output pixel (i, j):
 *   l = (i - nx/2) px,  m = (j - ny/2) py,  n = sqrt(1 - l^2 - m^2)
 *   n0 = sqrt(1 - l0^2 - m0^2),  c = 1 / (1 + n0)
 *   q0 = (1 - c l0^2) l - c l0 m0 m - l0 n
 *   q1 = -c l0 m0 l + (1 - c m0^2) m - m0 n
 *   q2 = l0 l + m0 m + n0 n            (the facet-plane n of this direction)
 *   x = q0 / fpx + fnx/2,  y = q1 / fpy + fny/2
 * q = Q^T s: Q is the minimal rotation that takes (0, 0, 1) to (l0, m0, n0),
 * the one cip_facet_rephase rotates the baselines by. The frames are rotated,
 * not shifted, so the facets are resampled, not pasted.
 *
 * Taps, per axis. ix = floor(x), fx = x - ix; the 2 half taps sit on the
 * pixels ix + k, k = -half + 1 .. half, with the values h(fx - k) divided by
 * their own sum (a constant image is reproduced; the flux scale is kept). This
 * sum and the two of `val` below add their terms from the outermost pair of
 * taps inwards (k = -half + 1, half, -half + 2, half - 1, .., 0, 1), the small
 * terms first, so the taps of a constant image sum to 1 within a few ulp:
 *   h(t) = sinc(t) exp(beta (sqrt(1 - (t / half)^2) - 1)),  |t| < half
 *   h(t) = 0,                                               |t| >= half
 * sinc(t) = sin(pi t) / (pi t), sinc(0) = 1; the sine is sinpi, so the taps at
 * fx = 0 are a delta. This is a sinc windowed by the gridder's own
 * exponential of a semicircle; with images band-limited to nu_max cycles per
 * facet pixel, beta = pi half (1 - 2 nu_max) (cip_mosaic_beta) puts the
 * window's spectral half-width beta / (2 pi half) into the guard band
 * 0.5 - nu_max, and the error falls exponentially with `half`.
 *
 * Validity and weight.
 *   lo_x = trim + half - 1,  hi_x = fnx - 1 - trim - half   (likewise y)
 *   dx = min(x - lo_x, hi_x - x),  dy likewise
 *   w = min(1, (dx + 1) / (feather + 1)) min(1, (dy + 1) / (feather + 1))
 *       if dx >= 0 and dy >= 0 and q2 > 0, else w = 0.
 * `trim` facet edge pixels are ignored; `feather` (pixels) blends overlapping
 * facets. Every tap of a pixel with w > 0 lies inside the facet.
 *
 * Value. val = sum_k tx[k] (sum_k' ty[k'] facet[ix + k, iy + k']), both sums
 * in that order; with CIP_MOSAIC_NSCALE val is multiplied by q2 / n:
 * w-stacked facets carry 1 / n' of their own plane, and the mosaic then
 * carries the 1 / n of its plane, as a w-stacked image of the whole field.
 *
 * cip_mosaic_add: num_io[p, i, j] += w val_p for the planes p of `facet`
 * (nplane, fnx, fny), num_io being (nplane, nx, ny), and wsum_io[i, j] += w,
 * for every output pixel with w > 0. Asynchronous on hip_stream; no workspace,
 * nothing allocated. One thread owns one output pixel, the planes share its
 * geometry and taps, there are no atomics: the result depends on the order of
 * the calls only. Only the facet's footprint is launched (a conservative
 * bounding box derived on the host); a facet that misses the output plane is
 * a no-op that returns CIP_OK. The facet must not overlap num_io or wsum_io.
 *
 * cip_mosaic_finish: num_io[p, i, j] = num_io[p, i, j] / wsum[i, j] where
 * wsum > 0, `fill` elsewhere (fill may be NaN). Synchronous on hip_stream;
 * *n_uncovered_out = the number of pixels (of one plane) with wsum <= 0.
 *
 * cip_mosaic_beta and cip_mosaic_taps are host-only (no device is touched):
 * the rule above, and the normalised taps of one axis as the kernel forms them.
 *
 * CIP_EINVAL, all checked before any device work, the message naming the
 * function: NULL pointers; a dimension or nplane < 1; nx ny nplane (or the
 * facet stack) overflowing int64; a pixel size not finite or <= 0; half
 * outside 2 .. CIP_MOSAIC_MAX_HALF; beta not finite or < 0; trim < 0; feather
 * not finite or < 0; flag bits other than CIP_MOSAIC_NSCALE; l0^2 + m0^2 >= 1
 * (or not finite); an output corner with l^2 + m^2 >= 1; a facet too small to
 * hold a valid pixel (hi < lo); for cip_mosaic_beta nu_max outside [0, 0.5);
 * for cip_mosaic_taps frac outside [0, 1).
 */
#ifndef CIP_MOSAIC_H
#define CIP_MOSAIC_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CIP_MOSAIC_MAX_HALF 8
#define CIP_MOSAIC_NSCALE 1 /* multiply by q2 / n (w-stacked facets) */

/* HOST memory */
typedef struct cip_mosaic_geom {
  int64_t nx;
  int64_t ny;
  double px;
  double py;
  int64_t fnx;
  int64_t fny;
  double fpx;
  double fpy;
  int32_t half;
  int32_t flags;
  double beta;
  int64_t trim;
  double feather;
} cip_mosaic_geom;

int cip_mosaic_beta(int half, double nu_max, double* beta_out);

int cip_mosaic_taps(int half, double beta, double frac, double* taps_out);

int cip_mosaic_add(const cip_mosaic_geom* g, const double* facet, int64_t nplane, double l0, double m0,
                   void* hip_stream, double* num_io, double* wsum_io);

int cip_mosaic_finish(double* num_io, const double* wsum, int64_t nplane, int64_t nx, int64_t ny, double fill,
                      void* hip_stream, int64_t* n_uncovered_out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_MOSAIC_H */
