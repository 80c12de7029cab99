/*
 * cip_ms.h - multiscale CLEAN (Cornwell 2008) with circular Gaussian scale
 * kernels in libcip_hip.so: the scale taps, the separable convolution and the
 * minor cycle over S = nscales scale-smoothed images. Sixth header of the C
 * ABI; the conventions are those of cip.h (extern "C", 0 or a negative CIP_E*
 * code, the message through cip_last_error(), device pointers on the current
 * device unless marked HOST). The reference has no counterpart: it stops at
 * the dirty image.
 *
 * Scale taps (host only, fp64, no FMA). `width` is the FWHM of a scale in
 * pixels, 0 or >= 1. Width 0 has radius 0 and the single tap 1.0. Otherwise,
 * with c = (4.0 log(2.0)) / (width width): e[d] = exp(-((d d) c)) for
 * d = -R .. R, sum = the e[d] added in ascending d, taps[d + R] = e[d] / sum.
 * The 2-D scale kernel is the outer product of the taps with themselves and
 * has unit sum. cip_ms_scale_radius returns ceil(sqrt(log(1 / tol) / c)), the
 * rule of cip_beam_radius (0 for width 0): CIP_ERANGE above
 * CIP_MS_MAX_RADIUS, CIP_EINVAL unless 0 < tol < 1 and width is 0 or >= 1 and
 * finite. cip_ms_scale_taps writes the 2 radius + 1 taps: CIP_EINVAL for a
 * width as above, a radius outside 0 .. CIP_MS_MAX_RADIUS, a width 0 with a
 * radius other than 0, or NULL taps_out. The table is readable and
 * cip_ms_convolve takes taps as an argument, so a test shares no exp with the
 * library.
 *
 * cip_ms_convolve, rounding included: every product and every sum is one
 * rounded fp64 operation, never an FMA. `in` and `out` are (nx, ny) row-major
 * as in cip.h, `taps` 2 radius + 1 values in HOST memory.
 *   pass 1: tmp[i, j] = +0.0, then for d = -R .. R ascending with
 *           0 <= j + d < ny: tmp[i, j] = tmp[i, j] + (taps[d + R] in[i, j + d]).
 *   pass 2: the same along axis 0, from tmp into out, with the same taps.
 * Terms whose index falls outside the image are skipped, not added as zeros.
 * tmp is a grow-only workspace buffer; out == in is allowed. The call only
 * queues work on hip_stream, like cip_restore. No atomics: identical calls
 * give identical bits. CIP_EINVAL: NULL in / taps / out, a dimension < 1, a
 * radius outside 0 .. CIP_MS_MAX_RADIUS, a tap that is not finite, nx ny
 * overflowing int64.
 *
 * cip_ms_clean: the minor cycle. residual_io is (S, nx, ny), plane s the
 * residual smoothed with scale s. psf holds S (S + 1) / 2 planes (psf_nx,
 * psf_ny), every plane with the same centre pixel (psf_cx, psf_cy), -1:
 * psf_n / 2; plane tri(s, q) = s S - s (s - 1) / 2 + (q - s), s <= q, is the
 * PSF smoothed with scales s and q. select_weight and flux_scale are S values
 * each in HOST memory: inputs, as hinv is for cip_mfs_clean (the library
 * derives nothing). mask (nx, ny) uint8 as for cip_hogbom_clean, one for all
 * scales. model_io is (S, nx, ny), one delta model per scale, may be NULL.
 *
 * The operator, rounding included (one rounded fp64 operation per product,
 * sum and difference, never an FMA). For k = 0, 1, ...:
 *   1. for every allowed pixel and every scale v = select_weight[s] r_s (one
 *      product; r_s: residual plane s at the pixel).
 *   2. (s*, p*) = the pair with the largest |v|; ties go to the lowest scale,
 *      then to the lowest flat index: the lowest key s nx ny + flat, so any
 *      reduction order gives the same winner; a v that is NaN is never
 *      selected (the comparison is >).
 *   3. stop, before anything changes, in this order: no pixel allowed ->
 *      CIP_CLEAN_EMPTY; |v| <= threshold -> CIP_CLEAN_THRESHOLD; k == niter ->
 *      CIP_CLEAN_NITER. result.peak is the signed v, result.peak_index the
 *      flat index, result.peak_scale s* (0, -1 and -1 if EMPTY).
 *   4. c = flux_scale[s*] r_{s*}[p*]; f = gain c; model_{s*}[p*] =
 *      model_{s*}[p*] + f; comp_index[k] = p*, comp_scale[k] = s*,
 *      comp_flux[k] = f.
 *   5. for every scale s and every image pixel (i, j) whose PSF index
 *      (i - i* + cx, j - j* + cy) lies inside the PSF:
 *      r_s[i, j] = r_s[i, j] - (f psf_{tri(min(s, s*), max(s, s*))}[...]).
 * Pixels outside the mask are still subtracted. niter == 0 changes nothing
 * and reports the peak. comp_index, comp_scale and comp_flux hold niter
 * entries each (all three or none). `batch` as for cip_hogbom_clean: the
 * result does not depend on it. Synchronous on hip_stream. No atomics:
 * identical calls give identical bits. With nscales == 1 and both host arrays
 * {1.0} every output equals cip_hogbom_clean's bit for bit (1.0 r is exact).
 *
 * CIP_EINVAL, all checked before the first launch: whatever cip_hogbom_clean
 * rejects (NULL residual_io / psf, a dimension < 1, a centre outside the PSF,
 * gain not finite or <= 0, threshold NaN or negative, niter < 0, batch < 0),
 * some but not all of comp_index / comp_scale / comp_flux, nscales outside
 * 1 .. CIP_MS_MAX_SCALES, select_weight or flux_scale NULL or with an entry
 * that is not finite, S nx ny or the PSF stack overflowing int64.
 */
#ifndef CIP_MS_H
#define CIP_MS_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CIP_MS_MAX_SCALES 6
#define CIP_MS_MAX_RADIUS 128

/* HOST memory; stop_reason is a CIP_CLEAN_* code of cip.h */
typedef struct cip_ms_result {
  int64_t niter_done;
  int32_t stop_reason;
  int32_t peak_scale;
  double peak;
  int64_t peak_index;
} cip_ms_result;

int cip_ms_scale_radius(double width, double tol);

int cip_ms_scale_taps(double width, int64_t radius, double* taps_out);

int cip_ms_convolve(const double* in, int64_t nx, int64_t ny, const double* taps,
                    int64_t radius, void* hip_stream, double* out);

int cip_ms_clean(double* residual_io, int64_t nscales, int64_t nx, int64_t ny,
                 const double* psf, int64_t psf_nx, int64_t psf_ny,
                 int64_t psf_cx, int64_t psf_cy, const double* select_weight,
                 const double* flux_scale, const uint8_t* mask, double gain,
                 double threshold, int64_t niter, int64_t batch, void* hip_stream,
                 double* model_io, int64_t* comp_index, int64_t* comp_scale,
                 double* comp_flux, cip_ms_result* result_out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_MS_H */
