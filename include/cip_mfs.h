/*
 * cip_mfs.h - multi-term multi-frequency synthesis (MT-MFS, Rau & Cornwell
 * 2011, point-source scale only) in libcip_hip.so: the joint minor cycle over
 * T = nterms Taylor-term images. Third header of the C ABI; the conventions
 * are those of cip.h (extern "C", 0 or a negative CIP_E* code, the message
 * through cip_last_error(), device pointers on the current device). The
 * reference has no counterpart: it stops at the dirty image.
 *
 * Images. With x_c = (nu_c - nu_ref) / nu_ref, residual term t is the dirty
 * image of the visibilities times x_c^t and PSF k the point-spread function
 * of the weights times x_c^k (k = 0 .. 2T - 2), all divided by the same
 * weight sum. residual_io is (T, nx, ny) and psf (2T - 1, psf_nx, psf_ny),
 * plane after plane, each plane row-major as in cip.h, every PSF plane with
 * the same centre pixel (psf_cx, psf_cy), -1: psf_n / 2. hinv is the inverse
 * of the T x T matrix H[t][q] = psf[t + q][centre], row-major in HOST memory:
 * an input (the library inverts nothing, so no host arithmetic enters the
 * definition). mask (nx, ny) uint8 as for cip_hogbom_clean, one for all
 * terms. model_io (T, nx, ny), may be NULL.
 *
 * The operator, rounding included: every product, sum and difference below
 * is one rounded fp64 operation, never an FMA. For k = 0, 1, ...:
 *   1. for every allowed pixel s = hinv[0][0] r_0, then s = s + hinv[0][t] r_t
 *      for t = 1 .. T - 1 in that order (r_t: residual term t at the pixel):
 *      the principal solution at the reference frequency.
 *   2. (i*, j*) = the allowed pixel with the largest |s|; ties go to the
 *      lowest flat index i ny + j; a pixel whose s is NaN is never selected
 *      (the comparison is >).
 *   3. stop, before anything changes, in this order: no pixel allowed ->
 *      CIP_CLEAN_EMPTY; |s| <= threshold -> CIP_CLEAN_THRESHOLD; k == niter
 *      -> CIP_CLEAN_NITER. result.peak is the signed s, result.peak_index the
 *      flat index (0 and -1 if EMPTY).
 *   4. at the peak c_q = hinv[q][0] r_0, then c_q = c_q + hinv[q][t] r_t for
 *      t = 1 .. T - 1 in order, q = 0 .. T - 1 (c_0 is s); f_q = gain c_q;
 *      model_q[i*, j*] = model_q[i*, j*] + f_q; comp_index[k] = i* ny + j*;
 *      comp_flux[k T + q] = f_q.
 *   5. for every term t and every image pixel (i, j) whose PSF index
 *      (i - i* + cx, j - j* + cy) lies inside the PSF, for q = 0 .. T - 1 in
 *      order: r_t[i, j] = r_t[i, j] - (f_q psf_{t + q}[...]).
 * Pixels outside the mask are still subtracted. niter == 0 changes nothing
 * and reports the peak. comp_index holds niter and comp_flux niter T entries
 * (both or neither). `batch` as for cip_hogbom_clean: the result does not
 * depend on it. Synchronous on hip_stream. No floating-point atomics:
 * identical calls give identical bits. With nterms == 1 and hinv = {1.0}
 * every output equals cip_hogbom_clean's bit for bit (1.0 r is exact).
 *
 * CIP_EINVAL, all checked before the first launch: whatever
 * cip_hogbom_clean rejects (NULL residual_io / psf, a dimension < 1, a centre
 * outside the PSF, gain not finite or <= 0, threshold NaN or negative,
 * niter < 0, batch < 0, exactly one of comp_index / comp_flux), nterms
 * outside 1 .. CIP_MFS_MAX_TERMS, hinv NULL or with an entry that is not
 * finite.
 */
#ifndef CIP_MFS_H
#define CIP_MFS_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CIP_MFS_MAX_TERMS 3

int cip_mfs_clean(double* residual_io, int64_t nterms, int64_t nx, int64_t ny,
                  const double* psf, int64_t psf_nx, int64_t psf_ny,
                  int64_t psf_cx, int64_t psf_cy, const double* hinv,
                  const uint8_t* mask, double gain, double threshold,
                  int64_t niter, int64_t batch, void* hip_stream,
                  double* model_io, int64_t* comp_index, double* comp_flux,
                  cip_clean_result* result_out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_MFS_H */
