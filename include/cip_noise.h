/*
 * cip_noise.h - the noise of an image and the island mask built on it, in
 * libcip_hip.so: an exact order statistic (cip_image_select), the robust noise
 * estimate from the median and the median absolute deviation
 * (cip_image_noise) and the hysteresis mask (cip_auto_mask). Seventh header of
 * the C ABI; the conventions are those of cip.h (extern "C", 0 or a negative
 * CIP_E* code, the message through cip_last_error(), device pointers on the
 * current device unless marked HOST). The reference has no counterpart: it
 * stops at the dirty image.
 *
 * Images are (nx, ny) row-major float64 as in cip.h; `region`, `base` and
 * `mask_out` are (nx, ny) uint8. All three calls are synchronous on
 * hip_stream: they return host scalars, as cip_hogbom_clean does. Scratch is
 * the library workspace; none of it is image-sized for the first two calls.
 *
 * The sample set S: the pixels with region[p] != 0 (region == NULL: all
 * pixels) whose value is finite. NaN and +-inf are not samples. count = |S|.
 * The order on finite fp64 is by value; -0.0 and +0.0 are equal as values and
 * which of the two is returned is unspecified.
 *
 * cip_image_select: *value_out is the sample of 0-based `rank` in the sorted
 * samples, an image value bit for bit (numpy: sort(v)[rank]). The result is
 * exact for every input: nothing is sampled or approximated. rank < 0 is
 * CIP_EINVAL; rank >= count is CIP_ERANGE with *count_out still set (and
 * *value_out NaN).
 *
 * cip_image_noise:
 *   median = the sample of rank (count - 1) / 2, the lower median: a
 *            selection, never the mean of two samples.
 *   mad    = the value of the same rank among d_p = |x_p - median| over S, one
 *            rounded fp64 subtraction each. A d that overflows to +inf sorts
 *            last and is still counted. d is formed on the fly.
 *   sigma  = CIP_MAD_TO_SIGMA mad, one rounded product.
 * count == 0 returns CIP_OK with count = 0 and the three doubles NaN.
 *
 * cip_auto_mask. a(p) = |image[p]|, or image[p] with CIP_MASK_POSITIVE.
 *   LO  = { p : region[p] != 0 (NULL: all) and a(p) >= grow }
 *   HI  = { p in LO : a(p) >= seed }
 *   ISL = every pixel of LO joined to a pixel of HI by a path inside LO;
 *         steps go to the 8 neighbours, or to the 4 edge neighbours with
 *         CIP_MASK_CONN4.
 *   mask_out[p] = 1 if p is in ISL or base[p] != 0 (base == NULL: no base),
 *                 else 0.
 * The comparisons are inclusive. A NaN pixel is in neither set, so it breaks
 * connectivity. mask_out may be the same buffer as base: masks only grow.
 * n_seed = |HI|, n_island = |ISL|, n_out = the number of ones written,
 * rounds = the propagation launches that ran (informative: it depends on the
 * library's tile, the other three do not). The set is unique, so the result
 * does not depend on the order of the work.
 *
 * CIP_EINVAL, all checked before any device work, the message naming the
 * function: NULL image / count_out / value_out / out / mask_out, a dimension
 * < 1, nx ny overflowing int64, rank < 0; for cip_auto_mask also seed or grow
 * not finite, not seed >= grow > 0, or flag bits other than the two below.
 */
#ifndef CIP_NOISE_H
#define CIP_NOISE_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sigma of a Gaussian over its median absolute deviation: 1 / Phi^-1(3/4) */
#define CIP_MAD_TO_SIGMA 1.482602218505602

#define CIP_MASK_POSITIVE 1 /* a(p) = image[p] instead of |image[p]| */
#define CIP_MASK_CONN4 2    /* 4-connectivity instead of 8 */

/* HOST memory */
typedef struct cip_noise_result {
  int64_t count;
  double median;
  double mad;
  double sigma;
} cip_noise_result;

/* HOST memory */
typedef struct cip_mask_result {
  int64_t n_seed;
  int64_t n_island;
  int64_t n_out;
  int64_t rounds;
} cip_mask_result;

int cip_image_select(const double* image, int64_t nx, int64_t ny, const uint8_t* region,
                     int64_t rank, void* hip_stream, int64_t* count_out, double* value_out);

int cip_image_noise(const double* image, int64_t nx, int64_t ny, const uint8_t* region,
                    void* hip_stream, cip_noise_result* out);

int cip_auto_mask(const double* image, int64_t nx, int64_t ny, double seed, double grow,
                  const uint8_t* region, const uint8_t* base, int flags, void* hip_stream,
                  uint8_t* mask_out, cip_mask_result* out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_NOISE_H */
