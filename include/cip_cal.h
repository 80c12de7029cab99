/*
 * cip_cal.h - antenna gain self-calibration (StEFCal, Salvini & Wijnholds
 * 2014) in libcip_hip.so: the calibration half of a continuum imaging /
 * self-calibration loop. Fourth header of the C ABI; the conventions are those
 * of cip.h (extern "C", 0 or a negative CIP_E* code, the message through
 * cip_last_error(), device pointers on the current device, arguments
 * validated before the first launch). The reference has no counterpart: it
 * stops at the dirty image, so this comment is the specification.
 *
 * Gain model. Gains are scalar (one polarisation product, Stokes I as the
 * gridder takes it), per antenna and per solution interval, shared by all
 * channels of a call: V_pq ~ g_p M_pq conj(g_q) for the row of antennas
 * p = ant1[r], q = ant2[r] in interval s = interval[r].
 *
 * Arrays. vis and model (nrow, nchan) complex64 / complex128, each with its
 * own dtype code (CIP_C64 / CIP_C128); wgt (nrow, nchan) float32 / float64
 * (CIP_F32 / CIP_F64); ant1, ant2, interval (nrow) int32; gains (n_int, n_ant)
 * complex128 stored as (re, im) double pairs; ant_ok (n_int, n_ant) uint8; corr
 * (n_int, n_ant, n_ant, 3) int64, of which only the cells (s, p, q) with p < q
 * are ever written. All of these are device arrays; the structs are HOST
 * memory.
 *
 * Rounding. Every product, sum, difference, quotient and square root below is
 * one rounded fp64 operation, never an FMA; inputs are converted to fp64 first
 * (exact). fp64 division and square root are correctly rounded on the device
 * (the library is built without fast-math), so each function is bit-identical
 * to its statement in numpy. A NaN result is a NaN in the same place; its sign
 * and payload are not part of the definition.
 *
 * cip_cal_scale_init (host only). B: the least integer with nsamp_max <= 2^B;
 * x = ((2 wmax) amax) amax in fp64; E: the least integer with x < 2^E;
 * shift = 61 - B - E, quantum = 2^-shift. A sample's three terms are at most
 * x in magnitude, so no sum of nsamp_max samples reaches 2^62. CIP_EINVAL:
 * amax or wmax not finite or <= 0 (or x not finite, or a shift beyond
 * +-1000), nsamp_max < 1, n_ant outside 2 .. CIP_CAL_MAX_ANT, n_int < 1,
 * scale_out NULL. nsamp_max bounds the samples of the whole data set (all
 * calls, all ranks): every rank passes the same values.
 *
 * cip_cal_correlate accumulates into corr_io. A row with ant1 == ant2, an
 * antenna outside 0 .. n_ant - 1 or an interval outside 0 .. n_int - 1 adds
 * nothing: all nchan of its samples count in n_outside. Of the other rows,
 * per sample (v = vis, m = model, w = wgt), in this order:
 *   w == 0                                      -> n_zero (v, m may be NaN)
 *   w < 0, w NaN, or w, vr, vi, mr, mi not finite -> n_bad
 *   w > wmax or one of |vr|, |vi|, |mr|, |mi| > amax -> n_outside
 *   else                                          -> n_added, and
 *     cr = vr mr + vi mi,  ci = vi mr - vr mi,  m2 = mr mr + mi mi,
 *     t = (w cr, w ci, w m2),  q(t) = llrint(ldexp(t, shift)) (ties to even);
 *     a row with ant1 > ant2 is folded: the antennas swap and q(w ci) is
 *     negated; corr[s, p, q, :] += (q(w cr), q(w ci), q(w m2)).
 * The sums are 64-bit integer adds and nothing else (no floating-point
 * atomic anywhere), so corr is bit-identical for any order of the rows, any
 * split of them into calls and any int64 SUM all-reduce across ranks.
 * counts_out (may be NULL) receives this call's four counts; a bad or outside
 * sample is no error. Synchronous on hip_stream (the counts come back).
 *
 * cip_cal_solve: StEFCal, per interval s (intervals are independent), n =
 * n_ant. D = (double)corr * quantum; A_pq = D0 + i D1 for p < q, its conjugate
 * for p > q and 0 for p == q; B_pq = D2 in both orders, 0 for p == q. With g
 * the gains on entry of iteration k = 1, 2, ..., for each antenna p:
 *   num = sum_q A_pq g_q: from (0, 0), q = 0 .. n - 1 in order,
 *         term = (Ar gr - Ai gi, Ar gi + Ai gr) (four rounded products, one
 *         rounded subtract, one rounded add), num = num + term (rounded adds);
 *   den = sum_q B_pq (g_qr g_qr + g_qi g_qi): from 0, in the same order;
 *   p is dead in s when den == 0 at k = 1: ant_ok[s, p] = 0 (else 1), its gain
 *   keeps the input bits to the end, and g'_p = g_p in every iteration;
 *   otherwise g' = (num_r / den, num_i / den);
 *   with CIP_CAL_PHASE_ONLY, a = sqrt(g'_r g'_r + g'_i g'_i), g' = (g'_r / a, g'_i / a);
 *   for even k, g' = (0.5 (g'_r + g_r), 0.5 (g'_i + g_i)).
 * Then d2 = sum_p (dr dr + di di) with (dr, di) = g'_p - g_p, and n2 = sum_p
 * (g'_pr g'_pr + g'_pi g'_pi), both from 0 over p = 0 .. n - 1 in order (dead
 * antennas included); g = g'; iters_out[s] = k; the interval is converged, and
 * stops, when d2 <= (tol tol) n2. At most niter iterations.
 * After the last iteration, with r = refant >= 0 and r alive in s:
 * a = sqrt(g_rr g_rr + g_ri g_ri), u = (g_rr / a, -(g_ri / a)), and every
 * live gain becomes (gr ur - gi ui, gr ui + gi ur). refant < 0: no rotation. A
 * dead reference antenna: no rotation, and info.ref_missing counts the
 * interval. niter == 0 fills ant_ok and info.n_dead and nothing else
 * (iters_out is 0). info_out (may be NULL): n_converged intervals, n_dead
 * (interval, antenna) pairs, max_iter_done = max_s iters, ref_missing, and
 * max_change = the largest sqrt(d2 / n2) of the intervals' last iterations
 * (host arithmetic; intervals with n2 == 0 or a NaN are left out; 0 without
 * an iteration). iters_out: device int64 (n_int), may be NULL. Synchronous.
 * CIP_EINVAL: niter < 0, tol not finite or negative, refant >= n_ant, a NULL
 * corr / gains_io / ant_ok_out, a scale cip_cal_scale_init did not fill.
 *
 * cip_cal_apply: per row h = g_p conj(g_q) = (gpr gqr + gpi gqi, gpi gqr -
 * gpr gqi) with p = ant1, q = ant2 as they stand (no fold), n2 = hr hr + hi hi.
 *   CIP_CAL_CORRECT: out = ((vr hr + vi hi) / n2, (vi hr - vr hi) / n2),
 *                    wgt_out = w n2
 *   CIP_CAL_CORRUPT: out = (hr vr - hi vi, hr vi + hi vr), wgt_out = w
 * in fp64, rounded once to the output dtype. Outputs have the input dtypes;
 * vis_out may be vis and wgt_out may be wgt. wgt and wgt_out are both NULL
 * (wgt_dtype CIP_NONE) or both set. A row with an antenna or interval index
 * out of range, or with ant_ok == 0 for either antenna, passes vis through
 * unchanged and gets weight 0. Stream-ordered: it does not wait for the
 * device.
 *
 * cip_gaincal, the one-shot call: (1) the largest |component| and the
 * largest w of the samples that will be added (an integer max of the bit
 * patterns), each replaced by 1.0 when nothing will be added;
 * (2) cip_cal_scale_init with nsamp_max = max(nrow nchan, 1); (3) a zeroed
 * corr in the workspace; (4) cip_cal_correlate; (5) cip_cal_solve from
 * gains_io. scale_out, counts_out and info_out may be NULL. Every output
 * equals that written-out sequence bit for bit.
 */
#ifndef CIP_CAL_H
#define CIP_CAL_H

#include "cip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CIP_CAL_MAX_ANT 1024
#define CIP_CAL_CORRECT 0
#define CIP_CAL_CORRUPT 1
#define CIP_CAL_PHASE_ONLY 1

typedef struct cip_cal_scale {
  int64_t n_ant;
  int64_t n_int;
  double amax;
  double wmax;
  double quantum;
  int32_t shift;
  int32_t reserved;
} cip_cal_scale;

typedef struct cip_cal_counts {
  int64_t n_added;
  int64_t n_zero;
  int64_t n_outside;
  int64_t n_bad;
} cip_cal_counts;

typedef struct cip_cal_solve_info {
  int64_t n_converged;
  int64_t n_dead;
  int64_t max_iter_done;
  int64_t ref_missing;
  double max_change;
} cip_cal_solve_info;

int cip_cal_scale_init(int64_t n_ant, int64_t n_int, double amax, double wmax,
                       int64_t nsamp_max, cip_cal_scale* scale_out);

int cip_cal_correlate(const void* vis, int vis_dtype, const void* model,
                      int model_dtype, const void* wgt, int wgt_dtype,
                      int64_t nrow, int64_t nchan, const int32_t* ant1,
                      const int32_t* ant2, const int32_t* interval,
                      const cip_cal_scale* scale, void* hip_stream,
                      int64_t* corr_io, cip_cal_counts* counts_out);

int cip_cal_solve(const int64_t* corr, const cip_cal_scale* scale,
                  int64_t niter, double tol, int64_t refant, int flags,
                  void* hip_stream, double* gains_io, uint8_t* ant_ok_out,
                  int64_t* iters_out, cip_cal_solve_info* info_out);

int cip_cal_apply(const void* vis, int vis_dtype, const void* wgt,
                  int wgt_dtype, int64_t nrow, int64_t nchan,
                  const int32_t* ant1, const int32_t* ant2,
                  const int32_t* interval, const double* gains,
                  const uint8_t* ant_ok, int64_t n_int, int64_t n_ant,
                  int mode, void* hip_stream, void* vis_out, void* wgt_out);

int cip_gaincal(const void* vis, int vis_dtype, const void* model,
                int model_dtype, const void* wgt, int wgt_dtype, int64_t nrow,
                int64_t nchan, const int32_t* ant1, const int32_t* ant2,
                const int32_t* interval, int64_t n_ant, int64_t n_int,
                int64_t niter, double tol, int64_t refant, int flags,
                void* hip_stream, double* gains_io, uint8_t* ant_ok_out,
                int64_t* iters_out, cip_cal_scale* scale_out,
                cip_cal_counts* counts_out, cip_cal_solve_info* info_out);

#ifdef __cplusplus
}
#endif
#endif /* CIP_CAL_H */
