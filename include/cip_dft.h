/*
 * cip_dft.h - sky-model predict in libcip_hip.so: the visibilities of a list
 * of point and Gaussian components by the direct Fourier sum, exact in the
 * components' positions (no grid, no pixel). Fifth header of the C ABI; the
 * conventions are those of cip.h (extern "C", 0 or a negative CIP_E* code, the
 * message through cip_last_error(), device pointers on the current device,
 * arguments validated before the first launch). The reference has no
 * counterpart, so this comment is the specification.
 *
 * Arrays (all device memory). uvw (nrow, 3) fp64 metres; freq (nchan) fp64 Hz;
 * lm (ncomp, 2) fp64 direction cosines (l, m), l with u and m with v as
 * everywhere in cip.h; flux (ncomp, nterms) fp64 Taylor coefficients, nterms
 * in 1 .. CIP_MFS_MAX_TERMS; shape (ncomp, 3) fp64 or NULL: FWHM of the major
 * axis, FWHM of the minor axis (radians, in the (l, m) plane) and the position
 * angle pa (radians); wgt (nrow, nchan) float32 / float64 (CIP_F32 / CIP_F64)
 * or NULL with CIP_NONE; vis_io (nrow, nchan) complex64 / complex128 (CIP_C64 /
 * CIP_C128). No array may overlap vis_io.
 *
 * Definition. With c0 = 299792458 m/s, fx_c = freq_c / c0 and x_c = (freq_c -
 * ref_freq) / ref_freq (the basis of the multi-term MFS, cip_mfs.h; x_c is not
 * formed and ref_freq not read when nterms == 1):
 *
 *   model[r, c] = sum_k S_k(c) G_k(r, c) exp(-2 pi i fx_c p_k(r))
 *   p_k(r) = u_r l_k + v_r m_k - w_r nm1_k                    (metres)
 *   nm1_k  = -(l^2 + m^2) / (sqrt(1 - l^2 - m^2) + 1)  with CIP_DFT_WTERM,
 *            0 without it (the 2-D image convention of cip_dirty2ms)
 *   S_k(c) = sum_t flux[k, t] x_c^t
 *   G_k(r, c) = exp(-fx_c^2 (ea_k a^2 + eb_k b^2)),
 *   ea_k = (pi^2 / (4 ln 2)) fwhm_major^2, eb_k = (pi^2 / (4 ln 2)) fwhm_minor^2,
 *   a = u_r sin(pa) + v_r cos(pa),  b = u_r cos(pa) - v_r sin(pa).
 *
 * This is the sign of the degridder (cip_dirty2ms), the conjugate of the
 * invert's. The position angle is measured from the +m axis towards the +l
 * axis (north through east on a sky image with l to the east): the major axis
 * lies along (l, m) = (sin pa, cos pa), and a and b are the baseline (u, v) in
 * metres projected on the major and the minor axis. G is the Fourier
 * transform of a Gaussian of unit integral: flux is the component's total
 * flux. shape NULL, or a component with both FWHM equal to 0, is a point
 * source (G = 1 exactly). No 1/n is applied: a component's flux is what the
 * visibilities see, so a pixel of value I of a cip_dirty2ms image under
 * w-stacking corresponds to a component of flux I / n, n = sqrt(1 - l^2 - m^2),
 * and to one of flux I without it.
 *
 * Components that contribute nothing: one with a field (l, m, a flux
 * coefficient, a shape entry) that is not finite, with either FWHM negative,
 * or, under CIP_DFT_WTERM, with 1 - l^2 - m^2 <= 0.
 *
 * The sum runs over k = 0 .. ncomp - 1 in index order, one thread per output
 * sample: no floating-point atomic anywhere. A small kernel first turns (l, m,
 * shape) into the per-component coefficients (l, m, nm1, sin pa, cos pa, ea,
 * eb) and a copy of flux (zero for the components left out) in the grow-only
 * workspace.
 *
 * Flags (a namespace of its own; the CIP_* flags of cip.h mean nothing here).
 *   default           vis_io  = wgt model   (vis_io = model without wgt)
 *   CIP_DFT_ADD       vis_io += wgt model
 *   CIP_DFT_SUBTRACT  vis_io -= wgt model   (excludes CIP_DFT_ADD)
 *   CIP_DFT_WTERM     the w term, see nm1 above
 *   CIP_DFT_FAST      the single-precision class, see below
 * A sample of weight zero is set to exactly 0 by default, and keeps its bits
 * under ADD and SUBTRACT whatever they are (NaN data included): the rule of
 * cip_dirty2ms. The product and the sum with vis_io are formed in fp64 and
 * rounded once to the dtype of vis_io.
 *
 * Precision classes.
 *   fp64 (default): p, the phase fx p in cycles, its reduction, sine and
 *   cosine, G, S and the accumulation are fp64. Against the same sum in exact
 *   arithmetic the error of a sample is a few rounding errors of the phase:
 *   about 2 pi PHI 2^-52 sum_k |S_k| with PHI the largest |fx p| in cycles.
 *   fast (CIP_DFT_FAST): p and the phase fx p are still formed in fp64 and the
 *   phase is reduced to its fraction fx p - rint(fx p) in [-1/2, 1/2] in fp64
 *   (phases reach 1e5 cycles on long baselines, which fp32 cannot hold); the
 *   fraction is then rounded to fp32 and the sine and cosine (the hardware's,
 *   which take revolutions), G, S and their products are fp32. The sums over k
 *   are kept in fp64, so the error does not grow with the rounding of a long
 *   fp32 sum. Measured: |error| <= 1.1e-7 sum_k |S_k|.
 *
 * Determinism. Identical calls give identical bits, and so does any split of
 * the rows into several calls: a sample's value depends on its own row, its
 * channel and the component list alone. A split of the COMPONENTS into two
 * CIP_DFT_ADD calls is not promised to equal one call (the intermediate is
 * rounded to the dtype of vis_io). The call has no readback and does not wait
 * for the device: it is stream-ordered on hip_stream, like cip_cal_apply.
 *
 * Empty inputs. nrow == 0 or nchan == 0: nothing is done. ncomp == 0 writes
 * zeros by default and is a no-op under CIP_DFT_ADD / CIP_DFT_SUBTRACT.
 *
 * CIP_EINVAL: nrow, nchan or ncomp negative (or nchan, ncomp > 2^30); nterms
 * outside 1 .. CIP_MFS_MAX_TERMS; ref_freq not finite or <= 0 when nterms > 1;
 * CIP_DFT_ADD together with CIP_DFT_SUBTRACT, or an unknown flag bit;
 * vis_dtype not CIP_C64 / CIP_C128; wgt_dtype not CIP_NONE / CIP_F32 /
 * CIP_F64; wgt NULL with a dtype given, or wgt set with CIP_NONE; lm or flux
 * NULL when ncomp > 0; uvw, freq or vis_io NULL when there is work to do
 * (nrow > 0 and nchan > 0, and ncomp > 0 or the default mode).
 */
#ifndef CIP_DFT_H
#define CIP_DFT_H

#include "cip.h"
#include "cip_mfs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CIP_DFT_ADD 1
#define CIP_DFT_SUBTRACT 2
#define CIP_DFT_WTERM 4
#define CIP_DFT_FAST 8

int cip_dft_predict(const double* uvw, int64_t nrow, const double* freq,
                    int64_t nchan, const double* lm, const double* flux,
                    const double* shape, int64_t ncomp, int64_t nterms,
                    double ref_freq, int flags, const void* wgt, int wgt_dtype,
                    void* hip_stream, void* vis_io, int vis_dtype);

#ifdef __cplusplus
}
#endif
#endif /* CIP_DFT_H */
