// cip_dft.hip - sky-model predict on the device (cip_dft_predict).
// The operator is defined in include/cip_dft.h.
//
// The work is nrow nchan ncomp phase evaluations against a few bytes per
// visibility: compute-bound, the opposite of the gridder. A group of L lanes
// (a power of two chosen from nchan) owns a row and lane l of it the channels
// c0 + l + L j, j < kDftRun, of each pass over the row's channels: consecutive
// lanes hold consecutive channels, so a row's store is coalesced, and the
// three fp64 multiply-adds of a (row, component) path are shared by the
// lane's kDftRun channels. The component index is the same in every lane of
// the launch, so the per-component coefficients are read through const
// __restrict__ pointers at a uniform index: scalar loads into scalar
// registers, no LDS tile and no barrier. One thread writes each sample and sums
// the components in index order.
#include <algorithm>
#include <cmath>

#include "cip_dft.h"
#include "cip_host.h"

namespace cip {

namespace {

constexpr int kDftThreads = 256;
constexpr int kDftRun = 4;          // channels a lane carries per pass
constexpr int kDftMaxLanes = 64;    // lanes per row at most: one wave
constexpr int kDftMaxBlocks = 2048;  // workgroups of the grid-stride launch (8 per CU)
constexpr int kDftCoef = 8;         // doubles per component: l, m, nm1, sin pa, cos pa, ea, eb, 0
constexpr int kDftModeBits = CIP_DFT_ADD | CIP_DFT_SUBTRACT;
constexpr int kDftFlagBits = kDftModeBits | CIP_DFT_WTERM | CIP_DFT_FAST;
constexpr double kDftEnvelope = 3.559707331246876;  // pi^2 / (4 ln 2)
enum { DFT_F64 = 0, DFT_FAST = 1 };

struct DftArgs {
  int64_t nrow, nblk;  // rows; row blocks of kDftThreads / lanes rows
  int nchan, ncomp;
  int lane_shift;  // lanes per row = 1 << lane_shift
  int mode;        // 0, CIP_DFT_ADD or CIP_DFT_SUBTRACT
  int vis_dtype, wgt_dtype;
  double ref_freq;
};

// (l, m, shape) -> the coefficients of cip_dft.h and a copy of flux; a component that contributes nothing gets
// zeros throughout. One thread per component; each operation rounded on its own, as the header states them.
__global__ __launch_bounds__(kDftThreads) void dft_prep_kernel(const double* __restrict__ lm,
                                                               const double* __restrict__ flux,
                                                               const double* __restrict__ shape, int ncomp,
                                                               int nterms, int wterm, double* __restrict__ coef,
                                                               double* __restrict__ fz) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * kDftThreads + threadIdx.x;
  if (k >= ncomp) return;
  const double l = lm[2 * (int64_t)k], m = lm[2 * (int64_t)k + 1];
  bool ok = isfinite(l) && isfinite(m);
  for (int t = 0; t < nterms; ++t) ok = ok && isfinite(flux[(int64_t)k * nterms + t]);
  double nm1 = 0.0, sp = 0.0, cp = 1.0, ea = 0.0, eb = 0.0;
  if (wterm) {
    const double e = l * l + m * m;
    const double n2 = 1.0 - e;
    if (n2 > 0.0)
      nm1 = -e / (sqrt(n2) + 1.0);
    else
      ok = false;
  }
  if (shape) {
    const double maj = shape[3 * (int64_t)k], mnr = shape[3 * (int64_t)k + 1], pa = shape[3 * (int64_t)k + 2];
    ok = ok && isfinite(maj) && isfinite(mnr) && isfinite(pa) && maj >= 0.0 && mnr >= 0.0;
    if (ok && (maj != 0.0 || mnr != 0.0)) {
      sp = sin(pa);
      cp = cos(pa);
      ea = kDftEnvelope * (maj * maj);
      eb = kDftEnvelope * (mnr * mnr);
    }
  }
  double* ck = coef + (int64_t)k * kDftCoef;
  ck[0] = ok ? l : 0.0;
  ck[1] = ok ? m : 0.0;
  ck[2] = ok ? nm1 : 0.0;
  ck[3] = ok ? sp : 0.0;
  ck[4] = ok ? cp : 1.0;
  ck[5] = ok ? ea : 0.0;
  ck[6] = ok ? eb : 0.0;
  ck[7] = 0.0;
  for (int t = 0; t < nterms; ++t) fz[(int64_t)k * nterms + t] = ok ? flux[(int64_t)k * nterms + t] : 0.0;
}

__device__ __forceinline__ double dft_weight(const void* wgt, int dtype, int64_t i) {
  if (dtype == CIP_F32) return (double)((const float*)wgt)[i];
  if (dtype == CIP_F64) return ((const double*)wgt)[i];
  return 1.0;
}

// T terms, SHAPES: Gaussian envelopes (shape given), CLS: the precision class.
template <int T, bool SHAPES, int CLS>
__global__ __launch_bounds__(kDftThreads) void dft_predict_kernel(const double* __restrict__ uvw,
                                                                  const double* __restrict__ freq,
                                                                  const double* __restrict__ coef,
                                                                  const double* __restrict__ fz,
                                                                  const void* __restrict__ wgt, DftArgs a,
                                                                  void* __restrict__ vis) {
  const int L = 1 << a.lane_shift;
  const int l = threadIdx.x & (L - 1);
  const int rows = kDftThreads >> a.lane_shift;
  for (int64_t rb = blockIdx.x; rb < a.nblk; rb += gridDim.x) {
    const int64_t r = rb * rows + (threadIdx.x >> a.lane_shift);
    if (r >= a.nrow) continue;
    const double u = uvw[3 * r], v = uvw[3 * r + 1], w = uvw[3 * r + 2];
    for (int c0 = l; c0 < a.nchan; c0 += L * kDftRun) {  // c0: the lane's first channel of this pass
      double fx[kDftRun];                                // freq / c0 (correctly rounded), 0 past the row's end
      double x[kDftRun], fx2[kDftRun];
      float xf[kDftRun], fx2f[kDftRun];
#pragma unroll
      for (int j = 0; j < kDftRun; ++j) {
        const int c = c0 + L * j;
        const double f = c < a.nchan ? freq[c] : 0.0;
        fx[j] = f / CIP_SPEED_OF_LIGHT;
        x[j] = T > 1 ? (f - a.ref_freq) / a.ref_freq : 0.0;
        fx2[j] = fx[j] * fx[j];
        xf[j] = (float)x[j];
        fx2f[j] = (float)fx2[j];
      }
      double re[kDftRun], im[kDftRun];
#pragma unroll
      for (int j = 0; j < kDftRun; ++j) re[j] = im[j] = 0.0;
      for (int k = 0; k < a.ncomp; ++k) {  // k is uniform over the launch: scalar loads
        const double* ck = coef + (int64_t)k * kDftCoef;
        const double* fk = fz + (int64_t)k * T;
        const double p = u * ck[0] + v * ck[1] - w * ck[2];
        double q = 0.0;
        if constexpr (SHAPES) {
          const double pa = u * ck[3] + v * ck[4], pb = u * ck[4] - v * ck[3];
          q = ck[5] * (pa * pa) + ck[6] * (pb * pb);
        }
        if constexpr (CLS == DFT_F64) {
#pragma unroll
          for (int j = 0; j < kDftRun; ++j) {
            const double ph = p * fx[j];
            const double fr = ph - rint(ph);  // exact: the phase's fraction in [-1/2, 1/2]
            double sn, cs;
            sincospi(2.0 * fr, &sn, &cs);
            double s = fk[T - 1];
#pragma unroll
            for (int t = T - 2; t >= 0; --t) s = s * x[j] + fk[t];
            if constexpr (SHAPES) s *= exp(-(fx2[j] * q));
            re[j] += s * cs;
            im[j] -= s * sn;
          }
        } else {
          float fkf[T];
#pragma unroll
          for (int t = 0; t < T; ++t) fkf[t] = (float)fk[t];
          const float qf = (float)q;
#pragma unroll
          for (int j = 0; j < kDftRun; ++j) {
            const double ph = p * fx[j];
            const float fr = (float)(ph - rint(ph));  // reduced in fp64, then rounded
            // the hardware sine and cosine take revolutions (v_sin_f32, v_cos_f32): DESIGN.md 17
            const float sn = __builtin_amdgcn_sinf(fr), cs = __builtin_amdgcn_cosf(fr);
            float s = fkf[T - 1];
#pragma unroll
            for (int t = T - 2; t >= 0; --t) s = s * xf[j] + fkf[t];
            if constexpr (SHAPES) s *= __expf(-(fx2f[j] * qf));
            re[j] += (double)(s * cs);
            im[j] -= (double)(s * sn);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kDftRun; ++j) {
        const int c = c0 + L * j;
        if (c >= a.nchan) continue;
        const int64_t i = r * a.nchan + c;
        const double wv = dft_weight(wgt, a.wgt_dtype, i);
        double mr = wv * re[j], mi = wv * im[j];
        if (wv == 0.0) {
          if (a.mode != 0) continue;  // ADD / SUBTRACT: the sample keeps its bits
          mr = mi = 0.0;              // exactly 0, whatever the model holds
        }
        if (a.vis_dtype == CIP_C64) {
          float2* o = (float2*)vis + i;
          if (a.mode != 0) {
            const float2 old = *o;
            mr = a.mode == CIP_DFT_ADD ? (double)old.x + mr : (double)old.x - mr;
            mi = a.mode == CIP_DFT_ADD ? (double)old.y + mi : (double)old.y - mi;
          }
          *o = make_float2((float)mr, (float)mi);
        } else {
          double2* o = (double2*)vis + i;
          if (a.mode != 0) {
            const double2 old = *o;
            mr = a.mode == CIP_DFT_ADD ? old.x + mr : old.x - mr;
            mi = a.mode == CIP_DFT_ADD ? old.y + mi : old.y - mi;
          }
          *o = make_double2(mr, mi);
        }
      }
    }
  }
}

// lanes per row as a shift: the least power of two with kDftRun * L >= nchan, one wave at most
int dft_lane_shift(int64_t nchan) {
  int shift = 0;
  while ((1 << shift) < kDftMaxLanes && (int64_t)(1 << shift) * kDftRun < nchan) ++shift;
  return shift;
}

hipError_t launch_predict(const double* uvw, const double* freq, const double* coef, const double* fz,
                          const void* wgt, const DftArgs& a, int nterms, bool shapes, bool fast, void* vis,
                          hipStream_t s) {
  return dispatch_int<1, 2, 3>(nterms, hipErrorInvalidValue, [&](auto terms) {
    return dispatch_bool(shapes, [&](auto sh) {
      return dispatch_bool(fast, [&](auto fa) {
        constexpr int kCls = decltype(fa)::value ? DFT_FAST : DFT_F64;
        dft_predict_kernel<decltype(terms)::value, decltype(sh)::value, kCls>
            <<<dim3((unsigned)std::min<int64_t>(a.nblk, kDftMaxBlocks)), dim3(kDftThreads), 0, s>>>(
                uvw, freq, coef, fz, wgt, a, vis);
        return hipGetLastError();
      });
    });
  });
}
static_assert(CIP_MFS_MAX_TERMS == 3, "launch_predict instantiates 1 .. CIP_MFS_MAX_TERMS terms");

int predict_impl(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const double* lm,
                 const double* flux, const double* shape, int64_t ncomp, int64_t nterms, double ref_freq, int flags,
                 const void* wgt, int wgt_dtype, void* hip_stream, void* vis, int vis_dtype) {
  const std::string w("cip_dft_predict");
  if (nrow < 0 || nchan < 0 || ncomp < 0) return set_error(CIP_EINVAL, w + ": nrow, nchan and ncomp must be >= 0");
  if (nchan > (1 << 30) || ncomp > (1 << 30))
    return set_error(CIP_EINVAL, w + ": nchan and ncomp must be <= 2^30");
  if (nterms < 1 || nterms > CIP_MFS_MAX_TERMS)
    return set_error(CIP_EINVAL, w + ": nterms must be in 1 .. CIP_MFS_MAX_TERMS (3)");
  if (nterms > 1 && (!std::isfinite(ref_freq) || !(ref_freq > 0.0)))
    return set_error(CIP_EINVAL, w + ": ref_freq must be finite and > 0 when nterms > 1");
  if (flags & ~kDftFlagBits) return set_error(CIP_EINVAL, w + ": unknown flags");
  const int mode = flags & kDftModeBits;
  if (mode == kDftModeBits) return set_error(CIP_EINVAL, w + ": CIP_DFT_ADD and CIP_DFT_SUBTRACT exclude each other");
  if (vis_dtype != CIP_C64 && vis_dtype != CIP_C128)
    return set_error(CIP_EINVAL, w + ": vis_dtype must be CIP_C64 or CIP_C128");
  if (wgt_dtype != CIP_NONE && wgt_dtype != CIP_F32 && wgt_dtype != CIP_F64)
    return set_error(CIP_EINVAL, w + ": wgt_dtype must be CIP_NONE, CIP_F32 or CIP_F64");
  const bool samples = nrow > 0 && nchan > 0;
  if (samples && (wgt == nullptr) != (wgt_dtype == CIP_NONE))
    return set_error(CIP_EINVAL, w + ": wgt is NULL with CIP_NONE, or set with CIP_F32 / CIP_F64");
  if (ncomp > 0 && (!lm || !flux)) return set_error(CIP_EINVAL, w + ": lm and flux must not be NULL");
  const bool work = samples && (ncomp > 0 || mode == 0);
  if (work && !vis) return set_error(CIP_EINVAL, w + ": vis_io must not be NULL");
  if (work && ncomp > 0 && (!uvw || !freq)) return set_error(CIP_EINVAL, w + ": uvw and freq must not be NULL");
  if (!work) return CIP_OK;
  CIP_BEGIN_CALL(hip_stream, false)
  if (ncomp == 0) {  // default mode: zeros
    const size_t bytes = (size_t)nrow * (size_t)nchan * (vis_dtype == CIP_C64 ? 8u : 16u);
    CIP_HIP_CHECK(hipMemsetAsync(vis, 0, bytes, s));
    return CIP_OK;
  }
  CIP_ALLOC(coef, double, "dft_coef", ncomp * kDftCoef)
  CIP_ALLOC(fz, double, "dft_flux", ncomp * nterms)
  dft_prep_kernel<<<dim3((unsigned)((ncomp + kDftThreads - 1) / kDftThreads)), dim3(kDftThreads), 0, s>>>(
      lm, flux, shape, (int)ncomp, (int)nterms, (flags & CIP_DFT_WTERM) ? 1 : 0, coef, fz);
  CIP_HIP_CHECK(hipGetLastError());
  DftArgs a;
  a.nrow = nrow;
  a.nchan = (int)nchan;
  a.ncomp = (int)ncomp;
  a.lane_shift = dft_lane_shift(nchan);
  const int64_t rows = kDftThreads >> a.lane_shift;
  a.nblk = (nrow + rows - 1) / rows;
  a.mode = mode;
  a.vis_dtype = vis_dtype;
  a.wgt_dtype = wgt_dtype;
  a.ref_freq = nterms > 1 ? ref_freq : 1.0;
  CIP_HIP_CHECK(launch_predict(uvw, freq, coef, fz, wgt, a, (int)nterms, shape != nullptr,
                               (flags & CIP_DFT_FAST) != 0, vis, s));
  return CIP_OK;
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_dft_predict(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const double* lm,
                    const double* flux, const double* shape, int64_t ncomp, int64_t nterms, double ref_freq,
                    int flags, const void* wgt, int wgt_dtype, void* hip_stream, void* vis_io, int vis_dtype) {
  clear_error();
  return predict_impl(uvw, nrow, freq, nchan, lm, flux, shape, ncomp, nterms, ref_freq, flags, wgt, wgt_dtype,
                      hip_stream, vis_io, vis_dtype);
}

}  // extern "C"
