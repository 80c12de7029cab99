// cip_ms.hip - the scale kernels of multiscale CLEAN (cip_ms_scale_radius,
// cip_ms_scale_taps, cip_ms_convolve). The operator, rounding
// included, is defined in include/cip_ms.h; the minor cycle (cip_ms_clean) is
// in cip_clean.hip beside the other two.
//
// A scale kernel is a circular Gaussian, the outer product of one tap table
// with itself, so the convolution is two 1-D passes of 2R + 1 taps each:
//   rows:    tmp[i, j] = sum_d taps[d + R] in[i, j + d]. A workgroup takes
//            kRowsPerBlock rows x kSegment columns and stages each row segment
//            with its 2R halo in LDS (one coalesced read of the input; every
//            value is then read 2R + 1 times from LDS).
//   columns: out[i, j] = sum_d taps[d + R] tmp[i + d, j]. Adjacent lanes take
//            adjacent j, so every input row is one coalesced read per wave; a
//            thread computes kColRows consecutive rows from each value it
//            loads, and the rest of the 2R + 1-fold reuse of tmp, between the
//            waves of a workgroup and between neighbouring workgroups, is L2's.
// Each output is one thread's sum in ascending d, terms outside the image
// skipped: no cross-lane reduction, so the tap order is the definition. The
// tap index is uniform, so the taps come through the scalar cache. No atomics.
#include <algorithm>
#include <cmath>
#include <string>

#include "cip_host.h"
#include "cip_ms.h"
#include "cip_rounded.h"

namespace cip {

namespace {

constexpr int kMaxR = CIP_MS_MAX_RADIUS;
constexpr int kMaxTaps = 2 * kMaxR + 1;
constexpr int kThreads = 256;
constexpr int kSegment = 256;     // columns of a row segment: one per thread
constexpr int kRowsPerBlock = 4;  // rows the row pass stages at a time
constexpr int kColTileY = 64;     // the column pass: a wave takes 64 adjacent columns ...
constexpr int kColRows = 4;       // ... of kColRows consecutive rows, which share every input row they read
constexpr int kColTileX = kThreads / kColTileY * kColRows;
static_assert(kSegment == kThreads && kColTileY == 64, "one column per thread; a wave is 64 adjacent columns");
static_assert(kRowsPerBlock <= kColTileX && kSegment >= kColTileY, "convolve_impl bounds both grids by one product");

// grid: ceil(nx / kRowsPerBlock) * nseg workgroups
__global__ __launch_bounds__(kThreads) void ms_rows_kernel(const double* __restrict__ in, int64_t nx, int64_t ny,
                                                          int64_t nseg, int R, const double* __restrict__ taps,
                                                          double* __restrict__ tmp) {
  __shared__ double s_in[kRowsPerBlock][kSegment + 2 * kMaxR];
  const int64_t i0 = ((int64_t)blockIdx.x / nseg) * kRowsPerBlock, j0 = ((int64_t)blockIdx.x % nseg) * kSegment;
  const int width = kSegment + 2 * R;
  for (int r = 0; r < kRowsPerBlock; ++r) {
    const int64_t i = i0 + r;
    if (i >= nx) break;  // the same in every thread
    for (int c = threadIdx.x; c < width; c += kThreads) {
      const int64_t j = j0 - R + c;
      s_in[r][c] = (j >= 0 && j < ny) ? in[i * ny + j] : 0.0;  // outside: never read back
    }
  }
  __syncthreads();
  const int64_t j = j0 + threadIdx.x;
  if (j >= ny) return;
  // the taps d = d_lo .. d_hi whose column j + d lies inside the image
  const int d_lo = (int)std::max<int64_t>(-R, -j), d_hi = (int)std::min<int64_t>(R, ny - 1 - j);
  for (int r = 0; r < kRowsPerBlock; ++r) {
    const int64_t i = i0 + r;
    if (i >= nx) break;
    const double* row = s_in[r] + threadIdx.x + R;  // row[d]: column j + d
    double acc = 0.0;
    for (int d = -R; d <= R; ++d)  // uniform bounds: taps[d + R] is a scalar load
      if (d >= d_lo && d <= d_hi) acc = add_rounded(acc, mul_rounded(taps[d + R], row[d]));
    tmp[i * ny + j] = acc;
  }
}

// grid: ceil(nx / kColTileX) * ncol workgroups; thread (wave w, lane l) takes the kColRows pixels
// (i0 + kColRows w + r, j0 + l): it walks the input rows once, and row i0 + e feeds output row r with
// the tap d = e - r, so every output still adds its terms in ascending d
__global__ __launch_bounds__(kThreads) void ms_cols_kernel(const double* __restrict__ tmp, int64_t nx, int64_t ny,
                                                          int64_t ncol, int R, const double* __restrict__ taps,
                                                          double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)blockIdx.x / ncol) * kColTileX + wave * kColRows;
  const int64_t j = ((int64_t)blockIdx.x % ncol) * kColTileY + lane;
  if (i0 >= nx || j >= ny) return;
  // input rows i0 + e inside the image, e = -R .. R + kColRows - 1 (wave-uniform)
  const int e_lo = (int)std::max<int64_t>(-R, -i0), e_hi = (int)std::min<int64_t>(R + kColRows - 1, nx - 1 - i0);
  const double* col = tmp + i0 * ny + j;
  double acc[kColRows];
#pragma unroll
  for (int r = 0; r < kColRows; ++r) acc[r] = 0.0;
  for (int e = e_lo; e <= e_hi; ++e) {
    const double x = col[(int64_t)e * ny];
#pragma unroll
    for (int r = 0; r < kColRows; ++r) {
      const int d = e - r;
      if (d >= -R && d <= R) acc[r] = add_rounded(acc[r], mul_rounded(taps[d + R], x));
    }
  }
#pragma unroll
  for (int r = 0; r < kColRows; ++r)
    if (i0 + r < nx) out[(i0 + r) * ny + j] = acc[r];
}

hipError_t launch_convolve(const double* in, int64_t nx, int64_t ny, int R, const double* taps, double* tmp,
                           double* out, hipStream_t s) {
  const int64_t nseg = (ny + kSegment - 1) / kSegment, nrb = (nx + kRowsPerBlock - 1) / kRowsPerBlock;
  ms_rows_kernel<<<dim3((unsigned)(nrb * nseg)), dim3(kThreads), 0, s>>>(in, nx, ny, nseg, R, taps, tmp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t ncol = (ny + kColTileY - 1) / kColTileY, ncb = (nx + kColTileX - 1) / kColTileX;
  ms_cols_kernel<<<dim3((unsigned)(ncb * ncol)), dim3(kThreads), 0, s>>>(tmp, nx, ny, ncol, R, taps, out);
  return hipGetLastError();
}

// ------------------------------------------------------------ host API ----
int width_check(const char* who, double width) {
  if (!std::isfinite(width) || !(width == 0.0 || width >= 1.0))
    return set_error(CIP_EINVAL, std::string(who) + ": width (FWHM in pixels) must be 0 or a finite value >= 1");
  return CIP_OK;
}

// (4 log 2) / width^2: exp(-d^2 c) is a Gaussian of that FWHM
double scale_coefficient(double width) {
#pragma clang fp contract(off)
  return (4.0 * std::log(2.0)) / (width * width);
}

int scale_radius_impl(double width, double tol) {
  const char* who = "cip_ms_scale_radius";
  if (const int rc = width_check(who, width); rc != CIP_OK) return rc;
  if (!(tol > 0.0 && tol < 1.0)) return set_error(CIP_EINVAL, std::string(who) + ": tol must lie in (0, 1)");
  if (width == 0.0) return 0;
  const double rad = std::ceil(std::sqrt(std::log(1.0 / tol) / scale_coefficient(width)));
  if (!(rad <= (double)kMaxR))
    return set_error(CIP_ERANGE, std::string(who) + ": the scale needs a radius above CIP_MS_MAX_RADIUS (" +
                                     std::to_string(kMaxR) + " pixels) at this tol");
  return (int)rad;
}

int scale_taps_impl(double width, int64_t R, double* taps) {
#pragma clang fp contract(off)
  const char* who = "cip_ms_scale_taps";
  if (const int rc = width_check(who, width); rc != CIP_OK) return rc;
  if (!taps) return set_error(CIP_EINVAL, std::string(who) + ": taps_out must not be NULL");
  if (R < 0 || R > kMaxR) return set_error(CIP_EINVAL, std::string(who) + ": radius must be in 0 .. CIP_MS_MAX_RADIUS");
  if (width == 0.0) {
    if (R != 0) return set_error(CIP_EINVAL, std::string(who) + ": width 0 has radius 0");
    taps[0] = 1.0;
    return CIP_OK;
  }
  const double c = scale_coefficient(width);
  double sum = 0.0;
  for (int64_t d = -R; d <= R; ++d) {
    const double dd = (double)d;
    taps[d + R] = std::exp(-((dd * dd) * c));
    sum = sum + taps[d + R];
  }
  for (int64_t k = 0; k <= 2 * R; ++k) taps[k] = taps[k] / sum;
  return CIP_OK;
}

// both passes, queued on the caller's stream; the taps go up only when they
// differ from the table already on the device
int convolve_impl(const double* in, int64_t nx, int64_t ny, const double* taps, int64_t R, void* hip_stream,
                  double* out) {
  const char* who = "cip_ms_convolve";
  if (!in || !taps || !out) return set_error(CIP_EINVAL, std::string(who) + ": in, taps and out must not be NULL");
  if (nx < 1 || ny < 1) return set_error(CIP_EINVAL, std::string(who) + ": image dimensions must be >= 1");
  if (R < 0 || R > kMaxR) return set_error(CIP_EINVAL, std::string(who) + ": radius must be in 0 .. CIP_MS_MAX_RADIUS");
  for (int64_t k = 0; k <= 2 * R; ++k)
    if (!std::isfinite(taps[k])) return set_error(CIP_EINVAL, std::string(who) + ": every tap must be finite");
  if (nx > INT64_MAX / ny) return set_error(CIP_EINVAL, std::string(who) + ": image too large");
  // no more workgroups than this in either pass (kRowsPerBlock <= kColTileX rows, kColTileY <= kSegment columns)
  if (nx / kRowsPerBlock + 1 > (((int64_t)1 << 31) - 1) / (ny / kColTileY + 1))
    return set_error(CIP_EINVAL, std::string(who) + ": image needs 2^31 workgroups or more");
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(tmp, double, "ms_tmp", nx * ny)
  CIP_ALLOC(dtaps, double, "ms_taps", kMaxTaps)
  std::vector<double> key(taps, taps + 2 * R + 1);
  key.push_back((double)R);
  if (const int rc = host_table(ws, "ms_taps", key, dtaps, sizeof(double) * (size_t)(2 * R + 1), s,
                                [&](void* staging) { std::copy(taps, taps + 2 * R + 1, (double*)staging); });
      rc != CIP_OK)
    return rc;
  CIP_HIP_CHECK(launch_convolve(in, nx, ny, (int)R, dtaps, tmp, out, s));
  return CIP_OK;
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_ms_scale_radius(double width, double tol) {
  clear_error();
  return scale_radius_impl(width, tol);
}

int cip_ms_scale_taps(double width, int64_t radius, double* taps_out) {
  clear_error();
  return scale_taps_impl(width, radius, taps_out);
}

int cip_ms_convolve(const double* in, int64_t nx, int64_t ny, const double* taps, int64_t radius, void* hip_stream,
                    double* out) {
  clear_error();
  return convolve_impl(in, nx, ny, taps, radius, hip_stream, out);
}

}  // extern "C"
