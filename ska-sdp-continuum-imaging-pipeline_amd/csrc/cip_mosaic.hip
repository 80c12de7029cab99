// cip_mosaic.hip - facet mosaicking (cip_mosaic_beta, cip_mosaic_taps,
// cip_mosaic_add, cip_mosaic_finish). The operator is defined in
// include/cip_mosaic.h.
//
// The add is a gather: one thread owns one output pixel of the facet's
// footprint, maps it into the facet (q = Q^T s), forms its 2 x 2a taps once and
// applies them to every plane. The kernel is instantiated per half-width a, so
// the tap arrays are indexed at compile time and stay in registers (64 VGPRs
// at a = 8). Per pixel and axis the taps cost one sinpi and 2a times (sqrt,
// exp, divide): sin(pi (fx - k)) = (-1)^k sin(pi fx).
//
// The map is nearly affine, so the 16 x 16 pixels of a workgroup read one
// facet window of about (16 fpx / px + 2a)^2 doubles. With staging on, the
// workgroup finds the window of its valid pixels (a wave reduction, then four
// LDS atomics a wave), and when it fits kWin x kWin it is copied to LDS once
// per plane with coalesced rows and the 4a^2 reads of a pixel are LDS reads;
// a tile whose window does not fit reads the facet directly. CIP_MOSAIC_LDS
// chooses (cip_params.hip; the A/B is in DESIGN.md 20).
//
// The geometry and the taps are written without fused multiply-adds (fp
// contract off) in the order of the header, so a pixel's coordinates are the
// numpy statement's to the rounding of sqrt; the tap sums may fuse.
#include <climits>
#include <cmath>
#include <string>
#include <type_traits>

#include "cip_host.h"
#include "cip_mosaic.h"

namespace cip {

namespace {

constexpr int kTile = 16;  // output pixels a workgroup covers per axis (256 threads)
constexpr int kWin = 48;   // the LDS window's edge and pitch: 48 = 16 mod 32 doubles, so the two 16-pixel rows
                           // of a 32-lane ds_read_b64 group fall on disjoint banks
constexpr double kPi = 3.141592653589793;
static_assert(kTile + 2 * CIP_MOSAIC_MAX_HALF + 2 <= kWin, "an unscaled tile's window fits at every half-width");

struct MosaicArgs {
  const double* facet;
  double* num;
  double* wsum;
  int64_t nplane, nx, ny, fnx, fny;
  int64_t i0, j0, ni, nj, tiles_j, tiles;  // the footprint's box, its tiles per row and in all
  int64_t cx, cy, fcx, fcy;         // nx / 2, ny / 2, fnx / 2, fny / 2
  double px, py, fpx, fpy;
  double a00, a01, a11, l0, m0, n0;  // Q^T = [a00 a01 -l0; a01 a11 -m0; l0 m0 n0]
  double beta, lo_x, hi_x, lo_y, hi_y, feather1;
  int nscale, stage;
};

// sin(pi f), 0 <= f < 1: exactly 0 at f = 0
__host__ __device__ inline double sinpi_frac(double f) {
#ifdef __HIP_DEVICE_COMPILE__
  return sinpi(f);
#else
  return std::sin(kPi * (f > 0.5 ? 1.0 - f : f));  // 1 - f is exact on (0.5, 1)
#endif
}

// the 2A normalised taps h(f - k), k = -A + 1 .. A (cip_mosaic.h)
template <int A>
__host__ __device__ inline void mosaic_taps(double beta, double f, double* t) {
#pragma clang fp contract(off)
  const double s = sinpi_frac(f);
#pragma unroll
  for (int q = 0; q < 2 * A; ++q) {
    const int k = q - A + 1;
    const double d = f - (double)k;
    const double u = d / (double)A;
    const double e = exp(beta * (sqrt(fmax(0.0, 1.0 - u * u)) - 1.0));
    double v = (((k & 1) ? -s : s) * e) / (kPi * d);
    if (d == 0.0) v = 1.0;
    if (fabs(d) >= (double)A) v = 0.0;
    t[q] = v;
  }
  double total = 0.0;
#pragma unroll
  for (int q = 0; q < A; ++q) total = (total + t[q]) + t[2 * A - 1 - q];  // outermost pair first
#pragma unroll
  for (int q = 0; q < 2 * A; ++q) t[q] = t[q] / total;
}

// the facet coordinates (x, y), the weight w (0: not valid) and q2 / n of the
// output pixel (i, j)
__device__ __forceinline__ double pixel_weight(const MosaicArgs& a, int64_t i, int64_t j, double* x, double* y,
                                               double* scale) {
#pragma clang fp contract(off)
  const double l = (double)(i - a.cx) * a.px, m = (double)(j - a.cy) * a.py;
  const double n = sqrt((1.0 - l * l) - m * m);
  const double q0 = (a.a00 * l + a.a01 * m) - a.l0 * n;
  const double q1 = (a.a01 * l + a.a11 * m) - a.m0 * n;
  const double q2 = (a.l0 * l + a.m0 * m) + a.n0 * n;
  *x = q0 / a.fpx + (double)a.fcx;
  *y = q1 / a.fpy + (double)a.fcy;
  *scale = q2 / n;
  const double dx = fmin(*x - a.lo_x, a.hi_x - *x), dy = fmin(*y - a.lo_y, a.hi_y - *y);
  if (!(dx >= 0.0 && dy >= 0.0 && q2 > 0.0)) return 0.0;
  return fmin(1.0, (dx + 1.0) / a.feather1) * fmin(1.0, (dy + 1.0) / a.feather1);
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// sum_k tx[k] (sum_q ty[q] f[k pitch + q]), both sums from the outermost pair
// of taps inwards (cip_mosaic.h)
template <int A, typename Pitch>
__device__ __forceinline__ double tap_sum(const double* tx, const double* ty, const double* f, Pitch pitch) {
  double val = 0.0;
#pragma unroll
  for (int kk = 0; kk < 2 * A; ++kk) {
    const int k = (kk & 1) ? 2 * A - 1 - kk / 2 : kk / 2;
    const double* r = f + k * pitch;
    double row = 0.0;
#pragma unroll
    for (int q = 0; q < A; ++q) {
      row += ty[q] * r[q];
      row += ty[2 * A - 1 - q] * r[2 * A - 1 - q];
    }
    val += tx[k] * row;
  }
  return val;
}

template <int A>
__global__ __launch_bounds__(kTile* kTile, 3) void mosaic_add_kernel(const MosaicArgs a) {
  __shared__ double s_win[kWin * kWin];
  __shared__ int s_box[4];  // min ix, min iy, -max ix, -max iy over the tile's valid pixels
  const int64_t ti = (int64_t)blockIdx.x / a.tiles_j, tj = (int64_t)blockIdx.x % a.tiles_j;
  const int64_t di = ti * kTile + (threadIdx.x >> 4), dj = tj * kTile + (threadIdx.x & 15);
  const int64_t i = a.i0 + di, j = a.j0 + dj;
  double w = 0.0, scale = 1.0, tx[2 * A], ty[2 * A];
  int ix = 0, iy = 0;
  if (di < a.ni && dj < a.nj) {
    double x, y;
    w = pixel_weight(a, i, j, &x, &y, &scale);
    if (w > 0.0) {  // lo <= x <= hi, so every tap lies inside the facet
      const double fx = floor(x), fy = floor(y);
      ix = (int)fx;
      iy = (int)fy;
      mosaic_taps<A>(a.beta, x - fx, tx);
      mosaic_taps<A>(a.beta, y - fy, ty);
    }
  }
  const bool on = w > 0.0;
  if (!a.nscale) scale = 1.0;
  bool staged = false;
  int wx0 = 0, wy0 = 0, wnx = 0, wny = 0;
  if (a.stage) {  // uniform
    if (threadIdx.x < 4) s_box[threadIdx.x] = INT_MAX;
    __syncthreads();
    const int b0 = wave_min(on ? ix : INT_MAX), b1 = wave_min(on ? iy : INT_MAX);
    const int b2 = wave_min(on ? -ix : INT_MAX), b3 = wave_min(on ? -iy : INT_MAX);
    if ((threadIdx.x & 63) == 0 && b0 != INT_MAX) {
      atomicMin(&s_box[0], b0);
      atomicMin(&s_box[1], b1);
      atomicMin(&s_box[2], b2);
      atomicMin(&s_box[3], b3);
    }
    __syncthreads();
    if (s_box[0] == INT_MAX) return;  // uniform: no valid pixel in this tile
    wx0 = s_box[0] - A + 1;
    wy0 = s_box[1] - A + 1;
    wnx = -s_box[2] + A - wx0 + 1;
    wny = -s_box[3] + A - wy0 + 1;
    staged = wnx <= kWin && wny <= kWin;
  }
  const int64_t plane = a.nx * a.ny, fplane = a.fnx * a.fny, out = i * a.ny + j;
  if (staged) {  // uniform
    const int base = (ix - A + 1 - wx0) * kWin + (iy - A + 1 - wy0);
    for (int64_t p = 0; p < a.nplane; ++p) {
      const double* f = a.facet + p * fplane + (int64_t)wx0 * a.fny + wy0;
      if (p) __syncthreads();  // the last plane's reads are done
      for (int c = threadIdx.x; c < wnx * wny; c += kTile * kTile) {
        const int r = c / wny, q = c - r * wny;
        s_win[r * kWin + q] = f[(int64_t)r * a.fny + q];
      }
      __syncthreads();
      if (on) {
        const double val = tap_sum<A>(tx, ty, s_win + base, kWin);
        a.num[p * plane + out] += w * (val * scale);
      }
    }
  } else if (on) {
    for (int64_t p = 0; p < a.nplane; ++p) {
      const double* f = a.facet + p * fplane + (int64_t)(ix - A + 1) * a.fny + (iy - A + 1);
      const double val = tap_sum<A>(tx, ty, f, a.fny);
      a.num[p * plane + out] += w * (val * scale);
    }
  }
  if (on) a.wsum[out] += w;
}

constexpr int kFinThreads = 256;
constexpr int kFinMaxBlocks = 2048;

__global__ __launch_bounds__(kFinThreads) void mosaic_finish_kernel(double* __restrict__ num,
                                                                    const double* __restrict__ wsum, int64_t nplane,
                                                                    int64_t n, double fill,
                                                                    unsigned long long* __restrict__ uncovered) {
  unsigned miss = 0;
  for (int64_t e = (int64_t)blockIdx.x * kFinThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kFinThreads) {
    const double ws = wsum[e];
    const bool on = ws > 0.0;
    miss += !on;
    for (int64_t p = 0; p < nplane; ++p) num[p * n + e] = on ? num[p * n + e] / ws : fill;
  }
  miss = wave_sum(miss);
  if ((threadIdx.x & 63) == 0 && miss) atomicAdd(uncovered, (unsigned long long)miss);
}

// ----------------------------------------------------------------- host ----
bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

int half_check(const std::string& who, int half) {
  if (half < 2 || half > CIP_MOSAIC_MAX_HALF)
    return set_error(CIP_EINVAL, who + ": half must be in 2 .. CIP_MOSAIC_MAX_HALF");
  return CIP_OK;
}

// f<A>() for the runtime half-width
template <typename F>
void for_half(int half, F&& f) {
  switch (half) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 8>()); break;
  }
}

int beta_impl(int half, double nu_max, double* beta_out) {
  const std::string who = "cip_mosaic_beta";
  if (!beta_out) return set_error(CIP_EINVAL, who + ": beta_out must not be NULL");
  if (const int rc = half_check(who, half); rc != CIP_OK) return rc;
  if (!(nu_max >= 0.0 && nu_max < 0.5)) return set_error(CIP_EINVAL, who + ": nu_max must lie in [0, 0.5)");
  *beta_out = kPi * half * (1.0 - 2.0 * nu_max);
  return CIP_OK;
}

int taps_impl(int half, double beta, double frac, double* taps_out) {
  const std::string who = "cip_mosaic_taps";
  if (!taps_out) return set_error(CIP_EINVAL, who + ": taps_out must not be NULL");
  if (const int rc = half_check(who, half); rc != CIP_OK) return rc;
  if (!(std::isfinite(beta) && beta >= 0.0)) return set_error(CIP_EINVAL, who + ": beta must be finite and >= 0");
  if (!(frac >= 0.0 && frac < 1.0)) return set_error(CIP_EINVAL, who + ": frac must lie in [0, 1)");
  for_half(half, [&](auto a) { mosaic_taps<decltype(a)::value>(beta, frac, taps_out); });
  return CIP_OK;
}

// The box of output pixels that can receive weight from the facet: the image
// of the valid rectangle [lo_x, hi_x] x [lo_y, hi_y] under the forward map
// s = Q (l', m', n'). On the front hemisphere the projection is one-to-one, so
// the footprint's extremes lie on the image of the rectangle's edges, which
// are walked a facet pixel at a time; the box is padded by two pixels and the
// longest step between two samples (an extreme between two samples lies no
// further out than a step). Along an edge l'^2 + m'^2 is convex and s2
// concave, so a rectangle that reaches the facet's limb or the far side does
// so at a corner: then the whole plane is taken. Returns false when the box
// misses the plane. Too tight a box would be a wrong answer, too wide a one
// only costs threads that find w = 0.
bool footprint(const MosaicArgs& a, int64_t* i0, int64_t* i1, int64_t* j0, int64_t* j1) {
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, step = 0.0;
  bool whole = false;
  const auto walk = [&](bool along_x, double fixed) {
    const double from = along_x ? a.lo_x : a.lo_y, to = along_x ? a.hi_x : a.hi_y;
    double last[2] = {0.0, 0.0};
    for (double t = from; t <= to && !whole; t += 1.0) {
      const double lf = ((along_x ? t : fixed) - (double)a.fcx) * a.fpx;
      const double mf = ((along_x ? fixed : t) - (double)a.fcy) * a.fpy;
      const double r2 = lf * lf + mf * mf;
      if (!(r2 < 1.0)) {
        whole = true;
        break;
      }
      const double nf = std::sqrt(1.0 - r2);
      const double s[3] = {a.a00 * lf + a.a01 * mf + a.l0 * nf, a.a01 * lf + a.a11 * mf + a.m0 * nf,
                           -a.l0 * lf - a.m0 * mf + a.n0 * nf};
      if (!(s[2] > 0.0)) {
        whole = true;
        break;
      }
      const double at[2] = {s[0] / a.px + (double)a.cx, s[1] / a.py + (double)a.cy};
      for (int d = 0; d < 2; ++d) {
        lo[d] = std::fmin(lo[d], at[d]);
        hi[d] = std::fmax(hi[d], at[d]);
        if (t > from) step = std::fmax(step, std::fabs(at[d] - last[d]));
        last[d] = at[d];
      }
    }
  };
  walk(true, a.lo_y);
  walk(true, a.hi_y);
  walk(false, a.lo_x);
  walk(false, a.hi_x);
  *i0 = 0, *i1 = a.nx - 1, *j0 = 0, *j1 = a.ny - 1;
  if (whole) return true;
  const double pad = 2.0 + std::ceil(step);
  if (hi[0] + pad < 0.0 || lo[0] - pad > (double)(a.nx - 1) || hi[1] + pad < 0.0 || lo[1] - pad > (double)(a.ny - 1))
    return false;
  *i0 = (int64_t)std::fmax(0.0, std::floor(lo[0] - pad));
  *i1 = (int64_t)std::fmin((double)(a.nx - 1), std::ceil(hi[0] + pad));
  *j0 = (int64_t)std::fmax(0.0, std::floor(lo[1] - pad));
  *j1 = (int64_t)std::fmin((double)(a.ny - 1), std::ceil(hi[1] + pad));
  return true;
}

// The argument checks of cip_mosaic_add and the kernel's arguments: the
// geometry, and the footprint's box and tiles (*empty: the facet misses the plane)
int mosaic_args(const cip_mosaic_geom* g, const double* facet, int64_t nplane, double l0, double m0, double* num_io,
                double* wsum_io, MosaicArgs* out, bool* empty) {
  const std::string who = "cip_mosaic_add";
  if (!g || !facet || !num_io || !wsum_io)
    return set_error(CIP_EINVAL, who + ": g, facet, num_io and wsum_io must not be NULL");
  if (g->nx < 1 || g->ny < 1 || g->fnx < 1 || g->fny < 1 || nplane < 1)
    return set_error(CIP_EINVAL, who + ": image dimensions and nplane must be >= 1");
  if (g->nx > INT64_MAX / g->ny || g->nx * g->ny > INT64_MAX / nplane)
    return set_error(CIP_EINVAL, who + ": nx ny nplane overflows int64");
  if (g->fnx > INT32_MAX || g->fny > INT32_MAX || g->fnx * g->fny > INT64_MAX / nplane)
    return set_error(CIP_EINVAL, who + ": the facet stack is too large");
  if (!positive_finite(g->px) || !positive_finite(g->py) || !positive_finite(g->fpx) || !positive_finite(g->fpy))
    return set_error(CIP_EINVAL, who + ": pixel sizes must be finite and > 0");
  if (const int rc = half_check(who, g->half); rc != CIP_OK) return rc;
  if (!(std::isfinite(g->beta) && g->beta >= 0.0))
    return set_error(CIP_EINVAL, who + ": beta must be finite and >= 0");
  if (g->trim < 0) return set_error(CIP_EINVAL, who + ": trim must be >= 0");
  if (!(std::isfinite(g->feather) && g->feather >= 0.0))
    return set_error(CIP_EINVAL, who + ": feather must be finite and >= 0");
  if (g->flags & ~CIP_MOSAIC_NSCALE) return set_error(CIP_EINVAL, who + ": unknown flag bits");
  if (!(l0 * l0 + m0 * m0 < 1.0)) return set_error(CIP_EINVAL, who + ": need l0^2 + m0^2 < 1");
  MosaicArgs a;
  a.facet = facet, a.num = num_io, a.wsum = wsum_io;
  a.nplane = nplane, a.nx = g->nx, a.ny = g->ny, a.fnx = g->fnx, a.fny = g->fny;
  a.cx = g->nx / 2, a.cy = g->ny / 2, a.fcx = g->fnx / 2, a.fcy = g->fny / 2;
  a.px = g->px, a.py = g->py, a.fpx = g->fpx, a.fpy = g->fpy;
  {  // the output plane's corners lie inside the unit disc
    const double lc = std::fmax((double)a.cx, (double)(g->nx - 1 - a.cx)) * g->px;
    const double mc = std::fmax((double)a.cy, (double)(g->ny - 1 - a.cy)) * g->py;
    if (!(lc * lc + mc * mc < 1.0)) return set_error(CIP_EINVAL, who + ": an output corner has l^2 + m^2 >= 1");
  }
  if (g->trim > INT32_MAX) return set_error(CIP_EINVAL, who + ": the facet is too small for half and trim");
  a.lo_x = a.lo_y = (double)(g->trim + g->half - 1);
  a.hi_x = (double)(g->fnx - 1 - g->trim - g->half);
  a.hi_y = (double)(g->fny - 1 - g->trim - g->half);
  if (a.hi_x < a.lo_x || a.hi_y < a.lo_y)
    return set_error(CIP_EINVAL, who + ": the facet is too small for half and trim (no valid pixel)");
  a.l0 = l0, a.m0 = m0;
  a.n0 = std::sqrt((1.0 - l0 * l0) - m0 * m0);
  {
    const double c = 1.0 / (1.0 + a.n0);
    a.a00 = 1.0 - (c * l0) * l0;
    a.a01 = -((c * l0) * m0);
    a.a11 = 1.0 - (c * m0) * m0;
  }
  a.beta = g->beta, a.feather1 = g->feather + 1.0;
  a.nscale = (g->flags & CIP_MOSAIC_NSCALE) != 0;
  a.stage = mosaic_lds();
  int64_t i0, i1, j0, j1;
  *empty = !footprint(a, &i0, &i1, &j0, &j1);
  if (*empty) return CIP_OK;
  a.i0 = i0, a.j0 = j0, a.ni = i1 - i0 + 1, a.nj = j1 - j0 + 1;
  a.tiles_j = (a.nj + kTile - 1) / kTile;
  a.tiles = ((a.ni + kTile - 1) / kTile) * a.tiles_j;
  if (a.tiles >= ((int64_t)1 << 31)) return set_error(CIP_EINVAL, who + ": the footprint has 2^31 tiles or more");
  *out = a;
  return CIP_OK;
}

int add_impl(const cip_mosaic_geom* g, const double* facet, int64_t nplane, double l0, double m0, void* hip_stream,
             double* num_io, double* wsum_io) {
  MosaicArgs a;
  bool empty = false;
  if (const int rc = mosaic_args(g, facet, nplane, l0, m0, num_io, wsum_io, &a, &empty); rc != CIP_OK) return rc;
  if (empty) return CIP_OK;  // the facet misses the plane
  const hipStream_t s = (hipStream_t)hip_stream;
  for_half(g->half, [&](auto h) {
    mosaic_add_kernel<decltype(h)::value><<<dim3((unsigned)a.tiles), dim3(kTile * kTile), 0, s>>>(a);
  });
  CIP_HIP_CHECK(hipGetLastError());
  return CIP_OK;
}

int finish_impl(double* num_io, const double* wsum, int64_t nplane, int64_t nx, int64_t ny, double fill,
                void* hip_stream, int64_t* n_uncovered_out) {
  const std::string who = "cip_mosaic_finish";
  if (!num_io || !wsum || !n_uncovered_out)
    return set_error(CIP_EINVAL, who + ": num_io, wsum and n_uncovered_out must not be NULL");
  if (nx < 1 || ny < 1 || nplane < 1) return set_error(CIP_EINVAL, who + ": image dimensions and nplane must be >= 1");
  if (nx > INT64_MAX / ny || nx * ny > INT64_MAX / nplane)
    return set_error(CIP_EINVAL, who + ": nx ny nplane overflows int64");
  const int64_t n = nx * ny;
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(count, unsigned long long, "mosaic_count", 1)
  const int64_t want = (n + kFinThreads - 1) / kFinThreads;
  const int blocks = (int)(want > kFinMaxBlocks ? kFinMaxBlocks : want);
  CIP_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
  mosaic_finish_kernel<<<dim3(blocks), dim3(kFinThreads), 0, s>>>(num_io, wsum, nplane, n, fill, count);
  CIP_HIP_CHECK(hipGetLastError());
  unsigned long long* h = nullptr;
  if (const int rc = readback(ws, s, {{count, sizeof(unsigned long long)}}, &h); rc != CIP_OK) return rc;
  *n_uncovered_out = (int64_t)*h;
  return CIP_OK;
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_mosaic_beta(int half, double nu_max, double* beta_out) {
  clear_error();
  return beta_impl(half, nu_max, beta_out);
}

int cip_mosaic_taps(int half, double beta, double frac, double* taps_out) {
  clear_error();
  return taps_impl(half, beta, frac, taps_out);
}

int cip_mosaic_add(const cip_mosaic_geom* g, const double* facet, int64_t nplane, double l0, double m0,
                   void* hip_stream, double* num_io, double* wsum_io) {
  clear_error();
  return add_impl(g, facet, nplane, l0, m0, hip_stream, num_io, wsum_io);
}

int cip_mosaic_finish(double* num_io, const double* wsum, int64_t nplane, int64_t nx, int64_t ny, double fill,
                      void* hip_stream, int64_t* n_uncovered_out) {
  clear_error();
  return finish_impl(num_io, wsum, nplane, nx, ny, fill, hip_stream, n_uncovered_out);
}

}  // extern "C"
