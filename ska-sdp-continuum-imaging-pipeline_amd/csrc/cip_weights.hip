// cip_weights.hip - uniform and Briggs (robust) imaging weights on the device
// (cip_weight_grid_init, cip_weight_density, cip_weight_stats,
// cip_weight_apply, cip_imaging_weights). The operator, rounding
// included, is defined in include/cip.h.
//
// The density is a small int64 array (one field-of-view cell per image pixel
// of a half plane); the work is the walk over the (row, channel) samples. A
// lane owns one row and kWeightSeg consecutive channels of it. A row's cells
// are monotone in frequency, so the lane keeps (cell, partial int64 sum) in
// registers and issues one no-return 64-bit integer atomic add each time the
// cell changes: one atomic per run of equal cells, not one per visibility.
// The apply kernel walks the same way and loads a run's density word once.
// Integer adds commute, so the density does not depend on arrival order; the
// two statistics are reduced in a fixed shape without atomics.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cip_host.h"
#include "cip_rounded.h"

namespace cip {

namespace {

constexpr int kWeightSeg = 16;       // channels per lane: 64 B of f32 weights, 128 B of f64
constexpr int kWeightThreads = 256;
constexpr int kStatBlocks = 256;     // stage 1 of the statistics: a fixed shape, whatever the grid
constexpr int kStatThreads = 256;
constexpr int kMaxBlocks = 2048;     // the max-reduction's grid-stride launch

// the grid as the kernels read it
struct WeightGeom {
  double sx, sy;    // npix * pixsize per axis
  double hx, hy;    // npix / 2 as doubles (the inside test is made before the cast)
  int64_t hxi, ny;  // hx, and hy + 1: cell (iu, iv) at (iu + hxi) * ny + iv
  double wmax, quantum;
  int shift;
};

struct WeightStatPart {
  long long sum;  // of the density words (exact)
  double d2;      // of D^2
  long long nz;   // non-zero cells
};

// the sample's flat cell, -1 when it lies outside; su = u * SX, sv = v * SY
__device__ __forceinline__ int64_t weight_cell(double su, double sv, double wi, const WeightGeom& g) {
#pragma clang fp contract(off)
  double x = wi * su, y = wi * sv;
  if (y < 0.0 || (y == 0.0 && x < 0.0)) {
    x = -x;
    y = -y;
  }
  const double fx = floor(x + 0.5), fy = floor(y + 0.5);
  // a NaN fails every comparison and an infinity the <=; fy >= 0 holds after the fold
  if (!(fabs(fx) <= g.hx && fy >= 0.0 && fy <= g.hy)) return -1;
  return ((int64_t)fx + g.hxi) * g.ny + (int64_t)fy;
}

__device__ __forceinline__ double briggs_denominator(double d, double f2) {
#pragma clang fp contract(off)
  const double p = d * f2;
  return 1.0 + p;
}

// The lane's n <= kWeightSeg weights from element `base` on, as doubles: 16-byte
// loads for a whole, aligned segment. The segment is loaded before anything is
// stored, so cip_weight_apply may run in place.
template <int WK>
__device__ __forceinline__ void load_segment(const void* wgt, int64_t base, int n, double (&w)[kWeightSeg]) {
  if constexpr (WK == WK_NONE) {
#pragma unroll
    for (int k = 0; k < kWeightSeg; ++k) w[k] = 1.0;
  } else if constexpr (WK == WK_F32) {
    const float* p = (const float*)wgt + base;
    if (n == kWeightSeg && ((uintptr_t)p & 15u) == 0u) {
#pragma unroll
      for (int k = 0; k < kWeightSeg / 4; ++k) {
        const float4 v = reinterpret_cast<const float4*>(p)[k];
        w[4 * k] = (double)v.x;
        w[4 * k + 1] = (double)v.y;
        w[4 * k + 2] = (double)v.z;
        w[4 * k + 3] = (double)v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kWeightSeg; ++k) w[k] = k < n ? (double)p[k] : 0.0;
    }
  } else {
    const double* p = (const double*)wgt + base;
    if (n == kWeightSeg && ((uintptr_t)p & 15u) == 0u) {
#pragma unroll
      for (int k = 0; k < kWeightSeg / 2; ++k) {
        const double2 v = reinterpret_cast<const double2*>(p)[k];
        w[2 * k] = v.x;
        w[2 * k + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kWeightSeg; ++k) w[k] = k < n ? p[k] : 0.0;
    }
  }
}

// One 16-byte group of the lane's results (fp64, each rounded once to OutT as
// it is stored): elements [k0, k0 + 16 / sizeof(OutT)) of the segment at p.
// Storing group by group keeps only one group's values live (held to the end
// of the segment, the f32 form needed every register of the lane).
template <typename OutT>
__device__ __forceinline__ void store_group(OutT* p, int k0, int n, bool vec, const double* r) {
  if constexpr (sizeof(OutT) == 4) {
    if (vec) {
      *reinterpret_cast<float4*>(p + k0) = make_float4((float)r[0], (float)r[1], (float)r[2], (float)r[3]);
      return;
    }
  } else {
    if (vec) {
      *reinterpret_cast<double2*>(p + k0) = make_double2(r[0], r[1]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 16 / (int)sizeof(OutT); ++j)
    if (k0 + j < n) p[k0 + j] = (OutT)r[j];
}

// lane t: row t / nseg, channels [kWeightSeg (t % nseg), ...) of it.
// counts: samples added, samples with w > 0 outside, bad samples
template <int WK>
__global__ __launch_bounds__(kWeightThreads) void weight_density_kernel(const double* __restrict__ uvw, int64_t nrow,
                                                                        const double* __restrict__ winv, int nchan,
                                                                        int nseg, const void* __restrict__ wgt,
                                                                        WeightGeom g, unsigned long long* density,
                                                                        unsigned long long* counts) {
  const int64_t t = (int64_t)blockIdx.x * kWeightThreads + threadIdx.x;
  unsigned n_add = 0, n_out = 0, n_bad = 0;
  if (t < nrow * nseg) {
    const int64_t r = t / nseg;
    const int c0 = (int)(t - r * nseg) * kWeightSeg;
    const int n = min(kWeightSeg, nchan - c0);
    const double su = mul_rounded(uvw[3 * r], g.sx), sv = mul_rounded(uvw[3 * r + 1], g.sy);
    double w[kWeightSeg];
    load_segment<WK>(wgt, r * nchan + c0, n, w);
    int64_t cur = -1;
    long long acc = 0;
#pragma unroll
    for (int k = 0; k < kWeightSeg; ++k) {
      if (k >= n) continue;
      const double wk = w[k];
      if (wk == 0.0) continue;
      if (!(wk > 0.0) || wk > g.wmax) {  // negative, NaN, above the grid's bound
        ++n_bad;
        continue;
      }
      const int64_t cell = weight_cell(su, sv, winv[c0 + k], g);
      if (cell < 0) {
        ++n_out;
        continue;
      }
      if (cell != cur) {
        if (cur >= 0) atomicAdd(density + cur, (unsigned long long)acc);
        cur = cell;
        acc = 0;
      }
      acc += llrint(ldexp(wk, g.shift));
      ++n_add;
    }
    if (cur >= 0) atomicAdd(density + cur, (unsigned long long)acc);
  }
  // three integer adds per workgroup
  __shared__ unsigned s_cnt[kWeightThreads / 64][3];
  n_add = wave_sum(n_add);
  n_out = wave_sum(n_out);
  n_bad = wave_sum(n_bad);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_cnt[wave][0] = n_add;
    s_cnt[wave][1] = n_out;
    s_cnt[wave][2] = n_bad;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long v = 0;
    for (int q = 0; q < kWeightThreads / 64; ++q) v += s_cnt[q][threadIdx.x];
    if (v) atomicAdd(counts + threadIdx.x, v);
  }
}

// wgt and out may be the same array: no __restrict__ on them
template <int WK, typename OutT>
__global__ __launch_bounds__(kWeightThreads) void weight_apply_kernel(const double* __restrict__ uvw, int64_t nrow,
                                                                      const double* __restrict__ winv, int nchan,
                                                                      int nseg, const void* wgt, WeightGeom g,
                                                                      const long long* __restrict__ density, int mode,
                                                                      double f2, OutT* out) {
  const int64_t t = (int64_t)blockIdx.x * kWeightThreads + threadIdx.x;
  if (t >= nrow * nseg) return;
  const int64_t r = t / nseg;
  const int c0 = (int)(t - r * nseg) * kWeightSeg;
  const int n = min(kWeightSeg, nchan - c0);
  const double su = mul_rounded(uvw[3 * r], g.sx), sv = mul_rounded(uvw[3 * r + 1], g.sy);
  double w[kWeightSeg];
  load_segment<WK>(wgt, r * nchan + c0, n, w);
  OutT* p = out + (r * nchan + c0);
  const bool vec = n == kWeightSeg && ((uintptr_t)p & 15u) == 0u;
  constexpr int kGroup = 16 / (int)sizeof(OutT);
  int64_t cur = -1;
  double d = 0.0;
#pragma unroll
  for (int k0 = 0; k0 < kWeightSeg; k0 += kGroup) {
    if (k0 >= n) break;
    double res[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const int k = k0 + j;
      res[j] = 0.0;
      if (k >= n) continue;
      const double wk = w[k];
      if (wk == 0.0) continue;
      const int64_t cell = weight_cell(su, sv, winv[c0 + k], g);
      if (cell < 0) continue;
      if (cell != cur) {
        cur = cell;
        d = mul_rounded((double)density[cell], g.quantum);
      }
      // one division either way: uniform divides by D, Briggs by 1 + D f2
      const double den = mode == CIP_WEIGHT_UNIFORM ? d : briggs_denominator(d, f2);
      res[j] = (mode == CIP_WEIGHT_UNIFORM && !(d > 0.0)) ? 0.0 : wk / den;
    }
    store_group<OutT>(p, k0, n, vec, res);
  }
}

// out[0]: the bits of the largest weight > 0 (non-negative doubles order as
// their bit patterns, so an integer max is exact); out[1]: negative or NaN
// weights seen
template <int WK>
__global__ __launch_bounds__(kWeightThreads) void weight_max_kernel(const void* __restrict__ wgt, int64_t n,
                                                                    unsigned long long* out) {
  double m = 0.0;
  unsigned bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kWeightThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kWeightThreads) {
    double w;
    if constexpr (WK == WK_F32) {
      w = (double)((const float*)wgt)[i];
    } else {
      w = ((const double*)wgt)[i];
    }
    if (!(w >= 0.0)) ++bad;
    if (w > m) m = w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(m, off, 64);
    if (o > m) m = o;
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    if (m > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
    if (bad) atomicAdd(out + 1, (unsigned long long)bad);
  }
}

// the workgroup's sums in thread 0: wave shuffles, then the waves in order
__device__ __forceinline__ WeightStatPart stat_block_sum(WeightStatPart p) {
  __shared__ long long s_sum[kStatThreads / 64], s_nz[kStatThreads / 64];
  __shared__ double s_d2[kStatThreads / 64];
  p.sum = wave_sum(p.sum);
  p.d2 = wave_sum(p.d2);
  p.nz = wave_sum(p.nz);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_sum[wave] = p.sum;
    s_d2[wave] = p.d2;
    s_nz[wave] = p.nz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kStatThreads / 64; ++q) {
      p.sum += s_sum[q];
      p.d2 += s_d2[q];
      p.nz += s_nz[q];
    }
  }
  return p;
}

// stage 1: thread i of the kStatBlocks * kStatThreads takes cells i, i + that many, ...
__global__ __launch_bounds__(kStatThreads) void weight_stats_kernel(const long long* __restrict__ density, int64_t ncell,
                                                                    double quantum, WeightStatPart* part) {
  WeightStatPart p = {0, 0.0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kStatThreads + threadIdx.x; i < ncell;
       i += (int64_t)kStatBlocks * kStatThreads) {
    const long long v = density[i];
    const double d = mul_rounded((double)v, quantum);
    p.sum += v;
    p.d2 += mul_rounded(d, d);
    p.nz += v != 0;
  }
  p = stat_block_sum(p);
  if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// stage 2: one workgroup over the kStatBlocks partial sums
__global__ __launch_bounds__(kStatThreads) void weight_stats_final_kernel(const WeightStatPart* __restrict__ part,
                                                                          WeightStatPart* out) {
  static_assert(kStatBlocks == kStatThreads, "one partial sum per thread");
  const WeightStatPart p = stat_block_sum(part[threadIdx.x]);
  if (threadIdx.x == 0) *out = p;
}

// f(int_tag<WK>{}) for a weight dtype code (validated by the entry points)
template <typename F>
auto dispatch_wgt(int wgt_dtype, F&& f) {
  if (wgt_dtype == CIP_F32) return f(int_tag<WK_F32>{});
  if (wgt_dtype == CIP_F64) return f(int_tag<WK_F64>{});
  return f(int_tag<WK_NONE>{});
}

// what every walk takes: the chunk's columns, the reciprocal wavelengths and the grid
struct WeightWalk {
  const double* uvw = nullptr;
  int64_t nrow = 0;
  const double* winv = nullptr;
  int nchan = 0;
  const void* wgt = nullptr;
  int wgt_dtype = CIP_NONE;
  WeightGeom g;
};

int walk_segments(int nchan) { return (nchan + kWeightSeg - 1) / kWeightSeg; }

dim3 walk_grid(const WeightWalk& a) {
  const int64_t lanes = a.nrow * walk_segments(a.nchan);
  return dim3((unsigned)((lanes + kWeightThreads - 1) / kWeightThreads));
}

hipError_t launch_weight_density(const WeightWalk& a, int64_t* density, unsigned long long* counts, hipStream_t s) {
  return dispatch_wgt(a.wgt_dtype, [&](auto wk) {
    weight_density_kernel<decltype(wk)::value><<<walk_grid(a), dim3(kWeightThreads), 0, s>>>(
        a.uvw, a.nrow, a.winv, a.nchan, walk_segments(a.nchan), a.wgt, a.g, (unsigned long long*)density, counts);
    return hipGetLastError();
  });
}

hipError_t launch_weight_apply(const WeightWalk& a, const int64_t* density, int mode, double f2, void* out,
                               int out_dtype, hipStream_t s) {
  return dispatch_wgt(a.wgt_dtype, [&](auto wk) {
    return dispatch_bool(out_dtype == CIP_F64, [&](auto wide) {
      using OutT = std::conditional_t<decltype(wide)::value, double, float>;
      weight_apply_kernel<decltype(wk)::value, OutT><<<walk_grid(a), dim3(kWeightThreads), 0, s>>>(
          a.uvw, a.nrow, a.winv, a.nchan, walk_segments(a.nchan), a.wgt, a.g, (const long long*)density, mode, f2,
          (OutT*)out);
      return hipGetLastError();
    });
  });
}

// out2 (device, 2 words): zeroed here, then {bits of the max, bad samples}; wgt_dtype F32 / F64
hipError_t launch_weight_max(const void* wgt, int wgt_dtype, int64_t n, unsigned long long* out2, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  const unsigned nb = (unsigned)std::min<int64_t>(kMaxBlocks, (n + kWeightThreads - 1) / kWeightThreads);
  return dispatch_bool(wgt_dtype == CIP_F64, [&](auto wide) {
    constexpr int kWk = decltype(wide)::value ? WK_F64 : WK_F32;
    weight_max_kernel<kWk><<<dim3(nb), dim3(kWeightThreads), 0, s>>>(wgt, n, out2);
    return hipGetLastError();
  });
}

// part: kStatBlocks + 1 entries, the last one the result
hipError_t launch_weight_stats(const int64_t* density, int64_t ncell, double quantum, WeightStatPart* part,
                               hipStream_t s) {
  weight_stats_kernel<<<dim3(kStatBlocks), dim3(kStatThreads), 0, s>>>((const long long*)density, ncell, quantum, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  weight_stats_final_kernel<<<dim3(1), dim3(kStatThreads), 0, s>>>(part, part + kStatBlocks);
  return hipGetLastError();
}

// ------------------------------------------------------------ host API ----

// the least integer e with v <= 2^e (v > 0, finite)
int ceil_log2(double v) {
  int e = 0;
  const double m = std::frexp(v, &e);  // v = m 2^e, 0.5 <= m < 1
  return m == 0.5 ? e - 1 : e;
}

int grid_init_impl(int64_t npix_x, int64_t npix_y, double px, double py, double wmax, int64_t nvis_max,
                   cip_weight_grid* out) {
  if (!out) return set_error(CIP_EINVAL, "cip_weight_grid_init: out must not be NULL");
  if (npix_x < 1 || npix_y < 1 || npix_x > ((int64_t)1 << 30) || npix_y > ((int64_t)1 << 30))
    return set_error(CIP_EINVAL, "cip_weight_grid_init: npix_x and npix_y must be in 1 .. 2^30");
  if (!std::isfinite(px) || !std::isfinite(py) || !(px > 0.0) || !(py > 0.0))
    return set_error(CIP_EINVAL, "cip_weight_grid_init: pixel sizes must be finite and > 0");
  if (!std::isfinite(wmax) || !(wmax > 0.0))
    return set_error(CIP_EINVAL, "cip_weight_grid_init: wmax must be finite and > 0");
  if (nvis_max < 1) return set_error(CIP_EINVAL, "cip_weight_grid_init: nvis_max must be >= 1");
  int b = 0;
  while (b < 63 && ((int64_t)1 << b) < nvis_max) ++b;
  const int shift = 62 - b - ceil_log2(wmax);
  if (shift < -1000 || shift > 1000)
    return set_error(CIP_EINVAL, "cip_weight_grid_init: wmax is too extreme for a normal fp64 quantum");
  out->npix_x = npix_x;
  out->npix_y = npix_y;
  out->pixsize_x = px;
  out->pixsize_y = py;
  out->SX = (double)npix_x * px;
  out->SY = (double)npix_y * py;
  out->wmax = wmax;
  out->quantum = std::ldexp(1.0, -shift);
  out->shift = shift;
  out->reserved = 0;
  return CIP_OK;
}

int64_t grid_cells(const cip_weight_grid& gr) { return (2 * (gr.npix_x / 2) + 1) * (gr.npix_y / 2 + 1); }

// a caller's grid is plain host memory: refuse one cip_weight_grid_init did not fill
int grid_check(const char* who, const cip_weight_grid* gr) {
  const std::string w(who);
  if (!gr) return set_error(CIP_EINVAL, w + ": grid must not be NULL");
  if (gr->npix_x < 1 || gr->npix_y < 1 || gr->npix_x > ((int64_t)1 << 30) || gr->npix_y > ((int64_t)1 << 30) ||
      gr->shift < -1000 || gr->shift > 1000 || gr->quantum != std::ldexp(1.0, -gr->shift) || !(gr->wmax > 0.0) ||
      !std::isfinite(gr->SX) || !std::isfinite(gr->SY))
    return set_error(CIP_EINVAL, w + ": grid was not filled by cip_weight_grid_init");
  return CIP_OK;
}

// the chunk's shape and pointers
int walk_check(const char* who, const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
               int wgt_dtype) {
  const std::string w(who);
  if (nrow < 0) return set_error(CIP_EINVAL, w + ": nrow must be >= 0");
  if (nchan < 1 || nchan > 65535) return set_error(CIP_EINVAL, w + ": nchan must be in 1 .. 65535");
  if (wgt_dtype != CIP_NONE && wgt_dtype != CIP_F32 && wgt_dtype != CIP_F64)
    return set_error(CIP_EINVAL, w + ": wgt_dtype must be CIP_NONE, CIP_F32 or CIP_F64");
  if (nrow > 0 && (wgt == nullptr) != (wgt_dtype == CIP_NONE))
    return set_error(CIP_EINVAL, w + ": wgt == NULL goes with CIP_NONE, and only with it");
  if (nrow > 0 && (!uvw || !freq)) return set_error(CIP_EINVAL, w + ": uvw and freq must not be NULL");
  // the launch has one lane per 16 channels of a row and fewer than 2^31 workgroups
  if (nrow > ((int64_t)1 << 31) * kWeightThreads / walk_segments((int)nchan) - kWeightThreads)
    return set_error(CIP_EINVAL, w + ": too many samples for one call (split the rows)");
  return CIP_OK;
}

// the walk of a chunk: the reciprocal wavelengths in the workspace, the grid as the kernels read it
int make_walk(Workspace* ws, hipStream_t s, const double* uvw, int64_t nrow, const double* freq, int64_t nchan,
              const void* wgt, int wgt_dtype, const cip_weight_grid& gr, WeightWalk* a) {
  CIP_ALLOC(winv, double, "weight_winv", nchan)
  CIP_HIP_CHECK(launch_wavelength_inv(freq, nchan, winv, s));
  a->uvw = uvw;
  a->nrow = nrow;
  a->winv = winv;
  a->nchan = (int)nchan;
  a->wgt = wgt;
  a->wgt_dtype = wgt_dtype;
  a->g.sx = gr.SX;
  a->g.sy = gr.SY;
  a->g.hxi = gr.npix_x / 2;
  a->g.ny = gr.npix_y / 2 + 1;
  a->g.hx = (double)(gr.npix_x / 2);
  a->g.hy = (double)(gr.npix_y / 2);
  a->g.wmax = gr.wmax;
  a->g.quantum = gr.quantum;
  a->g.shift = gr.shift;
  return CIP_OK;
}

// Waits for the stream once.
int density_run(Workspace* ws, hipStream_t s, const char* who, const WeightWalk& a, int64_t* density,
                int64_t* counts_out) {
  CIP_ALLOC(counts, unsigned long long, "weight_counts", 3)
  CIP_HIP_CHECK(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), s));
  CIP_HIP_CHECK(launch_weight_density(a, density, counts, s));
  int64_t* host = nullptr;
  if (const int rc = readback(ws, s, {{counts, 3 * sizeof(int64_t)}}, &host); rc != CIP_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 3; ++k) counts_out[k] = host[k];
  if (host[2] > 0)
    return set_error(CIP_ERANGE, std::string(who) + ": " + std::to_string(host[2]) +
                                     " weights are negative, NaN or above the grid's wmax");
  return CIP_OK;
}

// stats: sum_w, sum_d2, non-zero cells. Waits for the stream once.
int stats_run(Workspace* ws, hipStream_t s, const int64_t* density, const cip_weight_grid& gr, double* stats) {
  CIP_ALLOC(part, WeightStatPart, "weight_stat_part", kStatBlocks + 1)
  CIP_HIP_CHECK(launch_weight_stats(density, grid_cells(gr), gr.quantum, part, s));
  const WeightStatPart* p = nullptr;
  if (const int rc = readback(ws, s, {{part + kStatBlocks, sizeof(WeightStatPart)}}, &p); rc != CIP_OK) return rc;
  stats[0] = (double)p->sum * gr.quantum;
  stats[1] = p->d2;
  stats[2] = (double)p->nz;
  return CIP_OK;
}

int apply_check(const char* who, int mode, double f2, const void* out, int out_dtype, const void* wgt, int wgt_dtype,
                int64_t nrow) {
  const std::string w(who);
  if (mode != CIP_WEIGHT_UNIFORM && mode != CIP_WEIGHT_BRIGGS)
    return set_error(CIP_EINVAL, w + ": mode must be CIP_WEIGHT_UNIFORM or CIP_WEIGHT_BRIGGS");
  if (mode == CIP_WEIGHT_BRIGGS && !(f2 >= 0.0 && std::isfinite(f2)))
    return set_error(CIP_EINVAL, w + ": f2 must be finite and >= 0");
  if (out_dtype != CIP_F32 && out_dtype != CIP_F64)
    return set_error(CIP_EINVAL, w + ": out_dtype must be CIP_F32 or CIP_F64");
  if (nrow > 0 && !out) return set_error(CIP_EINVAL, w + ": wgt_out must not be NULL");
  if (out && out == wgt && out_dtype != wgt_dtype)
    return set_error(CIP_EINVAL, w + ": in place needs out_dtype == wgt_dtype");
  return CIP_OK;
}

int weight_density_impl(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                        int wgt_dtype, const cip_weight_grid* gr, void* hip_stream, int64_t* density,
                        int64_t* counts_out) {
  const char* who = "cip_weight_density";
  if (const int rc = grid_check(who, gr); rc != CIP_OK) return rc;
  if (const int rc = walk_check(who, uvw, nrow, freq, nchan, wgt, wgt_dtype); rc != CIP_OK) return rc;
  if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = 0;
  if (nrow == 0) return CIP_OK;
  if (!density) return set_error(CIP_EINVAL, "cip_weight_density: density_io must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  WeightWalk a;
  if (const int rc = make_walk(ws, s, uvw, nrow, freq, nchan, wgt, wgt_dtype, *gr, &a); rc != CIP_OK) return rc;
  return density_run(ws, s, who, a, density, counts_out);
}

int weight_stats_impl(const int64_t* density, const cip_weight_grid* gr, void* hip_stream, double* stats_out) {
  if (const int rc = grid_check("cip_weight_stats", gr); rc != CIP_OK) return rc;
  if (!density || !stats_out) return set_error(CIP_EINVAL, "cip_weight_stats: density and stats_out must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  return stats_run(ws, s, density, *gr, stats_out);
}

int weight_apply_impl(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                      int wgt_dtype, const int64_t* density, const cip_weight_grid* gr, int mode, double f2,
                      void* hip_stream, void* wgt_out, int out_dtype) {
  const char* who = "cip_weight_apply";
  if (const int rc = grid_check(who, gr); rc != CIP_OK) return rc;
  if (const int rc = walk_check(who, uvw, nrow, freq, nchan, wgt, wgt_dtype); rc != CIP_OK) return rc;
  if (const int rc = apply_check(who, mode, f2, wgt_out, out_dtype, wgt, wgt_dtype, nrow); rc != CIP_OK) return rc;
  if (nrow == 0) return CIP_OK;
  if (!density) return set_error(CIP_EINVAL, "cip_weight_apply: density must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  WeightWalk a;
  if (const int rc = make_walk(ws, s, uvw, nrow, freq, nchan, wgt, wgt_dtype, *gr, &a); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_weight_apply(a, density, mode, mode == CIP_WEIGHT_BRIGGS ? f2 : 0.0, wgt_out, out_dtype, s));
  return CIP_OK;
}

int imaging_weights_impl(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                         int wgt_dtype, int64_t npix_x, int64_t npix_y, double px, double py, int mode, double robust,
                         void* hip_stream, void* wgt_out, int out_dtype, cip_weight_info* info_out) {
  const char* who = "cip_imaging_weights";
  if (!std::isfinite(robust)) return set_error(CIP_EINVAL, "cip_imaging_weights: robust must be finite");
  if (const int rc = walk_check(who, uvw, nrow, freq, nchan, wgt, wgt_dtype); rc != CIP_OK) return rc;
  cip_weight_grid gr;
  // the shape checks with a provisional bound; the grid proper follows the max-reduction
  if (const int rc = grid_init_impl(npix_x, npix_y, px, py, 1.0, std::max<int64_t>(nrow * nchan, 1), &gr);
      rc != CIP_OK)
    return rc;
  if (const int rc = apply_check(who, mode, 0.0, wgt_out, out_dtype, wgt, wgt_dtype, nrow); rc != CIP_OK) return rc;
  cip_weight_info info = {0.0, 0.0, 0.0, gr.quantum, 0, 0, 0};
  if (info_out) *info_out = info;
  if (nrow == 0) return CIP_OK;
  CIP_BEGIN_CALL(hip_stream, false)
  const int64_t nvis = nrow * nchan;
  double wmax = 1.0;
  if (wgt) {
    CIP_ALLOC(mx, unsigned long long, "weight_max", 2)
    CIP_HIP_CHECK(launch_weight_max(wgt, wgt_dtype, nvis, mx, s));
    int64_t* host = nullptr;
    if (const int rc = readback(ws, s, {{mx, 2 * sizeof(int64_t)}}, &host); rc != CIP_OK) return rc;
    if (host[1] > 0)
      return set_error(CIP_ERANGE, "cip_imaging_weights: " + std::to_string(host[1]) + " weights are negative or NaN");
    std::memcpy(&wmax, &host[0], sizeof(double));
    if (!std::isfinite(wmax)) return set_error(CIP_ERANGE, "cip_imaging_weights: a weight is infinite");
    if (wmax == 0.0) {  // all weights zero: all-zero output
      CIP_HIP_CHECK(hipMemsetAsync(wgt_out, 0, (size_t)nvis * (out_dtype == CIP_F64 ? 8 : 4), s));
      return end_call(call);
    }
  }
  if (const int rc = grid_init_impl(npix_x, npix_y, px, py, wmax, nvis, &gr); rc != CIP_OK) return rc;
  const int64_t ncell = grid_cells(gr);
  CIP_ALLOC(density, int64_t, "weight_density", ncell)
  CIP_HIP_CHECK(hipMemsetAsync(density, 0, (size_t)ncell * sizeof(int64_t), s));
  WeightWalk a;
  if (const int rc = make_walk(ws, s, uvw, nrow, freq, nchan, wgt, wgt_dtype, gr, &a); rc != CIP_OK) return rc;
  int64_t counts[3];
  if (const int rc = density_run(ws, s, who, a, density, counts); rc != CIP_OK) return rc;
  double stats[3];
  if (const int rc = stats_run(ws, s, density, gr, stats); rc != CIP_OK) return rc;
  double f2 = 0.0;
  if (mode == CIP_WEIGHT_BRIGGS && stats[0] > 0.0) {
    const double t = 5.0 * std::pow(10.0, -robust);
    f2 = (t * t) / (stats[1] / stats[0]);
    if (!std::isfinite(f2)) return set_error(CIP_EINVAL, "cip_imaging_weights: robust gives no finite f2");
  }
  CIP_HIP_CHECK(launch_weight_apply(a, density, mode, f2, wgt_out, out_dtype, s));
  info.sum_w = stats[0];
  info.sum_d2 = stats[1];
  info.f2 = f2;
  info.quantum = gr.quantum;
  info.n_added = counts[0];
  info.n_outside = counts[1];
  info.n_cells = (int64_t)stats[2];
  if (info_out) *info_out = info;
  return end_call(call);
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_weight_grid_init(int64_t npix_x, int64_t npix_y, double pixsize_x, double pixsize_y, double wmax,
                         int64_t nvis_max, cip_weight_grid* out) {
  clear_error();
  return grid_init_impl(npix_x, npix_y, pixsize_x, pixsize_y, wmax, nvis_max, out);
}

int cip_weight_density(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                       int wgt_dtype, const cip_weight_grid* grid, void* hip_stream, int64_t* density_io,
                       int64_t* counts_out) {
  clear_error();
  return weight_density_impl(uvw, nrow, freq, nchan, wgt, wgt_dtype, grid, hip_stream, density_io, counts_out);
}

int cip_weight_stats(const int64_t* density, const cip_weight_grid* grid, void* hip_stream, double* stats_out) {
  clear_error();
  return weight_stats_impl(density, grid, hip_stream, stats_out);
}

int cip_weight_apply(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                     int wgt_dtype, const int64_t* density, const cip_weight_grid* grid, int mode, double f2,
                     void* hip_stream, void* wgt_out, int out_dtype) {
  clear_error();
  return weight_apply_impl(uvw, nrow, freq, nchan, wgt, wgt_dtype, density, grid, mode, f2, hip_stream, wgt_out,
                           out_dtype);
}

int cip_imaging_weights(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* wgt,
                        int wgt_dtype, int64_t npix_x, int64_t npix_y, double pixsize_x, double pixsize_y, int mode,
                        double robust, void* hip_stream, void* wgt_out, int out_dtype, cip_weight_info* info_out) {
  clear_error();
  return imaging_weights_impl(uvw, nrow, freq, nchan, wgt, wgt_dtype, npix_x, npix_y, pixsize_x, pixsize_y, mode,
                              robust, hip_stream, wgt_out, out_dtype, info_out);
}

}  // extern "C"
