// cip_clean_util.h - device helpers the minor-cycle units share (cip_clean.hip,
// cip_mfs_clean.hip): the (|value|, flat index) candidate and its reductions,
// and the arithmetic that must not be contracted into FMAs.
#pragma once
#include "cip_internal.h"

namespace cip {

struct Cand {
  double a;     // |value|; -1: nothing selected yet
  int64_t idx;  // flat index; INT64_MAX: none
};

__device__ __forceinline__ Cand cand_none() { return {-1.0, INT64_MAX}; }

// `>` keeps NaN out (every comparison with it is false); ties go to the lower
// flat index, so any reduction order gives the same winner
__device__ __forceinline__ void cand_take(Cand& b, double a, int64_t idx) {
  if (a > b.a || (a == b.a && idx < b.idx)) {
    b.a = a;
    b.idx = idx;
  }
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(c.a, off, 64);
    const long long i = __shfl_down((long long)c.idx, off, 64);
    cand_take(c, a, (int64_t)i);
  }
  return c;  // lane 0 holds the wave's best
}

// the workgroup's best in thread 0 (nwaves <= 16)
template <int NWAVES>
__device__ __forceinline__ Cand block_best(Cand c) {
  __shared__ double s_a[NWAVES];
  __shared__ long long s_i[NWAVES];
  c = wave_best(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_a[wave] = c.a;
    s_i[wave] = (long long)c.idx;
  }
  __syncthreads();
  if (wave == 0) {
    Cand d = cand_none();
    if (lane < NWAVES) {
      d.a = s_a[lane];
      d.idx = (int64_t)s_i[lane];
    }
    c = wave_best(d);
  }
  return c;
}

// one rounded multiply, one rounded subtract: contraction is off for this
// expression (hipcc contracts a * b - c into an FMA by default)
__device__ __forceinline__ double sub_rounded(double r, double f, double p) {
#pragma clang fp contract(off)
  const double prod = f * p;
  return r - prod;
}

__device__ __forceinline__ double add_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

}  // namespace cip
