// cip_rounded.h - fp64 arithmetic that is one rounded operation per step, never
// an FMA: hipcc contracts a * b + c by default, and the operators that are
// defined to the bit against numpy (CLEAN, restore, weights, gain calibration)
// must not. Contraction is off inside each helper.
#pragma once
#include <hip/hip_runtime.h>

namespace cip {

__device__ __forceinline__ double add_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// r - f * p: one rounded multiply, then one rounded subtract
__device__ __forceinline__ double sub_rounded(double r, double f, double p) {
#pragma clang fp contract(off)
  const double prod = f * p;
  return r - prod;
}

}  // namespace cip
