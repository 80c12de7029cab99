// cip_cal.hip - antenna gain self-calibration on the device (cip_cal_scale_init,
// cip_cal_correlate, cip_cal_solve, cip_cal_apply, cip_gaincal).
// The operators, rounding included, are defined in include/cip_cal.h.
//
// The correlate is the hot part: one streaming pass over vis, model and wgt. A
// group of L lanes (a power of two chosen from nchan) owns a row; a lane owns
// runs of kCalRun consecutive channels, loaded 16 bytes at a time where nchan
// and the base pointers allow. The three fixed-point terms are summed in int64
// registers, reduced over the group with 64-bit shuffles, and the group's lead
// lane issues three no-return integer atomic adds into the row's cell: three
// atomics per row, not per sample. Integer adds commute, so corr does not
// depend on arrival order. The max pass of cip_gaincal and cip_cal_apply walk
// the rows the same way.
//
// The solve first expands corr into full Hermitian fp64 A and B, stored
// [s][q][p] so that lane p reads consecutive addresses for a fixed q; then one
// workgroup per interval, one thread per antenna, runs every iteration inside
// one launch with the gains double-buffered in LDS.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cip_cal.h"
#include "cip_host.h"
#include "cip_rounded.h"

// every kernel below is defined to the bit: no a * b + c becomes an FMA
#pragma clang fp contract(off)

namespace cip {

namespace {

constexpr int kCalThreads = 256;
constexpr int kCalRun = 4;         // consecutive channels a lane takes per step
constexpr int kCalMaxLanes = 64;   // lanes per row at most: one wave
constexpr int kCalMaxBlocks = 4096;  // workgroups of the correlate's grid-stride launch
constexpr int kMaxAnt = CIP_CAL_MAX_ANT;
enum { CAL_ADD = 0, CAL_MAX = 1 };

// the rows as the walks read them
struct CalRows {
  const int32_t* ant1;
  const int32_t* ant2;
  const int32_t* interval;
  int64_t nrow;
  int nchan;
  int lanes;  // L: lanes per row
  int n_ant, n_int;
  bool vec;   // nchan % kCalRun == 0 and every base pointer 16-byte aligned
};

struct CalBounds {
  double amax, wmax;
  int shift;
};

// n <= kCalRun complex samples from p on, as doubles
template <typename C>
__device__ __forceinline__ void load_cplx_run(const C* p, int n, bool vec, double (&re)[kCalRun],
                                              double (&im)[kCalRun]) {
  if (vec) {
    if constexpr (sizeof(C) == 8) {
#pragma unroll
      for (int k = 0; k < kCalRun / 2; ++k) {
        const float4 a = reinterpret_cast<const float4*>(p)[k];
        re[2 * k] = (double)a.x;
        im[2 * k] = (double)a.y;
        re[2 * k + 1] = (double)a.z;
        im[2 * k + 1] = (double)a.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCalRun; ++k) {
        const double2 a = reinterpret_cast<const double2*>(p)[k];
        re[k] = a.x;
        im[k] = a.y;
      }
    }
  } else {
    using R = std::conditional_t<sizeof(C) == 8, float, double>;
    const R* f = reinterpret_cast<const R*>(p);
#pragma unroll
    for (int k = 0; k < kCalRun; ++k) {
      re[k] = k < n ? (double)f[2 * k] : 0.0;
      im[k] = k < n ? (double)f[2 * k + 1] : 0.0;
    }
  }
}

// n <= kCalRun weights from element `base` on (WK_NONE: ones)
template <int WK>
__device__ __forceinline__ void load_real_run(const void* wgt, int64_t base, int n, bool vec, double (&w)[kCalRun]) {
  if constexpr (WK == WK_NONE) {
#pragma unroll
    for (int k = 0; k < kCalRun; ++k) w[k] = 1.0;
  } else if constexpr (WK == WK_F32) {
    const float* p = (const float*)wgt + base;
    if (vec) {
      const float4 a = *reinterpret_cast<const float4*>(p);
      w[0] = (double)a.x;
      w[1] = (double)a.y;
      w[2] = (double)a.z;
      w[3] = (double)a.w;
    } else {
#pragma unroll
      for (int k = 0; k < kCalRun; ++k) w[k] = k < n ? (double)p[k] : 0.0;
    }
  } else {
    const double* p = (const double*)wgt + base;
    if (vec) {
#pragma unroll
      for (int k = 0; k < kCalRun / 2; ++k) {
        const double2 a = reinterpret_cast<const double2*>(p)[k];
        w[2 * k] = a.x;
        w[2 * k + 1] = a.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCalRun; ++k) w[k] = k < n ? p[k] : 0.0;
    }
  }
}

// the run's results, each rounded once to the element type of C
template <typename C>
__device__ __forceinline__ void store_cplx_run(C* p, int n, bool vec, const double (&re)[kCalRun],
                                               const double (&im)[kCalRun]) {
  if (vec) {
    if constexpr (sizeof(C) == 8) {
#pragma unroll
      for (int k = 0; k < kCalRun / 2; ++k)
        reinterpret_cast<float4*>(p)[k] =
            make_float4((float)re[2 * k], (float)im[2 * k], (float)re[2 * k + 1], (float)im[2 * k + 1]);
    } else {
#pragma unroll
      for (int k = 0; k < kCalRun; ++k) reinterpret_cast<double2*>(p)[k] = make_double2(re[k], im[k]);
    }
  } else {
    using R = std::conditional_t<sizeof(C) == 8, float, double>;
    R* f = reinterpret_cast<R*>(p);
#pragma unroll
    for (int k = 0; k < kCalRun; ++k)
      if (k < n) {
        f[2 * k] = (R)re[k];
        f[2 * k + 1] = (R)im[k];
      }
  }
}

template <typename R>
__device__ __forceinline__ void store_real_run(R* p, int n, bool vec, const double (&w)[kCalRun]) {
  if (vec) {
    if constexpr (sizeof(R) == 4) {
      *reinterpret_cast<float4*>(p) = make_float4((float)w[0], (float)w[1], (float)w[2], (float)w[3]);
    } else {
      reinterpret_cast<double2*>(p)[0] = make_double2(w[0], w[1]);
      reinterpret_cast<double2*>(p)[1] = make_double2(w[2], w[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kCalRun; ++k)
      if (k < n) p[k] = (R)w[k];
  }
}

__device__ __forceinline__ bool finite4(double a, double b, double c, double d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

__device__ __forceinline__ double max_abs4(double a, double b, double c, double d) {
  return fmax(fmax(fabs(a), fabs(b)), fmax(fabs(c), fabs(d)));
}

// Workgroup b takes the row blocks b, b + gridDim, ... of kCalThreads / L rows each (nblk in all); in a block,
// thread t has row t / L and is lane t % L of it, channels [kCalRun (l + L j), + kCalRun) for j = 0, 1, ...
// The counts and the maxima stay in registers over the row blocks, so the few words every workgroup
// shares see one atomic per workgroup (or wave), not one per row block.
// CAL_ADD: corr += the rows' fixed-point terms; out4 = the four counts.
// CAL_MAX: out4[0], out4[1] = the bits of the largest |component| and the
// largest w of the samples CAL_ADD would add without its two bounds.
template <typename VC, typename MC, int WK, int MODE>
__global__ __launch_bounds__(kCalThreads) void cal_correlate_kernel(const VC* __restrict__ vis,
                                                                    const MC* __restrict__ model,
                                                                    const void* __restrict__ wgt, CalRows a,
                                                                    CalBounds b, int64_t nblk,
                                                                    unsigned long long* corr,
                                                                    unsigned long long* out4) {
  const int L = a.lanes;
  const int l = threadIdx.x & (L - 1);
  unsigned n_add = 0, n_zero = 0, n_out = 0, n_bad = 0;
  double ma = 0.0, mw = 0.0;
  for (int64_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {  // uniform over the workgroup
    const int64_t r = rb * (kCalThreads / L) + threadIdx.x / L;
    const bool in = r < a.nrow;
    int p = 0, q = 0, s = 0;
    bool row_ok = false, fold = false;
    if (in) {
      p = a.ant1[r];
      q = a.ant2[r];
      s = a.interval[r];
      row_ok = p != q && p >= 0 && p < a.n_ant && q >= 0 && q < a.n_ant && s >= 0 && s < a.n_int;
      if (p > q) {
        const int t = p;
        p = q;
        q = t;
        fold = true;
      }
    }
    long long s0 = 0, s1 = 0, s2 = 0;
    if (in) {
      for (int c0 = l * kCalRun; c0 < a.nchan; c0 += L * kCalRun) {
        const int n = min(kCalRun, a.nchan - c0);
        if (!row_ok) {
          n_out += n;
          continue;
        }
        const int64_t base = r * a.nchan + c0;
        double w[kCalRun], vr[kCalRun], vi[kCalRun], mr[kCalRun], mi[kCalRun];
        load_real_run<WK>(wgt, base, n, a.vec, w);
        load_cplx_run(vis + base, n, a.vec, vr, vi);
        load_cplx_run(model + base, n, a.vec, mr, mi);
#pragma unroll
        for (int k = 0; k < kCalRun; ++k) {
          if (k >= n) continue;
          const double wk = w[k];
          if (wk == 0.0) {
            ++n_zero;
            continue;
          }
          if (!(wk > 0.0) || !isfinite(wk) || !finite4(vr[k], vi[k], mr[k], mi[k])) {
            ++n_bad;
            continue;
          }
          const double big = max_abs4(vr[k], vi[k], mr[k], mi[k]);
          if constexpr (MODE == CAL_MAX) {
            ma = fmax(ma, big);
            mw = fmax(mw, wk);
          } else {
            if (wk > b.wmax || big > b.amax) {
              ++n_out;
              continue;
            }
            const double cr = add_rounded(mul_rounded(vr[k], mr[k]), mul_rounded(vi[k], mi[k]));
            const double ci = add_rounded(mul_rounded(vi[k], mr[k]), -mul_rounded(vr[k], mi[k]));
            const double m2 = add_rounded(mul_rounded(mr[k], mr[k]), mul_rounded(mi[k], mi[k]));
            s0 += llrint(ldexp(mul_rounded(wk, cr), b.shift));
            s1 += llrint(ldexp(mul_rounded(wk, ci), b.shift));
            s2 += llrint(ldexp(mul_rounded(wk, m2), b.shift));
            ++n_add;
          }
        }
      }
    }
    if constexpr (MODE == CAL_ADD) {
      // the group's sums in its lead lane
      s0 = wave_sum(s0, L);
      s1 = wave_sum(s1, L);
      s2 = wave_sum(s2, L);
      if (l == 0 && row_ok && (s0 | s1 | s2) != 0) {
        unsigned long long* cell = corr + (((int64_t)s * a.n_ant + p) * a.n_ant + q) * 3;
        atomicAdd(cell, (unsigned long long)s0);
        atomicAdd(cell + 1, (unsigned long long)(fold ? -s1 : s1));
        atomicAdd(cell + 2, (unsigned long long)s2);
      }
    }
  }
  if constexpr (MODE == CAL_MAX) {
    // non-negative doubles order as their bit patterns: an integer max is exact
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ma = fmax(ma, __shfl_down(ma, off, 64));
      mw = fmax(mw, __shfl_down(mw, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      if (ma > 0.0) atomicMax(out4, (unsigned long long)__double_as_longlong(ma));
      if (mw > 0.0) atomicMax(out4 + 1, (unsigned long long)__double_as_longlong(mw));
    }
  } else {
    // four integer adds per workgroup
    __shared__ unsigned long long s_cnt[kCalThreads / 64][4];
    using u64 = unsigned long long;
    const u64 c_add = wave_sum((u64)n_add), c_zero = wave_sum((u64)n_zero);
    const u64 c_out = wave_sum((u64)n_out), c_bad = wave_sum((u64)n_bad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
      s_cnt[wave][0] = c_add;
      s_cnt[wave][1] = c_zero;
      s_cnt[wave][2] = c_out;
      s_cnt[wave][3] = c_bad;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      unsigned long long v = 0;
      for (int k = 0; k < kCalThreads / 64; ++k) v += s_cnt[k][threadIdx.x];
      if (v) atomicAdd(out4 + threadIdx.x, v);
    }
  }
}

// corr -> A (re, im) and B, each [s][q][p]; thread per element
__global__ __launch_bounds__(kCalThreads) void cal_expand_kernel(const long long* __restrict__ corr, int64_t total,
                                                                 int n, double quantum, double* __restrict__ ar,
                                                                 double* __restrict__ ai, double* __restrict__ bb) {
  const int64_t t = (int64_t)blockIdx.x * kCalThreads + threadIdx.x;
  if (t >= total) return;
  const int p = (int)(t % n);
  const int64_t sq = t / n;
  const int q = (int)(sq % n);
  const int64_t s = sq / n;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  if (p != q) {
    const int lo = min(p, q), hi = max(p, q);
    const long long* cell = corr + ((s * n + lo) * n + hi) * 3;
    d0 = mul_rounded((double)cell[0], quantum);
    d1 = mul_rounded((double)cell[1], quantum);
    d2 = mul_rounded((double)cell[2], quantum);
    if (p > q) d1 = -d1;  // A_pq = conj(A_qp)
  }
  ar[t] = d0;
  ai[t] = d1;
  bb[t] = d2;
}

struct SolveStat {
  long long iters, converged, n_dead, ref_missing;
  double d2, n2;
};

// One workgroup per interval, thread p = antenna p. gains (n_int, n) as double2.
__global__ __launch_bounds__(kMaxAnt) void cal_solve_kernel(const double* __restrict__ ar,
                                                            const double* __restrict__ ai,
                                                            const double* __restrict__ bb, int n, long long niter,
                                                            double tol2, int refant, int phase_only, double2* gains,
                                                            uint8_t* ant_ok, long long* iters_out,
                                                            SolveStat* stat) {
  __shared__ double s_gr[2][kMaxAnt], s_gi[2][kMaxAnt], s_m2[2][kMaxAnt];
  __shared__ uint8_t s_dead[kMaxAnt];
  __shared__ int s_conv;
  __shared__ double s_d2, s_n2;
  const int64_t s = blockIdx.x;
  const int p = threadIdx.x;
  const bool mine = p < n;
  const int64_t off = s * (int64_t)n * n;
  const double* arp = ar + off + p;
  const double* aip = ai + off + p;
  const double* bbp = bb + off + p;
  double2 g_in = make_double2(0.0, 0.0);
  if (mine) {
    g_in = gains[s * n + p];
    s_gr[0][p] = g_in.x;
    s_gi[0][p] = g_in.y;
    s_m2[0][p] = add_rounded(mul_rounded(g_in.x, g_in.x), mul_rounded(g_in.y, g_in.y));
    s_dead[p] = 0;
  }
  if (p == 0) {
    s_conv = 0;
    s_d2 = 0.0;
    s_n2 = 0.0;
  }
  __syncthreads();
  int cur = 0;
  bool dead = false;
  long long k_done = 0;
  if (niter == 0 && mine) {  // ant_ok alone: the denominator of iteration 1
    double den = 0.0;
    for (int q = 0; q < n; ++q) den = add_rounded(den, mul_rounded(bbp[(int64_t)q * n], s_m2[0][q]));
    dead = den == 0.0;
    s_dead[p] = dead;
  }
  for (long long k = 1; k <= niter; ++k) {
    const int nxt = cur ^ 1;
    if (mine) {
      double gr = s_gr[cur][p], gi = s_gi[cur][p];
      if (!dead) {
        double nr = 0.0, ni = 0.0, den = 0.0;
        for (int q = 0; q < n; ++q) {
          const double a_r = arp[(int64_t)q * n], a_i = aip[(int64_t)q * n], b_q = bbp[(int64_t)q * n];
          const double qr = s_gr[cur][q], qi = s_gi[cur][q];
          nr = add_rounded(nr, add_rounded(mul_rounded(a_r, qr), -mul_rounded(a_i, qi)));
          ni = add_rounded(ni, add_rounded(mul_rounded(a_r, qi), mul_rounded(a_i, qr)));
          den = add_rounded(den, mul_rounded(b_q, s_m2[cur][q]));
        }
        if (k == 1 && den == 0.0) {
          dead = true;
          s_dead[p] = 1;
        } else {
          double xr = nr / den, xi = ni / den;
          if (phase_only) {
            const double av = sqrt(add_rounded(mul_rounded(xr, xr), mul_rounded(xi, xi)));
            xr = xr / av;
            xi = xi / av;
          }
          if ((k & 1) == 0) {
            xr = mul_rounded(0.5, add_rounded(xr, gr));
            xi = mul_rounded(0.5, add_rounded(xi, gi));
          }
          gr = xr;
          gi = xi;
        }
      }
      s_gr[nxt][p] = gr;
      s_gi[nxt][p] = gi;
      s_m2[nxt][p] = add_rounded(mul_rounded(gr, gr), mul_rounded(gi, gi));
    }
    __syncthreads();
    if (p == 0) {  // the norms, summed in antenna order
      double d2 = 0.0, n2 = 0.0;
      for (int q = 0; q < n; ++q) {
        const double dr = add_rounded(s_gr[nxt][q], -s_gr[cur][q]), di = add_rounded(s_gi[nxt][q], -s_gi[cur][q]);
        d2 = add_rounded(d2, add_rounded(mul_rounded(dr, dr), mul_rounded(di, di)));
        n2 = add_rounded(n2, s_m2[nxt][q]);
      }
      s_d2 = d2;
      s_n2 = n2;
      s_conv = d2 <= mul_rounded(tol2, n2);
    }
    __syncthreads();
    cur = nxt;
    k_done = k;
    if (s_conv) break;  // uniform: read after the barrier, rewritten only after the next one
  }
  // the reference rotation, live antennas only
  bool ref_missing = false;
  double gr = mine ? s_gr[cur][p] : 0.0, gi = mine ? s_gi[cur][p] : 0.0;
  if (niter > 0 && refant >= 0) {
    if (s_dead[refant]) {
      ref_missing = true;
    } else {
      const double rr = s_gr[cur][refant], ri = s_gi[cur][refant];
      const double av = sqrt(s_m2[cur][refant]);
      const double ur = rr / av, ui = -(ri / av);
      if (mine && !dead) {
        const double xr = add_rounded(mul_rounded(gr, ur), -mul_rounded(gi, ui));
        const double xi = add_rounded(mul_rounded(gr, ui), mul_rounded(gi, ur));
        gr = xr;
        gi = xi;
      }
    }
  }
  if (mine) {
    ant_ok[s * n + p] = dead ? 0 : 1;
    if (!dead && niter > 0) gains[s * n + p] = make_double2(gr, gi);
  }
  __syncthreads();  // s_dead of the niter == 0 path
  if (p == 0) {
    long long nd = 0;
    for (int q = 0; q < n; ++q) nd += s_dead[q];
    SolveStat st;
    st.iters = k_done;
    st.converged = s_conv;
    st.n_dead = nd;
    st.ref_missing = ref_missing;
    st.d2 = s_d2;
    st.n2 = s_n2;
    stat[s] = st;
    if (iters_out) iters_out[s] = k_done;
  }
}

// vis and vis_out, wgt and wgt_out may be the same arrays: no __restrict__ on them
template <typename VC, int WK>
__global__ __launch_bounds__(kCalThreads) void cal_apply_kernel(const VC* vis, const void* wgt, CalRows a,
                                                                const double2* __restrict__ gains,
                                                                const uint8_t* __restrict__ ant_ok, int mode,
                                                                VC* vis_out, void* wgt_out) {
  const int L = a.lanes;
  const int64_t r = (int64_t)blockIdx.x * (kCalThreads / L) + threadIdx.x / L;
  const int l = threadIdx.x & (L - 1);
  if (r >= a.nrow) return;
  const int p = a.ant1[r], q = a.ant2[r], s = a.interval[r];
  bool pass = !(p >= 0 && p < a.n_ant && q >= 0 && q < a.n_ant && s >= 0 && s < a.n_int);
  double hr = 1.0, hi = 0.0, n2 = 1.0;
  if (!pass) {
    const int64_t ip = (int64_t)s * a.n_ant + p, iq = (int64_t)s * a.n_ant + q;
    pass = !(ant_ok[ip] && ant_ok[iq]);
    if (!pass) {
      const double2 gp = gains[ip], gq = gains[iq];
      hr = add_rounded(mul_rounded(gp.x, gq.x), mul_rounded(gp.y, gq.y));
      hi = add_rounded(mul_rounded(gp.y, gq.x), -mul_rounded(gp.x, gq.y));
      n2 = add_rounded(mul_rounded(hr, hr), mul_rounded(hi, hi));
    }
  }
  using WT = std::conditional_t<WK == WK_F64, double, float>;
  for (int c0 = l * kCalRun; c0 < a.nchan; c0 += L * kCalRun) {
    const int n = min(kCalRun, a.nchan - c0);
    const int64_t base = r * a.nchan + c0;
    double w[kCalRun], vr[kCalRun], vi[kCalRun];
    load_real_run<WK>(wgt, base, n, a.vec, w);
    load_cplx_run(vis + base, n, a.vec, vr, vi);
#pragma unroll
    for (int k = 0; k < kCalRun; ++k) {
      if (pass) {
        w[k] = 0.0;
      } else if (mode == CIP_CAL_CORRECT) {
        const double xr = add_rounded(mul_rounded(vr[k], hr), mul_rounded(vi[k], hi));
        const double xi = add_rounded(mul_rounded(vi[k], hr), -mul_rounded(vr[k], hi));
        vr[k] = xr / n2;
        vi[k] = xi / n2;
        w[k] = mul_rounded(w[k], n2);
      } else {
        const double xr = add_rounded(mul_rounded(hr, vr[k]), -mul_rounded(hi, vi[k]));
        const double xi = add_rounded(mul_rounded(hr, vi[k]), mul_rounded(hi, vr[k]));
        vr[k] = xr;
        vi[k] = xi;
      }
    }
    store_cplx_run(vis_out + base, n, a.vec, vr, vi);
    if constexpr (WK != WK_NONE) store_real_run((WT*)wgt_out + base, n, a.vec, w);
  }
}

// ------------------------------------------------------------ launchers ----

// lanes per row: the least power of two with kCalRun * L >= nchan, one wave at most
int cal_lanes(int nchan) {
  int lanes = 1;
  while (lanes < kCalMaxLanes && lanes * kCalRun < nchan) lanes *= 2;
  return lanes;
}

// row blocks of kCalThreads / L rows
int64_t cal_row_blocks(const CalRows& a) {
  const int rows = kCalThreads / a.lanes;
  return (a.nrow + rows - 1) / rows;
}

// the apply has one workgroup per row block (rows_check bounds their number)
dim3 cal_grid(const CalRows& a) { return dim3((unsigned)cal_row_blocks(a)); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }

// f(type_tag<float2 or double2>{}) for a complex dtype code (validated by the entry points)
template <typename F>
auto dispatch_cplx(int dtype, F&& f) {
  if (dtype == CIP_C64) return f(type_tag<float2>{});
  return f(type_tag<double2>{});
}

template <typename F>
auto dispatch_real(int dtype, F&& f) {
  if (dtype == CIP_F32) return f(int_tag<WK_F32>{});
  if (dtype == CIP_F64) return f(int_tag<WK_F64>{});
  return f(int_tag<WK_NONE>{});
}

struct CalColumns {
  const void* vis = nullptr;
  int vis_dtype = CIP_C64;
  const void* model = nullptr;
  int model_dtype = CIP_C64;
  const void* wgt = nullptr;
  int wgt_dtype = CIP_F32;
};

template <int MODE>
hipError_t launch_correlate(const CalColumns& c, const CalRows& a, const CalBounds& b, int64_t* corr,
                            unsigned long long* out4, hipStream_t s) {
  return dispatch_cplx(c.vis_dtype, [&](auto vt) {
    return dispatch_cplx(c.model_dtype, [&](auto mt) {
      return dispatch_bool(c.wgt_dtype == CIP_F64, [&](auto wide) {
        using VC = typename decltype(vt)::type;
        using MC = typename decltype(mt)::type;
        constexpr int kWk = decltype(wide)::value ? WK_F64 : WK_F32;
        const int64_t nblk = cal_row_blocks(a);
        cal_correlate_kernel<VC, MC, kWk, MODE><<<dim3((unsigned)std::min<int64_t>(nblk, kCalMaxBlocks)),
                                                  dim3(kCalThreads), 0, s>>>(
            (const VC*)c.vis, (const MC*)c.model, c.wgt, a, b, nblk, (unsigned long long*)corr, out4);
        return hipGetLastError();
      });
    });
  });
}

hipError_t launch_apply(const void* vis, int vis_dtype, const void* wgt, int wgt_dtype, const CalRows& a,
                        const double* gains, const uint8_t* ant_ok, int mode, void* vis_out, void* wgt_out,
                        hipStream_t s) {
  return dispatch_cplx(vis_dtype, [&](auto vt) {
    return dispatch_real(wgt_dtype, [&](auto wk) {
      using VC = typename decltype(vt)::type;
      cal_apply_kernel<VC, decltype(wk)::value><<<cal_grid(a), dim3(kCalThreads), 0, s>>>(
          (const VC*)vis, wgt, a, (const double2*)gains, ant_ok, mode, (VC*)vis_out, wgt_out);
      return hipGetLastError();
    });
  });
}

// ------------------------------------------------------------ host API ----

int scale_init_impl(int64_t n_ant, int64_t n_int, double amax, double wmax, int64_t nsamp_max, cip_cal_scale* out) {
  const char* who = "cip_cal_scale_init";
  const std::string w(who);
  if (!out) return set_error(CIP_EINVAL, w + ": scale_out must not be NULL");
  if (n_ant < 2 || n_ant > CIP_CAL_MAX_ANT)
    return set_error(CIP_EINVAL, w + ": n_ant must be in 2 .. " + std::to_string(CIP_CAL_MAX_ANT));
  if (n_int < 1 || n_int > INT32_MAX) return set_error(CIP_EINVAL, w + ": n_int must be in 1 .. 2^31 - 1");
  if (!std::isfinite(amax) || !(amax > 0.0)) return set_error(CIP_EINVAL, w + ": amax must be finite and > 0");
  if (!std::isfinite(wmax) || !(wmax > 0.0)) return set_error(CIP_EINVAL, w + ": wmax must be finite and > 0");
  if (nsamp_max < 1) return set_error(CIP_EINVAL, w + ": nsamp_max must be >= 1");
  const double x = ((2.0 * wmax) * amax) * amax;
  if (!std::isfinite(x) || !(x > 0.0))
    return set_error(CIP_EINVAL, w + ": amax and wmax are too extreme for a normal fp64 quantum");
  int b = 0;
  while (b < 63 && ((int64_t)1 << b) < nsamp_max) ++b;
  int e = 0;
  (void)std::frexp(x, &e);  // x = m 2^e with 0.5 <= m < 1: e is the least integer with x < 2^e
  const int shift = 61 - b - e;
  if (shift < -1000 || shift > 1000)
    return set_error(CIP_EINVAL, w + ": amax and wmax are too extreme for a normal fp64 quantum");
  out->n_ant = n_ant;
  out->n_int = n_int;
  out->amax = amax;
  out->wmax = wmax;
  out->quantum = std::ldexp(1.0, -shift);
  out->shift = shift;
  out->reserved = 0;
  return CIP_OK;
}

// a caller's scale is plain host memory: refuse one cip_cal_scale_init did not fill
int scale_check(const char* who, const cip_cal_scale* sc) {
  const std::string w(who);
  if (!sc) return set_error(CIP_EINVAL, w + ": scale must not be NULL");
  if (sc->n_ant < 2 || sc->n_ant > CIP_CAL_MAX_ANT || sc->n_int < 1 || sc->n_int > INT32_MAX || sc->shift < -1000 ||
      sc->shift > 1000 || sc->quantum != std::ldexp(1.0, -sc->shift) || !(sc->amax > 0.0) || !(sc->wmax > 0.0) ||
      !std::isfinite(sc->amax) || !std::isfinite(sc->wmax))
    return set_error(CIP_EINVAL, w + ": scale was not filled by cip_cal_scale_init");
  return CIP_OK;
}

bool cplx_code(int d) { return d == CIP_C64 || d == CIP_C128; }
bool real_code(int d) { return d == CIP_F32 || d == CIP_F64; }

// the shape and the row columns every walk takes
int rows_check(const char* who, int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2,
               const int32_t* interval) {
  const std::string w(who);
  if (nrow < 0) return set_error(CIP_EINVAL, w + ": nrow must be >= 0");
  if (nchan < 1 || nchan > 65535) return set_error(CIP_EINVAL, w + ": nchan must be in 1 .. 65535");
  if (nrow > 0 && (!ant1 || !ant2 || !interval))
    return set_error(CIP_EINVAL, w + ": ant1, ant2 and interval must not be NULL");
  // fewer than 2^31 workgroups of kCalThreads / L rows
  if (nrow > (((int64_t)1 << 31) - 1) * (kCalThreads / cal_lanes((int)nchan)))
    return set_error(CIP_EINVAL, w + ": too many rows for one call (split the rows)");
  return CIP_OK;
}

int columns_check(const char* who, const CalColumns& c, int64_t nrow) {
  const std::string w(who);
  if (!cplx_code(c.vis_dtype) || !cplx_code(c.model_dtype))
    return set_error(CIP_EINVAL, w + ": vis_dtype and model_dtype must be CIP_C64 or CIP_C128");
  if (!real_code(c.wgt_dtype)) return set_error(CIP_EINVAL, w + ": wgt_dtype must be CIP_F32 or CIP_F64");
  if (nrow > 0 && (!c.vis || !c.model || !c.wgt))
    return set_error(CIP_EINVAL, w + ": vis, model and wgt must not be NULL");
  return CIP_OK;
}

int solve_check(const char* who, int64_t n_ant, int64_t niter, double tol, int64_t refant, int flags,
                const double* gains, const uint8_t* ant_ok) {
  const std::string w(who);
  if (niter < 0) return set_error(CIP_EINVAL, w + ": niter must be >= 0");
  if (!std::isfinite(tol) || tol < 0.0) return set_error(CIP_EINVAL, w + ": tol must be finite and >= 0");
  if (refant >= n_ant) return set_error(CIP_EINVAL, w + ": refant must be < n_ant (negative: no rotation)");
  if (flags & ~CIP_CAL_PHASE_ONLY) return set_error(CIP_EINVAL, w + ": unknown flags");
  if (!gains || !ant_ok) return set_error(CIP_EINVAL, w + ": gains_io and ant_ok_out must not be NULL");
  return CIP_OK;
}

CalRows make_rows(int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2, const int32_t* interval,
                  int64_t n_ant, int64_t n_int, bool vec) {
  CalRows a;
  a.ant1 = ant1;
  a.ant2 = ant2;
  a.interval = interval;
  a.nrow = nrow;
  a.nchan = (int)nchan;
  a.lanes = cal_lanes((int)nchan);
  a.n_ant = (int)n_ant;
  a.n_int = (int)n_int;
  a.vec = vec && nchan % kCalRun == 0;
  return a;
}

// Waits for the stream once.
int correlate_run(Workspace* ws, hipStream_t s, const CalColumns& c, const CalRows& a, const cip_cal_scale& sc,
                  int64_t* corr, cip_cal_counts* counts_out) {
  CIP_ALLOC(counts, unsigned long long, "cal_counts", 4)
  CIP_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), s));
  const CalBounds b = {sc.amax, sc.wmax, sc.shift};
  CIP_HIP_CHECK(launch_correlate<CAL_ADD>(c, a, b, corr, counts, s));
  int64_t* host = nullptr;
  if (const int rc = readback(ws, s, {{counts, 4 * sizeof(int64_t)}}, &host); rc != CIP_OK) return rc;
  if (counts_out) *counts_out = {host[0], host[1], host[2], host[3]};
  return CIP_OK;
}

int solve_run(Workspace* ws, hipStream_t s, const int64_t* corr, const cip_cal_scale& sc, int64_t niter, double tol,
              int64_t refant, int flags, double* gains, uint8_t* ant_ok, int64_t* iters_out,
              cip_cal_solve_info* info_out) {
  const int64_t n = sc.n_ant, total = sc.n_int * n * n;
  if ((total + kCalThreads - 1) / kCalThreads > (((int64_t)1 << 31) - 1))
    return set_error(CIP_EINVAL, "cip_cal_solve: n_int n_ant^2 is too large for one call");
  CIP_ALLOC(ar, double, "cal_a_re", total)
  CIP_ALLOC(ai, double, "cal_a_im", total)
  CIP_ALLOC(bb, double, "cal_b", total)
  CIP_ALLOC(stat, SolveStat, "cal_stat", sc.n_int)
  cal_expand_kernel<<<dim3((unsigned)((total + kCalThreads - 1) / kCalThreads)), dim3(kCalThreads), 0, s>>>(
      (const long long*)corr, total, (int)n, sc.quantum, ar, ai, bb);
  CIP_HIP_CHECK(hipGetLastError());
  const unsigned threads = (unsigned)((n + 63) / 64 * 64);
  cal_solve_kernel<<<dim3((unsigned)sc.n_int), dim3(threads), 0, s>>>(
      ar, ai, bb, (int)n, (long long)niter, tol * tol, (int)refant, (flags & CIP_CAL_PHASE_ONLY) ? 1 : 0,
      (double2*)gains, ant_ok, (long long*)iters_out, stat);
  CIP_HIP_CHECK(hipGetLastError());
  SolveStat* host = nullptr;
  if (const int rc = readback(ws, s, {{stat, (size_t)sc.n_int * sizeof(SolveStat)}}, &host); rc != CIP_OK) return rc;
  cip_cal_solve_info info = {0, 0, 0, 0, 0.0};
  for (int64_t i = 0; i < sc.n_int; ++i) {
    const SolveStat& st = host[i];
    info.n_converged += st.converged != 0;
    info.n_dead += st.n_dead;
    info.max_iter_done = std::max<int64_t>(info.max_iter_done, st.iters);
    info.ref_missing += st.ref_missing;
    if (st.iters > 0 && st.n2 > 0.0) {
      const double change = std::sqrt(st.d2 / st.n2);
      if (change > info.max_change) info.max_change = change;
    }
  }
  if (info_out) *info_out = info;
  return CIP_OK;
}

int correlate_impl(const CalColumns& c, int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2,
                   const int32_t* interval, const cip_cal_scale* sc, void* hip_stream, int64_t* corr,
                   cip_cal_counts* counts_out) {
  const char* who = "cip_cal_correlate";
  if (const int rc = scale_check(who, sc); rc != CIP_OK) return rc;
  if (const int rc = rows_check(who, nrow, nchan, ant1, ant2, interval); rc != CIP_OK) return rc;
  if (const int rc = columns_check(who, c, nrow); rc != CIP_OK) return rc;
  if (counts_out) *counts_out = {0, 0, 0, 0};
  if (nrow == 0) return CIP_OK;
  if (!corr) return set_error(CIP_EINVAL, "cip_cal_correlate: corr_io must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  const CalRows a = make_rows(nrow, nchan, ant1, ant2, interval, sc->n_ant, sc->n_int,
                              aligned16(c.vis) && aligned16(c.model) && aligned16(c.wgt));
  return correlate_run(ws, s, c, a, *sc, corr, counts_out);
}

int solve_impl(const int64_t* corr, const cip_cal_scale* sc, int64_t niter, double tol, int64_t refant, int flags,
               void* hip_stream, double* gains, uint8_t* ant_ok, int64_t* iters_out, cip_cal_solve_info* info_out) {
  const char* who = "cip_cal_solve";
  if (const int rc = scale_check(who, sc); rc != CIP_OK) return rc;
  if (const int rc = solve_check(who, sc->n_ant, niter, tol, refant, flags, gains, ant_ok); rc != CIP_OK) return rc;
  if (!corr) return set_error(CIP_EINVAL, "cip_cal_solve: corr must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  return solve_run(ws, s, corr, *sc, niter, tol, refant, flags, gains, ant_ok, iters_out, info_out);
}

int apply_impl(const void* vis, int vis_dtype, const void* wgt, int wgt_dtype, int64_t nrow, int64_t nchan,
               const int32_t* ant1, const int32_t* ant2, const int32_t* interval, const double* gains,
               const uint8_t* ant_ok, int64_t n_int, int64_t n_ant, int mode, void* hip_stream, void* vis_out,
               void* wgt_out) {
  const char* who = "cip_cal_apply";
  const std::string w(who);
  if (n_ant < 2 || n_ant > CIP_CAL_MAX_ANT)
    return set_error(CIP_EINVAL, w + ": n_ant must be in 2 .. " + std::to_string(CIP_CAL_MAX_ANT));
  if (n_int < 1 || n_int > INT32_MAX) return set_error(CIP_EINVAL, w + ": n_int must be in 1 .. 2^31 - 1");
  if (mode != CIP_CAL_CORRECT && mode != CIP_CAL_CORRUPT)
    return set_error(CIP_EINVAL, w + ": mode must be CIP_CAL_CORRECT or CIP_CAL_CORRUPT");
  if (const int rc = rows_check(who, nrow, nchan, ant1, ant2, interval); rc != CIP_OK) return rc;
  if (!cplx_code(vis_dtype)) return set_error(CIP_EINVAL, w + ": vis_dtype must be CIP_C64 or CIP_C128");
  if (wgt_dtype != CIP_NONE && !real_code(wgt_dtype))
    return set_error(CIP_EINVAL, w + ": wgt_dtype must be CIP_NONE, CIP_F32 or CIP_F64");
  if (nrow > 0 && ((wgt == nullptr) != (wgt_dtype == CIP_NONE) || (wgt == nullptr) != (wgt_out == nullptr)))
    return set_error(CIP_EINVAL, w + ": wgt and wgt_out are both NULL (with CIP_NONE) or both set");
  if (nrow > 0 && (!vis || !vis_out)) return set_error(CIP_EINVAL, w + ": vis and vis_out must not be NULL");
  if (nrow > 0 && (!gains || !ant_ok)) return set_error(CIP_EINVAL, w + ": gains and ant_ok must not be NULL");
  if (nrow == 0) return CIP_OK;
  CIP_BEGIN_CALL(hip_stream, false)
  const CalRows a = make_rows(nrow, nchan, ant1, ant2, interval, n_ant, n_int,
                              aligned16(vis) && aligned16(vis_out) && aligned16(wgt) && aligned16(wgt_out));
  CIP_HIP_CHECK(launch_apply(vis, vis_dtype, wgt, wgt_dtype, a, gains, ant_ok, mode, vis_out, wgt_out, s));
  return CIP_OK;
}

int gaincal_impl(const CalColumns& c, int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2,
                 const int32_t* interval, int64_t n_ant, int64_t n_int, int64_t niter, double tol, int64_t refant,
                 int flags, void* hip_stream, double* gains, uint8_t* ant_ok, int64_t* iters_out,
                 cip_cal_scale* scale_out, cip_cal_counts* counts_out, cip_cal_solve_info* info_out) {
  const char* who = "cip_gaincal";
  cip_cal_scale sc;
  // the shape checks with provisional bounds; the scale proper follows the max pass
  if (const int rc = scale_init_impl(n_ant, n_int, 1.0, 1.0, 1, &sc); rc != CIP_OK) return rc;
  if (const int rc = rows_check(who, nrow, nchan, ant1, ant2, interval); rc != CIP_OK) return rc;
  if (const int rc = columns_check(who, c, nrow); rc != CIP_OK) return rc;
  if (const int rc = solve_check(who, n_ant, niter, tol, refant, flags, gains, ant_ok); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, false)
  const CalRows a = make_rows(nrow, nchan, ant1, ant2, interval, n_ant, n_int,
                              aligned16(c.vis) && aligned16(c.model) && aligned16(c.wgt));
  double amax = 0.0, wmax = 0.0;
  if (nrow > 0) {
    CIP_ALLOC(mx, unsigned long long, "cal_max", 2)
    CIP_HIP_CHECK(hipMemsetAsync(mx, 0, 2 * sizeof(unsigned long long), s));
    CIP_HIP_CHECK(launch_correlate<CAL_MAX>(c, a, CalBounds{0.0, 0.0, 0}, nullptr, mx, s));
    int64_t* host = nullptr;
    if (const int rc = readback(ws, s, {{mx, 2 * sizeof(int64_t)}}, &host); rc != CIP_OK) return rc;
    std::memcpy(&amax, &host[0], sizeof(double));
    std::memcpy(&wmax, &host[1], sizeof(double));
  }
  if (!(amax > 0.0)) amax = 1.0;
  if (!(wmax > 0.0)) wmax = 1.0;
  if (const int rc = scale_init_impl(n_ant, n_int, amax, wmax, std::max<int64_t>(nrow * nchan, 1), &sc);
      rc != CIP_OK)
    return rc;
  if (scale_out) *scale_out = sc;
  const int64_t ncorr = n_int * n_ant * n_ant * 3;
  CIP_ALLOC(corr, int64_t, "cal_corr", ncorr)
  CIP_HIP_CHECK(hipMemsetAsync(corr, 0, (size_t)ncorr * sizeof(int64_t), s));
  if (counts_out) *counts_out = {0, 0, 0, 0};
  if (nrow > 0)
    if (const int rc = correlate_run(ws, s, c, a, sc, corr, counts_out); rc != CIP_OK) return rc;
  return solve_run(ws, s, corr, sc, niter, tol, refant, flags, gains, ant_ok, iters_out, info_out);
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_cal_scale_init(int64_t n_ant, int64_t n_int, double amax, double wmax, int64_t nsamp_max,
                       cip_cal_scale* scale_out) {
  clear_error();
  return scale_init_impl(n_ant, n_int, amax, wmax, nsamp_max, scale_out);
}

int cip_cal_correlate(const void* vis, int vis_dtype, const void* model, int model_dtype, const void* wgt,
                      int wgt_dtype, int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2,
                      const int32_t* interval, const cip_cal_scale* scale, void* hip_stream, int64_t* corr_io,
                      cip_cal_counts* counts_out) {
  clear_error();
  return correlate_impl(CalColumns{vis, vis_dtype, model, model_dtype, wgt, wgt_dtype}, nrow, nchan, ant1, ant2,
                        interval, scale, hip_stream, corr_io, counts_out);
}

int cip_cal_solve(const int64_t* corr, const cip_cal_scale* scale, int64_t niter, double tol, int64_t refant,
                  int flags, void* hip_stream, double* gains_io, uint8_t* ant_ok_out, int64_t* iters_out,
                  cip_cal_solve_info* info_out) {
  clear_error();
  return solve_impl(corr, scale, niter, tol, refant, flags, hip_stream, gains_io, ant_ok_out, iters_out, info_out);
}

int cip_cal_apply(const void* vis, int vis_dtype, const void* wgt, int wgt_dtype, int64_t nrow, int64_t nchan,
                  const int32_t* ant1, const int32_t* ant2, const int32_t* interval, const double* gains,
                  const uint8_t* ant_ok, int64_t n_int, int64_t n_ant, int mode, void* hip_stream, void* vis_out,
                  void* wgt_out) {
  clear_error();
  return apply_impl(vis, vis_dtype, wgt, wgt_dtype, nrow, nchan, ant1, ant2, interval, gains, ant_ok, n_int, n_ant,
                    mode, hip_stream, vis_out, wgt_out);
}

int cip_gaincal(const void* vis, int vis_dtype, const void* model, int model_dtype, const void* wgt, int wgt_dtype,
                int64_t nrow, int64_t nchan, const int32_t* ant1, const int32_t* ant2, const int32_t* interval,
                int64_t n_ant, int64_t n_int, int64_t niter, double tol, int64_t refant, int flags, void* hip_stream,
                double* gains_io, uint8_t* ant_ok_out, int64_t* iters_out, cip_cal_scale* scale_out,
                cip_cal_counts* counts_out, cip_cal_solve_info* info_out) {
  clear_error();
  return gaincal_impl(CalColumns{vis, vis_dtype, model, model_dtype, wgt, wgt_dtype}, nrow, nchan, ant1, ant2,
                      interval, n_ant, n_int, niter, tol, refant, flags, hip_stream, gains_io, ant_ok_out, iters_out,
                      scale_out, counts_out, info_out);
}

}  // extern "C"
