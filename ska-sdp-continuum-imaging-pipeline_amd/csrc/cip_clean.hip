// cip_clean.hip - the CLEAN minor cycles on the device: the joint cycle of
// multi-term MFS over T coupled images (cip_mfs_clean, include/cip_mfs.h,
// DESIGN.md 15), Hogbom CLEAN, its one-term case with hinv = {1.0}
// (cip_hogbom_clean, include/cip.h), and the multiscale cycle
// over S scale-smoothed images (cip_ms_clean, include/cip_ms.h).
// The tile pass, the table, the launches and the host loop are one; what the
// two cycles do to a pixel's values is a policy (MfsCycle, MsCycle). The text
// below describes the MFS cycle; the multiscale one follows it.
//
// The image is cut into fixed tiles of kCleanTileX rows x kCleanTileY columns
// (4096 pixels, every row segment contiguous). A table in the workspace holds
// each tile's (largest |s| under the mask, its flat index), where
// s = sum_t hinv[0][t] r_t is the principal solution at the reference
// frequency (T = 1, hinv = 1: the residual itself, 1.0 * r being exact). One
// iteration is two plain launches on the caller's stream, templated on T:
//   subtract: the workgroups whose tile meets the PSF window around the peak
//             (read from the device state) load the T residual values of each
//             pixel once, apply the T x T updates r_t -= f_q * psf_{t+q} from
//             the 2T - 1 PSF planes, store T values and recompute their tile's
//             entry over ALL of the tile's pixels; tiles outside the window
//             keep their entries.
//   select:   one workgroup reduces the table (wave shuffles, then LDS),
//             applies the stop rule, recomputes c_q = sum_t hinv[q][t] r_t at
//             the peak in the tile pass's operation order, writes the
//             component, updates the T models and stores the next
//             (i*, j*, f_0 .. f_{T-1}) in the state.
// The host never waits per iteration: once the state says stopped every queued
// kernel returns without touching memory, so the result does not depend on how
// many iterations the host queues between two readbacks.
//
// The multiscale cycle keeps S planes and S (S + 1) / 2 cross PSFs. Its tile
// pass scores v = select_weight[s] r_s for every plane of a pixel and the
// table's index field carries the key s nx ny + flat (lowest key wins ties:
// lowest scale, then lowest flat index); its subtract reads (s*, f) from the
// state and updates plane s with the one cross PSF tri(min(s, s*), max(s, s*)):
// S loads, S PSF loads and S stores per pixel.
//
// Rounding is part of the definition (cip.h, cip_mfs.h, cip_ms.h): every product, sum
// and difference is one rounded fp64 operation, never an FMA, so a run is
// bit-identical to the numpy statement res[win] -= f * psf[win'].
#include <algorithm>
#include <cmath>
#include <string>

#include "cip_host.h"
#include "cip_mfs.h"
#include "cip_ms.h"
#include "cip_rounded.h"

namespace cip {

namespace {

constexpr int kTX = kCleanTileX;  // tile rows
constexpr int kTY = kCleanTileY;  // tile columns
constexpr int kThreads = 1024;    // 16 waves: a wave covers one 128-column row as 64 column pairs
constexpr int kWaves = kThreads / 64;
constexpr int kSelectThreads = 1024;
constexpr int kSelectUnroll = 8;  // table entries one select thread loads before it compares
static_assert(kTY == 128 && kTX % kWaves == 0, "a wave covers one tile row as 64 column pairs");

using CleanTerms = IntList<1, 2, 3>;
static_assert(CIP_MFS_MAX_TERMS == 3, "CleanTerms and CleanState::f hold CIP_MFS_MAX_TERMS terms");
using CleanScales = IntList<1, 2, 3, 4, 5, 6>;
static_assert(CIP_MS_MAX_SCALES == 6, "CleanScales holds CIP_MS_MAX_SCALES scales");
// CleanArgs::coef: hinv (T x T), or select_weight at [s] and flux_scale at [CIP_MS_MAX_SCALES + s]
constexpr int kCoefs = 2 * CIP_MS_MAX_SCALES;
static_assert(kCoefs >= CIP_MFS_MAX_TERMS * CIP_MFS_MAX_TERMS, "coef holds either cycle's host array");

// device state of one call: the select kernel writes it, the subtract kernel
// reads the peak and f, the host reads it back once per batch
struct CleanState {
  int64_t k;                    // components written so far
  int64_t pi, pj;               // the peak the next subtract is centred on
  double f[CIP_MFS_MAX_TERMS];  // gain * c_q of that component (multiscale: f[0] alone)
  int32_t stopped;              // nonzero: every queued kernel returns at once
  int32_t reason;               // CIP_CLEAN_* once stopped
  double peak;                  // signed s at the stopping peak (0 if EMPTY)
  int64_t peak_index;           // its flat index (-1 if EMPTY)
  int64_t ps;                   // multiscale: the scale of the peak (-1 if EMPTY)
};

// what the three kernels share, by value
struct CleanArgs {
  double* res;  // (T, nx, ny); multiscale: (S, nx, ny)
  int64_t nx, ny, nty;
  const double* psf;  // (2T - 1, px, py); multiscale: (S (S + 1) / 2, px, py)
  int64_t px, py, cx, cy;
  const uint8_t* mask;
  CleanEntry* table;
  CleanState* state;
  double coef[kCoefs];  // hinv, row-major T x T; multiscale: select_weight, flux_scale
};

struct Cand {
  double a;     // |value|; -1: nothing selected yet
  int64_t idx;  // flat index; INT64_MAX: none
};

__device__ __forceinline__ Cand cand_none() { return {-1.0, INT64_MAX}; }

// `>` keeps NaN out (every comparison with it is false); ties go to the lower
// flat index (multiscale: the lower key), so any reduction order gives the same winner
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

// row q of hinv times (r_0 .. r_{T-1}): hinv[q][0] r_0, then + hinv[q][t] r_t in order
template <int T>
__device__ __forceinline__ double solve_row(const double* __restrict__ hrow, const double (&r)[T]) {
  double s = mul_rounded(hrow[0], r[0]);
#pragma unroll
  for (int t = 1; t < T; ++t) s = add_rounded(s, mul_rounded(hrow[t], r[t]));
  return s;
}

// ---- what a cycle does to the N values of one pixel ----
// N residual planes, NP PSF values per pixel (value k from plane psf_plane(k)),
// the update of the N values by the component read from the state, and the
// pixel's candidates for the tile's table entry.
template <int T>
struct MfsCycle {
  static constexpr int N = T, NP = 2 * T - 1;
  double f[T];
  __device__ __forceinline__ void load(const CleanState* state) {
#pragma unroll
    for (int q = 0; q < T; ++q) f[q] = state->f[q];
  }
  __device__ __forceinline__ int psf_plane(int k) const { return k; }
  // r_t -= f_q * psf_{t+q}, q = 0 .. T - 1 in order
  __device__ __forceinline__ void subtract(double (&v)[N], const double (&p)[NP]) const {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int q = 0; q < T; ++q) v[t] = sub_rounded(v[t], f[q], p[t + q]);
  }
  __device__ __forceinline__ void take(const CleanArgs& a, Cand& best, const double (&v)[N], int64_t idx) const {
    cand_take(best, fabs(solve_row<T>(a.coef, v)), idx);
  }
};

template <int S>
struct MsCycle {
  static constexpr int N = S, NP = S;
  double f;
  int sel;  // s*
  __device__ __forceinline__ void load(const CleanState* state) {
    f = state->f[0];
    sel = (int)state->ps;
  }
  // plane s takes the cross PSF of (s, s*): tri(min, max)
  __device__ __forceinline__ int psf_plane(int s) const {
    const int lo = s < sel ? s : sel, hi = s < sel ? sel : s;
    return lo * S - lo * (lo - 1) / 2 + (hi - lo);
  }
  __device__ __forceinline__ void subtract(double (&v)[N], const double (&p)[NP]) const {
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = sub_rounded(v[s], f, p[s]);
  }
  // one candidate per plane, under the key s nx ny + flat
  __device__ __forceinline__ void take(const CleanArgs& a, Cand& best, const double (&v)[N], int64_t idx) const {
    const int64_t plane = a.nx * a.ny;
#pragma unroll
    for (int s = 0; s < S; ++s) cand_take(best, fabs(mul_rounded(a.coef[s], v[s])), s * plane + idx);
  }
};

// One tile (tx, ty) by one workgroup: with SUB, the cycle's update on the
// pixels inside the PSF window around the peak (oi = i* - cx, oj = j* - cy);
// then the tile's table entry over all of its pixels.
template <typename Cycle, bool SUB>
__device__ __forceinline__ void tile_pass(const CleanArgs& a, int64_t tx, int64_t ty, int64_t oi, int64_t oj,
                                          const Cycle& cyc) {
  constexpr int T = Cycle::N, NP = Cycle::NP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nx = a.nx, ny = a.ny, px = a.px, py = a.py;
  const int64_t plane = nx * ny, pplane = px * py;
  double* __restrict__ res = a.res;
  const double* __restrict__ psf = a.psf;
  const uint8_t* __restrict__ mask = a.mask;
  const int64_t j = ty * kTY + 2 * lane;
  // 16-byte accesses where every row of every plane starts 16-byte aligned
  // (an even ny makes the plane stride even too)
  const bool vec = ((ny & 1) == 0) && (((uintptr_t)res & 15u) == 0u) && (j + 1 < ny);
  Cand best = cand_none();
#pragma unroll
  for (int r = 0; r < kTX / kWaves; ++r) {
    const int64_t i = tx * kTX + wave + kWaves * r;
    if (i >= nx || j >= ny) continue;
    const int64_t idx = i * ny + j;
    const bool two = j + 1 < ny;
    double v0[T], v1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const double* p = res + t * plane + idx;
      if (vec) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        v0[t] = v.x;
        v1[t] = v.y;
      } else {
        v0[t] = p[0];
        v1[t] = two ? p[1] : 0.0;
      }
    }
    if (SUB) {
      // PSF index of pixel (i, j): (i - oi, j - oj)
      const int64_t pr = i - oi, pc = j - oj;
      if (pr >= 0 && pr < px) {
        const bool in0 = pc >= 0 && pc < py;
        const bool in1 = two && pc + 1 >= 0 && pc + 1 < py;
        const double* prow = psf + pr * py + pc;
        double p0[NP], p1[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const int64_t off = cyc.psf_plane(k) * pplane;
          p0[k] = in0 ? prow[off] : 0.0;
          p1[k] = in1 ? prow[off + 1] : 0.0;
        }
        if (in0) cyc.subtract(v0, p0);
        if (in1) cyc.subtract(v1, p1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          double* p = res + t * plane + idx;
          if (vec && in0 && in1) {
            *reinterpret_cast<double2*>(p) = make_double2(v0[t], v1[t]);
          } else {
            if (in0) p[0] = v0[t];
            if (in1) p[1] = v1[t];
          }
        }
      }
    }
    const bool m0 = mask ? mask[idx] != 0 : true;
    const bool m1 = two && (mask ? mask[idx + 1] != 0 : true);
    if (m0) cyc.take(a, best, v0, idx);
    if (m1) cyc.take(a, best, v1, idx + 1);
  }
  best = block_best<kWaves>(best);
  if (threadIdx.x == 0) {
    CleanEntry e;
    e.absmax = best.a;
    e.index = best.idx == INT64_MAX ? (int64_t)-1 : best.idx;
    a.table[tx * a.nty + ty] = e;
  }
}

template <typename Cycle>
__global__ __launch_bounds__(kThreads) void clean_init_kernel(CleanArgs a) {
  const int64_t t = blockIdx.x;
  const Cycle cyc{};
  tile_pass<Cycle, false>(a, t / a.nty, t % a.nty, 0, 0, cyc);
}

// grid: gx * gy workgroups, sized by the host from the PSF and image shapes
// alone; workgroup (bx, by) takes the tile (first tile row of the window + bx,
// first tile column + by) and leaves when that tile does not meet the window
template <typename Cycle>
__global__ __launch_bounds__(kThreads) void clean_subtract_kernel(CleanArgs a, int64_t gy) {
  const CleanState* state = a.state;
  if (state->stopped) return;
  const int64_t oi = state->pi - a.cx, oj = state->pj - a.cy;
  Cycle cyc;
  cyc.load(state);
  // the window in image coordinates (never empty: 0 <= c < p and 0 <= peak < n)
  const int64_t i_lo = oi > 0 ? oi : 0, i_hi = oi + a.px < a.nx ? oi + a.px : a.nx;
  const int64_t j_lo = oj > 0 ? oj : 0, j_hi = oj + a.py < a.ny ? oj + a.py : a.ny;
  const int64_t bx = (int64_t)blockIdx.x / gy, by = (int64_t)blockIdx.x % gy;
  const int64_t tx = i_lo / kTX + bx, ty = j_lo / kTY + by;
  if (tx * kTX >= i_hi || ty * kTY >= j_hi) return;
  tile_pass<Cycle, true>(a, tx, ty, oi, oj, cyc);
}

// The table's best entry, in thread 0 of the select workgroup; false when the
// table has none (the stop EMPTY, written to the state) and in every other thread.
__device__ __forceinline__ bool table_best(const CleanArgs& a, int64_t ntiles, Cand& best) {
  best = cand_none();
  // one 16-byte load per entry, kSelectUnroll of them in flight per thread: a
  // single workgroup reads the whole table, so its time is load latency over
  // the loads it keeps outstanding
  for (int64_t base = threadIdx.x; base < ntiles; base += (int64_t)kSelectUnroll * kSelectThreads) {
    double2 raw[kSelectUnroll];
#pragma unroll
    for (int u = 0; u < kSelectUnroll; ++u) {
      const int64_t t = base + (int64_t)u * kSelectThreads;
      raw[u] = t < ntiles ? *reinterpret_cast<const double2*>(a.table + t) : make_double2(-1.0, __longlong_as_double(-1));
    }
#pragma unroll
    for (int u = 0; u < kSelectUnroll; ++u) {
      const int64_t idx = (int64_t)__double_as_longlong(raw[u].y);
      if (idx >= 0) cand_take(best, raw[u].x, idx);
    }
  }
  best = block_best<kSelectThreads / 64>(best);
  if (threadIdx.x != 0) return false;
  if (best.idx == INT64_MAX) {
    CleanState* state = a.state;
    state->stopped = 1;
    state->reason = CIP_CLEAN_EMPTY;
    state->peak = 0.0;
    state->peak_index = -1;
    state->ps = -1;
    return false;
  }
  return true;
}

// model, comp_index / comp_flux may be NULL
template <int T>
__global__ __launch_bounds__(kSelectThreads) void clean_select_kernel(CleanArgs a, int64_t ntiles, double gain,
                                                                     double threshold, int64_t niter, double* model,
                                                                     int64_t* comp_index, double* comp_flux) {
  CleanState* state = a.state;
  if (state->stopped) return;
  Cand best;
  if (!table_best(a, ntiles, best)) return;
  const int64_t k = state->k;
  const int64_t plane = a.nx * a.ny;
  double r[T], c[T];
#pragma unroll
  for (int t = 0; t < T; ++t) r[t] = a.res[t * plane + best.idx];
#pragma unroll
  for (int q = 0; q < T; ++q) c[q] = solve_row<T>(a.coef + q * T, r);
  // c[0] is the s the tile pass took |.| of: same operands, same order
  if (best.a <= threshold || k == niter) {
    state->stopped = 1;
    state->reason = best.a <= threshold ? CIP_CLEAN_THRESHOLD : CIP_CLEAN_NITER;
    state->peak = c[0];
    state->peak_index = best.idx;
    return;
  }
#pragma unroll
  for (int q = 0; q < T; ++q) {
    const double f = mul_rounded(gain, c[q]);
    if (model) model[q * plane + best.idx] = add_rounded(model[q * plane + best.idx], f);
    if (comp_index) comp_flux[k * T + q] = f;
    state->f[q] = f;
  }
  if (comp_index) comp_index[k] = best.idx;
  state->pi = best.idx / a.ny;
  state->pj = best.idx % a.ny;
  state->k = k + 1;
}

// The multiscale select: the winning key is s* nx ny + flat, which is also the
// offset of the peak in the residual and model stacks. model, comp_index /
// comp_scale / comp_flux may be NULL.
__global__ __launch_bounds__(kSelectThreads) void ms_select_kernel(CleanArgs a, int64_t ntiles, double gain,
                                                                  double threshold, int64_t niter, double* model,
                                                                  int64_t* comp_index, int64_t* comp_scale,
                                                                  double* comp_flux) {
  CleanState* state = a.state;
  if (state->stopped) return;
  Cand best;
  if (!table_best(a, ntiles, best)) return;
  const int64_t k = state->k;
  const int64_t plane = a.nx * a.ny;
  const int64_t sel = best.idx / plane, flat = best.idx % plane;
  const double r = a.res[best.idx];
  if (best.a <= threshold || k == niter) {
    state->stopped = 1;
    state->reason = best.a <= threshold ? CIP_CLEAN_THRESHOLD : CIP_CLEAN_NITER;
    state->peak = mul_rounded(a.coef[sel], r);  // the v the tile pass took |.| of
    state->peak_index = flat;
    state->ps = sel;
    return;
  }
  const double f = mul_rounded(gain, mul_rounded(a.coef[CIP_MS_MAX_SCALES + sel], r));
  if (model) model[best.idx] = add_rounded(model[best.idx], f);
  if (comp_index) {
    comp_index[k] = flat;
    comp_scale[k] = sel;
    comp_flux[k] = f;
  }
  state->f[0] = f;
  state->ps = sel;
  state->pi = flat / a.ny;
  state->pj = flat % a.ny;
  state->k = k + 1;
}

// ---- launchers: the cycle (multiscale or MFS) and its plane count n -> the
// policy type through the typed dispatch ----
template <typename F>
hipError_t with_cycle(bool ms, int64_t n, F&& f) {
  if (ms)
    return dispatch_int(CleanScales{}, n, hipErrorInvalidValue,
                        [&](auto t) { return f(type_tag<MsCycle<decltype(t)::value>>{}); });
  return dispatch_int(CleanTerms{}, n, hipErrorInvalidValue,
                      [&](auto t) { return f(type_tag<MfsCycle<decltype(t)::value>>{}); });
}

// zeroes the state and builds the table from res under mask (may be NULL)
hipError_t launch_init(bool ms, int64_t n, const CleanArgs& a, hipStream_t s) {
  hipError_t e = hipMemsetAsync(a.state, 0, sizeof(CleanState), s);
  if (e != hipSuccess) return e;
  return with_cycle(ms, n, [&](auto c) {
    using Cycle = typename decltype(c)::type;
    clean_init_kernel<Cycle><<<dim3((unsigned)clean_tiles(a.nx, a.ny)), dim3(kThreads), 0, s>>>(a);
    return hipGetLastError();
  });
}

hipError_t launch_subtract(bool ms, int64_t n, const CleanArgs& a, hipStream_t s) {
  // the tiles a px x py window can meet: its extent plus one tile of slack per
  // axis for a window that does not start on a tile edge, never more than the
  // image has (the host does not know the peak)
  const int64_t ntx = (a.nx + kTX - 1) / kTX, nty = a.nty;
  const int64_t gx = std::min<int64_t>(ntx, (std::min(a.px, a.nx) + kTX - 1) / kTX + 1);
  const int64_t gy = std::min<int64_t>(nty, (std::min(a.py, a.ny) + kTY - 1) / kTY + 1);
  return with_cycle(ms, n, [&](auto c) {
    using Cycle = typename decltype(c)::type;
    clean_subtract_kernel<Cycle><<<dim3((unsigned)(gx * gy)), dim3(kThreads), 0, s>>>(a, gy);
    return hipGetLastError();
  });
}

// comp_scale: the multiscale cycle's alone
hipError_t launch_select(bool ms, int64_t n, const CleanArgs& a, double gain, double threshold, int64_t niter,
                         double* model, int64_t* comp_index, int64_t* comp_scale, double* comp_flux, hipStream_t s) {
  if (ms) {
    ms_select_kernel<<<dim3(1), dim3(kSelectThreads), 0, s>>>(a, clean_tiles(a.nx, a.ny), gain, threshold, niter,
                                                              model, comp_index, comp_scale, comp_flux);
    return hipGetLastError();
  }
  return dispatch_int(CleanTerms{}, n, hipErrorInvalidValue, [&](auto t) {
    clean_select_kernel<decltype(t)::value><<<dim3(1), dim3(kSelectThreads), 0, s>>>(
        a, clean_tiles(a.nx, a.ny), gain, threshold, niter, model, comp_index, comp_flux);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------ host API ----
// what an entry point's cycle adds to the arguments the three share
struct CycleHost {
  bool ms;               // the multiscale cycle over n scales; else the MFS cycle over n terms
  int64_t n;
  const double* coef;    // HOST: hinv (n x n); multiscale: select_weight (n)
  const double* coef2;   // HOST, multiscale: flux_scale (n)
  int64_t* comp_scale;   // multiscale: goes with comp_index and comp_flux
};

// All three entry points; `entry` is the name their messages carry. init builds
// the tile table, then select and (subtract, select) pairs are queued `batch`
// iterations at a time; the device state is read back once per batch. Kernels
// queued behind a stop return at once, so the result does not depend on `batch`.
// Returns the final state in *final (readback()'s staging: read it before the next call).
int clean_impl(const char* entry, const CycleHost& cyc, double* res, int64_t nx, int64_t ny, const double* psf,
               int64_t px, int64_t py, int64_t cx, int64_t cy, const uint8_t* mask, double gain, double threshold,
               int64_t niter, int64_t batch, void* hip_stream, double* model, int64_t* comp_index, double* comp_flux,
               const CleanState** final) {
  const auto fail = [entry](int code, const char* what) { return set_error(code, std::string(entry) + ": " + what); };
  const bool ms = cyc.ms;
  const int64_t nterms = cyc.n;  // planes of the residual stack
  if (!res || !psf) return fail(CIP_EINVAL, "residual_io and psf must not be NULL");
  // cip_hogbom_clean passes nterms = 1 and a finite hinv: these are the other two's alone
  if (ms) {
    if (nterms < 1 || nterms > CIP_MS_MAX_SCALES) return fail(CIP_EINVAL, "nscales must be 1 .. CIP_MS_MAX_SCALES (6)");
    if (!cyc.coef || !cyc.coef2) return fail(CIP_EINVAL, "select_weight and flux_scale must not be NULL");
    for (int64_t e = 0; e < nterms; ++e)
      if (!std::isfinite(cyc.coef[e]) || !std::isfinite(cyc.coef2[e]))
        return fail(CIP_EINVAL, "every entry of select_weight and flux_scale must be finite");
  } else {
    if (nterms < 1 || nterms > CIP_MFS_MAX_TERMS) return fail(CIP_EINVAL, "nterms must be 1 .. CIP_MFS_MAX_TERMS (3)");
    if (!cyc.coef) return fail(CIP_EINVAL, "hinv must not be NULL");
    for (int64_t e = 0; e < nterms * nterms; ++e)
      if (!std::isfinite(cyc.coef[e])) return fail(CIP_EINVAL, "every entry of hinv must be finite");
  }
  if (nx < 1 || ny < 1 || px < 1 || py < 1) return fail(CIP_EINVAL, "image and PSF dimensions must be >= 1");
  if (cx == -1) cx = px / 2;
  if (cy == -1) cy = py / 2;
  if (cx < 0 || cx >= px || cy < 0 || cy >= py) return fail(CIP_EINVAL, "the PSF centre lies outside the PSF");
  if (!std::isfinite(gain) || !(gain > 0.0)) return fail(CIP_EINVAL, "gain must be finite and > 0");
  if (std::isnan(threshold) || threshold < 0.0) return fail(CIP_EINVAL, "threshold must be >= 0 and not NaN");
  if (niter < 0 || batch < 0) return fail(CIP_EINVAL, "niter and batch must be >= 0");
  if ((comp_index == nullptr) != (comp_flux == nullptr))
    return fail(CIP_EINVAL, "comp_index and comp_flux go together (both or neither)");
  if (ms && (comp_index == nullptr) != (cyc.comp_scale == nullptr))
    return fail(CIP_EINVAL, "comp_index, comp_scale and comp_flux go together (all three or none)");
  // the stacks' sizes (the multiscale key runs up to S nx ny) and so every plane offset stay in int64
  const int64_t npsf = ms ? nterms * (nterms + 1) / 2 : 2 * nterms - 1;
  if (nx > INT64_MAX / ny / nterms || px > INT64_MAX / py / npsf) return fail(CIP_EINVAL, "image or PSF too large");
  const int64_t ntiles = clean_tiles(nx, ny);
  if (ntiles >= ((int64_t)1 << 31)) return fail(CIP_EINVAL, "image has 2^31 tiles or more");
  if (batch == 0) batch = CIP_CLEAN_DEFAULT_BATCH;
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(table, CleanEntry, "clean_table", ntiles)
  CIP_ALLOC(state, CleanState, "clean_state", 1)
  CleanState* h = nullptr;
  CleanArgs a{};
  a.res = res, a.nx = nx, a.ny = ny, a.nty = (ny + kTY - 1) / kTY;
  a.psf = psf, a.px = px, a.py = py, a.cx = cx, a.cy = cy;
  a.mask = mask, a.table = table, a.state = state;
  if (ms) {
    std::copy(cyc.coef, cyc.coef + nterms, a.coef);
    std::copy(cyc.coef2, cyc.coef2 + nterms, a.coef + CIP_MS_MAX_SCALES);
  } else {
    std::copy(cyc.coef, cyc.coef + nterms * nterms, a.coef);
  }
  const auto select = [&] {
    return launch_select(ms, nterms, a, gain, threshold, niter, model, comp_index, cyc.comp_scale, comp_flux, s);
  };
  CIP_HIP_CHECK(launch_init(ms, nterms, a, s));
  CIP_HIP_CHECK(select());
  for (int64_t queued = 0;;) {
    const int64_t n = std::min(batch, niter - queued);
    for (int64_t q = 0; q < n; ++q) {
      CIP_HIP_CHECK(launch_subtract(ms, nterms, a, s));
      CIP_HIP_CHECK(select());
    }
    queued += n;
    if (const int rc = readback(ws, s, {{state, sizeof(CleanState)}}, &h); rc != CIP_OK) return rc;
    if (h->stopped) break;
    // after niter pairs the last select saw k == niter and stopped
    if (queued >= niter) return fail(CIP_EHIP, "the device state did not stop");
  }
  *final = h;
  return CIP_OK;
}

// cip_hogbom_clean and cip_mfs_clean
int mfs_clean_impl(const char* entry, double* res, int64_t nterms, int64_t nx, int64_t ny, const double* psf,
                   int64_t px, int64_t py, int64_t cx, int64_t cy, const double* hinv, const uint8_t* mask,
                   double gain, double threshold, int64_t niter, int64_t batch, void* hip_stream, double* model,
                   int64_t* comp_index, double* comp_flux, cip_clean_result* result_out) {
  const CleanState* h = nullptr;
  const CycleHost cyc{false, nterms, hinv, nullptr, nullptr};
  if (const int rc = clean_impl(entry, cyc, res, nx, ny, psf, px, py, cx, cy, mask, gain, threshold, niter, batch,
                                hip_stream, model, comp_index, comp_flux, &h);
      rc != CIP_OK)
    return rc;
  if (result_out) {
    result_out->niter_done = h->k;
    result_out->stop_reason = h->reason;
    result_out->reserved = 0;
    result_out->peak = h->peak;
    result_out->peak_index = h->peak_index;
  }
  return CIP_OK;
}

}  // namespace

int64_t clean_tiles(int64_t nx, int64_t ny) { return ((nx + kTX - 1) / kTX) * ((ny + kTY - 1) / kTY); }

}  // namespace cip

using namespace cip;

extern "C" {

// the one-term case: the image and the PSF are one-plane stacks, comp_flux (n) is (n, 1)
int cip_hogbom_clean(double* residual_io, int64_t nx, int64_t ny, const double* psf, int64_t psf_nx, int64_t psf_ny,
                     int64_t psf_cx, int64_t psf_cy, const uint8_t* mask, double gain, double threshold,
                     int64_t niter, int64_t batch, void* hip_stream, double* model_io, int64_t* comp_index,
                     double* comp_flux, cip_clean_result* result_out) {
  static const double identity = 1.0;
  clear_error();
  return mfs_clean_impl("cip_hogbom_clean", residual_io, 1, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, &identity,
                        mask, gain, threshold, niter, batch, hip_stream, model_io, comp_index, comp_flux, result_out);
}

int cip_mfs_clean(double* residual_io, int64_t nterms, int64_t nx, int64_t ny, const double* psf, int64_t psf_nx,
                  int64_t psf_ny, int64_t psf_cx, int64_t psf_cy, const double* hinv, const uint8_t* mask, double gain,
                  double threshold, int64_t niter, int64_t batch, void* hip_stream, double* model_io,
                  int64_t* comp_index, double* comp_flux, cip_clean_result* result_out) {
  clear_error();
  return mfs_clean_impl("cip_mfs_clean", residual_io, nterms, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, hinv, mask,
                        gain, threshold, niter, batch, hip_stream, model_io, comp_index, comp_flux, result_out);
}

int cip_ms_clean(double* residual_io, int64_t nscales, int64_t nx, int64_t ny, const double* psf, int64_t psf_nx,
                 int64_t psf_ny, int64_t psf_cx, int64_t psf_cy, const double* select_weight, const double* flux_scale,
                 const uint8_t* mask, double gain, double threshold, int64_t niter, int64_t batch, void* hip_stream,
                 double* model_io, int64_t* comp_index, int64_t* comp_scale, double* comp_flux,
                 cip_ms_result* result_out) {
  clear_error();
  const CleanState* h = nullptr;
  const CycleHost cyc{true, nscales, select_weight, flux_scale, comp_scale};
  if (const int rc = clean_impl("cip_ms_clean", cyc, residual_io, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, mask,
                                gain, threshold, niter, batch, hip_stream, model_io, comp_index, comp_flux, &h);
      rc != CIP_OK)
    return rc;
  if (result_out) {
    result_out->niter_done = h->k;
    result_out->stop_reason = h->reason;
    result_out->peak_scale = (int32_t)h->ps;
    result_out->peak = h->peak;
    result_out->peak_index = h->peak_index;
  }
  return CIP_OK;
}

}  // extern "C"
