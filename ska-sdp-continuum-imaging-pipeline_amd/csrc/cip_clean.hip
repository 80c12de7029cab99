// cip_clean.hip - the CLEAN minor cycle on the device: the joint cycle of
// multi-term MFS over T coupled images (cip_mfs_clean, include/cip_mfs.h,
// DESIGN.md 15) and Hogbom CLEAN, its one-term case with hinv = {1.0}
// (cip_hogbom_clean, include/cip.h).
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
// Rounding is part of the definition (cip.h, cip_mfs.h): every product, sum
// and difference is one rounded fp64 operation, never an FMA, so a run is
// bit-identical to the numpy statement res[win] -= f * psf[win'].
#include <algorithm>
#include <cmath>
#include <string>

#include "cip_host.h"
#include "cip_mfs.h"
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

// device state of one call: the select kernel writes it, the subtract kernel
// reads the peak and f, the host reads it back once per batch
struct CleanState {
  int64_t k;                    // components written so far
  int64_t pi, pj;               // the peak the next subtract is centred on
  double f[CIP_MFS_MAX_TERMS];  // gain * c_q of that component
  int32_t stopped;              // nonzero: every queued kernel returns at once
  int32_t reason;               // CIP_CLEAN_* once stopped
  double peak;                  // signed s at the stopping peak (0 if EMPTY)
  int64_t peak_index;           // its flat index (-1 if EMPTY)
};

// what the three kernels share, by value
struct CleanArgs {
  double* res;  // (T, nx, ny)
  int64_t nx, ny, nty;
  const double* psf;  // (2T - 1, px, py)
  int64_t px, py, cx, cy;
  const uint8_t* mask;
  CleanEntry* table;
  CleanState* state;
  double hinv[CIP_MFS_MAX_TERMS * CIP_MFS_MAX_TERMS];  // row-major T x T
};

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

// row q of hinv times (r_0 .. r_{T-1}): hinv[q][0] r_0, then + hinv[q][t] r_t in order
template <int T>
__device__ __forceinline__ double solve_row(const double* __restrict__ hrow, const double (&r)[T]) {
  double s = mul_rounded(hrow[0], r[0]);
#pragma unroll
  for (int t = 1; t < T; ++t) s = add_rounded(s, mul_rounded(hrow[t], r[t]));
  return s;
}

// One tile (tx, ty) by one workgroup: with SUB, r_t -= f_q * psf_{t+q} on the
// pixels inside the PSF window around the peak (oi = i* - cx, oj = j* - cy);
// then the tile's table entry over all of its pixels.
template <int T, bool SUB>
__device__ __forceinline__ void tile_pass(const CleanArgs& a, int64_t tx, int64_t ty, int64_t oi, int64_t oj,
                                          const double (&f)[T]) {
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
        double p0[2 * T - 1], p1[2 * T - 1];
#pragma unroll
        for (int k = 0; k < 2 * T - 1; ++k) {
          p0[k] = in0 ? prow[k * pplane] : 0.0;
          p1[k] = in1 ? prow[k * pplane + 1] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
#pragma unroll
          for (int q = 0; q < T; ++q) {
            if (in0) v0[t] = sub_rounded(v0[t], f[q], p0[t + q]);
            if (in1) v1[t] = sub_rounded(v1[t], f[q], p1[t + q]);
          }
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
    if (m0) cand_take(best, fabs(solve_row<T>(a.hinv, v0)), idx);
    if (m1) cand_take(best, fabs(solve_row<T>(a.hinv, v1)), idx + 1);
  }
  best = block_best<kWaves>(best);
  if (threadIdx.x == 0) {
    CleanEntry e;
    e.absmax = best.a;
    e.index = best.idx == INT64_MAX ? (int64_t)-1 : best.idx;
    a.table[tx * a.nty + ty] = e;
  }
}

template <int T>
__global__ __launch_bounds__(kThreads) void clean_init_kernel(CleanArgs a) {
  const int64_t t = blockIdx.x;
  const double f[T] = {};
  tile_pass<T, false>(a, t / a.nty, t % a.nty, 0, 0, f);
}

// grid: gx * gy workgroups, sized by the host from the PSF and image shapes
// alone; workgroup (bx, by) takes the tile (first tile row of the window + bx,
// first tile column + by) and leaves when that tile does not meet the window
template <int T>
__global__ __launch_bounds__(kThreads) void clean_subtract_kernel(CleanArgs a, int64_t gy) {
  const CleanState* state = a.state;
  if (state->stopped) return;
  const int64_t oi = state->pi - a.cx, oj = state->pj - a.cy;
  double f[T];
#pragma unroll
  for (int q = 0; q < T; ++q) f[q] = state->f[q];
  // the window in image coordinates (never empty: 0 <= c < p and 0 <= peak < n)
  const int64_t i_lo = oi > 0 ? oi : 0, i_hi = oi + a.px < a.nx ? oi + a.px : a.nx;
  const int64_t j_lo = oj > 0 ? oj : 0, j_hi = oj + a.py < a.ny ? oj + a.py : a.ny;
  const int64_t bx = (int64_t)blockIdx.x / gy, by = (int64_t)blockIdx.x % gy;
  const int64_t tx = i_lo / kTX + bx, ty = j_lo / kTY + by;
  if (tx * kTX >= i_hi || ty * kTY >= j_hi) return;
  tile_pass<T, true>(a, tx, ty, oi, oj, f);
}

// model, comp_index / comp_flux may be NULL
template <int T>
__global__ __launch_bounds__(kSelectThreads) void clean_select_kernel(CleanArgs a, int64_t ntiles, double gain,
                                                                     double threshold, int64_t niter, double* model,
                                                                     int64_t* comp_index, double* comp_flux) {
  CleanState* state = a.state;
  if (state->stopped) return;
  Cand best = cand_none();
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
  if (threadIdx.x != 0) return;
  const int64_t k = state->k;
  if (best.idx == INT64_MAX) {
    state->stopped = 1;
    state->reason = CIP_CLEAN_EMPTY;
    state->peak = 0.0;
    state->peak_index = -1;
    return;
  }
  const int64_t plane = a.nx * a.ny;
  double r[T], c[T];
#pragma unroll
  for (int t = 0; t < T; ++t) r[t] = a.res[t * plane + best.idx];
#pragma unroll
  for (int q = 0; q < T; ++q) c[q] = solve_row<T>(a.hinv + q * T, r);
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

// ---- launchers: nterms -> T through the typed dispatch ----
// zeroes the state and builds the table from res under mask (may be NULL)
hipError_t launch_init(int64_t nterms, const CleanArgs& a, hipStream_t s) {
  hipError_t e = hipMemsetAsync(a.state, 0, sizeof(CleanState), s);
  if (e != hipSuccess) return e;
  return dispatch_int(CleanTerms{}, nterms, hipErrorInvalidValue, [&](auto t) {
    clean_init_kernel<decltype(t)::value><<<dim3((unsigned)clean_tiles(a.nx, a.ny)), dim3(kThreads), 0, s>>>(a);
    return hipGetLastError();
  });
}

hipError_t launch_subtract(int64_t nterms, const CleanArgs& a, hipStream_t s) {
  // the tiles a px x py window can meet: its extent plus one tile of slack per
  // axis for a window that does not start on a tile edge, never more than the
  // image has (the host does not know the peak)
  const int64_t ntx = (a.nx + kTX - 1) / kTX, nty = a.nty;
  const int64_t gx = std::min<int64_t>(ntx, (std::min(a.px, a.nx) + kTX - 1) / kTX + 1);
  const int64_t gy = std::min<int64_t>(nty, (std::min(a.py, a.ny) + kTY - 1) / kTY + 1);
  return dispatch_int(CleanTerms{}, nterms, hipErrorInvalidValue, [&](auto t) {
    clean_subtract_kernel<decltype(t)::value><<<dim3((unsigned)(gx * gy)), dim3(kThreads), 0, s>>>(a, gy);
    return hipGetLastError();
  });
}

hipError_t launch_select(int64_t nterms, const CleanArgs& a, double gain, double threshold, int64_t niter,
                         double* model, int64_t* comp_index, double* comp_flux, hipStream_t s) {
  return dispatch_int(CleanTerms{}, nterms, hipErrorInvalidValue, [&](auto t) {
    clean_select_kernel<decltype(t)::value><<<dim3(1), dim3(kSelectThreads), 0, s>>>(
        a, clean_tiles(a.nx, a.ny), gain, threshold, niter, model, comp_index, comp_flux);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------ host API ----
// Both entry points; `entry` is the name their messages carry. init builds the
// tile table, then select and (subtract, select) pairs are queued `batch`
// iterations at a time; the device state is read back once per batch. Kernels
// queued behind a stop return at once, so the result does not depend on `batch`.
int clean_impl(const char* entry, double* res, int64_t nterms, int64_t nx, int64_t ny, const double* psf,
               int64_t px, int64_t py, int64_t cx, int64_t cy, const double* hinv, const uint8_t* mask, double gain,
               double threshold, int64_t niter, int64_t batch, void* hip_stream, double* model, int64_t* comp_index,
               double* comp_flux, cip_clean_result* result_out) {
  const auto fail = [entry](int code, const char* what) { return set_error(code, std::string(entry) + ": " + what); };
  if (!res || !psf) return fail(CIP_EINVAL, "residual_io and psf must not be NULL");
  // cip_hogbom_clean passes nterms = 1 and a finite hinv: these three are cip_mfs_clean's alone
  if (nterms < 1 || nterms > CIP_MFS_MAX_TERMS) return fail(CIP_EINVAL, "nterms must be 1 .. CIP_MFS_MAX_TERMS (3)");
  if (!hinv) return fail(CIP_EINVAL, "hinv must not be NULL");
  for (int64_t e = 0; e < nterms * nterms; ++e)
    if (!std::isfinite(hinv[e])) return fail(CIP_EINVAL, "every entry of hinv must be finite");
  if (nx < 1 || ny < 1 || px < 1 || py < 1) return fail(CIP_EINVAL, "image and PSF dimensions must be >= 1");
  if (cx == -1) cx = px / 2;
  if (cy == -1) cy = py / 2;
  if (cx < 0 || cx >= px || cy < 0 || cy >= py) return fail(CIP_EINVAL, "the PSF centre lies outside the PSF");
  if (!std::isfinite(gain) || !(gain > 0.0)) return fail(CIP_EINVAL, "gain must be finite and > 0");
  if (std::isnan(threshold) || threshold < 0.0) return fail(CIP_EINVAL, "threshold must be >= 0 and not NaN");
  if (niter < 0 || batch < 0) return fail(CIP_EINVAL, "niter and batch must be >= 0");
  if ((comp_index == nullptr) != (comp_flux == nullptr))
    return fail(CIP_EINVAL, "comp_index and comp_flux go together (both or neither)");
  // the largest plane offsets, (T - 1) nx ny and (2T - 2) px py, stay in int64
  if (nx > INT64_MAX / ny / nterms || px > INT64_MAX / py / (2 * nterms - 1))
    return fail(CIP_EINVAL, "image or PSF too large");
  const int64_t ntiles = clean_tiles(nx, ny);
  if (ntiles >= ((int64_t)1 << 31)) return fail(CIP_EINVAL, "image has 2^31 tiles or more");
  if (batch == 0) batch = CIP_CLEAN_DEFAULT_BATCH;
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(table, CleanEntry, "clean_table", ntiles)
  CIP_ALLOC(state, CleanState, "clean_state", 1)
  CleanState* h = (CleanState*)pinned(ws, sizeof(CleanState));
  if (!h) return CIP_ENOMEM;
  CleanArgs a{};
  a.res = res, a.nx = nx, a.ny = ny, a.nty = (ny + kTY - 1) / kTY;
  a.psf = psf, a.px = px, a.py = py, a.cx = cx, a.cy = cy;
  a.mask = mask, a.table = table, a.state = state;
  std::copy(hinv, hinv + nterms * nterms, a.hinv);
  const auto select = [&] { return launch_select(nterms, a, gain, threshold, niter, model, comp_index, comp_flux, s); };
  CIP_HIP_CHECK(launch_init(nterms, a, s));
  CIP_HIP_CHECK(select());
  for (int64_t queued = 0;;) {
    const int64_t n = std::min(batch, niter - queued);
    for (int64_t q = 0; q < n; ++q) {
      CIP_HIP_CHECK(launch_subtract(nterms, a, s));
      CIP_HIP_CHECK(select());
    }
    queued += n;
    CIP_HIP_CHECK(hipMemcpyAsync(h, state, sizeof(CleanState), hipMemcpyDeviceToHost, s));
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    if (h->stopped) break;
    // after niter pairs the last select saw k == niter and stopped
    if (queued >= niter) return fail(CIP_EHIP, "the device state did not stop");
  }
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
  return clean_impl("cip_hogbom_clean", residual_io, 1, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, &identity,
                    mask, gain, threshold, niter, batch, hip_stream, model_io, comp_index, comp_flux, result_out);
}

int cip_mfs_clean(double* residual_io, int64_t nterms, int64_t nx, int64_t ny, const double* psf, int64_t psf_nx,
                  int64_t psf_ny, int64_t psf_cx, int64_t psf_cy, const double* hinv, const uint8_t* mask, double gain,
                  double threshold, int64_t niter, int64_t batch, void* hip_stream, double* model_io,
                  int64_t* comp_index, double* comp_flux, cip_clean_result* result_out) {
  clear_error();
  return clean_impl("cip_mfs_clean", residual_io, nterms, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, hinv, mask,
                    gain, threshold, niter, batch, hip_stream, model_io, comp_index, comp_flux, result_out);
}

}  // extern "C"
