// cip_clean.hip - Hogbom CLEAN minor cycle on the device (cip_hogbom_clean,
// DESIGN.md 12).
//
// The image is cut into fixed tiles of kCleanTileX rows x kCleanTileY columns
// (4096 pixels, every row segment contiguous). A table in the workspace holds
// each tile's (largest |res| under the mask, its flat index). One iteration is
// two plain launches on the caller's stream:
//   subtract: the workgroups whose tile meets the PSF window around the peak
//             (read from the device state) subtract f * psf from the window's
//             pixels and recompute their tile's table entry over ALL of the
//             tile's pixels; tiles outside the window keep their entries.
//   select:   one workgroup reduces the table (wave shuffles, then LDS),
//             applies the stop rule, writes the component, updates the model
//             and stores the next (i*, j*, f) in the state.
// The host never waits per iteration: once the state says stopped every queued
// kernel returns without touching memory, so the result does not depend on how
// many iterations the host queues between two readbacks.
//
// Rounding is part of the definition (cip.h): f = gain * peak, f * psf and
// res - (f * psf) are each one rounded fp64 operation, never an FMA, so the run
// is bit-identical to the numpy statement res[win] -= f * psf[win'].
#include <algorithm>

#include "cip_clean_util.h"
#include "cip_host.h"

namespace cip {

namespace {

constexpr int kTX = kCleanTileX;  // tile rows
constexpr int kTY = kCleanTileY;  // tile columns
constexpr int kThreads = 1024;    // 16 waves: a wave covers one 128-column row as 64 column pairs
constexpr int kWaves = kThreads / 64;
constexpr int kSelectThreads = 1024;
constexpr int kSelectUnroll = 8;  // table entries one select thread loads before it compares
static_assert(kTY == 128 && kTX % kWaves == 0, "a wave covers one tile row as 64 column pairs");

// One tile (tx, ty) by one workgroup: with SUB, res -= f * psf on the pixels
// inside the PSF window around (pi, pj); then the tile's table entry over all
// of its pixels.
template <bool SUB>
__device__ __forceinline__ void tile_pass(double* __restrict__ res, int64_t nx, int64_t ny, int64_t tx, int64_t ty,
                                          int64_t nty, const double* __restrict__ psf, int64_t px, int64_t py,
                                          int64_t oi, int64_t oj, double f, const uint8_t* __restrict__ mask,
                                          CleanEntry* __restrict__ table) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = ty * kTY + 2 * lane;
  // 16-byte accesses where every row of the image starts 16-byte aligned
  const bool vec = ((ny & 1) == 0) && (((uintptr_t)res & 15u) == 0u) && (j + 1 < ny);
  Cand best = cand_none();
#pragma unroll
  for (int r = 0; r < kTX / kWaves; ++r) {
    const int64_t i = tx * kTX + wave + kWaves * r;
    if (i >= nx || j >= ny) continue;
    const int64_t idx = i * ny + j;
    const bool two = j + 1 < ny;
    double v0, v1 = 0.0;
    if (vec) {
      const double2 v = *reinterpret_cast<const double2*>(res + idx);
      v0 = v.x;
      v1 = v.y;
    } else {
      v0 = res[idx];
      if (two) v1 = res[idx + 1];
    }
    if (SUB) {
      // PSF index of pixel (i, j): (i - oi, j - oj), oi = i* - cx, oj = j* - cy
      const int64_t pr = i - oi, pc = j - oj;
      if (pr >= 0 && pr < px) {
        const double* prow = psf + pr * py;
        const bool in0 = pc >= 0 && pc < py;
        const bool in1 = two && pc + 1 >= 0 && pc + 1 < py;
        if (in0) v0 = sub_rounded(v0, f, prow[pc]);
        if (in1) v1 = sub_rounded(v1, f, prow[pc + 1]);
        if (vec && in0 && in1) {
          *reinterpret_cast<double2*>(res + idx) = make_double2(v0, v1);
        } else {
          if (in0) res[idx] = v0;
          if (in1) res[idx + 1] = v1;
        }
      }
    }
    if (mask) {
      if (mask[idx]) cand_take(best, fabs(v0), idx);
      if (two && mask[idx + 1]) cand_take(best, fabs(v1), idx + 1);
    } else {
      cand_take(best, fabs(v0), idx);
      if (two) cand_take(best, fabs(v1), idx + 1);
    }
  }
  best = block_best<kWaves>(best);
  if (threadIdx.x == 0) {
    CleanEntry e;
    e.absmax = best.a;
    e.index = best.idx == INT64_MAX ? (int64_t)-1 : best.idx;
    table[tx * nty + ty] = e;
  }
}

__global__ __launch_bounds__(kThreads) void clean_init_kernel(double* res, int64_t nx, int64_t ny, int64_t nty,
                                                             const uint8_t* mask, CleanEntry* table) {
  const int64_t t = blockIdx.x;
  tile_pass<false>(res, nx, ny, t / nty, t % nty, nty, nullptr, 0, 0, 0, 0, 0.0, mask, table);
}

// grid: gx * gy workgroups, sized by the host from the PSF and image shapes
// alone; workgroup (bx, by) takes the tile (first tile row of the window + bx,
// first tile column + by) and leaves when that tile does not meet the window
__global__ __launch_bounds__(kThreads) void clean_subtract_kernel(double* res, int64_t nx, int64_t ny, int64_t nty,
                                                                 const double* psf, int64_t px, int64_t py,
                                                                 int64_t cx, int64_t cy, int64_t gy,
                                                                 const uint8_t* mask, CleanEntry* table,
                                                                 const CleanState* state) {
  if (state->stopped) return;
  const int64_t oi = state->pi - cx, oj = state->pj - cy;
  const double f = state->f;
  // the window in image coordinates (never empty: 0 <= c < p and 0 <= peak < n)
  const int64_t i_lo = oi > 0 ? oi : 0, i_hi = oi + px < nx ? oi + px : nx;
  const int64_t j_lo = oj > 0 ? oj : 0, j_hi = oj + py < ny ? oj + py : ny;
  const int64_t bx = (int64_t)blockIdx.x / gy, by = (int64_t)blockIdx.x % gy;
  const int64_t tx = i_lo / kTX + bx, ty = j_lo / kTY + by;
  if (tx * kTX >= i_hi || ty * kTY >= j_hi) return;
  tile_pass<true>(res, nx, ny, tx, ty, nty, psf, px, py, oi, oj, f, mask, table);
}

__global__ __launch_bounds__(kSelectThreads) void clean_select_kernel(const double* res, const CleanEntry* table,
                                                                     int64_t ntiles, double gain, double threshold,
                                                                     int64_t niter, int64_t ny, double* model,
                                                                     int64_t* comp_index, double* comp_flux,
                                                                     CleanState* state) {
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
      raw[u] = t < ntiles ? *reinterpret_cast<const double2*>(table + t) : make_double2(-1.0, __longlong_as_double(-1));
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
  const double peak = res[best.idx];
  if (best.a <= threshold || k == niter) {
    state->stopped = 1;
    state->reason = best.a <= threshold ? CIP_CLEAN_THRESHOLD : CIP_CLEAN_NITER;
    state->peak = peak;
    state->peak_index = best.idx;
    return;
  }
  const double f = mul_rounded(gain, peak);
  if (model) model[best.idx] = add_rounded(model[best.idx], f);
  if (comp_index) {
    comp_index[k] = best.idx;
    comp_flux[k] = f;
  }
  state->pi = best.idx / ny;
  state->pj = best.idx % ny;
  state->f = f;
  state->k = k + 1;
}

}  // namespace

int64_t clean_tiles(int64_t nx, int64_t ny) { return ((nx + kTX - 1) / kTX) * ((ny + kTY - 1) / kTY); }

hipError_t launch_clean_init(double* res, int64_t nx, int64_t ny, const uint8_t* mask, CleanEntry* table,
                             CleanState* state, hipStream_t s) {
  hipError_t e = hipMemsetAsync(state, 0, sizeof(CleanState), s);
  if (e != hipSuccess) return e;
  const int64_t nty = (ny + kTY - 1) / kTY;
  clean_init_kernel<<<dim3((unsigned)clean_tiles(nx, ny)), dim3(kThreads), 0, s>>>(res, nx, ny, nty, mask, table);
  return hipGetLastError();
}

hipError_t launch_clean_subtract(double* res, int64_t nx, int64_t ny, const double* psf, int64_t px, int64_t py,
                                 int64_t cx, int64_t cy, const uint8_t* mask, CleanEntry* table,
                                 const CleanState* state, hipStream_t s) {
  // the tiles a px x py window can meet: its extent plus one tile of slack per
  // axis for a window that does not start on a tile edge, never more than the
  // image has (the host does not know the peak)
  const int64_t ntx = (nx + kTX - 1) / kTX, nty = (ny + kTY - 1) / kTY;
  const int64_t gx = std::min<int64_t>(ntx, (std::min(px, nx) + kTX - 1) / kTX + 1);
  const int64_t gy = std::min<int64_t>(nty, (std::min(py, ny) + kTY - 1) / kTY + 1);
  clean_subtract_kernel<<<dim3((unsigned)(gx * gy)), dim3(kThreads), 0, s>>>(res, nx, ny, nty, psf, px, py, cx, cy, gy,
                                                                             mask, table, state);
  return hipGetLastError();
}

hipError_t launch_clean_select(const double* res, int64_t nx, int64_t ny, const CleanEntry* table, double gain,
                               double threshold, int64_t niter, double* model, int64_t* comp_index, double* comp_flux,
                               CleanState* state, hipStream_t s) {
  clean_select_kernel<<<dim3(1), dim3(kSelectThreads), 0, s>>>(res, table, clean_tiles(nx, ny), gain, threshold, niter,
                                                               ny, model, comp_index, comp_flux, state);
  return hipGetLastError();
}

}  // namespace cip

// ------------------------------------------------------------ host API ----
namespace cip {

// Hogbom CLEAN (cip_hogbom_clean): init builds the tile table,
// then select and (subtract, select) pairs are queued `batch` iterations at a
// time; the device state is read back once per batch. Kernels queued behind a
// stop return at once, so the result does not depend on `batch`.
static int hogbom_clean_impl(double* res, int64_t nx, int64_t ny, const double* psf, int64_t px, int64_t py,
                             int64_t cx, int64_t cy, const uint8_t* mask, double gain, double threshold,
                             int64_t niter, int64_t batch, void* hip_stream, double* model, int64_t* comp_index,
                             double* comp_flux, cip_clean_result* result_out) {
  if (!res || !psf) return set_error(CIP_EINVAL, "cip_hogbom_clean: residual_io and psf must not be NULL");
  if (nx < 1 || ny < 1 || px < 1 || py < 1)
    return set_error(CIP_EINVAL, "cip_hogbom_clean: image and PSF dimensions must be >= 1");
  if (cx == -1) cx = px / 2;
  if (cy == -1) cy = py / 2;
  if (cx < 0 || cx >= px || cy < 0 || cy >= py)
    return set_error(CIP_EINVAL, "cip_hogbom_clean: the PSF centre lies outside the PSF");
  if (!std::isfinite(gain) || !(gain > 0.0)) return set_error(CIP_EINVAL, "cip_hogbom_clean: gain must be finite and > 0");
  if (std::isnan(threshold) || threshold < 0.0)
    return set_error(CIP_EINVAL, "cip_hogbom_clean: threshold must be >= 0 and not NaN");
  if (niter < 0 || batch < 0) return set_error(CIP_EINVAL, "cip_hogbom_clean: niter and batch must be >= 0");
  if ((comp_index == nullptr) != (comp_flux == nullptr))
    return set_error(CIP_EINVAL, "cip_hogbom_clean: comp_index and comp_flux go together (both or neither)");
  if (nx > INT64_MAX / ny || px > INT64_MAX / py)
    return set_error(CIP_EINVAL, "cip_hogbom_clean: image or PSF too large");
  const int64_t ntiles = clean_tiles(nx, ny);
  if (ntiles >= ((int64_t)1 << 31)) return set_error(CIP_EINVAL, "cip_hogbom_clean: image has 2^31 tiles or more");
  if (batch == 0) batch = CIP_CLEAN_DEFAULT_BATCH;
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(table, CleanEntry, "clean_table", ntiles)
  CIP_ALLOC(state, CleanState, "clean_state", 1)
  CleanState* h = (CleanState*)pinned(ws, sizeof(CleanState));
  if (!h) return CIP_ENOMEM;
  CIP_HIP_CHECK(launch_clean_init(res, nx, ny, mask, table, state, s));
  CIP_HIP_CHECK(launch_clean_select(res, nx, ny, table, gain, threshold, niter, model, comp_index, comp_flux, state, s));
  for (int64_t queued = 0;;) {
    const int64_t n = std::min(batch, niter - queued);
    for (int64_t q = 0; q < n; ++q) {
      CIP_HIP_CHECK(launch_clean_subtract(res, nx, ny, psf, px, py, cx, cy, mask, table, state, s));
      CIP_HIP_CHECK(
          launch_clean_select(res, nx, ny, table, gain, threshold, niter, model, comp_index, comp_flux, state, s));
    }
    queued += n;
    CIP_HIP_CHECK(hipMemcpyAsync(h, state, sizeof(CleanState), hipMemcpyDeviceToHost, s));
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    if (h->stopped) break;
    // after niter pairs the last select saw k == niter and stopped
    if (queued >= niter) return set_error(CIP_EHIP, "cip_hogbom_clean: the device state did not stop");
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

}  // namespace cip

using namespace cip;

extern "C" {

int cip_hogbom_clean(double* residual_io, int64_t nx, int64_t ny, const double* psf, int64_t psf_nx, int64_t psf_ny,
                     int64_t psf_cx, int64_t psf_cy, const uint8_t* mask, double gain, double threshold,
                     int64_t niter, int64_t batch, void* hip_stream, double* model_io, int64_t* comp_index,
                     double* comp_flux, cip_clean_result* result_out) {
  clear_error();
  return hogbom_clean_impl(residual_io, nx, ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, mask, gain, threshold, niter,
                           batch, hip_stream, model_io, comp_index, comp_flux, result_out);
}

}  // extern "C"
