// cip_strips.hip - the uv-strip split of the strong-scaling path (DESIGN.md 7,
// SURVEY.md 8(e) option 1) on the device: which grid rows each rank owns and
// which visibilities it grids. The reference's counterpart is its offline
// bucket step - uvw_tiling/tiling_plan.py:29-61 (tile keys and row runs) and
// reorder.py:19-111 (regrouping the visibilities by tile) - here cut by
// footprint-origin grid row instead of by uvw tile, so that a rank's share is
// a contiguous strip of grid rows.
//
// Three kernels, all of them one wave per MS row walking its channels 64 at a
// time (lane = channel), with the gridder's own fp64 placement (place_origin's
// operations and order, so a visibility lands in the strip its footprint
// starts in - bit for bit the planner's origin):
//  * strip_hist_kernel: per grid row, the visibilities whose footprint origin
//    lies in it and the row slices starting there (the cost model's inputs,
//    strips.row_costs); wave-segmented counts into a block-private LDS
//    histogram, per-block partials summed by strip_hist_reduce_kernel;
//  * strip_count_kernel: per MS row, the maximal channel runs whose origin row
//    lies in [y0, y1) and their visibilities (then two exclusive scans);
//  * strip_emit_kernel: the runs as Tile-layout row slices (uvw, channel
//    range, MS row) and the strip's visibilities and weights gathered into
//    slice order - the whole strip in one pass over the dense columns.
#include "cip_host.h"

namespace cip {

// Footprint origin index along one axis: floor((c fx) s + n / 2 - W / 2) + 1
// wrapped into [0, n) (n a power of two), the gridder's placement arithmetic
// (cip_common.h place_origin / place_vis: the same fp64 operations, no
// contraction). Non-finite or huge coordinates give 0 (the planner rejects
// such visibilities when they are gridded).
__device__ __forceinline__ int64_t strip_origin(double c_m, double fx, double scale, int64_t n, int hw) {
#pragma clang fp contract(off)
  const double x = (c_m * fx) * scale + (double)(n / 2);
  const double fl = floor(x - (double)hw);
  const bool ok = fabs(fl) < 4.0e18;  // false for NaN / inf too
  const int64_t i = ok ? (int64_t)fl + 1 : 0;
  return i & (n - 1);
}

constexpr int kStripThreads = 1024;

// Block-private histograms (2 nv uint32 in dynamic LDS: visibilities, then
// slice starts, per footprint-origin grid row) over a grid-stride of MS rows,
// one wave per row. A slice starts at channel 0 and wherever the origin's
// 32-cell tile (iy / 32, ix / 32) changes along the channels (strips.py
// row_costs' key). Lanes of one wave with equal origin rows are counted by
// their segment head (consecutive channels mostly share a row), so the LDS
// atomics per 64 channels are the number of row changes, not 64.
__global__ __launch_bounds__(kStripThreads) void strip_hist_kernel(const double* __restrict__ uvw, int64_t nrow,
                                                                   const double* __restrict__ fx, int64_t nchan,
                                                                   int64_t nu, int64_t nv, double scale_u,
                                                                   double scale_v, int hw,
                                                                   uint32_t* __restrict__ partial) {
  extern __shared__ uint32_t s_h[];  // [0, nv): visibilities, [nv, 2 nv): slice starts
  for (int64_t k = threadIdx.x; k < 2 * nv; k += kStripThreads) s_h[k] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (kStripThreads / 64);
  const int64_t key_row = nu / 32 + 1;
  for (int64_t r = (int64_t)blockIdx.x * (kStripThreads / 64) + (threadIdx.x >> 6); r < nrow; r += waves) {
    const double u = uvw[3 * r], v = uvw[3 * r + 1];
    int64_t carry_key = -1;  // the previous chunk's last key (-1: row start)
    for (int64_t c0 = 0; c0 < nchan; c0 += 64) {
      const int64_t c = c0 + lane;
      const bool valid = c < nchan;
      const double f = fx[valid ? c : 0];
      const int64_t iy = strip_origin(v, f, scale_v, nv, hw);
      const int64_t ix = strip_origin(u, f, scale_u, nu, hw);
      const int64_t key = (iy >> 5) * key_row + (ix >> 5);
      int64_t prev = __shfl_up(key, 1, 64);
      if (lane == 0) prev = carry_key;
      const bool start = valid && (prev < 0 || key != prev);
      // segments of equal origin row: heads where the row differs from the
      // previous lane's (or lane 0); a head counts up to the next head
      const int64_t prev_iy = __shfl_up(iy, 1, 64);
      const bool head = valid && (lane == 0 || iy != prev_iy);
      const unsigned long long heads = __ballot(head);
      const unsigned long long starts = __ballot(start);
      const int nvalid = __popcll(__ballot(valid));
      if (head) {
        const unsigned long long above = heads & ~((2ull << lane) - 1ull);  // lane 63: 2 << 63 == 0
        const int next = above ? (__ffsll((long long)above) - 1) : nvalid;
        const unsigned long long seg = (next >= 64 ? ~0ull : ((1ull << next) - 1ull)) & ~((1ull << lane) - 1ull);
        atomicAdd(&s_h[iy], (uint32_t)(next - lane));
        const int ns = __popcll(starts & seg);
        if (ns) atomicAdd(&s_h[nv + iy], (uint32_t)ns);
      }
      carry_key = __shfl(key, 63, 64);
    }
  }
  __syncthreads();
  uint32_t* out = partial + (int64_t)blockIdx.x * 2 * nv;
  for (int64_t k = threadIdx.x; k < 2 * nv; k += kStripThreads) out[k] = s_h[k];
}

// hist[k] = sum over blocks of partial[b][k] (int64; k < 2 nv: the
// visibilities, then the slice starts, per grid row)
__global__ void strip_hist_reduce_kernel(const uint32_t* __restrict__ partial, int nblocks, int64_t n2,
                                         int64_t* __restrict__ hist) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n2) return;
  int64_t s = 0;
  for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * n2 + k];
  hist[k] = s;
}

int strip_hist_blocks(int64_t nrow) {
  const int64_t b = (nrow + kStripThreads / 64 - 1) / (kStripThreads / 64);
  return (int)(b < 256 ? (b > 0 ? b : 1) : 256);
}

hipError_t launch_strip_hist(const double* uvw, int64_t nrow, const double* fx, int64_t nchan,
                             const GridGeometry& g, uint32_t* partial, int nblocks, int64_t* hist, hipStream_t s) {
  const size_t lds = sizeof(uint32_t) * 2 * (size_t)g.nv;
  if (lds > 160 * 1024 - 1024) return hipErrorInvalidValue;
  strip_hist_kernel<<<dim3(nblocks), dim3(kStripThreads), lds, s>>>(uvw, nrow, fx, nchan, g.nu, g.nv, g.scale_u,
                                                                    g.scale_v, g.support / 2, partial);
  const int64_t n2 = 2 * g.nv;
  strip_hist_reduce_kernel<<<dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s>>>(partial, nblocks, n2, hist);
  return hipGetLastError();
}

// The runs of channels of row r whose origin row lies in [y0, y1), chunk by
// chunk: in = the channel's origin row inside the strip; a run starts where
// `in` rises and stops where it falls (or at the row's end).
struct StripWalk {
  int64_t runs = 0, vis = 0;  // before this chunk
  bool carry_in = false;      // the previous chunk's last channel was inside
};

__device__ __forceinline__ bool strip_in(double v, const double* __restrict__ fx, int64_t c, int64_t nchan,
                                         double scale_v, int64_t nv, int hw, int64_t y0, int64_t y1) {
  if (c >= nchan) return false;
  const int64_t iy = strip_origin(v, fx[c], scale_v, nv, hw);
  return iy >= y0 && iy < y1;
}

// row_runs[r] / row_vis[r]: the strip's runs and visibilities in MS row r
// (entry nrow: 0, so the exclusive scans' last entries are the totals)
__global__ __launch_bounds__(256) void strip_count_kernel(const double* __restrict__ uvw, int64_t nrow,
                                                          const double* __restrict__ fx, int64_t nchan, int64_t nv,
                                                          double scale_v, int hw, int64_t y0, int64_t y1,
                                                          int64_t* __restrict__ row_runs,
                                                          int64_t* __restrict__ row_vis) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r == nrow && lane == 0) {
    row_runs[nrow] = 0;
    row_vis[nrow] = 0;
  }
  if (r >= nrow) return;
  const double v = uvw[3 * r + 1];
  StripWalk w;
  for (int64_t c0 = 0; c0 < nchan; c0 += 64) {
    const bool in = strip_in(v, fx, c0 + lane, nchan, scale_v, nv, hw, y0, y1);
    const unsigned long long ins = __ballot(in);
    const unsigned long long rises = ins & ~((ins << 1) | (w.carry_in ? 1ull : 0ull));
    w.runs += __popcll(rises);
    w.vis += __popcll(ins);
    w.carry_in = (ins >> 63) & 1ull;
    if (c0 + 64 > nchan) w.carry_in = false;
  }
  if (lane == 0) {
    row_runs[r] = w.runs;
    row_vis[r] = w.vis;
  }
}

hipError_t launch_strip_count(const double* uvw, int64_t nrow, const double* fx, int64_t nchan,
                              const GridGeometry& g, int64_t y0, int64_t y1, int64_t* row_runs, int64_t* row_vis,
                              hipStream_t s) {
  strip_count_kernel<<<dim3((unsigned)(nrow / 4 + 1)), dim3(256), 0, s>>>(uvw, nrow, fx, nchan, g.nv, g.scale_v,
                                                                         g.support / 2, y0, y1, row_runs, row_vis);
  return hipGetLastError();
}

// The strip's row slices and its visibilities, from the scanned counts: slice
// k of row r (k-th rise of `in`) at run_off[r] + k with the row's uvw, the
// channel range and the MS row; its visibilities (and weights) copied to
// vis_off[r] + (the row's inside channels before them), in channel order -
// slices in (row, channel) order, the Tile layout of reference
// uvw_tiling/tile.py:14-124. VB / WB: bytes per visibility / weight (0: none).
template <int VB, int WB>
__global__ __launch_bounds__(256) void strip_emit_kernel(
    const double* __restrict__ uvw, int64_t nrow, const double* __restrict__ fx, int64_t nchan, int64_t nv,
    double scale_v, int hw, int64_t y0, int64_t y1, const int64_t* __restrict__ run_off,
    const int64_t* __restrict__ vis_off, const void* __restrict__ vis, const void* __restrict__ wgt,
    double* __restrict__ slice_uvw, int32_t* __restrict__ chan_start, int32_t* __restrict__ chan_stop,
    int64_t* __restrict__ slice_row, void* __restrict__ vis_out, void* __restrict__ wgt_out) {
  using VT = typename std::conditional<VB == 16, uint4, uint2>::type;
  using WT = typename std::conditional<WB == 8, uint64_t, uint32_t>::type;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrow) return;
  const int64_t rb = run_off[r], vb = vis_off[r];
  if (run_off[r + 1] == rb) return;  // nothing of this row in the strip
  const double u = uvw[3 * r], v = uvw[3 * r + 1], w = uvw[3 * r + 2];
  StripWalk st;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t c0 = 0; c0 < nchan; c0 += 64) {
    const int64_t c = c0 + lane;
    const bool in = strip_in(v, fx, c, nchan, scale_v, nv, hw, y0, y1);
    const unsigned long long ins = __ballot(in);
    const unsigned long long prev = (ins << 1) | (st.carry_in ? 1ull : 0ull);
    const unsigned long long rises = ins & ~prev;
    const unsigned long long falls = ~ins & prev;  // lane l: channel c0 + l is the first one outside
    if ((rises >> lane) & 1ull) {
      const int64_t k = rb + st.runs + __popcll(rises & below);
      slice_uvw[3 * k] = u;
      slice_uvw[3 * k + 1] = v;
      slice_uvw[3 * k + 2] = w;
      chan_start[k] = (int32_t)c;
      slice_row[k] = r;
    }
    if (((falls >> lane) & 1ull) && c <= nchan) {
      // the run that fell here is the last one started before this lane
      const int64_t k = rb + st.runs + __popcll(rises & below) - 1;
      chan_stop[k] = (int32_t)c;
    }
    if constexpr (VB > 0) {
      if (in) {
        const int64_t d = vb + st.vis + __popcll(ins & below);
        ((VT*)vis_out)[d] = ((const VT*)vis)[r * nchan + c];
        if constexpr (WB > 0) ((WT*)wgt_out)[d] = ((const WT*)wgt)[r * nchan + c];
      }
    }
    st.runs += __popcll(rises);
    st.vis += __popcll(ins);
    st.carry_in = (ins >> 63) & 1ull;
  }
  // a run still open at the row's end stops at nchan (when nchan is a
  // multiple of 64 no lane of the loop saw position nchan)
  if (nchan % 64 == 0 && st.carry_in && lane == 0) chan_stop[rb + st.runs - 1] = (int32_t)nchan;
}

hipError_t launch_strip_emit(const double* uvw, int64_t nrow, const double* fx, int64_t nchan, const GridGeometry& g,
                             int64_t y0, int64_t y1, const int64_t* run_off, const int64_t* vis_off, const void* vis,
                             int vis_bytes, const void* wgt, int wgt_bytes, double* slice_uvw, int32_t* chan_start,
                             int32_t* chan_stop, int64_t* slice_row, void* vis_out, void* wgt_out, hipStream_t s) {
  const dim3 gd((unsigned)((nrow + 3) / 4)), bd(256);
  auto emit = [&](auto vb, auto wb) {
    strip_emit_kernel<decltype(vb)::value, decltype(wb)::value><<<gd, bd, 0, s>>>(
        uvw, nrow, fx, nchan, g.nv, g.scale_v, g.support / 2, y0, y1, run_off, vis_off, vis, wgt, slice_uvw,
        chan_start, chan_stop, slice_row, vis_out, wgt_out);
    return hipGetLastError();
  };
  if (vis_bytes == 0) return emit(int_tag<0>{}, int_tag<0>{});  // no visibilities: no weights either
  return dispatch_int<8, 16>(vis_bytes, hipErrorInvalidValue, [&](auto vb) {
    return dispatch_int<0, 4, 8>(wgt_bytes, hipErrorInvalidValue, [&](auto wb) { return emit(vb, wb); });
  });
}

// A strip's dirty-tile bits for its masked pass A (cip_strip_rows_masked):
// the planner's own per-plane mask of the gridded strip (dirty_mask_kernel:
// every tile the scatter's flush may write), plus every tile of the tile rows
// holding buffer rows [0, halo) - grid rows row0 .. row0 + halo - 1 (mod nv),
// where the previous rank's halo is added after the gridding. dmask may be
// NULL (an empty strip). words = nty * (ntx / 32) per plane.
__global__ void strip_mask_kernel(const uint32_t* __restrict__ dmask, int64_t nplanes, int64_t nty, int64_t wpr,
                                  int64_t row0, int64_t halo, int64_t nv, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nplanes * nty * wpr) return;
  const int64_t ty = (i / wpr) % nty;
  // tile rows of grid rows row0 .. row0 + halo - 1 (wrapping)
  const int64_t t0 = row0 / 32, t1 = (row0 + (halo > 0 ? halo : 1) - 1) / 32;  // unwrapped tile rows
  const int64_t nt = nv / 32;
  bool in_halo = false;
  for (int64_t t = t0; t <= t1; ++t) in_halo = in_halo || (t % nt) == ty;
  out[i] = (dmask ? dmask[i] : 0u) | (in_halo ? 0xffffffffu : 0u);
}

hipError_t launch_strip_mask(const uint32_t* dmask, const GridGeometry& g, int64_t row0, int64_t halo, uint32_t* out,
                             hipStream_t s) {
  const int64_t wpr = g.mtx / 32;
  const int64_t n = g.nplanes * g.mty * wpr;
  if (n <= 0) return hipSuccess;
  strip_mask_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(dmask, g.nplanes, g.mty, wpr, row0, halo,
                                                                          g.nv, out);
  return hipGetLastError();
}

}  // namespace cip

// ------------------------------------------------------------ host API ----
using namespace cip;

extern "C" {

// ---- the uv-strip split on the device (cip_strips.hip) ----
static int strip_split_check(const cip_gridder_params* params, const double* uvw, int64_t nrow, const double* freq,
                             int64_t nchan, GridGeometry* g) {
  if (!params) return set_error(CIP_EINVAL, "params is NULL");
  if (nrow < 0 || nchan < 1 || nchan > 65535) return set_error(CIP_EINVAL, "need nrow >= 0 and 1 <= nchan <= 65535");
  if (nrow > 0 && (!uvw || !freq)) return set_error(CIP_EINVAL, "NULL uvw or freq");
  const bool pow2 = params->nu > 0 && params->nv > 0 && (params->nu & (params->nu - 1)) == 0 &&
                    (params->nv & (params->nv - 1)) == 0;
  if (!pow2 || params->nv < 32 || params->nv > 16384)
    return set_error(CIP_EINVAL, "strips need a power-of-two grid of 32 .. 16384 rows");
  *g = geometry(*params, 1.0, 1.0);
  return CIP_OK;
}

int cip_strip_histogram(const double* uvw, int64_t nrow, const double* freq, int64_t nchan,
                        const cip_gridder_params* params, double pixsize_x, double pixsize_y, void* hip_stream,
                        int64_t* hist) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_split_check(params, uvw, nrow, freq, nchan, &g); rc != CIP_OK) return rc;
  if (!hist) return set_error(CIP_EINVAL, "NULL hist");
  g = geometry(*params, pixsize_x, pixsize_y);
  CIP_BEGIN_CALL(hip_stream, false)
  if (nrow == 0) {
    CIP_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(int64_t) * 2 * g.nv, s));
    return CIP_OK;
  }
  CIP_ALLOC(fx, double, "strip_fx", nchan)
  CIP_HIP_CHECK(launch_freq_scale(freq, nchan, fx, nullptr, s));
  const int nb = strip_hist_blocks(nrow);
  CIP_ALLOC(partial, uint32_t, "strip_hist_partial", (int64_t)nb * 2 * g.nv)
  CIP_HIP_CHECK(launch_strip_hist(uvw, nrow, fx, nchan, g, partial, nb, hist, s));
  return CIP_OK;
}

int cip_strip_split(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis,
                    int vis_dtype, const void* wgt, int wgt_dtype, const cip_gridder_params* params, double pixsize_y,
                    int64_t y0, int64_t y1, void* hip_stream, int64_t* counts, double* slice_uvw,
                    int32_t* chan_start, int32_t* chan_stop, int64_t* slice_row, void* vis_out, void* wgt_out) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_split_check(params, uvw, nrow, freq, nchan, &g); rc != CIP_OK) return rc;
  g = geometry(*params, 1.0, pixsize_y);
  if (!counts) return set_error(CIP_EINVAL, "NULL counts");
  if (y0 < 0 || y1 > g.nv || y1 <= y0) return set_error(CIP_EINVAL, "strip rows outside the grid");
  const int vb = vis ? (vis_dtype == CIP_C64 ? 8 : (vis_dtype == CIP_C128 ? 16 : -1)) : 0;
  const int wb = (vis && wgt) ? (wgt_dtype == CIP_F32 ? 4 : (wgt_dtype == CIP_F64 ? 8 : -1)) : 0;
  if (vb < 0) return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  if (wb < 0) return set_error(CIP_EINVAL, "wgt dtype must be float32 or float64");
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(fx, double, "strip_fx", nchan)
  CIP_ALLOC(row_runs, int64_t, "strip_row_runs", nrow + 1)
  CIP_ALLOC(row_vis, int64_t, "strip_row_vis", nrow + 1)
  CIP_ALLOC(scan_tmp, int64_t, "strip_scan_tmp", scan_tmp_elems(nrow + 1))
  CIP_HIP_CHECK(launch_freq_scale(freq, nchan, fx, nullptr, s));
  // the counts and their scans: phase 1 (slice_uvw == NULL) reports the totals;
  // phase 2 recounts (the same arithmetic, the same numbers) and emits
  CIP_HIP_CHECK(launch_strip_count(uvw, nrow, fx, nchan, g, y0, y1, row_runs, row_vis, s));
  CIP_HIP_CHECK(exclusive_scan_i64(row_runs, nrow + 1, scan_tmp, s));
  CIP_HIP_CHECK(exclusive_scan_i64(row_vis, nrow + 1, scan_tmp, s));
  if (!slice_uvw) {
    int64_t* h = nullptr;
    if (const int rc = readback(ws, s, {{row_runs + nrow, sizeof(int64_t)}, {row_vis + nrow, sizeof(int64_t)}}, &h);
        rc != CIP_OK)
      return rc;
    counts[0] = h[0];
    counts[1] = h[1];
    return CIP_OK;
  }
  if (!chan_start || !chan_stop || !slice_row) return set_error(CIP_EINVAL, "NULL slice outputs");
  if (vb > 0 && !vis_out) return set_error(CIP_EINVAL, "NULL vis_out");
  if (wb > 0 && !wgt_out) return set_error(CIP_EINVAL, "NULL wgt_out");
  if (nrow > 0)
    CIP_HIP_CHECK(launch_strip_emit(uvw, nrow, fx, nchan, g, y0, y1, row_runs, row_vis, vis, vb, wgt, wb, slice_uvw,
                                    chan_start, chan_stop, slice_row, vb ? vis_out : nullptr, wb ? wgt_out : nullptr,
                                    s));
  return CIP_OK;
}

// strips of the pruned FFT (multi-GPU strong scaling)
static int strip_check(const cip_gridder_params* params, int64_t npix_x, int64_t npix_y, GridGeometry* g) {
  if (!params) return set_error(CIP_EINVAL, "params is NULL");
  *g = geometry(*params, 1.0, 1.0);
  if (!grid_is_transposed(*g, npix_x, npix_y))
    return set_error(CIP_EINVAL, "strips need the pruned-FFT grid layout (power-of-two grids, cip_grid_layout == 1)");
  return CIP_OK;
}

// pass A of a strip, after the caller's own checks: rows [y0, y1) of the
// buffer into H; dmask / row0 / row_slot / nlive as launch_fft_rows_strip
static int strip_rows(void* hip_stream, double* grid, const GridGeometry& g, int64_t npix_x, int64_t y0, int64_t y1,
                      double* H, const uint32_t* dmask = nullptr, int64_t row0 = 0,
                      const int64_t* row_slot = nullptr, int64_t nlive = 0) {
  CIP_BEGIN_CALL(hip_stream, false)
  double* tw_u = nullptr;
  if (const int rc = fft_twiddles(ws, g.nu, s, &tw_u); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_fft_rows_strip(grid, g.nu, g.nv, npix_x, tw_u, y0, y1, H, dmask, row0, row_slot, nlive, s));
  return end_call(call);
}

// [i0, i1): image rows of a strip's pass B, whole column blocks of 4
static int strip_cols_range_check(int64_t i0, int64_t i1, int64_t npix_x) {
  if (i0 < 0 || i1 > npix_x || i1 <= i0 || i0 % 4 || i1 % 4)
    return set_error(CIP_EINVAL, "image row range must be multiples of 4 inside [0, npix_x]");
  return CIP_OK;
}

int cip_strip_rows(double* grid, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y, int64_t y0,
                   int64_t y1, void* hip_stream, double* H) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (!grid || !H) return set_error(CIP_EINVAL, "NULL grid or H");
  if (y0 < 0 || y1 > g.nv || y1 <= y0) return set_error(CIP_EINVAL, "row range outside the grid");
  return strip_rows(hip_stream, grid, g, npix_x, y0, y1, H);
}

int cip_strip_rows_masked(double* grid, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y,
                          int64_t y0, int64_t y1, int64_t row0, const uint32_t* tile_bits, void* hip_stream,
                          double* H) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (!grid || !H || !tile_bits) return set_error(CIP_EINVAL, "NULL grid, H or tile_bits");
  if (y0 < 0 || y1 > g.nv || y1 <= y0) return set_error(CIP_EINVAL, "row range outside the grid");
  if (row0 < 0 || row0 >= g.nv) return set_error(CIP_EINVAL, "row0 outside the grid");
  if (g.mtx % 32 != 0) return set_error(CIP_EINVAL, "tile masks need nu / 32 to be a multiple of 32 tiles");
  return strip_rows(hip_stream, grid, g, npix_x, y0, y1, H, tile_bits, row0);
}

int cip_strip_rows_packed(double* grid, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y,
                          int64_t y0, int64_t y1, int64_t row0, const uint32_t* tile_bits, const int64_t* row_slot,
                          int64_t nlive, void* hip_stream, double* H) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (!grid || !tile_bits || !row_slot) return set_error(CIP_EINVAL, "NULL grid, tile_bits or row_slot");
  if (y0 < 0 || y1 > g.nv || y1 <= y0) return set_error(CIP_EINVAL, "row range outside the grid");
  if (row0 < 0 || row0 >= g.nv) return set_error(CIP_EINVAL, "row0 outside the grid");
  if (nlive < 0 || nlive > y1 - y0) return set_error(CIP_EINVAL, "nlive outside [0, y1 - y0]");
  if (nlive > 0 && !H) return set_error(CIP_EINVAL, "NULL H");
  if (g.mtx % 32 != 0) return set_error(CIP_EINVAL, "tile masks need nu / 32 to be a multiple of 32 tiles");
  return strip_rows(hip_stream, grid, g, npix_x, y0, y1, H, tile_bits, row0, row_slot, nlive);
}

int cip_strip_cols(const double* H, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y, int64_t i0,
                   int64_t i1, const double* norm, void* hip_stream, double* dirty_rows) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (params->do_wstacking)
    return set_error(CIP_EINVAL, "cip_strip_cols: 2-D grids only (w-stacking strips use cip_strip_cols_wplane + "
                                 "cip_strip_wfinal)");
  if (!H || !dirty_rows) return set_error(CIP_EINVAL, "NULL H or dirty_rows");
  if (const int rc = strip_cols_range_check(i0, i1, npix_x); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, false)
  double *tw_v = nullptr, *cx = nullptr, *cy = nullptr;
  if (const int rc = fft_twiddles(ws, g.nv, s, &tw_v); rc != CIP_OK) return rc;
  if (const int rc = correction_vectors(ws, g, npix_x, npix_y, s, &cx, &cy); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_fft_cols_strip(H, g.nv, npix_x, npix_y, tw_v, i0, i1, dirty_rows, cx, cy, norm, s));
  return end_call(call);
}

int cip_strip_pack_rows(const void* H, int64_t nb, int64_t h, int elem_bytes, const int64_t* slot, int64_t nlive,
                        void* hip_stream, void* out) {
  clear_error();
  if (elem_bytes != 8 && elem_bytes != 16) return set_error(CIP_EINVAL, "elem_bytes must be 8 or 16");
  if (nb < 0 || h < 0 || nlive < 0 || nlive > h) return set_error(CIP_EINVAL, "bad pack sizes");
  if (nb > 65535) return set_error(CIP_EINVAL, "more than 65535 column blocks");
  if (nb * h * nlive > 0 && (!H || !slot || !out)) return set_error(CIP_EINVAL, "NULL pointer");
  CIP_HIP_CHECK(launch_strip_pack(H, nb, h, elem_bytes / 4, slot, nlive, out, (hipStream_t)hip_stream));
  return CIP_OK;
}

int cip_strip_unpack_rows(const void* recv, int64_t nb, int64_t nv, int elem_bytes, const int64_t* rec,
                          const int64_t* stride, void* hip_stream, void* H) {
  clear_error();
  if (elem_bytes != 8 && elem_bytes != 16) return set_error(CIP_EINVAL, "elem_bytes must be 8 or 16");
  if (nb < 0 || nv < 0) return set_error(CIP_EINVAL, "bad unpack sizes");
  if (nb > 65535) return set_error(CIP_EINVAL, "more than 65535 column blocks");
  if (nb * nv > 0 && (!rec || !stride || !H)) return set_error(CIP_EINVAL, "NULL pointer");
  CIP_HIP_CHECK(launch_strip_unpack(recv, nb, nv, elem_bytes / 4, rec, stride, H, (hipStream_t)hip_stream));
  return CIP_OK;
}

int cip_strip_cols_wplane(const double* H, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y,
                          double pixsize_x, double pixsize_y, int64_t i0, int64_t i1, int64_t plane, int first,
                          void* hip_stream, double* acc_rows) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (!params->do_wstacking) return set_error(CIP_EINVAL, "cip_strip_cols_wplane: w-stacking parameters only");
  if (!H || !acc_rows) return set_error(CIP_EINVAL, "NULL H or acc_rows");
  if (plane < 0 || plane >= params->nplanes) return set_error(CIP_EINVAL, "plane out of range");
  if (const int rc = strip_cols_range_check(i0, i1, npix_x); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, false)
  double* tw_v = nullptr;
  if (const int rc = fft_twiddles(ws, g.nv, s, &tw_v); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_fft_cols_strip_wplane(H, g.nv, npix_x, npix_y, tw_v, i0, i1, acc_rows, pixsize_x, pixsize_y,
                                             params->w0 + (double)plane * params->dw, first != 0, s));
  return end_call(call);
}

int cip_strip_wfinal(double* acc_rows, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y,
                     double pixsize_x, double pixsize_y, int64_t i0, int64_t i1, const double* norm,
                     void* hip_stream) {
  clear_error();
  GridGeometry g;
  if (const int rc = strip_check(params, npix_x, npix_y, &g); rc != CIP_OK) return rc;
  if (!params->do_wstacking) return set_error(CIP_EINVAL, "cip_strip_wfinal: w-stacking parameters only");
  if (!acc_rows) return set_error(CIP_EINVAL, "NULL acc_rows");
  if (i0 < 0 || i1 > npix_x || i1 <= i0) return set_error(CIP_EINVAL, "image rows outside [0, npix_x)");
  CIP_BEGIN_CALL(hip_stream, false)
  double *cx = nullptr, *cy = nullptr, *fwd = nullptr;
  int64_t fw_n = 0;
  double dnu = 0.0;
  if (const int rc = correction_vectors(ws, g, npix_x, npix_y, s, &cx, &cy); rc != CIP_OK) return rc;
  if (const int rc = w_correction_table(ws, *params, g, s, &fwd, &fw_n, &dnu); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_wfinal_correct(acc_rows, npix_x, npix_y, pixsize_x, pixsize_y, cx, cy, fwd, fw_n, dnu, g.dw, i0,
                                      i1 - i0, norm, nullptr, s));
  return end_call(call);
}

}  // extern "C"
