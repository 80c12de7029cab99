// cip_invert.hip - the invert (gridding) drivers: scatter_plane, the
// grid -> dirty image stage, ms2dirty_impl and grid_accumulate, with the
// cip_ms2dirty*, cip_grid_ms*, cip_grid_tiles*, cip_grid_to_dirty and
// cip_grid_plane entry points.
#include <algorithm>
#include <cmath>

#include "cip_host.h"

namespace cip {

// Sole-unit private-cell stores in the scatter's flush (cip_scatter.h) on grid
// planes of >= 16384^2 cells: C4's flush goes to a 4 GiB plane that no cache
// holds, and stores cut the C4-shard scatter 4.87 -> 4.59 ms; on C3's 8192^2
// plane they cost 1-3 % (profiles/r03_ab_flush_store.txt). CIP_FLUSH_STORE=0 /
// 1 forces them off / on for any grid (A/B).
static bool flush_store_enabled(const GridGeometry& g) {
  const int mode = flush_store_mode();
  return mode < 0 ? g.nu * g.nv >= ((int64_t)1 << 28) : mode == 1;
}

// Work-unit range q of the plan (w-stacking: plane group q = planes
// [q G, q G + G), written to grid + k planes for plane q G + k; 2-D: q = 0).
// rq: the request pp was prepared from (its visibilities and weights)
// transposed: store the grid as gT[y, x] (input layout of the pruned FFT)
// zeroed: the group's planes are already zero (no memset: zeroed on the side
// stream and joined by the caller, or left clean); share_cus: launch_scatter's;
// accumulate: they hold earlier chunks' sums (cip_grid_ms: += onto them), so
// the flush never stores
struct ScatterMode {
  bool transposed = false, zeroed = false, share_cus = false, accumulate = false;
};
static int scatter_plane(const Prepared& pp, const PlanRequest& rq, int64_t q, const ScatterMode& mode, double* grid,
                         hipStream_t s) {
  GridGeometry g = pp.g;
  g.transposed = mode.transposed ? 1 : 0;
  const int G = pp.plan.group;
  const int64_t p0 = g.do_wstacking ? q * G : 0;
  const int64_t np = g.do_wstacking ? std::min<int64_t>(G, g.nplanes - p0) : 1;
  if (!mode.zeroed)
    CIP_HIP_CHECK(hipMemsetAsync(grid, 0, (g.grid_f32 ? sizeof(float) : sizeof(double)) * 2 * g.nu * g.nv * np, s));
  if (pp.plan.nchunks == 0) return CIP_OK;
  const int64_t k = g.do_wstacking ? q : 0;
  const int64_t cb = pp.plan.plane_chunk_off[k], ce = pp.plan.plane_chunk_off[k + 1];
  const int wgt_dtype = rq.wgt == nullptr ? CIP_NONE : rq.wgt_dtype;
  hipEvent_t a = g_prof.mark(s);
  ScatterLaunch sc;
  sc.plan.uvw = rq.uvw, sc.plan.fx = pp.fx, sc.plan.vis = rq.vis, sc.plan.wgt = rq.wgt;
  sc.plan.m = pp.m;
  sc.plan.m.row_phase = pp.plan.phases ? 1 : 0;
  sc.plan.runs = pp.plan.runs, sc.plan.run_goff = pp.plan.run_goff, sc.plan.tile_run_off = pp.plan.tile_run_off;
  sc.plan.perm = pp.plan.perm, sc.plan.chunks = pp.plan.chunks;
  sc.chunk_begin = cb, sc.nchunks = ce - cb;
  sc.g = g, sc.plane = p0, sc.fixed_scale = pp.fixed_scale, sc.grid = grid;
  sc.support = g.support, sc.vis_dtype = rq.vis_dtype, sc.wgt_dtype = wgt_dtype;
  sc.packed = pp.packed, sc.group = G, sc.share_cus = mode.share_cus;
  sc.store_private = !mode.accumulate && flush_store_enabled(g);
  CIP_HIP_CHECK(launch_scatter(sc, s));
  g_prof.span(2, a, g_prof.mark(s));
  if (ce > cb) g_prof.counts[4] += 1;
  return CIP_OK;
}

// Correction vectors, FFT plan / twiddles and the pass-A buffer for one
// (grid, image) geometry; then per plane: FFT + crop/correct (2-D) or the
// w-screen accumulation, and the final w-stacking correction.
struct DirtyStage {
  int64_t npix_x = 0, npix_y = 0;
  double px = 0, py = 0;
  bool fast = false;
  hipfftHandle plan = nullptr;
  double *tw_u = nullptr, *tw_v = nullptr, *fft_h = nullptr, *cx = nullptr, *cy = nullptr;
};
static int dirty_stage(Workspace* ws, const GridGeometry& g, int64_t npix_x, int64_t npix_y, double px, double py,
                       hipStream_t s, DirtyStage* st) {
  *st = DirtyStage{npix_x, npix_y, px, py};
  if (const int rc = correction_vectors(ws, g, npix_x, npix_y, s, &st->cx, &st->cy); rc != CIP_OK) return rc;
  // pruned FFT (cip_fft.hip) for power-of-two grids; hipFFT 2-D otherwise
  // (CIP_FFT_PRUNED=0 forces the latter)
  st->fast = grid_is_transposed(g, npix_x, npix_y);
  if (!st->fast) return fft_plan(ws, g.nu, g.nv, s, &st->plan);
  if (const int rc = fft_twiddles(ws, g.nu, s, &st->tw_u); rc != CIP_OK) return rc;
  if (const int rc = fft_twiddles(ws, g.nv, s, &st->tw_v); rc != CIP_OK) return rc;
  st->fft_h = buf<double>(ws, "fft_pass_a", 2 * npix_x * g.nv);
  return st->fft_h ? CIP_OK : CIP_ENOMEM;
}

// plane p's grid (consumed: the hipFFT path transforms it in place) into
// dirty_out (overwritten by the first plane, accumulated after it)
struct PlaneExtras {
  // (pruned FFT only, may be NULL): the grid tiles the scatter wrote; the rest
  // of the grid is zero, and pass A zeroes the masked tiles after reading
  const uint32_t* dmask = nullptr;
  // (pruned 2-D path only, may be NULL): device weight sum the image is
  // divided by in pass B's epilogue (CIP_NORMALISE)
  const double* norm = nullptr;
  const uint32_t* rowbits = nullptr;  // (with dmask): the plane's tile-row bits (row_bits_kernel)
  int first = -1;                     // overwrite the image (1) or add to it (0); -1: plane 0 overwrites
  bool acc_f32 = false;               // dirty_out is the packed class's float plane accumulator
};
static int plane_to_dirty(const DirtyStage& st, const GridGeometry& g, int64_t p, double* grid, double* dirty_out,
                          hipStream_t s, const PlaneExtras& x = PlaneExtras()) {
  const uint32_t *dmask = x.dmask, *rowbits = x.rowbits;
  const int first = x.first < 0 ? p == 0 : x.first;
  hipEvent_t f0 = g_prof.mark(s);
  // 16384-point fp64 columns of a 2-D image: pass B by even / odd halves
  // (cip_fft.hip fft_cols_eo_kernel), pass A writing H in that order
  const bool eo = st.fast && fft_cols_eo(g.nv, st.npix_y, g.grid_f32 != 0, g.do_wstacking ? 1 : 0);
  if (st.fast) {
    if (!fft_rowskip()) rowbits = nullptr;
    CIP_HIP_CHECK(launch_fft_rows(grid, g.nu, g.nv, st.npix_x, st.tw_u, st.fft_h, dmask, g.mtx, rowbits != nullptr,
                                  g.grid_f32 != 0, eo, s));
  } else if (hipfftExecZ2Z(st.plan, (hipfftDoubleComplex*)grid, (hipfftDoubleComplex*)grid, HIPFFT_BACKWARD) !=
             HIPFFT_SUCCESS) {
    return set_error(CIP_EHIP, "hipfftExecZ2Z failed");
  }
  const double w_plane = g.w0 + (double)p * g.dw;
  // pass B carries the crop epilogue: it is booked under "fft"
  if (st.fast)
    CIP_HIP_CHECK(launch_fft_cols(st.fft_h, g.nv, st.npix_x, st.npix_y, st.tw_v, g.do_wstacking ? 1 : 0, dirty_out,
                                  st.cx, st.cy, st.px, st.py, w_plane, first, g.do_wstacking ? nullptr : x.norm,
                                  dmask ? rowbits : nullptr, g.grid_f32 != 0, x.acc_f32, eo, s));
  hipEvent_t f1 = g_prof.mark(s);
  g_prof.span(3, f0, f1);
  if (!st.fast && g.do_wstacking)
    CIP_HIP_CHECK(launch_wplane_accumulate(grid, g, st.npix_x, st.npix_y, st.px, st.py, w_plane, first, dirty_out,
                                           s));
  else if (!st.fast)
    CIP_HIP_CHECK(launch_crop_correct_2d(grid, g, st.npix_x, st.npix_y, st.cx, st.cy, dirty_out, s));
  g_prof.span(4, f1, g_prof.mark(s));
  return CIP_OK;
}

// after the last plane: the w-stacking correction (2-D: nothing)
static int finish_dirty(Workspace* ws, const DirtyStage& st, const cip_gridder_params& prm, const GridGeometry& g,
                        double* dirty_out, hipStream_t s, const float* acc_f32 = nullptr) {
  if (!g.do_wstacking) return CIP_OK;
  double* fwd = nullptr;
  int64_t fw_n = 0;
  double dnu = 0.0;
  if (const int rc = w_correction_table(ws, prm, g, s, &fwd, &fw_n, &dnu); rc != CIP_OK) return rc;
  CIP_HIP_CHECK(launch_wfinal_correct(dirty_out, st.npix_x, st.npix_y, st.px, st.py, st.cx, st.cy, fwd, fw_n, dnu,
                                      g.dw, 0, -1, nullptr, acc_f32, s));
  return CIP_OK;
}

// CIP_PSF: unit visibilities (vis is not read); then the rows' NULL-pointer check
static int psf_and_inputs(PlanRequest* rq, int flags) {
  if (flags & CIP_PSF) {
    rq->vis = nullptr;
    if (rq->vis_dtype != CIP_POL4I) rq->vis_dtype = CIP_C64;
  }
  if (rq->nrow > 0 && (!rq->uvw || !rq->freq || (!rq->vis && !(flags & CIP_PSF))))
    return set_error(CIP_EINVAL, "NULL input pointer");
  return CIP_OK;
}

// Grid visibilities (dense MS rows, or ragged row slices) onto nplanes
// resident accumulator planes (no zeroing: += onto what they hold), and add
// their weight sum to *sum_wgt.
// rq: the visibilities (dense rows, or rq.ragged) and the fixed parameters
// (PlanRequest::fixed). t: where they go.
struct GridTarget {
  int64_t npix_x = 0, npix_y = 0;  // the image: decides the grid's HBM layout
  int flags = 0;
  double* grids = nullptr;
  double* sum_wgt = nullptr;
  // a strip's row window (cip_grid_tiles_strip*): rows [row0, row0 + nrows) mod nv; nrows == 0: whole planes
  int64_t row0 = 0, nrows = 0;
  uint32_t* strip_bits = nullptr;  // cip_grid_tiles_strip_mask's tile_bits
};
static int grid_accumulate(PlanRequest rq, const GridTarget& t, void* hip_stream) {
  int flags = t.flags;
  double* const grids = t.grids;
  const int64_t row0 = t.row0, nrows = t.nrows;
  if (flags & ~(CIP_ACC_SINGLE | CIP_PSF | CIP_GRID_ZEROED)) return set_error(CIP_EINVAL, "unknown flags");
  if (!rq.given || !grids) return set_error(CIP_EINVAL, "NULL params or grids");
  // the flush's private-cell stores (CIP_GRID_ZEROED) write 16-byte cells:
  // planes that are only 8-byte aligned take the atomic path instead
  if (((uintptr_t)grids & 15u) != 0u) flags &= ~CIP_GRID_ZEROED;
  if (const int rc = psf_and_inputs(&rq, flags); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, true)
  Prepared pp;
  int rc = prepare(ws, rq, s, &pp);
  if (rc != CIP_OK) return rc;
  const bool transposed = grid_is_transposed(pp.g, t.npix_x, t.npix_y);
  unsigned* oob = nullptr;
  if (nrows > 0) {
    // a strip's row window (cip_grid_tiles_strip): rows [row0, row0 + nrows) mod nv
    if (!transposed) return set_error(CIP_EINVAL, "strip buffers need the pruned-FFT grid layout");
    if (row0 < 0 || row0 >= pp.g.nv || nrows > pp.g.nv) return set_error(CIP_EINVAL, "strip rows outside the grid");
    oob = buf<unsigned>(ws, "strip_oob", 1);
    if (!oob) return CIP_ENOMEM;
    CIP_HIP_CHECK(hipMemsetAsync(oob, 0, sizeof(unsigned), s));
    pp.g.row0 = row0;
    pp.g.rows = nrows;
    pp.g.oob = oob;
  }
  uint32_t* wmask = nullptr;
  if (t.strip_bits) {
    // the strip's dirty-tile bits for its masked pass A: the tiles this
    // call's flush writes (GridGeometry::wmask, exact) + the tile rows
    // receiving the previous rank's halo (after the scatter, below)
    if (pp.g.mtx % 32 != 0) return set_error(CIP_EINVAL, "tile masks need nu / 32 to be a multiple of 32 tiles");
    const int64_t words = pp.g.nplanes * pp.g.mty * (pp.g.mtx / 32);
    wmask = buf<uint32_t>(ws, "strip_wmask", words);
    if (!wmask) return CIP_ENOMEM;
    CIP_HIP_CHECK(hipMemsetAsync(wmask, 0, sizeof(uint32_t) * words, s));
    pp.g.wmask = wmask;
  }
  const GridGeometry& g = pp.g;
  const int64_t plane_elems = 2 * g.nu * g.rows;
  const int G = pp.plan.group;
  ScatterMode mode;
  mode.transposed = transposed;
  mode.zeroed = true;  // no zeroing: += onto what the planes hold
  mode.accumulate = (flags & CIP_GRID_ZEROED) == 0;
  for (int64_t q = 0; q * G < g.nplanes; ++q) {
    if (rc = scatter_plane(pp, rq, q, mode, grids + q * G * plane_elems, s); rc != CIP_OK) return rc;
  }
  if (t.sum_wgt) CIP_HIP_CHECK(launch_add_scalar(pp.red, t.sum_wgt, s));
  if (t.strip_bits) CIP_HIP_CHECK(launch_strip_mask(wmask, g, row0, g.support - 1, t.strip_bits, s));
  // the strip's dropped-cells flag comes back with the call's synchronisation
  unsigned* h_oob = nullptr;
  if (oob) {
    h_oob = (unsigned*)pinned(ws, sizeof(unsigned));
    if (!h_oob) return CIP_ENOMEM;
    CIP_HIP_CHECK(hipMemcpyAsync(h_oob, oob, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  }
  if (rc = end_call(call); rc != CIP_OK) return rc;
  if (h_oob && *h_oob != 0u)
    return set_error(CIP_ERANGE, "a visibility's footprint leaves the strip's rows (cells dropped)");
  return CIP_OK;
}

// The invert. rq: the visibilities, image and accuracy as the entry point
// received them (and a w-plane range, cip_ms2dirty_wplanes); what `flags`
// decides (w-stacking, the packed class, plan reuse) is filled here.
struct DirtyOut {
  double* dirty = nullptr;
  double* sum_wgt = nullptr;
  cip_gridder_params* params = nullptr;
};
static int ms2dirty_impl(PlanRequest rq, int flags, void* hip_stream, const DirtyOut& o) {
  const int64_t npix_x = rq.npix_x, npix_y = rq.npix_y;
  double* const dirty_out = o.dirty;
  if (flags & ~(CIP_WSTACKING | CIP_ACC_SINGLE | CIP_PSF | CIP_NORMALISE | CIP_ASYNC | CIP_PIPELINE | CIP_REUSE_PLAN))
    return set_error(CIP_EINVAL, "unknown flags");
  if ((flags & CIP_REUSE_PLAN) && (flags & CIP_PIPELINE))
    return set_error(CIP_EINVAL, "CIP_REUSE_PLAN cannot be combined with CIP_PIPELINE");
  rq.do_wstacking = (flags & CIP_WSTACKING) ? 1 : 0;
  const bool normalise = (flags & CIP_NORMALISE) != 0;
  rq.packed = (flags & CIP_ACC_SINGLE) != 0;
  rq.reuse = (flags & CIP_REUSE_PLAN) != 0;
  rq.wide_tile = true;
  if (!dirty_out) return set_error(CIP_EINVAL, "dirty_out is NULL");
  if (const int rc = psf_and_inputs(&rq, flags); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, true)
  // CIP_ASYNC | CIP_PIPELINE (resident inputs): the planner beside the previous call's scatter and FFT (PlanPipeline)
  const bool pipelined = (flags & CIP_ASYNC) && (flags & CIP_PIPELINE) && !g_prof.on;
  PlanScope plan{ws->pipeline, s};
  if (const int rc = plan.open(pipelined); rc != CIP_OK) return rc;
  Prepared pp;
  GridUse gu;
  gu.beside = !pipelined;
  int rc = prepare(ws, rq, plan.ps, &pp, &gu);
  // s waits for the plan and the side stream whatever happened (a later call
  // must not write the workspace grid while its memset is still queued)
  const int jr = plan.join(), sr = gu.pending ? join_side(ws, s) : CIP_OK;
  if (rc == CIP_OK) rc = jr != CIP_OK ? jr : sr;
  if (rc != CIP_OK) return rc;
  if (o.params) *o.params = pp.p;
  DirtyStage st;
  if (rc = dirty_stage(ws, pp.g, npix_x, npix_y, rq.px, rq.py, s, &st); rc != CIP_OK) return rc;
  pp.g.grid_f32 = gu.f32 ? 1 : 0;
  const GridGeometry& g = pp.g;
  double* const grid = gu.grid;
  const int G = pp.plan.group;
  const size_t plane_bytes = gu.bytes / (size_t)G;
  // zeroed beside the planner, or left all-zero by the previous call; dirty
  // until a masked pass A has consumed every written tile. A larger clean
  // prefix survives: the call writes only its own group's bytes
  bool clean = gu.zeroed;
  const size_t keep = ws->grid_zero.prefix(grid);
  ws->grid_zero.invalidate();
  const uint32_t* dmask = st.fast ? pp.plan.dmask : nullptr;
  // the plane groups holding planes [plane_lo, plane_hi) (the whole stack
  // unless cip_ms2dirty_wplanes); an empty range leaves a zero image
  const int64_t p_lo = g.plane_lo, p_hi = g.plane_hi;
  if (p_lo >= p_hi) CIP_HIP_CHECK(hipMemsetAsync(dirty_out, 0, sizeof(double) * npix_x * npix_y, s));
  const int64_t rb_stride = (g.mty + 31) / 32;
  const uint32_t* rowbits0 = dmask ? dmask + g.nplanes * (g.mtx * g.mty / 32) : nullptr;
  // the packed class's w planes accumulate in a float image (its own
  // precision, one rounding per plane; the final correction writes the fp64
  // image): half the per-plane read-modify-write of pass B. Only beside fp32
  // transforms of complex64 planes (launch_fft_cols refuses any other pairing).
  float* wacc = nullptr;
  if (st.fast && g.do_wstacking && g.grid_f32 && fft_f32_enabled() && p_lo < p_hi && wacc_f32_enabled()) {
    wacc = buf<float>(ws, "wacc_f32", npix_x * npix_y);
    if (!wacc) return CIP_ENOMEM;
  }
  ScatterMode mode;
  mode.transposed = st.fast;
  // pipelined calls: leave CU slots to the next call's planner (profiles/r03_ab_scatter_share.txt)
  mode.share_cus = pipelined;
  PlaneExtras x;
  x.norm = normalise ? pp.red : nullptr;
  x.acc_f32 = wacc != nullptr;
  for (int64_t q = p_lo / G; q * G < p_hi; ++q) {
    mode.zeroed = clean;
    if (rc = scatter_plane(pp, rq, q, mode, grid, s); rc != CIP_OK) return rc;
    for (int64_t p = std::max(q * G, p_lo); p < std::min<int64_t>(q * G + G, p_hi); ++p) {
      double* plane_p = (double*)((char*)grid + (size_t)(p - q * G) * plane_bytes);
      x.dmask = dmask ? dmask + p * (g.mtx * g.mty / 32) : nullptr;
      x.rowbits = rowbits0 ? rowbits0 + p * rb_stride : nullptr;
      x.first = p == p_lo;
      if (rc = plane_to_dirty(st, g, p, plane_p, wacc ? (double*)wacc : dirty_out, s, x); rc != CIP_OK) return rc;
    }
    // a group's planes outside the range were neither written (the scatter
    // skips them) nor read, so a masked pass A still leaves the group clean
    clean = dmask != nullptr;
  }
  if (rc = finish_dirty(ws, st, pp.p, g, dirty_out, s, wacc); rc != CIP_OK) return rc;
  // fused into pass B on the pruned 2-D path; a separate pass otherwise
  if (normalise && (!st.fast || g.do_wstacking))
    CIP_HIP_CHECK(launch_scale_inverse(dirty_out, npix_x * npix_y, pp.red, s));
  if (o.sum_wgt) CIP_HIP_CHECK(hipMemcpyAsync(o.sum_wgt, pp.red, sizeof(double), hipMemcpyDeviceToDevice, s));
  // CIP_ASYNC: later calls of this thread reuse the workspace (grid, planner buffers) in stream order, so
  // nothing on the host waits for it; the grid-clean mark holds in stream order too
  if (rc = end_call(call, !(flags & CIP_ASYNC)); rc != CIP_OK) return rc;
  if (clean) ws->grid_zero.mark(grid, std::max(keep, gu.bytes));
  return CIP_OK;
}

}  // namespace cip

using namespace cip;

extern "C" {

int cip_ms2dirty(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis, int vis_dtype,
                 const void* wgt, int wgt_dtype, int64_t npix_x, int64_t npix_y, double pixsize_x,
                 double pixsize_y, double epsilon, int support, int flags, void* hip_stream,
                 double* dirty_out, double* sum_wgt_out, cip_gridder_params* params_out) {
  clear_error();
  if (const int rc = public_dtype_check(vis_dtype, wgt_dtype, (flags & CIP_PSF) != 0); rc != CIP_OK) return rc;
  const PlanRequest rq = PlanRequest::image(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support)
                             .dense(uvw, nrow, freq, nchan, vis, vis_dtype, wgt, wgt_dtype);
  return ms2dirty_impl(rq, flags, hip_stream, {dirty_out, sum_wgt_out, params_out});
}

int cip_ms2dirty_wplanes(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis,
                         int vis_dtype, const void* wgt, int wgt_dtype, int64_t npix_x, int64_t npix_y,
                         double pixsize_x, double pixsize_y, double epsilon, int support, int flags,
                         int64_t plane_begin, int64_t plane_end, void* hip_stream, double* dirty_out,
                         double* sum_wgt_out, cip_gridder_params* params_out) {
  clear_error();
  if (!(flags & CIP_WSTACKING)) return set_error(CIP_EINVAL, "a w-plane range needs CIP_WSTACKING");
  if (plane_begin < 0 || plane_end < plane_begin) return set_error(CIP_EINVAL, "invalid w-plane range");
  if (const int rc = public_dtype_check(vis_dtype, wgt_dtype, (flags & CIP_PSF) != 0); rc != CIP_OK) return rc;
  PlanRequest rq = PlanRequest::image(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support)
                       .dense(uvw, nrow, freq, nchan, vis, vis_dtype, wgt, wgt_dtype);
  rq.plane_begin = plane_begin, rq.plane_end = plane_end;
  return ms2dirty_impl(rq, flags, hip_stream, {dirty_out, sum_wgt_out, params_out});
}

int cip_ms2dirty_stokes_i(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis4,
                          const uint8_t* flags4, const float* wgt4, int64_t npix_x, int64_t npix_y,
                          double pixsize_x, double pixsize_y, double epsilon, int support, int flags,
                          void* hip_stream, double* dirty_out, double* sum_wgt_out, cip_gridder_params* params_out) {
  clear_error();
  if (nrow > 0 && (!wgt4 || (!vis4 && !(flags & CIP_PSF)))) return set_error(CIP_EINVAL, "NULL vis4 or wgt4");
  if (((uintptr_t)flags4 & 3u) != 0u) return set_error(CIP_EINVAL, "flags4 must be 4-byte aligned");
  const PlanRequest rq = PlanRequest::image(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support)
                             .raw(uvw, nrow, freq, nchan, vis4, flags4, wgt4);
  return ms2dirty_impl(rq, flags, hip_stream, {dirty_out, sum_wgt_out, params_out});
}

int cip_grid_ms(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis, int vis_dtype,
                const void* wgt, int wgt_dtype, const cip_gridder_params* params, double pixsize_x, double pixsize_y,
                int64_t npix_x, int64_t npix_y, int flags, void* hip_stream, double* grids, double* sum_wgt) {
  clear_error();
  if (nrow < 0) return set_error(CIP_EINVAL, "nrow must be >= 0");
  if (!public_dtypes(vis_dtype, wgt_dtype)) return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  const PlanRequest rq = PlanRequest::fixed(params, pixsize_x, pixsize_y, flags)
                             .dense(uvw, nrow, freq, nchan, vis, vis_dtype, wgt, wgt_dtype);
  return grid_accumulate(rq, {npix_x, npix_y, flags, grids, sum_wgt}, hip_stream);
}

int cip_grid_ms_stokes_i(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis4,
                         const uint8_t* flags4, const float* wgt4, const cip_gridder_params* params,
                         double pixsize_x, double pixsize_y, int64_t npix_x, int64_t npix_y, int flags,
                         void* hip_stream, double* grids, double* sum_wgt) {
  clear_error();
  if (nrow < 0) return set_error(CIP_EINVAL, "nrow must be >= 0");
  if (nrow > 0 && (!wgt4 || (!vis4 && !(flags & CIP_PSF)))) return set_error(CIP_EINVAL, "NULL vis4 or wgt4");
  if (((uintptr_t)flags4 & 3u) != 0u) return set_error(CIP_EINVAL, "flags4 must be 4-byte aligned");
  const PlanRequest rq =
      PlanRequest::fixed(params, pixsize_x, pixsize_y, flags).raw(uvw, nrow, freq, nchan, vis4, flags4, wgt4);
  return grid_accumulate(rq, {npix_x, npix_y, flags, grids, sum_wgt}, hip_stream);
}

// the ragged arguments the three cip_grid_tiles* share
static int ragged_args_check(const int32_t* chan_start, const int32_t* chan_stop, int64_t nslices, int64_t nvis) {
  if (nslices < 0 || nvis < 0) return set_error(CIP_EINVAL, "nslices and nvis must be >= 0");
  if (nslices > 0 && (!chan_start || !chan_stop)) return set_error(CIP_EINVAL, "NULL channel ranges");
  if (nslices >= ((int64_t)1 << 32) - 1) return set_error(CIP_EINVAL, "nslices must be < 2^32 - 1");
  return CIP_OK;
}

// what stands behind the three, after their own argument checks
static int grid_tiles(const double* slice_uvw, const RaggedRows& rr, int64_t nslices, const double* freq,
                      int64_t nchan, const void* vis, int vis_dtype, const void* wgt, int wgt_dtype,
                      const cip_gridder_params* params, double pixsize_x, double pixsize_y, const GridTarget& t,
                      void* hip_stream) {
  if (!public_dtypes(vis_dtype, wgt_dtype)) return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  PlanRequest rq = PlanRequest::fixed(params, pixsize_x, pixsize_y, t.flags)
                       .dense(slice_uvw, nslices, freq, nchan, vis, vis_dtype, wgt, wgt_dtype);
  rq.ragged = &rr;
  return grid_accumulate(rq, t, hip_stream);
}

int cip_grid_tiles(const double* slice_uvw, const int32_t* chan_start, const int32_t* chan_stop, int64_t nslices,
                   const double* freq, int64_t nchan, const void* vis, int64_t nvis, int vis_dtype, const void* wgt,
                   int wgt_dtype, const cip_gridder_params* params, double pixsize_x, double pixsize_y,
                   int64_t npix_x, int64_t npix_y, int flags, void* hip_stream, double* grids, double* sum_wgt) {
  clear_error();
  if (const int rc = ragged_args_check(chan_start, chan_stop, nslices, nvis); rc != CIP_OK) return rc;
  return grid_tiles(slice_uvw, {chan_start, chan_stop, nvis}, nslices, freq, nchan, vis, vis_dtype, wgt, wgt_dtype,
                    params, pixsize_x, pixsize_y, {npix_x, npix_y, flags, grids, sum_wgt}, hip_stream);
}

int cip_grid_tiles_strip(const double* slice_uvw, const int32_t* chan_start, const int32_t* chan_stop,
                         int64_t nslices, const double* freq, int64_t nchan, const void* vis, int64_t nvis,
                         int vis_dtype, const void* wgt, int wgt_dtype, const cip_gridder_params* params,
                         double pixsize_x, double pixsize_y, int64_t npix_x, int64_t npix_y, int64_t row0,
                         int64_t nrows, int flags, void* hip_stream, double* strip, double* sum_wgt) {
  clear_error();
  if (const int rc = ragged_args_check(chan_start, chan_stop, nslices, nvis); rc != CIP_OK) return rc;
  if (nrows < 1) return set_error(CIP_EINVAL, "nrows must be >= 1");
  return grid_tiles(slice_uvw, {chan_start, chan_stop, nvis}, nslices, freq, nchan, vis, vis_dtype, wgt, wgt_dtype,
                    params, pixsize_x, pixsize_y, {npix_x, npix_y, flags, strip, sum_wgt, row0, nrows}, hip_stream);
}

int cip_grid_tiles_strip_mask(const double* slice_uvw, const int32_t* chan_start, const int32_t* chan_stop,
                              int64_t nslices, const double* freq, int64_t nchan, const void* vis, int64_t nvis,
                              int vis_dtype, const void* wgt, int wgt_dtype, const cip_gridder_params* params,
                              double pixsize_x, double pixsize_y, int64_t npix_x, int64_t npix_y, int64_t row0,
                              int64_t nrows, int flags, void* hip_stream, double* strip, double* sum_wgt,
                              uint32_t* tile_bits) {
  clear_error();
  if (const int rc = ragged_args_check(chan_start, chan_stop, nslices, nvis); rc != CIP_OK) return rc;
  if (nrows < 1) return set_error(CIP_EINVAL, "nrows must be >= 1");
  if (!tile_bits) return set_error(CIP_EINVAL, "NULL tile_bits");
  return grid_tiles(slice_uvw, {chan_start, chan_stop, nvis}, nslices, freq, nchan, vis, vis_dtype, wgt, wgt_dtype,
                    params, pixsize_x, pixsize_y, {npix_x, npix_y, flags, strip, sum_wgt, row0, nrows, tile_bits},
                    hip_stream);
}

int cip_grid_to_dirty(double* grids, const cip_gridder_params* params, int64_t npix_x, int64_t npix_y,
                      double pixsize_x, double pixsize_y, void* hip_stream, double* dirty_out) {
  clear_error();
  if (!params || !grids || !dirty_out) return set_error(CIP_EINVAL, "NULL params, grids or dirty_out");
  if (npix_x < 1 || npix_y < 1 || npix_x > params->nu || npix_y > params->nv)
    return set_error(CIP_EINVAL, "image larger than the grid");
  CIP_BEGIN_CALL(hip_stream, true)
  const GridGeometry g = geometry(*params, pixsize_x, pixsize_y);
  DirtyStage st;
  int rc = dirty_stage(ws, g, npix_x, npix_y, pixsize_x, pixsize_y, s, &st);
  if (rc != CIP_OK) return rc;
  for (int64_t p = 0; p < g.nplanes; ++p) {
    if (rc = plane_to_dirty(st, g, p, grids + p * 2 * g.nu * g.nv, dirty_out, s); rc != CIP_OK) return rc;
  }
  if (rc = finish_dirty(ws, st, *params, g, dirty_out, s); rc != CIP_OK) return rc;
  return end_call(call);
}

int cip_grid_plane(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const void* vis,
                   int vis_dtype, const void* wgt, int wgt_dtype, const cip_gridder_params* params,
                   double pixsize_x, double pixsize_y, int64_t plane, int flags, void* hip_stream,
                   double* grid_out) {
  clear_error();
  if (flags & ~CIP_ACC_SINGLE) return set_error(CIP_EINVAL, "unknown flags");
  if (!params || !grid_out) return set_error(CIP_EINVAL, "NULL params or grid_out");
  if (plane < 0 || plane >= params->nplanes) return set_error(CIP_EINVAL, "plane out of range");
  if (!public_dtypes(vis_dtype, wgt_dtype)) return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  CIP_BEGIN_CALL(hip_stream, true)
  PlanRequest rq = PlanRequest::fixed(params, pixsize_x, pixsize_y, flags)
                       .dense(uvw, nrow, freq, nchan, vis, vis_dtype, wgt, wgt_dtype);
  rq.want_group = false;  // one plane per work unit: `plane` indexes the plan's ranges
  Prepared pp;
  int rc = prepare(ws, rq, s, &pp);
  if (rc != CIP_OK) return rc;
  if (rc = scatter_plane(pp, rq, plane, ScatterMode(), grid_out, s); rc != CIP_OK) return rc;
  return end_call(call);
}

}  // extern "C"
