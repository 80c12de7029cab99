// cip_planner.hip - the tile planner on the host: make_plan (place, radix
// sort by tile, work units, bank-class order) and prepare (validation, row
// map, parameters, plan reuse) for the invert, predict and gridding drivers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cip_host.h"

namespace cip {

// ------------------------------------------------------------- planner ----
// Visibilities per scatter work unit: <= kChunkVis (64-bit fixed point) or
// kChunkVisPacked (packed class, complex64 input); multiples of kOrderWindow,
// so 2-D ordering windows never straddle chunks (w-stacking units: see
// kOrderWindow in cip_common.h).
static int64_t chunk_vis(bool packed, int64_t nu) {
  // grids of 16384+ cells per axis (C4): half-size work units - shorter slices
  // on finer cells, the scatter's tail matters more (interleaved A/B at C4:
  // scatter 4.76 vs 4.89 ms, profiles/r02_ab_c4.txt)
  return packed ? kChunkVisPacked : (nu >= 16384 ? kChunkVis / 2 : kChunkVis);
}

// sub-blocks per radix workgroup: pass 0 (place blocks of ~500 runs) and the
// dense passes (4096 runs)
static int radix_group(int pass) { return pass ? 1 : 8; }

static bool wgt_dtype_ok(int d) { return d == CIP_NONE || d == CIP_F32 || d == CIP_F64 || d == CIP_POL4I; }

// the planner's error bits (launch_freq_scale, the place pass or its
// reduction alone), read back with the run count
static int plan_error(unsigned errbits) {
  if (errbits & 4u) return set_error(CIP_EINVAL, "channel frequencies must be positive");
  if (errbits & 2u) return set_error(CIP_EINVAL, "non-finite visibility or weight");
  if (errbits & 1u)
    return set_error(CIP_ERANGE, "non-finite (u, v, w) coordinates, or w outside the w-plane stack");
  return CIP_OK;
}

// Also reduces {sum w, max |w V|} into red (device) and returns max |w V| in
// *maxabs (the place pass reads the visibilities anyway).
static int make_plan(Workspace* ws, const double* uvw, const double* fx, const RowMap& m,
                     const void* vis, int vis_dtype, const void* wgt, int wgt_dtype, double* red,
                     const GridGeometry& g, int64_t cv, hipStream_t s, PlanResult* pr, double* maxabs,
                     int group = 1) {
  const int64_t ntiles = g.ntx * g.nty * g.ntw;
  pr->ntiles = ntiles;
  pr->phases = false;
  CIP_ALLOC(tile_runs, int64_t, "tile_runs", ntiles + 1)
  CIP_ALLOC(tile_vis, int64_t, "tile_vis", ntiles + 1)
  CIP_ALLOC(tile_vis_off, int64_t, "tile_vis_off", ntiles + 1)
  CIP_ALLOC(chunk_off, int64_t, "chunk_off", 2 * ntiles + 1)
  CIP_ALLOC(err, unsigned, "err_flag", 1)  // cleared by prepare() before the frequency check
  CIP_ALLOC(scan_tmp, int64_t, "scan_tmp", scan_tmp_elems(ntiles + 1))
  const int64_t nvis = m.nvis;
  const int nblk = plan_place_blocks(nvis);
  // the bank-class order of dense rows stores 32-bit flattened indices (larger
  // inputs grid in plain tile order); ragged row slices store 64-bit
  // (row, channel) entries
  const bool ragged = m.delta != nullptr;
  const bool order = scatter_order() && (ragged || nvis < ((int64_t)1 << 32));
  uint8_t* vis_class = nullptr;
  if (order) {
    vis_class = buf<uint8_t>(ws, "vis_class", nvis);
    if (!vis_class) return CIP_ENOMEM;
  }
  CIP_ALLOC(blk_cnt, int64_t, "blk_cnt", nblk)
  CIP_ALLOC(park_key, uint32_t, "park_key", (int64_t)nblk * 4096)
  CIP_ALLOC(park_run, uint64_t, "park_run", (int64_t)nblk * 4096)
  CIP_ALLOC(partial, double, "prep_partial", 2 * nblk + kPrepFinalScratch)
  // the place pass also writes radix pass 0's histogram per place block; summed
  // per radix group of g0 blocks, its scan's last entry = runs
  const int g0 = radix_group(0), g1 = radix_group(1);
  const int64_t ng0 = (nblk + g0 - 1) / g0;
  CIP_ALLOC(hist0, int64_t, "radix_hist0", 256 * (int64_t)nblk + 1)
  CIP_ALLOC(hist0g, int64_t, "radix_hist0g", 256 * ng0 + 1)
  CIP_ALLOC(scan_h0, int64_t, "scan_hist0", scan_tmp_elems(256 * ng0 + 1))
  int key_bits = 1;
  while (key_bits < 32 && ((int64_t)1 << key_bits) < ntiles) ++key_bits;
  const int npass = (key_bits + 7) / 8;
  // packed ragged runs (RowMap::pk_runs): the lane scatter's ordered plans
  // whose radix digits stay below the length bits
  RowMap mp = m;
  mp.pk_runs = (ragged && m.pk_cbits && order && g.support <= 16 && 8 * npass <= kRunLenShift && packed_runs()) ? 1 : 0;
  CIP_HIP_CHECK(launch_plan_place(uvw, fx, mp, vis, vis_dtype, wgt, wgt_dtype, g, err, vis_class, blk_cnt, park_key,
                                  park_run, partial, hist0, s));
  CIP_HIP_CHECK(launch_prep_final(partial, nblk, red, s));
  CIP_HIP_CHECK(launch_radix_group_hist(hist0, nblk, g0, hist0g, s));
  CIP_HIP_CHECK(exclusive_scan_i64(hist0g, 256 * ng0 + 1, scan_h0, s));
  int64_t* h = nullptr;
  if (const int rc = readback(
          ws, s, {{hist0g + 256 * ng0, sizeof(int64_t)}, {err, sizeof(unsigned)}, {red + 1, sizeof(double)}}, &h);
      rc != CIP_OK)
    return rc;
  const int64_t nruns = h[0];
  std::memcpy(maxabs, &h[2], sizeof(double));
  if (const int rc = plan_error((unsigned)h[1]); rc != CIP_OK) return rc;
  pr->nruns = nruns;
  // bucket the runs by tile: stable LSD radix sort, pass 0 from the parked runs
  CIP_ALLOC(key_a, uint32_t, "sort_key_a", nruns)
  CIP_ALLOC(key_b, uint32_t, "sort_key_b", nruns)
  CIP_ALLOC(run_a, uint64_t, "sort_run_a", nruns)
  CIP_ALLOC(run_b, uint64_t, "sort_run_b", nruns)
  const int64_t nbd = radix_blocks(nruns);
  const int64_t ng1 = (nbd + g1 - 1) / g1;
  CIP_ALLOC(hist, int64_t, "radix_hist", 256 * ng1 + 1)
  CIP_ALLOC(scan_h, int64_t, "scan_hist", scan_tmp_elems(256 * ng1 + 1))
  CIP_HIP_CHECK(launch_radix_scatter(park_key, park_run, 0, blk_cnt, nblk, g0, 0, hist0g, key_a, run_a, s));
  uint32_t *kin = key_a, *kout = key_b;
  uint64_t *rin = run_a, *rout = run_b;
  for (int p = 1; p < npass; ++p) {
    CIP_HIP_CHECK(launch_radix_hist(kin, nruns, nullptr, nbd, g1, 8 * p, hist, s));
    CIP_HIP_CHECK(exclusive_scan_i64(hist, 256 * ng1 + 1, scan_h, s));
    CIP_HIP_CHECK(launch_radix_scatter(kin, rin, nruns, nullptr, nbd, g1, 8 * p, hist, kout, rout, s));
    std::swap(kin, kout);
    std::swap(rin, rout);
  }
  uint64_t* runs = rin;
  CIP_HIP_CHECK(launch_tile_offsets(kin, nruns, ntiles, tile_runs, mp.pk_runs ? kRunKeyMask : 0xffffffffu, s));
  const int64_t* tile_run_off = tile_runs;
  CIP_ALLOC(run_goff, int64_t, "run_goff", nruns + 1)
  CIP_ALLOC(scan_tmp2, int64_t, "scan_tmp2", scan_tmp_elems(nruns + 1))
  CIP_HIP_CHECK(scan_run_offsets(runs, nruns, run_goff, scan_tmp2, mp.pk_runs ? kin : nullptr, s));
  CIP_HIP_CHECK(launch_tile_vis(run_goff, tile_run_off, ntiles, tile_vis_off, tile_vis, s));
  if (g.mtx % 32 == 0 && grid_mask()) {
    // 32-cell mask tiles, whatever the plan's work tile
    CIP_ALLOC(dmask, uint8_t, "dirty_mask", g.mtx * g.mty * g.nplanes)
    // tile bits, then tile-row bits (row_bits_kernel), per plane
    CIP_ALLOC(dbits, uint32_t, "dirty_bits", g.mtx * g.mty / 32 * g.nplanes + (g.mty + 31) / 32 * g.nplanes)
    CIP_HIP_CHECK(hipMemsetAsync(dmask, 0, (size_t)(g.mtx * g.mty * g.nplanes), s));
    CIP_HIP_CHECK(launch_dirty_mask(tile_vis, g, dmask, dbits, s));
    pr->dmask = dbits;
  }
  // 2-D: the scatter's work units largest first (one tile layer, so the
  // plane's chunk range stays contiguous); w-stacking: per plane, one unit
  // sequence per uv tile over its layers feeding the plane (tile-major keys
  // make that a contiguous range), plane after plane
  const int64_t ntxy = g.ntx * g.nty;
  const bool per_plane = g.do_wstacking != 0;
  pr->group = per_plane ? group : 1;
  const int64_t ngroups = per_plane ? (g.nplanes + group - 1) / group : 1;
  const int64_t nrange = ngroups;  // chunk ranges: per plane group, or the one 2-D layer
  const int full_first = per_plane ? 0 : 1;
  CIP_ALLOC(layer_off, int64_t, "layer_off", nrange + 1)
  int64_t* pc_off = nullptr;
  if (per_plane) {
    const int64_t nentp = ngroups * ntxy;
    pc_off = buf<int64_t>(ws, "plane_chunk_cnt", nentp + 1);
    int64_t* scan_tmpp = buf<int64_t>(ws, "scan_tmp_pchunks", scan_tmp_elems(nentp + 1));
    if (!pc_off || !scan_tmpp) return CIP_ENOMEM;
    CIP_HIP_CHECK(launch_plane_chunk_counts(tile_vis_off, ntxy, g.ntw, ngroups, group, g.support, cv, pc_off, s));
    CIP_HIP_CHECK(exclusive_scan_i64(pc_off, nentp + 1, scan_tmpp, s));
    CIP_HIP_CHECK(launch_gather_i64(pc_off, ntxy, nrange + 1, layer_off, s));
  } else {
    const int64_t nent = full_first ? 2 * ntiles : ntiles;
    CIP_ALLOC(scan_tmpc, int64_t, "scan_tmp_chunks", scan_tmp_elems(2 * ntiles + 1))
    CIP_HIP_CHECK(launch_chunk_counts(tile_vis, ntiles, cv, full_first, chunk_off, s));
    CIP_HIP_CHECK(exclusive_scan_i64(chunk_off, nent + 1, scan_tmpc, s));
    CIP_HIP_CHECK(launch_gather_i64(chunk_off, full_first ? nent : ntiles, nrange + 1, layer_off, s));
  }
  // bank-class ordering windows: the same split with kOrderWindow, per tile key
  CIP_ALLOC(win_off, int64_t, "win_off", ntiles + 1)
  if (order) {
    CIP_HIP_CHECK(launch_chunk_counts(tile_vis, ntiles, kOrderWindow, 0, win_off, s));
    CIP_HIP_CHECK(exclusive_scan_i64(win_off, ntiles + 1, scan_tmp, s));
  }
  int64_t* hl = nullptr;
  if (const int rc = readback(ws, s,
                              {{layer_off, sizeof(int64_t) * (nrange + 1)},
                               {order ? win_off + ntiles : nullptr, sizeof(int64_t)}},
                              &hl);
      rc != CIP_OK)
    return rc;
  pr->plane_chunk_off.assign(hl, hl + nrange + 1);
  const int64_t nwin = order ? hl[nrange + 1] : 0;
  pr->nchunks = pr->plane_chunk_off.back();
  CIP_ALLOC(chunks, Chunk, "chunks", pr->nchunks)
  if (per_plane)
    CIP_HIP_CHECK(launch_plane_chunk_emit(tile_vis_off, pc_off, run_goff, tile_runs, ntxy, g.ntw, ngroups, group,
                                          g.support, cv, pr->nchunks, chunks, s));
  else
    CIP_HIP_CHECK(launch_chunk_emit(tile_vis_off, tile_vis, chunk_off, run_goff, tile_runs, ntiles, cv, full_first,
                                    pr->nchunks, chunks, s));
  pr->runs = runs;
  pr->run_goff = run_goff;
  pr->tile_run_off = tile_runs;
  pr->chunks = chunks;
  if (order && nwin > 0) {
    CIP_ALLOC(windows, Chunk, "windows", nwin)
    CIP_HIP_CHECK(launch_chunk_emit(tile_vis_off, tile_vis, win_off, run_goff, tile_runs, ntiles, kOrderWindow, 0, nwin,
                                    windows, s));
    CIP_ALLOC(perm, uint32_t, "perm", ragged ? 2 * nvis : nvis)
    const bool ph = row_phases() && order_phases_ok(mp, g.support);
    CIP_HIP_CHECK(launch_order(vis_class, mp, runs, run_goff, windows, nwin, perm, ph ? g.support : 0, s));
    pr->phases = ph;
    pr->perm = perm;
  }
  return CIP_OK;
}

int prepare(Workspace* ws, const PlanRequest& rq, hipStream_t s, Prepared* out, GridUse* grid_out) {
  const int64_t nrow = rq.nrow, nchan = rq.nchan;
  const int vis_dtype = rq.vis_dtype;
  const bool packed = rq.packed;
  const RaggedRows* ragged = rq.ragged;
  ws->pipeline.planner_starts();
  if (!vis_dtype_ok(vis_dtype)) return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  if (!wgt_dtype_ok(rq.wgt_dtype)) return set_error(CIP_EINVAL, "wgt dtype must be float32, float64 or none");
  const int wgt_dtype = rq.wgt == nullptr ? CIP_NONE : rq.wgt_dtype;
  // raw linear-feed columns: visibilities and weights come as one (internal) pair
  if ((vis_dtype == CIP_POL4I) != (wgt_dtype == CIP_POL4I))
    return set_error(CIP_EINVAL, "raw linear-feed visibilities need their raw weights");
  if (nrow < 0 || nchan < 1 || nchan > 65535) return set_error(CIP_EINVAL, "need 1 <= nchan <= 65535, nrow >= 0");
  if (nrow >= ((int64_t)1 << 32)) return set_error(CIP_EINVAL, "nrow must be < 2^32");
  CIP_ALLOC(fx, double, "fx", nchan)
  CIP_ALLOC(red, double, "red", 4)
  // the planner's error bits: cleared here, read back with the run count
  CIP_ALLOC(err, unsigned, "err_flag", 1)
  CIP_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(unsigned), s));
  CIP_HIP_CHECK(launch_freq_scale(rq.freq, nchan, fx, err, s));
  // the frequency range on the host only where the w range needs it (the
  // positivity check otherwise travels as error bit 2 to the planner's
  // readback: one host synchronisation less per 2-D call)
  const bool host_fx = nrow == 0 || (rq.do_wstacking && rq.given == nullptr);
  double fxmin = 0.0, fxmax = 0.0;
  if (host_fx) {
    double* h = nullptr;
    if (const int rc = readback(ws, s, {{fx, sizeof(double) * nchan}}, &h); rc != CIP_OK) return rc;
    fxmin = h[0];
    fxmax = h[0];
    for (int64_t c = 1; c < nchan; ++c) {
      fxmin = std::fmin(fxmin, h[c]);
      fxmax = std::fmax(fxmax, h[c]);
    }
    if (!(fxmin > 0.0) || !std::isfinite(fxmax)) return set_error(CIP_EINVAL, "channel frequencies must be positive");
  }
  RowMap& m = out->m;
  m.nchan = nchan;
  m.inv_nchan = 1.0 / (double)nchan;
  m.delta = nullptr;
  m.off = nullptr;
  m.seg_row = nullptr;
  m.nrow = 0;
  m.pk_cbits = m.pk_rbits = 0;
  m.flags4 = vis_dtype == CIP_POL4I ? rq.flags4 : nullptr;
  m.nvis = nrow * nchan;
  if (ragged) {
    if (ragged->nvis < 0 || ragged->nvis >= ((int64_t)1 << 40)) return set_error(CIP_EINVAL, "bad visibility count");
    m.nvis = ragged->nvis;
    if (nrow > 0) {
      int64_t* off = buf<int64_t>(ws, "ragged_off", nrow + 1);
      int64_t* delta = buf<int64_t>(ws, "ragged_delta", nrow);
      uint32_t* seg_row = buf<uint32_t>(ws, "ragged_seg_row", (ragged->nvis + 63) / 64 + 1);
      int64_t* scan_tmp = buf<int64_t>(ws, "ragged_scan", scan_tmp_elems(nrow + 1));
      unsigned* rerr = buf<unsigned>(ws, "ragged_err", 1);
      if (!off || !delta || !seg_row || !scan_tmp || !rerr) return CIP_ENOMEM;
      CIP_HIP_CHECK(hipMemsetAsync(rerr, 0, sizeof(unsigned), s));
      CIP_HIP_CHECK(launch_ragged_lengths(ragged->chan_start, ragged->chan_stop, nrow, nchan, off, rerr, s));
      CIP_HIP_CHECK(exclusive_scan_i64(off, nrow + 1, scan_tmp, s));
      int64_t* hr = nullptr;
      if (const int rc = readback(ws, s, {{off + nrow, sizeof(int64_t)}, {rerr, sizeof(unsigned)}}, &hr); rc != CIP_OK)
        return rc;
      if ((unsigned)hr[1] != 0u) return set_error(CIP_EINVAL, "row slice channel range outside [0, nchan)");
      if (hr[0] != ragged->nvis) return set_error(CIP_EINVAL, "visibility count differs from the row slices' total");
      CIP_HIP_CHECK(launch_ragged_expand(off, ragged->chan_start, nrow, delta, seg_row, s));
      m.delta = delta;
      m.off = off;
      m.seg_row = seg_row;
      m.nrow = nrow;
      // ordered-stream entries (index, row, channel) when they fit 64 bits
      const int cb = index_bits(nchan), rb = index_bits(nrow), ib = index_bits(ragged->nvis);
      if (cb + rb + ib <= 64 && ragged_pack()) {
        m.pk_cbits = cb;
        m.pk_rbits = rb;
      }
    }
  }
  // CIP_REUSE_PLAN: the previous plan, if it was made for this geometry (its
  // parameters then also stand in for the w range: same uvw by the caller's
  // promise)
  const std::vector<double> key = {(double)nrow, (double)nchan, (double)rq.npix_x, (double)rq.npix_y, rq.px, rq.py,
                                   rq.epsilon, (double)rq.support, (double)rq.do_wstacking, (double)packed,
                                   rq.given ? 1.0 : 0.0, rq.want_group ? 1.0 : 0.0, (double)rq.plane_begin,
                                   (double)rq.plane_end};
  // the saved plan's work tile is part of the match (below, once this call's
  // own is known); a saved 32 x 32 plan - a predict's - also serves an invert
  // whose rule would pick a larger tile: it then runs the 32 x 32 scatter
  const bool reusable = rq.reuse && !ragged && rq.given == nullptr && ws->saved_valid && ws->saved_key == key;
  const cip_gridder_params* given = reusable ? &ws->saved_p : rq.given;
  double wmin = 0.0, wmax = 0.0;
  if (rq.do_wstacking && nrow > 0 && given == nullptr) {
    const int nb = 256;
    CIP_ALLOC(wpart, double, "w_partial", 2 * nb)
    CIP_HIP_CHECK(launch_w_range(rq.uvw, nrow, fxmin, fxmax, wpart, nb, s));
    double* hw = nullptr;
    if (const int rc = readback(ws, s, {{wpart, sizeof(double) * 2 * nb}}, &hw); rc != CIP_OK) return rc;
    wmin = INFINITY;
    wmax = -INFINITY;
    for (int i = 0; i < nb; ++i) {
      wmin = std::fmin(wmin, hw[2 * i]);
      wmax = std::fmax(wmax, hw[2 * i + 1]);
    }
  }
  if (given) {
    out->p = *given;
  } else {
    const int rc = choose(rq.npix_x, rq.npix_y, rq.px, rq.py, rq.epsilon, rq.support, rq.do_wstacking, wmin, wmax,
                          &out->p);
    if (rc != CIP_OK) return rc;
  }
  // the plan's work tile: larger than 32 x 32 only on the 2-D ordered-stream
  // lane path of an invert (make_plan orders dense rows of < 2^32 visibilities)
  const bool tile_ok = rq.wide_tile && !ragged && scatter_order() && m.nvis < ((int64_t)1 << 32);
  TileShape shape = scatter_tile_shape(out->p, packed, tile_ok);
  const TileShape saved_shape{ws->saved_plan.tx_shift, ws->saved_plan.ty_shift};
  const bool saved32 = saved_shape.tx_shift == kTileShift && saved_shape.ty_shift == kTileShift;
  const bool reusing =
      reusable && ((saved_shape.tx_shift == shape.tx_shift && saved_shape.ty_shift == shape.ty_shift) || saved32);
  // (a matching key with another tile - a predict after a 64-tile invert -
  // plans afresh; 2-D only, where the saved parameters are this call's own)
  if (reusing) shape = saved_shape;
  out->g = geometry(out->p, rq.px, rq.py, shape);
  if (rq.plane_end >= 0) {
    // a range of the w-plane stack (cip_ms2dirty_wplanes)
    if (rq.plane_begin < 0 || rq.plane_begin > rq.plane_end || rq.plane_end > out->p.nplanes)
      return set_error(CIP_EINVAL, "w-plane range outside [0, nplanes]");
    out->g.plane_lo = rq.plane_begin;
    out->g.plane_hi = rq.plane_end;
  }
  // tile keys are 32-bit ((iy0 / T) ntx + ix0 / T) ntw + iw0 (cip_plan.hip):
  // a larger key space would wrap and mis-sort the runs
  if ((double)out->g.ntx * (double)out->g.nty * (double)out->g.ntw >= 4294967295.0)
    return set_error(CIP_EINVAL, "grid tiles x w layers exceed the 32-bit tile key space");
  if (packed && vis_dtype != CIP_C64 && vis_dtype != CIP_POL4I)
    return set_error(CIP_EINVAL, "single-precision accumulation needs complex64 visibilities");
  if (packed && out->g.support > 16)
    return set_error(CIP_EINVAL, "single-precision accumulation supports kernel supports <= 16");
  out->packed = packed;
  out->fixed_scale = 1.0;
  out->fx = fx;
  out->red = red;
  const int group = rq.want_group ? wstack_group(out->g, packed) : 1;
  if (grid_out) {
    // the grid is known now: its first plane group (sized for complex128 cells
    // whatever the cell type), zeroed beside the planner unless left clean
    GridUse& u = *grid_out;
    const size_t cells = (size_t)(2 * out->g.nu * out->g.nv) * (size_t)group;
    u.f32 = grid_planes_f32(packed, out->g, rq.npix_x, rq.npix_y);
    u.bytes = (u.f32 ? sizeof(float) : sizeof(double)) * cells;
    u.grid = grid_buffer(ws, sizeof(double) * cells);
    if (!u.grid) return CIP_ENOMEM;
    u.zeroed = ws->grid_zero.covers(u.grid, u.bytes);
    if (!u.zeroed && u.beside) {
      if (const int zr = zero_on_side(ws, u.grid, u.bytes, s); zr != CIP_OK) return zr;
      u.zeroed = u.pending = true;
    }
  }
  hipEvent_t e_prep = g_prof.mark(s);
  g_prof.span(0, g_prof.pool.empty() ? nullptr : g_prof.pool[0], e_prep);
  if (nrow == 0 || m.nvis == 0) {
    CIP_HIP_CHECK(hipMemsetAsync(red, 0, 2 * sizeof(double), s));
    out->plan = PlanResult();
    out->plan.plane_chunk_off.assign((out->g.do_wstacking ? out->g.nplanes : 1) + 1, 0);  // group 1
    return CIP_OK;
  }
  double maxabs = 0.0;
  int rc;
  if (reusing) {
    // the plan's buffers are read-only here; only the weight reduction runs
    // (it places nothing, so it never sets error bit 0)
    const int nblk = plan_place_blocks(m.nvis);
    CIP_ALLOC(partial, double, "prep_partial_reuse", 2 * nblk + kPrepFinalScratch)
    CIP_HIP_CHECK(launch_prep_reduce(m, rq.vis, vis_dtype, rq.wgt, wgt_dtype, out->g, err, partial, s));
    CIP_HIP_CHECK(launch_prep_final(partial, nblk, red, s));
    unsigned* h = nullptr;
    if (rc = readback(ws, s, {{err, sizeof(unsigned)}, {red + 1, sizeof(double)}}, &h); rc != CIP_OK) return rc;
    std::memcpy(&maxabs, (double*)h + 1, sizeof(double));
    if (rc = plan_error(h[0]); rc != CIP_OK) return rc;
    out->plan = ws->saved_plan;
  } else {
    ws->saved_valid = false;
    rc = make_plan(ws, rq.uvw, fx, m, rq.vis, vis_dtype, rq.wgt, wgt_dtype, red, out->g, chunk_vis(packed, out->g.nu),
                   s, &out->plan, &maxabs, group);
    out->plan.tx_shift = out->g.tx_shift;
    out->plan.ty_shift = out->g.ty_shift;
    if (rc == CIP_OK && !ragged) {
      ws->saved_key = key;
      ws->saved_p = out->p;
      ws->saved_plan = out->plan;
      ws->saved_valid = true;
    }
  }
  g_prof.span(1, e_prep, g_prof.mark(s));
  if (rc != CIP_OK) return rc;
  if (!std::isfinite(maxabs)) return set_error(CIP_EINVAL, "non-finite visibility or weight");
  // fixed point: max contribution <= 2^kFixedBits, or 2^kPackedBits for a
  // full packed chunk (the scatter raises it for shorter chunks)
  int e2 = 0;
  if (maxabs > 0.0) std::frexp(maxabs, &e2);  // maxabs < 2^e2
  out->fixed_scale = std::ldexp(1.0, (packed ? kPackedBits : kFixedBits) - e2);
  g_prof.counts[0] = m.nvis;
  g_prof.counts[1] = out->plan.nruns;
  g_prof.counts[2] = out->plan.nchunks;
  g_prof.counts[3] = out->g.nplanes;
  return rc;
}

}  // namespace cip
