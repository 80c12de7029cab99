// cip_predict.hip - the predict (degridding) driver: cip_dirty2ms.
#include <algorithm>
#include <cmath>

#include "cip_host.h"

using namespace cip;

extern "C" {

// Predict: the transpose of ms2dirty_impl's pipeline, run backwards - prepare
// the image, zero-pad it into grid planes, forward FFT, degrid through the
// scatter's tile plan.
int cip_dirty2ms(const double* uvw, int64_t nrow, const double* freq, int64_t nchan, const double* dirty,
                 int64_t npix_x, int64_t npix_y, double pixsize_x, double pixsize_y, double epsilon, int support,
                 int flags, const void* wgt, int wgt_dtype, void* hip_stream, void* vis_io, int vis_dtype,
                 cip_gridder_params* params_out) {
  clear_error();
  if (flags & CIP_ACC_SINGLE)
    return set_error(CIP_EINVAL, "cip_dirty2ms: CIP_ACC_SINGLE is not supported (the degridder is fp64)");
  if (flags & CIP_PSF) return set_error(CIP_EINVAL, "cip_dirty2ms: CIP_PSF has no meaning for a predict");
  if (flags & CIP_NORMALISE) return set_error(CIP_EINVAL, "cip_dirty2ms: CIP_NORMALISE has no meaning for a predict");
  if (flags & (CIP_ASYNC | CIP_PIPELINE))
    return set_error(CIP_EINVAL, "cip_dirty2ms: CIP_ASYNC / CIP_PIPELINE are not supported (the call is synchronous)");
  if (flags & ~(CIP_WSTACKING | CIP_REUSE_PLAN | CIP_SUBTRACT)) return set_error(CIP_EINVAL, "unknown flags");
  if (const int rc = public_dtype_check(vis_dtype, wgt_dtype, false); rc != CIP_OK) return rc;
  if (wgt == nullptr) wgt_dtype = CIP_NONE;
  if (support > 16) return set_error(CIP_EINVAL, "cip_dirty2ms: support must be an even number in [4, 16]");
  if (!dirty) return set_error(CIP_EINVAL, "dirty is NULL");
  if (nrow < 0 || nchan < 1 || nchan > 65535) return set_error(CIP_EINVAL, "need 1 <= nchan <= 65535, nrow >= 0");
  if (nrow > 0 && (!uvw || !freq || !vis_io)) return set_error(CIP_EINVAL, "NULL input pointer");
  const int do_wstacking = (flags & CIP_WSTACKING) ? 1 : 0;
  if (nrow == 0) {
    // nothing to predict: the parameters of an empty w range, no device work
    cip_gridder_params p;
    const int rc = choose(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support, do_wstacking, 0.0, 0.0, &p);
    if (rc == CIP_OK && params_out) *params_out = p;
    return rc;
  }
  CIP_BEGIN_CALL(hip_stream, true)
  ws->pipeline.rewind();
  // the invert's planner on unit visibilities (vis == NULL, as a PSF call): the
  // same placement, tiles and work units, and the same CIP_REUSE_PLAN key as a
  // fp64-class cip_ms2dirty of this geometry
  PlanRequest rq = PlanRequest::image(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support)
                       .dense(uvw, nrow, freq, nchan, nullptr, CIP_C64, wgt, wgt_dtype);
  rq.do_wstacking = do_wstacking;
  rq.reuse = (flags & CIP_REUSE_PLAN) != 0;
  Prepared pp;
  int rc = prepare(ws, rq, s, &pp);
  if (rc != CIP_OK) return rc;
  if (params_out) *params_out = pp.p;
  const GridGeometry& g = pp.g;
  double *cx = nullptr, *cy = nullptr;
  if (rc = correction_vectors(ws, g, npix_x, npix_y, s, &cx, &cy); rc != CIP_OK) return rc;
  double* fwd = nullptr;
  int64_t fw_n = 0;
  double fw_dnu = 0.0;
  if (g.do_wstacking)
    if (rc = w_correction_table(ws, pp.p, g, s, &fwd, &fw_n, &fw_dnu); rc != CIP_OK) return rc;
  hipfftHandle plan;
  if (rc = fft_plan(ws, g.nu, g.nv, s, &plan); rc != CIP_OK) return rc;
  const int G = pp.plan.group;
  const int64_t plane_cells = g.nu * g.nv;
  // the invert's grid buffer, borrowed: it holds dense FFT output afterwards,
  // so the invert's all-zero promise about it ends here
  double* planes = grid_buffer(ws, sizeof(double) * (size_t)(2 * plane_cells * G));
  if (!planes) return CIP_ENOMEM;
  ws->grid_zero.invalidate();
  CIP_ALLOC(image, double, "degrid_image", npix_x * npix_y)
  const int64_t nvis = pp.m.nvis;
  DegridOut o;
  o.vis_io = vis_io;
  o.vis_dtype = vis_dtype;
  o.wgt = wgt;
  o.wgt_dtype = wgt_dtype;
  o.subtract = (flags & CIP_SUBTRACT) ? 1 : 0;
  o.acc = nullptr;
  if (g.do_wstacking) {
    // the plane groups' shares meet in a complex128 accumulator: the output
    // itself when it is complex128 and holds no data to subtract from
    if (vis_dtype == CIP_C128 && !o.subtract) {
      o.acc = (double2*)vis_io;
    } else {
      o.acc = (double2*)buf<double>(ws, "degrid_acc", 2 * nvis);
      if (!o.acc) return CIP_ENOMEM;
    }
  }
  hipEvent_t c0 = g_prof.mark(s);
  CIP_HIP_CHECK(launch_degrid_image(dirty, npix_x, npix_y, pixsize_x, pixsize_y, cx, cy, fwd, fw_n, fw_dnu, g.dw, image,
                                    s));
  g_prof.span(4, c0, g_prof.mark(s));
  const int64_t ngroups = (int64_t)pp.plan.plane_chunk_off.size() - 1;
  for (int64_t q = 0; q < ngroups; ++q) {
    const int64_t p0 = q * G;
    const int np = (int)std::min<int64_t>(G, g.nplanes - p0);
    const int64_t cb = pp.plan.plane_chunk_off[q], ce = pp.plan.plane_chunk_off[q + 1];
    if (ce <= cb) continue;  // no visibility is fed by this group
    hipEvent_t a = g_prof.mark(s);
    CIP_HIP_CHECK(launch_degrid_pad(image, npix_x, npix_y, pixsize_x, pixsize_y, g, g.w0 + (double)p0 * g.dw, np,
                                    planes, s));
    hipEvent_t b = g_prof.mark(s);
    g_prof.span(4, a, b);
    for (int k = 0; k < np; ++k) {
      hipfftDoubleComplex* pl = (hipfftDoubleComplex*)(planes + 2 * plane_cells * k);
      if (hipfftExecZ2Z(plan, pl, pl, HIPFFT_FORWARD) != HIPFFT_SUCCESS)
        return set_error(CIP_EHIP, "hipfftExecZ2Z failed");
    }
    hipEvent_t c = g_prof.mark(s);
    g_prof.span(3, b, c);
    DegridLaunch dg;
    dg.plan.uvw = uvw, dg.plan.fx = pp.fx, dg.plan.m = pp.m;
    dg.plan.runs = pp.plan.runs, dg.plan.run_goff = pp.plan.run_goff, dg.plan.chunks = pp.plan.chunks;
    dg.chunk_begin = cb, dg.nchunks = ce - cb;
    dg.g = g, dg.plane = p0, dg.planes = planes;
    dg.support = g.support, dg.group = G, dg.out = o;
    CIP_HIP_CHECK(launch_degrid(dg, s));
    g_prof.span(2, c, g_prof.mark(s));
    g_prof.counts[4] += 1;
  }
  if (o.acc) {
    hipEvent_t a = g_prof.mark(s);
    CIP_HIP_CHECK(launch_degrid_finish(o, nvis, s));
    g_prof.span(2, a, g_prof.mark(s));
  }
  return end_call(call);
}

}  // extern "C"
