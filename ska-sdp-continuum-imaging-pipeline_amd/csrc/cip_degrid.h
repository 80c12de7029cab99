// cip_degrid.h - the degridder of cip_dirty2ms (predict: the transpose of the
// scatter, ducc0.wgridder.dirty2ms), as device templates. cip_degrid_w.hip
// instantiates launch_degrid_w<W> once per kernel support W (one translation
// unit each, compiled in parallel); launch_degrid (cip_degrid.hip) dispatches
// on W.
//
// Degrid design: one 256-thread workgroup per Chunk of the
// scatter's plan (<= kChunkVis visibilities of one T x T grid tile, walked in
// plain tile order through the row slices). The tile's (T+W-1)^2 patch of the
// forward-transformed plane(s) is staged into LDS as 16-byte complex128 cells;
// each lane owns one visibility at a time, places it with place_vis (the
// planner's arithmetic, bit for bit), evaluates the 2 x W kernel values and
// gathers sum_i ku[i] (sum_j kv[j] cell(i, j)) in fp64, row sums first. No LDS
// atomics, no MFMA, no floating-point atomics on the visibilities: every
// visibility is written by exactly one lane of one unit per launch, so two
// identical calls give identical bits.
#pragma once
#include "cip_internal.h"

namespace cip {

constexpr int kDegridThreads = 256;
constexpr int kDegridRunBatch = 256;

__device__ __forceinline__ double degrid_weight(const DegridOut& o, int64_t idx) {
  if (o.wgt_dtype == CIP_F32) return (double)((const float*)o.wgt)[idx];
  if (o.wgt_dtype == CIP_F64) return ((const double*)o.wgt)[idx];
  return 1.0;
}

// vis_io[idx] = wt (re, im) or -= wt (re, im). The product is rounded before
// the subtraction (no contraction): vis - wt * model as two fp64 operations,
// whatever the output dtype.
__device__ __forceinline__ void degrid_store(const DegridOut& o, int64_t idx, double wt, double re, double im) {
#pragma clang fp contract(off)
  if (o.subtract && wt == 0.0) return;
  const double mr = wt == 0.0 ? 0.0 : wt * re, mi = wt == 0.0 ? 0.0 : wt * im;
  if (o.vis_dtype == CIP_C64) {
    float2* p = (float2*)o.vis_io + idx;
    if (o.subtract) {
      const float2 v = *p;
      *p = make_float2((float)((double)v.x - mr), (float)((double)v.y - mi));
    } else {
      *p = make_float2((float)mr, (float)mi);
    }
  } else {
    double2* p = (double2*)o.vis_io + idx;
    if (o.subtract) {
      const double2 v = *p;
      *p = make_double2(v.x - mr, v.y - mi);
    } else {
      *p = make_double2(mr, mi);
    }
  }
}

// What one visibility needs, loaded one iteration ahead of its use (as the
// scatter's fetch_vis: the run that holds tile-order position q, then its row
// and channel).
struct DegridFetch {
  double u, v, w, fx, wt;
  int64_t idx;
};

__device__ __forceinline__ void degrid_fetch(int64_t q, const int64_t* s_voff, const uint64_t* s_run, int nst,
                                             const double* __restrict__ uvw, const double* __restrict__ fx,
                                             const RowMap& m, const DegridOut& o, bool want_wt, DegridFetch& f) {
  int lo = 0, hi = nst - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_voff[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t rec = s_run[lo];
  const int64_t irow = (int64_t)(rec >> 32);
  const int64_t c = (int64_t)((rec >> 16) & 0xffff) + (q - s_voff[lo]);
  f.idx = vis_index(m, irow, c);
  f.u = uvw[3 * irow];
  f.v = uvw[3 * irow + 1];
  f.w = uvw[3 * irow + 2];
  f.fx = fx[c];
  f.wt = want_wt ? degrid_weight(o, f.idx) : 1.0;
}

// One visibility against the unit's staged patch(es). G > 1 (w-stacking): the
// unit holds planes plane .. plane + G - 1 (G patches, P * P cells apart); the
// visibility is placed and its u, v, w kernels are evaluated once for all.
template <int W, bool WSTACK, int G>
__device__ __forceinline__ void degrid_fetched(const DegridFetch& f, const GridGeometry& g, int64_t plane, int64_t X0,
                                               int64_t Y0, const double2* patch, const DegridOut& o) {
  constexpr int T = kTile;
  constexpr int P = T + W - 1;
  int64_t ix0, iy0, iw0;
  double yu, yv, yw;
  if (!place_vis(f.u, f.v, f.w, f.fx, g, &ix0, &yu, &iy0, &yv, &iw0, &yw)) return;  // the planner raised
  const int64_t lx = ix0 - X0, ly = iy0 - Y0;
  if (lx < 0 || lx >= T || ly < 0 || ly >= T) return;  // never for a consistent plan
  if (!WSTACK && f.wt == 0.0) {
    degrid_store(o, f.idx, 0.0, 0.0, 0.0);
    return;
  }
  double ku[W], kv[W];
  eval_kernel<W>(yu, ku);
  eval_kernel<W>(yv, kv);
  const double2* base = patch + (lx * P + ly);
  // sum_i ku[i] (sum_j kv[j] cell(i, j)): one 16-byte LDS read per tap
  auto gather = [&](const double2* b, double& re, double& im) {
    re = 0.0;
    im = 0.0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      double rr = 0.0, ri = 0.0;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double2 c = b[i * P + j];
        rr = fma(kv[j], c.x, rr);
        ri = fma(kv[j], c.y, ri);
      }
      re = fma(ku[i], rr, re);
      im = fma(ku[i], ri, im);
    }
  };
  if constexpr (!WSTACK) {
    double re, im;
    gather(base, re, im);
    degrid_store(o, f.idx, f.wt, re, im);
  } else {
    double kwv[W];
    eval_kernel<W>(yw, kwv);
    double ar = 0.0, ai = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int64_t kw = plane + k - iw0;
      if (kw < 0 || kw >= W || plane + k >= g.nplanes) continue;  // the visibility is not fed by plane + k
      double sel = 0.0;
#pragma unroll
      for (int q = 0; q < W; ++q) sel = (q == kw) ? kwv[q] : sel;
      double re, im;
      gather(base + k * P * P, re, im);
      ar = fma(sel, re, ar);
      ai = fma(sel, im, ai);
    }
    // the planes feeding a visibility, iw0 .. iw0 + W - 1, meet the groups in
    // ascending order: the first one is the group that holds plane iw0
    double2* a = o.acc + f.idx;
    if (iw0 >= plane) {
      *a = make_double2(ar, ai);
    } else {
      const double2 v = *a;
      *a = make_double2(v.x + ar, v.y + ai);
    }
  }
}

// planes: the unit's G transformed planes, (nu, nv) complex128 row-major
// (g[x][y]), nu * nv cells apart, plane `plane` first.
template <int W, bool WSTACK, int G>
__global__ __launch_bounds__(kDegridThreads) void degrid_kernel(
    const double* __restrict__ uvw, const double* __restrict__ fx, RowMap m, const uint64_t* __restrict__ runs,
    const int64_t* __restrict__ run_goff, const Chunk* __restrict__ chunks, int64_t chunk_begin, GridGeometry g,
    int64_t plane, const double2* __restrict__ planes, DegridOut o) {
  constexpr int T = kTile;
  constexpr int P = T + W - 1;
  constexpr int NT = kDegridThreads;
  __shared__ double2 patch[G * P * P];
  __shared__ int64_t s_voff[kDegridRunBatch + 1];
  __shared__ uint64_t s_run[kDegridRunBatch];

  const Chunk ch = chunks[chunk_begin + blockIdx.x];
  int64_t X0, Y0;
  tile_origin(ch.tile, g, &X0, &Y0);
  // stage the patch: cell (lx, ly) <- plane[(X0 + lx) mod nu][(Y0 + ly) mod nv]
  // (lanes along y, the planes' contiguous axis); planes past the stack stay
  // unread (degrid_fetched skips them)
  const int nu = (int)g.nu, nv = (int)g.nv;
  for (int cell = threadIdx.x; cell < P * P; cell += NT) {
    const int gx = ((int)X0 + cell / P) % nu, gy = ((int)Y0 + cell % P) % nv;
    const int64_t off = (int64_t)gx * nv + gy;
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (plane + k < g.nplanes) patch[k * P * P + cell] = planes[(int64_t)k * g.nu * g.nv + off];
  }
  const bool want_wt = !WSTACK && o.wgt_dtype != CIP_NONE;
  const int64_t rb = ch.last_run + 1;  // (a w-stacking unit spans several tile keys)
  int64_t r = ch.first_run;
  int64_t v = ch.g0;
  while (v < ch.g1 && r < rb) {
    const int nst = (int)((rb - r) < kDegridRunBatch ? (rb - r) : kDegridRunBatch);
    __syncthreads();  // (first pass: also the patch)
    for (int k = threadIdx.x; k <= nst; k += NT) {
      s_voff[k] = run_goff[r + k];
      if (k < nst) s_run[k] = runs[r + k];
    }
    __syncthreads();
    const int64_t bend = ch.g1 < s_voff[nst] ? ch.g1 : s_voff[nst];
    // software pipeline: fetch visibility q + 256 while q gathers
    int64_t q = v + threadIdx.x;
    bool have = q < bend;
    DegridFetch cur;
    if (have) degrid_fetch(q, s_voff, s_run, nst, uvw, fx, m, o, want_wt, cur);
    while (have) {
      const int64_t qn = q + NT;
      const bool hn = qn < bend;
      DegridFetch nxt;
      if (hn) degrid_fetch(qn, s_voff, s_run, nst, uvw, fx, m, o, want_wt, nxt);
      degrid_fetched<W, WSTACK, G>(cur, g, plane, X0, Y0, patch, o);
      cur = nxt;
      q = qn;
      have = hn;
    }
    v = bend;
    r += nst;
  }
}

// group: w planes per work unit (the plan's: 1 in 2-D, 1 .. 3 in w-stacking)
template <int W>
hipError_t launch_degrid_w(const DegridLaunch& a, dim3 gd, hipStream_t s) {
  const PlanView& p = a.plan;
  auto launch = [&](auto wstack, auto group) {
    degrid_kernel<W, decltype(wstack)::value, decltype(group)::value><<<gd, dim3(kDegridThreads), 0, s>>>(
        p.uvw, p.fx, p.m, p.runs, p.run_goff, p.chunks, a.chunk_begin, a.g, a.plane, (const double2*)a.planes, a.out);
    return hipGetLastError();
  };
  if (!a.g.do_wstacking) {
    if (a.group != 1 || a.out.acc) return hipErrorInvalidValue;
    return launch(std::false_type{}, int_tag<1>{});
  }
  if (!a.out.acc) return hipErrorInvalidValue;
  return dispatch_int<1, 2, 3>(a.group, hipErrorInvalidValue,
                               [&](auto group) { return launch(std::true_type{}, group); });
}

}  // namespace cip
