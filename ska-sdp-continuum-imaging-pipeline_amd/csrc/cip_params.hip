// cip_params.hip - gridding parameters on the host: the ES kernel tables and
// the kernel's Fourier transform, parameter choice, the grid geometry, the
// correction tables, and the table of CIP_* switches.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cip_host.h"

namespace cip {

// ------------------------------------------------------------ kernels ----
// Host copies of the kernel coefficient tables (same data as the device side).
struct HostKernel {
  int W, D;
  double beta;
  const double* coef;  // [W/2][D+1]
};

#define CIP_HOST_TABLE(WW)                                                          \
  static const double host_coef_##WW[WW / 2][CIP_ES_DEGREE_##WW + 1] = CIP_ES_COEFFS_##WW;
CIP_HOST_TABLE(4)
CIP_HOST_TABLE(6)
CIP_HOST_TABLE(8)
CIP_HOST_TABLE(10)
CIP_HOST_TABLE(12)
CIP_HOST_TABLE(14)
CIP_HOST_TABLE(16)
CIP_HOST_TABLE(24)
CIP_HOST_TABLE(32)
CIP_HOST_TABLE(48)
CIP_HOST_TABLE(64)
#undef CIP_HOST_TABLE

static bool host_kernel(int W, HostKernel* k) {
  switch (W) {
#define CASE(WW)                                                              \
  case WW:                                                                    \
    *k = {WW, CIP_ES_DEGREE_##WW, CIP_ES_BETA_##WW, &host_coef_##WW[0][0]};  \
    return true;
    CASE(4) CASE(6) CASE(8) CASE(10) CASE(12) CASE(14) CASE(16) CASE(24) CASE(32) CASE(48) CASE(64)
#undef CASE
    default:
      return false;
  }
}

static double piece_value(const HostKernel& k, int piece, double y) {
  const int half = k.W / 2;
  const double* c = (piece < half) ? k.coef + piece * (k.D + 1) : k.coef + (k.W - 1 - piece) * (k.D + 1);
  const double yy = (piece < half) ? y : -y;
  double r = c[k.D];
  for (int d = k.D - 1; d >= 0; --d) r = r * yy + c[d];
  return r;
}

// Gauss-Legendre nodes/weights on [-1, 1]
static void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& w) {
  x.resize(n);
  w.resize(n);
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5));
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = z;
      for (int j = 2; j <= n; ++j) {
        const double p2 = ((2.0 * j - 1.0) * z * p1 - (j - 1.0) * p0) / j;
        p0 = p1;
        p1 = p2;
      }
      const double dp = n * (z * p1 - p0) / (z * z - 1.0);
      const double dz = p1 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    double p0 = 1.0, p1 = z;
    for (int j = 2; j <= n; ++j) {
      const double p2 = ((2.0 * j - 1.0) * z * p1 - (j - 1.0) * p0) / j;
      p0 = p1;
      p1 = p2;
    }
    const double dp = n * (z * p1 - p0) / (z * z - 1.0);
    x[i] = z;
    w[i] = 2.0 / ((1.0 - z * z) * dp * dp);
  }
}

// F(nu) = integral of the piecewise kernel phi(d) cos(2 pi d nu) over its support
// (d in cells); the grid correction of axis u is 1 / F(p / n_u).
struct KernelFT {
  HostKernel k;
  std::vector<double> gx, gw;
  explicit KernelFT(const HostKernel& kk) : k(kk) { gauss_legendre(24, gx, gw); }
  double operator()(double nu) const {
    double acc = 0.0;
    for (int piece = 0; piece < k.W; ++piece) {
      const double a = piece - 0.5 * k.W;  // piece spans d in [a, a + 1]
      for (size_t i = 0; i < gx.size(); ++i) {
        const double d = a + 0.5 * (gx[i] + 1.0);
        const double y = 2.0 * piece + 1.0 - k.W - 2.0 * d;
        acc += 0.5 * gw[i] * piece_value(k, piece, y) * std::cos(2.0 * M_PI * d * nu);
      }
    }
    return acc;
  }
};

// ------------------------------------------------------------- params ----
static int64_t good_size(int64_t n) {
  if (n < 16) n = 16;
  for (int64_t m = n + (n & 1);; m += 2) {
    int64_t r = m;
    for (int64_t p : {2, 3, 5, 7})
      while (r % p == 0) r /= p;
    if (r == 1) return m;
  }
}

static int support_for_epsilon(double eps) {
  // calibrated against the fp64 direct DFT (DESIGN.md "Accuracy")
  // max |err| / sum(w) vs the direct DFT measured 2e-3, 2e-5, 3e-7, 4e-9,
  // 5e-11, 6e-13, 2e-14 for W = 4 .. 16 (tests/test_oracle_accuracy.py)
  if (eps >= 2e-3) return 4;
  if (eps >= 2e-5) return 6;
  if (eps >= 3e-7) return 8;
  if (eps >= 4e-9) return 10;
  if (eps >= 5e-11) return 12;
  if (eps >= 6e-13) return 14;
  return 16;
}

int choose(int64_t npix_x, int64_t npix_y, double px, double py, double epsilon, int support, int do_wstacking,
           double wmin, double wmax, cip_gridder_params* out) {
  if (npix_x < 2 || npix_y < 2 || (npix_x & 1) || (npix_y & 1))
    return set_error(CIP_EINVAL, "npix_x and npix_y must be even and >= 2");
  if (!(px > 0.0) || !(py > 0.0)) return set_error(CIP_EINVAL, "pixel sizes must be positive");
  if (support > 0) {
    // W <= 16: lane-per-visibility scatter; 24..64 (BASELINE configs[2]'s
    // LDS-tile stress case): wave-per-visibility scatter (cip_scatter_large.hip)
    const bool small = !(support & 1) && support >= 4 && support <= 16;
    const bool large = support == 24 || support == 32 || support == 48 || support == 64;
    if (!small && !large)
      return set_error(CIP_EINVAL, "support must be an even number in [4, 16] or one of 24, 32, 48, 64");
    // (the large supports' shape beta keeps W = 16's edge ratio F(1/4)/F(0),
    // tools/gen_es_kernels.py, so their grid and w corrections amplify the
    // fixed-point quantum no more than W = 16's: w-stacking at every support)
  } else {
    if (!(epsilon > 0.0)) return set_error(CIP_EINVAL, "epsilon must be positive");
    support = support_for_epsilon(epsilon);
  }
  HostKernel hk;
  host_kernel(support, &hk);
  cip_gridder_params p;
  std::memset(&p, 0, sizeof(p));
  p.sigma = 2.0;
  p.nu = good_size((int64_t)std::ceil(p.sigma * npix_x));
  p.nv = good_size((int64_t)std::ceil(p.sigma * npix_y));
  // a footprint wraps around the periodic grid at most once
  if (p.nu < support || p.nv < support) return set_error(CIP_EINVAL, "grid smaller than the kernel support");
  p.support = support;
  p.degree = hk.D;
  p.beta = hk.beta;
  p.tile = kTile;
  const double x0 = -0.5 * npix_x * px, y0 = -0.5 * npix_y * py;
  const double e = x0 * x0 + y0 * y0;
  if (e >= 1.0) return set_error(CIP_EINVAL, "field of view extends beyond the horizon");
  p.nmin = -e / (std::sqrt(1.0 - e) + 1.0);
  p.do_wstacking = do_wstacking ? 1 : 0;
  if (do_wstacking) {
    if (!(wmax >= wmin)) return set_error(CIP_EINVAL, "invalid w range");
    p.dw = 0.5 / p.sigma / std::fabs(p.nmin);
    p.nplanes = (int64_t)std::ceil((wmax - wmin) / p.dw) + support;
    p.w0 = 0.5 * (wmin + wmax) - 0.5 * (double)(p.nplanes - 1) * p.dw;
  } else {
    p.nplanes = 1;
    p.w0 = 0.0;
    p.dw = 1.0;
  }
  *out = p;
  return CIP_OK;
}

GridGeometry geometry(const cip_gridder_params& p, double px, double py, TileShape t) {
  GridGeometry g;
  g.nu = p.nu;
  g.nv = p.nv;
  g.support = p.support;
  g.scale_u = (double)p.nu * px;
  g.scale_v = (double)p.nv * py;
  g.do_wstacking = p.do_wstacking;
  g.w0 = p.w0;
  g.dw = p.dw;
  g.inv_dw = 1.0 / p.dw;
  g.nplanes = p.nplanes;
  g.tile = kTile;
  g.tx_shift = t.tx_shift;
  g.ty_shift = t.ty_shift;
  g.ntx = (p.nu + ((int64_t)1 << t.tx_shift) - 1) >> t.tx_shift;
  g.nty = (p.nv + ((int64_t)1 << t.ty_shift) - 1) >> t.ty_shift;
  g.mtx = (p.nu + kTile - 1) / kTile;
  g.mty = (p.nv + kTile - 1) / kTile;
  g.ntw = p.do_wstacking ? (p.nplanes - p.support + 1) : 1;
  g.transposed = 0;
  g.row0 = 0;
  g.rows = p.nv;
  g.oob = nullptr;
  g.plane_lo = 0;
  g.plane_hi = p.nplanes;
  g.grid_f32 = 0;
  g.wmask = nullptr;
  return g;
}

// the grid-correction vectors cx = 1 / F(p / nu), cy = 1 / F(q / nv) (cached
// per workspace and geometry)
int correction_vectors(Workspace* ws, const GridGeometry& g, int64_t npix_x, int64_t npix_y, hipStream_t s,
                       double** cx_out, double** cy_out) {
  CIP_ALLOC(cx, double, "cx", npix_x)
  CIP_ALLOC(cy, double, "cy", npix_y)
  *cx_out = cx;
  *cy_out = cy;
  HostKernel hk;
  host_kernel(g.support, &hk);
  KernelFT F(hk);
  // each vector depends only on its (npix, grid length, W): one cached table per axis
  const auto axis = [&](const char* name, double* dev, int64_t npix, int64_t n) {
    return host_table(ws, name, {(double)npix, (double)n, (double)g.support}, dev, sizeof(double) * npix, s,
                      [&](void* staging) {
                        double* h = (double*)staging;
                        for (int64_t i = 0; i < npix; ++i) h[i] = 1.0 / F((double)(i - npix / 2) / (double)n);
                      });
  };
  if (const int rc = axis("cx", cx, npix_x, g.nu); rc != CIP_OK) return rc;
  return axis("cy", cy, npix_y, g.nv);
}

// the w-stacking final correction's table of F (cached per workspace)
int w_correction_table(Workspace* ws, const cip_gridder_params& prm, const GridGeometry& g, hipStream_t s,
                       double** table, int64_t* n, double* dnu_out) {
  HostKernel hk;
  host_kernel(g.support, &hk);
  KernelFT F(hk);
  const int64_t fw_n = 4100;
  const double numax = g.dw * std::fabs(prm.nmin);
  const double dnu = (numax > 0 ? numax : 1e-3) * 1.0001 / 4096.0;
  CIP_ALLOC(fwd, double, "fw_table", fw_n)
  *table = fwd;
  *n = fw_n;
  *dnu_out = dnu;
  return host_table(ws, "fw_table", {(double)g.support, numax}, fwd, sizeof(double) * fw_n, s, [&](void* staging) {
    double* fw = (double*)staging;
    for (int64_t k = 0; k < fw_n; ++k) fw[k] = F((double)k * dnu);
  });
}

// w planes per scatter work unit in w-stacking mode: G = 3 (a visibility
// placed and its u, v, w kernels evaluated once for three planes; the unit
// holds G sub-grids in 512-thread blocks), fewer where two such blocks would
// not fit a CU's LDS (W >= 10: 2); the packed class's 8-byte cells allow up to
// 7 (round 5); CIP_WSTACK_GROUP=1..7 caps it (tests compare the groups with
// G = 1); the large supports always 1. Refcall C3 (round 3, fp64 taps): G = 1
// / 2 / 3 -> 13.4 / 12.2 / 11.8 ms of scatter (profiles/r03_ab_wstack_group*.txt).
// One 14-plane group per CU (W = 6) measured slower: 6.94 -> 8.34 ms
// (profiles/r05at_ab_wstack_g14.txt).
int wstack_group(const GridGeometry& g, bool packed) {
  const int env = wstack_group_cap();
  if (!g.do_wstacking || g.support > 16 || g.nplanes < 2) return 1;
  const int64_t P = kTile + g.support - 1;
  if (packed) {
    // 8-byte cells: up to 7 sub-grids in one 512-thread block, two blocks per
    // CU (<= 80 KB of static LDS each; cip_scatter.h kFitG7 .. kFitG4). Round
    // 5: G = 7 at W = 6 (the reference call: 14 planes in two groups, a
    // visibility visits 1.6 groups instead of 2) scatter 7.15 -> 6.93 ms,
    // call 7.35 -> 7.51-7.54 Gvis/s (profiles/r05ah_ab_wstack_group.txt)
    int G = env ? env : 7;
    while (G > 5 && G <= 7 && G * P * P * 8 + 4200 > 81920) --G;
    while (G > 3 && G <= 5 && G * P * P * 8 + 4200 > 65536) --G;
    return G;
  }
  // two 512-thread blocks per CU must fit their G sub-grids in 160 KB of LDS
  const int64_t per_plane = P * P * 16;
  int G = env ? (env > 3 ? 3 : env) : 3;
  while (G > 1 && 2 * G * per_plane > 160 * 1024) --G;
  return G;
}

// The 2-D lane scatter's work tile (the one selection rule). A larger tile
// makes longer row slices - fewer runs for the planner's sort, scans and order
// pass, fewer partly used lines in the scatter's gathers, less halo per cell in
// the flush - but fewer, larger work units: only where all of
// `eligible` holds (prepare(): a cip_ms2dirty* call, 2-D, dense rows, the
// ordered stream) and the support's sub-grids fit (scatter_tile_fits); unforced,
// also only on grids of whole 64-cell tiles with enough of them to fill the
// CUs (nu nv >= 2048^2: smaller grids keep their 32 x 32 plans). Everything
// else - w-stacking, cip_grid_*, ragged slices, the large supports, predict -
// plans 32 x 32. CIP_SCATTER_TILE forces a shape wherever it is eligible and fits.
TileShape scatter_tile_shape(const cip_gridder_params& p, bool packed, bool eligible) {
  const TileShape t32;
  if (!eligible || p.do_wstacking || p.support > 16) return t32;
  const int force = scatter_tile_force();
  TileShape t = force ? TileShape{5 + (force >> 1), 5 + (force & 1)} : kDefaultScatterTile;
  if (force == 4) t = t32;
  if (!force && (p.nu % 64 != 0 || p.nv % 64 != 0 || p.nu * p.nv < (int64_t)2048 * 2048)) return t32;
  return scatter_tile_fits(p.support, packed, 1 << t.tx_shift, 1 << t.ty_shift) ? t : t32;
}

// ----------------------------------------------------------- switches ----
// Every CIP_* environment switch of the library (DESIGN.md lists them with
// the tests that use them). Unset means the default; a value whose first
// character is '0' turns a switch off. Read once per process unless noted.
static const char* env(const char* name) { return getenv(name); }
static bool env_on(const char* name) {
  const char* e = env(name);
  return !(e && e[0] == '0');
}
#define CIP_SWITCH(fn, name)             \
  bool fn() {                            \
    static const bool on = env_on(name); \
    return on;                           \
  }
// CIP_FFT_PRUNED=0 selects the full 2-D hipFFT transform (A/B experiments)
CIP_SWITCH(fft_pruned, "CIP_FFT_PRUNED")
// CIP_GRID_MASK=0: no dirty-tile mask - the grid is zeroed in full before
// every scatter and pass A reads all of it (A/B experiments)
CIP_SWITCH(grid_mask, "CIP_GRID_MASK")
// CIP_SCATTER_ORDER=0 skips the bank-class order (A/B experiments)
CIP_SWITCH(scatter_order, "CIP_SCATTER_ORDER")
// CIP_PACKED_RUNS=0: ragged runs keep the (row, channel start, channel stop)
// record and the order pass gathers delta[row] per run (A/B experiments);
// read per call (tests switch it)
bool packed_runs() { return env_on("CIP_PACKED_RUNS"); }
// CIP_RAGGED_PACK=0: ragged ordered-stream entries in the (row << 16) |
// channel form with the delta[row] gather, as for inputs too large to pack
// (tests: the fallback form on small inputs); read per call
bool ragged_pack() { return env_on("CIP_RAGGED_PACK"); }
// CIP_ROW_PHASES=0: the order pass assigns no row phases (cip_grid.hip
// order_kernel; A/B experiments and the phase test)
CIP_SWITCH(row_phases, "CIP_ROW_PHASES")
// CIP_WSTACK_GROUP=1..7 caps the w planes per scatter work unit
// (wstack_group); unset or 0: no cap
int wstack_group_cap() {
  static const int cap = [] {
    const char* e = env("CIP_WSTACK_GROUP");
    const int v = e ? atoi(e) : 0;
    return v < 0 ? 0 : (v > 7 ? 7 : v);
  }();
  return cap;
}
// CIP_FLUSH_STORE=0 / anything else forces the flush's private-cell stores
// off (0) / on (1) for any grid; unset (-1): by grid size (cip_invert.hip
// flush_store_enabled)
int flush_store_mode() {
  static const int mode = env("CIP_FLUSH_STORE") ? (env_on("CIP_FLUSH_STORE") ? 1 : 0) : -1;
  return mode;
}
// CIP_GRID_F32=0: the packed class keeps complex128 grid planes (A/B)
CIP_SWITCH(grid_f32_enabled, "CIP_GRID_F32")
// CIP_WACC_F32=0: the packed class's w planes accumulate in the fp64 image
// (A/B); default: a float accumulator
CIP_SWITCH(wacc_f32_enabled, "CIP_WACC_F32")
// CIP_FFT_ROWSKIP=0: pass A transforms (and pass B reads) clean tile rows too (A/B)
CIP_SWITCH(fft_rowskip, "CIP_FFT_ROWSKIP")
// CIP_PLACE_ROWS64=0: dense 64-channel rows through place_body (cip_plan.hip; A/B)
CIP_SWITCH(place_rows64, "CIP_PLACE_ROWS64")
// CIP_FFT_F32=0: the packed class's complex64 planes transformed in fp64
// (the round-4 form); default: in fp32, the class's own precision (cip_fft.hip)
CIP_SWITCH(fft_f32_enabled, "CIP_FFT_F32")
// CIP_ORDER_CLASSES=32: bank classes mod 32 (rounds 1-6) instead of mod 16
// (cip_grid.hip launch_order; A/B). On when the first character is '3'.
bool order_classes32() {
  static const bool on = [] {
    const char* e = env("CIP_ORDER_CLASSES");
    return e && e[0] == '3';
  }();
  return on;
}
// CIP_SCATTER_TILE=32 / 64x32 / 32x64 / 64: the 2-D lane scatter's work tile
// wherever a call is eligible for one and it fits (scatter_tile_shape; A/B
// runs and the tile tests at small sizes); unset: by the rule. Returns 0
// unset, 4 for 32, else (x edge is 64) * 2 + (y edge is 64).
int scatter_tile_force() {
  static const int v = [] {
    const char* e = env("CIP_SCATTER_TILE");
    if (!e) return 0;
    if (!strcmp(e, "32")) return 4;
    if (!strcmp(e, "64x32")) return 2;
    if (!strcmp(e, "32x64")) return 1;
    if (!strcmp(e, "64") || !strcmp(e, "64x64")) return 3;
    return 0;
  }();
  return v;
}
// CIP_MOSAIC_LDS=0: cip_mosaic_add reads the facet directly instead of staging
// each tile's window in LDS (cip_mosaic.hip; A/B and the path test); read per call
bool mosaic_lds() { return env_on("CIP_MOSAIC_LDS"); }
#undef CIP_SWITCH

// the HBM layout of the uv grid the FFT stage expects: gT[y, x] when the
// pruned FFT runs
bool grid_is_transposed(const GridGeometry& g, int64_t npix_x, int64_t npix_y) {
  return fft_pruned() && fast_fft_supported(g.nu, g.nv, npix_x, npix_y);
}

// the internal raw linear-feed code is reached through cip_ms2dirty_stokes_i only
bool public_dtypes(int vis_dtype, int wgt_dtype) { return vis_dtype != CIP_POL4I && wgt_dtype != CIP_POL4I; }
bool vis_dtype_ok(int d) { return d == CIP_C64 || d == CIP_C128 || d == CIP_POL4I; }
// the dtypes of a public call (cip_ms2dirty*, cip_dirty2ms); any_vis: the
// visibilities are not read (CIP_PSF), so their dtype is not checked
int public_dtype_check(int vis_dtype, int wgt_dtype, bool any_vis) {
  if (vis_dtype != CIP_C64 && vis_dtype != CIP_C128 && !any_vis)
    return set_error(CIP_EINVAL, "vis dtype must be complex64 or complex128");
  if (wgt_dtype != CIP_NONE && wgt_dtype != CIP_F32 && wgt_dtype != CIP_F64)
    return set_error(CIP_EINVAL, "wgt dtype must be float32, float64 or none");
  return CIP_OK;
}

}  // namespace cip

using namespace cip;

extern "C" {

int cip_choose_params(int64_t npix_x, int64_t npix_y, double pixsize_x, double pixsize_y, double epsilon,
                      int support, int do_wstacking, double wmin, double wmax, cip_gridder_params* out) {
  clear_error();
  if (!out) return set_error(CIP_EINVAL, "out is NULL");
  return choose(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support, do_wstacking, wmin, wmax, out);
}

int cip_grid_layout(const cip_gridder_params* params, int64_t npix_x, int64_t npix_y) {
  clear_error();
  if (!params) return set_error(CIP_EINVAL, "params is NULL");
  return grid_is_transposed(geometry(*params, 1.0, 1.0), npix_x, npix_y) ? 1 : 0;
}

int cip_plane_group(const cip_gridder_params* params, int packed) {
  clear_error();
  if (!params) return set_error(CIP_EINVAL, "params is NULL");
  return wstack_group(geometry(*params, 1.0, 1.0), packed != 0);
}

}  // extern "C"
