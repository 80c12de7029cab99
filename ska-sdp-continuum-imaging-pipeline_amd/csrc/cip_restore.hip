// cip_restore.hip - the clean beam and the restored image (cip_beam_*,
// cip_restore). The operator, rounding included, is defined in
// include/cip_restore.h.
//
// A CLEAN model is sparse, so the restore does work only where the model is
// non-zero. The image is cut into the CLEAN tiles (kCleanTileX rows x
// kCleanTileY columns). Two plain launches on the caller's stream:
//   mark:  one workgroup per model tile writes a 32-bit word, bit r set when
//          row r of the tile holds a non-zero (one streaming read of the model).
//   apply: one workgroup per output tile. With R <= 32 the tile sees at most
//          3 x 3 model tiles; when none of their words has a bit on a row
//          within R of the tile it copies the residual (nothing at all in
//          place). Otherwise it stages the tap table in LDS and walks the model
//          rows i0 - R .. i0 + 31 + R in ascending blocks of kBlockRows rows,
//          skipping blocks and rows whose bit is clear. Per block the waves
//          compact the non-zeros of the 128 + 2 R columns into an LDS list in
//          flat-index order (one wave per half row: ballot, prefix count, wave
//          offsets through LDS); then every thread runs down the list and adds
//          into its four pixels in registers. The list entry is wave-uniform
//          (an LDS broadcast made scalar), and so is the row test: a wave owns
//          rows w and w + 16 of the tile, lane l the columns l and l + 64, so a
//          tap read is 64 consecutive table words per wave.
// Blocks, rows and columns ascend, so every pixel adds its components in
// ascending flat index: the order of the definition. No atomics.
#include <algorithm>
#include <cmath>
#include <limits>

#include "cip_host.h"
#include "cip_restore.h"
#include "cip_rounded.h"

namespace cip {

namespace {

constexpr int kTX = kCleanTileX;  // tile rows
constexpr int kTY = kCleanTileY;  // tile columns
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxR = CIP_RESTORE_MAX_RADIUS;
constexpr int kMaxTaps = (2 * kMaxR + 1) * (2 * kMaxR + 1);
constexpr int kBlockRows = 8;                 // model rows compacted at a time
constexpr int kHalf = (kTY + 2 * kMaxR) / 2;  // columns one wave compacts: half of the widest halo row
constexpr int kListCap = kBlockRows * 2 * kHalf;
static_assert(kTY == 128 && kTX == 32 && kMaxR <= kTX, "a wave owns rows w, w + 16; a tile sees 3 x 3 model tiles");
static_assert(kWaves == 2 * kBlockRows && kHalf <= 128, "one wave per half row of a block, two loads per lane");

// word t: bit r set when row r of model tile t holds a value != 0 (NaN counts)
__global__ __launch_bounds__(kThreads) void restore_mark_kernel(const double* __restrict__ model, int64_t nx,
                                                               int64_t ny, int64_t nty, uint32_t* __restrict__ rows) {
  __shared__ uint32_t s_row[kTX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tx = (int64_t)blockIdx.x / nty, ty = (int64_t)blockIdx.x % nty;
  const int64_t j = ty * kTY + 2 * lane;
  // 16-byte loads where every row of the image starts 16-byte aligned
  const bool vec = ((ny & 1) == 0) && (((uintptr_t)model & 15u) == 0u) && (j + 1 < ny);
#pragma unroll
  for (int r = 0; r < kTX / kWaves; ++r) {
    const int row = wave + kWaves * r;
    const int64_t i = tx * kTX + row;
    bool nz = false;
    if (i < nx && j < ny) {
      const int64_t idx = i * ny + j;
      double v0, v1 = 0.0;
      if (vec) {
        const double2 v = *reinterpret_cast<const double2*>(model + idx);
        v0 = v.x;
        v1 = v.y;
      } else {
        v0 = model[idx];
        if (j + 1 < ny) v1 = model[idx + 1];
      }
      nz = (v0 != 0.0) || (v1 != 0.0);
    }
    const bool any = __ballot(nz) != 0ull;
    if (lane == 0) s_row[row] = any ? 1u : 0u;
  }
  __syncthreads();
  if (wave == 0) {
    const unsigned long long bits = __ballot(lane < kTX && s_row[lane & (kTX - 1)] != 0u);
    if (lane == 0) rows[blockIdx.x] = (uint32_t)bits;
  }
}

__global__ __launch_bounds__(kThreads) void restore_apply_kernel(const double* __restrict__ model,
                                                                const double* residual, double* out, int64_t nx,
                                                                int64_t ny, int64_t ntx, int64_t nty, int R,
                                                                const double* __restrict__ taps,
                                                                const uint32_t* __restrict__ rows) {
  __shared__ double s_taps[kMaxTaps];
  __shared__ double s_val[kListCap];
  __shared__ uint32_t s_pos[kListCap];  // (row - (i0 - 32)) << 16 | (column - (j0 - 32))
  __shared__ int s_cnt[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: the row tests branch on it
  const int64_t tx = (int64_t)blockIdx.x / nty, ty = (int64_t)blockIdx.x % nty;
  const int64_t i0 = tx * kTX, j0 = ty * kTY;

  // this thread's pixels: rows i0 + wave, + 16; columns j0 + lane, + 64
  const int64_t pi[2] = {i0 + wave, i0 + wave + kWaves};
  const int64_t pj[2] = {j0 + lane, j0 + lane + 64};
  // the rows of the 3 x 3 model tiles that hold a non-zero, as 96 bits from
  // row i0 - 32, cut to the rows within R of this tile
  uint32_t m[3] = {0u, 0u, 0u};
  for (int dx = -1; dx <= 1; ++dx) {
    const int64_t ttx = tx + dx;
    if (ttx < 0 || ttx >= ntx) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int64_t tty = ty + dy;
      if (tty < 0 || tty >= nty) continue;
      m[dx + 1] |= rows[ttx * nty + tty];
    }
  }
  m[0] = R > 0 ? (m[0] & (~0u << (kTX - R))) : 0u;
  m[2] = R >= kTX ? m[2] : (m[2] & ((1u << R) - 1u));

  const bool work = (m[0] | m[1] | m[2]) != 0u;  // the same in every thread of the workgroup
  if (!work && out == residual) return;          // in place, nothing to add: the tile is not touched
  double acc[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int c = 0; c < 2; ++c)
      acc[q][c] = (residual && pi[q] < nx && pj[c] < ny) ? residual[pi[q] * ny + pj[c]] : 0.0;

  if (work) {
    const int T = 2 * R + 1;
    for (int k = threadIdx.x; k < T * T; k += kThreads) s_taps[k] = taps[k];
    const int rr = wave >> 1, half = wave & 1;
    for (int blk = 0; blk < 3 * kTX / kBlockRows; ++blk) {
      const uint32_t bits = (m[blk >> 2] >> ((blk & 3) * kBlockRows)) & 0xffu;
      if (bits == 0u) continue;
      // ---- compact the block's non-zeros, in flat-index order ----
      const int rel_i = blk * kBlockRows + rr;  // row - (i0 - 32); a set bit is a row inside the image
      const int64_t ip = i0 - kTX + rel_i;
      const bool active = ((bits >> rr) & 1u) != 0u;
      // the halo row is the columns j0 - R .. j0 + 127 + R; this wave takes
      // those from offset half * kHalf on, lane l the offsets l and l + 64
      const int o0 = half * kHalf + lane, o1 = o0 + 64;
      const int64_t c0 = j0 - R + o0, c1 = j0 - R + o1;
      const bool in0 = active && o0 < kTY + 2 * R && c0 >= 0 && c0 < ny;
      const bool in1 = active && lane < kHalf - 64 && o1 < kTY + 2 * R && c1 >= 0 && c1 < ny;
      const double v0 = in0 ? model[ip * ny + c0] : 0.0;
      const double v1 = in1 ? model[ip * ny + c1] : 0.0;
      const bool nz0 = v0 != 0.0, nz1 = v1 != 0.0;
      const unsigned long long b0 = __ballot(nz0), b1 = __ballot(nz1);
      if (lane == 0) s_cnt[wave] = __popcll(b0) + __popcll(b1);
      __syncthreads();  // also orders the tap staging before its first use
      int off = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int n = s_cnt[w];
        if (w < wave) off += n;
        total += n;
      }
      const unsigned long long below = (1ull << lane) - 1ull;
      if (nz0) {
        const int p = off + __popcll(b0 & below);
        s_val[p] = v0;
        s_pos[p] = ((uint32_t)rel_i << 16) | (uint32_t)(c0 - (j0 - kTX));
      }
      if (nz1) {
        const int p = off + __popcll(b0) + __popcll(b1 & below);
        s_val[p] = v1;
        s_pos[p] = ((uint32_t)rel_i << 16) | (uint32_t)(c1 - (j0 - kTX));
      }
      __syncthreads();
      // ---- every thread runs down the list ----
      // 64 entries at a time: lane l fetches entry n0 + l, then the wave reads
      // them back one by one as scalars (no LDS latency per entry)
      const int utotal = __builtin_amdgcn_readfirstlane(total);
      for (int n0 = 0; n0 < utotal; n0 += 64) {
        const int cnt = utotal - n0 < 64 ? utotal - n0 : 64;
        const bool mine = lane < cnt;
        const uint32_t my_pos = mine ? s_pos[n0 + lane] : 0u;
        const double my_val = mine ? s_val[n0 + lane] : 0.0;
        const int my_lo = __double2loint(my_val), my_hi = __double2hiint(my_val);
        // the list ascends in rows: skip the 64 when none of them is within R of this wave's rows
        const int row_first = __builtin_amdgcn_readlane((int)my_pos, 0) >> 16;
        const int row_last = __builtin_amdgcn_readlane((int)my_pos, cnt - 1) >> 16;
        if (row_last < wave + kTX - R || row_first > wave + kTX + kWaves + R) continue;
        for (int k = 0; k < cnt; ++k) {
          const uint32_t pos = (uint32_t)__builtin_amdgcn_readlane((int)my_pos, k);
          const double v = __hiloint2double(__builtin_amdgcn_readlane(my_hi, k), __builtin_amdgcn_readlane(my_lo, k));
          const int da0 = (wave + kTX) - (int)(pos >> 16);    // this wave's first row minus the component's
          const int db0 = (lane + kTX) - (int)(pos & 0xffffu);  // this lane's first column minus the component's
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int da = da0 + kWaves * q;
            if (da < -R || da > R) continue;  // wave-uniform
            const int trow = (da + R) * T + R;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int db = db0 + 64 * c;
              if (db >= -R && db <= R) acc[q][c] = add_rounded(acc[q][c], mul_rounded(v, s_taps[trow + db]));
            }
          }
        }
      }
      __syncthreads();  // the list is rewritten by the next block
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (pi[q] < nx && pj[c] < ny) out[pi[q] * ny + pj[c]] = acc[q][c];
}

}  // namespace

hipError_t launch_restore(const double* model, const double* residual, double* out, int64_t nx, int64_t ny, int R,
                          const double* taps, uint32_t* rows, hipStream_t s) {
  const int64_t ntx = (nx + kTX - 1) / kTX, nty = (ny + kTY - 1) / kTY;
  restore_mark_kernel<<<dim3((unsigned)(ntx * nty)), dim3(kThreads), 0, s>>>(model, nx, ny, nty, rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  restore_apply_kernel<<<dim3((unsigned)(ntx * nty)), dim3(kThreads), 0, s>>>(model, residual, out, nx, ny, ntx, nty, R,
                                                                             taps, rows);
  return hipGetLastError();
}

}  // namespace cip

// ------------------------------------------------------------ host API ----
namespace cip {

namespace {

const char* const kFitAdvice = "; lower cut (more pixels enter the fit) or pass a beam (cip_beam_from_fwhm)";

bool positive_definite(double a, double b, double c) {
  return std::isfinite(a) && std::isfinite(b) && std::isfinite(c) && a > 0.0 && c > 0.0 && a * c - b * b > 0.0;
}

// the smaller eigenvalue of [[a, b], [b, c]]
double lambda_min(double a, double b, double c) { return 0.5 * ((a + c) - std::hypot(a - c, 2.0 * b)); }

// fwhm_major, fwhm_minor and pa from a, b, c (cip_restore.h)
void fill_shape(cip_beam* bm) {
  const double tr = bm->a + bm->c, d = std::hypot(bm->a - bm->c, 2.0 * bm->b);
  const double lmin = 0.5 * (tr - d), lmax = 0.5 * (tr + d);
  const double ln2 = std::log(2.0), pi = std::acos(-1.0);
  bm->fwhm_major = 2.0 * std::sqrt(ln2 / lmin);
  bm->fwhm_minor = 2.0 * std::sqrt(ln2 / lmax);
  double pa = -0.5 * std::atan2(2.0 * bm->b, bm->a - bm->c);
  if (pa <= -0.5 * pi) pa += pi;
  bm->pa = pa;
}

int beam_check(const char* who, const cip_beam* bm) {
  if (!bm) return set_error(CIP_EINVAL, std::string(who) + ": beam must not be NULL");
  if (!positive_definite(bm->a, bm->b, bm->c))
    return set_error(CIP_EINVAL, std::string(who) + ": the beam's form is not positive definite "
                                                    "(a > 0, c > 0, a c - b^2 > 0)");
  return CIP_OK;
}

int fit_args_check(const char* who, double cut, int64_t radius) {
  if (!(cut > 0.0 && cut < 1.0)) return set_error(CIP_EINVAL, std::string(who) + ": cut must lie in (0, 1)");
  if (radius < 1 || radius > 64) return set_error(CIP_EINVAL, std::string(who) + ": radius must be in 1 .. 64");
  return CIP_OK;
}

int from_fwhm_impl(double major, double minor, double pa, cip_beam* out) {
  if (!out) return set_error(CIP_EINVAL, "cip_beam_from_fwhm: out must not be NULL");
  if (!std::isfinite(major) || !std::isfinite(minor) || !std::isfinite(pa) || !(minor > 0.0) || !(major >= minor))
    return set_error(CIP_EINVAL, "cip_beam_from_fwhm: need finite fwhm_major >= fwhm_minor > 0 and a finite pa");
  const double ln2 = std::log(2.0);
  const double lmin = 4.0 * ln2 / (major * major), lmax = 4.0 * ln2 / (minor * minor);
  const double sn = std::sin(pa), cs = std::cos(pa);
  out->a = lmin * sn * sn + lmax * cs * cs;
  out->b = (lmin - lmax) * sn * cs;
  out->c = lmin * cs * cs + lmax * sn * sn;
  out->n_fit = 0;
  if (!positive_definite(out->a, out->b, out->c))
    return set_error(CIP_EINVAL, "cip_beam_from_fwhm: these FWHMs give no positive definite form in fp64");
  fill_shape(out);
  return CIP_OK;
}

int fit_window_impl(const char* who, const double* win, int64_t r, double cut, cip_beam* out) {
  const std::string w(who);
  if (!win || !out) return set_error(CIP_EINVAL, w + ": window and out must not be NULL");
  if (const int rc = fit_args_check(who, cut, r); rc != CIP_OK) return rc;
  const int64_t n = 2 * r + 1;
  const double p0 = win[r * n + r];
  if (!std::isfinite(p0) || !(p0 > 0.0))
    return set_error(CIP_EINVAL, w + ": the PSF's centre pixel must be finite and > 0");
  const double level = cut * p0;
  // normal equations of y ~ a x0 + b x1 + c x2 with x = (da^2, 2 da db, db^2)
  double N[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, rhs[3] = {0.0, 0.0, 0.0};
  int64_t n_fit = 0;
  for (int64_t ia = 0; ia < n; ++ia)
    for (int64_t ib = 0; ib < n; ++ib) {
      if (ia == r && ib == r) continue;
      const double v = win[ia * n + ib];
      if (!(v >= level)) continue;  // NaN drops out here
      const double da = (double)(ia - r), db = (double)(ib - r);
      const double x[3] = {da * da, 2.0 * da * db, db * db};
      const double y = -std::log(v / p0);
      for (int p = 0; p < 3; ++p) {
        rhs[p] += x[p] * y;
        for (int q = 0; q < 3; ++q) N[p][q] += x[p] * x[q];
      }
      ++n_fit;
    }
  // Cramer's rule; the matrix is symmetric positive semi-definite, so its
  // determinant is at most the product of its diagonal (Hadamard): a
  // determinant tiny against that product is a singular matrix
  const double c00 = N[1][1] * N[2][2] - N[1][2] * N[2][1];
  const double c01 = N[1][0] * N[2][2] - N[1][2] * N[2][0];
  const double c02 = N[1][0] * N[2][1] - N[1][1] * N[2][0];
  const double det = N[0][0] * c00 - N[0][1] * c01 + N[0][2] * c02;
  const double scale = N[0][0] * N[1][1] * N[2][2];
  if (!(det > 1e-12 * scale) || !(scale > 0.0))
    return set_error(CIP_ERANGE, w + ": the fit is singular (" + std::to_string(n_fit) + " pixels at or above cut)" +
                                     kFitAdvice);
  auto det3 = [](const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  };
  double sol[3];
  for (int k = 0; k < 3; ++k) {
    double M[3][3];
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) M[p][q] = q == k ? rhs[p] : N[p][q];
    sol[k] = det3(M) / det;
  }
  if (!std::isfinite(sol[0]) || !std::isfinite(sol[1]) || !std::isfinite(sol[2]))
    return set_error(CIP_ERANGE, w + ": the fit has no finite solution" + kFitAdvice);
  if (!positive_definite(sol[0], sol[1], sol[2]))
    return set_error(CIP_ERANGE, w + ": the fitted form is not positive definite" + kFitAdvice);
  out->a = sol[0];
  out->b = sol[1];
  out->c = sol[2];
  out->n_fit = n_fit;
  fill_shape(out);
  return CIP_OK;
}

int beam_fit_impl(const double* psf, int64_t px, int64_t py, int64_t cx, int64_t cy, double cut, int64_t r,
                  void* hip_stream, cip_beam* out) {
  const char* who = "cip_beam_fit";
  if (!psf || !out) return set_error(CIP_EINVAL, "cip_beam_fit: psf and out must not be NULL");
  if (px < 1 || py < 1) return set_error(CIP_EINVAL, "cip_beam_fit: PSF dimensions must be >= 1");
  if (cx == -1) cx = px / 2;
  if (cy == -1) cy = py / 2;
  if (cx < 0 || cx >= px || cy < 0 || cy >= py)
    return set_error(CIP_EINVAL, "cip_beam_fit: the PSF centre lies outside the PSF");
  if (const int rc = fit_args_check(who, cut, r); rc != CIP_OK) return rc;
  CIP_BEGIN_CALL(hip_stream, false)
  const int64_t n = 2 * r + 1;
  double* win = (double*)pinned(ws, sizeof(double) * (size_t)(n * n));
  if (!win) return CIP_ENOMEM;
  std::fill(win, win + n * n, std::numeric_limits<double>::quiet_NaN());
  // the part of the window inside the PSF: rows i_lo .. i_hi - 1, columns j_lo .. j_hi - 1 (never empty)
  const int64_t i_lo = std::max<int64_t>(cx - r, 0), i_hi = std::min<int64_t>(cx + r + 1, px);
  const int64_t j_lo = std::max<int64_t>(cy - r, 0), j_hi = std::min<int64_t>(cy + r + 1, py);
  CIP_HIP_CHECK(hipMemcpy2DAsync(win + (i_lo - (cx - r)) * n + (j_lo - (cy - r)), sizeof(double) * (size_t)n,
                                 psf + i_lo * py + j_lo, sizeof(double) * (size_t)py,
                                 sizeof(double) * (size_t)(j_hi - j_lo), (size_t)(i_hi - i_lo), hipMemcpyDeviceToHost,
                                 s));
  if (const int rc = end_call(call); rc != CIP_OK) return rc;
  return fit_window_impl(who, win, r, cut, out);
}

int beam_radius_impl(const char* who, const cip_beam* bm, double tol) {
  if (const int rc = beam_check(who, bm); rc != CIP_OK) return rc;
  if (!(tol > 0.0 && tol < 1.0)) return set_error(CIP_EINVAL, std::string(who) + ": tol must lie in (0, 1)");
  const double lmin = lambda_min(bm->a, bm->b, bm->c);
  const double rad = std::ceil(std::sqrt(std::log(1.0 / tol) / lmin));
  if (!(rad <= (double)CIP_RESTORE_MAX_RADIUS))  // also a lmin that cancelled to <= 0
    return set_error(CIP_ERANGE, std::string(who) + ": the beam needs a radius above CIP_RESTORE_MAX_RADIUS (" +
                                     std::to_string(CIP_RESTORE_MAX_RADIUS) + " pixels) at this tol");
  return (int)rad;
}

void fill_taps(const cip_beam* bm, int64_t R, double* taps) {
#pragma clang fp contract(off)
  const double a = bm->a, b2 = 2.0 * bm->b, c = bm->c;
  const int64_t T = 2 * R + 1;
  for (int64_t ia = 0; ia < T; ++ia)
    for (int64_t ib = 0; ib < T; ++ib) {
      const double da = (double)(ia - R), db = (double)(ib - R);
      taps[ia * T + ib] = std::exp(-((a * (da * da) + b2 * (da * db)) + c * (db * db)));
    }
}

int beam_taps_impl(const cip_beam* bm, int64_t R, double* taps) {
  if (const int rc = beam_check("cip_beam_taps", bm); rc != CIP_OK) return rc;
  if (!taps) return set_error(CIP_EINVAL, "cip_beam_taps: taps_out must not be NULL");
  if (R < 0 || R > CIP_RESTORE_MAX_RADIUS)
    return set_error(CIP_EINVAL, "cip_beam_taps: radius must be in 0 .. CIP_RESTORE_MAX_RADIUS");
  fill_taps(bm, R, taps);
  return CIP_OK;
}

// mark and apply, queued on the caller's stream; the tap table goes up only
// when (a, b, c, R) differ from the table already on the device
int restore_impl(const double* model, const double* residual, int64_t nx, int64_t ny, const cip_beam* bm, int64_t R,
                 void* hip_stream, double* out) {
  if (!model || !out) return set_error(CIP_EINVAL, "cip_restore: model and out must not be NULL");
  if (out == model) return set_error(CIP_EINVAL, "cip_restore: out must not be the model (it may be the residual)");
  if (nx < 1 || ny < 1) return set_error(CIP_EINVAL, "cip_restore: image dimensions must be >= 1");
  if (const int rc = beam_check("cip_restore", bm); rc != CIP_OK) return rc;
  if (R > CIP_RESTORE_MAX_RADIUS)
    return set_error(CIP_EINVAL, "cip_restore: radius must not exceed CIP_RESTORE_MAX_RADIUS");
  if (R < 0) {
    const int rc = beam_radius_impl("cip_restore", bm, 1e-8);
    if (rc < 0) return rc;
    R = rc;
  }
  if (nx > INT64_MAX / ny) return set_error(CIP_EINVAL, "cip_restore: image too large");
  const int64_t ntiles = clean_tiles(nx, ny);
  if (ntiles >= ((int64_t)1 << 31)) return set_error(CIP_EINVAL, "cip_restore: image has 2^31 tiles or more");
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(rows, uint32_t, "restore_rows", ntiles)
  CIP_ALLOC(taps, double, "restore_taps", kMaxTaps)
  const size_t bytes = sizeof(double) * (size_t)((2 * R + 1) * (2 * R + 1));
  if (const int rc = host_table(ws, "restore_taps", {bm->a, bm->b, bm->c, (double)R}, taps, bytes, s,
                                [&](void* staging) { fill_taps(bm, R, (double*)staging); });
      rc != CIP_OK)
    return rc;
  CIP_HIP_CHECK(launch_restore(model, residual, out, nx, ny, (int)R, taps, rows, s));
  return CIP_OK;
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_beam_from_fwhm(double fwhm_major, double fwhm_minor, double pa, cip_beam* out) {
  clear_error();
  return from_fwhm_impl(fwhm_major, fwhm_minor, pa, out);
}

int cip_beam_fit_window(const double* window, int64_t radius, double cut, cip_beam* out) {
  clear_error();
  return fit_window_impl("cip_beam_fit_window", window, radius, cut, out);
}

int cip_beam_fit(const double* psf, int64_t psf_nx, int64_t psf_ny, int64_t psf_cx, int64_t psf_cy, double cut,
                 int64_t radius, void* hip_stream, cip_beam* out) {
  clear_error();
  return beam_fit_impl(psf, psf_nx, psf_ny, psf_cx, psf_cy, cut, radius, hip_stream, out);
}

int cip_beam_radius(const cip_beam* beam, double tol) {
  clear_error();
  return beam_radius_impl("cip_beam_radius", beam, tol);
}

int cip_beam_taps(const cip_beam* beam, int64_t radius, double* taps_out) {
  clear_error();
  return beam_taps_impl(beam, radius, taps_out);
}

int cip_restore(const double* model, const double* residual, int64_t nx, int64_t ny, const cip_beam* beam,
                int64_t radius, void* hip_stream, double* out) {
  clear_error();
  return restore_impl(model, residual, nx, ny, beam, radius, hip_stream, out);
}

}  // extern "C"
