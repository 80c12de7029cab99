// cip_degrid.hip - the degridder's helper kernels and dispatch (cip_dirty2ms):
// image preparation (correction, sign, zero padding, conjugate w screen), the
// per-support launch and the w-stacking final pass.
#include "cip_internal.h"

namespace cip {

// n - 1 of image pixel (i, j) (cip_grid.hip nm1_of)
__device__ __forceinline__ double degrid_nm1(int64_t i, int64_t j, int64_t nx, int64_t ny, double px, double py) {
  const double l = (double)(i - nx / 2) * px;
  const double m = (double)(j - ny / 2) * py;
  const double e = l * l + m * m;
  return -e / (sqrt(1.0 - e) + 1.0);
}

// out = (-1)^(p+q) dirty cx[i] cy[j] [/ (F(dw |n - 1|) n)]: the transpose of
// crop_correct_2d / wfinal_correct (the same table lookup of F, cubic Lagrange)
__global__ void degrid_image_kernel(const double* __restrict__ dirty, int64_t nx, int64_t ny, double px, double py,
                                    const double* __restrict__ cx, const double* __restrict__ cy,
                                    const double* __restrict__ fw, int64_t fw_n, double fw_dnu, double dw,
                                    double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (j >= ny) return;
  const int64_t p = i - nx / 2, q = j - ny / 2;
  double c = cx[i] * cy[j];
  if (fw) {
    const double nm1 = degrid_nm1(i, j, nx, ny, px, py);
    const double t = fabs(dw * nm1) / fw_dnu;
    int64_t k = (int64_t)t;
    if (k < 1) k = 1;
    if (k > fw_n - 3) k = fw_n - 3;
    const double x = t - (double)k;  // in [-1, 2]
    const double f0 = fw[k - 1], f1 = fw[k], f2 = fw[k + 1], f3 = fw[k + 2];
    const double F = -x * (x - 1.0) * (x - 2.0) / 6.0 * f0 + (x + 1.0) * (x - 1.0) * (x - 2.0) / 2.0 * f1 -
                     (x + 1.0) * x * (x - 2.0) / 2.0 * f2 + (x + 1.0) * x * (x - 1.0) / 6.0 * f3;
    c = c / (F * (nm1 + 1.0));
  }
  const double sgn = ((p + q) & 1) ? -1.0 : 1.0;
  out[i * ny + j] = sgn * dirty[i * ny + j] * c;
}

hipError_t launch_degrid_image(const double* dirty, int64_t npix_x, int64_t npix_y, double pixsize_x,
                               double pixsize_y, const double* cx, const double* cy, const double* fw_table,
                               int64_t fw_n, double fw_dnu, double dw, double* out, hipStream_t s) {
  degrid_image_kernel<<<dim3((unsigned)((npix_y + 255) / 256), (unsigned)npix_x), dim3(256), 0, s>>>(
      dirty, npix_x, npix_y, pixsize_x, pixsize_y, cx, cy, fw_table, fw_n, fw_dnu, dw, out);
  return hipGetLastError();
}

// Plane k = blockIdx.z, grid row x = blockIdx.y, lanes along y: the inverse of
// the crop (oracle._crop) - image pixel p = i - nx / 2 in [-nx / 2, nx / 2)
// sits at grid index p mod nu, so x < nx / 2 holds p = x, x >= nu - nx / 2
// holds p = x - nu, and the cells between are the zero padding (nu >= 2 nx).
__global__ void degrid_pad_kernel(const double* __restrict__ image, int64_t nx, int64_t ny, int64_t nu, int64_t nv,
                                  double px, double py, int wstack, double w_first, double dw,
                                  double2* __restrict__ planes) {
  const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t x = blockIdx.y;
  if (y >= nv) return;
  const int64_t hx = nx / 2, hy = ny / 2;
  const int64_t i = x < nx - hx ? x + hx : (x >= nu - hx ? x - nu + hx : -1);
  const int64_t j = y < ny - hy ? y + hy : (y >= nv - hy ? y - nv + hy : -1);
  double2 val = make_double2(0.0, 0.0);
  if (i >= 0 && j >= 0) {
    const double a = image[i * ny + j];
    if (wstack) {
      const double w_plane = w_first + (double)blockIdx.z * dw;
      double sn, cs;
      sincospi(2.0 * w_plane * degrid_nm1(i, j, nx, ny, px, py), &sn, &cs);
      val = make_double2(a * cs, a * sn);
    } else {
      val = make_double2(a, 0.0);
    }
  }
  planes[((int64_t)blockIdx.z * nu + x) * nv + y] = val;
}

hipError_t launch_degrid_pad(const double* image, int64_t npix_x, int64_t npix_y, double pixsize_x, double pixsize_y,
                             const GridGeometry& g, double w_first, int np, double* planes, hipStream_t s) {
  if (np <= 0) return hipSuccess;
  degrid_pad_kernel<<<dim3((unsigned)((g.nv + 255) / 256), (unsigned)g.nu, (unsigned)np), dim3(256), 0, s>>>(
      image, npix_x, npix_y, g.nu, g.nv, pixsize_x, pixsize_y, g.do_wstacking, w_first, g.dw, (double2*)planes);
  return hipGetLastError();
}

hipError_t launch_degrid(const DegridLaunch& a, hipStream_t s) {
  if (a.nchunks <= 0) return hipSuccess;
  if (a.plan.m.delta != nullptr) return hipErrorInvalidValue;  // dense MS rows only
  const dim3 gd((unsigned)a.nchunks);
  return dispatch_int(LaneSupports{}, a.support, hipErrorInvalidValue,
                      [&](auto w) { return launch_degrid_w<decltype(w)::value>(a, gd, s); });
}

// vis_io[i] = wt acc[i] (an exact 0 for a zero weight) or vis_io[i] -= wt
// acc[i]; the product rounded before the subtraction (no contraction)
__global__ void degrid_finish_kernel(DegridOut o, int64_t nvis) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvis) return;
  double wt = 1.0;
  if (o.wgt_dtype == CIP_F32) wt = (double)((const float*)o.wgt)[i];
  else if (o.wgt_dtype == CIP_F64) wt = ((const double*)o.wgt)[i];
  if (o.subtract && wt == 0.0) return;
  const double2 a = o.acc[i];
  const double mr = wt == 0.0 ? 0.0 : wt * a.x, mi = wt == 0.0 ? 0.0 : wt * a.y;
  if (o.vis_dtype == CIP_C64) {
    float2* p = (float2*)o.vis_io + i;
    if (o.subtract) {
      const float2 v = *p;
      *p = make_float2((float)((double)v.x - mr), (float)((double)v.y - mi));
    } else {
      *p = make_float2((float)mr, (float)mi);
    }
  } else {
    double2* p = (double2*)o.vis_io + i;
    if (o.subtract) {
      const double2 v = *p;
      *p = make_double2(v.x - mr, v.y - mi);
    } else {
      *p = make_double2(mr, mi);
    }
  }
}

hipError_t launch_degrid_finish(const DegridOut& o, int64_t nvis, hipStream_t s) {
  if (nvis <= 0) return hipSuccess;
  // the accumulator is the output itself and nothing scales it
  if ((void*)o.acc == o.vis_io && o.wgt_dtype == CIP_NONE) return hipSuccess;
  degrid_finish_kernel<<<dim3((unsigned)((nvis + 255) / 256)), dim3(256), 0, s>>>(o, nvis);
  return hipGetLastError();
}

}  // namespace cip
