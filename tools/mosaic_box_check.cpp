// Host check of cip_mosaic_add's footprint box (csrc/cip_mosaic.hip
// mosaic_args) under the host sanitizers; no GPU. Reads geometries, one a line
// (nx ny px py fnx fny fpx fpy half trim l0 m0), from the file named on the
// command line and prints for each the box of output pixels the kernel would
// be launched on ("i0 i1 j0 j1"), "none" when the facet misses the plane, or
// "err <code>". tools/mosaic_box_check.py writes the cases and compares the
// boxes with the numpy statement's covered sets. Build (after `make`):
//   cd ska-sdp-continuum-imaging-pipeline_amd/csrc
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I. -I../../include \
//     -Xarch_host -fsanitize=address,undefined ../../tools/mosaic_box_check.cpp -o build/mosaic_box_check \
//     -L../ska_sdp_cip_amd/_lib -l:libcip_hip.so -Wl,-rpath,$PWD/../ska_sdp_cip_amd/_lib
#include "cip_mosaic.hip"  // the unit itself: mosaic_args lives in its unnamed namespace

#include <cstdio>

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  cip_mosaic_geom g;
  long long nx, ny, fnx, fny, trim;
  int half;
  double l0, m0;
  while (std::fscanf(f, "%lld %lld %lf %lf %lld %lld %lf %lf %d %lld %lf %lf", &nx, &ny, &g.px, &g.py, &fnx, &fny,
                     &g.fpx, &g.fpy, &half, &trim, &l0, &m0) == 12) {
    g.nx = nx, g.ny = ny, g.fnx = fnx, g.fny = fny, g.half = half, g.trim = trim;
    g.flags = 0, g.beta = 1.0, g.feather = 0.0;
    cip::MosaicArgs a;
    bool empty = false;
    double unused = 0.0;  // the pointers are only checked against NULL
    const int rc = cip::mosaic_args(&g, &unused, 1, l0, m0, &unused, &unused, &a, &empty);
    if (rc != CIP_OK)
      std::printf("err %d\n", rc);
    else if (empty)
      std::printf("none\n");
    else
      std::printf("%lld %lld %lld %lld\n", (long long)a.i0, (long long)(a.i0 + a.ni - 1), (long long)a.j0,
                  (long long)(a.j0 + a.nj - 1));
  }
  std::fclose(f);
  return 0;
}
