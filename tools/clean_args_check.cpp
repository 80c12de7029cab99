// Host check of the argument validation shared by cip_hogbom_clean and
// cip_mfs_clean (csrc/cip_clean.hip) under the host sanitizers; no GPU. Every
// call below is refused before the library touches a device, so the pointers
// are never dereferenced. Build the unit and this file with the sanitizers on
// the host side and take the rest from the normal build of the library:
//   cd ska-sdp-continuum-imaging-pipeline_amd/csrc && make
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I. -I../../include \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     cip_clean.hip ../../tools/clean_args_check.cpp -o build/clean_args_check \
//     -L../ska_sdp_cip_amd/_lib -l:libcip_hip.so -Wl,-rpath,$PWD/../ska_sdp_cip_amd/_lib
//   build/clean_args_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "cip.h"
#include "cip_mfs.h"

namespace {

int failures = 0;

void expect(int rc, const char* entry, const char* what, const char* label) {
  const char* msg = cip_last_error();
  const bool ok = rc == CIP_EINVAL && msg && std::strncmp(msg, entry, std::strlen(entry)) == 0 &&
                  msg[std::strlen(entry)] == ':' && std::strstr(msg, what);
  if (!ok) {
    std::printf("FAIL %s %s: rc %d, message '%s' (wanted '%s')\n", entry, label, rc, msg ? msg : "(null)", what);
    ++failures;
  }
}

struct Args {
  double* res = reinterpret_cast<double*>(4096);
  int64_t nterms = 2, nx = 8, ny = 8;
  const double* psf = reinterpret_cast<const double*>(8192);
  int64_t px = 5, py = 5, cx = -1, cy = -1;
  const double* hinv = nullptr;
  double gain = 0.1, threshold = 0.0;
  int64_t niter = 4, batch = 0;
  int64_t* ci = nullptr;
  double* cf = nullptr;
};

int mfs(const Args& a) {
  cip_clean_result out;
  return cip_mfs_clean(a.res, a.nterms, a.nx, a.ny, a.psf, a.px, a.py, a.cx, a.cy, a.hinv, nullptr, a.gain, a.threshold,
                       a.niter, a.batch, nullptr, nullptr, a.ci, a.cf, &out);
}

int hogbom(const Args& a) {
  cip_clean_result out;
  return cip_hogbom_clean(a.res, a.nx, a.ny, a.psf, a.px, a.py, a.cx, a.cy, nullptr, a.gain, a.threshold, a.niter,
                          a.batch, nullptr, nullptr, a.ci, a.cf, &out);
}

}  // namespace

int main() {
  const double good[9] = {1.0, 0.1, 0.0, 0.1, 2.0, 0.0, 0.0, 0.0, 1.0};
  const double nan4[4] = {1.0, 0.0, std::nan(""), 1.0};
  const double inf4[4] = {1.0, std::numeric_limits<double>::infinity(), 0.0, 1.0};
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  int64_t* fake_i = reinterpret_cast<int64_t*>(12288);
  double* fake_f = reinterpret_cast<double*>(16384);
  const int64_t big = INT64_MAX / 2;
  Args base;
  base.hinv = good;
  // the checks both entry points share: (label, change, text of the message)
  struct Case {
    const char* label;
    std::function<void(Args&)> change;
    const char* what;
  };
  const Case shared[] = {
      {"res NULL", [=](Args& a) { a.res = nullptr; }, "must not be NULL"},
      {"psf NULL", [=](Args& a) { a.psf = nullptr; }, "must not be NULL"},
      {"nx 0", [=](Args& a) { a.nx = 0; }, "dimensions"},
      {"py -3", [=](Args& a) { a.py = -3; }, "dimensions"},
      {"cx = px", [=](Args& a) { a.cx = 5; }, "PSF centre"},
      {"cy -2", [=](Args& a) { a.cy = -2; }, "PSF centre"},
      {"gain 0", [=](Args& a) { a.gain = 0.0; }, "gain"},
      {"gain NaN", [=](Args& a) { a.gain = nan; }, "gain"},
      {"gain inf", [=](Args& a) { a.gain = inf; }, "gain"},
      {"threshold -1", [=](Args& a) { a.threshold = -1.0; }, "threshold"},
      {"threshold NaN", [=](Args& a) { a.threshold = nan; }, "threshold"},
      {"niter -1", [=](Args& a) { a.niter = -1; }, "niter and batch"},
      {"batch -1", [=](Args& a) { a.batch = -1; }, "niter and batch"},
      {"comp_index alone", [=](Args& a) { a.ci = fake_i; }, "go together"},
      {"comp_flux alone", [=](Args& a) { a.cf = fake_f; }, "go together"},
      {"nx ny overflows", [=](Args& a) { a.nx = a.ny = big; }, "too large"},
      {"px py overflows", [=](Args& a) { a.px = a.py = big; }, "too large"},
      {"2^31 tiles", [=](Args& a) { a.nx = (int64_t)1 << 36, a.ny = 128; }, "2^31 tiles"},
  };
  for (const Case& c : shared) {
    Args a = base;
    c.change(a);
    expect(mfs(a), "cip_mfs_clean", c.what, c.label);
    expect(hogbom(a), "cip_hogbom_clean", c.what, c.label);
  }
  // cip_mfs_clean's own
  for (int64_t nterms : {(int64_t)0, (int64_t)4, (int64_t)-1}) {
    Args a = base;
    a.nterms = nterms;
    expect(mfs(a), "cip_mfs_clean", "nterms", "nterms out of range");
  }
  Args a = base;
  a.hinv = nullptr;
  expect(mfs(a), "cip_mfs_clean", "hinv must not be NULL", "hinv NULL");
  a.hinv = nan4;
  expect(mfs(a), "cip_mfs_clean", "finite", "hinv NaN");
  a.hinv = inf4;
  expect(mfs(a), "cip_mfs_clean", "finite", "hinv inf");
  // nx ny fits in int64 but nx ny nterms (and the 2T - 1 PSF planes) does not: the MFS form of the check
  a = base, a.nterms = 3;
  a.nx = (int64_t)1 << 31, a.ny = (int64_t)1 << 31;  // 2^62: fits once, not three times
  expect(mfs(a), "cip_mfs_clean", "too large", "nx ny nterms overflows");
  a = base, a.nterms = 3;
  a.px = (int64_t)1 << 31, a.py = (int64_t)1 << 30;  // 2^61: fits four times, not five
  expect(mfs(a), "cip_mfs_clean", "too large", "px py (2 nterms - 1) overflows");
  std::printf(failures ? "%d check(s) FAILED\n" : "clean_args_check: every call refused as expected (%d failures)\n",
              failures);
  return failures != 0;
}
