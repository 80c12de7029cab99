"""csrc/cip_dispatch.h on its own: the runtime value -> template argument helpers
against the named value lists, as a stand-alone C++17 host program (no GPU, no
HIP header)."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ska-sdp-continuum-imaging-pipeline_amd" / "csrc"

PROGRAM = r"""
#include <cstdio>
#include <type_traits>

#include "cip_dispatch.h"

using namespace cip;

static int failures = 0;
#define CHECK(...)                                               \
  do {                                                           \
    if (!(__VA_ARGS__)) {                                        \
      std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__);      \
      ++failures;                                                \
    }                                                            \
  } while (0)

// stand-ins for float2, double2 and Pol4
struct C64 {};
struct C128 {};
struct P4 {};

// every value of the list reaches the functor once, with its own constant;
// values off the list return the no-match value and never call it
template <int... Vs>
static void check_list(IntList<Vs...> list, int expected_count) {
  const int values[] = {Vs...};
  CHECK((int)sizeof...(Vs) == expected_count);
  for (int v : values) {
    int calls = 0;
    const int r = dispatch_int(list, v, -1, [&](auto c) {
      ++calls;
      return (int)decltype(c)::value;
    });
    CHECK(calls == 1);
    CHECK(r == v);
    CHECK(list_has(list, v));
  }
  const long long off[] = {0, 5, 18, 20, 20000, -4, -1024, (1ll << 32) + 1024};
  for (long long v : off) {
    bool listed = false;
    for (int w : values) listed = listed || w == v;
    if (listed) continue;  // 0 is a Stokes code
    int calls = 0;
    const int r = dispatch_int(list, v, -7, [&](auto c) {
      ++calls;
      return (int)decltype(c)::value;
    });
    CHECK(calls == 0);
    CHECK(r == -7);
    CHECK(!list_has(list, v));
  }
}

struct Seen {
  int vis;  // 64, 128, 4
  int wk;
};
static Seen vis_wgt(int vis_dtype, int wgt_dtype) {
  int calls = 0;
  const Seen s = dispatch_vis_wgt<C64, C128, P4>(vis_dtype, wgt_dtype, [&](auto vt, auto wk) {
    using T = typename decltype(vt)::type;
    ++calls;
    return Seen{std::is_same<T, C64>::value ? 64 : std::is_same<T, C128>::value ? 128 : 4, (int)decltype(wk)::value};
  });
  CHECK(calls == 1);
  return s;
}

int main() {
  check_list(LaneSupports{}, 7);
  check_list(LargeSupports{}, 4);
  check_list(FftLengths{}, 5);
  check_list(StokesCodes{}, 4);
  CHECK(list_has(LaneSupports{}, 4) && list_has(LaneSupports{}, 16) && !list_has(LaneSupports{}, 2));
  CHECK(list_has(LargeSupports{}, 24) && list_has(LargeSupports{}, 64));
  CHECK(list_has(FftLengths{}, 1024) && list_has(FftLengths{}, 16384) && !list_has(FftLengths{}, 512));
  CHECK(!list_has(FftLengths{}, 32768));

  // an explicit list, and the functor's own result type
  CHECK(dispatch_int<8, 16>(16, 0.5, [](auto c) { return 0.25 * decltype(c)::value; }) == 4.0);
  CHECK(dispatch_int<8, 16>(4, 0.5, [](auto c) { return 0.25 * decltype(c)::value; }) == 0.5);

  CHECK(dispatch_bool(true, [](auto b) { return decltype(b)::value ? 1 : 2; }) == 1);
  CHECK(dispatch_bool(false, [](auto b) { return decltype(b)::value ? 1 : 2; }) == 2);

  // (visibility code, weight code) -> (VisT, WK): 3 x 4 pairs and an unknown code of each kind
  const int wgt_codes[] = {CIP_NONE, CIP_F32, CIP_F64, CIP_POL4I, 77};
  const int wgt_wk[] = {WK_NONE, WK_F32, WK_F64, WK_NONE, WK_NONE};
  for (int i = 0; i < 5; ++i) {
    Seen s = vis_wgt(CIP_POL4I, wgt_codes[i]);
    CHECK(s.vis == 4 && s.wk == WK_POL4I);
    s = vis_wgt(CIP_C64, wgt_codes[i]);
    CHECK(s.vis == 64 && s.wk == wgt_wk[i]);
    s = vis_wgt(CIP_C128, wgt_codes[i]);
    CHECK(s.vis == 128 && s.wk == wgt_wk[i]);
    s = vis_wgt(99, wgt_codes[i]);  // unknown visibility code: complex128
    CHECK(s.vis == 128 && s.wk == wgt_wk[i]);
  }
  if (failures == 0) std::printf("dispatch ok\n");
  return failures == 0 ? 0 : 1;
}
"""


def _host_compiler():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    for cand in (rocm / "lib" / "llvm" / "bin" / "clang++", rocm / "llvm" / "bin" / "clang++"):
        if cand.exists():
            return [str(cand)]
    hipcc = shutil.which("hipcc") or str(rocm / "bin" / "hipcc")
    return [hipcc, "-x", "c++"]


def test_dispatch_helpers_match_value_lists(tmp_path):
    src = tmp_path / "dispatch_host.cpp"
    exe = tmp_path / "dispatch_host"
    src.write_text(PROGRAM)
    cmd = _host_compiler() + ["-std=c++17", "-O0", "-Wall", "-Werror", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                              str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dispatch ok" in run.stdout
