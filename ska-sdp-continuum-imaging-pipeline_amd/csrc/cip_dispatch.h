// cip_dispatch.h - runtime value -> template argument, for the launchers of
// libcip_hip.so: the values a kernel is instantiated for as named lists, and
// three helpers that hand a functor the matching compile-time constant. Plain
// C++17 with no HIP types (tests/test_dispatch_host.py builds it on its own);
// cip_common.h includes it and binds dispatch_vis_wgt to the device types.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "cip.h"

namespace cip {

// ---- the instantiated values (the Makefile's lists repeat the first two) ----
template <int... Vs>
using IntList = std::integer_sequence<int, Vs...>;
// lane-per-visibility scatter and degridder: one object each per W (Makefile SUPPORTS)
using LaneSupports = IntList<4, 6, 8, 10, 12, 14, 16>;
// wave-per-visibility scatter, cip_scatter_large.hip (Makefile LARGE_SUPPORTS)
using LargeSupports = IntList<24, 32, 48, 64>;
// transform lengths of the pruned FFT (cip_fft.hip)
using FftLengths = IntList<1024, 2048, 4096, 8192, 16384>;
// I, Q, U, V of cip_stokes (cip_tiling.hip)
using StokesCodes = IntList<0, 1, 2, 3>;

// visibility / weight loads by dtype (CIP_C64 -> float2, CIP_C128 -> double2;
// raw linear-feed columns -> Pol4 + WK_POL4I, Stokes I formed on load)
enum { WK_NONE = 0, WK_F32 = 1, WK_F64 = 2, WK_POL4I = 3 };
// internal vis / wgt dtype code of the raw linear-feed input (not in cip.h:
// reached through cip_ms2dirty_stokes_i only)
constexpr int CIP_POL4I = 0x100;

template <typename T>
struct type_tag {
  using type = T;
};
template <int V>
using int_tag = std::integral_constant<int, V>;

// ---- helpers: the result is the functor's; every call of f must return the same type ----
// f(int_tag<V>{}) for the V of the list equal to v; no V matches: no_match, f not called
template <int... Vs, typename R, typename F>
R dispatch_int(int64_t v, R no_match, F&& f) {
  R r = no_match;
  (void)((v == Vs ? (r = f(int_tag<Vs>{}), true) : false) || ...);
  return r;
}
template <int... Vs, typename R, typename F>
R dispatch_int(IntList<Vs...>, int64_t v, R no_match, F&& f) {
  return dispatch_int<Vs...>(v, no_match, std::forward<F>(f));
}
template <int... Vs>
constexpr bool list_has(IntList<Vs...>, int64_t v) {
  return ((v == Vs) || ...);
}

template <typename F>
auto dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(type_tag<VisT>{}, int_tag<WK>{}) for a (visibility, weight) dtype pair; C64,
// C128, P4: the element types of complex64, complex128 and raw linear-feed
// visibilities. Never fails: prepare() validated the codes, an unknown
// visibility code loads as complex128 and an unknown weight code as no weights.
template <typename C64, typename C128, typename P4, typename F>
auto dispatch_vis_wgt(int vis_dtype, int wgt_dtype, F&& f) {
  if (vis_dtype == CIP_POL4I) return f(type_tag<P4>{}, int_tag<WK_POL4I>{});
  auto wk = [&](auto vt) {
    if (wgt_dtype == CIP_F32) return f(vt, int_tag<WK_F32>{});
    if (wgt_dtype == CIP_F64) return f(vt, int_tag<WK_F64>{});
    return f(vt, int_tag<WK_NONE>{});
  };
  if (vis_dtype == CIP_C64) return wk(type_tag<C64>{});
  return wk(type_tag<C128>{});
}

}  // namespace cip
