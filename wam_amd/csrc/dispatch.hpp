// Runtime value -> template argument for the DWT launchers: the filter lengths each kernel family
// serves, defined once, and the steps that pick a kernel instantiation from them. The launch itself
// (wam_lds_opt_in, WamTimer, hipLaunchKernelGGL) stays at the call site, in the lambda.
#pragma once
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "common.hpp"

template <int... Ls>
struct WamLens {};
using WamLensEven20 = WamLens<2, 4, 6, 8, 10, 12, 14, 16, 18, 20>;  // 1D tiles, 2D column strips, adjoint border
using WamLensTo8 = WamLens<2, 4, 6, 8>;                             // 2D plane, 3D tiles
using WamLensRows = WamLens<2, 4, 6, 8, 12, 16, 20>;                // 2D rows: 10, 14 and 18 take the column strips
using WamLevels8 = WamLens<1, 2, 3, 4, 5, 6, 7, 8>;                 // level counts of the persistent 1D synthesis

// membership: what a family's *_supported predicate asks
template <int... Ls>
constexpr bool wam_len_in(WamLens<Ls...>, int L) {
  return ((L == Ls) || ...);
}

// f(std::integral_constant<int, L>{}) for the list's entry equal to L, and its status;
// WAM_ERR_UNSUPPORTED, and no call, when there is none
template <int... Ls, class F>
int wam_dispatch_len(WamLens<Ls...>, int L, F&& f) {
  int rc = WAM_ERR_UNSUPPORTED;
  (void)((L == Ls && ((rc = f(std::integral_constant<int, Ls>{})), true)) || ...);
  return rc;
}

// the two-axis form: f(length, levels) over Lens x WamLevels8
template <class Lens, class F>
int wam_dispatch_len_levels(Lens lens, int L, int J, F&& f) {
  return wam_dispatch_len(lens, L, [&](auto l) -> int {
    return wam_dispatch_len(WamLevels8{}, J, [&](auto j) -> int { return f(l, j); });
  });
}

// a runtime flag (NOISE, COOP, two columns per lane) as std::bool_constant
template <class F>
int wam_dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// Compute units of the current device, queried once per device: what the persistent launchers size
// their grids by. *cus is written on hipSuccess only.
inline hipError_t wam_device_cus(int* cus) {
  static std::mutex mu;
  static std::map<int, int> known;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  auto it = known.find(dev);
  if (it == known.end()) {
    int n = 0;
    e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    it = known.emplace(dev, n).first;
  }
  *cus = it->second;
  return hipSuccess;
}
