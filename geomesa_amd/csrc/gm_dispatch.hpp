// gm_dispatch.hpp -- the one place where run-time switches become template arguments.  No HIP
// header: tools/dispatch_check.cpp tests it with a host compiler alone.
#pragma once

#include <type_traits>

#include "../../include/geomesa_hip.h"

namespace gm {

template <bool B> using Bool = std::integral_constant<bool, B>;
template <int V> using Int = std::integral_constant<int, V>;

// f(Int<V>{}) for the listed value equal to v; the last one listed is the default.  Returns f's result.
template <int V0, int... Vs, class F>
decltype(auto) with_value(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(Int<V0>{});
  else return v == V0 ? f(Int<V0>{}) : with_value<Vs...>(v, f);
}

// f(Int<GM_DAY>{}) ... f(Int<GM_YEAR>{}); entry points reject other values earlier (valid_period)
template <class F>
decltype(auto) with_period(int period, F&& f) {
  return with_value<GM_DAY, GM_WEEK, GM_MONTH, GM_YEAR>(period, f);
}

// f(Bool<a>{}, Bool<b>{}, ...): the flags in argument order.  Returns f's result.
template <class F>
decltype(auto) with_flags(F&& f) { return f(); }
template <class F, class... Rest>
decltype(auto) with_flags(F&& f, bool a, Rest... rest) {
  auto bind = [&](auto A) { return with_flags([&](auto... r) { return f(A, r...); }, rest...); };
  return a ? bind(Bool<true>{}) : bind(Bool<false>{});
}

}  // namespace gm
