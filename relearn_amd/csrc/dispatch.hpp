// dispatch.hpp — how a launcher turns a runtime value into a template argument: the value is looked up in a range or a
// listed set, and the match reaches a generic lambda as a constant (`[&](auto d) { k<decltype(d)::value><<<..>>> }`).
// Every kernel instantiation of kernels_*.hip is picked through these three functions.  A value outside the table is
// `false`, never a launch: the caller throws its refusal.  Plain C++17 without a HIP include, as handle_spec.hpp:
// tests/cpp/dispatch_demo.cpp.
#pragma once

#include <type_traits>
#include <utility>

template <int N>
using Int = std::integral_constant<int, N>;

// go(Int<v>{}) if `v` is one of Vs...; whether it was
template <int... Vs, class Go>
bool with_one_of(long v, Go &&go) {
  return ((v == Vs ? (go(Int<Vs>{}), true) : false) || ...);
}

namespace dispatch_detail {
template <int LO, class Go, int... Is>
bool with_offsets(long v, Go &&go, std::integer_sequence<int, Is...>) {
  return with_one_of<LO + Is...>(v, go);
}
}  // namespace dispatch_detail

// go(Int<v>{}) if LO <= v <= HI; whether it was
template <int LO, int HI, class Go>
bool with_range(long v, Go &&go) {
  static_assert(LO <= HI, "an empty range");
  return dispatch_detail::with_offsets<LO>(v, go, std::make_integer_sequence<int, HI - LO + 1>{});
}

// go(std::true_type{}) or go(std::false_type{})
template <class Go>
void with_bool(bool b, Go &&go) {
  if (b) go(std::true_type{});
  else go(std::false_type{});
}
