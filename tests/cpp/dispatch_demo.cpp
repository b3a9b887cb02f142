// dispatch_demo.cpp — the launchers' dispatch primitives (relearn_amd/csrc/dispatch.hpp) and the lane families with
// their feature ranges (relearn_amd/csrc/handle_spec.hpp through env_shape.hpp) on the CPU, one line per case on stdout:
//   range <v> <calls> <value> <returned>          with_range<3, 7>, v = 2..8
//   one_of <v> <calls> <value> <returned>         with_one_of<2, 8, 12>, v = 1..13
//   bool <b> <calls> <value>                      with_bool
//   nested <s> <a> <calls> <s seen> <a seen>      with_range<2, 4> around with_one_of<2, 5>
//   shape <kind> <states> <D> <code> <lanes> <D seen> | <message>      with_env_shape, kind 0..8, D 0..25
// (`value` is -1 where `go` did not run.)  tests/test_dispatch_cpp.py reads it.
//   g++ -std=c++17 -Wall -Wextra -Werror -I <repo> tests/cpp/dispatch_demo.cpp -o demo && ./demo
#include <iostream>

#include "relearn_amd/csrc/dispatch.hpp"
#include "relearn_amd/csrc/env_shape.hpp"

int main() {
  for (long v = 2; v <= 8; ++v) {
    int calls = 0, value = -1;
    const bool ran = with_range<3, 7>(v, [&](auto d) {
      static_assert(decltype(d)::value >= 3 && decltype(d)::value <= 7, "a constant inside the range");
      ++calls;
      value = decltype(d)::value;
    });
    std::cout << "range " << v << " " << calls << " " << value << " " << ran << "\n";
  }
  for (long v = 1; v <= 13; ++v) {
    int calls = 0, value = -1;
    const bool ran = with_one_of<2, 8, 12>(v, [&](auto d) {
      static_assert(decltype(d)::value == 2 || decltype(d)::value == 8 || decltype(d)::value == 12, "a listed constant");
      ++calls;
      value = decltype(d)::value;
    });
    std::cout << "one_of " << v << " " << calls << " " << value << " " << ran << "\n";
  }
  for (int b = 0; b < 2; ++b) {
    int calls = 0, value = -1;
    with_bool(b != 0, [&](auto t) {
      ++calls;
      value = decltype(t)::value ? 1 : 0;
    });
    std::cout << "bool " << b << " " << calls << " " << value << "\n";
  }
  for (long s = 1; s <= 5; ++s)
    for (long a = 1; a <= 6; ++a) {
      int calls = 0, s_seen = -1, a_seen = -1;
      with_range<2, 4>(s, [&](auto ss) {
        with_one_of<2, 5>(a, [&](auto aa) {
          ++calls;
          s_seen = decltype(ss)::value;
          a_seen = decltype(aa)::value;
        });
      });
      std::cout << "nested " << s << " " << a << " " << calls << " " << s_seen << " " << a_seen << "\n";
    }
  for (int kind = 0; kind <= 8; ++kind)
    for (uint32_t states : {8u, 10u})
      for (uint32_t D = 0; D <= 25; ++D) {
        std::cout << "shape " << kind << " " << states << " " << D << " ";
        int lanes = -1;
        try {
          lanes = (int)env_lanes_of(kind, states);
          int calls = 0, lanes_seen = -1, d_seen = -1;
          with_env_shape(kind, states, D, [&](auto l, auto d) {
            ++calls;
            lanes_seen = decltype(l)::value;
            d_seen = decltype(d)::value;
          });
          std::cout << (calls == 1 && lanes_seen == lanes ? 0 : -1) << " " << lanes << " " << d_seen << " |\n";
        } catch (const RlError &e) {
          std::cout << e.code << " " << lanes << " -1 | " << e.what() << "\n";
        }
      }
  return 0;
}
