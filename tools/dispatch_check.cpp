// dispatch_check.cpp -- host-only check of geomesa_amd/csrc/gm_dispatch.hpp: every run-time switch value
// reaches the callable as the matching compile-time constant, in argument order, and the callable's
// result comes back.  Prints "bad 0" on success.
//   c++ -std=c++17 -o dispatch_check tools/dispatch_check.cpp && ./dispatch_check
#include <cstdio>

#include "../geomesa_amd/csrc/gm_dispatch.hpp"

int main() {
  int bad = 0, calls = 0;
  for (int m = 0; m < 8; ++m) {
    const bool a = m & 4, b = m & 2, c = m & 1;
    const int got = gm::with_flags(
        [&](auto A, auto B, auto C) {
          static_assert(std::is_same<decltype(A()), bool>::value, "flags arrive as integral_constant<bool>");
          constexpr int packed = (A() ? 4 : 0) | (B() ? 2 : 0) | (C() ? 1 : 0);   // usable as template arguments
          ++calls;
          return packed;
        },
        a, b, c);
    if (got != m) { std::printf("with_flags(%d, %d, %d) handed over %d\n", a, b, c, got); ++bad; }
  }
  if (calls != 8) { std::printf("with_flags called f %d times for 8 combinations\n", calls); ++bad; }
  if (gm::with_flags([] { return 7; }) != 7) { std::printf("with_flags without flags\n"); ++bad; }

  // the library's `switch (period) ... default:`: 0-3 map to themselves, anything else to GM_YEAR
  const int periods[][2] = {{GM_DAY, GM_DAY}, {GM_WEEK, GM_WEEK}, {GM_MONTH, GM_MONTH}, {GM_YEAR, GM_YEAR},
                            {7, GM_YEAR}, {-1, GM_YEAR}};
  for (const auto& p : periods) {
    const int got = gm::with_period(p[0], [](auto P) {
      constexpr int v = P();
      return v;
    });
    if (got != p[1]) { std::printf("with_period(%d) handed over %d, expected %d\n", p[0], got, p[1]); ++bad; }
  }

  // with_value: the listed value, else the last one listed
  const int values[][2] = {{5, 5}, {9, 9}, {2, 2}, {0, 2}, {-5, 2}};
  for (const auto& v : values) {
    const int got = gm::with_value<5, 9, 2>(v[0], [](auto V) { return (int)V(); });
    if (got != v[1]) { std::printf("with_value(%d) handed over %d, expected %d\n", v[0], got, v[1]); ++bad; }
  }

  // a void callable and a nested use, as the entry points write it
  int seen = -1;
  gm::with_period(GM_MONTH, [&](auto P) {
    gm::with_flags([&](auto L, auto S) { seen = P() * 4 + (L() ? 2 : 0) + (S() ? 1 : 0); }, true, false);
  });
  if (seen != GM_MONTH * 4 + 2) { std::printf("nested dispatch handed over %d\n", seen); ++bad; }

  std::printf("bad %d\n", bad);
  return bad != 0;
}
