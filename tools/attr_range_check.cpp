// attr_range_check.cpp -- drives the host half of the attribute table's seek (csrc/gm_seek.hpp: AttrKey's order
// and successor, merge_ranges) alone, against a brute-force universe.  Build with a host compiler and the
// sanitizers, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o attr_range_check tools/attr_range_check.cpp
// Prints "bad <count>" last; the exit status is 0 iff the count is 0.
#include <stdio.h>

#include <random>

#include "../geomesa_amd/csrc/gm_seek.hpp"

using gm::AttrKey;
using R = gm::SeekRange<AttrKey>;

static bool eq(const AttrKey& a, const AttrKey& b) { return !AttrKey::lt(a, b) && !AttrKey::lt(b, a); }
static bool inside(const R& r, const AttrKey& k) { return !AttrKey::lt(k, r.lo) && !AttrKey::lt(r.hi, k); }

int main() {
  // every field at its ends and in the middle, so that every carry of next() happens
  const uint32_t shards[] = {0, 1, 255};
  const uint64_t vs[] = {0, 1, 0x80000000ull, ~0ull - 1, ~0ull};
  const uint32_t bins[] = {0, 1, 0xfffe, 0xffff};
  const uint64_t ts[] = {0, 1, 1ull << 63, ~0ull - 1, ~0ull};
  std::vector<AttrKey> u;
  for (uint32_t s : shards)
    for (uint64_t v : vs)
      for (uint32_t b : bins)
        for (uint64_t t : ts) u.push_back(AttrKey{v, t, (s << 16) | b});
  long bad = 0;
  // the listing order is the key order, and it is strict
  for (size_t i = 0; i + 1 < u.size(); ++i)
    if (!AttrKey::lt(u[i], u[i + 1]) || AttrKey::lt(u[i + 1], u[i])) ++bad;
  // next(k) is greater than k, nothing of the universe lies strictly between, and only the last key has none
  for (size_t i = 0; i < u.size(); ++i) {
    AttrKey n;
    const bool has = AttrKey::next(u[i], &n);
    const bool last = (u[i].sb >> 16) == 255 && u[i].v == ~0ull && (u[i].sb & 0xffffu) == 0xffffu && u[i].t == ~0ull;
    if (has == last) ++bad;
    if (!has) continue;
    if (!AttrKey::lt(u[i], n)) ++bad;
    for (const AttrKey& k : u)
      if (AttrKey::lt(u[i], k) && AttrKey::lt(k, n)) ++bad;
    AttrKey by_hand = u[i];   // the successor written out field by field
    if (by_hand.t != ~0ull) ++by_hand.t;
    else if ((by_hand.sb & 0xffffu) != 0xffffu) { by_hand.t = 0; ++by_hand.sb; }
    else if (by_hand.v != ~0ull) { by_hand.t = 0; by_hand.sb &= 0xffff0000u; ++by_hand.v; }
    else { by_hand.t = 0; by_hand.v = 0; by_hand.sb = ((by_hand.sb >> 16) + 1) << 16; }
    if (!eq(by_hand, n)) ++bad;
  }
  // merge_ranges: the union is kept, the output is sorted, disjoint and not adjacent, no empty range survives
  std::mt19937_64 rng(7);
  for (int round = 0; round < 4000; ++round) {
    std::vector<R> in;
    const int k = (int)(rng() % 9);
    for (int j = 0; j < k; ++j) {
      AttrKey a = u[rng() % u.size()], b = u[rng() % u.size()];
      if (rng() % 4 && AttrKey::lt(b, a)) std::swap(a, b);   // a quarter of the reversed ones stay: empty ranges
      if (rng() % 3 == 0) AttrKey::next(a, &b);              // two keys long: adjacency with its neighbours
      in.push_back(R{a, b});
    }
    const std::vector<R> out = gm::merge_ranges(in);
    for (const AttrKey& key : u) {
      bool want = false, got = false;
      for (const R& r : in) want = want || inside(r, key);
      for (const R& r : out) got = got || inside(r, key);
      if (want != got) ++bad;
    }
    for (size_t i = 0; i < out.size(); ++i) {
      if (AttrKey::lt(out[i].hi, out[i].lo)) ++bad;
      AttrKey n;
      if (i + 1 < out.size() && (!AttrKey::next(out[i].hi, &n) || !AttrKey::lt(n, out[i + 1].lo))) ++bad;
    }
    if (out.size() > in.size()) ++bad;
  }
  printf("keys %zu\nbad %ld\n", u.size(), bad);
  return bad ? 1 : 0;
}
