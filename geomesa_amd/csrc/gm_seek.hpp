// gm_seek.hpp -- the host half of a table scan's seek: a scan range over a table's key, the BatchScanner's
// merge of a query's ranges, and the attribute table's key.  No HIP header: tools/attr_range_check.cpp
// tests it with a host compiler alone, under the sanitizers.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define GM_HD __host__ __device__
#else
#define GM_HD
#endif

namespace gm {

// Key: lt(a, b), the table's byte order (host and device), and next(k, &out), the key after k in that
// order (host; false when k is the last key)
template <class Key>
struct SeekRange {
  Key lo, hi;   // inclusive
};

// the BatchScanner's view of the ranges: empty ones dropped, sorted, overlapping / adjacent ones merged
template <class Key>
std::vector<SeekRange<Key>> merge_ranges(std::vector<SeekRange<Key>> rs) {
  rs.erase(std::remove_if(rs.begin(), rs.end(), [](const SeekRange<Key>& r) { return Key::lt(r.hi, r.lo); }), rs.end());
  std::sort(rs.begin(), rs.end(), [](const SeekRange<Key>& a, const SeekRange<Key>& b) { return Key::lt(a.lo, b.lo); });
  std::vector<SeekRange<Key>> out;
  for (const SeekRange<Key>& r : rs) {
    if (!out.empty()) {
      SeekRange<Key>& last = out.back();
      Key nx;   // merge when r.lo <= last.hi + 1 in key order
      if (!Key::lt(last.hi, r.lo) || (Key::next(last.hi, &nx) && !Key::lt(nx, r.lo))) {
        if (Key::lt(last.hi, r.hi)) last.hi = r.hi;
        continue;
      }
    }
    out.push_back(r);
  }
  return out;
}

// The attribute table's key: (shard, v, bin as u16, t as u64), the byte order of
// [shard][hex text of v][0x00][bin BE16][t BE64]; a column the table does not have (bin: only the Z3 tier;
// t: no tier) reads as 0.
struct AttrKey {
  uint64_t v, t;
  uint32_t sb;   // shard << 16 | (uint16) bin
  GM_HD static bool lt(const AttrKey& a, const AttrKey& b) {
    const uint32_t as = a.sb >> 16, bs = b.sb >> 16;
    if (as != bs) return as < bs;
    if (a.v != b.v) return a.v < b.v;
    const uint32_t ab = a.sb & 0xffffu, bb = b.sb & 0xffffu;
    if (ab != bb) return ab < bb;
    return a.t < b.t;
  }
  // t + 1, carrying into bin, v and the shard
  static bool next(const AttrKey& k, AttrKey* out) {
    AttrKey n = k;
    uint32_t s = k.sb >> 16, b = k.sb & 0xffffu;
    if (++n.t == 0) {
      b = (b + 1) & 0xffffu;
      if (b == 0 && ++n.v == 0) ++s;
    }
    n.sb = (s << 16) | b;
    *out = n;
    return s < 256;
  }
};

}  // namespace gm
