// gm_sort_plan.hpp -- the digit plan of gm_sort_keys (gm_sort.hip): which digit passes one sort runs,
// from n and the OR / AND of the key columns.  Host-only and free of HIP, so that a plain C++ program
// (tools/sort_plan_check.cpp) compiles the same planner the library runs.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gm {

constexpr int NPASS = 11;               // digit positions: z bytes 0..7, bin bytes 0..1, shard
constexpr int WMAX = 9;                 // widest digit: 512 buckets

struct DigitOffs {
  int off[NPASS];
  int w[NPASS];
  int np;
};
inline DigitOffs digit_offs(const std::vector<int>& offs, int w) {   // digits of one width at `offs`
  DigitOffs o{};
  o.np = (int)offs.size();
  for (int k = 0; k < o.np; ++k) { o.off[k] = offs[k]; o.w[k] = w; }
  return o;
}

// The digits of one sort, from the OR / AND of the keys: `lsd` = every byte on which some keys differ
// (LSD order); prefix mode = npre digits of pw <= 9 bits, each ending at the highest varying bit below
// the previous one (only constant bits are skipped), over the top ~log2(n) - 1 varying bits (runs of
// ~2 equal prefixes for uniform keys), when that is fewer passes than the varying bytes
struct SortPlan {
  std::vector<int> lsd;
  int npre = 0, pw = 0, pofs[4] = {-1, -1, -1, -1};
  bool prefix = false;
  int sq = 16;            // the shard's bit in bs (squeeze_bs), and bin's constant bits above it
  uint32_t binhi = 0;
  std::vector<int> first_offs() const {   // the first digit passes, LSD order
    if (!prefix) return lsd;
    std::vector<int> o(pofs, pofs + npre);
    std::reverse(o.begin(), o.end());
    return o;
  }
  DigitOffs first_digits() const { return digit_offs(first_offs(), prefix ? pw : 8); }
};
inline bool operator==(const DigitOffs& a, const DigitOffs& b) {
  if (a.np != b.np) return false;
  for (int k = 0; k < a.np; ++k)
    if (a.off[k] != b.off[k] || a.w[k] != b.w[k]) return false;
  return true;
}
static SortPlan plan_sort(const unsigned long long h_raw[4], bool sh, int64_t n, int sort_mode) {
  SortPlan p;
  unsigned long long h[4] = {h_raw[0], h_raw[1], h_raw[2], h_raw[3]};
  if (sh) {   // the digits are planned over the squeezed key (squeeze_bs)
    const uint32_t vbin = (uint32_t)((h_raw[1] ^ h_raw[3]) & 0xffffu);
    p.sq = vbin ? 32 - __builtin_clz(vbin) : 0;
    p.binhi = (uint32_t)h_raw[3] & 0xffffu & ~((1u << p.sq) - 1u);
    auto sqz = [&](unsigned long long b) {
      return (unsigned long long)(((uint32_t)b & ((1u << p.sq) - 1u)) | (((uint32_t)b >> 16) << p.sq));
    };
    h[1] = sqz(h_raw[1]);
    h[3] = sqz(h_raw[3]);
  }
  for (int b = 0; b < NPASS; ++b) {
    if (b == 10 && !sh) continue;
    const uint64_t o = b < 8 ? h[0] >> (8 * b) : h[1] >> (8 * (b - 8));
    const uint64_t a = b < 8 ? h[2] >> (8 * b) : h[3] >> (8 * (b - 8));
    if (((o ^ a) & 255u) != 0) p.lsd.push_back(8 * b);
  }
  if (p.lsd.empty()) return p;
  const uint64_t vz = h[0] ^ h[2], vb = (h[1] ^ h[3]) & 0xffffffull;
  auto varying = [&](int bit) -> bool { return bit < 64 ? ((vz >> bit) & 1u) : ((vb >> (bit - 64)) & 1u); };
  int lg = 0;
  while (((int64_t)1 << lg) < n) ++lg;
  const int pbits = std::max(1, lg - 1);
  p.npre = std::min(4, (pbits + WMAX - 1) / WMAX);
  p.pw = std::min(WMAX, (pbits + p.npre - 1) / p.npre);
  int nfound = 0;
  int bit = 87;
  for (int k = 0; k < p.npre; ++k) {
    while (bit >= 0 && !varying(bit)) --bit;
    if (bit < 0) break;
    p.pofs[k] = std::max(0, bit - (p.pw - 1));
    bit = p.pofs[k] - 1;
    ++nfound;
  }
  p.prefix = sort_mode == 0 && (int)p.lsd.size() > p.npre && nfound == p.npre;
  return p;
}

}  // namespace gm
