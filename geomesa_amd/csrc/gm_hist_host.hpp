// gm_hist_host.hpp -- the host half of Histogram (utils/stats/Histogram.scala over BinnedArray.scala): the
// binnings of the whole-number, float and double bindings, copyInto, expandBins and += in plain C++.  No HIP
// header: gm_hist.hip's replay and host entries call it, and tools/hist_replay_check.cpp compiles it alone
// with a host compiler.  The contract is in include/geomesa_hip.h.  Long arithmetic wraps as the JVM's, so
// every sum and difference goes through uint64_t; d2i / d2l saturate and map NaN to 0.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/geomesa_hip.h"

namespace gm {
namespace hist {

inline int32_t d2i(double d) {
  if (!(d == d)) return 0;
  if (d >= 2147483647.0) return INT32_MAX;
  if (d <= -2147483648.0) return INT32_MIN;
  return (int32_t)d;
}
inline int64_t d2l(double d) {
  if (!(d == d)) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
inline int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
inline int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
// Math.round(double): floor(a + 1/2) without the double rounding of the sum
inline int64_t jround(double a) {
  if (!(a == a)) return 0;
  const double f = floor(a);
  const int64_t r = d2l(f);
  return (a - f >= 0.5 && r != INT64_MAX) ? r + 1 : r;
}
// the order of Double.compareTo as a signed key: NaN (canonical) above +Infinity, -0.0 below 0.0
inline int64_t order_key(double v) {
  int64_t b;
  if (!(v == v)) return 0x7ff8000000000000LL;
  memcpy(&b, &v, 8);
  return b ^ ((b >> 63) & INT64_MAX);
}

inline bool whole(int type) { return type == GM_ATTR_INT32 || type == GM_ATTR_INT64; }
inline bool known(int type) { return whole(type) || type == GM_ATTR_FLOAT32 || type == GM_ATTR_FLOAT64; }

// a value of any binding: i for the whole numbers, f for float (exactly widened) and double
struct Val {
  int64_t i;
  double f;
};

// BinnedArray.scala:187-193, :289, :323
inline double bin_size(const gm_hist_state& s) {
  if (whole(s.type)) return (double)wsub(s.hi, s.lo) / s.length;
  if (s.type == GM_ATTR_FLOAT32) return (double)(((float)s.fhi - (float)s.flo) / (float)s.length);
  return (s.fhi - s.flo) / s.length;
}

inline int clamp_index(int32_t i, int length) { return (i < 0 || i > length) ? -1 : (i == length ? length - 1 : i); }

// directIndex / indexOf (BinnedArray.scala:195-201, :293-299, :327-333); bs = bin_size(s)
inline int index_of(const gm_hist_state& s, double bs, Val v) {
  if (whole(s.type)) {
    if (v.i < s.lo || v.i > s.hi) return -1;
    return clamp_index(d2i(floor((double)wsub(v.i, s.lo) / bs)), s.length);
  }
  if (v.f < s.flo || v.f > s.fhi) return -1;
  if (s.type == GM_ATTR_FLOAT32) return clamp_index(d2i(floor((double)(((float)v.f - (float)s.flo) / (float)bs))), s.length);
  return clamp_index(d2i(floor((v.f - s.flo) / bs)), s.length);
}

inline bool is_below(const gm_hist_state& s, Val v) { return whole(s.type) ? v.i < s.lo : v.f < s.flo; }

// bounds(index) (BinnedArray.scala:213-223, :308-313, :342-347); 0 <= index <= length as the reference allows
inline void bin_bounds(const gm_hist_state& s, double bs, int index, Val& lo, Val& hi) {
  lo = hi = Val{0, 0.0};
  if (whole(s.type)) {
    const int64_t lol = wadd(s.lo, d2l(ceil(bs * index)));
    const int64_t hif = wadd(s.lo, d2l(floor(bs * (index + 1))));
    const int64_t hil = lol > hif ? lol : hif;
    lo.i = lol <= s.lo ? s.lo : lol;
    hi.i = hil >= s.hi ? s.hi : hil;
    if (s.type == GM_ATTR_INT32) {   // convertFromLong = toInt
      lo.i = (int32_t)(uint32_t)(uint64_t)lo.i;
      hi.i = (int32_t)(uint32_t)(uint64_t)hi.i;
    }
  } else if (s.type == GM_ATTR_FLOAT32) {
    const float b = (float)bs, l = (float)s.flo;
    lo.f = (double)(l + b * (float)index);
    hi.f = (double)(l + b * (float)(index + 1));
  } else {
    lo.f = s.flo + bs * index;
    hi.f = s.flo + bs * (index + 1);
  }
}

// medianValue(index) (BinnedArray.scala:205-211, :301-306, :335-340)
inline Val median(const gm_hist_state& s, double bs, int index) {
  Val m{0, 0.0};
  if (whole(s.type)) {
    const int64_t l = wadd(s.lo, jround(bs / 2 + bs * index));
    m.i = l > s.hi ? s.hi : l;
    if (s.type == GM_ATTR_INT32) m.i = (int32_t)(uint32_t)(uint64_t)m.i;
  } else if (s.type == GM_ATTR_FLOAT32) {
    const float b = (float)bs;
    m.f = (double)((float)s.flo + b / 2 + b * (float)index);
  } else {
    m.f = s.flo + bs / 2 + bs * index;
  }
  return m;
}

// Histogram.copyInto (Histogram.scala:260-292).  false: the reference's require(size > 0) fails; `to` is then
// left as it was (the reference drops the half-filled array with the exception).
inline bool copy_into(const gm_hist_state& to, int64_t* to_counts, const gm_hist_state& from, const int64_t* from_counts) {
  const double tbs = bin_size(to), fbs = bin_size(from);
  std::vector<int64_t> out(to_counts, to_counts + to.length);
  auto to_index = [&](Val v) {
    const int i = index_of(to, tbs, v);
    return i != -1 ? i : (is_below(to, v) ? 0 : to.length - 1);
  };
  for (int i = 0; i < from.length; ++i) {
    const int64_t count = from_counts[i];
    if (count <= 0) continue;
    Val mn, mx;
    bin_bounds(from, fbs, i, mn, mx);
    const int lo = to_index(mn), hi = to_index(mx);
    if (lo == hi) {
      out[lo] = wadd(out[lo], count);
      continue;
    }
    const int size = hi - lo + 1;
    if (size <= 0) return false;
    const int64_t avg = count / size, rem = count % size;
    for (int j = lo; j <= hi; ++j) out[j] = wadd(out[j], avg);
    out[lo + size / 2] = wadd(out[lo + size / 2], rem);
  }
  memcpy(to_counts, out.data(), sizeof(int64_t) * (size_t)to.length);
  return true;
}

inline bool out_of_bounds(const gm_hist_state& s, Val v) { return whole(s.type) ? (v.i < s.lo || v.i > s.hi) : (v.f < s.flo || v.f > s.fhi); }

// the bounds of expandBins (Histogram.scala:226-229): the value is outside by the primitive order (or, for
// a Long span that wrapped, inside: the bounds then stay), where compareTo and the primitive order agree
inline gm_hist_state expanded(const gm_hist_state& s, Val v) {
  gm_hist_state e = s;
  if (whole(s.type)) {
    if (v.i < s.lo) e.lo = v.i;
    if (v.i > s.hi) e.hi = v.i;
  } else {
    if (v.f < s.flo) e.flo = v.f;
    if (v.f > s.fhi) e.fhi = v.f;
  }
  return e;
}

// expandBins (Histogram.scala:226-232) for a value whose indexOf is -1.  false: copyInto threw, nothing
// changed (observe logs a warning and drops the feature).
inline bool expand(gm_hist_state& s, int64_t* counts, Val v) {
  const gm_hist_state e = expanded(s, v);
  std::vector<int64_t> fresh((size_t)s.length, 0);
  if (!copy_into(e, fresh.data(), s, counts)) return false;
  memcpy(counts, fresh.data(), sizeof(int64_t) * (size_t)s.length);
  s = e;
  return true;
}

// One feature of observe (sign +1) / unobserve (-1) (Histogram.scala:74-106)
inline void observe_one(gm_hist_state& s, int64_t* counts, Val v, int sign) {
  int i = index_of(s, bin_size(s), v);
  if (i == -1) {
    if (!expand(s, counts, v)) return;
    i = index_of(s, bin_size(s), v);   // add(value): a Long span that wrapped can still refuse it
    if (i == -1) return;
  }
  counts[i] = wadd(counts[i], sign);
}

inline bool same_bounds(const gm_hist_state& a, const gm_hist_state& b) {
  return whole(a.type) ? (a.lo == b.lo && a.hi == b.hi) : (a.flo == b.flo && a.fhi == b.fhi);
}
inline bool all_zero(const int64_t* c, int n) {
  for (int i = 0; i < n; ++i) if (c[i] != 0) return false;
  return true;
}

// getActualBounds (Histogram.scala:247-253)
inline void actual_bounds(const gm_hist_state& s, const int64_t* c, Val& mn, Val& mx) {
  int first = -1, last = -1;
  for (int i = 0; i < s.length; ++i) if (c[i] != 0) { if (first < 0) first = i; last = i; }
  const int max_index = last < 0 ? s.length : last;   // length - (-1) - 1 when nothing is set
  const double bs = bin_size(s);
  Val a, b;
  mn = Val{s.lo, s.flo};
  mx = Val{s.hi, s.fhi};
  if (first > 0) { bin_bounds(s, bs, first, a, b); mn = a; }
  if (max_index < s.length - 1) { bin_bounds(s, bs, max_index, a, b); mx = b; }
}

// Histogram.+= (Histogram.scala:123-154).  a_counts holds max(a.length, b.length) entries.  false: a copyInto
// of the last branch threw; a and a_counts are then as the reference leaves them (the first copy may have
// been taken).
inline bool merge(gm_hist_state& a, int64_t* a_counts, const gm_hist_state& b, const int64_t* b_counts) {
  if (a.length == b.length && same_bounds(a, b)) {
    for (int i = 0; i < a.length; ++i) a_counts[i] = wadd(a_counts[i], b_counts[i]);
    return true;
  }
  if (all_zero(b_counts, b.length)) return true;
  if (all_zero(a_counts, a.length)) {
    a = b;
    memcpy(a_counts, b_counts, sizeof(int64_t) * (size_t)b.length);
    return true;
  }
  Val lmn, lmx, rmn, rmx;
  actual_bounds(a, a_counts, lmn, lmx);
  actual_bounds(b, b_counts, rmn, rmx);
  gm_hist_state e = a;
  e.length = a.length > b.length ? a.length : b.length;
  if (whole(a.type)) {   // defaults.min / max by compareTo; a tie keeps the left
    e.lo = lmn.i > rmn.i ? rmn.i : lmn.i;
    e.hi = lmx.i < rmx.i ? rmx.i : lmx.i;
  } else {
    e.flo = order_key(lmn.f) > order_key(rmn.f) ? rmn.f : lmn.f;
    e.fhi = order_key(lmx.f) < order_key(rmx.f) ? rmx.f : lmx.f;
  }
  if (!same_bounds(e, a) || e.length != a.length) {
    if (whole(e.type) ? !(e.lo < e.hi) : !(e.flo < e.fhi)) return false;   // BinnedArray's require
    std::vector<int64_t> fresh((size_t)e.length, 0);
    if (!copy_into(e, fresh.data(), a, a_counts)) return false;
    memcpy(a_counts, fresh.data(), sizeof(int64_t) * (size_t)e.length);
    a = e;
  }
  return copy_into(a, a_counts, b, b_counts);
}

// the state's own errors; null: none
inline const char* state_check(const gm_hist_state* s) {
  if (!s) return "NULL histogram state";
  if (s->type == GM_ATTR_UTF8) return "GM_ATTR_UTF8: a String histogram bins base-36 prefixes, which is not restated";
  if (!known(s->type)) return "unknown attribute type";
  if (s->length < 1) return "length must be at least 1";
  if (whole(s->type) ? !(s->lo < s->hi) : !(s->flo < s->fhi)) return "the upper bound must be greater than the lower bound";
  if (s->type == GM_ATTR_INT32 && (s->lo < INT32_MIN || s->hi > INT32_MAX)) return "Int bounds outside the Int range";
  if (s->type == GM_ATTR_FLOAT32 && ((double)(float)s->flo != s->flo || (double)(float)s->fhi != s->fhi))
    return "Float bounds must be float32 values";
  return nullptr;
}

}  // namespace hist
}  // namespace gm
