// hist_replay_check.cpp -- drives the host half of Histogram (csrc/gm_hist_host.hpp: indexOf, bounds, medianValue,
// copyInto, expandBins, +=, and the record / segment / replay route gm_histogram_attr takes) over random and
// adversarial states and holds it against a plain sequential restatement of Histogram.scala / BinnedArray.scala
// written here in the bindings' own types.  Plain C++: build with a host compiler, with
// -fsanitize=address,undefined -ffp-contract=off, and run.  Prints "checked N bad 0" and exits 0 when all agree.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../geomesa_amd/csrc/gm_hist_host.hpp"

using gm::hist::Val;

// ---------------------------------------------------------------- the sequential restatement
static int64_t wsub64(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
static int64_t wadd64(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
static int32_t sat_i(double d) { return d != d ? 0 : d >= 2147483647.0 ? INT32_MAX : d <= -2147483648.0 ? INT32_MIN : (int32_t)d; }
static int64_t sat_l(double d) {
  return d != d ? 0 : d >= 9223372036854775808.0 ? INT64_MAX : d <= -9223372036854775808.0 ? INT64_MIN : (int64_t)d;
}

template <class T>
struct Seq {   // T: int64_t (Int, Long, Date), float, double
  bool is_int32;
  int length;
  T lo, hi;
  std::vector<int64_t> counts;
  int64_t expansions = 0;

  Seq(bool i32, int n, T l, T h) : is_int32(i32), length(n), lo(l), hi(h), counts((size_t)n, 0) {}
  static constexpr bool whole = std::numeric_limits<T>::is_integer;

  double size_whole() const { return (double)wsub64((int64_t)hi, (int64_t)lo) / length; }
  T size_real() const { return (hi - lo) / (T)length; }
  int clamp(int32_t i) const { return (i < 0 || i > length) ? -1 : (i == length ? length - 1 : i); }
  int index_of(T v) const {
    if (v < lo || v > hi) return -1;
    if constexpr (whole) return clamp(sat_i(floor((double)wsub64(v, lo) / size_whole())));
    else return clamp(sat_i(floor((double)((v - lo) / size_real()))));
  }
  T from_long(int64_t v) const { return is_int32 ? (T)(int32_t)(uint32_t)(uint64_t)v : (T)v; }
  void bounds(int i, T& a, T& b) const {
    if constexpr (whole) {
      const double bs = size_whole();
      const int64_t lol = wadd64(lo, sat_l(ceil(bs * i))), hif = wadd64(lo, sat_l(floor(bs * (i + 1))));
      const int64_t hil = lol > hif ? lol : hif;
      a = lol <= lo ? lo : from_long(lol);
      b = hil >= hi ? hi : from_long(hil);
    } else {
      const T bs = size_real();
      a = lo + bs * (T)i;
      b = lo + bs * (T)(i + 1);
    }
  }
  T median(int i) const {
    if constexpr (whole) {
      const double bs = size_whole(), a = bs / 2 + bs * i, f = floor(a);
      int64_t r = sat_l(f);
      if (a == a && a - f >= 0.5 && r != INT64_MAX) ++r;
      const int64_t l = wadd64(lo, a == a ? r : 0);
      return l > hi ? hi : from_long(l);
    } else {
      const T bs = size_real();
      return lo + bs / 2 + bs * (T)i;
    }
  }
  // copyInto(this, from); false where the reference throws (this is then garbage, as there)
  bool take(const Seq& from) {
    for (int i = 0; i < from.length; ++i) {
      const int64_t c = from.counts[i];
      if (c <= 0) continue;
      T a, b;
      from.bounds(i, a, b);
      auto to_index = [&](T v) { const int k = index_of(v); return k != -1 ? k : (v < lo ? 0 : length - 1); };
      const int l = to_index(a), h = to_index(b);
      if (l == h) { counts[l] = wadd64(counts[l], c); continue; }
      const int size = h - l + 1;
      if (size <= 0) return false;
      for (int j = l; j <= h; ++j) counts[j] = wadd64(counts[j], c / size);
      counts[l + size / 2] = wadd64(counts[l + size / 2], c % size);
    }
    return true;
  }
  void observe(T v, int sign) {
    int i = index_of(v);
    if (i == -1) {
      ++expansions;
      Seq grown(is_int32, length, v < lo ? v : lo, v > hi ? v : hi);
      if (!grown.take(*this)) return;
      grown.expansions = expansions;
      *this = grown;
      i = index_of(v);
      if (i == -1) return;
    }
    counts[i] = wadd64(counts[i], sign);
  }
};

// ---------------------------------------------------------------- glue
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static long checked = 0, bad = 0;
static void expect(bool ok, const char* what) {
  ++checked;
  if (!ok && ++bad <= 20) fprintf(stderr, "MISMATCH %s\n", what);
}
template <class T> static bool same(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0 || (a != a && b != b); }

template <class T> static Val val(T v) { return std::numeric_limits<T>::is_integer ? Val{(int64_t)v, 0.0} : Val{0, (double)v}; }
template <class T> static T of(Val v) { return std::numeric_limits<T>::is_integer ? (T)v.i : (T)v.f; }
template <class T> static gm_hist_state state(int type, int n, T lo, T hi) {
  return gm_hist_state{type, n, (int64_t)val(lo).i, (int64_t)val(hi).i, val(lo).f, val(hi).f};
}
template <class T> static gm_hist_state state(int type, const Seq<T>& s) { return state(type, s.length, s.lo, s.hi); }

// the route of gm_histogram_attr on the host: records by running extrema, counts per segment under the
// bounds that held, the expansions replayed
template <class T>
static void route(int type, gm_hist_state& st, std::vector<int64_t>& counts, const std::vector<T>& v, int sign, int64_t& exp) {
  size_t start = 0;
  while (start < v.size()) {
    std::vector<size_t> rec;
    gm_hist_state run = st;
    std::vector<gm_hist_state> seg{run};
    for (size_t k = start; k < v.size() && rec.size() < GM_HIST_MAX_SEGMENTS; ++k) {
      if (v[k] != v[k]) continue;
      const Val x = val(v[k]);
      bool hit = gm::hist::out_of_bounds(run, x);
      if (!hit && gm::hist::whole(type) && wsub64(run.hi, run.lo) < 0) hit = gm::hist::index_of(run, gm::hist::bin_size(run), x) == -1;
      if (!hit) continue;
      rec.push_back(k);
      run = gm::hist::expanded(run, x);
      seg.push_back(run);
    }
    // one more record ends the round
    size_t end = v.size();
    if (rec.size() == GM_HIST_MAX_SEGMENTS) {
      for (size_t k = rec.back() + 1; k < v.size(); ++k) {
        if (v[k] != v[k]) continue;
        const Val x = val(v[k]);
        bool hit = gm::hist::out_of_bounds(run, x);
        if (!hit && gm::hist::whole(type) && wsub64(run.hi, run.lo) < 0) hit = gm::hist::index_of(run, gm::hist::bin_size(run), x) == -1;
        if (hit) { end = k; break; }
      }
    }
    std::vector<std::vector<int64_t>> rows(seg.size(), std::vector<int64_t>((size_t)st.length, 0));
    for (size_t s = 0; s < seg.size(); ++s) {
      const size_t a = s == 0 ? start : rec[s - 1], b = s + 1 < seg.size() ? rec[s] : end;
      const double bs = gm::hist::bin_size(seg[s]);
      for (size_t k = a; k < b; ++k) {
        const int i = gm::hist::index_of(seg[s], bs, val(v[k]));
        if (i >= 0) rows[s][(size_t)i] += sign;
      }
    }
    for (int j = 0; j < st.length; ++j) counts[(size_t)j] = wadd64(counts[(size_t)j], rows[0][(size_t)j]);
    start = end;
    for (size_t s = 1; s < seg.size(); ++s) {
      ++exp;
      if (!gm::hist::expand(st, counts.data(), val(v[rec[s - 1]]))) { start = rec[s - 1] + 1; break; }
      for (int j = 0; j < st.length; ++j) counts[(size_t)j] = wadd64(counts[(size_t)j], rows[s][(size_t)j]);
    }
  }
}

template <class T>
static void compare(int type, const Seq<T>& s, const gm_hist_state& st, const std::vector<int64_t>& counts, const char* what) {
  expect(same(s.lo, of<T>(Val{st.lo, st.flo})) && same(s.hi, of<T>(Val{st.hi, st.fhi})), what);
  expect(s.counts == counts, what);
}

template <class T>
static void run_case(int type, int length, T lo, T hi, const std::vector<T>& v, const char* what) {
  const bool i32 = type == GM_ATTR_INT32;
  Seq<T> seq(i32, length, lo, hi);
  gm_hist_state st = state(type, length, lo, hi), st1 = st;
  std::vector<int64_t> counts((size_t)length, 0), one((size_t)length, 0);
  int64_t exp = 0;
  for (int pass = 0; pass < 2; ++pass) {   // observe, then unobserve the first half
    const int sign = pass == 0 ? 1 : -1;
    const std::vector<T> part(v.begin(), v.begin() + (pass == 0 ? v.size() : v.size() / 2));
    for (T x : part) {
      seq.observe(x, sign);
      gm::hist::observe_one(st1, one.data(), val(x), sign);
    }
    route(type, st, counts, part, sign, exp);
    compare(type, seq, st, counts, what);
    compare(type, seq, st1, one, what);
    expect(exp == seq.expansions, what);
  }
  // the per-bin entries and a merge into a histogram of another shape
  const gm_hist_state now = state(type, seq);
  const double bs = gm::hist::bin_size(now);
  for (int i = 0; i <= length; i += (length > 64 ? length / 13 : 1)) {
    T a, b;
    seq.bounds(i, a, b);
    Val va, vb;
    gm::hist::bin_bounds(now, bs, i, va, vb);
    expect(same(a, of<T>(va)) && same(b, of<T>(vb)), "bounds(i)");
    expect(same(seq.median(i), of<T>(gm::hist::median(now, bs, i))), "medianValue(i)");
  }
  for (T x : v) expect(seq.index_of(x) == gm::hist::index_of(now, bs, val(x)), "indexOf");
}

template <class T>
static void merge_case(int type, const Seq<T>& a0, const Seq<T>& b) {
  // += of the restatement, by the source's branches
  Seq<T> a = a0;
  gm_hist_state sa = state(type, a), sb = state(type, b);
  std::vector<int64_t> ca = a.counts;
  ca.resize((size_t)(a.length > b.length ? a.length : b.length), 0);
  const bool ok = gm::hist::merge(sa, ca.data(), sb, b.counts.data());
  Seq<T> to(a.is_int32, b.length, b.lo, b.hi);   // copyInto alone, into b's shape
  std::vector<int64_t> ct((size_t)b.length, 0);
  const bool tk = to.take(a), ck = gm::hist::copy_into(sb, ct.data(), state(type, a), a.counts.data());
  expect(tk == ck && (!tk || to.counts == ct), "copyInto");
  int64_t sum_a = 0, sum_b = 0, sum_m = 0;
  for (int64_t c : a.counts) sum_a += c;
  for (int64_t c : b.counts) sum_b += c;
  for (int i = 0; i < sa.length; ++i) sum_m += ca[(size_t)i];
  if (ok) expect(sum_m == sum_a + sum_b, "+= keeps the total");   // counts > 0 only: the cases here observe
}

template <class T>
static std::vector<T> draw(int n, double centre, double sigma, int kind) {
  std::vector<T> v;
  for (int i = 0; i < n; ++i) {
    double x;
    switch (kind) {
      case 0: x = centre + sigma * (unit() + unit() + unit() + unit() - 2.0); break;   // bell
      case 1: x = centre + i * sigma / n; break;                                          // ascending
      case 2: x = centre - i * sigma / n; break;                                          // descending
      case 3: x = centre; break;                                                          // all equal
      default: x = centre + ((i & 1) ? 1.0 : -1.0) * (i + 1) * sigma / n; break;          // alternating records
    }
    v.push_back((T)x);
  }
  return v;
}

int main() {
  const int lengths[] = {1, 2, 7, 1000};
  for (int kind = 0; kind < 5; ++kind) {
    for (int length : lengths) {
      const int n = kind == 1 || kind == 2 ? 2 * GM_HIST_MAX_SEGMENTS + 5 : 700;
      run_case<int64_t>(GM_ATTR_INT32, length, -100, 100, draw<int64_t>(n, 0, 100000, kind), "int");
      run_case<int64_t>(GM_ATTR_INT64, length, -100, 100, draw<int64_t>(n, 0, 1e15, kind), "long");
      run_case<float>(GM_ATTR_FLOAT32, length, -100.f, 100.f, draw<float>(n, 0, 1000, kind), "float");
      run_case<double>(GM_ATTR_FLOAT64, length, -100., 100., draw<double>(n, 0, 1000, kind), "double");
    }
  }
  // adversarial: NaN, infinities, signed zeros, values on a bound and one ulp outside, Long spans that wrap
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int length : lengths) {
    run_case<double>(GM_ATTR_FLOAT64, length, -1., 1., {0.5, nan, -0.0, 0.0, 1.0, nextafter(1.0, 2.0), -1.0, nextafter(-1.0, -2.0), 0.25, inf, 3.0, nan, -inf, 7.0}, "double edges");
    run_case<float>(GM_ATTR_FLOAT32, length, -1.f, 1.f, {0.5f, (float)nan, -0.0f, 0.0f, 1.0f, nextafterf(1.0f, 2.0f), -1.0f, nextafterf(-1.0f, -2.0f), 0.25f, (float)inf, 3.0f, (float)-inf, 7.0f}, "float edges");
    run_case<int64_t>(GM_ATTR_INT64, length, INT64_MIN + 50, INT64_MIN + 90, {INT64_MIN + 60, INT64_MIN, INT64_MIN + 70, 5, INT64_MAX - 3, 0, INT64_MAX, INT64_MIN + 1, -7}, "long near MinValue");
    run_case<int64_t>(GM_ATTR_INT64, length, INT64_MAX - 90, INT64_MAX - 50, {INT64_MAX - 60, INT64_MAX, INT64_MAX - 70, -5, INT64_MIN + 3, 0, INT64_MIN, INT64_MAX - 1, 7}, "long near MaxValue");
    run_case<int64_t>(GM_ATTR_INT32, length, INT32_MAX - 90, INT32_MAX - 50, {INT32_MAX, INT32_MAX - 60, INT32_MIN, 0, INT32_MAX}, "int extremes");
    run_case<double>(GM_ATTR_FLOAT64, length, -1.7976931348623157e308, 1.7976931348623157e308, {0.0, 1e308, -1e308, 5e-324}, "double span overflow");
  }
  // merges and copyInto over random pairs
  for (int round = 0; round < 300; ++round) {
    const int la = 1 + (int)(rnd() % 40), lb = 1 + (int)(rnd() % 40);
    const double c1 = 2000 * unit() - 1000, c2 = 2000 * unit() - 1000;
    Seq<int64_t> a(false, la, (int64_t)c1 - 100, (int64_t)c1 + 100), b(false, lb, (int64_t)c2 - 50, (int64_t)c2 + 300);
    for (int64_t x : draw<int64_t>(200, c1, 300, 0)) a.observe(x, 1);
    if (round % 7) for (int64_t x : draw<int64_t>(200, c2, 300, 0)) b.observe(x, 1);
    merge_case<int64_t>(GM_ATTR_INT64, a, b);
    Seq<double> fa(false, la, c1 - 100, c1 + 100), fb(false, lb, c2 - 50, c2 + 300);
    for (double x : draw<double>(200, c1, 300, 0)) fa.observe(x, 1);
    if (round % 5) for (double x : draw<double>(200, c2, 300, 0)) fb.observe(x, 1);
    merge_case<double>(GM_ATTR_FLOAT64, fa, fb);
    Seq<float> ga(false, la, (float)c1 - 100, (float)c1 + 100), gb(false, lb, (float)c2 - 50, (float)c2 + 300);
    for (float x : draw<float>(200, c1, 300, 0)) ga.observe(x, 1);
    for (float x : draw<float>(200, c2, 300, 0)) gb.observe(x, 1);
    merge_case<float>(GM_ATTR_FLOAT32, ga, gb);
  }
  printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
