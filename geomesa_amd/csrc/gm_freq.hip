// gm_freq.hip -- Frequency.observe and Z3Frequency.observe over a batch of features on gfx950: the two
// count-min stats (the third and fourth callers of the curves after the key spaces and Z3Histogram).
//
// Reference: Z3Frequency (utils/stats/Z3Frequency.scala:54-60, 104-115) and Frequency
// (utils/stats/Frequency.scala:159-168, 284-306) turn a feature into (time bin, Long key) and call
// CountMinSketch.add(key, 1) (utils/clearspring/CountMinSketch.scala:48-73) on that bin's sketch: for
// every hash row i < depth, table(i)(hash(key, i)) += 1, and size += 1.  The contract -- key rules, the
// dense block that stands for the map of sketches, the three tallies -- is in include/geomesa_hip.h.
//
// Shape: k_z3_hist_lds (gm_stats.hip) with `depth` increments per row where the histogram has one.  The
// same streaming read (16-B non-temporal pair loads when every column is 16-B aligned, the next pairs in
// flight while the current ones are hashed), a key functor per source fused into the scan (freq_row: no
// key column is written and read back), and every workgroup keeps a block of time bins in LDS as uint32
// counters, depth * width + 1 per bin: the sketch's rows and, last, the bin's size.  A row adds to exactly
// one counter of hash row 0, so the size is not counted per row (every lane of a wave would hit the one
// LDS word): the flush sums hash row 0 into it.  The flush is one 64-bit device atomic per nonzero
// counter; the grid is one resident wave of workgroups, raised so that a workgroup sees fewer than 2^31
// rows and no counter wraps.  A window of more bins than one LDS block takes several passes over the
// rows, a block of bins each (a row of another pass's bin leaves before it is hashed); beyond
// FREQ_MAX_PASSES, or when one bin alone does not fit, every increment is a device atomic on the table
// (k_freq<.., LDS = false>), the sizes added once per wave and bin.  Under a mask a pair of rows is
// loaded only when one of its bits is set, so the rows of a zero mask word are never read.
#include <algorithm>

#include "gm_arrow.hpp"
#include "gm_keys.hpp"
#include "gm_scan.hpp"

namespace gm {

constexpr int QTPB = 1024;
constexpr int FREQ_LDS_INTS = 32768;   // uint32 counters per workgroup (128 KB of the 160 KB LDS, as HIST_LDS_MAX)
// LDS passes beyond which the device-atomic kernel runs instead.  Measured over 1B points at depth 5 x width
// 400 (tools/frequency_probe.py, profiles/frequency_probe.json): one LDS pass 6.2-6.9 ms, 2 / 4 / 8 passes
// 12.4 / 24.6 / 41.4 ms (6.2 ms a pass, less for a pass whose bins hold no rows), against 4.4 ms for
// Z3Histogram's one increment per row; the device-atomic kernel 493 ms into one bin and 2,051 ms into 54
// (2.4-10 G increments/s: 2,000 counters per bin are few, hot lines).  So atomics catch up only after 80
// passes at their best and 330 at 54 bins; 64 passes x 6.2 ms = 0.40 s stays below the fastest atomic run
// measured.  The histogram's HIST_MAX_PASSES = 4 came from scattered atomics at 22 G/s; these are not.
constexpr int FREQ_MAX_PASSES = 64;

enum : int { K_Z3 = 0, K_Z2 = 1, K_I32 = 2, K_I64 = 3, K_F32 = 4, K_F64 = 5 };

struct FreqSrc {
  const double* x;          // K_Z3, K_Z2
  const double* y;
  const int64_t* t;         // K_Z3: t_ms; the other sources: the dtg column (null: time bin 0)
  const uint8_t* t_valid;
  int64_t t_voff;
  const void* v;            // the attribute column's values
  const uint8_t* v_valid;
  int64_t v_voff;
};

struct FreqArgs {
  RowSel sel;
  int depth, width;
  int cells;          // depth * width + 1: the LDS counters of one time bin, the last one its size
  int bin_lo, n_bins;
  int row_lo, row_n;  // this pass counts the bins [row_lo, row_lo + row_n) of the window
  int first;          // this pass reports the tallies (every row is seen by every pass)
  int period;         // of the dtg column (K_Z3 takes the period as a template argument)
  int prec;           // the attribute rules' divisor / factor
  int64_t zmask;      // Frequency.getMask(precision), the curve sources
  NDim lon, lat, tim;
  int64_t hash_a[GM_CMS_MAX_DEPTH];
};

// CountMinSketch.hash (CountMinSketch.scala:48-57): hashA(i) * item wrapping, += the arithmetic >> 32, the low
// 31 bits, then the Int remainder by width (both operands non-negative)
__device__ __forceinline__ int cms_bucket(int64_t a, int64_t item, int width) {
  const uint32_t alo = (uint32_t)a, ahi = (uint32_t)((uint64_t)a >> 32);
  uint64_t h = (uint64_t)alo * (uint64_t)item;
  if (ahi) h += (uint64_t)(ahi * (uint32_t)item) << 32;   // uniform; nextInt(Int.MaxValue) never has high bits
  h += (uint64_t)((int64_t)h >> 32);
  return (int)((uint32_t)(h & 0x7fffffffull) % (uint32_t)width);
}

// Math.round(float): the closest int, ties toward +Infinity, NaN -> 0, saturating.  a - floor(a) is exact,
// and not below 0.5 for an |a| >= 2^23 (an integer), so the increment cannot overflow.
__device__ __forceinline__ int32_t jvm_round_f(float a) {
  if (!(a == a)) return 0;
  const float f = floorf(a);
  int32_t r = f >= 2147483648.0f ? INT32_MAX : (f <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)f);
  if (a - f >= 0.5f) ++r;
  return r;
}
// Math.round(double): the closest long, likewise
__device__ __forceinline__ int64_t jvm_round_d(double a) {
  const double f = floor(a);
  int64_t r = jvm_d2l(f);
  if (a - f >= 0.5) ++r;
  return r;
}

__device__ __forceinline__ uint8_t binned_time_of(int period, int64_t ms, int16_t& b) {
  int64_t off;
  switch (period) {
    case DAY: return binned_time<DAY>(ms, b, off);
    case WEEK: return binned_time<WEEK>(ms, b, off);
    case MONTH: return binned_time<MONTH>(ms, b, off);
    default: return binned_time<YEAR>(ms, b, off);
  }
}

// One row -> (time bin, key).  0: observe it; 1: the reference throws (BinnedTime's require, the curve's
// bounds check; a NaN ordinate fails the latter) -> tally[0]; 2: a null attribute slot, not observed.
// x / y: the ordinates (curve sources); raw: the attribute value (sign-extended, or the float's / double's bits).
template <int KEY, int PERIOD>
__device__ __forceinline__ int freq_row(const FreqSrc& s, const FreqArgs& a, const uint32_t* sp, int64_t r, double x,
                                        double y, int64_t raw, int64_t t, int& bin, int64_t& key) {
  if constexpr (KEY == K_Z3) {   // Z3Frequency.toKey (Z3Frequency.scala:54-60): the spread through the LDS table, as hist_slot_tab
    int16_t b;
    int64_t off;
    if (binned_time<PERIOD>(t, b, off) != ST_OK) return 1;
    const double td = (double)off;
    const bool inb = x >= a.lon.min && x <= a.lon.max && y >= a.lat.min && y <= a.lat.max && td >= a.tim.min &&
                     td <= a.tim.max;
    if (!inb) return 1;
    key = (int64_t)(z3_split_tab(normalize(a.lon, x), sp) | (z3_split_tab(normalize(a.lat, y), sp) << 1) |
                    (z3_split_tab(normalize(a.tim, td), sp) << 2)) & a.zmask;
    bin = b;
    return 0;
  }
  if (KEY >= K_I32 && !arrow_valid(s.v_valid, s.v_voff, r)) return 2;
  bin = 0;   // Frequency.DefaultTimeBin: no dtg, or a null date (Frequency.scala:162-165)
  if (s.t && arrow_valid(s.t_valid, s.t_voff, r)) {
    int16_t b;
    if (binned_time_of(a.period, t, b) != ST_OK) return 1;
    bin = b;
  }
  if (KEY == K_Z2) {          // geomToKey (Frequency.scala:289-293)
    int64_t z;
    if (z2_index_one<false>(x, y, a.lon, a.lat, z) != ST_OK) return 1;
    key = z & a.zmask;
  } else if (KEY == K_I32) {  // intToKey: Int division, widened (prec >= 1: no INT_MIN / -1)
    key = (int64_t)((int32_t)raw / a.prec);
  } else if (KEY == K_I64) {  // longToKey, dateToKey
    key = a.prec == 1 ? raw : raw / (int64_t)a.prec;
  } else if (KEY == K_F32) {  // floatToKey: a float product, Math.round(float): Int
    key = (int64_t)jvm_round_f(__int_as_float((int32_t)raw) * (float)a.prec);
  } else {                    // doubleToKey
    key = jvm_round_d(__longlong_as_double(raw) * (double)a.prec);
  }
  return 0;
}

// size[rb] += 1 for every lane with rb >= 0, one device atomic per distinct bin of the wave (the rows of a
// wave mostly share theirs; one atomic per row would put every lane of the grid on a few words).  Called
// by whole waves.
__device__ __forceinline__ void wave_size_add(unsigned long long* __restrict__ size, int rb) {
  const int lane = threadIdx.x & 63;
  uint64_t todo = __ballot(rb >= 0);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int b = __shfl(rb, leader, 64);
    const uint64_t same = __ballot(rb == b);
    if (lane == leader) atomicAdd(&size[b], (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// KEY: the source and its key rule.  PERIOD: K_Z3's (the other sources read a.period).  SEL: every row, the
// rows of a mask, or the rows ids names.  LDS: the pass's bins live in LDS and are flushed at the end; else
// every increment is a device atomic.  VEC (LDS, 8-byte columns, no ids): 16-B pair loads.
template <int KEY, int PERIOD, int SEL, bool LDS, bool VEC>
__global__ __launch_bounds__(QTPB) void k_freq(FreqSrc s, FreqArgs a, unsigned long long* __restrict__ table,
                                               unsigned long long* __restrict__ size,
                                               unsigned long long* __restrict__ tally) {
  extern __shared__ uint32_t freq_lds[];
  const int total = LDS ? a.row_n * a.cells : 0;
  uint32_t* cnt = freq_lds;            // [row_n][cells]
  uint32_t* sp = freq_lds + total;     // [2048]: spread3_11 table (K_Z3)
  __shared__ unsigned long long s_tally[3];
  for (int i = threadIdx.x; i < total; i += QTPB) cnt[i] = 0u;
  if (KEY == K_Z3) fill_spread_table(sp, threadIdx.x, QTPB);
  if (threadIdx.x < 3) s_tally[threadIdx.x] = 0ull;
  __syncthreads();
  const int dw = a.cells - 1;
  unsigned skip = 0, out = 0, bad = 0;   // a workgroup sees fewer than 2^31 entries
  // one row, its values loaded; returns the row's bin of the window when it was added (the atomic form's sizes)
  auto one = [&](int64_t r, int64_t av, int64_t bv, int64_t tv) -> int {
    int bin = 0;
    int64_t key = 0;
    const int st = freq_row<KEY, PERIOD>(s, a, sp, r, __longlong_as_double(av), __longlong_as_double(bv), av, tv, bin, key);
    const int rb = bin - a.bin_lo;
    const bool inside = (unsigned)rb < (unsigned)a.n_bins;
    // both counters move on every row, by 0 or 1: counted under the branches, the two share a select of
    // their addresses and live in scratch
    skip += st == 1;
    out += (st == 0) & !inside;
    if (st != 0 || !inside) return -1;
    if (LDS) {
      const int pb = rb - a.row_lo;
      if ((unsigned)pb >= (unsigned)a.row_n) return -1;   // a bin of another pass
      uint32_t* c = cnt + pb * a.cells;
      for (int i = 0; i < a.depth; ++i) atomicAdd(&c[i * a.width + cms_bucket(a.hash_a[i], key, a.width)], 1u);
    } else {
      unsigned long long* c = table + (int64_t)rb * dw;
      for (int i = 0; i < a.depth; ++i) atomicAdd(&c[i * a.width + cms_bucket(a.hash_a[i], key, a.width)], 1ull);
    }
    return rb;
  };
  auto row = [&](int64_t r) -> int {   // 0 <= r < a.sel.n, scalar loads
    int64_t av = 0, bv = 0, tv = 0;
    if (KEY == K_Z3 || KEY == K_Z2) {
      av = __double_as_longlong(s.x[r]);
      bv = __double_as_longlong(s.y[r]);
    } else if (KEY == K_I32) {
      av = ((const int32_t*)s.v)[r];
    } else if (KEY == K_F32) {
      av = __float_as_int(((const float*)s.v)[r]);
    } else {
      av = ((const int64_t*)s.v)[r];
    }
    if (KEY == K_Z3 || s.t) tv = s.t[r];
    return one(r, av, bv, tv);
  };
  const int64_t stride = (int64_t)gridDim.x * QTPB;
  if constexpr (VEC) {
    const lv2* A2 = (const lv2*)((KEY == K_Z3 || KEY == K_Z2) ? (const void*)s.x : s.v);
    const lv2* B2 = (const lv2*)s.y;
    const lv2* T2 = (const lv2*)s.t;
    constexpr bool XY = KEY == K_Z3 || KEY == K_Z2;
    const bool has_t = KEY == K_Z3 || s.t != nullptr;
    const int64_t np = a.sel.n >> 1;
    if constexpr (SEL == SEL_MASK) {
      // pair q = rows 2q and 2q + 1, both in mask word q >> 5; loaded only when selected
      for (int64_t q = (int64_t)blockIdx.x * QTPB + threadIdx.x; q < np; q += stride) {
        bool se, so;
        mask_pair(a.sel.mask[q >> 5], q, se, so);
        if (!(se || so)) continue;
        lv2 av = ld_stream(&A2[q]), bv = av, tv = av;
        if (XY) bv = ld_stream(&B2[q]);
        if (has_t) tv = ld_stream(&T2[q]);
        if (se) one(2 * q, av.x, bv.x, tv.x);
        if (so) one(2 * q + 1, av.y, bv.y, tv.y);
      }
    } else {
      // software-pipelined with unconditional (clamped) loads, as k_z3_hist_lds
      constexpr int HU = 2;
      lv2 xa[HU], ya[HU], ta[HU];
      auto load = [&](int64_t q, lv2& av, lv2& bv, lv2& tv) {
        const int64_t qc = q < np ? q : np - 1;
        av = ld_stream(&A2[qc]);
        bv = av;
        tv = av;
        if (XY) bv = ld_stream(&B2[qc]);
        if (has_t) tv = ld_stream(&T2[qc]);
      };
      const int64_t p0 = (int64_t)blockIdx.x * QTPB;
      if (p0 < np) {   // uniform per block; below it every clamped index is a valid pair
#pragma unroll
        for (int u = 0; u < HU; ++u) load(p0 + threadIdx.x + u * stride, xa[u], ya[u], ta[u]);
      }
      for (int64_t pb = p0; pb < np; pb += HU * stride) {
        const int64_t p = pb + threadIdx.x, pn = p + HU * stride;
        lv2 xb[HU], yb[HU], tb[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) load(pn + u * stride, xb[u], yb[u], tb[u]);
#pragma unroll
        for (int u = 0; u < HU; ++u) {
          const int64_t q = p + u * stride;
          if (q < np) {
            one(2 * q, xa[u].x, ya[u].x, ta[u].x);
            one(2 * q + 1, xa[u].y, ya[u].y, ta[u].y);
          }
          xa[u] = xb[u]; ya[u] = yb[u]; ta[u] = tb[u];
        }
      }
    }
    if ((a.sel.n & 1) && blockIdx.x == 0 && threadIdx.x == 0 && (SEL != SEL_MASK || mask_bit(a.sel.mask, a.sel.n - 1)))
      row(a.sel.n - 1);
  } else {
    // whole blocks of entries, so the waves of the atomic form reach wave_size_add together
    for (int64_t ub = (int64_t)blockIdx.x * QTPB; ub < a.sel.units; ub += stride) {
      const int64_t u = ub + threadIdx.x;
      int rb = -1;
      if (u < a.sel.units) {
        int64_t r;
        const int k = sel_row<SEL>(a.sel, u, r);
        if (k > 0) rb = row(r); else if (k < 0) ++bad;
      }
      if (!LDS) wave_size_add(size, rb);
    }
  }
  if (skip) atomicAdd(&s_tally[0], (unsigned long long)skip);
  if (out) atomicAdd(&s_tally[1], (unsigned long long)out);
  if (bad) atomicAdd(&s_tally[2], (unsigned long long)bad);
  __syncthreads();
  if (LDS) {
    // a bin's size: the sum of its hash row 0 (every added row incremented exactly one of its counters)
    for (int i = threadIdx.x; i < a.row_n * a.width; i += QTPB) {
      const int b = i / a.width;
      const uint32_t v = cnt[b * a.cells + (i - b * a.width)];
      if (v) atomicAdd(&cnt[b * a.cells + dw], v);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += QTPB) {
      const uint32_t v = cnt[i];
      if (!v) continue;
      const int b = i / a.cells, c = i - b * a.cells;
      if (c == dw) atomicAdd(&size[a.row_lo + b], (unsigned long long)v);
      else atomicAdd(&table[(int64_t)(a.row_lo + b) * dw + c], (unsigned long long)v);
    }
  }
  if (threadIdx.x == 0 && a.first) {
    if (s_tally[0]) atomicAdd(&tally[0], s_tally[0]);
    if (s_tally[1]) atomicAdd(&tally[1], s_tally[1]);
    if (s_tally[2]) atomicAdd(&tally[2], s_tally[2]);
  }
}

// CountMinSketch.estimateCount (CountMinSketch.scala:96-105) of one key per lane: in bins[i]'s sketch (0 for a
// bin outside the window), or summed over the window's sketches (Frequency.count(value), Frequency.scala:78)
__global__ __launch_bounds__(256) void k_cms_estimate(FreqArgs a, const int64_t* __restrict__ table,
                                                      const int64_t* __restrict__ keys,
                                                      const int16_t* __restrict__ bins, int64_t n,
                                                      int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t key = keys[i];
  const int dw = a.cells - 1;
  auto estimate = [&](int rb) {
    const int64_t* c = table + (int64_t)rb * dw;
    int64_t m = INT64_MAX;
    for (int k = 0; k < a.depth; ++k) {
      const int64_t v = c[k * a.width + cms_bucket(a.hash_a[k], key, a.width)];
      m = v < m ? v : m;
    }
    return m;
  };
  if (bins) {
    const int rb = (int)bins[i] - a.bin_lo;
    out[i] = (unsigned)rb < (unsigned)a.n_bins ? estimate(rb) : 0;
  } else {
    uint64_t sum = 0;
    for (int rb = 0; rb < a.n_bins; ++rb) sum += (uint64_t)estimate(rb);
    out[i] = (int64_t)sum;
  }
}

inline int freq_fail(const char* who, const char* why) {
  set_error(std::string(who) + ": " + why);
  return GM_E_INVALID;
}

// time bins one LDS pass holds (0: one bin's counters do not fit)
inline int freq_bins_per_pass(const gm_cms* c) {
  return (int)((int64_t)FREQ_LDS_INTS / ((int64_t)c->depth * c->width + 1));
}

// the sketch description's own errors; null: none
inline const char* cms_check(const gm_cms* c) {
  if (c->depth < 1 || c->depth > GM_CMS_MAX_DEPTH) return "depth must be within 1..GM_CMS_MAX_DEPTH";
  if (c->width < 1) return "width must be at least 1";
  if (c->n_bins < 1) return "n_bins must be at least 1";
  if (c->bin_lo < -32768 || (int64_t)c->bin_lo + c->n_bins > 32768) return "the window leaves the Short range";
  if ((int64_t)c->n_bins * c->depth * c->width > 2147483647LL) return "n_bins * depth * width exceeds 2^31 - 1";
  return nullptr;
}

// every GM_E_INVALID of the three scans that does not depend on the source
int freq_check(const char* who, gm_ctx* ctx, int64_t n, const uint64_t* mask, const int64_t* ids, int64_t n_ids,
               int period, const gm_cms* c, const int64_t* table, const int64_t* size, const int64_t* tally) {
  if (!ctx) return freq_fail(who, "NULL context");
  if (!c) return freq_fail(who, "NULL sketch description");
  if (!table || !size || !tally) return freq_fail(who, "NULL table, size or tally");
  if (n < 0) return freq_fail(who, "negative row count");
  if (!valid_period(period)) return freq_fail(who, "unknown period");
  if (const char* why = cms_check(c)) return freq_fail(who, why);
  if (const char* why = sel_check(mask, ids, n_ids)) return freq_fail(who, why);
  if (c->path < 0 || c->path > 2) return freq_fail(who, "path must be 0, 1 or 2");
  if (c->path == 1 && freq_bins_per_pass(c) < 1)
    return freq_fail(who, "path 1: one time bin's counters do not fit workgroup-private counters");
  if (c->workgroups < 0) return freq_fail(who, "negative workgroups");
  if (!aligned_to<8>(table) || !aligned_to<8>(size) || !aligned_to<8>(tally))
    return freq_fail(who, "columns and outputs need 8-B alignment");
  return GM_OK;
}

void freq_args(FreqArgs& a, RowSel rows, int period, int prec, int64_t zmask, const gm_cms* c) {
  a.sel = rows;
  a.depth = c->depth;
  a.width = c->width;
  a.cells = c->depth * c->width + 1;
  a.bin_lo = c->bin_lo;
  a.n_bins = c->n_bins;
  a.row_lo = 0;
  a.row_n = c->n_bins;
  a.first = 1;
  a.period = period;
  a.prec = prec;
  a.zmask = zmask;
  a.lon = lon_dim(21);
  a.lat = lat_dim(21);
  a.tim = time_dim(period, 21);
  for (int i = 0; i < GM_CMS_MAX_DEPTH; ++i) a.hash_a[i] = i < c->depth ? c->hash_a[i] : 0;
}

// Frequency.getMask (Frequency.scala:284-287): Long.MaxValue << (64 - precision), the count taken mod 64
inline int64_t freq_mask(int precision) {
  return (int64_t)((uint64_t)INT64_MAX << ((64 - precision) & 63));
}

int launch_freq(gm_ctx* ctx, int key, FreqSrc s, FreqArgs a, const gm_cms* c, int64_t* table, int64_t* size,
                int64_t* tally) {
  const int sel = sel_of(a.sel);
  const int64_t units = a.sel.units;
  const int fit = freq_bins_per_pass(c);
  const int passes = fit > 0 ? (a.n_bins + fit - 1) / fit : 0;
  const bool lds = c->path == 1 || (c->path == 0 && fit > 0 && passes <= FREQ_MAX_PASSES);
  const bool eight = key != K_I32 && key != K_F32;   // 4-byte columns take the scalar-load kernels
  const bool xy = key == K_Z3 || key == K_Z2;
  const bool vec = lds && eight && sel != SEL_IDS && aligned16(s.t) &&
                   (xy ? aligned16(s.x) && aligned16(s.y) : aligned16(s.v));
  int cus = 256;
  GM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int rows = lds ? fit : a.n_bins;
  for (int k = 0; k * rows < a.n_bins; ++k) {
    a.row_lo = k * rows;
    a.row_n = std::min(rows, a.n_bins - a.row_lo);
    a.first = k == 0;
    const size_t bytes = ((lds ? (size_t)a.row_n * a.cells : 0) + (key == K_Z3 ? 2048 : 0)) * sizeof(uint32_t);
    const int per_cu = bytes <= 72 * 1024 ? 2 : 1;   // 2 x 1024 threads is the CU's wave limit
    // a workgroup sees fewer than 2^31 entries, each at most one increment of a counter: no uint32 wraps
    const int64_t need = units / 2147483647LL + 1;
    int64_t wgs = std::min<int64_t>((int64_t)cus * per_cu, std::max<int64_t>((units + QTPB - 1) / QTPB, 1));
    if (c->workgroups > 0) wgs = c->workgroups;
    wgs = std::max(wgs, need);
    auto go = [&](auto kern) -> int {
      GM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
      hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(QTPB), bytes, ctx->stream, s, a, (unsigned long long*)table,
                         (unsigned long long*)size, (unsigned long long*)tally);
      GM_CHECK_LAUNCH();
      return GM_OK;
    };
    // the switches that exist for a source: the period for Z3 keys, vector loads for 8-byte columns in LDS
    const int rc = with_value<K_Z3, K_Z2, K_I32, K_I64, K_F32, K_F64>(key, [&](auto K) {
      return with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) {
        return with_flags([&](auto L, auto V) {
          constexpr bool v = V() && L() && E() != SEL_IDS && K() != K_I32 && K() != K_F32;
          if constexpr (K() == K_Z3)
            return with_period(a.period, [&](auto P) { return go(k_freq<K_Z3, P(), E(), L(), v>); });
          else
            return go(k_freq<K(), -1, E(), L(), v>);
        }, lds, vec);
      });
    });
    if (rc) return rc;
  }
  return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_z3_frequency(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n,
                    const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                    const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally) {
  const char* who = "gm_z3_frequency";
  const int rc = freq_check(who, ctx, n, mask, ids, n_ids, period, cms, table, size, tally);
  if (rc) return rc;
  if (precision < 0 || precision > 64) return freq_fail(who, "precision must be within 0..64");
  if (n == 0 && !ids) return GM_OK;
  if (n > 0 && (!x || !y || !t_ms || !aligned_to<8>(x) || !aligned_to<8>(y) || !aligned_to<8>(t_ms)))
    return freq_fail(who, "x, y and t_ms must be given, 8-B aligned");
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  FreqSrc s{x, y, t_ms, nullptr, 0, nullptr, nullptr, 0};
  FreqArgs a;
  freq_args(a, row_sel(n, mask, ids, n_ids), period, 1, freq_mask(precision), cms);
  return launch_freq(ctx, K_Z3, s, a, cms, table, size, tally);
}

int gm_frequency_points(gm_ctx* ctx, const double* x, const double* y, const gm_time_column* dtg, int64_t n,
                        const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                        const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally) {
  const char* who = "gm_frequency_points";
  const int rc = freq_check(who, ctx, n, mask, ids, n_ids, period, cms, table, size, tally);
  if (rc) return rc;
  if (precision < 0 || precision > 64) return freq_fail(who, "precision must be within 0..64");
  if (n == 0 && !ids) return GM_OK;
  if (n > 0 && (!x || !y || !aligned_to<8>(x) || !aligned_to<8>(y)))
    return freq_fail(who, "x and y must be given, 8-B aligned");
  if (n > 0 && dtg && (!dtg->millis || !aligned_to<8>(dtg->millis)))
    return freq_fail(who, "dtg needs its millis, 8-B aligned");
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  FreqSrc s{x, y, nullptr, nullptr, 0, nullptr, nullptr, 0};
  if (n > 0 && dtg) { s.t = dtg->millis; s.t_valid = dtg->validity; s.t_voff = dtg->validity_offset; }
  FreqArgs a;
  freq_args(a, row_sel(n, mask, ids, n_ids), period, 1, freq_mask(precision), cms);
  a.lon = lon_dim(31);   // Z2SFC (z3/curve/Z2SFC.scala): 31 bits per dimension
  a.lat = lat_dim(31);
  return launch_freq(ctx, K_Z2, s, a, cms, table, size, tally);
}

int gm_frequency_attr(gm_ctx* ctx, const gm_attr_column* col, const gm_time_column* dtg, int64_t n,
                      const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                      const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally) {
  const char* who = "gm_frequency_attr";
  const int rc = freq_check(who, ctx, n, mask, ids, n_ids, period, cms, table, size, tally);
  if (rc) return rc;
  if (!col) return freq_fail(who, "NULL attribute column");
  int key;
  switch (col->type) {
    case GM_ATTR_INT32: key = K_I32; break;
    case GM_ATTR_INT64: key = K_I64; break;
    case GM_ATTR_FLOAT32: key = K_F32; break;
    case GM_ATTR_FLOAT64: key = K_F64; break;
    case GM_ATTR_UTF8:
      return freq_fail(who, "GM_ATTR_UTF8: a string key hashes through MurmurHash, which is not restated");
    default: return freq_fail(who, "unknown attribute type");
  }
  if ((key == K_I32 || key == K_I64) && precision < 1)
    return freq_fail(who, "an integer column needs precision >= 1");
  if (n == 0 && !ids) return GM_OK;
  const bool eight = key == K_I64 || key == K_F64;
  if (n > 0 && (!col->values || (eight ? !aligned_to<8>(col->values) : !aligned_to<4>(col->values))))
    return freq_fail(who, "the column needs its values, naturally aligned");
  if (n > 0 && dtg && (!dtg->millis || !aligned_to<8>(dtg->millis)))
    return freq_fail(who, "dtg needs its millis, 8-B aligned");
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  FreqSrc s{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0};
  if (n > 0) {
    s.v = col->values; s.v_valid = col->validity; s.v_voff = col->validity_offset;
    if (dtg) { s.t = dtg->millis; s.t_valid = dtg->validity; s.t_voff = dtg->validity_offset; }
  }
  FreqArgs a;
  freq_args(a, row_sel(n, mask, ids, n_ids), period, precision, 0, cms);
  return launch_freq(ctx, key, s, a, cms, table, size, tally);
}

int gm_cms_estimate(gm_ctx* ctx, const gm_cms* cms, const int64_t* table, const int64_t* keys, const int16_t* bins,
                    int64_t n, int64_t* out) {
  const char* who = "gm_cms_estimate";
  if (!ctx) return freq_fail(who, "NULL context");
  if (!cms || !table) return freq_fail(who, "NULL sketch description or table");
  if (n < 0) return freq_fail(who, "negative key count");
  if (const char* why = cms_check(cms)) return freq_fail(who, why);
  if (n == 0) return GM_OK;
  if (!keys || !out) return freq_fail(who, "NULL keys or output");
  if (!aligned_to<8>(table) || !aligned_to<8>(keys) || !aligned_to<8>(out) || !aligned_to<2>(bins))
    return freq_fail(who, "misaligned pointer");
  GM_HIP(hipSetDevice(ctx->device));
  FreqArgs a;
  freq_args(a, row_sel(0, nullptr, nullptr, 0), WEEK, 1, 0, cms);
  hipLaunchKernelGGL(k_cms_estimate, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, a, table, keys, bins, n, out);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

}  // extern "C"
