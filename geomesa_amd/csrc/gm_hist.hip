// gm_hist.hip -- Histogram.observe / unobserve and MinMax.observe over an attribute column on gfx950.
//
// Reference: Histogram (utils/stats/Histogram.scala:74-106, 226-232, 260-292) over BinnedArray
// (utils/stats/BinnedArray.scala:185-201, 284-350), MinMax (utils/stats/MinMax.scala:51-62) with
// HyperLogLog(10) (utils/clearspring/HyperLogLog.scala:99-131).  The arithmetic is stated in
// include/geomesa_hip.h; its host half (copyInto, expandBins, +=) is gm_hist_host.hpp.
//
// MinMax is a reduction: one grid-stride pass, min and max as order keys in registers, reduced per wave by
// shuffles and once per workgroup through LDS (one device atomicMin / atomicMax per workgroup); the HyperLogLog
// registers as a 4 KB LDS image under atomicMax, flushed with one device atomicMax per nonzero register.
//
// Histogram depends on the order of the rows: a value outside the bounds re-bins every count so far.  The rows
// that do so are the records of the prefix extrema.  Per round of at most HIST_MAX_SEGMENTS records:
//   pass R  k_hist_ext: the extrema of each block of FROWS units (non-null, non-NaN); k_hist_prefix: one
//           workgroup's exclusive prefix over them, seeded with the bounds; k_hist_flag: the in-block prefix
//           (wave shuffles, then the block's waves) and the record bit of every unit, written as the mask
//           words and block counts of a filter scan, so finish_scan compacts the records' units in order and
//           reads their number back; k_hist_gather fetches their values.
//   pass C  k_hist_count: segment s = the units from record s to record s + 1, binned under the running
//           bounds after record s.  Persistent workgroups walk contiguous runs of tiles; a tile inside one
//           segment counts into the workgroup's LDS image of that segment (flushed by 64-bit device atomics
//           when the segment changes and at the end), a tile that holds a record finds each unit's segment by
//           upper-bound search of the staged record list and adds by device atomics.
//   replay  no record: segment 0 is added into counts on the device.  Else counts and the segment rows come
//           back, and per record the host runs expandBins and adds that segment's row.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "gm_arrow.hpp"
#include "gm_hist_host.hpp"
#include "gm_scan.hpp"

namespace gm {

constexpr int HIST_MAX_SEGMENTS = GM_HIST_MAX_SEGMENTS;
constexpr int HIST_LDS_BINS = GM_HIST_LDS_BINS;   // 64 KB of uint32: two workgroups a CU
constexpr int HLL_REGS = 1024;

enum : int { B_I32 = 0, B_I64 = 1, B_F32 = 2, B_F64 = 3 };

template <int B>
using ValT = std::conditional_t<B == B_F32, float, std::conditional_t<B == B_F64, double, int64_t>>;

struct HistSrc {
  const void* v;
  const uint8_t* valid;
  int64_t voff;
};

template <int B> __device__ __forceinline__ ValT<B> min_id() {
  if constexpr (B == B_F32 || B == B_F64) return (ValT<B>)__builtin_huge_val(); else return INT64_MAX;
}
template <int B> __device__ __forceinline__ ValT<B> max_id() {
  if constexpr (B == B_F32 || B == B_F64) return (ValT<B>)-__builtin_huge_val(); else return INT64_MIN;
}
// a value in an 8-byte slot: a whole number as itself, a float widened to double (exact), as hist::Val
template <int B> __device__ __forceinline__ int64_t to_slot(ValT<B> v) {
  if constexpr (B == B_F32 || B == B_F64) return __double_as_longlong((double)v); else return v;
}
template <int B> __device__ __forceinline__ ValT<B> from_slot(int64_t s) {
  if constexpr (B == B_F32 || B == B_F64) return (ValT<B>)__longlong_as_double(s); else return s;
}
template <class V> __device__ __forceinline__ V shfl_up_v(V v, int d) {
  if constexpr (std::is_same<V, int64_t>::value) return (int64_t)__shfl_up((long long)v, d, 64);
  else return __shfl_up(v, d, 64);
}
template <class V> __device__ __forceinline__ V shfl_xor_v(V v, int d) {
  if constexpr (std::is_same<V, int64_t>::value) return (int64_t)__shfl_xor((long long)v, d, 64);
  else return __shfl_xor(v, d, 64);
}
template <class V> __device__ __forceinline__ V vmin(V a, V b) { return b < a ? b : a; }
template <class V> __device__ __forceinline__ V vmax(V a, V b) { return b > a ? b : a; }

// unit u of the selection -> its value.  1: a non-null value; 0: not selected or null; -1: an id outside [0, n)
template <int B, int SEL>
__device__ __forceinline__ int unit_value(const HistSrc& s, const RowSel& sel, int64_t u, ValT<B>& v) {
  int64_t r;
  const int k = sel_row<SEL>(sel, u, r);
  if (k <= 0) return k;
  if (!arrow_valid(s.valid, s.voff, r)) return 0;
  if constexpr (B == B_I32) v = ((const int32_t*)s.v)[r];
  else if constexpr (B == B_I64) v = ((const int64_t*)s.v)[r];
  else if constexpr (B == B_F32) v = ((const float*)s.v)[r];
  else v = ((const double*)s.v)[r];
  return 1;
}

// indexOf (BinnedArray.scala:195-201, :293-299, :327-333); bs: the binning's binSize (a float's widened)
template <int B>
__device__ __forceinline__ int hist_index(ValT<B> v, ValT<B> lo, ValT<B> hi, double bs, int length) {
  if (v < lo || v > hi) return -1;
  double q;
  if constexpr (B == B_F32) q = (double)((v - lo) / (float)bs);   // the float32 quotient, correctly rounded
  else if constexpr (B == B_F64) q = (v - lo) / bs;
  else q = (double)(int64_t)((uint64_t)v - (uint64_t)lo) / bs;
  const int i = jvm_d2i(floor(q));
  return (i < 0 || i > length) ? -1 : (i == length ? length - 1 : i);
}

// The block's prefix extrema in thread order: (mn, mx) in, the extrema of everything before this thread
// (the running pair included) out; the running pair then takes the whole block.  FTPB threads, two barriers.
template <int B>
__device__ __forceinline__ void block_prefix_ext(ValT<B> mn, ValT<B> mx, ValT<B>& run_mn, ValT<B>& run_mx,
                                                 ValT<B>& before_mn, ValT<B>& before_mx) {
  using V = ValT<B>;
  __shared__ int64_t s_mn[FTPB / 64], s_mx[FTPB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  V imn = mn, imx = mx;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const V a = shfl_up_v(imn, off), b = shfl_up_v(imx, off);
    if (lane >= off) { imn = vmin(imn, a); imx = vmax(imx, b); }
  }
  V emn = shfl_up_v(imn, 1), emx = shfl_up_v(imx, 1);
  if (lane == 0) { emn = min_id<B>(); emx = max_id<B>(); }
  if (lane == 63) { s_mn[w] = to_slot<B>(imn); s_mx[w] = to_slot<B>(imx); }
  __syncthreads();
  before_mn = vmin(run_mn, emn);
  before_mx = vmax(run_mx, emx);
#pragma unroll
  for (int i = 0; i < FTPB / 64; ++i) {
    const V a = from_slot<B>(s_mn[i]), b = from_slot<B>(s_mx[i]);
    if (i < w) { before_mn = vmin(before_mn, a); before_mx = vmax(before_mx, b); }
    run_mn = vmin(run_mn, a);
    run_mx = vmax(run_mx, b);
  }
  __syncthreads();
}

// pass R, 1: the extrema of block b's units [u0 + b * FROWS, ...) -> bmin[b], bmax[b] (slots)
template <int B, int SEL>
__global__ __launch_bounds__(FTPB) void k_hist_ext(HistSrc s, RowSel sel, int64_t u0, int64_t m,
                                                   int64_t* __restrict__ bmin, int64_t* __restrict__ bmax) {
  using V = ValT<B>;
  __shared__ int64_t s_mn[FTPB / 64], s_mx[FTPB / 64];
  const int64_t base = (int64_t)blockIdx.x * FROWS;
  V mn = min_id<B>(), mx = max_id<B>();
#pragma unroll 4
  for (int u = 0; u < FELEMS; ++u) {
    const int64_t i = base + (int64_t)u * FTPB + threadIdx.x;
    V v;
    if (i < m && unit_value<B, SEL>(s, sel, u0 + i, v) == 1 && v == v) { mn = vmin(mn, v); mx = vmax(mx, v); }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = vmin(mn, shfl_xor_v(mn, off));
    mx = vmax(mx, shfl_xor_v(mx, off));
  }
  if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = to_slot<B>(mn); s_mx[threadIdx.x >> 6] = to_slot<B>(mx); }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < FTPB / 64; ++i) { mn = vmin(mn, from_slot<B>(s_mn[i])); mx = vmax(mx, from_slot<B>(s_mx[i])); }
    bmin[blockIdx.x] = to_slot<B>(mn);
    bmax[blockIdx.x] = to_slot<B>(mx);
  }
}

// pass R, 2: in place, the exclusive prefix of the block extrema seeded with the bounds; one workgroup
template <int B>
__global__ __launch_bounds__(FTPB) void k_hist_prefix(int64_t* __restrict__ bmin, int64_t* __restrict__ bmax, int64_t nb,
                                                      int64_t lo, int64_t hi) {
  using V = ValT<B>;
  V run_mn = from_slot<B>(lo), run_mx = from_slot<B>(hi);
  for (int64_t c0 = 0; c0 < nb; c0 += FTPB) {
    const int64_t j = c0 + threadIdx.x;
    const V a = j < nb ? from_slot<B>(bmin[j]) : min_id<B>(), b = j < nb ? from_slot<B>(bmax[j]) : max_id<B>();
    V pmn, pmx;
    block_prefix_ext<B>(a, b, run_mn, run_mx, pmn, pmx);
    if (j < nb) { bmin[j] = to_slot<B>(pmn); bmax[j] = to_slot<B>(pmx); }
  }
}

// pass R, 3: the record bit of every unit, as the mask words and block counts of row_scan.  A unit is a
// record when indexOf under the extrema of everything before it is -1: the primitive comparison, and for a
// Long span that has wrapped the binning itself.
template <int B, int SEL>
__global__ __launch_bounds__(FTPB) void k_hist_flag(HistSrc s, RowSel sel, int64_t u0, int64_t m, int length,
                                                    const int64_t* __restrict__ pmin, const int64_t* __restrict__ pmax,
                                                    uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  using V = ValT<B>;
  const int64_t base = (int64_t)blockIdx.x * FROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  V run_mn = from_slot<B>(pmin[blockIdx.x]), run_mx = from_slot<B>(pmax[blockIdx.x]);
  int cnt = 0;
  for (int u = 0; u < FELEMS; ++u) {
    const int64_t i = base + (int64_t)u * FTPB + threadIdx.x;
    V v = 0;
    const bool ok = i < m && unit_value<B, SEL>(s, sel, u0 + i, v) == 1 && v == v;
    V bmn, bmx;
    block_prefix_ext<B>(ok ? v : min_id<B>(), ok ? v : max_id<B>(), run_mn, run_mx, bmn, bmx);
    bool rec = ok && (v < bmn || v > bmx);
    if constexpr (B == B_I64) {
      const int64_t span = (int64_t)((uint64_t)bmx - (uint64_t)bmn);
      if (ok && !rec && span < 0) rec = hist_index<B>(v, bmn, bmx, (double)span / length, length) < 0;
    }
    const uint64_t w = __ballot(rec);
    if (lane == 0) {
      const int64_t word = (base + (int64_t)u * FTPB + wave * 64) >> 6;
      if ((word << 6) < m) mask[word] = w;
      cnt += __popcll(w);
    }
  }
  block_count_waves(cnt, block_counts);   // reads lane 0's
}

// the values of the k compacted records (units relative to u0) -> slots
template <int B, int SEL>
__global__ __launch_bounds__(FTPB) void k_hist_gather(HistSrc s, RowSel sel, int64_t u0, const int64_t* __restrict__ units,
                                                      int k, int64_t* __restrict__ out) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  if (i >= k) return;
  ValT<B> v = 0;
  unit_value<B, SEL>(s, sel, u0 + units[i], v);
  out[i] = to_slot<B>(v);
}

// the staged segment table of pass C: nseg starts (units relative to u0; start[0] = 0), then per segment the
// bounds as slots and the binSize
struct SegTab {
  const int64_t* start;
  const int64_t* lo;
  const int64_t* hi;
  const double* bs;
  int nseg;
};

// pass C.  seg_counts[nseg][length + 2]: the bins, then the segment's observed rows and its ids out of range.
template <int B, int SEL, bool LDS>
__global__ __launch_bounds__(FTPB) void k_hist_count(HistSrc s, RowSel sel, int64_t u0, int64_t end, int length,
                                                     SegTab t, int64_t tiles_per, long long sign,
                                                     unsigned long long* __restrict__ seg_counts) {
  using V = ValT<B>;
  extern __shared__ uint32_t hist_cnt[];   // LDS: length + 2
  __shared__ int64_t s_start[HIST_MAX_SEGMENTS + 1], s_lo[HIST_MAX_SEGMENTS + 1], s_hi[HIST_MAX_SEGMENTS + 1];
  __shared__ double s_bs[HIST_MAX_SEGMENTS + 1];
  const int row = length + 2;
  for (int i = threadIdx.x; i < t.nseg; i += FTPB) {
    s_start[i] = t.start[i]; s_lo[i] = t.lo[i]; s_hi[i] = t.hi[i]; s_bs[i] = t.bs[i];
  }
  if (LDS) for (int i = threadIdx.x; i < row; i += FTPB) hist_cnt[i] = 0u;
  __syncthreads();
  auto seg_of = [&](int64_t i) {   // upper bound of i in the starts, minus one
    int lo = 0, hi = t.nseg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_start[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
  };
  auto flush = [&](int seg) {      // between barriers
    unsigned long long* dst = seg_counts + (int64_t)seg * row;
    for (int i = threadIdx.x; i < row; i += FTPB) {
      const uint32_t c = hist_cnt[i];
      if (!c) continue;
      atomicAdd(&dst[i], i < length ? (unsigned long long)(sign * (long long)c) : (unsigned long long)c);
      hist_cnt[i] = 0u;
    }
  };
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (end + FROWS - 1) / FROWS;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per, t1 = t0 + tiles_per < tiles ? t0 + tiles_per : tiles;
  int cur = -1;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t base = tile * FROWS, last = (base + FROWS < end ? base + FROWS : end) - 1;
    const int sa = seg_of(base), sb = seg_of(last);
    const bool uniform = sa == sb;   // the same for every thread
    if (LDS && uniform && sa != cur) {
      __syncthreads();
      if (cur >= 0) flush(cur);
      cur = sa;
      __syncthreads();
    }
    for (int u = 0; u < FELEMS; ++u) {
      const int64_t i = base + (int64_t)u * FTPB + threadIdx.x;
      V v = 0;
      const int g = i < end ? unit_value<B, SEL>(s, sel, u0 + i, v) : 0;
      const int seg = uniform ? sa : (g != 0 ? seg_of(i) : 0);
      int bin = -1;
      if (g == 1) bin = hist_index<B>(v, from_slot<B>(s_lo[seg]), from_slot<B>(s_hi[seg]), s_bs[seg], length);
      if (uniform) {
        const uint64_t rows = __ballot(g == 1), bad = SEL == SEL_IDS ? __ballot(g < 0) : 0ull;
        if (LDS) {
          if (bin >= 0) atomicAdd(&hist_cnt[bin], 1u);
          if (lane == 0 && rows) atomicAdd(&hist_cnt[length], (uint32_t)__popcll(rows));
          if (lane == 0 && bad) atomicAdd(&hist_cnt[length + 1], (uint32_t)__popcll(bad));
        } else {
          unsigned long long* dst = seg_counts + (int64_t)sa * row;
          if (bin >= 0) atomicAdd(&dst[bin], (unsigned long long)sign);
          if (lane == 0 && rows) atomicAdd(&dst[length], (unsigned long long)__popcll(rows));
          if (lane == 0 && bad) atomicAdd(&dst[length + 1], (unsigned long long)__popcll(bad));
        }
      } else if (g != 0) {   // a tile that holds a record: few of them, every add a device atomic
        unsigned long long* dst = seg_counts + (int64_t)seg * row;
        if (bin >= 0) atomicAdd(&dst[bin], (unsigned long long)sign);
        atomicAdd(&dst[g == 1 ? length : length + 1], 1ull);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    if (cur >= 0) flush(cur);
  }
}

// no record: counts += segment 0, tally += its rows and bad ids
__global__ __launch_bounds__(FTPB) void k_hist_add_row(const int64_t* __restrict__ seg, int length,
                                                       int64_t* __restrict__ counts, int64_t* __restrict__ tally) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  if (i < length) counts[i] = (int64_t)((uint64_t)counts[i] + (uint64_t)seg[i]);
  if (i == 0) { tally[0] += seg[length]; tally[2] += seg[length + 1]; }
}
__global__ void k_tally_add(int64_t* __restrict__ tally, int64_t a, int64_t b, int64_t c) {
  tally[0] += a; tally[1] += b; tally[2] += c;
}

// ------------------------------------------------------------------ MinMax
// Double.compareTo's order as a signed key (hist::order_key): every NaN canonical first
__device__ __forceinline__ int64_t dev_order_key(double v) {
  const int64_t b = v == v ? __double_as_longlong(v) : 0x7ff8000000000000LL;
  return b ^ ((b >> 63) & INT64_MAX);
}
// MurmurHash.hashLong as include/geomesa_hip.h defines it (parity unpinned)
__device__ __forceinline__ uint32_t hash_long(int64_t key) {
  const uint32_t m = 0x5bd1e995u;
  uint32_t h = 0, k = (uint32_t)key * m;
  k ^= k >> 24;
  h ^= k * m;
  k = (uint32_t)((uint64_t)key >> 32) * m;
  k ^= k >> 24;
  h *= m;
  h ^= k * m;
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}

template <int B, int SEL, bool REG>
__global__ __launch_bounds__(FTPB) void k_minmax(HistSrc s, RowSel sel, long long* __restrict__ minmax,
                                                 int* __restrict__ registers, unsigned long long* __restrict__ tally) {
  using V = ValT<B>;
  __shared__ int s_reg[REG ? HLL_REGS : 1];
  __shared__ int64_t s_mn[FTPB / 64], s_mx[FTPB / 64];
  __shared__ unsigned s_rows, s_bad;
  if (REG) for (int i = threadIdx.x; i < HLL_REGS; i += FTPB) s_reg[i] = 0;
  if (threadIdx.x == 0) { s_rows = 0u; s_bad = 0u; }
  __syncthreads();
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  unsigned rows = 0, bad = 0;   // a workgroup sees fewer than 2^32 units (launch_minmax)
  const int64_t stride = (int64_t)gridDim.x * FTPB;
  for (int64_t u = (int64_t)blockIdx.x * FTPB + threadIdx.x; u < sel.units; u += stride) {
    V v;
    const int g = unit_value<B, SEL>(s, sel, u, v);
    bad += g < 0;
    if (g != 1) continue;
    ++rows;
    int64_t key, hk;
    if constexpr (B == B_F32) { key = dev_order_key((double)v); hk = (int64_t)__float_as_int(v); }
    else if constexpr (B == B_F64) { key = dev_order_key(v); hk = __double_as_longlong(v); }
    else { key = v; hk = v; }
    mn = key < mn ? key : mn;
    mx = key > mx ? key : mx;
    if (REG) {
      const uint32_t h = hash_long(hk);
      atomicMax(&s_reg[h >> 22], __clz((int)((h << 10) | 513u)) + 1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = vmin(mn, shfl_xor_v(mn, off));
    mx = vmax(mx, shfl_xor_v(mx, off));
  }
  if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
  if (rows) atomicAdd(&s_rows, rows);
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < FTPB / 64; ++i) { mn = vmin(mn, s_mn[i]); mx = vmax(mx, s_mx[i]); }
    if (s_rows) {
      atomicMin(&minmax[0], (long long)mn);
      atomicMax(&minmax[1], (long long)mx);
      atomicAdd(&tally[0], (unsigned long long)s_rows);
    }
    if (s_bad) atomicAdd(&tally[2], (unsigned long long)s_bad);
  }
  if (REG) {
    for (int i = threadIdx.x; i < HLL_REGS; i += FTPB) {
      const int r = s_reg[i];
      if (r) atomicMax(&registers[i], r);
    }
  }
}

// ------------------------------------------------------------------ host
inline int hist_fail(const char* who, const char* why) {
  set_error(std::string(who) + ": " + why);
  return GM_E_INVALID;
}

inline int binding_of(int type) {
  switch (type) {
    case GM_ATTR_INT32: return B_I32;
    case GM_ATTR_INT64: return B_I64;
    case GM_ATTR_FLOAT32: return B_F32;
    case GM_ATTR_FLOAT64: return B_F64;
    default: return -1;
  }
}

// what both scans check of their column and selection
int attr_check(const char* who, gm_ctx* ctx, const gm_attr_column* col, int64_t n, const uint64_t* mask,
               const int64_t* ids, int64_t n_ids) {
  if (!ctx) return hist_fail(who, "NULL context");
  if (!col) return hist_fail(who, "NULL attribute column");
  if (col->type == GM_ATTR_UTF8) return hist_fail(who, "GM_ATTR_UTF8: the String binding is not restated");
  const int b = binding_of(col->type);
  if (b < 0) return hist_fail(who, "unknown attribute type");
  if (n < 0) return hist_fail(who, "negative row count");
  if (const char* why = sel_check(mask, ids, n_ids)) return hist_fail(who, why);
  const bool eight = b == B_I64 || b == B_F64;
  if (n > 0 && (!col->values || (eight ? !aligned_to<8>(col->values) : !aligned_to<4>(col->values))))
    return hist_fail(who, "the column needs its values, naturally aligned");
  return GM_OK;
}

template <class F>
int with_binding_sel(int b, int sel, F&& f) {
  return with_value<B_I32, B_I64, B_F32, B_F64>(b, [&](auto Bv) {
    return with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) { return f(Bv, E); });
  });
}

inline hist::Val slot_val(int b, int64_t slot) {
  hist::Val v{0, 0.0};
  if (b == B_F32 || b == B_F64) memcpy(&v.f, &slot, 8); else v.i = slot;
  return v;
}
inline int64_t val_slot(int b, hist::Val v) {
  int64_t s = v.i;
  if (b == B_F32 || b == B_F64) memcpy(&s, &v.f, 8);
  return s;
}

// one round over the units [u0, units): at most HIST_MAX_SEGMENTS records.  *next: the first unit of the
// next round (units when the selection is consumed).
int hist_round(gm_ctx* ctx, int b, HistSrc src, RowSel sel, int64_t u0, int sign, bool lds, gm_hist_state* st,
               int64_t* counts, int64_t* tally, int64_t* next) {
  hipStream_t s = ctx->stream;
  const int64_t m = sel.units - u0;
  const int64_t nb = (m + FROWS - 1) / FROWS;
  const int seln = sel_of(sel), length = st->length, row = length + 2;
  DevTemps tmp(s);
  int64_t *bmin = nullptr, *bmax = nullptr, *rec = nullptr;
  int rc = tmp.alloc_async((size_t)nb * 8, &bmin);
  if (!rc) rc = tmp.alloc_async((size_t)nb * 8, &bmax);
  if (!rc) rc = tmp.alloc_async((size_t)(HIST_MAX_SEGMENTS + 1) * 16, &rec);   // units, then values
  if (rc) return rc;
  ScanBufs bufs;
  if ((rc = alloc_scan(ctx, m, nullptr, 0, bufs))) return rc;
  const int64_t lo_slot = val_slot(b, hist::Val{st->lo, st->flo}), hi_slot = val_slot(b, hist::Val{st->hi, st->fhi});
  // ---- pass R
  rc = with_binding_sel(b, seln, [&](auto Bv, auto E) -> int {
    constexpr int BB = decltype(Bv)::value, EE = decltype(E)::value;
    hipLaunchKernelGGL((k_hist_ext<BB, EE>), dim3((unsigned)nb), dim3(FTPB), 0, s, src, sel, u0, m, bmin, bmax);
    GM_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_hist_prefix<BB>), dim3(1), dim3(FTPB), 0, s, bmin, bmax, nb, lo_slot, hi_slot);
    GM_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_hist_flag<BB, EE>), dim3((unsigned)nb), dim3(FTPB), 0, s, src, sel, u0, m, length, bmin, bmax,
                       bufs.mask, bufs.counts);
    GM_CHECK_LAUNCH();
    return GM_OK;
  });
  if (rc) return rc;
  int64_t found = 0;
  const int64_t cap = HIST_MAX_SEGMENTS + 1;   // one more than a round replays: where the next round starts
  if ((rc = finish_scan(ctx, m, bufs, rec, cap, &found))) return rc;
  const int k = (int)std::min<int64_t>(found, cap);
  std::vector<int64_t> h_rec((size_t)2 * cap, 0);
  if (k > 0) {
    rc = with_binding_sel(b, seln, [&](auto Bv, auto E) -> int {
      hipLaunchKernelGGL((k_hist_gather<decltype(Bv)::value, decltype(E)::value>), dim3(grid_for(k, FTPB)), dim3(FTPB), 0,
                         s, src, sel, u0, rec, k, rec + cap);
      GM_CHECK_LAUNCH();
      return GM_OK;
    });
    if (!rc) rc = copy_d2h(ctx, h_rec.data(), rec, (size_t)2 * cap * 8);
    if (rc) return rc;
  }
  const int nrec = std::min(k, HIST_MAX_SEGMENTS);
  const int64_t end = k > HIST_MAX_SEGMENTS ? h_rec[HIST_MAX_SEGMENTS] : m;   // this round's units, relative
  // ---- the segment table: segment 0 under the incoming bounds, segment i after record i - 1
  const int nseg = nrec + 1;
  std::vector<int64_t> tab((size_t)4 * nseg);
  gm_hist_state run = *st;
  for (int i = 0; i < nseg; ++i) {
    if (i > 0) run = hist::expanded(run, slot_val(b, h_rec[cap + i - 1]));
    tab[i] = i > 0 ? h_rec[i - 1] : 0;
    tab[nseg + i] = val_slot(b, hist::Val{run.lo, run.flo});
    tab[2 * nseg + i] = val_slot(b, hist::Val{run.hi, run.fhi});
    const double bs = hist::bin_size(run);
    memcpy(&tab[3 * nseg + i], &bs, 8);
  }
  int64_t* d_tab = nullptr;
  unsigned long long* seg = nullptr;
  rc = tmp.alloc_async(tab.size() * 8, &d_tab);
  if (!rc) rc = tmp.alloc_async((size_t)nseg * row * 8, &seg);
  if (rc) return rc;
  GM_HIP(hipMemsetAsync(seg, 0, (size_t)nseg * row * 8, s));
  if ((rc = copy_h2d(ctx, d_tab, tab.data(), tab.size() * 8))) return rc;
  // ---- pass C
  int cus = 256;
  GM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int64_t tiles = (end + FROWS - 1) / FROWS;
  if (tiles > 0) {
    const int64_t want = std::min<int64_t>(tiles, (int64_t)cus * 2);
    const int64_t tiles_per = (tiles + want - 1) / want;   // below 2^20 tiles a workgroup: no uint32 counter wraps
    const int64_t wgs = (tiles + tiles_per - 1) / tiles_per;
    const SegTab t{d_tab, d_tab + nseg, d_tab + 2 * nseg, (const double*)(d_tab + 3 * nseg), nseg};
    const size_t bytes = lds ? (size_t)row * 4 : 0;
    rc = with_binding_sel(b, seln, [&](auto Bv, auto E) -> int {
      return with_flags([&](auto L) -> int {
        auto kern = k_hist_count<decltype(Bv)::value, decltype(E)::value, decltype(L)::value>;
        GM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(FTPB), bytes, s, src, sel, u0, end, length, t, tiles_per,
                           (long long)sign, seg);
        GM_CHECK_LAUNCH();
        return GM_OK;
      }, lds);
    });
    if (rc) return rc;
  }
  *next = u0 + end;
  // ---- replay
  if (nrec == 0) {
    hipLaunchKernelGGL(k_hist_add_row, dim3(grid_for(length, FTPB)), dim3(FTPB), 0, s, (const int64_t*)seg, length, counts,
                       tally);
    GM_CHECK_LAUNCH();
    return GM_OK;
  }
  std::vector<int64_t> h_counts((size_t)length), h_seg((size_t)nseg * row);
  if ((rc = copy_d2h(ctx, h_counts.data(), counts, (size_t)length * 8))) return rc;
  if ((rc = copy_d2h(ctx, h_seg.data(), seg, h_seg.size() * 8))) return rc;
  int64_t rows = 0, bad = 0, expansions = 0;
  auto add_row = [&](int i) {
    const int64_t* r = h_seg.data() + (size_t)i * row;
    for (int j = 0; j < length; ++j) h_counts[j] = hist::wadd(h_counts[j], r[j]);
    rows += r[length];
    bad += r[length + 1];
  };
  add_row(0);
  for (int i = 1; i < nseg; ++i) {
    const hist::Val v = slot_val(b, h_rec[cap + i - 1]);
    ++expansions;
    if (!hist::expand(*st, h_counts.data(), v)) {
      // the reference's expandBins threw: the feature is dropped and the bounds stay, so the later segments
      // were counted under bounds that never held; the next round starts behind this record
      ++rows;
      *next = u0 + h_rec[i - 1] + 1;
      break;
    }
    add_row(i);   // the record's own add(value) is the first unit of its segment
  }
  if ((rc = copy_h2d(ctx, counts, h_counts.data(), (size_t)length * 8))) return rc;
  hipLaunchKernelGGL(k_tally_add, dim3(1), dim3(1), 0, s, tally, rows, expansions, bad);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_minmax_attr(gm_ctx* ctx, const gm_attr_column* col, int64_t n, const uint64_t* mask, const int64_t* ids,
                   int64_t n_ids, int64_t* minmax, int32_t* registers, int64_t* tally) {
  const char* who = "gm_minmax_attr";
  const int rc = attr_check(who, ctx, col, n, mask, ids, n_ids);
  if (rc) return rc;
  if (!minmax || !tally) return hist_fail(who, "NULL minmax or tally");
  if (!aligned_to<8>(minmax) || !aligned_to<8>(tally) || !aligned_to<4>(registers))
    return hist_fail(who, "columns and outputs need 8-B alignment");
  const RowSel sel = row_sel(n, mask, ids, n_ids);
  if (sel.units == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  const HistSrc src{col->values, col->validity, col->validity_offset};
  int cus = 256;
  GM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  // a resident wave of workgroups, raised so that a workgroup sees fewer than 2^32 units
  int64_t wgs = std::min<int64_t>((int64_t)cus * 8, (sel.units + FTPB - 1) / FTPB);
  wgs = std::max<int64_t>(wgs, sel.units / 4294967295LL + 1);
  return with_binding_sel(binding_of(col->type), sel_of(sel), [&](auto Bv, auto E) -> int {
    return with_flags([&](auto R) -> int {
      hipLaunchKernelGGL((k_minmax<decltype(Bv)::value, decltype(E)::value, decltype(R)::value>), dim3((unsigned)wgs),
                         dim3(FTPB), 0, ctx->stream, src, sel, (long long*)minmax, (int*)registers,
                         (unsigned long long*)tally);
      GM_CHECK_LAUNCH();
      return GM_OK;
    }, registers != nullptr);
  });
}

int gm_histogram_attr(gm_ctx* ctx, const gm_attr_column* col, int64_t n, const uint64_t* mask, const int64_t* ids,
                      int64_t n_ids, int sign, int path, gm_hist_state* state, int64_t* counts, int64_t* tally) {
  const char* who = "gm_histogram_attr";
  int rc = attr_check(who, ctx, col, n, mask, ids, n_ids);
  if (rc) return rc;
  if (const char* why = hist::state_check(state)) return hist_fail(who, why);
  if (state->type != col->type) return hist_fail(who, "the column's type differs from the state's");
  if (!counts || !tally) return hist_fail(who, "NULL counts or tally");
  if (sign != 1 && sign != -1) return hist_fail(who, "sign must be +1 or -1");
  if (path < 0 || path > 2) return hist_fail(who, "path must be 0, 1 or 2");
  if (path == 1 && state->length > HIST_LDS_BINS)
    return hist_fail(who, "path 1: the histogram does not fit workgroup-private counters");
  if (!aligned_to<8>(counts) || !aligned_to<8>(tally)) return hist_fail(who, "columns and outputs need 8-B alignment");
  const RowSel sel = row_sel(n, mask, ids, n_ids);
  if (sel.units == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  const HistSrc src{col->values, col->validity, col->validity_offset};
  const bool lds = path == 1 || (path == 0 && state->length <= HIST_LDS_BINS);
  int64_t u0 = 0;
  while (u0 < sel.units) {
    int64_t next = sel.units;
    if ((rc = hist_round(ctx, binding_of(col->type), src, sel, u0, sign, lds, state, counts, tally, &next))) return rc;
    u0 = next;
  }
  return GM_OK;
}

static int host_state(const char* who, const gm_hist_state* s) {
  if (const char* why = hist::state_check(s)) return hist_fail(who, why);
  return GM_OK;
}

int gm_hist_index_of(const gm_hist_state* state, const void* values, int64_t n, int32_t* index) {
  const char* who = "gm_hist_index_of";
  if (int rc = host_state(who, state)) return rc;
  if (n < 0 || (n > 0 && (!values || !index))) return hist_fail(who, "NULL values or index");
  const double bs = hist::bin_size(*state);
  for (int64_t i = 0; i < n; ++i) {
    hist::Val v{0, 0.0};
    switch (state->type) {
      case GM_ATTR_INT32: v.i = ((const int32_t*)values)[i]; break;
      case GM_ATTR_INT64: v.i = ((const int64_t*)values)[i]; break;
      case GM_ATTR_FLOAT32: v.f = (double)((const float*)values)[i]; break;
      default: v.f = ((const double*)values)[i]; break;
    }
    index[i] = hist::index_of(*state, bs, v);
  }
  return GM_OK;
}

int gm_hist_bin_bounds(const gm_hist_state* state, int32_t i, gm_hist_state* out) {
  const char* who = "gm_hist_bin_bounds";
  if (int rc = host_state(who, state)) return rc;
  if (!out) return hist_fail(who, "NULL output");
  if (i < 0 || i > state->length) return hist_fail(who, "index out of range");
  hist::Val lo, hi;
  hist::bin_bounds(*state, hist::bin_size(*state), i, lo, hi);
  *out = gm_hist_state{state->type, state->length, lo.i, hi.i, lo.f, hi.f};
  return GM_OK;
}

int gm_hist_median(const gm_hist_state* state, int32_t i, int64_t* iv, double* fv) {
  const char* who = "gm_hist_median";
  if (int rc = host_state(who, state)) return rc;
  if (!iv || !fv) return hist_fail(who, "NULL output");
  if (i < 0 || i > state->length) return hist_fail(who, "index out of range");
  const hist::Val m = hist::median(*state, hist::bin_size(*state), i);
  *iv = m.i;
  *fv = m.f;
  return GM_OK;
}

int gm_hist_copy_into(const gm_hist_state* to, int64_t* to_counts, const gm_hist_state* from,
                      const int64_t* from_counts) {
  const char* who = "gm_hist_copy_into";
  if (int rc = host_state(who, to)) return rc;
  if (int rc = host_state(who, from)) return rc;
  if (!to_counts || !from_counts) return hist_fail(who, "NULL counts");
  if (to->type != from->type) return hist_fail(who, "the two histograms differ in type");
  if (!hist::copy_into(*to, to_counts, *from, from_counts)) return hist_fail(who, "Error calculating bounds");
  return GM_OK;
}

int gm_hist_merge(gm_hist_state* a, int64_t* a_counts, const gm_hist_state* b, const int64_t* b_counts) {
  const char* who = "gm_hist_merge";
  if (int rc = host_state(who, a)) return rc;
  if (int rc = host_state(who, b)) return rc;
  if (!a_counts || !b_counts) return hist_fail(who, "NULL counts");
  if (a->type != b->type) return hist_fail(who, "the two histograms differ in type");
  if (!hist::merge(*a, a_counts, *b, b_counts)) return hist_fail(who, "Error calculating bounds");
  return GM_OK;
}

}  // extern "C"
