// gm_ranges_z.hip -- batched ZN.zranges (Z2 / Z3) on gfx950: the walk kernel k_zranges, its workspace
// and the entry points gm_z3_ranges, gm_z2_ranges and gm_zranges.  The host batch driver is
// gm_ranges.hip; the XZ curves are gm_ranges_xz.hip.
//
// One 512-thread workgroup (RTPB) per query.  The Scala code walks a FIFO queue one node at a time
// (ZN.scala:193-218) and its maxRanges budget truncates at an exact FIFO position.  Here a whole tree
// level is processed in parallel and the FIFO semantics are reconstructed with prefix sums: after node i
// of a level the queue holds (K-i-1) level nodes + the queued children, so the budget fires at the
// first i with
//      nR + CC(i) + CO(i) + (K - i - 1) >= rangeStop          (ZN.scala:214)
// (CC/CO = inclusive counts of contained / overlapping children).  Nodes after i are bottomed out as
// overlapping ranges at their own level, queued children at theirs.
//
// Emitted ranges are tree nodes that never nest, so after the walk they are disjoint; a merge of the
// walk's sorted runs by rank (or an LDS bitonic sort) followed by a parallel adjacency merge
// reproduces the sort + merge of ZN.scala:221-241 exactly.
//
// Frontier and range lists live in per-query global workspaces (HBM is plentiful); the zbounds sit
// in LDS.
#include <algorithm>

#include "gm_ranges.hpp"

namespace gm {

constexpr int RNW = RTPB / 64;

// ------------------------------------------------------------------ block helpers

__device__ __forceinline__ int64_t block_exscan(int64_t v, int64_t* s_tmp, int64_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_tmp[w] = x;
  __syncthreads();
  int64_t pre = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < RNW; ++k) {
    const int64_t t = s_tmp[k];
    if (k < w) pre += t;
    tot += t;
  }
  __syncthreads();
  total = tot;
  return pre + x - v;
}

// Java `(1L << s) - 1` with the shift distance masked to 6 bits
__device__ __forceinline__ int64_t low_mask(int s) { return (int64_t)(((uint64_t)1 << (s & 63)) - 1u); }
__device__ __forceinline__ int64_t jshl(int64_t v, int s) { return (int64_t)((uint64_t)v << (s & 63)); }

template <int D>
__device__ __forceinline__ int32_t zdim(int64_t z, int d) {
  return D == 3 ? z3_combine(z >> d) : z2_combine(z >> d);
}

// Z3.contains / Z2.contains (Z3.scala:93-98, Z2.scala:80-83) on decoded dims
template <int D>
__device__ __forceinline__ bool z_contains(const int32_t* b, int64_t v) {
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int32_t x = zdim<D>(v, d);
    if (!(x >= b[d] && x <= b[D + d])) return false;
  }
  return true;
}

// bitonic sort of (key, idx) pairs, P a power of two, keys padded with INT64_MAX
template <class K, class I>
__device__ void bitonic(K* key, I* idx, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += RTPB) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool up = (i & k) == 0;
          const int64_t a = key[i], b = key[ixj];
          if ((a > b) == up) {
            key[i] = b; key[ixj] = a;
            const auto t = idx[i]; idx[i] = idx[ixj]; idx[ixj] = t;
          }
        }
      }
      __syncthreads();
    }
  }
}

constexpr int MAXRUNS = 64;   // sorted runs merged by rank; more fall back to the bitonic sort

// rank of `key` among run [lo, hi) of keys: elements < key (or <= key when `le`)
__device__ __forceinline__ int run_rank(const int64_t* keys, int lo, int hi, int64_t key, bool le) {
  int a = lo, b = hi;
  while (a < b) {
    const int m = (a + b) >> 1;
    const int64_t v = keys[m];
    if (v < key || (le && v == key)) a = m + 1;
    else b = m;
  }
  return a - lo;
}

// Sort the n ranges of this query by lower and merge adjacent ones into out (ZN.scala:221-241);
// returns the merged count (same on every thread).  The walk emits each tree level in curve order
// (children are generated in quadrant order from a curve-ordered frontier, and bottom-out appends
// ordered frontiers), so the list is a concatenation of a few ascending runs: they are merged by
// rank -- each range's sorted position is its offset in its run plus its rank in every other run,
// found by binary search (stable: ties rank after earlier runs) -- with one barrier.  A list with
// more than MAXRUNS runs takes the bitonic sort.
__device__ int sort_merge(const int64_t* rlo, const int64_t* rhi, const uint8_t* rc, int n, int64_t* gkey,
                          int32_t* gidx, gm_range* out, int64_t* s_key, int16_t* s_idx, int64_t* s_tmp) {
  __shared__ int s_run[MAXRUNS + 1];
  if (n == 0) return 0;
  const bool lds = n <= LDS_SORT;
  // run starts: rlo[j] < rlo[j - 1]
  if (threadIdx.x == 0) s_run[0] = 0;
  __syncthreads();
  int64_t nrun = 1;
  for (int c = 0; c < n && nrun <= MAXRUNS; c += RTPB) {
    const int j = c + threadIdx.x;
    const int f = (j > 0 && j < n && rlo[j] < rlo[j - 1]) ? 1 : 0;
    int64_t tot;
    const int64_t ex = block_exscan(f, s_tmp, tot);
    if (f && nrun + ex < MAXRUNS) s_run[nrun + ex] = j;
    nrun += tot;
    if (lds && j < n) s_key[j] = rlo[j];
  }
  __syncthreads();
  if (nrun <= MAXRUNS) {
    const int R = (int)nrun;
    if (threadIdx.x == 0) s_run[R] = n;
    __syncthreads();
    const int64_t* keys = lds ? s_key : rlo;
    for (int j = threadIdx.x; j < n; j += RTPB) {
      int r = 0;
      while (r + 1 < R && s_run[r + 1] <= j) ++r;   // R is small: linear scan
      const int64_t key = keys[j];
      int pos = j - s_run[r];
      for (int r2 = 0; r2 < R; ++r2)
        if (r2 != r) pos += run_rank(keys, s_run[r2], s_run[r2 + 1], key, r2 < r);
      if (lds) s_idx[pos] = (int16_t)j;
      else gidx[pos] = j;
    }
    __syncthreads();
  } else {
    int P = 1;
    while (P < n) P <<= 1;
    const bool lp = P <= LDS_SORT;
    for (int i = threadIdx.x; i < P; i += RTPB) {
      const int64_t k = i < n ? rlo[i] : INT64_MAX;
      if (lp) { s_key[i] = k; s_idx[i] = (int16_t)i; }
      else { gkey[i] = k; gidx[i] = i; }
    }
    __syncthreads();
    if (lp) bitonic(s_key, s_idx, P);
    else bitonic(gkey, gidx, P);
  }
  // run starts: lower > previous upper + 1 (Java long wrap); sorted disjoint ranges have increasing
  // uppers, so the previous upper is the merged run's max (ZN.scala:228-230)
  int64_t* run_of = lds ? s_key : gkey;  // keys are dead after the sort: reuse for run ids
  int64_t base = 0;
  for (int c = 0; c < n; c += RTPB) {
    const int j = c + threadIdx.x;
    int start = 0, src = 0;
    if (j < n) {
      src = lds ? (int)(uint16_t)s_idx[j] : gidx[j];
      if (j == 0) start = 1;
      else {
        const int prev = lds ? (int)(uint16_t)s_idx[j - 1] : gidx[j - 1];
        start = !(rlo[src] <= (int64_t)((uint64_t)rhi[prev] + 1u));
      }
    }
    int64_t tot;
    const int64_t ex = block_exscan(start, s_tmp, tot);
    if (j < n) {
      const int64_t run = base + ex + start - 1;
      run_of[j] = run;
      if (start) { out[run].lower = rlo[src]; out[run].contained = 1; out[run].reserved = 0; }
      bool last = (j == n - 1);
      if (!last) {
        const int nx = lds ? (int)(uint16_t)s_idx[j + 1] : gidx[j + 1];
        last = !(rlo[nx] <= (int64_t)((uint64_t)rhi[src] + 1u));
      }
      if (last) out[run].upper = rhi[src];
    }
    base += tot;
  }
  __syncthreads();
  // contained = AND over the run
  for (int j = threadIdx.x; j < n; j += RTPB) {
    const int src = lds ? (int)(uint16_t)s_idx[j] : gidx[j];
    if (!rc[src]) out[run_of[j]].contained = 0;
  }
  __syncthreads();
  const int total_runs = (int)base;
  return total_runs;
}

// record a query's result (every thread of the block calls it; `ws` = its m merged ranges)
__device__ void batch_finish(const BatchOut& bo, int64_t q, int m, int status, const gm_range* ws) {
  __shared__ unsigned long long s_base;
  if (threadIdx.x == 0) {
    s_base = (status == QS_OK && m > 0) ? atomicAdd(bo.total, (unsigned long long)m) : 0ull;
    batch_record(bo, q, (int64_t)s_base, m, status);
  }
  __syncthreads();
  if (status == QS_OK)
    for (int j = threadIdx.x; j < m; j += RTPB)
      if ((int64_t)s_base + j < bo.dcap) bo.dbuf[s_base + j] = ws[j];
}

// ------------------------------------------------------------------ Z ranges kernel

struct ZRangesArgs {
  const int32_t* box_off;   // [nq + 1]
  const double* xy;         // 4 per box
  const int32_t* time_off;  // [nq + 1] (Z3 only)
  const int64_t* t;         // 2 per interval
  const int32_t* zb_off;    // raw ZRange mode (gm_zranges): [nq + 1] bound offsets, else null
  const int64_t* zb;        //   (min, max) per bound
  int64_t q0;               // first query of this chunk
  NDim lon, lat, tim;
  int range_precision, range_stop, recurse_stop;
  int64_t fcap, rcap;
  int64_t* fa;              // frontier ping / pong, 2 x fcap per query
  int64_t* rlo;
  int64_t* rhi;
  uint8_t* rc;
  int64_t* gkey;
  int32_t* gidx;
  gm_range* out;            // merged ranges scratch, rcap per query
  BatchOut bo;
};

template <int D>
__global__ __launch_bounds__(RTPB) void k_zranges(ZRangesArgs a) {
  __shared__ int64_t s_zb[2 * MAXB];
  __shared__ int32_t s_dim[2 * D * MAXB];  // decoded min dims, max dims per bound
  __shared__ int64_t s_tmp[RNW];
  __shared__ int s_err, s_stop;
  __shared__ int64_t s_prefix;
  __shared__ int s_common;
  __shared__ int64_t s_key[LDS_SORT];
  __shared__ int16_t s_idx[LDS_SORT];

  const int64_t qc = blockIdx.x;            // query within the chunk
  const int64_t q = batch_query(a.bo, a.q0, qc);
  int64_t* F = a.fa + qc * 2 * a.fcap;      // F, G adjacent per query
  int64_t* G = F + a.fcap;
  int64_t* rlo = a.rlo + qc * a.rcap;
  int64_t* rhi = a.rhi + qc * a.rcap;
  uint8_t* rc = a.rc + qc * a.rcap;

  const bool raw = a.zb != nullptr;
  const int b0 = raw ? a.zb_off[q] : a.box_off[q];
  const int nbx = (raw ? a.zb_off[q + 1] : a.box_off[q + 1]) - b0;
  int t0 = 0, ntm = 1;
  if (D == 3 && !raw) { t0 = a.time_off[q]; ntm = a.time_off[q + 1] - t0; }
  const int nb = nbx * ntm;
  if (threadIdx.x == 0) s_err = (nb > MAXB) ? QS_TOO_MANY_BOUNDS : QS_OK;
  __syncthreads();
  if (s_err || nb <= 0) {
    batch_finish(a.bo, q, 0, s_err, nullptr);
    return;
  }
  // zbounds: Z3SFC.ranges builds ZRange(index(xmin, ymin, tmin), index(xmax, ymax, tmax)) for the
  // cross product xy x t, non-lenient (Z3SFC.scala:63-65); Z2SFC.ranges likewise (Z2SFC.scala:50)
  for (int j = threadIdx.x; j < nb; j += RTPB) {
    int64_t lo = 0, hi = 0;
    uint8_t st = ST_OK;
    if (raw) {   // ZN.zranges(Array[ZRange], ...) (ZN.scala:110-113): the bounds as given
      lo = a.zb[2 * (int64_t)(b0 + j)];
      hi = a.zb[2 * (int64_t)(b0 + j) + 1];
    } else if (D == 3) {
      const double* bx = a.xy + 4 * (int64_t)(b0 + j / ntm);
      const int64_t* tt = a.t + 2 * (int64_t)(t0 + j % ntm);
      auto idx = [&](double x, double y, int64_t tv, int64_t& z) -> uint8_t {
        const double td = (double)tv;
        if (!(x >= a.lon.min && x <= a.lon.max && y >= a.lat.min && y <= a.lat.max && td >= a.tim.min &&
              td <= a.tim.max))
          return ST_OUT_OF_BOUNDS;
        z = z3_apply(normalize(a.lon, x), normalize(a.lat, y), normalize(a.tim, td));
        return ST_OK;
      };
      st = idx(bx[0], bx[1], tt[0], lo);
      if (!st) st = idx(bx[2], bx[3], tt[1], hi);
    } else {
      const double* bx = a.xy + 4 * (int64_t)(b0 + j);
      auto idx = [&](double x, double y, int64_t& z) -> uint8_t {
        if (!(x >= a.lon.min && x <= a.lon.max && y >= a.lat.min && y <= a.lat.max)) return ST_OUT_OF_BOUNDS;
        z = z2_apply(normalize(a.lon, x), normalize(a.lat, y));
        return ST_OK;
      };
      st = idx(bx[0], bx[1], lo);
      if (!st) st = idx(bx[2], bx[3], hi);
    }
    if (!st && lo > hi) st = QS_UNORDERED;  // ZRange require(min <= max) (package.scala:24)
    if (st) atomicMax(&s_err, (int)st);
    s_zb[2 * j] = lo;
    s_zb[2 * j + 1] = hi;
    for (int d = 0; d < D; ++d) {
      s_dim[(2 * D) * j + d] = zdim<D>(lo, d);
      s_dim[(2 * D) * j + D + d] = zdim<D>(hi, d);
    }
  }
  __syncthreads();
  if (s_err) {
    batch_finish(a.bo, q, 0, s_err, nullptr);
    return;
  }
  // longestCommonPrefix (ZN.scala:272-281)
  if (threadIdx.x == 0) {
    const int total_bits = D == 3 ? 63 : 62;
    int shift = total_bits - D;
    int64_t head = (int64_t)((uint64_t)s_zb[0] >> (shift & 63));
    for (;;) {
      bool all = true;
      for (int i = 1; i < 2 * nb; ++i)
        if ((int64_t)((uint64_t)s_zb[i] >> (shift & 63)) != head) { all = false; break; }
      if (!(all && shift > -1)) break;
      shift -= D;
      head = (int64_t)((uint64_t)s_zb[0] >> (shift & 63));
    }
    shift += D;
    s_prefix = s_zb[0] & jshl(INT64_MAX, shift);
    s_common = 64 - shift;
  }
  __syncthreads();

  auto is_contained = [&](int64_t mn, int64_t mx) {
    for (int i = 0; i < nb; ++i)
      if (z_contains<D>(&s_dim[2 * D * i], mn) && z_contains<D>(&s_dim[2 * D * i], mx)) return true;
    return false;
  };
  auto is_overlapped = [&](int64_t mn, int64_t mx) {
    for (int i = 0; i < nb; ++i) {
      const int32_t* b = &s_dim[2 * D * i];
      bool ok = true;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int32_t v1 = zdim<D>(mn, d), v2 = zdim<D>(mx, d);
        const int32_t lo = b[d] > v1 ? b[d] : v1, hi = b[D + d] < v2 ? b[D + d] : v2;
        ok = ok && (lo <= hi);
      }
      if (ok) return true;
    }
    return false;
  };

  const int64_t range_stop = a.range_stop;
  int offset = 64 - s_common;
  int64_t nR = 0, K = 0;
  // initial level: checkValue(commonPrefix, 0) (ZN.scala:183)
  if (threadIdx.x == 0) {
    const int64_t mn = s_prefix, mx = mn | low_mask(offset);
    if (is_contained(mn, mx) || offset < 64 - a.range_precision) {
      rlo[0] = mn; rhi[0] = mx; rc[0] = 1; s_stop = 1;
    } else if (is_overlapped(mn, mx)) {
      F[0] = mn; s_stop = 2;
    } else {
      s_stop = 0;
    }
  }
  __syncthreads();
  if (s_stop == 1) nR = 1;
  if (s_stop == 2) K = 1;
  offset -= D;
  int level = 0;
  bool done = (K == 0);
  int err = QS_OK;
  while (!done) {
    // process level: K nodes in F at child offset `offset`; children -> G
    int64_t cc_carry = 0, co_carry = 0;
    int64_t stop_at = -1;
    for (int64_t c = 0; c < K; c += RTPB) {
      const int64_t i = c + threadIdx.x;
      uint32_t cmask = 0, omask = 0;
      int64_t p = 0;
      if (i < K) {
        p = F[i];
        for (int qd = 0; qd < (1 << D); ++qd) {
          const int64_t mn = p | jshl(qd, offset);
          const int64_t mx = mn | low_mask(offset);
          if (is_contained(mn, mx) || offset < 64 - a.range_precision) cmask |= 1u << qd;
          else if (is_overlapped(mn, mx)) omask |= 1u << qd;
        }
      }
      const int cc = __popc(cmask), co = __popc(omask);
      int64_t pt;   // one scan of (contained | overlapping << 32)
      const int64_t px = block_exscan((int64_t)cc | ((int64_t)co << 32), s_tmp, pt);
      const int64_t ccx = px & 0xffffffff, cox = px >> 32, cct = pt & 0xffffffff, cot = pt >> 32;
      // budget (ZN.scala:214) after node i; bounded above by the chunk totals at its first node
      int sl = INT32_MAX;
      if (nR + cc_carry + cct + co_carry + cot + (K - c - 1) >= range_stop) {
        if (threadIdx.x == 0) s_stop = INT32_MAX;
        __syncthreads();
        if (i < K) {
          const int64_t f = nR + cc_carry + ccx + cc + co_carry + cox + co + (K - i - 1);
          if (f >= range_stop) atomicMin(&s_stop, (int)threadIdx.x);
        }
        __syncthreads();
        sl = s_stop;
      }
      const bool emit = (i < K) && (sl == INT32_MAX || (int)threadIdx.x <= sl);
      if (emit) {
        int64_t rpos = nR + cc_carry + ccx, fpos = co_carry + cox;
        if (rpos + cc > a.rcap || fpos + co > a.fcap) {
          atomicMax(&s_err, QS_CAPACITY);
        } else {
          for (int qd = 0; qd < (1 << D); ++qd) {
            const int64_t mn = p | jshl(qd, offset);
            if (cmask >> qd & 1) { rlo[rpos] = mn; rhi[rpos] = mn | low_mask(offset); rc[rpos] = 1; ++rpos; }
            else if (omask >> qd & 1) { G[fpos++] = mn; }
          }
        }
      }
      if (sl != INT32_MAX) {
        // counts up to and including node c + sl
        __shared__ int64_t s_cc_upto, s_co_upto;
        if ((int)threadIdx.x == sl) { s_cc_upto = cc_carry + ccx + cc; s_co_upto = co_carry + cox + co; }
        __syncthreads();
        stop_at = c + sl;
        cc_carry = s_cc_upto;
        co_carry = s_co_upto;
        break;
      }
      cc_carry += cct;
      co_carry += cot;
      __syncthreads();
    }
    __syncthreads();
    if (s_err) { err = s_err; break; }
    if (stop_at >= 0) {
      // bottomOut (ZN.scala:173-180): rest of this level, then the queued children, as overlapping
      int64_t pos = nR + cc_carry;
      const int64_t rest = K - stop_at - 1, kids = co_carry;
      if (pos + rest + kids > a.rcap) { err = QS_CAPACITY; break; }
      for (int64_t j = threadIdx.x; j < rest; j += RTPB) {
        const int64_t mn = F[stop_at + 1 + j];
        rlo[pos + j] = mn; rhi[pos + j] = mn | low_mask(offset + D); rc[pos + j] = 0;
      }
      pos += rest;
      for (int64_t j = threadIdx.x; j < kids; j += RTPB) {
        const int64_t mn = G[j];
        rlo[pos + j] = mn; rhi[pos + j] = mn | low_mask(offset); rc[pos + j] = 0;
      }
      nR = pos + kids;
      break;
    }
    nR += cc_carry;
    K = co_carry;
    if (K == 0) break;
    // level terminator (ZN.scala:195-205)
    level += 1;
    offset -= D;
    int64_t* tmp = F; F = G; G = tmp;
    if (level >= a.recurse_stop || offset < 0) {
      if (nR + K > a.rcap) { err = QS_CAPACITY; break; }
      for (int64_t j = threadIdx.x; j < K; j += RTPB) {
        const int64_t mn = F[j];
        rlo[nR + j] = mn; rhi[nR + j] = mn | low_mask(offset + D); rc[nR + j] = 0;
      }
      nR += K;
      break;
    }
    __syncthreads();
  }
  __syncthreads();
  if (err) {
    batch_finish(a.bo, q, 0, err, nullptr);
    return;
  }
  gm_range* ws = a.out + qc * a.rcap;
  const int m = sort_merge(rlo, rhi, rc, (int)nR, a.gkey + qc * a.rcap, a.gidx + qc * a.rcap, ws, s_key, s_idx, s_tmp);
  batch_finish(a.bo, q, m, QS_OK, ws);
}

// ------------------------------------------------------------------ host side
namespace {

// The kernel's workspace for m queries with caps (fc, rc), as byte offsets: frontier ping / pong | rlo |
// rhi | rc | sort keys and ids (empty unless the lists sort in global memory) | merged scratch
struct ZWs { size_t fa, rlo, rhi, rc, gkey, gidx, out, total; };
constexpr ZWs z_ws(int64_t m, int64_t fc, int64_t rc) {
  const size_t f = (size_t)(m * fc), r = (size_t)(m * rc), g = rc > LDS_SORT ? r : 0;
  Carve c{16};   // the initializers run in order, the total last
  return ZWs{c.take(f * 16), c.take(r * 8), c.take(r * 8), c.take(r), c.take(g * 8), c.take(g * 4),
             c.take(r * sizeof(gm_range)), c.total};
}
// every region holds its elements, 16-B aligned and in order; the sort regions exist past LDS_SORT only
constexpr bool z_ws_ok(int64_t m, int64_t fc, int64_t rc) {
  const ZWs w = z_ws(m, fc, rc);
  const size_t r = (size_t)(m * rc), g = rc > LDS_SORT ? r : 0;
  const size_t o[8] = {w.fa, w.rlo, w.rhi, w.rc, w.gkey, w.gidx, w.out, w.total};
  const size_t need[7] = {(size_t)(m * fc) * 16, r * 8, r * 8, r, g * 8, g * 4, r * sizeof(gm_range)};
  for (int k = 0; k < 7; ++k)
    if (o[k] % 16 || o[k + 1] < o[k] + need[k] || (need[k] && o[k + 1] <= o[k])) return false;
  return w.total % 16 == 0 && (w.gkey == w.gidx && w.gidx == w.out) == (rc <= LDS_SORT);
}
static_assert(z_ws_ok(1, 4096, 4096) && z_ws_ok(1, 70024, 131072) && z_ws_ok(7, 4096, 4096) &&
                  z_ws_ok(7, 70024, 131072), "the Z workspace, for one query and for a chunk");
static_assert(z_ws(7, 70024, 131072).total <= 7 * z_ws(1, 70024, 131072).total, "per-query bytes bound a chunk's share");

// workspace sizing: the FIFO never holds more than rangeStop + 2^D items before the budget fires
inline int64_t z_caps(int max_ranges, int D, int64_t cap_hint) {
  return max_ranges > 0 ? (int64_t)max_ranges + (1 << D) + 16 : std::max<int64_t>(cap_hint, 1 << 16);
}

// the one body of the three Z entry points: `a` holds the inputs and the curve set-up
int z_ranges(gm_ctx* ctx, int D, ZRangesArgs a, int64_t nq, int max_ranges, const RangesOut& o) {
  a.range_stop = stop_of(max_ranges);
  RangesFamily fam;
  fam.fcap = fam.rcap = z_caps(max_ranges, D, o.cap);
  fam.per_query = [](int64_t fc, int64_t rc) { return (int64_t)z_ws(1, fc, rc).total; };
  fam.launch = [&](int64_t q0, int64_t m, int64_t fc, int64_t rc, char* base, const BatchOut& bo) {
    const ZWs w = z_ws(m, fc, rc);
    ZRangesArgs b = a;
    b.q0 = q0; b.bo = bo; b.fcap = fc; b.rcap = rc;
    b.fa = (int64_t*)(base + w.fa); b.rlo = (int64_t*)(base + w.rlo); b.rhi = (int64_t*)(base + w.rhi);
    b.rc = (uint8_t*)(base + w.rc); b.out = (gm_range*)(base + w.out);
    if (rc > LDS_SORT) { b.gkey = (int64_t*)(base + w.gkey); b.gidx = (int32_t*)(base + w.gidx); }   // else null
    if (D == 3) hipLaunchKernelGGL(k_zranges<3>, dim3((unsigned)m), dim3(RTPB), 0, ctx->stream, b);
    else hipLaunchKernelGGL(k_zranges<2>, dim3((unsigned)m), dim3(RTPB), 0, ctx->stream, b);
  };
  return run_ranges(ctx, nq, fam, o);
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" {

int gm_z3_ranges(gm_ctx* ctx, int64_t nq, const int32_t* box_off, const double* xy, const int32_t* time_off,
                 const int64_t* t, int period, int precision, int range_precision, int max_ranges, int max_recurse,
                 int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed, int32_t* query_status) {
  if (!ctx || nq < 0 || !box_off || !time_off || !out_off || period < 0 || period > 3 || precision < 1 ||
      precision > 21 || range_precision < 1 || range_precision > 64)
    return GM_E_INVALID;
  if (nq == 0) return empty_ranges(out_off, needed);
  const int64_t nbox = box_off[nq], ntim = time_off[nq];
  DevTemps tmp(ctx->stream);
  ZRangesArgs a{};
  int rc = to_dev(ctx, tmp, box_off, (size_t)nq + 1, &a.box_off);
  if (!rc) rc = to_dev(ctx, tmp, time_off, (size_t)nq + 1, &a.time_off);
  if (!rc) rc = to_dev(ctx, tmp, xy, (size_t)nbox * 4, &a.xy);
  if (!rc) rc = to_dev(ctx, tmp, t, (size_t)ntim * 2, &a.t);
  if (rc) return rc;
  a.lon = make_ndim(-180.0, 180.0, precision);
  a.lat = make_ndim(-90.0, 90.0, precision);
  a.tim = make_ndim(0.0, (double)max_offset(period), precision);
  a.range_precision = range_precision;
  a.recurse_stop = max_recurse < 0 ? INT32_MAX : max_recurse;   // Z3SFC.MaxRecursion = Int.MaxValue
  return z_ranges(ctx, 3, a, nq, max_ranges, {out_off, out, cap, needed, query_status});
}

int gm_z2_ranges(gm_ctx* ctx, int64_t nq, const int32_t* box_off, const double* xy, int precision,
                 int range_precision, int max_ranges, int max_recurse, int64_t* out_off, gm_range* out, int64_t cap,
                 int64_t* needed, int32_t* query_status) {
  if (!ctx || nq < 0 || !box_off || !out_off || precision < 1 || precision > 31 || range_precision < 1 ||
      range_precision > 64)
    return GM_E_INVALID;
  if (nq == 0) return empty_ranges(out_off, needed);
  const int64_t nbox = box_off[nq];
  DevTemps tmp(ctx->stream);
  ZRangesArgs a{};
  int rc = to_dev(ctx, tmp, box_off, (size_t)nq + 1, &a.box_off);
  if (!rc) rc = to_dev(ctx, tmp, xy, (size_t)nbox * 4, &a.xy);
  if (rc) return rc;
  a.lon = make_ndim(-180.0, 180.0, precision);
  a.lat = make_ndim(-90.0, 90.0, precision);
  a.range_precision = range_precision;
  a.recurse_stop = max_recurse < 0 ? 7 : max_recurse;   // ZN.DefaultRecurse (ZN.scala:293)
  return z_ranges(ctx, 2, a, nq, max_ranges, {out_off, out, cap, needed, query_status});
}

int gm_zranges(gm_ctx* ctx, int dims, int64_t nq, const int32_t* bound_off, const int64_t* zbounds,
               int range_precision, int max_ranges, int max_recurse, int64_t* out_off, gm_range* out, int64_t cap,
               int64_t* needed, int32_t* query_status) {
  if (!ctx || (dims != 2 && dims != 3) || nq < 0 || !bound_off || !out_off || range_precision < 1 ||
      range_precision > 64)
    return GM_E_INVALID;
  if (nq == 0) return empty_ranges(out_off, needed);
  const int64_t nb = bound_off[nq];
  if (nb > 0 && !zbounds) return GM_E_INVALID;
  DevTemps tmp(ctx->stream);
  ZRangesArgs a{};
  int rc = to_dev(ctx, tmp, bound_off, (size_t)nq + 1, &a.zb_off);
  if (!rc) rc = to_dev(ctx, tmp, zbounds, (size_t)nb * 2, &a.zb);
  if (rc) return rc;
  a.range_precision = range_precision;
  a.recurse_stop = max_recurse < 0 ? 7 : max_recurse;   // maxRecurse = Some(ZN.DefaultRecurse) (ZN.scala:113,293)
  return z_ranges(ctx, dims, a, nq, max_ranges, {out_off, out, cap, needed, query_status});
}

}  // extern "C"
