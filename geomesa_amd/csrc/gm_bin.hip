// gm_bin.hip -- the BIN track-record scan on gfx950: encode, sort by date and merge.
//
// Reference: BinAggregatingScan (idx/iterators/BinAggregatingScan.scala:129-168) turns every feature that
// passed the scan's filters into 16-B or 24-B little-endian records in one buffer
// (geomesa-utils/.../bin/BinaryOutputCallback.scala:28-41: int32 trackId, int32 (dtg / 1000).toInt,
// float32 lat, float32 lon[, int64 label]) and, asked to sort, orders the batch with BinSorter.compare
// (idx/utils/bin/BinSorter.scala:38-79: the int32 at offset 4, signed).  The values come from
// BinaryOutputEncoder (geomesa-utils/.../bin/BinaryOutputEncoder.scala): convertToTrack (:149-150),
// convertToDate (:153-154), convertToLabel (:156-168), pointToXY / pointToYX (:295-301, the JVM's d2f),
// the axis order (:281-286) and the six ToValues classes (:326-419: points, lines with one date, lines
// with a date per vertex, each with or without a label).  The contract is in include/geomesa_hip.h.
//
// Shape.  A candidate is a record the selection asks for: a row (points) or a vertex of a selected line
// slot.  Points take their candidates from the selection directly; lines take one pass over the slots
// (k_bin_slots: min(vertices, dates) per selected slot), a scan of those counts, and find a candidate's
// slot again by binary search over the scanned offsets, so a slot of any length is spread over as many
// lanes as it has vertices and still comes out in vertex order.  From there both run the count ->
// scan -> write pipeline of gm_scan.hpp (CountScan) over blocks of BROWS candidates: k_bin<false> counts
// the records of each block (a candidate with a null geometry or a NaN ordinate writes none; the selection
// is gm_scan.hpp's RowSel, resolved per entry by sel_row, per pair of rows by mask_pair) and takes
// the tallies, k_bin<true> reads the rows again, ranks them with wave ballots in candidate order and
// writes.  Without a mask that pipeline is the second attempt: the records are first written in one pass
// at their candidates' own positions, which is the result whenever every candidate wrote one (bin_encode).
// Columns load as pairs of rows per lane, one 16-B non-temporal load per 8-byte column, when
// every column is 16-B aligned (28-36 B per row), and with scalar loads otherwise; under a mask a pair
// neither of whose rows is selected loads nothing.  Records are staged per wave in LDS and leave as 16-B
// stores, a contiguous KiB per instruction (8-B stores when `out` is only 8-B aligned).  Measured on
// MI355X over 1B points (tools/bin_scan_probe.py, profiles/bin_scan_probe.json): 7.6 ms for 16-B records,
// 10.5 ms for 24-B, 96-97 % of the same run's copy rate over their 44 / 60 B per row.  The sort is gm_sort_keys over z = (uint32)(seconds ^ 2^31)
// -- stable, so the result is fixed and a sorted concatenation is BinSorter.mergeSort
// (BinSorter.scala:115-145) -- and a gather of the records through its permutation.
#include <algorithm>

#include "gm_arrow.hpp"
#include "gm_keys.hpp"
#include "gm_scan.hpp"

namespace gm {

constexpr int BTPB = 256;
constexpr int BPAIRS = 4;                     // pair steps per lane
constexpr int BROWS = BTPB * BPAIRS * 2;      // candidates per block (2048)
constexpr int BWAVES = BTPB / 64;

enum : int { BSRC_COLS = 0, BSRC_POINT = 1, BSRC_LINE = 2 };

struct BinArgs {
  RowSel sel;       // over the rows (columns) or slots (Arrow)
  int64_t ncand;    // candidate records: sel.units (points), the scanned slot counts' total (lines)
  int64_t cap;      // records `out` holds
  const double* x;
  const double* y;
  ArrowPts pts;
  const int32_t* o0;            // line: slot -> tuples
  const int64_t* dtg;           // per row / slot; NULL: date 0
  const uint8_t* dtg_valid;
  int64_t dtg_voff;
  const int32_t* date_off;      // line with a date list: slot -> dates
  const int64_t* dates;
  const uint8_t* dates_valid;
  int64_t dates_voff;
  const int32_t* track;
  const int64_t* label;
  const int64_t* cand_off;      // line: sel.units + 1 scanned candidate counts
  unsigned long long* holes;    // the direct write: candidates that wrote no record
  int32_t lat_lon;
  int32_t out16;                // `out` is 16-B aligned
};

struct BinRow {
  double x, y;
  long long t;
  long long label;
  int track;
  bool ok;
};

// (dtg / 1000).toInt: Long division truncates toward zero, toInt keeps the low 32 bits
__device__ __forceinline__ uint32_t bin_seconds(long long t_ms) { return (uint32_t)(uint64_t)(t_ms / 1000); }

// the first 16 bytes of a record as two little-endian words
__device__ __forceinline__ void bin_words(const BinRow& r, int lat_lon, uint64_t& w0, uint64_t& w1) {
  const float fx = __double2float_rn(r.x), fy = __double2float_rn(r.y);   // Double.toFloat (d2f)
  const float lat = lat_lon ? fx : fy, lon = lat_lon ? fy : fx;           // BinaryOutputEncoder.scala:281-286
  w0 = (uint64_t)(uint32_t)r.track | ((uint64_t)bin_seconds(r.t) << 32);
  w1 = (uint64_t)__float_as_uint(lat) | ((uint64_t)__float_as_uint(lon) << 32);
}

__device__ __forceinline__ void bin_store16(uint64_t* p, uint64_t a, uint64_t b) {
  lv2 v;
  v.x = (long long)a;
  v.y = (long long)b;
  __builtin_nontemporal_store(v, (lv2*)p);
}

// the per-slot pass of a line column: the candidates (vertices that can become records) of every entry
// of the selection -- min(vertices, dates) (ToValuesLinesDates, BinaryOutputEncoder.scala:386-389), 0 for
// an entry the selection leaves out, a bad id and a null slot
template <int SEL>
__global__ __launch_bounds__(256) void k_bin_slots(BinArgs a, int32_t* __restrict__ cand,
                                                   unsigned long long* __restrict__ tally) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= a.sel.units) return;
  int64_t r;
  const int sel = sel_row<SEL>(a.sel, u, r);
  if (sel < 0) atomicAdd(&tally[1], 1ull);
  int32_t m = 0;
  if (sel > 0) {
    if (!arrow_valid(a.pts.valid, a.pts.voff, r)) {
      atomicAdd(&tally[0], 1ull);   // the reference throws a NullPointerException
    } else {
      m = a.o0[r + 1] - a.o0[r];
      if (a.date_off) {
        const int32_t nd = a.date_off[r + 1] - a.date_off[r];
        if (nd != m) {
          atomicAdd(&tally[2], 1ull);
          m = nd < m ? nd : m;
        }
      }
      if (m < 0) m = 0;
    }
  }
  cand[u] = m;
}

// WRITE false: counts[block] = the records of the block's candidates, and the tallies.  WRITE true: the
// records, block b's from record offs[b] on, in candidate order.  SRC: x / y columns, an Arrow point
// column, an Arrow line column (F32: Float4 ordinates).  SEL: every row, the rows of a mask, the rows ids
// names (a line column resolved its mask in k_bin_slots).  VEC (columns, no ids): 16-B pair loads.
// DIRECT (WRITE, no mask): candidate c's record goes to record c, with no count pass before it, and
// *a.holes counts the candidates that wrote none; the result stands when there were none (bin_encode).
template <bool WRITE, int SRC, int SEL, bool LABEL, bool VEC, bool F32, bool DIRECT = false>
__global__ __launch_bounds__(BTPB) void k_bin(BinArgs a, int32_t* __restrict__ counts,
                                              const int64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                              unsigned long long* __restrict__ tally) {
  constexpr int RW = LABEL ? 3 : 2;   // 8-B words per record
  __shared__ int s_cnt[BPAIRS][BWAVES];
  __shared__ unsigned long long s_tally[2];
  __shared__ uint64_t s_stage[WRITE ? BWAVES : 1][WRITE ? 128 * RW : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t pbase = (int64_t)blockIdx.x * (BTPB * BPAIRS);
  if (!WRITE && threadIdx.x < 2) s_tally[threadIdx.x] = 0ull;
  long long skip = 0, bad = 0;

  // the values of a selected row rr (vertex i of it for a line) whose ordinates are x, y
  auto keep = [&](BinRow& row, double x, double y) {
    if (x != x || y != y) { ++skip; return false; }
    row.ok = true;
    row.x = x;
    row.y = y;
    return true;
  };
  auto take = [&](BinRow& row, int64_t rr, int64_t i, double x, double y) {
    if (!keep(row, x, y) || !WRITE) return;
    if (SRC == BSRC_LINE && a.dates) {
      const int64_t k = (int64_t)a.date_off[rr] + i;
      row.t = arrow_valid(a.dates_valid, a.dates_voff, k) ? a.dates[k] : 0;
    } else {
      row.t = a.dtg && arrow_valid(a.dtg_valid, a.dtg_voff, rr) ? a.dtg[rr] : 0;   // convertToDate: null -> 0
    }
    row.track = a.track[rr];
    row.label = LABEL ? a.label[rr] : 0;
  };
  auto fetch = [&](int64_t c, BinRow& row) {   // 0 <= c < a.ncand
    int64_t rr = c, i = 0;
    double x, y;
    if (SRC == BSRC_LINE) {
      const int64_t u = offset_slot(a.cand_off, a.sel.units, c);
      i = c - a.cand_off[u];
      rr = SEL == SEL_IDS ? a.sel.ids[u] : u;
      arrow_tuple<F32>(a.pts.c, (int64_t)a.o0[rr] + i, a.pts.flip, x, y);
    } else {
      const int k = sel_row<SEL>(a.sel, c, rr);
      if (k <= 0) { bad += k < 0; return; }
      if (SRC == BSRC_COLS) {
        x = a.x[rr];
        y = a.y[rr];
      } else {
        if (!arrow_valid(a.pts.valid, a.pts.voff, rr)) { ++skip; return; }   // the reference throws an NPE
        arrow_tuple<F32>(a.pts.c, rr, a.pts.flip, x, y);
      }
    }
    take(row, rr, i, x, y);
  };

  BinRow r[BPAIRS][2];
#pragma unroll
  for (int u = 0; u < BPAIRS; ++u) {
    const int64_t p = pbase + (int64_t)u * BTPB + threadIdx.x, c = 2 * p;
    r[u][0].ok = r[u][1].ok = false;
    if (VEC && c + 1 < a.ncand) {   // rows c and c + 1 of 16-B aligned columns, both in mask word c >> 6
      bool se = true, so = true;
      if (SEL == SEL_MASK) mask_pair(a.sel.mask[p >> 5], p, se, so);
      if (se || so) {
        const dv2 xv = ld_stream((const dv2*)a.x + p), yv = ld_stream((const dv2*)a.y + p);
        if (se) keep(r[u][0], xv.x, yv.x);
        if (so) keep(r[u][1], xv.y, yv.y);
        if (WRITE) {
          lv2 tv = {0, 0}, lb = {0, 0};
          if (a.dtg) tv = ld_stream((const lv2*)a.dtg + p);
          if (LABEL) lb = ld_stream((const lv2*)a.label + p);
          const int2 tr = *((const int2*)a.track + p);
          r[u][0].t = tv.x; r[u][1].t = tv.y;
          r[u][0].label = lb.x; r[u][1].label = lb.y;
          r[u][0].track = tr.x; r[u][1].track = tr.y;
        }
      }
    } else {
      if (c < a.ncand) fetch(c, r[u][0]);
      if (c + 1 < a.ncand) fetch(c + 1, r[u][1]);
    }
  }

  uint64_t be[BPAIRS], bo[BPAIRS];
#pragma unroll
  for (int u = 0; u < BPAIRS; ++u) {
    be[u] = __ballot(r[u][0].ok);
    bo[u] = __ballot(r[u][1].ok);
    if (!DIRECT && lane == 0) s_cnt[u][wave] = __popcll(be[u]) + __popcll(bo[u]);
  }
  if (!DIRECT) __syncthreads();

  if (!WRITE) {
    if (skip) atomicAdd(&s_tally[0], (unsigned long long)skip);
    if (bad) atomicAdd(&s_tally[1], (unsigned long long)bad);
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
#pragma unroll
      for (int u = 0; u < BPAIRS; ++u)
#pragma unroll
        for (int w = 0; w < BWAVES; ++w) tot += s_cnt[u][w];
      counts[blockIdx.x] = tot;
      if (s_tally[0]) atomicAdd(&tally[0], s_tally[0]);
      if (s_tally[1]) atomicAdd(&tally[1], s_tally[1]);
    }
    return;
  }

  uint64_t* ow = (uint64_t*)out;
  if (DIRECT && skip + bad) atomicAdd(a.holes, (unsigned long long)(skip + bad));
  int64_t run = DIRECT ? 0 : offs[blockIdx.x];
#pragma unroll
  for (int u = 0; u < BPAIRS; ++u) {
    int64_t base;                                                // the wave's first record
    if (DIRECT) {
      base = 2 * (pbase + (int64_t)u * BTPB + wave * 64);        // its first candidate
    } else {
      int before = 0, step = 0;
#pragma unroll
      for (int w = 0; w < BWAVES; ++w) {
        if (w < wave) before += s_cnt[u][w];
        step += s_cnt[u][w];
      }
      base = run + before;
      run += step;
    }
    const int rank = lanes_below(be[u]) + lanes_below(bo[u]);    // the lane's first record in the wave
    const int mine = __popcll(be[u]) + __popcll(bo[u]);
    uint64_t w0, w1;
    if (!a.out16) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t pos = base + rank + (j ? (int)r[u][0].ok : 0);
        if (r[u][j].ok && pos < a.cap) {
          bin_words(r[u][j], a.lat_lon, w0, w1);
          ow[RW * pos] = w0;
          ow[RW * pos + 1] = w1;
          if (LABEL) ow[RW * pos + 2] = (uint64_t)r[u][j].label;
        }
      }
    } else {
      // the wave's `mine` records (at most 128) as RW * mine words in LDS, then out as 16-B stores, a
      // contiguous KiB per instruction (a lane's own two records are 2 RW words apart: stored from
      // registers they leave as half-written 32-B pieces, which measured 11.4 ms per 1B 16-B records
      // against 7.6 staged; 8-B stores of 24-B records 12.0 ms against 10.5).  Global word g0 + k is
      // 16-B aligned when it is even
      uint64_t* st = s_stage[WRITE ? wave : 0];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (r[u][j].ok) {
          const int k = rank + (j ? (int)r[u][0].ok : 0);
          bin_words(r[u][j], a.lat_lon, w0, w1);
          st[RW * k] = w0;
          st[RW * k + 1] = w1;
          if (LABEL) st[RW * k + 2] = (uint64_t)r[u][j].label;
        }
      }
      wave_lds_sync();
      int64_t room = a.cap - base;
      if (room < 0) room = 0;
      const int nw = RW * (int)(room < mine ? room : mine);
      if (nw > 0) {
        const int64_t g0 = RW * base;
        const int s = (int)(g0 & 1);
        if (s && lane == 0) ow[g0] = st[0];
        const int np = (nw - s) >> 1;
        for (int k = lane; k < np; k += 64) bin_store16(ow + g0 + s + 2 * k, st[s + 2 * k], st[s + 2 * k + 1]);
        if (((nw - s) & 1) && lane == 63) ow[g0 + nw - 1] = st[nw - 1];
      }
      wave_lds_sync();
    }
  }
}

// ------------------------------------------------------------------ sort by date
// BinSorter.compare (BinSorter.scala:38-79) orders by the int32 at offset 4, signed: unsigned order of
// seconds ^ 2^31
__global__ __launch_bounds__(256) void k_bin_sort_keys(const uint8_t* __restrict__ in, int64_t n, int words,
                                                       int64_t* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t secs = (uint32_t)(((const uint64_t*)in)[i * words] >> 32);
  z[i] = (int64_t)(uint64_t)(secs ^ 0x80000000u);
}

// out record i = in record perm[i], one 8-B word per thread
__global__ __launch_bounds__(256) void k_bin_gather(const uint64_t* __restrict__ in, const int64_t* __restrict__ perm,
                                                    int64_t n, int words, uint64_t* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n * words) return;
  const int64_t i = w / words;
  const int k = (int)(w - i * words);
  out[w] = in[perm[i] * words + k];
}

int bin_sort(gm_ctx* ctx, const uint8_t* in, int64_t n, int record_bytes, uint8_t* out) {
  if (n == 0) return GM_OK;
  const int words = record_bytes / 8;
  DevTemps tmp(ctx->stream);
  int64_t *z, *z_out, *perm;
  int rc = tmp.alloc_async((size_t)n * 8, &z);
  if (!rc) rc = tmp.alloc_async((size_t)n * 8, &z_out);
  if (!rc) rc = tmp.alloc_async((size_t)n * 8, &perm);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bin_sort_keys, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in, n, words, z);
  GM_CHECK_LAUNCH();
  rc = gm_sort_keys(ctx, nullptr, nullptr, z, n, nullptr, nullptr, z_out, perm);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bin_gather, dim3(grid_for(n * words, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)in,
                     (const int64_t*)perm, n, words, (uint64_t*)out);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

// ------------------------------------------------------------------ encode
int bin_fail(const char* who, const char* why) {
  set_error(std::string(who) + ": " + why);
  return GM_E_INVALID;
}

// every GM_E_INVALID of the encode entries that does not depend on the source
int bin_check(const char* who, gm_ctx* ctx, int64_t n, const int32_t* track, const int64_t* label, const uint64_t* mask,
              const int64_t* ids, int64_t n_ids, const gm_bin_opts* o, const uint8_t* out, int64_t cap,
              const int64_t* n_records, const int64_t* tally) {
  if (!ctx) return bin_fail(who, "NULL context");
  if (!o) return bin_fail(who, "NULL options");
  if (!tally) return bin_fail(who, "NULL tally");
  if (!n_records) return bin_fail(who, "NULL n_records");
  if (n < 0) return bin_fail(who, "negative row count");
  if (cap < 0) return bin_fail(who, "negative capacity");
  if (cap > 0 && !out) return bin_fail(who, "NULL output with a capacity");
  if (const char* why = sel_check(mask, ids, n_ids)) return bin_fail(who, why);
  if (o->sort < 0 || o->sort > 1) return bin_fail(who, "sort must be 0 or 1");
  if (o->lat_lon < 0 || o->lat_lon > 1) return bin_fail(who, "lat_lon must be 0 or 1");
  if (!track && n > 0) return bin_fail(who, "NULL track column (hash the feature ids with gm_bin_track)");
  if (!aligned_to<8>(track) || !aligned_to<8>(label) || !aligned_to<8>(out) || !aligned_to<8>(tally))
    return bin_fail(who, "columns and outputs need 8-B alignment");
  return GM_OK;
}

int bin_encode(const char* who, gm_ctx* ctx, int src, bool f32, BinArgs a, const gm_bin_opts* o, uint8_t* out,
               int64_t* n_records, int64_t* tally) {
  GM_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int sel = sel_of(a.sel);
  const bool label = a.label != nullptr;
  const int rb = label ? 24 : 16;
  a.lat_lon = o->lat_lon;
  *n_records = 0;
  if (a.sel.units == 0) return GM_OK;
  DevTemps tmp(s);
  a.ncand = a.sel.units;
  if (src == BSRC_LINE) {
    CountScan slots;   // one count per entry of the selection
    int rc = slots.alloc(tmp, a.sel.units);
    if (rc) return rc;
    rc = with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) -> int {
      hipLaunchKernelGGL(k_bin_slots<E()>, dim3(grid_for(a.sel.units, 256)), dim3(256), 0, s, a, slots.counts,
                         (unsigned long long*)tally);
      GM_CHECK_LAUNCH();
      return GM_OK;
    });
    if (!rc) rc = slots.scan(ctx);
    if (!rc) rc = slots.total(ctx, &a.ncand);
    if (rc) return rc;
    a.cand_off = slots.offsets;
    if (a.ncand == 0) return GM_OK;
  }
  const int64_t nb = (a.ncand + BROWS - 1) / BROWS;
  if (nb > 2147483647LL) return bin_fail(who, "more than 2^31 - 1 blocks of candidate records");
  const bool vec = src == BSRC_COLS && sel != SEL_IDS && aligned16(a.x) && aligned16(a.y) && aligned16(a.dtg) &&
                   aligned16(a.label);
  const int64_t user_cap = a.cap;
  CountScan blocks;   // one count per block of candidates
  uint8_t* dst = out;
  // with sort the records are written to a temporary of `recs` records, then sorted into out
  auto stage = [&](int64_t recs) -> int {
    if (o->sort && dst == out) {
      const int rc = tmp.alloc_async((size_t)recs * rb, &dst);
      if (rc) return rc;
      a.cap = recs;
    }
    a.out16 = aligned16(dst);
    return GM_OK;
  };
  // the switches that exist for a source: vector loads for columns, Float4 for Arrow tuples; a line column's
  // mask was resolved per slot
  auto launch = [&](auto W, auto D) -> int {
    auto go = [&](auto kern) -> int {
      hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(BTPB), 0, s, a, blocks.counts, (const int64_t*)blocks.offsets,
                         dst, (unsigned long long*)tally);
      GM_CHECK_LAUNCH();
      return GM_OK;
    };
    return with_value<BSRC_COLS, BSRC_POINT, BSRC_LINE>(src, [&](auto S) {
      return with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) {
        return with_flags([&](auto L, auto V, auto F) {
          constexpr bool WR = decltype(W)::value;
          constexpr bool DR = decltype(D)::value;
          if constexpr (S() == BSRC_COLS)
            return go(k_bin<WR, BSRC_COLS, E(), WR && L(), V() && E() != SEL_IDS, false, DR && E() != SEL_MASK>);
          else if constexpr (S() == BSRC_LINE)
            return go(k_bin<WR, BSRC_LINE, E() == SEL_IDS ? SEL_IDS : SEL_NONE, WR && L(), false, F(), DR>);
          else
            return go(k_bin<WR, BSRC_POINT, E(), WR && L(), false, F(), DR && E() != SEL_MASK>);
        }, label, vec, f32);
      });
    });
  };
  // The direct write.  Without a mask every candidate writes a record unless its geometry is null, an
  // ordinate is NaN or its id is bad, so candidate c's record is written at record c at once and the
  // candidates that wrote none are counted: none, and the buffer is the result -- one pass over 44 B a
  // row where count + write take 60 (7.6 ms per 1B 16-B records against 10.6: tools/bin_scan_probe.py's
  // NaN-row leg runs both, 18.3 ms).  Any, and the count -> scan -> write pipeline below runs over the
  // same rows and writes the buffer again.
  if ((src == BSRC_LINE || sel != SEL_MASK) && a.ncand <= user_cap && !(o->sort && a.ncand > (int64_t)UINT32_MAX)) {
    int rc = tmp.alloc_async(8, &a.holes);
    if (rc) return rc;
    GM_HIP(hipMemsetAsync(a.holes, 0, 8, s));
    rc = stage(a.ncand);
    if (!rc) rc = launch(Bool<true>{}, Bool<true>{});
    int64_t holes = 0;
    if (!rc) rc = read_i64(ctx, a.holes, &holes);
    if (rc) return rc;
    if (holes == 0) {
      *n_records = a.ncand;
      return o->sort ? bin_sort(ctx, dst, a.ncand, rb, out) : GM_OK;
    }
  }
  int64_t total = 0;
  int rc = blocks.alloc(tmp, nb);
  if (!rc) rc = launch(Bool<false>{}, Bool<false>{});
  if (!rc) rc = blocks.scan(ctx);
  if (!rc) rc = blocks.total(ctx, &total);
  if (rc) return rc;
  *n_records = total;
  if (total > user_cap) return GM_E_CAPACITY;
  if (total == 0) return GM_OK;
  if (o->sort && total > (int64_t)UINT32_MAX) return bin_fail(who, "more than 2^32 - 1 records with sort");
  rc = stage(total);
  if (!rc) rc = launch(Bool<true>{}, Bool<false>{});
  if (rc) return rc;
  return o->sort ? bin_sort(ctx, dst, total, rb, out) : GM_OK;
}

// ------------------------------------------------------------------ track ids and labels
// convertToTrack (BinaryOutputEncoder.scala:149-150): null -> 0, else hashCode.  String.hashCode is
// s[0] * 31^(n-1) + ... over UTF-16 code units: the slot's UTF-8 is decoded a code point at a time, a
// 4-byte sequence giving its two surrogates.  No read leaves [b, e): a sequence the slot's end cuts short
// takes the bytes there are.
__device__ __forceinline__ int32_t bin_hash_utf8(const uint8_t* __restrict__ s, int64_t b, int64_t e) {
  uint32_t h = 0;
  int64_t i = b;
  while (i < e) {
    const uint32_t b0 = s[i++];
    uint32_t cp = b0;
    if (b0 >= 0x80u) {
      const int need = b0 >= 0xf0u ? 3 : (b0 >= 0xe0u ? 2 : 1);
      cp = b0 & (0x3fu >> need);
      for (int k = 0; k < need && i < e; ++k) cp = (cp << 6) | (s[i++] & 0x3fu);
    }
    if (cp >= 0x10000u) {
      cp -= 0x10000u;
      h = 31u * h + (0xd800u + ((cp >> 10) & 0x3ffu));
      h = 31u * h + (0xdc00u + (cp & 0x3ffu));
    } else {
      h = 31u * h + cp;
    }
  }
  return (int32_t)h;
}

__device__ __forceinline__ int32_t bin_fold(uint64_t v) { return (int32_t)(uint32_t)(v ^ (v >> 32)); }

// one lane per slot.  LABEL false: convertToTrack into int32; true: convertToLabel
// (BinaryOutputEncoder.scala:156-168) into int64 -- Number.longValue, else the first 8 UTF-8 bytes, byte
// i at bits 8i
template <int TYPE, bool LABEL>
__global__ __launch_bounds__(256) void k_bin_attr(const void* __restrict__ values, const int32_t* __restrict__ offsets,
                                                  const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                  int32_t* __restrict__ track, int64_t* __restrict__ label) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t h = 0;
  int64_t l = 0;
  if (arrow_valid(valid, voff, i)) {
    if (TYPE == GM_ATTR_INT32) {
      h = ((const int32_t*)values)[i];           // Integer.hashCode
      l = h;                                     // Integer.longValue
    } else if (TYPE == GM_ATTR_INT64) {
      l = ((const int64_t*)values)[i];
      h = bin_fold((uint64_t)l);                 // Long.hashCode
    } else if (TYPE == GM_ATTR_FLOAT64) {
      const double d = ((const double*)values)[i];
      if (LABEL) l = jvm_d2l(d);                 // Double.longValue
      // Double.hashCode folds doubleToLongBits, which gives every NaN the canonical bits
      else h = bin_fold(d != d ? 0x7ff8000000000000ull : (uint64_t)__double_as_longlong(d));
    } else {
      const uint8_t* s = (const uint8_t*)values;
      const int64_t b = offsets[i], e = offsets[i + 1];
      if (LABEL) {
        uint64_t sum = 0;
        for (int k = 0; k < 8 && b + k < e; ++k) sum += (uint64_t)s[b + k] << (8 * k);
        l = (int64_t)sum;
      } else {
        h = bin_hash_utf8(s, b, e);
      }
    }
  }
  if (LABEL) label[i] = l; else track[i] = h;
}

int bin_attr(const char* who, gm_ctx* ctx, const gm_attr_column* col, int64_t n, int32_t* track, int64_t* label) {
  if (!ctx) return bin_fail(who, "NULL context");
  if (n < 0) return bin_fail(who, "negative row count");
  if (n == 0) return GM_OK;
  if (!col) return bin_fail(who, "NULL column");
  if (col->type < GM_ATTR_INT32 || col->type > GM_ATTR_UTF8) return bin_fail(who, "unknown attribute type");
  if (!track && !label) return bin_fail(who, "NULL output");
  if (col->type == GM_ATTR_UTF8 ? !col->offsets : !col->values) return bin_fail(who, "NULL values or offsets");
  const bool a8 = col->type == GM_ATTR_INT64 || col->type == GM_ATTR_FLOAT64;
  if ((a8 && !aligned_to<8>(col->values)) || (col->type == GM_ATTR_INT32 && !aligned_to<4>(col->values)) ||
      !aligned_to<4>(col->offsets) || !aligned_to<4>(track) || !aligned_to<8>(label))
    return bin_fail(who, "values, offsets and the output need their natural alignment");
  GM_HIP(hipSetDevice(ctx->device));
  return with_value<GM_ATTR_INT32, GM_ATTR_INT64, GM_ATTR_FLOAT64, GM_ATTR_UTF8>(col->type, [&](auto T) {
    return with_flags([&](auto L) -> int {
      hipLaunchKernelGGL((k_bin_attr<T(), L()>), dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, col->values,
                         col->offsets, col->validity, col->validity_offset, n, track, label);
      GM_CHECK_LAUNCH();
      return GM_OK;
    }, label != nullptr);
  });
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_bin_track(gm_ctx* ctx, const gm_attr_column* col, int64_t n, int32_t* track) {
  return bin_attr("gm_bin_track", ctx, col, n, track, nullptr);
}

int gm_bin_label(gm_ctx* ctx, const gm_attr_column* col, int64_t n, int64_t* label) {
  return bin_attr("gm_bin_label", ctx, col, n, nullptr, label);
}

int gm_bin_points(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, const int32_t* track,
                  const int64_t* label, int64_t n, const uint64_t* mask, const int64_t* ids, int64_t n_ids,
                  const gm_bin_opts* o, uint8_t* out, int64_t cap, int64_t* n_records, int64_t* tally) {
  const char* who = "gm_bin_points";
  const int rc = bin_check(who, ctx, n, track, label, mask, ids, n_ids, o, out, cap, n_records, tally);
  if (rc) return rc;
  if (n > 0 && (!x || !y)) return bin_fail(who, "x and y must be given");
  if (!aligned_to<8>(x) || !aligned_to<8>(y) || !aligned_to<8>(t_ms))
    return bin_fail(who, "x, y and t_ms need 8-B alignment");
  BinArgs a{};
  a.sel = row_sel(n, mask, ids, n_ids);
  a.cap = cap;
  a.x = x;
  a.y = y;
  a.dtg = t_ms;
  a.track = track;
  a.label = label;
  return bin_encode(who, ctx, BSRC_COLS, false, a, o, out, n_records, tally);
}

int gm_bin_arrow(gm_ctx* ctx, const gm_geom_column* geom, const gm_time_column* dtg, const int32_t* date_off,
                 const gm_time_column* dates, const int32_t* track, const int64_t* label, int64_t n,
                 const uint64_t* mask, const int64_t* ids, int64_t n_ids, const gm_bin_opts* o, uint8_t* out,
                 int64_t cap, int64_t* n_records, int64_t* tally) {
  const char* who = "gm_bin_arrow";
  const int rc = bin_check(who, ctx, n, track, label, mask, ids, n_ids, o, out, cap, n_records, tally);
  if (rc) return rc;
  if ((date_off == nullptr) != (dates == nullptr)) return bin_fail(who, "date_off and dates come together");
  if (rejects_wkb(geom, who, true)) return GM_E_INVALID;
  if (geom && geom->type != GM_GEOM_POINT && geom->type != GM_GEOM_LINESTRING)
    return bin_fail(who, "geom must be a GM_GEOM_POINT or GM_GEOM_LINESTRING column");
  if (geom && geom->type == GM_GEOM_POINT && dates) return bin_fail(who, "a date list needs a GM_GEOM_LINESTRING column");
  if (n > 0 && !geom_col_ok(geom)) return bin_fail(who, "geom needs coords, 64- or 32-bit ordinates and its List offsets");
  if (n > 0 && ((dtg && !dtg->millis) || (dates && !dates->millis))) return bin_fail(who, "a date column without millis");
  if ((dtg && !aligned_to<8>(dtg->millis)) || (dates && !aligned_to<8>(dates->millis)) || !aligned_to<4>(date_off) ||
      (geom && (!aligned_to<8>(geom->coords) || !aligned_to<4>(geom->offsets[0]))))
    return bin_fail(who, "ordinates and dates need 8-B alignment, List offsets 4-B");
  BinArgs a{};
  a.sel = row_sel(n, mask, ids, n_ids);
  a.cap = cap;
  a.track = track;
  a.label = label;
  int src = BSRC_POINT;
  bool f32 = false;
  if (n > 0) {
    f32 = geom->ordinal_bits == 32;
    a.pts = ArrowPts{geom->coords, geom->validity, geom->validity_offset, geom->flip_axis, f32};
    if (geom->type == GM_GEOM_LINESTRING) {
      src = BSRC_LINE;
      a.o0 = geom->offsets[0];
    }
    if (dtg) {
      a.dtg = dtg->millis;
      a.dtg_valid = dtg->validity;
      a.dtg_voff = dtg->validity_offset;
    }
    if (dates && src == BSRC_LINE) {
      a.date_off = date_off;
      a.dates = dates->millis;
      a.dates_valid = dates->validity;
      a.dates_voff = dates->validity_offset;
    }
  }
  return bin_encode(who, ctx, src, f32, a, o, out, n_records, tally);
}

int gm_bin_sort(gm_ctx* ctx, const uint8_t* in, int64_t n_records, int32_t record_bytes, uint8_t* out) {
  const char* who = "gm_bin_sort";
  if (!ctx) return bin_fail(who, "NULL context");
  if (record_bytes != 16 && record_bytes != 24) return bin_fail(who, "record_bytes must be 16 or 24");
  if (n_records < 0) return bin_fail(who, "negative record count");
  if (n_records > (int64_t)UINT32_MAX) return bin_fail(who, "more than 2^32 - 1 records with sort");
  if (n_records == 0) return GM_OK;
  if (!in || !out) return bin_fail(who, "NULL records");
  if (in == out) return bin_fail(who, "the sort is not in place");
  if (!aligned_to<8>(in) || !aligned_to<8>(out)) return bin_fail(who, "records need 8-B alignment");
  GM_HIP(hipSetDevice(ctx->device));
  return bin_sort(ctx, in, n_records, record_bytes, out);
}

}  // extern "C"
