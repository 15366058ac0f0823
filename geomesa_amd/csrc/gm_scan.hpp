// gm_scan.hpp -- what the streaming scans share: the two mask-pass skeletons (pair_scan: two rows per
// lane; row_scan: one), the device-wide exclusive scan with its count -> scan -> total helper
// (CountScan), the row selection of the aggregating scans (RowSel, sel_row) and the mask -> block scan ->
// ordered compaction pipeline of the filter scans (alloc_scan / finish_scan / end_scan), and the seek and
// candidate scan of the sorted tables (k_range_bounds, seek_ranges, scan_candidates).  Used by gm_filter.hip,
// gm_geom_filter.hip, gm_pip_query.hip, gm_density.hip, gm_bin.hip, gm_freq.hip and gm_attr_table.hip.
#pragma once

#include <algorithm>

#include "gm_internal.hpp"
#include "gm_poly_query_host.hpp"
#include "gm_seek.hpp"

namespace gm {

constexpr int FTPB = 256;             // threads per block
#ifndef GM_FELEMS
#define GM_FELEMS 16  // sweep (profiles/r2_felems_sweep.txt, z3filter_scan ms per 1B rows): 4 2.27, 8 1.81-1.94, 16 1.68-1.80, 32 1.92-1.94
#endif
constexpr int FELEMS = GM_FELEMS;     // rows per thread per block
static_assert(FELEMS % 2 == 0 && FELEMS >= 2, "pair layout");
constexpr int FROWS = FTPB * FELEMS;  // rows per block (4096) -> 64 mask words

// ------------------------------------------------------------------ pass A, the pair layout
// A lane-per-row load moves 2 B (bin) and 8 B (z) per lane per instruction; on gfx950 narrow per-lane
// accesses stream at roughly half the 16-B rate.  The column scans (k_*_mask_v, k_query_mask) use the
// layout of the encode kernels: each lane takes PAIRS of consecutive rows, one 16-B load per 8-byte
// column (z, x, y, t) and one 4-B load of the two bins (VEC; two scalar loads per column when a column
// is not 16-B aligned), and pair p of lane l in step u sits at block_base + u*256 + l, so every wave
// instruction reads one contiguous 1 KiB run.  A wave step covers 128 rows: ballot(row 2l) and
// ballot(row 2l+1) interleave bit by bit into the two 64-bit mask words of those rows.  A block covers
// FROWS = 4096 rows (8 steps), as a row_scan block does, so block_counts, the count scan and
// k_mask_to_ids are shared with the lane-per-row kernels.
typedef short sv2 __attribute__((ext_vector_type(2)));
constexpr int FPAIRS = FELEMS / 2;   // pair steps per lane

// 32 -> 64-bit bit spread (bit k -> bit 2k)
__device__ __forceinline__ uint64_t spread2_32(uint32_t v) {
  return (uint64_t)spread2_16(v & 0xffffu) | ((uint64_t)spread2_16(v >> 16) << 32);
}

// the wave's two mask words from the even-row and odd-row ballots; lanes 0 and 1 store one each
__device__ __forceinline__ void put_pair_words(uint64_t even, uint64_t odd, uint64_t* __restrict__ mask, int64_t word,
                                               int64_t nwords) {
  const int lane = threadIdx.x & 63;
  if (lane < 2) {
    const uint32_t e = (uint32_t)(lane ? (even >> 32) : even), o = (uint32_t)(lane ? (odd >> 32) : odd);
    if (word + lane < nwords) mask[word + lane] = spread2_32(e) | (spread2_32(o) << 1);
  }
}

template <int TPB = FTPB>
__device__ __forceinline__ void block_count_waves(int wave_cnt, int32_t* block_counts) {
  __shared__ int s_wc[TPB / 64];
  if ((threadIdx.x & 63) == 0) s_wc[threadIdx.x >> 6] = wave_cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < TPB / 64; ++i) s += s_wc[i];
    block_counts[blockIdx.x] = s;
  }
}

// Row predicate over a pair layout: LOAD(p, u) stages pair p, ROW(u, j) evaluates row j (0/1) of the
// staged pair, TAIL(u) evaluates the odd last row n-1 (pair index n/2) with scalar loads.
template <class Load, class Row, class Tail>
__device__ __forceinline__ void pair_scan(int64_t n, uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts,
                                          Load load, Row row, Tail tail) {
  const int64_t npairs = n >> 1, nwords = (n + 63) >> 6;
  const int wave = threadIdx.x >> 6;
  const int64_t pbase = (int64_t)blockIdx.x * (FTPB * FPAIRS);
#pragma unroll
  for (int u = 0; u < FPAIRS; ++u) {
    const int64_t p = pbase + (int64_t)u * FTPB + threadIdx.x;
    if (p < npairs) load(p, u);
  }
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < FPAIRS; ++u) {
    const int64_t p = pbase + (int64_t)u * FTPB + threadIdx.x;
    bool e = false, o = false;
    if (p < npairs) { e = row(u, 0); o = row(u, 1); }
    else if (p == npairs && (n & 1)) e = tail(p);
    const uint64_t be = __ballot(e), bo = __ballot(o);
    cnt += __popcll(be) + __popcll(bo);
    put_pair_words(be, bo, mask, ((pbase + (int64_t)u * FTPB + wave * 64) * 2) >> 6, nwords);
  }
  block_count_waves(cnt, block_counts);
}

// The lane-per-row counterpart (row keys, candidate spaces: the row's bytes are found per row): PRED(i)
// evaluates row i < total; step u of a block takes rows block_base + u*256 + [0, 256), one ballot word
// per wave.  UNROLL steps are in flight at once: 1 for a predicate that searches or walks a descriptor, 4 for
// one that only streams its columns.
template <int UNROLL = 1, class Pred>
__device__ __forceinline__ void row_scan(int64_t total, uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts,
                                         Pred pred) {
  const int64_t base = (int64_t)blockIdx.x * FROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
#pragma unroll UNROLL
  for (int u = 0; u < FELEMS; ++u) {
    const int64_t i = base + (int64_t)u * FTPB + threadIdx.x;
    bool ok = false;
    if (i < total) ok = pred(i);
    const uint64_t w = __ballot(ok);
    if (lane == 0) {
      const int64_t word = (base + (int64_t)u * FTPB + wave * 64) >> 6;
      if ((word << 6) < total) mask[word] = w;
      cnt += __popcll(w);
    }
  }
  block_count_waves(cnt, block_counts);   // reads lane 0's
}

// Device-wide exclusive scan, two levels (block counts of the mask scans, radix-sort histograms).
// A single workgroup walking ~500k counts took 1.2-1.5 ms per call -- a third of the 1B-row scan
// it followed.
//   k_scan_partials: one block per SCAN_CHUNK values -> chunk sums
//   k_scan_chunks  : one workgroup scans the chunk sums (a few hundred) in place; total -> *total_out
//   k_scan_apply   : per chunk, block-wide exclusive scan + the chunk's base -> out[] (in place is fine:
//                    every thread reads its 16 values before writing them)
constexpr int SCAN_TPB = 256;
constexpr int SCAN_PER = 16;                          // consecutive counts per thread
constexpr int SCAN_CHUNK = SCAN_TPB * SCAN_PER;       // 4096 counts per block

// block-wide exclusive scan of one value per thread (256 threads); *total gets the block sum
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t* total) {
  __shared__ int64_t s_w[SCAN_TPB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int64_t wbase = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SCAN_TPB / 64; ++i) {
    if (i < w) wbase += s_w[i];
    tot += s_w[i];
  }
  *total = tot;
  return wbase + inc - v;
}

template <class TIn>
__global__ __launch_bounds__(SCAN_TPB) void k_scan_partials(const TIn* __restrict__ counts, int64_t nb,
                                                            int64_t* __restrict__ partials) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK;
  int64_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_PER; ++i) {
    const int64_t j = base + (int64_t)i * SCAN_TPB + threadIdx.x;   // coalesced
    if (j < nb) s += counts[j];
  }
  int64_t tot;
  block_excl_scan(s, &tot);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

static __global__ __launch_bounds__(SCAN_TPB) void k_scan_chunks(int64_t* __restrict__ partials, int64_t np,
                                                          int64_t* __restrict__ total_out) {
  int64_t run = 0;
  for (int64_t c0 = 0; c0 < np; c0 += SCAN_TPB) {   // np is small: a few rounds at most
    const int64_t j = c0 + threadIdx.x;
    const int64_t v = j < np ? partials[j] : 0;
    int64_t tot;
    const int64_t ex = block_excl_scan(v, &tot);
    if (j < np) partials[j] = run + ex;
    run += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total_out) *total_out = run;
}

template <class TIn, class TOut>
__global__ __launch_bounds__(SCAN_TPB) void k_scan_apply(const TIn* counts, int64_t nb,
                                                         const int64_t* __restrict__ partials, TOut* offsets) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_PER;   // 16 consecutive
  TIn c[SCAN_PER];
  int64_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_PER; ++i) {
    c[i] = base + i < nb ? counts[base + i] : 0;
    s += c[i];
  }
  int64_t tot;
  int64_t run = partials[blockIdx.x] + block_excl_scan(s, &tot);
#pragma unroll
  for (int i = 0; i < SCAN_PER; ++i) {
    if (base + i < nb) offsets[base + i] = (TOut)run;
    run += c[i];
  }
}

inline int64_t scan_partials_len(int64_t n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1; }

// out[i] = sum(in[0, i)), total -> *total_out (device, may be null); partials: scan_partials_len(n)
// int64 of device scratch
template <class TIn, class TOut>
inline void launch_excl_scan(hipStream_t s, const TIn* in, int64_t n, TOut* out, int64_t* partials,
                             int64_t* total_out) {
  const int64_t nchunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  if (nchunks > 0)
    hipLaunchKernelGGL((k_scan_partials<TIn>), dim3((unsigned)nchunks), dim3(SCAN_TPB), 0, s, in, n, partials);
  hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(SCAN_TPB), 0, s, partials, nchunks, total_out);
  if (nchunks > 0)
    hipLaunchKernelGGL((k_scan_apply<TIn, TOut>), dim3((unsigned)nchunks), dim3(SCAN_TPB), 0, s, in, n, partials, out);
}

// One call's count -> scan -> total over nb blocks, in the stream's pool: the caller's count kernel fills
// counts[nb], scan() enqueues the exclusive scan into offsets[nb] (the total behind them), total() reads
// the total back (synchronises); a write kernel then takes block b's output from offsets[b] on.
struct CountScan {
  int64_t nb = 0;
  int32_t* counts = nullptr;
  int64_t* offsets = nullptr;
  int64_t* partials = nullptr;
  int alloc(DevTemps& tmp, int64_t nblocks) {
    nb = nblocks;
    int rc = tmp.alloc_async((size_t)nb * 4, &counts);
    if (!rc) rc = tmp.alloc_async((size_t)(nb + 1) * 8, &offsets);
    if (!rc) rc = tmp.alloc_async((size_t)scan_partials_len(nb) * 8, &partials);
    return rc;
  }
  int scan(gm_ctx* ctx);   // gm_filter.hip, with finish_scan: one instantiation of the scan kernels
  int total(gm_ctx* ctx, int64_t* t) { return read_i64(ctx, offsets + nb, t); }
};

struct ScanBufs {
  uint64_t* mask = nullptr;
  int32_t* counts = nullptr;
  int64_t* offsets = nullptr;
  int64_t* partials = nullptr;   // chunk sums of the two-level count scan
  int32_t* desc = nullptr;
};

// pass A outputs (mask words + per-block counts) and a descriptor area, carved from the context's
// scan workspace; user_mask, when given, receives the mask instead
int alloc_scan(gm_ctx* ctx, int64_t n, uint64_t* user_mask, size_t desc_words, ScanBufs& b);
// passes B and C: block-count scan, ids in ascending row order, match count readback
int finish_scan(gm_ctx* ctx, int64_t n, ScanBufs& b, int64_t* ids, int64_t ids_cap, int64_t* n_match);

// A scan's epilogue: finish_scan, then whatever the scan reads back or answers first (`before`), then
// GM_E_CAPACITY when the caller asked for both the count and the ids and ids[] was too short.
template <class Before>
int end_scan(gm_ctx* ctx, int64_t n, ScanBufs& b, int64_t* ids, int64_t ids_cap, int64_t* n_match, Before before) {
  int rc = finish_scan(ctx, n, b, ids, ids_cap, n_match);
  if (!rc) rc = before();
  if (rc) return rc;
  return n_match && ids && *n_match > ids_cap ? GM_E_CAPACITY : GM_OK;
}
inline int end_scan(gm_ctx* ctx, int64_t n, ScanBufs& b, int64_t* ids, int64_t ids_cap, int64_t* n_match) {
  return end_scan(ctx, n, b, ids, ids_cap, n_match, [] { return (int)GM_OK; });
}

// ------------------------------------------------------------------ row selection of an aggregating scan
// Every row, the rows of a mask, or the rows ids names (gm_density_*, gm_bin_*: what a scan or a table
// query kept).
enum : int { SEL_NONE = 0, SEL_MASK = 1, SEL_IDS = 2 };
struct RowSel {
  int64_t n;              // rows (or slots) of the source
  int64_t units;          // entries of the selection: n, or the entries of ids
  const uint64_t* mask;   // bit r & 63 of word r >> 6 selects row r
  const int64_t* ids;     // the selected rows, in the caller's order
};
inline RowSel row_sel(int64_t n, const uint64_t* mask, const int64_t* ids, int64_t n_ids) {
  return RowSel{n, ids ? n_ids : n, mask, ids};
}
inline int sel_of(const RowSel& s) { return s.ids ? SEL_IDS : (s.mask ? SEL_MASK : SEL_NONE); }
// the selection errors of an entry point that do not depend on its source; null: none
inline const char* sel_check(const uint64_t* mask, const int64_t* ids, int64_t n_ids) {
  if (ids && n_ids < 0) return "negative id count";
  if (mask && ids) return "mask and ids are exclusive";
  if (!aligned_to<8>(mask) || !aligned_to<8>(ids)) return "columns and outputs need 8-B alignment";
  return nullptr;
}

__device__ __forceinline__ bool mask_bit(const uint64_t* __restrict__ mask, int64_t r) {
  return (mask[r >> 6] >> (r & 63)) & 1ull;
}
// the bits of rows 2p and 2p + 1 out of their word w = mask[p >> 5]
__device__ __forceinline__ void mask_pair(uint64_t w, int64_t p, bool& even, bool& odd) {
  const uint64_t b = w >> ((2 * p) & 63);
  even = b & 1ull;
  odd = (b >> 1) & 1ull;
}
// entry u < s.units of the selection -> row r.  1: selected; 0: not; -1: an id outside [0, n), for the
// caller's tally (the count comes back as a value: a counter taken by reference cost k_density's ids
// instantiations 4 SGPRs and one of them a wave of occupancy)
template <int SEL>
__device__ __forceinline__ int sel_row(const RowSel& s, int64_t u, int64_t& r) {
  if (SEL == SEL_IDS) {
    r = s.ids[u];
    return (uint64_t)r < (uint64_t)s.n ? 1 : -1;
  }
  r = u;
  return SEL != SEL_MASK || mask_bit(s.mask, u);
}

// ------------------------------------------------------------------ candidate space of a table scan
// the entry of the scanned offsets off[0, n) that holds c: upper_bound, minus one
__device__ __forceinline__ int64_t offset_slot(const int64_t* __restrict__ off, int64_t n, int64_t c) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (off[m] <= c) lo = m + 1; else hi = m;
  }
  return lo - 1;
}
// candidate c -> its range -> table row
__device__ __forceinline__ int64_t cand_row(const int64_t* __restrict__ coff, const int64_t* __restrict__ start,
                                            int64_t nr, int64_t c) {
  const int64_t r = offset_slot(coff, nr, c);
  return start[r] + (c - coff[r]);
}

// ------------------------------------------------------------------ the seek of a table scan
// A sorted table's key columns are a Cols type: Cols::Key with lt(a, b), the table's byte order (host and
// device), and next(k, &out), the key after k (host; false past the last key); Cols::at(i) is row i's key
// (device).  The Z tables' is ZCols (gm_filter.hip), the attribute table's AttrCols (gm_attr_table.hip).  SeekRange,
// merge_ranges and the attribute key are gm_seek.hpp's, which a host compiler takes alone.
// row interval of each range: [first row >= lo, first row > hi)
template <class Cols>
__global__ __launch_bounds__(FTPB) void k_range_bounds(Cols c, int64_t n, const SeekRange<typename Cols::Key>* __restrict__ rg,
                                                       int64_t nr, int64_t* __restrict__ start, int64_t* __restrict__ len) {
  using Key = typename Cols::Key;
  const int64_t r = (int64_t)blockIdx.x * FTPB + threadIdx.x;
  if (r >= nr) return;
  const SeekRange<Key> q = rg[r];
  int64_t lo = 0, hi = n;  // lower_bound(lo key)
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (Key::lt(c.at(m), q.lo)) lo = m + 1; else hi = m;
  }
  const int64_t a = lo;
  hi = n;  // upper_bound(hi key)
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (!Key::lt(q.hi, c.at(m))) lo = m + 1; else hi = m;
  }
  start[r] = a;
  len[r] = lo - a;
}

// the merged ranges to the device and their row intervals: start[nr], and the lengths in coff[nr] (+ 1 entry
// for scan_candidates' total)
template <class Cols>
int seek_ranges(gm_ctx* ctx, DevTemps& tmp, const Cols& c, int64_t n, const std::vector<SeekRange<typename Cols::Key>>& rg,
                int64_t** start, int64_t** coff) {
  using R = SeekRange<typename Cols::Key>;
  const int64_t nr = (int64_t)rg.size();
  R* d_rg = nullptr;
  int rc = tmp.alloc_async((size_t)nr * sizeof(R), &d_rg);
  if (!rc) rc = tmp.alloc_async((size_t)nr * 8, start);
  if (!rc) rc = tmp.alloc_async((size_t)(nr + 1) * 8, coff);
  if (!rc) rc = copy_h2d(ctx, d_rg, rg.data(), (size_t)nr * sizeof(R));
  if (rc) return rc;
  hipLaunchKernelGGL(k_range_bounds<Cols>, dim3((unsigned)((nr + FTPB - 1) / FTPB)), dim3(FTPB), 0, ctx->stream, c, n,
                     (const R*)d_rg, nr, *start, *coff);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

// The row filter the tablet server runs on the key (k_range_mask, gm_filter.hip): none, Z3Filter.inBounds on
// (bin, z) or Z2Filter.inBounds on z, with its descriptor words and the key columns it reads.
enum : int { RF_NONE = 0, RF_Z3 = 1, RF_Z2 = 2 };
struct RowFilter {
  int rf, nxy;
  const std::vector<int32_t>* words;
  const uint16_t* bin;
  const uint64_t* z;
};
// the full filter's own argument rules (gm_scan_filter): boxes with their envelope columns, during with t_ms
inline bool full_filter_ok(const gm_scan_filter* f) {
  const bool env = f->n_boxes > 0;
  return !(f->n_boxes < 0 || (env && (!f->boxes || !f->xmin || !f->ymin || !f->xmax || !f->ymax)) || (f->during != 0 && !f->t_ms));
}
// a scan without rows or ranges
inline int no_candidates(int64_t* n_match, int64_t* n_scanned, int64_t* n_envelope) {
  if (n_match) *n_match = 0;
  if (n_scanned) *n_scanned = 0;
  if (n_envelope) *n_envelope = 0;
  return GM_OK;
}
// after seek_ranges: the candidate count (*n_scanned), the mask pass over the candidates (row filter, full
// filter; with geom the exact refine, hq: the query polygons), the compaction, ids through perm.  Synchronises.
int scan_candidates(gm_ctx* ctx, DevTemps& tmp, const int64_t* start, int64_t* coff, int64_t nr,
                    const gm_scan_filter* f, const RowFilter& row_filter, const gm_geom_column* geom,
                    const polyq::HostQuery* hq, const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match,
                    int64_t* n_scanned, int64_t* n_envelope);

// JTS Envelope.intersects(Envelope): false for a null envelope (maxx < minx) on either side
__device__ __forceinline__ bool env_intersects(double ax0, double ay0, double ax1, double ay1, const double* q) {
  if (ax1 < ax0 || q[2] < q[0]) return false;
  return !(q[0] > ax1 || q[2] < ax0 || q[1] > ay1 || q[3] < ay0);
}

// The exact full filter of gm_table_scan_geom (geom_refine, gm_geom_filter.hip) over the survivors of the
// envelope pass: candidate surv[s] keeps its bit of `mask` iff its geometry slot meets one of the boxes --
// or, given query polygons, one of their parts; then the per-block counts are taken again from the mask, so
// finish_scan runs on it as on pass A's output.
struct GeomRefine {
  const int64_t* surv;                          // surviving candidate indices, ascending
  int64_t n_surv;
  const int64_t *coff, *start;                  // candidate -> table row (cand_row)
  int64_t nr, total;
  const int64_t* rows;                          // table row -> column row (null: the identity)
  const double *xmin, *ymin, *xmax, *ymax;      // the slots' JTS envelopes (column order)
  const double* boxes;                          // nbox x (xmin, ymin, xmax, ymax), device
  int nbox;
  uint64_t* mask;
  int32_t* counts;
};

// The query polygons of gm_scan_filter.polys on the device (gm_poly_query_host.hpp builds them): the ring
// edges bucketed by y-slab, each entry with its coordinates, its ring and its part * 2 + shell flag, and
// each part's first shell vertex.  The parts' envelopes are the boxes of the mask pass.
struct PolyQuery {
  const double* edge;              // entries x (ax, ay, bx, by), slab by slab, ring order within a slab
  const int32_t *ering, *epart;
  const int32_t* soff;             // ns + 1
  const double* pv0;               // n_parts x (x, y)
  int32_t n_parts, ns, entries;
  double x0, y0, x1, y1, inv_h;    // the envelope of every ring; slabs per unit of y
};
// the host images into `tmp`, one copy (synchronises the stream)
int upload_polys(gm_ctx* ctx, DevTemps& tmp, const polyq::HostQuery& h, PolyQuery& q);
// q null: against a.boxes; else against the query polygons (a.boxes, the parts' envelopes, are not read)
int geom_refine(gm_ctx* ctx, const gm_geom_column* geom, const GeomRefine& a, const PolyQuery* q);

}  // namespace gm
