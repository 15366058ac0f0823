// gm_filter.hip -- fused key-space / strict filter scans with wave-ballot compaction.
//
// Z3Filter.inBounds (idx/filters/Z3Filter.scala:26-62) is evaluated for every row of a columnar
// key store in one pass: 10 B/row (bin i16 + z i64) in, 1 bit/row out.  The Scala code runs it per
// row inside RowFilterIterator (geomesa-accumulo-iterators/.../RowFilterIterator.scala:52-66) or
// Z3HBaseFilter; here a wave of 64 rows produces one 64-bit ballot word.
//
// Output pipeline (all on the context stream, deterministic, ids ascending):
//   pass A  k_*_mask     : per-row predicate -> mask words + per-block match counts.  A kernel is its
//                          predicate: the ballots, the mask words and the block count are pair_scan's
//                          (columns: two rows per lane) or row_scan's (row keys, candidates) of gm_scan.hpp
//   pass B  launch_excl_scan (gm_scan.hpp): exclusive scan of the per-block counts
//   pass C  k_mask_to_ids: expand mask bits into row ids at the scanned offsets; read_i64: the match count
// Pass C reads n/8 bytes of mask, so the ids cost ~1/80 of pass A's traffic plus 8 B per match.
#include <string.h>

#include <algorithm>
#include <vector>

#include "gm_arrow.hpp"
#include "gm_scan.hpp"

namespace gm {

// ------------------------------------------------------------------ device filter descriptor
// flat int32 layout (built on the host from Z3Filter.serializeToBytes):
//   [0] nxy, [1] min_epoch, [2] max_epoch, [3] nt, [4] reserved
//   [5 .. 5+4*nxy)        xy boxes (xmin, ymin, xmax, ymax) in normalized cells
//   then nt (start, end) interval index pairs, (-1, -1) for a null epoch
//   then the intervals (t0, t1)
__device__ __forceinline__ bool z3_in_bounds_time(const int32_t* f, int16_t epoch, int64_t z);

// Z3Filter.pointInBounds && timeInBounds (Z3Filter.scala:31-62)
__device__ __forceinline__ bool z3_in_bounds(const int32_t* f, int16_t epoch, int64_t z) {
  const int nxy = f[0];
  const int32_t* xy = f + 5;
  const int32_t x = z3_combine(z), y = z3_combine(z >> 1);
  bool pin = false;
  for (int i = 0; i < nxy; ++i) {
    const int32_t* q = xy + 4 * i;
    if (x >= q[0] && x <= q[2] && y >= q[1] && y <= q[3]) { pin = true; break; }
  }
  if (!pin) return false;
  return z3_in_bounds_time(f, epoch, z);
}

// timeInBounds part of Z3Filter.inBounds (Z3Filter.scala:45-62)
__device__ __forceinline__ bool z3_in_bounds_time(const int32_t* f, int16_t epoch, int64_t z) {
  const int nxy = f[0];
  const int32_t* xy = f + 5;
  const int min_e = f[1], max_e = f[2];
  if (epoch > max_e || epoch < min_e) return true;   // whole epochs are left out (:46-47)
  const int nt = f[3];
  const int32_t* ep = xy + 4 * nxy;
  const int k = epoch - min_e;
  if (k >= nt) return true;
  const int a = ep[2 * k], b = ep[2 * k + 1];
  if (a < 0) return true;                             // null epoch -> true (:49)
  const int32_t* tiv = ep + 2 * nt;
  const int32_t t = z3_combine(z >> 2);
  for (int i = a; i < b; ++i)
    if (t >= tiv[2 * i] && t <= tiv[2 * i + 1]) return true;
  return false;
}

__device__ __forceinline__ bool bin_allowed(const int32_t* br, int nbr, int16_t b) {
  if (nbr == 0) return true;
  for (int i = 0; i < nbr; ++i)
    if (b >= br[2 * i] && b <= br[2 * i + 1]) return true;
  return false;
}

// Descriptor access.  Per-row reads of even wave-uniform descriptor words cost scalar loads plus
// loop and exec-mask bookkeeping, and decoding x and y with Z3.combine costs ~60 VALU per row
// (PMC: ~110 VALU per row, issue-bound at 45% of HBM).  The fast path (<= FBOX boxes,
// <= FBIN bin ranges: every bbox/during query) instead keeps the boxes as DILATED bounds in
// registers: spreading bits to every third position preserves order, so
//     lo <= Z3.combine(z) <= hi   <=>   dilate(lo) <= (z & X_BITS) <= dilate(hi)     (unsigned)
// (and likewise for y with the mask shifted by one).  A row then costs two ANDs and four 64-bit
// compares per box.  Bounds outside the 21-bit dimension are clamped on the host (an empty box gets
// lo > hi).  Only rows that pass bin + box read the per-epoch interval table (lane-varying, L1/L2).
constexpr int FBOX = 4, FBIN = 4;
constexpr uint64_t Z3_XBITS = 0x1249249249249249ull;   // Z3.combine's mask (Z3.scala:84)

// bin_allowed && Z3Filter.inBounds with dilated boxes and bin ranges in registers
__device__ __forceinline__ bool z3_row_fast(const uint64_t* bx, int nxy, const int32_t* br, int nbr,
                                            const int32_t* __restrict__ fdesc, int16_t b, int64_t z) {
  bool ba = nbr == 0;
#pragma unroll
  for (int i = 0; i < FBIN; ++i) {
    if (i >= nbr) break;
    ba |= (b >= br[2 * i]) & (b <= br[2 * i + 1]);
  }
  const uint64_t xv = (uint64_t)z & Z3_XBITS, yv = (uint64_t)z & (Z3_XBITS << 1);
  bool pin = false;
#pragma unroll
  for (int i = 0; i < FBOX; ++i) {
    if (i >= nxy) break;
    pin |= (xv >= bx[4 * i]) & (xv <= bx[4 * i + 1]) & (yv >= bx[4 * i + 2]) & (yv <= bx[4 * i + 3]);
  }
  if (!(ba && pin)) return false;
  return z3_in_bounds_time(fdesc, b, z);
}

// A pair of rows of a column of T, as its vector type V: one non-temporal load when the column is 16-B
// aligned (4-B for the bins), else the two rows' own loads.
template <bool VEC, class V, class T>
__device__ __forceinline__ V load_pair(const T* __restrict__ col, int64_t p) {
  if (VEC) return __builtin_nontemporal_load(&((const V*)col)[p]);
  return V{col[2 * p], col[2 * p + 1]};
}

// pass A for Z3Filter.  The generic path reads the descriptor straight from global memory with
// wave-uniform indices.
template <bool FAST, bool VEC>
__global__ __launch_bounds__(FTPB) void k_z3filter_mask_v(const int16_t* __restrict__ bin, const int64_t* __restrict__ z,
                                                          int64_t n, const uint64_t* __restrict__ dil,
                                                          const int32_t* __restrict__ fdesc,
                                                          const int32_t* __restrict__ bins, int nbr,
                                                          uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  sv2 bv[FPAIRS];
  lv2 zv[FPAIRS];
  const int nxy = fdesc[0];
  uint64_t bx[4 * FBOX];
  int32_t br[2 * FBIN];
#pragma unroll
  for (int i = 0; i < 4 * FBOX; ++i) bx[i] = (FAST && i < 4 * nxy) ? dil[i] : 0;
#pragma unroll
  for (int i = 0; i < 2 * FBIN; ++i) br[i] = (FAST && i < 2 * nbr) ? bins[i] : 0;
  auto pred = [&](int16_t b, int64_t z) {
    if (FAST) return z3_row_fast(bx, nxy, br, nbr, fdesc, b, z);
    return bin_allowed(bins, nbr, b) && z3_in_bounds(fdesc, b, z);
  };
  pair_scan(
      n, mask, block_counts,
      [&](int64_t p, int u) { bv[u] = load_pair<VEC, sv2>(bin, p); zv[u] = load_pair<VEC, lv2>(z, p); },
      [&](int u, int j) { return j ? pred(bv[u].y, zv[u].y) : pred(bv[u].x, zv[u].x); },
      [&](int64_t p) { return pred(bin[2 * p], z[2 * p]); });
}

__device__ __forceinline__ bool z2_in_xy(const int32_t* __restrict__ xy, int nxy, int64_t zz) {
  const int32_t x = z2_combine(zz), y = z2_combine(zz >> 1);
  for (int k = 0; k < nxy; ++k) {
    const int32_t* q = xy + 4 * k;
    if (x >= q[0] && x <= q[2] && y >= q[1] && y <= q[3]) return true;
  }
  return false;
}

// Z2: Z2.combine yields 32 bits (z bit 62 -> x bit 31, the sign bit of z -> y bit 31) compared as
// signed Ints, so the dilated form flips the dimension's top bit (signed -> unsigned order) on both
// sides: lo <= x  <=>  dilate(lo ^ 2^31) <= (z & X_BITS) ^ top.
constexpr uint64_t Z2_XBITS = 0x5555555555555555ull;

// Z2Filter.inBounds (idx/filters/Z2Filter.scala:20-35)
template <bool FAST, bool VEC>
__global__ __launch_bounds__(FTPB) void k_z2filter_mask_v(const int64_t* __restrict__ z, int64_t n,
                                                          const uint64_t* __restrict__ dil,
                                                          const int32_t* __restrict__ xy, int nxy,
                                                          uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  lv2 zv[FPAIRS];
  uint64_t bx[4 * FBOX];
#pragma unroll
  for (int i = 0; i < 4 * FBOX; ++i) bx[i] = (FAST && i < 4 * nxy) ? dil[i] : 0;
  auto pred = [&](int64_t zz) {
    if (!FAST) return z2_in_xy(xy, nxy, zz);
    const uint64_t xv = ((uint64_t)zz & Z2_XBITS) ^ (1ull << 62), yv = ((uint64_t)zz & (Z2_XBITS << 1)) ^ (1ull << 63);
    bool pin = false;
#pragma unroll
    for (int i = 0; i < FBOX; ++i) {
      if (i >= nxy) break;
      pin |= (xv >= bx[4 * i]) & (xv <= bx[4 * i + 1]) & (yv >= bx[4 * i + 2]) & (yv <= bx[4 * i + 3]);
    }
    return pin;
  };
  pair_scan(
      n, mask, block_counts, [&](int64_t p, int u) { zv[u] = load_pair<VEC, lv2>(z, p); },
      [&](int u, int j) { return pred(j ? zv[u].y : zv[u].x); },
      [&](int64_t p) { return pred(z[2 * p]); });
}

// strict: GeoTools BBOX on a point (inclusive) AND FastDuring (exclusive, ms).  Without 16-B aligned columns
// (VEC false) this scan keeps a lane per row: it streams 24 B a row and has no boxes to hold in registers,
// and the pair layout's two 8-B loads per lane, 16 B apart, measured 3.80-3.91 ms per 1B rows against the
// 3.34-3.60 of contiguous 8-B loads (profiles/scan_skeleton_ab.txt).
template <bool DURING, bool VEC>
__global__ __launch_bounds__(FTPB) void k_strict_mask_v(const double* __restrict__ x, const double* __restrict__ y,
                                                        const int64_t* __restrict__ t, int64_t n, double bx0, double by0,
                                                        double bx1, double by1, int64_t lo, int64_t hi,
                                                        uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  auto pred = [&](double px, double py, int64_t tt) {
    bool ok = px >= bx0 && px <= bx1 && py >= by0 && py <= by1;
    if (DURING) ok = ok && tt > lo && tt < hi;
    return ok;
  };
  if constexpr (!VEC) {
    row_scan<4>(n, mask, block_counts, [&](int64_t i) { return pred(x[i], y[i], DURING ? t[i] : 0); });
  } else {
    dv2 xv[FPAIRS], yv[FPAIRS];
    lv2 tv[FPAIRS];
    pair_scan(
        n, mask, block_counts,
        [&](int64_t p, int u) {
          xv[u] = load_pair<true, dv2>(x, p);
          yv[u] = load_pair<true, dv2>(y, p);
          if (DURING) tv[u] = load_pair<true, lv2>(t, p);
          else tv[u] = lv2{0, 0};
        },
        [&](int u, int j) { return j ? pred(xv[u].y, yv[u].y, tv[u].y) : pred(xv[u].x, yv[u].x, tv[u].x); },
        [&](int64_t p) { return pred(x[2 * p], y[2 * p], DURING ? t[2 * p] : 0); });
  }
}

// pass C: one block per pass-A block; per (step, wave) popcount prefix gives each lane its slot
__global__ __launch_bounds__(FTPB) void k_mask_to_ids(const uint64_t* __restrict__ mask, int64_t n,
                                                      const int64_t* __restrict__ offsets, int64_t* __restrict__ ids,
                                                      int64_t cap) {
  __shared__ int32_t s_pre[FELEMS * (FTPB / 64)];
  const int64_t base = (int64_t)blockIdx.x * FROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NW = FTPB / 64;
  if (threadIdx.x < FELEMS * NW) {
    const int u = threadIdx.x / NW, w = threadIdx.x % NW;
    const int64_t word = (base + (int64_t)u * FTPB + w * 64) >> 6;
    s_pre[threadIdx.x] = ((word << 6) < n) ? __popcll(mask[word]) : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < FELEMS * NW; ++k) { int c = s_pre[k]; s_pre[k] = run; run += c; }
  }
  __syncthreads();
  const int64_t blk_off = offsets[blockIdx.x];
  for (int u = 0; u < FELEMS; ++u) {
    const int64_t word = (base + (int64_t)u * FTPB + wave * 64) >> 6;
    if ((word << 6) >= n) break;
    const uint64_t w = mask[word];
    if ((w >> lane) & 1ull) {
      const int before = __popcll(w & ((1ull << lane) - 1ull));
      const int64_t slot = blk_off + s_pre[u * NW + wave] + before;
      if (slot < cap) ids[slot] = (word << 6) + lane;
    }
  }
}

// ------------------------------------------------------------------ row-key bytes (RowFilter.inBounds)
// RowFilterIterator.findTop calls filter.inBounds(row bytes, offset) once per row
// (geomesa-accumulo-iterators/.../RowFilterIterator.scala:52-66).  Here row i is
// rows[row_off[i] .. row_off[i+1]): the key is read from aligned dwords covering its bytes (a dword
// holding at least one byte of the row never crosses a page) and byte-swapped from big-endian
// (ByteArrays.readShort / readLong).  A row too short for its key is a non-match counted in
// *short_rows (the JVM read would throw ArrayIndexOutOfBoundsException).
template <int KEYLEN>
__device__ __forceinline__ bool row_key(const uint8_t* __restrict__ rows, const int64_t* __restrict__ row_off,
                                        int64_t i, int key_offset, int16_t& epoch, int64_t& z) {
  const int64_t a = row_off[i], len = row_off[i + 1] - a;
  if (len < (int64_t)key_offset + KEYLEN) return false;
  const uintptr_t p = (uintptr_t)(rows + a + key_offset);
  const uint32_t* w = (const uint32_t*)(p & ~(uintptr_t)3);
  const int sh = (int)(p & 3);
  const uint32_t w0 = w[0], w1 = w[1];
  const uint32_t w2 = (KEYLEN == 10 || sh > 0) ? w[2] : 0u;
  const uint32_t w3 = (KEYLEN == 10 && sh == 3) ? w[3] : 0u;
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
  const uint64_t k0 = sh ? (lo >> (8 * sh)) | (hi << (64 - 8 * sh)) : lo;   // key bytes 0..7, little-endian
  if (KEYLEN == 8) {
    z = (int64_t)__builtin_bswap64(k0);
    epoch = 0;
  } else {
    const uint64_t k1 = hi >> (8 * sh);                                      // key bytes 8..
    epoch = (int16_t)(uint16_t)(((k0 & 0xffu) << 8) | ((k0 >> 8) & 0xffu));
    z = (int64_t)__builtin_bswap64((k0 >> 16) | (k1 << 48));
  }
  return true;
}

template <bool Z3>
__global__ __launch_bounds__(FTPB) void k_filter_rows_mask(const uint8_t* __restrict__ rows,
                                                           const int64_t* __restrict__ row_off, int key_offset,
                                                           int64_t n, const int32_t* __restrict__ fdesc, int fwords,
                                                           uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts,
                                                           unsigned long long* __restrict__ short_rows) {
  extern __shared__ int32_t s_f[];
  for (int i = threadIdx.x; i < fwords; i += FTPB) s_f[i] = fdesc[i];
  __syncthreads();
  int nshort = 0;
  row_scan(n, mask, block_counts, [&](int64_t i) {
    int16_t e;
    int64_t zz;
    if (row_key<Z3 ? 10 : 8>(rows, row_off, i, key_offset, e, zz))
      return Z3 ? z3_in_bounds(s_f, e, zz) : z2_in_xy(s_f, fwords / 4, zz);   // Z3Filter.scala:26-28 / Z2Filter
    ++nshort;
    return false;
  });
  if (nshort && short_rows) atomicAdd(short_rows, (unsigned long long)nshort);
}

// ------------------------------------------------------------------ range scan of a sorted table
// gm_key_range_scan: the seek-and-filter loop of a Z3 query against a table sorted by gm_sort_keys.
// Each range [lo, hi] of the (shard, bin, z) key prefix (getRangeBytes, Z3IndexKeySpace.scala:196-238)
// maps to a row interval by two binary searches; the intervals' rows are the candidates
// (Accumulo/HBase scan), and Z3Filter.inBounds runs on each (RowFilterIterator.scala:52-66) in the
// same mask -> block scan -> ordered compaction pipeline as the full scans.
// The Z tables' key: (shard << 16 | (uint16) bin, z), the byte order of [shard][bin BE16][z BE64].  The seek
// itself (k_range_bounds, merge_ranges, seek_ranges) is gm_scan.hpp's, shared with the attribute table.
struct ZKey {
  uint64_t z;
  uint32_t kb;   // shard << 16 | (uint16) bin
  __host__ __device__ static bool lt(const ZKey& a, const ZKey& b) { return a.kb < b.kb || (a.kb == b.kb && a.z < b.z); }
  static bool next(const ZKey& k, ZKey* out) {
    *out = ZKey{k.z + 1, k.z == ~0ull ? k.kb + 1 : k.kb};
    return !(k.z == ~0ull && k.kb == ~0u);
  }
};
// bin = null: a key space without a time bin (Z2 / XZ2: [shard][z BE64]), every row's bin reads as 0
struct ZCols {
  using Key = ZKey;
  const uint8_t* sh;
  const uint16_t* bin;
  const uint64_t* z;
  __device__ __forceinline__ ZKey at(int64_t i) const {
    return ZKey{z[i], ((uint32_t)(sh ? sh[i] : 0) << 16) | (bin ? bin[i] : 0u)};
  }
};

// in-place exclusive scan of int64 lengths (one block); total -> a[len]
__global__ __launch_bounds__(1024) void k_scan_i64(int64_t* __restrict__ a, int64_t len) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (len + 1023) / 1024, lo = t * per, hi = min(len, lo + per);
  int64_t s = 0;
  for (int64_t k = lo; k < hi; ++k) s += a[k];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t k = lo; k < hi; ++k) { const int64_t c = a[k]; a[k] = run; run += c; }
  if (t == 1023) a[len] = part[1023];
}

// candidate-space mask: candidate c = the c-th row inside the (disjoint, sorted) intervals.  RF: the row
// filter the tablet server runs on the key (RowFilterIterator.scala:52-66): none, Z3Filter.inBounds on
// (bin, z) (Z3Filter.scala:26-62) or Z2Filter.inBounds on z (Z2Filter.scala:20-35).  ENV / DUR: the full
// filter on the feature (the XZ key spaces' useFullFilter = true, XZ2IndexKeySpace.scala:122-125,
// XZ3IndexKeySpace.scala:247-250) over the caller's feature columns, reached through `rows` (table row ->
// column row; not the id map k_cand_to_row applies): JTS Envelope.intersects with any query box
// (inclusive), and FastDuring (exclusive, ms) on the dtg.
struct FullFilter {
  const double *xmin, *ymin, *xmax, *ymax;   // feature envelopes (column order)
  const int64_t* t;                           // feature dtg (column order)
  const double* boxes;                        // nbox x (xmin, ymin, xmax, ymax), device
  int nbox;
  int64_t t_lo, t_hi;
  const int64_t* rows;                        // table row -> column row (null: the identity)
};
template <int RF, bool ENV, bool DUR>
__global__ __launch_bounds__(FTPB) void k_range_mask(const uint16_t* __restrict__ bin, const uint64_t* __restrict__ z,
                                                     const int64_t* __restrict__ coff, const int64_t* __restrict__ start,
                                                     int64_t nr, int64_t total, const int32_t* __restrict__ fdesc, int nxy,
                                                     FullFilter ff, uint64_t* __restrict__ mask,
                                                     int32_t* __restrict__ block_counts) {
  row_scan(total, mask, block_counts, [&](int64_t c) {
    bool ok = true;
    if (RF != RF_NONE || ENV || DUR) {
      const int64_t row = cand_row(coff, start, nr, c);
      if (RF == RF_Z3) ok = z3_in_bounds(fdesc, (int16_t)bin[row], (int64_t)z[row]);
      if (RF == RF_Z2) ok = z2_in_xy(fdesc, nxy, (int64_t)z[row]);
      if ((ENV || DUR) && ok) {
        const int64_t r = ff.rows ? ff.rows[row] : row;
        if (DUR) {
          const int64_t t = ff.t[r];
          ok = t > ff.t_lo && t < ff.t_hi;
        }
        if (ENV && ok) {
          const double x0 = ff.xmin[r], y0 = ff.ymin[r], x1 = ff.xmax[r], y1 = ff.ymax[r];
          bool in = false;
          for (int k = 0; k < ff.nbox && !in; ++k) in = env_intersects(x0, y0, x1, y1, ff.boxes + 4 * k);
          ok = in;
        }
      }
    }
    return ok;
  });
}

// compacted candidate indices -> table rows (-> input rows through perm)
__global__ __launch_bounds__(FTPB) void k_cand_to_row(int64_t* __restrict__ ids, int64_t m,
                                                      const int64_t* __restrict__ coff, const int64_t* __restrict__ start,
                                                      int64_t nr, const int64_t* __restrict__ perm) {
  for (int64_t j = (int64_t)blockIdx.x * FTPB + threadIdx.x; j < m; j += (int64_t)gridDim.x * FTPB) {
    const int64_t row = cand_row(coff, start, nr, ids[j]);
    ids[j] = perm ? perm[row] : row;
  }
}

// ------------------------------------------------------------------ host side

static inline int32_t be32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]);
}
static inline int16_t be16(const uint8_t* p) { return (int16_t)(uint16_t)((uint16_t)p[0] << 8 | p[1]); }

// bit spread with `stride` (2 or 3), the host mirror of Z2.split / Z3.split without masking
static uint64_t dilate(uint64_t v, int bits, int stride) {
  uint64_t o = 0;
  for (int i = 0; i < bits; ++i) o |= ((v >> i) & 1ull) << (stride * i);
  return o;
}

// Z3 boxes (xmin, ymin, xmax, ymax) as dilated (xlo, xhi, ylo, yhi); dims are 21-bit, non-negative
static void z3_dilated_boxes(const int32_t* xy, int nxy, std::vector<uint64_t>& out) {
  out.clear();
  const int64_t top = (1 << 21) - 1;
  for (int i = 0; i < nxy; ++i) {
    for (int d = 0; d < 2; ++d) {
      const int64_t lo = std::max<int64_t>(xy[4 * i + d], 0), hi = std::min<int64_t>(xy[4 * i + 2 + d], top);
      if (lo > hi || lo > top || hi < 0) { out.push_back(1ull << 63); out.push_back(0); continue; }   // empty
      out.push_back(dilate((uint64_t)lo, 21, 3) << d);
      out.push_back(dilate((uint64_t)hi, 21, 3) << d);
    }
  }
}

// Z2 boxes: signed 32-bit dims, top bit flipped into unsigned order
static void z2_dilated_boxes(const int32_t* xy, int nxy, std::vector<uint64_t>& out) {
  out.clear();
  for (int i = 0; i < nxy; ++i) {
    for (int d = 0; d < 2; ++d) {
      const int32_t lo = xy[4 * i + d], hi = xy[4 * i + 2 + d];
      if (lo > hi) { out.push_back(~0ull); out.push_back(0); continue; }   // empty
      out.push_back(dilate((uint32_t)lo ^ 0x80000000u, 32, 2) << d);
      out.push_back(dilate((uint32_t)hi ^ 0x80000000u, 32, 2) << d);
    }
  }
}

// Z3Filter.deserializeFromBytes (Z3Filter.scala:139-153) -> flat descriptor
static bool build_z3_desc(const uint8_t* b, size_t len, std::vector<int32_t>& d) {
  size_t o = 0;
  auto need = [&](size_t k) { return o + k <= len; };
  if (!need(4)) return false;
  const int32_t nxy = be32(b + o); o += 4;
  if (nxy < 0 || !need((size_t)nxy * 16)) return false;
  std::vector<int32_t> xy((size_t)nxy * 4);
  for (size_t i = 0; i < xy.size(); ++i) { xy[i] = be32(b + o); o += 4; }
  if (!need(4)) return false;
  const int32_t nt = be32(b + o); o += 4;
  if (nt < 0) return false;
  std::vector<int32_t> ep((size_t)nt * 2, 0), tiv;
  for (int k = 0; k < nt; ++k) {
    if (!need(4)) return false;
    const int32_t l = be32(b + o); o += 4;
    if (l == -1) { ep[2 * k] = -1; ep[2 * k + 1] = -1; continue; }   // null epoch: whole period
    if (l < 0 || !need((size_t)l * 8)) return false;
    ep[2 * k] = (int32_t)(tiv.size() / 2);
    for (int i = 0; i < 2 * l; ++i) { tiv.push_back(be32(b + o)); o += 4; }
    ep[2 * k + 1] = (int32_t)(tiv.size() / 2);
  }
  if (!need(4)) return false;
  const int16_t min_e = be16(b + o), max_e = be16(b + o + 2);
  d.clear();
  d.push_back(nxy);
  d.push_back(min_e);
  d.push_back(max_e);
  d.push_back(nt);
  d.push_back(0);
  d.insert(d.end(), xy.begin(), xy.end());
  d.insert(d.end(), ep.begin(), ep.end());
  d.insert(d.end(), tiv.begin(), tiv.end());
  return true;
}

// Z2Filter's bytes (a count, then xmin, ymin, xmax, ymax per box, big-endian) -> the boxes' 4 nxy words
static bool build_z2_desc(const uint8_t* b, size_t len, std::vector<int32_t>& xy) {
  if (len < 4) return false;
  const int32_t nxy = be32(b);
  if (nxy < 0 || 4 + (size_t)nxy * 16 > len) return false;
  xy.resize((size_t)nxy * 4);
  for (size_t i = 0; i < xy.size(); ++i) xy[i] = be32(b + 4 + 4 * i);
  return true;
}

// a scan's descriptor, from pageable host memory to b.desc: the copy is waited for
static int upload_desc(gm_ctx* ctx, const ScanBufs& b, const int32_t* words, size_t count) {
  GM_HIP(hipMemcpyAsync(b.desc, words, count * 4, hipMemcpyHostToDevice, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

}  // namespace gm

using namespace gm;

namespace gm {

// scratch buffers per call, carved from the context's scan workspace (stream-ordered reuse)
int alloc_scan(gm_ctx* ctx, int64_t n, uint64_t* user_mask, size_t desc_words, ScanBufs& b) {
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  const int64_t nwords = nblocks * (FROWS / 64);
  Carve c{16};
  const size_t o_mask = c.take(user_mask ? 0 : (size_t)nwords * 8);   // whole 512-B blocks: no rounding
  const size_t o_cnt = c.take((size_t)nblocks * 4 + 4);
  const size_t o_off = c.take((size_t)(nblocks + 1) * 8);
  const size_t o_part = c.take((size_t)(nblocks / SCAN_CHUNK + 2) * 8);
  const size_t o_desc = c.take(desc_words * 4);
  char* base = nullptr;
  int rc = ctx_workspace(ctx, WS_SCAN, c.total + 16, (void**)&base);
  if (rc) return rc;
  b.mask = user_mask ? user_mask : (uint64_t*)(base + o_mask);
  b.counts = (int32_t*)(base + o_cnt);
  b.offsets = (int64_t*)(base + o_off);
  b.partials = (int64_t*)(base + o_part);
  b.desc = desc_words ? (int32_t*)(base + o_desc) : nullptr;
  return GM_OK;
}

int CountScan::scan(gm_ctx* ctx) {
  launch_excl_scan(ctx->stream, (const int32_t*)counts, nb, offsets, partials, offsets + nb);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

// passes B and C + count readback
int finish_scan(gm_ctx* ctx, int64_t n, ScanBufs& b, int64_t* ids, int64_t ids_cap, int64_t* n_match) {
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  if (ids || n_match) {
    launch_excl_scan(ctx->stream, b.counts, nblocks, b.offsets, b.partials, b.offsets + nblocks);
    GM_CHECK_LAUNCH();
  }
  if (ids) {
    hipLaunchKernelGGL(k_mask_to_ids, dim3((unsigned)nblocks), dim3(FTPB), 0, ctx->stream, b.mask, n, b.offsets, ids,
                       ids_cap);
    GM_CHECK_LAUNCH();
  }
  return n_match ? read_i64(ctx, b.offsets + nblocks, n_match) : GM_OK;
}

}  // namespace gm

extern "C" {

int gm_z3filter_scan(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const int16_t* bin_ranges,
                     int n_bin_ranges, const int16_t* bin, const int64_t* z, int64_t n, uint64_t* mask,
                     int64_t* ids, int64_t ids_cap, int64_t* n_match) {
  if (!ctx || !filter_bytes || n < 0 || n_bin_ranges < 0 || (ids && ids_cap < 0)) return GM_E_INVALID;
  std::vector<int32_t> desc;
  if (!build_z3_desc(filter_bytes, filter_len, desc)) {
    set_error("gm_z3filter_scan: malformed Z3Filter bytes");
    return GM_E_INVALID;
  }
  if (n == 0) { if (n_match) *n_match = 0; return GM_OK; }
  if (!bin || !z) return GM_E_INVALID;
  const int fwords = (int)desc.size();
  for (int i = 0; i < n_bin_ranges; ++i) { desc.push_back(bin_ranges[2 * i]); desc.push_back(bin_ranges[2 * i + 1]); }
  // device layout: [dilated boxes u64 x 4 nxy][descriptor][bin ranges]
  std::vector<uint64_t> dil;
  z3_dilated_boxes(desc.data() + 5, desc[0], dil);
  std::vector<int32_t> buf(2 * dil.size() + desc.size());
  if (!dil.empty()) memcpy(buf.data(), dil.data(), dil.size() * 8);
  memcpy(buf.data() + 2 * dil.size(), desc.data(), desc.size() * 4);
  ScanBufs b;
  int rc = alloc_scan(ctx, n, mask, buf.size(), b);
  if (rc) return rc;
  if ((rc = upload_desc(ctx, b, buf.data(), buf.size()))) return rc;
  const uint64_t* d_dil = (const uint64_t*)b.desc;
  const int32_t* d_desc = b.desc + 2 * dil.size();
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  with_flags([&](auto FAST, auto VEC) {
    hipLaunchKernelGGL((k_z3filter_mask_v<FAST(), VEC()>), dim3((unsigned)nblocks), dim3(FTPB), 0, ctx->stream, bin, z,
                       n, d_dil, d_desc, d_desc + fwords, n_bin_ranges, b.mask, b.counts);
  }, desc[0] <= FBOX && n_bin_ranges <= FBIN, aligned16(bin) && aligned16(z));
  GM_CHECK_LAUNCH();
  return end_scan(ctx, n, b, ids, ids_cap, n_match);
}

int gm_z2filter_scan(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const int64_t* z, int64_t n,
                     uint64_t* mask, int64_t* ids, int64_t ids_cap, int64_t* n_match) {
  if (!ctx || !filter_bytes || n < 0 || filter_len < 4 || (ids && ids_cap < 0)) return GM_E_INVALID;
  std::vector<int32_t> xy;
  if (!build_z2_desc(filter_bytes, filter_len, xy)) {
    set_error("gm_z2filter_scan: malformed Z2Filter bytes");
    return GM_E_INVALID;
  }
  if (n == 0) { if (n_match) *n_match = 0; return GM_OK; }
  if (!z) return GM_E_INVALID;
  const int nxy = (int)(xy.size() / 4);
  // device layout: [dilated boxes u64 x 4 nxy][boxes int32 x 4 nxy]
  std::vector<uint64_t> dil;
  z2_dilated_boxes(xy.data(), nxy, dil);
  std::vector<int32_t> buf(2 * dil.size() + xy.size() + 1);
  if (!dil.empty()) memcpy(buf.data(), dil.data(), dil.size() * 8);
  if (!xy.empty()) memcpy(buf.data() + 2 * dil.size(), xy.data(), xy.size() * 4);
  ScanBufs b;
  int rc = alloc_scan(ctx, n, mask, buf.size(), b);
  if (rc) return rc;
  if ((rc = upload_desc(ctx, b, buf.data(), buf.size()))) return rc;
  const uint64_t* d_dil = (const uint64_t*)b.desc;
  const int32_t* d_xy = b.desc + 2 * dil.size();
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  with_flags([&](auto FAST, auto VEC) {
    hipLaunchKernelGGL((k_z2filter_mask_v<FAST(), VEC()>), dim3((unsigned)nblocks), dim3(FTPB), 0, ctx->stream, z, n,
                       d_dil, d_xy, nxy, b.mask, b.counts);
  }, nxy <= FBOX, aligned16(z));
  GM_CHECK_LAUNCH();
  return end_scan(ctx, n, b, ids, ids_cap, n_match);
}

// shared driver of gm_z3filter_scan_rows / gm_z2filter_scan_rows
static int filter_rows(gm_ctx* ctx, bool z3, const std::vector<int32_t>& desc, const uint8_t* rows,
                       const int64_t* row_off, int key_offset, int64_t n, uint64_t* mask, int64_t* ids,
                       int64_t ids_cap, int64_t* n_match, int64_t* n_short) {
  if (n == 0) { if (n_match) *n_match = 0; if (n_short) *n_short = 0; return GM_OK; }
  if (!rows || !row_off || key_offset < 0) return GM_E_INVALID;
  ScanBufs b;
  // descriptor words, then one 8-B short-row counter (16-B aligned)
  const size_t dw = (desc.size() + 3) & ~(size_t)3;
  int rc = alloc_scan(ctx, n, mask, dw + 4, b);
  if (rc) return rc;
  unsigned long long* d_short = (unsigned long long*)(b.desc + dw);
  GM_HIP(hipMemsetAsync(d_short, 0, 8, ctx->stream));
  if ((rc = upload_desc(ctx, b, desc.data(), desc.size()))) return rc;
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  const size_t lds = std::max<size_t>(desc.size() * 4, 4);
  with_flags([&](auto Z3) {
    hipLaunchKernelGGL(k_filter_rows_mask<Z3()>, dim3((unsigned)nblocks), dim3(FTPB), lds, ctx->stream, rows, row_off,
                       key_offset, n, b.desc, (int)desc.size(), b.mask, b.counts, d_short);
  }, z3);
  GM_CHECK_LAUNCH();
  // the short-row count is read back before the capacity is answered
  return end_scan(ctx, n, b, ids, ids_cap, n_match,
                  [&]() -> int { return n_short ? read_i64(ctx, d_short, n_short) : GM_OK; });
}

int gm_z3filter_scan_rows(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const uint8_t* rows,
                          const int64_t* row_off, int key_offset, int64_t n, uint64_t* mask, int64_t* ids,
                          int64_t ids_cap, int64_t* n_match, int64_t* n_short) {
  if (!ctx || !filter_bytes || n < 0 || (ids && ids_cap < 0)) return GM_E_INVALID;
  std::vector<int32_t> desc;
  if (!build_z3_desc(filter_bytes, filter_len, desc)) {
    set_error("gm_z3filter_scan_rows: malformed Z3Filter bytes");
    return GM_E_INVALID;
  }
  return filter_rows(ctx, true, desc, rows, row_off, key_offset, n, mask, ids, ids_cap, n_match, n_short);
}

int gm_z2filter_scan_rows(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const uint8_t* rows,
                          const int64_t* row_off, int key_offset, int64_t n, uint64_t* mask, int64_t* ids,
                          int64_t ids_cap, int64_t* n_match, int64_t* n_short) {
  if (!ctx || !filter_bytes || n < 0 || filter_len < 4 || (ids && ids_cap < 0)) return GM_E_INVALID;
  std::vector<int32_t> xy;
  if (!build_z2_desc(filter_bytes, filter_len, xy)) {
    set_error("gm_z2filter_scan_rows: malformed Z2Filter bytes");
    return GM_E_INVALID;
  }
  return filter_rows(ctx, false, xy, rows, row_off, key_offset, n, mask, ids, ids_cap, n_match, n_short);
}

int gm_strict_scan(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n, const double* bbox,
                   int has_during, int64_t lo, int64_t hi, uint64_t* mask, int64_t* ids, int64_t ids_cap,
                   int64_t* n_match) {
  if (!ctx || !bbox || n < 0 || (ids && ids_cap < 0)) return GM_E_INVALID;
  if (n == 0) { if (n_match) *n_match = 0; return GM_OK; }
  if (!x || !y || (has_during && !t_ms)) return GM_E_INVALID;
  ScanBufs b;
  int rc = alloc_scan(ctx, n, mask, 0, b);
  if (rc) return rc;
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  const bool vec = aligned16(x) && aligned16(y) && (!has_during || aligned16(t_ms));
  with_flags([&](auto D, auto VEC) {
    hipLaunchKernelGGL((k_strict_mask_v<D(), VEC()>), dim3((unsigned)nblocks), dim3(FTPB), 0, ctx->stream, x, y, t_ms,
                       n, bbox[0], bbox[1], bbox[2], bbox[3], lo, hi, b.mask, b.counts);
  }, has_during != 0, vec);
  GM_CHECK_LAUNCH();
  return end_scan(ctx, n, b, ids, ids_cap, n_match);
}

}  // extern "C"

// gm_table_scan and gm_table_scan_geom: the seek, the mask pass and the compaction.  geom = NULL is
// gm_table_scan, launch for launch; with geom the survivors of the envelope pass are compacted as
// candidate indices, refined against their geometries (geom_refine; against the query polygons when the
// filter carries them, whose parts' envelopes then stand in for the boxes) and the mask is compacted again.
static int table_scan(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                      const gm_key_range* ranges, int64_t n_ranges, const gm_scan_filter* f,
                      const gm_geom_column* geom, const int64_t* perm, int64_t* ids, int64_t ids_cap,
                      int64_t* n_match, int64_t* n_scanned, int64_t* n_envelope) {
  const std::string who = geom ? "gm_table_scan_geom" : "gm_table_scan";   // the entry the error texts name
  if (!ctx || n < 0 || n_ranges < 0 || (n_ranges > 0 && !ranges) || ids_cap < 0) return GM_E_INVALID;
  if (n > 0 && !z) return GM_E_INVALID;
  gm_scan_filter none{};
  if (!f) f = &none;
  if (f->z3filter && f->z2filter) return set_error(who + ": a Z3Filter and a Z2Filter together"), GM_E_INVALID;
  if (f->z3filter && !bin) return set_error(who + ": a Z3Filter needs the bin column"), GM_E_INVALID;
  // query polygons: the prefilter's boxes are the parts' envelopes, derived here
  polyq::HostQuery hq;
  gm_scan_filter with_boxes;
  const bool polys = f->polys != nullptr;
  if (polys) {
    if (!geom) return set_error(who + ": polys needs the geometry column (gm_table_scan_geom)"), GM_E_INVALID;
    if (f->boxes || f->n_boxes != 0) return set_error(who + ": polys and boxes together"), GM_E_INVALID;
    if (const char* bad = polyq::validate(f->polys)) return set_error(who + ": " + bad), GM_E_INVALID;
    polyq::build(f->polys, hq);
    with_boxes = *f;
    with_boxes.boxes = hq.penv.data();
    with_boxes.n_boxes = hq.n_parts;
    f = &with_boxes;
  }
  if (!full_filter_ok(f)) return GM_E_INVALID;
  // the row filter's descriptor: Z3Filter.deserializeFromBytes or Z2Filter's boxes
  std::vector<int32_t> desc;
  int rf = RF_NONE, nxy = 0;
  if (f->z3filter) {
    if (!build_z3_desc(f->z3filter, f->z3filter_len, desc)) {
      set_error(who + ": malformed Z3Filter bytes");
      return GM_E_INVALID;
    }
    rf = RF_Z3;
  } else if (f->z2filter) {
    if (f->z2filter_len < 4) return GM_E_INVALID;
    if (!build_z2_desc(f->z2filter, f->z2filter_len, desc)) {
      set_error(who + ": malformed Z2Filter bytes");
      return GM_E_INVALID;
    }
    nxy = (int)(desc.size() / 4);
    rf = RF_Z2;
  }
  // the BatchScanner's view of the ranges: sorted, overlapping / adjacent ones merged
  std::vector<SeekRange<ZKey>> rs;
  rs.reserve((size_t)n_ranges);
  for (int64_t i = 0; i < n_ranges; ++i) {
    const gm_key_range& r = ranges[i];
    rs.push_back(SeekRange<ZKey>{ZKey{(uint64_t)r.z_lo, ((uint32_t)r.shard << 16) | (uint16_t)r.bin_lo},
                                 ZKey{(uint64_t)r.z_hi, ((uint32_t)r.shard << 16) | (uint16_t)r.bin_hi}});
  }
  const std::vector<SeekRange<ZKey>> dr = merge_ranges(std::move(rs));
  const int64_t nr = (int64_t)dr.size();
  if (n == 0 || nr == 0) return no_candidates(n_match, n_scanned, n_envelope);
  DevTemps tmp(ctx->stream);
  int64_t *start = nullptr, *coff = nullptr;
  const int rc = seek_ranges(ctx, tmp, ZCols{shard, (const uint16_t*)bin, (const uint64_t*)z}, n, dr, &start, &coff);
  if (rc) return rc;
  const RowFilter row_filter{rf, nxy, &desc, (const uint16_t*)bin, (const uint64_t*)z};
  return scan_candidates(ctx, tmp, start, coff, nr, f, row_filter, geom, polys ? &hq : nullptr, perm, ids, ids_cap,
                         n_match, n_scanned, n_envelope);
}

namespace gm {

// The candidates of the seek's row intervals (start, and their lengths in coff) through the mask pass and
// the compaction: what gm_table_scan, gm_table_scan_geom and gm_attr_table_scan share after their own seek.
int scan_candidates(gm_ctx* ctx, DevTemps& tmp, const int64_t* start, int64_t* coff, int64_t nr,
                    const gm_scan_filter* f, const RowFilter& row_filter, const gm_geom_column* geom,
                    const polyq::HostQuery* hq, const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match,
                    int64_t* n_scanned, int64_t* n_envelope) {
  hipStream_t s = ctx->stream;
  const bool env = f->n_boxes > 0, dur = f->during != 0, polys = hq != nullptr;
  const std::vector<int32_t>& desc = *row_filter.words;
  const uint16_t* bin = row_filter.bin;
  const uint64_t* z = row_filter.z;
  const int rf = row_filter.rf, nxy = row_filter.nxy;
  int rc = GM_OK;
  hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, s, coff, nr);
  GM_CHECK_LAUNCH();
  int64_t total = 0;   // the candidate count sizes the pass below (and the ranges are pageable: the wait covers their copy)
  if ((rc = read_i64(ctx, coff + nr, &total))) return rc;
  if (n_scanned) *n_scanned = total;
  int64_t nm = 0, ne = 0;
  if (total > 0) {
    // device descriptor: [query boxes f64 x 4 nbox][row-filter words]
    const size_t box_words = env ? (size_t)f->n_boxes * 8 : 0;
    std::vector<int32_t> buf(box_words + desc.size());
    if (env) memcpy(buf.data(), f->boxes, (size_t)f->n_boxes * 32);
    if (!desc.empty()) memcpy(buf.data() + box_words, desc.data(), desc.size() * 4);
    ScanBufs b;
    rc = alloc_scan(ctx, total, nullptr, buf.size() + 4, b);
    if (rc) return rc;
    if (!buf.empty() && (rc = upload_desc(ctx, b, buf.data(), buf.size()))) return rc;
    FullFilter ff{f->xmin, f->ymin, f->xmax, f->ymax, f->t_ms, env ? (const double*)b.desc : nullptr, f->n_boxes,
                  f->t_lo, f->t_hi, f->rows ? f->rows : perm};
    const int32_t* d_desc = b.desc + box_words;
    const int64_t nblocks = (total + FROWS - 1) / FROWS;
    with_value<RF_Z3, RF_Z2, RF_NONE>(rf, [&](auto RF) {
      with_flags([&](auto ENV, auto DUR) {
        hipLaunchKernelGGL((k_range_mask<RF(), ENV(), DUR()>), dim3((unsigned)nblocks), dim3(FTPB), 0, s,
                           (const uint16_t*)bin, (const uint64_t*)z, coff, start, nr, total, d_desc, nxy, ff, b.mask,
                           b.counts);
      }, env, dur);
    });
    GM_CHECK_LAUNCH();
    if (geom) {
      // the envelope pass's survivors as candidate indices, then the exact test clears the failing bits
      if ((rc = finish_scan(ctx, total, b, nullptr, 0, &ne))) return rc;
      int64_t* surv = nullptr;
      if (ne > 0) {
        if ((rc = tmp.alloc_async((size_t)ne * 8, &surv))) return rc;
        hipLaunchKernelGGL(k_mask_to_ids, dim3((unsigned)nblocks), dim3(FTPB), 0, s, b.mask, total, b.offsets, surv, ne);
        GM_CHECK_LAUNCH();
        const GeomRefine gr{surv, ne, coff, start, nr, total, ff.rows, f->xmin, f->ymin, f->xmax, f->ymax, ff.boxes,
                            f->n_boxes, b.mask, b.counts};
        PolyQuery pq;
        if (polys && (rc = upload_polys(ctx, tmp, *hq, pq))) return rc;
        if ((rc = geom_refine(ctx, geom, gr, polys ? &pq : nullptr))) return rc;
      }
    }
    rc = (geom && ne == 0) ? GM_OK : finish_scan(ctx, total, b, ids, ids_cap, &nm);
    if (rc) return rc;
    const int64_t m = std::min(nm, ids_cap);
    if (ids && m > 0) {
      hipLaunchKernelGGL(k_cand_to_row, dim3((unsigned)std::min<int64_t>(4096, (m + FTPB - 1) / FTPB)), dim3(FTPB), 0,
                         s, ids, m, coff, start, nr, perm);
      GM_CHECK_LAUNCH();
    }
  }
  if (n_match) *n_match = nm;
  if (n_envelope) *n_envelope = ne;
  if (ids && nm > ids_cap) return GM_E_CAPACITY;
  return GM_OK;
}

}  // namespace gm

extern "C" {

int gm_table_scan(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                  const gm_key_range* ranges, int64_t n_ranges, const gm_scan_filter* f, const int64_t* perm,
                  int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned) {
  return table_scan(ctx, shard, bin, z, n, ranges, n_ranges, f, nullptr, perm, ids, ids_cap, n_match, n_scanned,
                    nullptr);
}

int gm_table_scan_geom(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                       const gm_key_range* ranges, int64_t n_ranges, const gm_scan_filter* f,
                       const gm_geom_column* geom, const int64_t* perm, int64_t* ids, int64_t ids_cap,
                       int64_t* n_match, int64_t* n_scanned, int64_t* n_envelope) {
  if (!ctx) return GM_E_INVALID;
  if (!f) return set_error("gm_table_scan_geom: the filter (query boxes, envelope columns) is required"), GM_E_INVALID;
  if (!f->polys && f->n_boxes <= 0)
    return set_error("gm_table_scan_geom: at least one query box is required"), GM_E_INVALID;
  if ((!f->polys && !f->boxes) || !f->xmin || !f->ymin || !f->xmax || !f->ymax)
    return set_error("gm_table_scan_geom: the boxes and the four envelope columns are required"), GM_E_INVALID;
  if (!geom) return set_error("gm_table_scan_geom: the geometry column is required"), GM_E_INVALID;
  if (geom->ordinal_bits != 64 && geom->ordinal_bits != 32)
    return set_error("gm_table_scan_geom: ordinal_bits must be 64 or 32"), GM_E_INVALID;
  if ((geom->type < GM_GEOM_POINT || geom->type > GM_GEOM_MULTIPOLYGON) && geom->type != GM_GEOM_WKB)
    return set_error("gm_table_scan_geom: unknown geometry type"), GM_E_INVALID;
  if (geom->type == GM_GEOM_WKB && geom->ordinal_bits != 64)
    return set_error("gm_table_scan_geom: ordinal_bits must be 64 for a GM_GEOM_WKB column"), GM_E_INVALID;
  if (!geom_col_ok(geom))
    return set_error("gm_table_scan_geom: coords or a List offsets level of the geometry type is NULL"), GM_E_INVALID;
  return table_scan(ctx, shard, bin, z, n, ranges, n_ranges, f, geom, perm, ids, ids_cap, n_match, n_scanned,
                    n_envelope);
}

int gm_key_range_scan(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                      const gm_key_range* ranges, int64_t n_ranges, const uint8_t* filter_bytes, size_t filter_len,
                      const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned) {
  if (!ctx) return GM_E_INVALID;
  if (n > 0 && !bin) return GM_E_INVALID;
  gm_scan_filter f{};
  f.z3filter = filter_bytes;
  f.z3filter_len = filter_len;
  return gm_table_scan(ctx, shard, bin, z, n, ranges, n_ranges, &f, perm, ids, ids_cap, n_match, n_scanned);
}

}  // extern "C"
