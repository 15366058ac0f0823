// gm_sort.hip -- gm_sort_keys: the key table's rows sorted on the device into table order.
//
// A GeoMesa Z3 table is the set of row keys [shard?][bin BE16][z BE64][id] kept in byte order by the store
// (Z3IndexKeySpace.toIndexKey, idx/index/z3/Z3IndexKeySpace.scala:63-95); a query seeks each byte range
// getRangeBytes produces (Z3IndexKeySpace.scala:196-238).  Here the table is columnar and resident in HBM,
// and gm_sort_keys is a stable sort of (shard u8, bin u16, z u64) in that byte order: K = shard:bin:z, 88 bits.
//   k_key_or_and_sample, k_sort_count -- which bits of K vary (OR / AND), and every pass's digit counts;
//   k_sort_pass  -- a one-sweep digit pass (a digit of <= 9 bits) over 8192-row tiles, into 16-B records;
//   k_local_bounds, k_sort_local -- after passes over the top ~log2(n) - 1 varying bits (three 9-bit digits
//                   at 250M rows), every run of equal prefixes (a few rows) ranked by full key in LDS;
//   gm_sort_keys -- the driver, in named steps (SortCall).  A run longer than 256 rows (skewed keys) sends
//                   the call to 8-bit passes over every varying byte (LSD), as does GM_PARAM_SORT_MODE 1.
// The table's other key passes are in gm_key_table.hip, its range scan in gm_filter.hip.  KeyCols comes from
// gm_keycols.hpp; no device code crosses units.
#include <algorithm>
#include <vector>

#include "gm_keycols.hpp"
#include "gm_sort_plan.hpp"

namespace gm {

constexpr int MAXTAG = 16;              // pass tags per call: prefix passes + a fallback's digit passes

// 24 bits of K = bs:z (bs = bin | shard << 16) from bit `off` (0 <= off < 88) up
__device__ __forceinline__ uint32_t key_bits(uint32_t bs, uint64_t z, int off) {
  uint64_t v;
  if (off >= 64) v = (uint64_t)bs >> (off - 64);
  else {
    v = z >> off;
    if (off > 0) v |= (uint64_t)bs << (64 - off);
  }
  return (uint32_t)v & 0xffffffu;
}

// a row in flight between passes: {z lo, z hi, input row, bs} (bs = bin | shard << sq, squeeze_bs)
__device__ __forceinline__ uint64_t rec_z(uint4 r) { return (uint64_t)r.x | ((uint64_t)r.y << 32); }
__device__ __forceinline__ uint4 make_rec(uint64_t z, uint32_t row, uint32_t bs) {
  return make_uint4((uint32_t)z, (uint32_t)(z >> 32), row, bs);
}

// With a shard byte, the sort's key packs it right above bin's highest varying bit: bs = bin low bits |
// shard << sq (sq = that bit + 1, 16 without a shard).  The bits of bin above it are the same in every
// key (binhi), so this order is the (shard, bin) order, and the key's varying bits are contiguous: the
// prefix digits cover shard and bin together instead of a 9-bit digit spanning bin's constant top bits
// (with 4 shards and weekly bins that digit held 2 varying bits of 9, the runs of equal prefixes grew to
// ~128 rows and the sort took 31.5 ms per 250M rows instead of ~10.5).
__device__ __forceinline__ uint32_t squeeze_bs(uint32_t b, int sq) { return (b & ((1u << sq) - 1u)) | ((b >> 16) << sq); }
__device__ __forceinline__ uint16_t bs_bin(uint32_t w, int sq, uint32_t binhi) {
  return (uint16_t)((w & ((1u << sq) - 1u)) | binhi);
}

// which digit passes carry information: the OR and the AND of every key column (a digit on which
// OR == AND is the same for every key, so its pass would be the identity and is skipped).
__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_and(uint64_t v) { return ~wave_or(~v); }
// the block's OR (zo, bo) and AND (za, ba) of z and bs into acc[0..3] = OR z, OR bs, AND z, AND bs: per wave, then through
// LDS one device atomic per value per block (not per wave: same 4 addresses).  Every thread calls it: one block barrier.
template <int NWAVE>
__device__ __forceinline__ void block_or_and(uint64_t zo, uint64_t bo, uint64_t za, uint64_t ba,
                                             unsigned long long* __restrict__ acc) {
  __shared__ uint64_t s_oa[NWAVE][4];
  zo = wave_or(zo); za = wave_and(za); bo = wave_or(bo); ba = wave_and(ba);
  if ((threadIdx.x & 63) == 0) {
    uint64_t* e = s_oa[threadIdx.x >> 6];
    e[0] = zo; e[1] = bo; e[2] = za; e[3] = ba;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    uint64_t v = s_oa[0][j];
    for (int w = 1; w < NWAVE; ++w) v = j < 2 ? (v | s_oa[w][j]) : (v & s_oa[w][j]);
    if (j < 2) atomicOr(&acc[j], (unsigned long long)v);
    else atomicAnd(&acc[j], (unsigned long long)v);
  }
}
// f(z, bs) over every row of the caller's columns, one wave per 512-row chunk.  With 16-B aligned
// columns (`wide`) every load is one contiguous 1 KiB per wave instruction: z as 16-B pairs (rows
// 128 u + 2 lane, + 1), bin as 8 rows per lane and the shard byte as 16 per lane, staged through the
// wave's LDS slice so each lane meets the bins of its z rows (narrow per-lane loads stream at about
// half the 16-B rate on gfx950); other chunks go row by row.
constexpr int RCH = 512;   // rows per wave chunk
template <bool SH, int NWAVE, class F>
__device__ __forceinline__ void for_rows(const KeyCols& c, int64_t n, int wide, F f) {
  __shared__ __attribute__((aligned(16))) uint16_t s_b[NWAVE][RCH];
  __shared__ __attribute__((aligned(16))) uint8_t s_s[NWAVE][SH ? RCH : 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nchunk = (n + RCH - 1) / RCH, stride = (int64_t)gridDim.x * NWAVE;
  for (int64_t ch = (int64_t)blockIdx.x * NWAVE + wave; ch < nchunk; ch += stride) {   // wave-uniform
    const int64_t r0 = ch * RCH;
    if (wide && r0 + RCH <= n) {
      ulonglong2 zz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) zz[u] = *(const ulonglong2*)(c.z + r0 + 128 * u + 2 * lane);
      *(uint4*)&s_b[wave][8 * lane] = *(const uint4*)(c.bin + r0 + 8 * lane);
      if (SH && lane < RCH / 16) *(uint4*)&s_s[wave][16 * lane] = *(const uint4*)(c.sh + r0 + 16 * lane);
      wave_lds_sync();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = 128 * u + 2 * lane;
        f(zz[u].x, (uint32_t)s_b[wave][j] | (SH ? (uint32_t)s_s[wave][j] << 16 : 0u));
        f(zz[u].y, (uint32_t)s_b[wave][j + 1] | (SH ? (uint32_t)s_s[wave][j + 1] << 16 : 0u));
      }
      wave_lds_sync();   // the slice is free for the next chunk
    } else {
      for (int64_t r = r0 + lane; r < min(n, r0 + RCH); r += 64) f(c.z[r], c.bs<SH>(r));
    }
  }
}

// The OR / AND of a strided sample of the keys (65,536 rows, the last row included): the host plans the
// digits from it and k_sort_count counts them in the same read that takes the exact OR / AND; a plan
// that the exact bits change is counted again (GM_PARAM_SORT_LAST reports the path either way)
constexpr int SAMPLE = 65536;
template <bool SH>
__global__ __launch_bounds__(256) void k_key_or_and_sample(KeyCols c, int64_t n, unsigned long long* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t step = n > SAMPLE ? n / SAMPLE : 1;
  uint64_t zo = 0, za = ~0ull, bo = 0, ba = ~0ull;
  auto take = [&](int64_t r) {
    const uint64_t z = c.z[r], b = c.bs<SH>(r);
    zo |= z; za &= z; bo |= b; ba &= b;
  };
  if (i < SAMPLE && i * step < n) take(i * step);
  if (i == 0) take(n - 1);
  block_or_and<4>(zo, bo, za, ba, acc);
}

// Every pass's digit counts in one read: counts[base_k + d] = rows whose digit k (bits [off_k, off_k +
// w_k) of K) is d, base_k = k * 512.  Four LDS copies of the counters (by wave) cut the atomic
// collisions.  ORAND: the same read also takes the exact OR / AND of the caller's columns (block_or_and).
constexpr int NB_MAX = 1 << WMAX;
__device__ __forceinline__ uint32_t key_digit_w(uint32_t bs, uint64_t z, int off, int w) {
  return key_bits(bs, z, off) & ((1u << w) - 1u);
}
constexpr int CNT_LDS = 2816;           // 11 byte digits x 256, or 4 prefix digits x 512 (<= 2048)
constexpr int CT = 1024;   // count threads per block
#ifndef GM_SORT_CGRID   // count blocks: 1024 vs 512 -0.04 ms per sort, 256 +0.07 (profiles/r5/sort_count_grid_ab.txt)
#define GM_SORT_CGRID 1024
#endif
template <bool SH, bool ORAND>
__global__ __launch_bounds__(CT) void k_sort_count(KeyCols c, int64_t n, DigitOffs o, uint32_t* __restrict__ counts, int wide,
                                                   unsigned long long* __restrict__ acc, int sq) {
  __shared__ uint32_t h[4][CNT_LDS];
  const int copy = (threadIdx.x >> 6) & 3;
  for (int i = threadIdx.x; i < 4 * CNT_LDS; i += CT) (&h[0][0])[i] = 0u;
  __syncthreads();
  uint64_t zo = 0, za = ~0ull, bo = 0, ba = ~0ull;
  for_rows<SH, CT / 64>(c, n, wide, [&](uint64_t z, uint32_t b) {
    if (ORAND) { zo |= z; za &= z; bo |= b; ba &= b; }   // of the caller's bs (bin | shard << 16)
    const uint32_t bk_s = SH ? squeeze_bs(b, sq) : b;
    for (int k = 0, bk = 0; k < o.np; bk += 1 << o.w[k], ++k)
      atomicAdd(&h[copy][bk + key_digit_w(bk_s, z, o.off[k], o.w[k])], 1u);
  });
  if (ORAND) block_or_and<CT / 64>(zo, bo, za, ba, acc);   // its barrier also closes the counting
  else __syncthreads();
  for (int k = 0, bk = 0; k < o.np; bk += 1 << o.w[k], ++k)
    for (int d = threadIdx.x; d < (1 << o.w[k]); d += CT) {
      const int i = bk + d;
      const uint32_t v = h[0][i] + h[1][i] + h[2][i] + h[3][i];
      if (v) atomicAdd(&counts[k * NB_MAX + d], v);
    }
}

// One-sweep digit pass over a digit of w <= 9 bits.  Block b takes tile k (the next in a counter, so
// every lower tile is already running) of 8192 rows; wave w owns rows [512 w, 512 w + 512) of it and
// reads them in 4 slots of 128 rows, 2 per lane (rows r and r + 64: two halves of 64 consecutive rows).
// Within a half, lanes holding the same digit find each other through a 64-bit LDS slot per digit; a
// per-wave LDS counter per digit turns half ranks into wave ranks, a scan over the waves into tile
// ranks, so a row's place in the tile is (digit, wave, slot, half, lane) = stable.  The tile's digit
// offsets in the output are the digit's global start plus its rows in every lower tile: thread d
// publishes digit d's tile count as soon as the tile is ranked ({count, AGG} granule, one 8-B write-through
// store), then walks back over the lower tiles' granules, adding counts until it meets an inclusive prefix
// (PRE), and publishes its own (decoupled look-back).  The tile is reordered in LDS meanwhile and leaves as
// digit runs of 16-B records.  Granule tags carry the pass (tag) so no pass reads another's; the status array
// is cleared once per call.  1024-thread blocks over 8192-row tiles (LDS ~148 KB: one block, 16 waves, per CU):
// 10.84-10.86 -> 10.48-10.51 ms per 250M-row sort against 512 threads / 4096 rows at two blocks per CU
// once the tile's loads were all in flight together (profiles/r5/sort_tile_shape_ab.txt; 768 threads
// 11.97-11.99, 1024 x 2048 rows 13.75-13.77, 1024 x 6144 11.63-11.67, 512 x 8192 11.30-11.35).
#ifndef GM_SORT_PSLOT
#define GM_SORT_PSLOT 4
#endif
#ifndef GM_SORT_PT
#define GM_SORT_PT 1024
#endif
constexpr int PT = GM_SORT_PT, PW = PT / 64, PSLOT = GM_SORT_PSLOT, PTILE = PT * 2 * PSLOT;   // 8192 rows per tile
static_assert(PT >= NB_MAX, "one thread per digit");
constexpr uint64_t GR_VAL = (1ull << 48) - 1;
#ifndef GM_SORT_LB
#define GM_SORT_LB 4
#endif
constexpr int LB = GM_SORT_LB;   // look-back granules per round trip

struct PassArgs {
  KeyCols in;             // the caller's columns (first pass) ...
  const uint4* rec_in;    // ... or the previous pass's records
  uint8_t* sh_out; uint16_t* bin_out; uint64_t* z_out; int64_t* perm_out;   // the caller's outputs (last pass) ...
  uint4* rec_out;         // ... or records
  int64_t n;
  int off, w;             // digit: bits [off, off + w) of K
  uint32_t tag;           // 1..MAXTAG
  const uint32_t* counts;           // this pass's 2^w digit counts
  unsigned long long* status;       // ntiles x 2^w granules
  unsigned int* ctr;                // this pass's tile counter
  int vec;
  int sq;                 // the shard's place in the records' bs (squeeze_bs) ...
  uint32_t binhi;         // ... and bin's constant bits above it
};

template <bool IN_REC, bool OUT_USER, bool SH>
__global__ __launch_bounds__(PT) void k_sort_pass(PassArgs a) {
  __shared__ uint4 s_rec[PTILE];
  __shared__ uint16_t s_wcnt[PW][NB_MAX];   // per wave: rows of each digit so far (then: wave offsets)
  __shared__ uint32_t s_dstart[NB_MAX];     // the digit's first slot in the tile
  __shared__ uint32_t s_gpos[NB_MAX];       // output row of tile slot q = s_gpos[d] + q (mod 2^32)
  __shared__ uint32_t s_wsum[2][PW];
  __shared__ uint32_t s_tile;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int w = a.w, nb = 1 << w;
  // this pass's global count of digit t, loaded before anything waits (used after the ranking)
  const uint32_t cg_early = t < nb ? a.counts[t] : 0u;
  if (t == 0) s_tile = atomicAdd(a.ctr, 1u);
  for (int i = t; i < PW * NB_MAX / 2; i += PT) ((uint32_t*)&s_wcnt[0][0])[i] = 0u;
  __syncthreads();
  const int64_t tile = s_tile, t0 = tile * PTILE, n = a.n;
  // this lane's rows: slot k of wave w holds rows r = t0 + 512 w + 128 k + lane (A) and r + 64 (B), so in input order a
  // slot is its 64 A rows, then its 64 B rows, and each half ranks like one row per lane, with one mask per row.  (Pairs
  // (2 lane, 2 lane + 1) would interleave the halves: four cross masks per pair, ~80 not ~45 VALU per row, profiles/r6.)
  uint4 rv[PSLOT][2];
  const bool full = t0 + PTILE <= n;   // every tile but the last (uniform)
  auto row = [&](int k, int e) -> int64_t { return t0 + wave * (2 * 64 * PSLOT) + k * 128 + 64 * e + lane; };
  auto rec = [&](int64_t i) -> uint4 {   // row i: the previous pass's record, or one from the caller's columns
    if (IN_REC) return a.rec_in[i];
    uint32_t b = a.in.bs<SH>(i);
    if (SH) b = squeeze_bs(b, a.sq);
    return make_rec(a.in.z[i], (uint32_t)i, b);
  };
  auto load = [&](auto get) {
#pragma unroll
    for (int k = 0; k < PSLOT; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) rv[k][e] = get(row(k, e));
  };
  // Three load shapes.  A full tile of records and a full tile of aligned columns (a.vec) load unconditionally,
  // so the compiler counts the loads: all 2 * PSLOT are in flight before the first wait.  Any other tile is
  // guarded row by row (a lane without a row holds zeros and ranks nothing).
  if (full && (IN_REC || a.vec)) load(rec);
  else load([&](int64_t i) { return i < n ? rec(i) : make_uint4(0u, 0u, 0u, 0u); });
  const uint64_t lt = lanemask_lt();
  uint32_t rd[PSLOT][2];   // wave rank | digit << 16; rank 0xffff = no row
  // lanes sharing a digit found through LDS instead of 9 ballot rounds: each row ORs its lane bit into
  // its digit's 64-bit slot, reads the slot back, and clears it.  The slots (512 per wave, 64 KB) alias
  // s_rec, which is written only after the ranking's barrier.
  static_assert(PW * NB_MAX * sizeof(uint64_t) <= sizeof(uint4) * PTILE, "digit-match slots alias s_rec");
  uint64_t* mslot = (uint64_t*)s_rec + wave * NB_MAX;
  for (int j = lane; j < NB_MAX; j += 64) mslot[j] = 0ull;
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < PSLOT; ++k)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool ok = row(k, e) < n;
      const uint32_t d = key_digit_w(rv[k][e].w, rec_z(rv[k][e]), a.off, w);
      if (ok) atomicOr((unsigned long long*)&mslot[d], 1ull << lane);
      wave_lds_sync();
      const uint64_t m = ok ? mslot[d] : 0ull;   // lanes of this half whose row holds my row's digit
      wave_lds_sync();
      if (ok) mslot[d] = 0ull;
      const int r = __popcll(m & lt);
      // the wave's counter: read before this half's increment, then the first row of each digit adds
      const uint32_t c = s_wcnt[wave][d];
      rd[k][e] = (ok ? c + r : 0xffffu) | (d << 16);
      __builtin_amdgcn_wave_barrier();
      if (ok && r == 0) s_wcnt[wave][d] = (uint16_t)(c + __popcll(m));
      __builtin_amdgcn_wave_barrier();
    }
  __syncthreads();
  // thread t owns digit t (t < nb): wave offsets, the tile total, scans of totals and global counts
  uint32_t tot = 0, xt = 0, xb = 0, cg = 0;
  const bool own = t < nb;
  if (own) {
#pragma unroll
    for (int v = 0; v < PW; ++v) {
      const uint32_t c = s_wcnt[v][t];
      s_wcnt[v][t] = (uint16_t)tot;
      tot += c;
    }
    // the tile's count for this digit, published before anything else
    const uint64_t g0 = ((uint64_t)(2 * a.tag + (tile == 0 ? 1 : 0)) << 48) | tot;
    __hip_atomic_store(a.status + tile * nb + t, g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cg = cg_early;
  }
  xt = tot; xb = cg;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(xt, o, 64), yb = __shfl_up(xb, o, 64);
    if (lane >= o) { xt += y; xb += yb; }
  }
  if (lane == 63) { s_wsum[0][wave] = xt; s_wsum[1][wave] = xb; }
  __syncthreads();
  uint32_t dstart = 0, gbase = 0;
  if (own) {
    uint32_t pt = 0, pb = 0;
    for (int v = 0; v < wave; ++v) { pt += s_wsum[0][v]; pb += s_wsum[1][v]; }
    dstart = pt + xt - tot;
    gbase = pb + xb - cg;
    s_dstart[t] = dstart;
  }
  __syncthreads();
  // the tile reordered by digit in LDS
#pragma unroll
  for (int k = 0; k < PSLOT; ++k) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t r = rd[k][e] & 0xffffu, d = rd[k][e] >> 16;
      if (r == 0xffffu) continue;
      s_rec[s_dstart[d] + s_wcnt[wave][d] + r] = rv[k][e];
    }
  }
  if (own) {   // look-back: the digit's rows in every lower tile
    uint64_t excl = 0;
    if (tile > 0) {
      const uint64_t tag_agg = 2 * a.tag, tag_pre = 2 * a.tag + 1;
      int64_t p = tile - 1;
      // LB granules (tiles p, p - 1, ..., p - LB + 1) per round trip, all loads in flight together:
      // the walk adds aggregates up to the first inclusive prefix, or re-polls from the first
      // granule not yet published.  Tile 0 always publishes a prefix, so no walk passes below it.
      for (;;) {
        uint64_t v[LB];
#pragma unroll
        for (int i = 0; i < LB; ++i)
          v[i] = p - i >= 0 ? __hip_atomic_load(a.status + (p - i) * nb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : 0ull;
        int i = 0;
        bool done = false;
        for (; i < LB; ++i) {
          const uint64_t tg = v[i] >> 48;
          if (tg == tag_pre) { excl += v[i] & GR_VAL; done = true; break; }
          if (tg != tag_agg) break;
          excl += v[i] & GR_VAL;
        }
        if (done) break;
        p -= i;
        if (i < LB) __builtin_amdgcn_s_sleep(1);
      }
      __hip_atomic_store(a.status + tile * nb + t, ((uint64_t)(2 * a.tag + 1) << 48) | (excl + tot),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_gpos[t] = gbase + (uint32_t)excl - dstart;   // mod 2^32: every output row is < n <= 2^32 - 1
  }
  __syncthreads();
  const int cnt = (int)min((int64_t)PTILE, n - t0);
  for (int q = t; q < cnt; q += PT) {
    const uint4 r = s_rec[q];
    const int64_t g = (int64_t)(uint32_t)(s_gpos[key_digit_w(r.w, rec_z(r), a.off, w)] + (uint32_t)q);
    if (OUT_USER) {
      a.z_out[g] = rec_z(r);
      a.bin_out[g] = SH ? bs_bin(r.w, a.sq, a.binhi) : (uint16_t)r.w;
      if (SH) a.sh_out[g] = (uint8_t)(r.w >> a.sq);
      a.perm_out[g] = (int64_t)r.z;
    } else {
      a.rec_out[g] = r;
    }
  }
}

// Final placement after the prefix passes: the digit passes at bit offsets o1 > o2 > ... (each digit
// ends at a varying bit, and only constant bits lie between them) leave the rows grouped, stably, by
// P = digit(o1) : digit(o2) : ... -- the key's top varying bits, ~log2(n) - 1 of them, so that runs
// of equal P are short (Poisson(n / 2^bits) for uniform keys, 2 rows on average).  Tile k covers the
// runs of equal P that start in [k LSTEP, (k + 1) LSTEP); its rows are staged in LDS, a block scan
// marks each row's run (start, and at the start its end), each row counts the rows of its run with a
// smaller key (ties by position: stable) and goes to run start + rank: O(run length) LDS reads per
// row.  A run longer than RUN_MAX rows (skewed or repeated keys) sets *flag and the host sorts with
// digit passes over every varying byte instead.
#ifndef GM_SORT_LCAP
#define GM_SORT_LCAP 2048
#endif
#ifndef GM_SORT_LT
#define GM_SORT_LT 512
#endif
constexpr int LT = GM_SORT_LT, LCAP = GM_SORT_LCAP, LPT = LCAP / LT, RUN_MAX = 256, LSTEP = LCAP - RUN_MAX;

// the prefix digits of width w (offsets o.x > o.y > ...; an offset < 0: no digit, and every later
// offset is < 0 too): npre * w <= 32 bits (gm_sort_keys), so the digits that exist are shifted in and
// the absent ones are not -- a shift per absent digit would push the first digit's top bits out of the
// word and merge distinct prefixes into one run
__device__ __forceinline__ uint32_t prefix4(uint32_t bs, uint64_t z, int4 o, int w) {
  uint32_t p = o.x >= 0 ? key_digit_w(bs, z, o.x, w) : 0u;
  if (o.y >= 0) p = (p << w) | key_digit_w(bs, z, o.y, w);
  if (o.z >= 0) p = (p << w) | key_digit_w(bs, z, o.z, w);
  if (o.w >= 0) p = (p << w) | key_digit_w(bs, z, o.w, w);
  return p;
}

// the local tiles' bounds: bounds[k] = the first run start at or after k LSTEP (0 and n at the ends;
// -1 and the flag when no run starts within RUN_MAX rows), one wave per bound, so that k_sort_local
// reads its next tile's bounds while it ranks the current one
__global__ __launch_bounds__(256) void k_local_bounds(const uint4* __restrict__ rec_in, int64_t n, int4 po, int pw,
                                                      int64_t* __restrict__ bounds, uint32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t ntile = (n + LSTEP - 1) / LSTEP;
  if (k > ntile) return;   // wave-uniform
  int64_t p = min(n, k * LSTEP);
  if (p > 0 && p < n) {
    const uint4 v0 = rec_in[p - 1];
    const uint32_t pp = prefix4(v0.w, rec_z(v0), po, pw);
    int64_t found = -1;
    for (int c = 0; c <= RUN_MAX / 64 && found < 0; ++c) {   // wave-uniform
      const int64_t r = p + c * 64 + lane;
      bool diff = r >= n;
      if (!diff) { const uint4 v = rec_in[r]; diff = prefix4(v.w, rec_z(v), po, pw) != pp; }
      const uint64_t bal = __ballot(diff);
      if (bal) found = p + c * 64 + __builtin_ctzll(bal);
    }
    p = (found < 0 || found - p > RUN_MAX) ? -1 : found;
    if (p < 0 && lane == 0) *flag = 1u;
  }
  if (lane == 0) bounds[k] = p;
}

// waves per SIMD: 8 = four resident 512-thread blocks per CU (64 VGPRs, no spills; the tiles' LDS is
// 32 KB each): 10.42-10.44 -> 10.22-10.25 ms per sort over the compiler's 75 VGPRs / three blocks;
// loading the next tile while ranking the current one instead: 11.61-11.66 ms
// (profiles/r5/sort_local_occupancy_ab.txt)
#ifndef GM_SORT_LOCAL_WPE
#define GM_SORT_LOCAL_WPE 8
#endif
template <bool SH>
__global__ __launch_bounds__(LT) __attribute__((amdgpu_waves_per_eu(GM_SORT_LOCAL_WPE))) void k_sort_local(
    const uint4* __restrict__ rec_in, uint8_t* __restrict__ sh_out, uint16_t* __restrict__ bin_out,
    uint64_t* __restrict__ z_out, int64_t* __restrict__ perm_out, int64_t n, int4 po, int pw,
    uint32_t* __restrict__ flag, const int64_t* __restrict__ bounds, int sq, uint32_t binhi) {
  __shared__ uint64_t s_z[LCAP];
  __shared__ uint32_t s_bs[LCAP];
  __shared__ uint32_t s_run[LCAP];   // prefix; then run start (low 16) | at a run start, its end << 16
  __shared__ uint32_t s_wmax[LT / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t ntile = (n + LSTEP - 1) / LSTEP;
  int64_t an = -1, bn = -1;   // the next tile's bounds (uniform: scalar loads, one tile ahead)
  if ((int64_t)blockIdx.x < ntile) { an = bounds[blockIdx.x]; bn = bounds[blockIdx.x + 1]; }
  for (int64_t tk = blockIdx.x; tk < ntile; tk += gridDim.x) {   // block-uniform
    const int64_t a = an, b = bn;
    if (tk + gridDim.x < ntile) { an = bounds[tk + gridDim.x]; bn = bounds[tk + gridDim.x + 1]; }
    if (a < 0 || b < 0) continue;   // flagged: the host redoes the sort
    const int m = (int)(b - a);     // <= LSTEP + RUN_MAX = LCAP
    // the tile's rows: all LPT loads of a thread issued together; a row's input index stays in a
    // register for the write-out (thread t handles rows t + k LT in both phases)
    uint4 v[LPT];
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int i = t + k * LT;
      if (i < m) v[k] = rec_in[a + i];
    }
    uint32_t row[LPT];
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int i = t + k * LT;
      row[k] = v[k].z;
      if (i < m) {
        const uint64_t zz = rec_z(v[k]);
        s_z[i] = zz; s_bs[i] = v[k].w; s_run[i] = prefix4(v[k].w, zz, po, pw);
      }
    }
    __syncthreads();
    // run starts: a block max-scan of (row starts a run ? row : 0) over rows [LPT t, LPT t + LPT)
    uint32_t st[LPT];
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int i = LPT * t + k;
      if (i < m && (i == 0 || s_run[i] != s_run[i - 1])) run = (uint32_t)i;
      st[k] = run;
    }
    uint32_t x = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x = max(x, y);
    }
    if (lane == 63) s_wmax[wave] = x;
    __syncthreads();
    uint32_t carry = 0;
    for (int w = 0; w < wave; ++w) carry = max(carry, s_wmax[w]);
    const uint32_t prev = __shfl_up(x, 1, 64);
    if (lane > 0) carry = max(carry, prev);
#pragma unroll
    for (int k = 0; k < LPT; ++k) st[k] = max(st[k], carry);
    __syncthreads();   // every prefix read before s_run is overwritten
#pragma unroll
    for (int k = 0; k < LPT; ++k)
      if (LPT * t + k < m) s_run[LPT * t + k] = st[k];
    __syncthreads();
    // a run's end, stored at its start: written by the next run's first row (or the tile's last row)
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int i = LPT * t + k;
      if (i < m && i > 0 && st[k] == (uint32_t)i) {
        const uint32_t ps = s_run[i - 1] & 0xffffu;
        s_run[ps] = ps | ((uint32_t)i << 16);
      }
      if (i == m - 1) s_run[st[k]] = st[k] | ((uint32_t)m << 16);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      const int i = t + k * LT;
      if (i >= m) continue;
      const int s0 = (int)(s_run[i] & 0xffffu), e0 = (int)(s_run[s0] >> 16);
      if (e0 - s0 > RUN_MAX) { *flag = 1u; continue; }
      const uint64_t zi = s_z[i];
      const uint32_t bi = s_bs[i];
      int r = 0;
      for (int j = s0; j < e0; ++j) {
        const uint32_t bj = s_bs[j];
        const uint64_t zj = s_z[j];
        r += (bj < bi) || (bj == bi && (zj < zi || (zj == zi && j < i)));
      }
      const int64_t dst = a + s0 + r;
      z_out[dst] = zi;
      bin_out[dst] = SH ? bs_bin(bi, sq, binhi) : (uint16_t)bi;
      if (SH) sh_out[dst] = (uint8_t)(bi >> sq);
      perm_out[dst] = (int64_t)row[k];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(STPB) void k_widen_perm(int64_t n, int64_t* __restrict__ p64) {
  for (int64_t i = (int64_t)blockIdx.x * STPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * STPB) p64[i] = i;
}

}  // namespace gm

using namespace gm;

namespace {

// The sort's slots of ctx->d_scratch (u64 each).  An OR / AND set is {OR z, OR bs, AND z, AND bs} of the
// caller's keys: 0..3 of every key (k_sort_count), 8..11 of the sample (k_key_or_and_sample); 4 is the flag
// of a run of equal prefixes too long to rank locally (k_local_bounds, k_sort_local)
constexpr int ACC_EXACT = 0, ACC_FLAG = 4, ACC_SAMPLE = 8;

// Z2 / XZ2 tables have no time bin: the sort runs over a zero bin column (constant, so no digit pass looks
// at it) and its bin output goes to scratch
int zero_bin(gm_ctx* ctx, int64_t n, const int16_t** bin, int16_t** bin_out) {
  Carve c{16};
  const size_t o_in = c.take((size_t)n * 2), o_out = c.take((size_t)n * 2);
  char* zb = nullptr;
  const int rc = ctx_workspace(ctx, WS_SCAN, c.total, (void**)&zb);
  if (rc) return rc;
  *bin = (const int16_t*)(zb + o_in); *bin_out = (int16_t*)(zb + o_out);
  GM_HIP(hipMemsetAsync(zb + o_in, 0, (size_t)n * 2, ctx->stream));
  return GM_OK;
}

// The context's sort workspace: records x 2 | look-back granules (ntiles x NB_MAX) | digit counts (by tag) |
// tile counters (by tag) | local bounds, 16-B aligned
constexpr size_t COUNTS_BYTES = (size_t)MAXTAG * NB_MAX * 4;
struct SortWs {
  uint4* rec[2];
  unsigned long long* status; uint32_t* counts; unsigned int* ctr; int64_t* lbounds;
  int take(gm_ctx* ctx, int64_t n) {
    Carve c{16};
    const size_t o_r0 = c.take((size_t)n * 16), o_r1 = c.take((size_t)n * 16),
                 o_st = c.take((size_t)((n + PTILE - 1) / PTILE) * NB_MAX * 8), o_c = c.take(COUNTS_BYTES),
                 o_t = c.take((size_t)MAXTAG * 4), o_b = c.take((size_t)((n + LSTEP - 1) / LSTEP + 1) * 8);
    char* base = nullptr;
    const int rc = ctx_workspace(ctx, WS_SORT, c.total, (void**)&base);
    if (rc) return rc;
    rec[0] = (uint4*)(base + o_r0); rec[1] = (uint4*)(base + o_r1);
    status = (unsigned long long*)(base + o_st); counts = (uint32_t*)(base + o_c);
    ctr = (unsigned int*)(base + o_t); lbounds = (int64_t*)(base + o_b);
    GM_HIP(hipMemsetAsync(status, 0, o_b - o_st, ctx->stream));   // granules (tag 0 = none), counts, counters: adjacent
    return GM_OK;
  }
};

// One validated gm_sort_keys call and the driver's steps
struct SortCall {
  gm_ctx* ctx; hipStream_t s;
  unsigned long long* acc;   // ctx->d_scratch, by the ACC_ slots
  KeyCols in; int64_t n;
  uint8_t* sh_out; uint16_t* bin_out; uint64_t* z_out; int64_t* perm_out;
  SortWs ws; SortPlan plan;
  // digit counts of `o` into cnt, one read of every key; `orand`: the same read takes the exact OR / AND
  int count(const DigitOffs& o, uint32_t* cnt, bool orand, int sq) {
    const int wide = aligned16(in.z) && aligned16(in.bin) && aligned16(in.sh);   // 16-B loads of every column
    const int64_t nchunk = (n + RCH - 1) / RCH;
    const int cgrid = (int)std::max<int64_t>(1, std::min<int64_t>(GM_SORT_CGRID, (nchunk + CT / 64 - 1) / (CT / 64)));
    with_flags([&](auto SH, auto ORAND) {
      hipLaunchKernelGGL((k_sort_count<SH(), ORAND()>), dim3(cgrid), dim3(CT), 0, s, in, n, o, cnt, wide,
                         ORAND() ? acc + ACC_EXACT : nullptr, sq);
    }, in.sh != nullptr, orand);
    GM_CHECK_LAUNCH();
    return GM_OK;
  }
  // the plan of the OR / AND set at `slot`, read back (synchronises the stream)
  int read_plan(int slot, SortPlan* p) {
    unsigned long long h[4];
    GM_HIP(hipMemcpyAsync(h, acc + slot, sizeof(h), hipMemcpyDeviceToHost, s));
    GM_HIP(hipStreamSynchronize(s));
    *p = plan_sort(h, in.sh != nullptr, n, ctx->sort_mode);
    return GM_OK;
  }
  // Planning: the sample's OR / AND -> plan_sort -> that guess's first digit set counted in the read that
  // takes the exact OR / AND -> plan_sort.  *counted: the exact bits give the same first digits, so their
  // counts stand; else they are cleared and the passes count again.
  int make_plan(bool* counted) {
    GM_HIP(hipMemsetAsync(acc + ACC_EXACT, 0, 16, s));            // OR z, OR bs
    GM_HIP(hipMemsetAsync(acc + ACC_EXACT + 2, 0xff, 16, s));     // AND z, AND bs
    GM_HIP(hipMemsetAsync(acc + ACC_FLAG, 0, 8, s));
    GM_HIP(hipMemsetAsync(acc + ACC_SAMPLE, 0, 16, s));
    GM_HIP(hipMemsetAsync(acc + ACC_SAMPLE + 2, 0xff, 16, s));
    with_flags([&](auto SH) {
      hipLaunchKernelGGL(k_key_or_and_sample<SH()>, dim3(SAMPLE / 256), dim3(256), 0, s, in, n, acc + ACC_SAMPLE);
    }, in.sh != nullptr);
    GM_CHECK_LAUNCH();
    SortPlan guess;
    int rc = read_plan(ACC_SAMPLE, &guess);
    if (rc || (rc = count(guess.first_digits(), ws.counts, true, guess.sq)) || (rc = read_plan(ACC_EXACT, &plan))) return rc;
    *counted = guess.first_digits() == plan.first_digits() && guess.sq == plan.sq;
    if (!*counted) GM_HIP(hipMemsetAsync(ws.counts, 0, COUNTS_BYTES, s));
    return GM_OK;
  }
  // every key equal: table order = input order
  int copy_equal() {
    if (in.sh) GM_HIP(hipMemcpyAsync(sh_out, in.sh, (size_t)n, hipMemcpyDeviceToDevice, s));
    GM_HIP(hipMemcpyAsync(bin_out, in.bin, (size_t)n * 2, hipMemcpyDeviceToDevice, s));
    GM_HIP(hipMemcpyAsync(z_out, in.z, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_widen_perm, dim3((unsigned)std::min<int64_t>(4096, (n + STPB - 1) / STPB)), dim3(STPB), 0, s, n,
                       perm_out);
    GM_CHECK_LAUNCH();
    ctx->sort_last = 0;
    return GM_OK;
  }
  // Digit passes of width w at bit offsets `offs` (LSD order) from the caller's columns, under tags tag0 + 1...;
  // the last one lands in the user columns when `to_user`, else in records (*last, when asked for).  `counted`:
  // the digits' counts are already at counts[tag0 * NB_MAX] (make_plan); else one read counts them first.
  int digit_passes(const std::vector<int>& offs, int w, bool to_user, int tag0, bool counted, const uint4** last) {
    const int np = (int)offs.size();
    uint32_t* cnt = ws.counts + (size_t)tag0 * NB_MAX;
    const int rc = counted ? GM_OK : count(digit_offs(offs, w), cnt, false, plan.sq);
    if (rc) return rc;
    // aligned caller columns: the first pass then loads a full tile's rows unconditionally
    const int vec = aligned_to<16>(in.z) && aligned_to<4>(in.bin) && aligned_to<2>(in.sh);
    for (int k = 0; k < np; ++k) {   // pass k reads what pass k - 1 wrote; PassArgs in its declared order
      const PassArgs a{in, k > 0 ? ws.rec[(k - 1) & 1] : nullptr, sh_out, bin_out, z_out, perm_out, ws.rec[k & 1], n,
                       offs[k], w, (uint32_t)(tag0 + k + 1), cnt + (size_t)k * NB_MAX, ws.status, ws.ctr + tag0 + k, vec,
                       plan.sq, plan.binhi};
      with_flags([&](auto IN_REC, auto OUT_USER, auto SH) {
        hipLaunchKernelGGL((k_sort_pass<IN_REC(), OUT_USER(), SH()>), dim3((unsigned)((n + PTILE - 1) / PTILE)), dim3(PT), 0,
                           s, a);
      }, k > 0, to_user && k == np - 1, in.sh != nullptr);
      GM_CHECK_LAUNCH();
    }
    if (last) *last = ws.rec[(np - 1) & 1];
    return GM_OK;
  }
  // The prefix passes, then every run of equal prefixes ranked in LDS into the user columns.  *done: the
  // table is sorted; else a run was longer than RUN_MAX and the byte passes redo the sort.
  int prefix_attempt(bool counted, bool* done) {
    const uint4* last = nullptr;
    const int rc = digit_passes(plan.first_offs(), plan.pw, false, 0, counted, &last);
    if (rc) return rc;
    const int4 po = make_int4(plan.pofs[0], plan.pofs[1], plan.pofs[2], plan.pofs[3]);
    const int lgrid = resident_blocks((const void*)k_sort_local<false>, ctx->device, LT, 2);
    const int64_t nbound = (n + LSTEP - 1) / LSTEP + 1;   // as SortWs carves lbounds
    uint32_t* d_flag = (uint32_t*)(acc + ACC_FLAG);
    hipLaunchKernelGGL(k_local_bounds, dim3((unsigned)((nbound + 3) / 4)), dim3(256), 0, s, last, n, po, plan.pw,
                       ws.lbounds, d_flag);
    with_flags([&](auto SH) {
      hipLaunchKernelGGL(k_sort_local<SH()>, dim3(lgrid), dim3(LT), 0, s, last, sh_out, bin_out, z_out, perm_out, n, po,
                         plan.pw, d_flag, ws.lbounds, plan.sq, plan.binhi);
    }, in.sh != nullptr);
    GM_CHECK_LAUNCH();
    uint32_t flag = 0;
    GM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s));
    GM_HIP(hipStreamSynchronize(s));
    *done = !flag;
    if (*done) ctx->sort_last = 256 + plan.npre;
    return GM_OK;
  }
};

}  // namespace

extern "C" int gm_sort_keys(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                            uint8_t* shard_out, int16_t* bin_out, int64_t* z_out, int64_t* perm_out) {
  if (!ctx || n < 0 || n > (int64_t)UINT32_MAX) return GM_E_INVALID;
  if (n == 0) return GM_OK;
  if (!z || !z_out || !perm_out || ((shard == nullptr) != (shard_out == nullptr)) ||
      ((bin == nullptr) != (bin_out == nullptr)))
    return GM_E_INVALID;
  int rc = bin ? GM_OK : zero_bin(ctx, n, &bin, &bin_out);
  if (rc) return rc;
  SortCall c{ctx, ctx->stream, (unsigned long long*)ctx->d_scratch, KeyCols{shard, (const uint16_t*)bin, (const uint64_t*)z},
             n, shard_out, (uint16_t*)bin_out, (uint64_t*)z_out, perm_out};
  bool counted = false;
  if ((rc = c.ws.take(ctx, n)) || (rc = c.make_plan(&counted))) return rc;
  if (c.plan.lsd.empty()) return c.copy_equal();
  int tag0 = 0;
  if (c.plan.prefix) {
    bool done = false;
    if ((rc = c.prefix_attempt(counted, &done)) || done) return rc;
    tag0 = c.plan.npre;   // flagged: the byte passes run under the tags after the attempt's ...
    counted = false;      // ... and count their own digits
  }
  ctx->sort_last = (int64_t)c.plan.lsd.size() + tag0;   // (a failed prefix attempt included)
  return c.digit_passes(c.plan.lsd, 8, true, tag0, counted, nullptr);
}
