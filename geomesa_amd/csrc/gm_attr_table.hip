// gm_attr_table.hip -- the attribute index table (`attr`, version 8) for the fixed-width bindings:
//   * gm_attr_index_key  -- AttributeIndexKeySpace.toIndexKey (idx/index/attribute/AttributeIndexKeySpace.scala:
//     68-137): the lexicoded value of every non-null slot as an ordered unsigned integer v (the key text is
//     v's lower-case hex digits, include/geomesa_hip.h) and the slot's row.  A null slot writes no row: the
//     validity bits go through the mask -> block scan -> ordered compaction pipeline of gm_scan.hpp, and the
//     surviving rows are encoded on the row_stream skeleton;
//   * gm_attr_key_bytes  -- the row-key prefix [shard?][hex text of v][0x00][tier] (:116-134), staged through
//     LDS as k_key_bytes does (gm_key_table.hip);
//   * gm_attr_sort       -- table order (shard, v, tier) by two stable passes of gm_sort_keys: by tier, a
//     gather, by (shard, v), the permutations composed;
//   * gm_attr_table_scan -- the seek over the wider key (k_range_bounds / merge_ranges / seek_ranges of
//     gm_scan.hpp with AttrCols) and the candidate scan gm_table_scan runs (scan_candidates, gm_filter.hip).
#include <vector>

#include "gm_arrow.hpp"
#include "gm_keycols.hpp"
#include "gm_scan.hpp"
#include "gm_stream.hpp"

namespace gm {

// ------------------------------------------------------------------ the lexicoders
// The ordered value of include/geomesa_hip.h's table: unsigned order of v = byte order of the key text.
template <int TYPE>
__device__ __forceinline__ uint64_t attr_ordered(const void* __restrict__ values, int64_t r) {
  if constexpr (TYPE == GM_ATTR_INT32) {
    return (uint32_t)((const int32_t*)values)[r] ^ 0x80000000u;
  } else if constexpr (TYPE == GM_ATTR_INT64) {
    return (uint64_t)((const int64_t*)values)[r] ^ (1ull << 63);
  } else if constexpr (TYPE == GM_ATTR_FLOAT32) {
    const float x = ((const float*)values)[r];
    const uint32_t b = x != x ? 0x7fc00000u : __float_as_uint(x);   // floatToIntBits: one NaN
    return (b >> 31) ? ~b : (b ^ 0x80000000u);
  } else {
    const double x = ((const double*)values)[r];
    const uint64_t b = x != x ? 0x7ff8000000000000ull : (uint64_t)__double_as_longlong(x);   // doubleToLongBits
    return (b >> 63) ? ~b : (b ^ (1ull << 63));
  }
}

// pass A of the compaction: a slot's validity bit
__global__ __launch_bounds__(FTPB) void k_attr_valid_mask(const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                          uint64_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  row_scan<4>(n, mask, block_counts, [&](int64_t i) { return arrow_valid(valid, voff, i); });
}

constexpr int ATPB = 256;
// table row j <- the ordered value of slot rows[j]
template <int TYPE>
__global__ __launch_bounds__(ATPB) void k_attr_encode(const void* __restrict__ values, const int64_t* __restrict__ rows,
                                                      int64_t m, uint64_t* __restrict__ v_out) {
  row_stream<ATPB>(m, [&](int64_t j) { v_out[j] = attr_ordered<TYPE>(values, rows[j]); });
}

// ------------------------------------------------------------------ row-key bytes
// 256 rows per block: each thread writes its row's bytes into LDS, then the block's contiguous 256 * klen
// bytes (a multiple of 16) leave with 16-B stores.  HEX = digits of the key text: 8 or 16.
constexpr int ATTR_KEY_MAX = 1 + 16 + 1 + 10;
__device__ __forceinline__ void put_be64(uint8_t* o, uint64_t w) {
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (uint8_t)(w >> (8 * (7 - j)));
}
template <int HEX>
__global__ __launch_bounds__(STPB) void k_attr_key_bytes(const uint8_t* __restrict__ sh, const uint64_t* __restrict__ v,
                                                         int tier, const int16_t* __restrict__ bin,
                                                         const int64_t* __restrict__ t, int64_t m, int klen,
                                                         uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s[STPB * ATTR_KEY_MAX];
  const int64_t r0 = (int64_t)blockIdx.x * STPB;
  const int64_t i = r0 + threadIdx.x;
  if (i < m) {
    uint8_t* o = s + threadIdx.x * klen;
    int k = 0;
    if (sh) o[k++] = sh[i];
    const uint64_t w = v[i];
#pragma unroll
    for (int j = HEX - 1; j >= 0; --j) {
      const uint32_t d = (uint32_t)(w >> (4 * j)) & 15u;
      o[k++] = (uint8_t)(d < 10 ? '0' + d : 'a' + (d - 10));
    }
    o[k++] = 0;   // ByteArrays.ZeroByte: the end of the value
    if (tier == GM_ATTR_TIER_DATE) {
      put_be64(o + k, (uint64_t)t[i] ^ (1ull << 63));   // ByteArrays.toOrderedBytes
    } else if (tier == GM_ATTR_TIER_Z3) {
      const uint16_t b = (uint16_t)bin[i];
      o[k++] = (uint8_t)(b >> 8);
      o[k++] = (uint8_t)b;
      put_be64(o + k, (uint64_t)t[i]);
    }
  }
  __syncthreads();
  const int64_t rows = min((int64_t)STPB, m - r0);
  const int64_t bytes = rows * klen;
  uint8_t* dst = out + r0 * klen;
  if (rows == STPB && (((uintptr_t)dst) & 15u) == 0) {
    const uint4* s4 = (const uint4*)s;
    uint4* d4 = (uint4*)dst;
    for (int j = threadIdx.x; j < bytes / 16; j += STPB) d4[j] = s4[j];
  } else {
    for (int64_t j = threadIdx.x; j < bytes; j += STPB) dst[j] = s[j];
  }
}

// ------------------------------------------------------------------ sort: the gathers between the passes
// after the tier pass: the primary columns in tier order
__global__ __launch_bounds__(ATPB) void k_attr_gather_primary(const int64_t* __restrict__ perm, int64_t m,
                                                              const uint8_t* __restrict__ sh, const uint64_t* __restrict__ v,
                                                              uint8_t* __restrict__ sh_o, uint64_t* __restrict__ v_o) {
  row_stream<ATPB>(m, [&](int64_t j) {
    const int64_t r = perm[j];
    v_o[j] = v[r];
    if (sh) sh_o[j] = sh[r];
  });
}
// after the primary pass: the tier columns in table order, and the composed permutation
__global__ __launch_bounds__(ATPB) void k_attr_gather_tier(const int64_t* __restrict__ perm2, int64_t m,
                                                           const int16_t* __restrict__ bin1, const int64_t* __restrict__ t1,
                                                           const int64_t* __restrict__ perm1, int16_t* __restrict__ bin_o,
                                                           int64_t* __restrict__ t_o, int64_t* __restrict__ perm_o) {
  row_stream<ATPB>(m, [&](int64_t j) {
    const int64_t r = perm2[j];
    t_o[j] = t1[r];
    if (bin1) bin_o[j] = bin1[r];
    perm_o[j] = perm1[r];
  });
}

// ------------------------------------------------------------------ scan: the table's key
// (shard, v, bin as u16, t as u64), the byte order of [shard][hex text of v][0x00][bin BE16][t BE64]; a
// column the table does not have (bin: only the Z3 tier; t: no tier) reads as 0.
struct AttrCols {
  using Key = AttrKey;
  const uint8_t* sh;
  const uint64_t* v;
  const uint16_t* bin;
  const uint64_t* t;
  __device__ __forceinline__ AttrKey at(int64_t i) const {
    return AttrKey{v[i], t ? t[i] : 0ull, ((uint32_t)(sh ? sh[i] : 0) << 16) | (bin ? bin[i] : 0u)};
  }
};

static int attr_fail(const char* who, const char* why) {
  set_error(std::string(who) + ": " + why);
  return GM_E_INVALID;
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_attr_index_key(gm_ctx* ctx, const gm_attr_column* col, int64_t n, uint64_t* v_out, int64_t* rows_out,
                      int64_t* n_rows) {
  const char* who = "gm_attr_index_key";
  if (!ctx || !col || n < 0 || !n_rows) return attr_fail(who, "ctx, col and n_rows are required, n >= 0");
  if (col->type == GM_ATTR_UTF8)
    return attr_fail(who, "GM_ATTR_UTF8: the String binding needs variable-length keys and is not built");
  if (col->type != GM_ATTR_INT32 && col->type != GM_ATTR_INT64 && col->type != GM_ATTR_FLOAT32 && col->type != GM_ATTR_FLOAT64)
    return attr_fail(who, "unknown GM_ATTR_* type");
  *n_rows = 0;
  if (n == 0) return GM_OK;
  const bool eight = col->type == GM_ATTR_INT64 || col->type == GM_ATTR_FLOAT64;
  if (!col->values || (eight ? !aligned_to<8>(col->values) : !aligned_to<4>(col->values)))
    return attr_fail(who, "the column needs its values, naturally aligned");
  if (!v_out || !rows_out || !aligned_to<8>(v_out) || !aligned_to<8>(rows_out))
    return attr_fail(who, "v_out and rows_out are required, 8-B aligned");
  ScanBufs b;
  int rc = alloc_scan(ctx, n, nullptr, 0, b);
  if (rc) return rc;
  const int64_t nblocks = (n + FROWS - 1) / FROWS;
  hipLaunchKernelGGL(k_attr_valid_mask, dim3((unsigned)nblocks), dim3(FTPB), 0, ctx->stream, col->validity,
                     col->validity_offset, n, b.mask, b.counts);
  GM_CHECK_LAUNCH();
  int64_t m = 0;
  if ((rc = finish_scan(ctx, n, b, rows_out, n, &m))) return rc;
  if (m > 0) {
    with_value<GM_ATTR_INT32, GM_ATTR_INT64, GM_ATTR_FLOAT32, GM_ATTR_FLOAT64>(col->type, [&](auto TYPE) {
      hipLaunchKernelGGL(k_attr_encode<TYPE()>, dim3(stride_grid(m, ATPB, 1 << 16)), dim3(ATPB), 0, ctx->stream,
                         col->values, (const int64_t*)rows_out, m, v_out);
    });
    GM_CHECK_LAUNCH();
  }
  *n_rows = m;
  return GM_OK;
}

int gm_attr_key_bytes(gm_ctx* ctx, int type, const uint8_t* shard, const uint64_t* v, int tier_kind, const int16_t* bin,
                      const int64_t* t, int64_t m, uint8_t* out) {
  const char* who = "gm_attr_key_bytes";
  if (!ctx || m < 0) return GM_E_INVALID;
  if (type == GM_ATTR_UTF8)
    return attr_fail(who, "GM_ATTR_UTF8: the String binding needs variable-length keys and is not built");
  if (type != GM_ATTR_INT32 && type != GM_ATTR_INT64 && type != GM_ATTR_FLOAT32 && type != GM_ATTR_FLOAT64)
    return attr_fail(who, "unknown GM_ATTR_* type");
  if (tier_kind != GM_ATTR_TIER_NONE && tier_kind != GM_ATTR_TIER_DATE && tier_kind != GM_ATTR_TIER_Z3)
    return attr_fail(who, "unknown GM_ATTR_TIER_* kind (the XZ3, Z2 and XZ2 tiers are not built)");
  if (m == 0) return GM_OK;
  if (!v || !out || (tier_kind != GM_ATTR_TIER_NONE && !t) || (tier_kind == GM_ATTR_TIER_Z3 && !bin)) return GM_E_INVALID;
  if (!aligned_to<8>(v) || !aligned_to<8>(t) || !aligned_to<2>(bin)) return attr_fail(who, "columns need natural alignment");
  const int hex = (type == GM_ATTR_INT32 || type == GM_ATTR_FLOAT32) ? 8 : 16;
  const int klen = (shard ? 1 : 0) + hex + 1 + (tier_kind == GM_ATTR_TIER_DATE ? 8 : tier_kind == GM_ATTR_TIER_Z3 ? 10 : 0);
  with_value<8, 16>(hex, [&](auto HEX) {
    hipLaunchKernelGGL(k_attr_key_bytes<HEX()>, dim3((unsigned)((m + STPB - 1) / STPB)), dim3(STPB), 0, ctx->stream, shard,
                       v, tier_kind, bin, t, m, klen, out);
  });
  GM_CHECK_LAUNCH();
  return GM_OK;
}

int gm_attr_sort(gm_ctx* ctx, const uint8_t* shard, const uint64_t* v, const int16_t* bin, const int64_t* t, int64_t m,
                 uint8_t* shard_out, uint64_t* v_out, int16_t* bin_out, int64_t* t_out, int64_t* perm_out) {
  if (!ctx || m < 0 || m > (int64_t)UINT32_MAX) return GM_E_INVALID;
  if (m == 0) return GM_OK;
  if (!v || !v_out || !perm_out || ((shard == nullptr) != (shard_out == nullptr)) ||
      ((bin == nullptr) != (bin_out == nullptr)) || ((t == nullptr) != (t_out == nullptr)) || (bin && !t))
    return GM_E_INVALID;
  if (!aligned_to<8>(v) || !aligned_to<8>(v_out) || !aligned_to<8>(t) || !aligned_to<8>(t_out) || !aligned_to<8>(perm_out) ||
      !aligned_to<2>(bin) || !aligned_to<2>(bin_out))
    return attr_fail("gm_attr_sort", "columns and outputs need natural alignment");
  if (!t)   // no tier: the key is (shard, v)
    return gm_sort_keys(ctx, shard, nullptr, (const int64_t*)v, m, shard_out, nullptr, (int64_t*)v_out, perm_out);
  // by tier (stable), the primary columns gathered into that order, by (shard, v) (stable): ties of the
  // primary key keep the tier order, ties of the whole key the input order
  hipStream_t s = ctx->stream;
  DevTemps tmp(s);
  int16_t* bin1 = nullptr;
  int64_t *t1 = nullptr, *perm1 = nullptr, *perm2 = nullptr;
  uint64_t* v1 = nullptr;
  uint8_t* sh1 = nullptr;
  int rc = tmp.alloc_async((size_t)m * 8, &t1);
  if (!rc) rc = tmp.alloc_async((size_t)m * 8, &perm1);
  if (!rc) rc = tmp.alloc_async((size_t)m * 8, &perm2);
  if (!rc) rc = tmp.alloc_async((size_t)m * 8, &v1);
  if (!rc && bin) rc = tmp.alloc_async((size_t)m * 2, &bin1);
  if (!rc && shard) rc = tmp.alloc_async((size_t)m, &sh1);
  if (rc) return rc;
  if ((rc = gm_sort_keys(ctx, nullptr, bin, t, m, nullptr, bin1, t1, perm1))) return rc;
  const dim3 grid(stride_grid(m, ATPB, 1 << 16));
  hipLaunchKernelGGL(k_attr_gather_primary, grid, dim3(ATPB), 0, s, (const int64_t*)perm1, m, shard, v, sh1, v1);
  GM_CHECK_LAUNCH();
  if ((rc = gm_sort_keys(ctx, sh1, nullptr, (const int64_t*)v1, m, shard_out, nullptr, (int64_t*)v_out, perm2))) return rc;
  hipLaunchKernelGGL(k_attr_gather_tier, grid, dim3(ATPB), 0, s, (const int64_t*)perm2, m, (const int16_t*)bin1,
                     (const int64_t*)t1, (const int64_t*)perm1, bin_out, t_out, perm_out);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

int gm_attr_table_scan(gm_ctx* ctx, const uint8_t* shard, const uint64_t* v, const int16_t* bin, const int64_t* t,
                       int64_t m, const gm_attr_range* ranges, int64_t n_ranges, const gm_scan_filter* f,
                       const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned) {
  const char* who = "gm_attr_table_scan";
  if (!ctx || m < 0 || n_ranges < 0 || (n_ranges > 0 && !ranges) || ids_cap < 0) return GM_E_INVALID;
  if (m > 0 && (!v || (bin && !t))) return GM_E_INVALID;
  if (!aligned_to<8>(v) || !aligned_to<8>(t) || !aligned_to<2>(bin) || !aligned_to<8>(perm) || !aligned_to<8>(ids))
    return attr_fail(who, "columns and outputs need natural alignment");
  gm_scan_filter none{};
  if (!f) f = &none;
  if (f->z3filter || f->z2filter) return attr_fail(who, "a Z3Filter or Z2Filter: the attribute table has no row filter");
  if (f->polys) return attr_fail(who, "polys: the secondary filter is boxes and during");
  if (!full_filter_ok(f)) return GM_E_INVALID;
  // a column the table lacks reads as 0, and so do its range fields
  std::vector<SeekRange<AttrKey>> rs;
  rs.reserve((size_t)n_ranges);
  for (int64_t i = 0; i < n_ranges; ++i) {
    const gm_attr_range& r = ranges[i];
    const uint32_t s16 = (uint32_t)r.shard << 16;
    rs.push_back(SeekRange<AttrKey>{AttrKey{r.v_lo, t ? r.t_lo : 0ull, s16 | (bin ? r.b_lo : 0u)},
                                    AttrKey{r.v_hi, t ? r.t_hi : 0ull, s16 | (bin ? r.b_hi : 0u)}});
  }
  const std::vector<SeekRange<AttrKey>> dr = merge_ranges(std::move(rs));
  const int64_t nr = (int64_t)dr.size();
  if (m == 0 || nr == 0) return no_candidates(n_match, n_scanned, nullptr);
  DevTemps tmp(ctx->stream);
  int64_t *start = nullptr, *coff = nullptr;
  const int rc = seek_ranges(ctx, tmp, AttrCols{shard, v, (const uint16_t*)bin, (const uint64_t*)t}, m, dr, &start, &coff);
  if (rc) return rc;
  const std::vector<int32_t> no_words;
  const RowFilter row_filter{RF_NONE, 0, &no_words, nullptr, nullptr};
  return scan_candidates(ctx, tmp, start, coff, nr, f, row_filter, nullptr, nullptr, perm, ids, ids_cap, n_match,
                         n_scanned, nullptr);
}

}  // extern "C"
