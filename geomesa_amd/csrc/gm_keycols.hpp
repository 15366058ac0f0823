// gm_keycols.hpp -- what the sort (gm_sort.hip) and the table's other key passes (gm_key_table.hip) share:
// the caller's key columns.  All of it is inlined into the kernels of the including unit: no device code
// crosses units.
#pragma once

#include "gm_internal.hpp"

namespace gm {

constexpr int STPB = 256;   // threads per block of the row-per-thread kernels (k_key_bytes, k_widen_perm)

// The caller's columns.  bs = bin | shard << 16.
struct KeyCols {
  const uint8_t* sh; const uint16_t* bin; const uint64_t* z;
  template <bool SH>
  __device__ __forceinline__ uint32_t bs(int64_t r) const { return (uint32_t)bin[r] | (SH ? (uint32_t)sh[r] << 16 : 0u); }
};

__device__ __forceinline__ uint64_t lanemask_lt() {   // the lanes below mine
  const int lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

}  // namespace gm
