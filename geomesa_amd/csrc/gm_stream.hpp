// gm_stream.hpp -- the two loop shapes of the element-wise key kernels (gm_curve.hip, gm_arrow.hip,
// gm_legacy.hip), their status epilogues and their grids.  A kernel supplies only its per-element body.
#pragma once

#include "gm_internal.hpp"

namespace gm {

// Pair shape: lane l of block b takes the pairs b * TPB * UNROLL + u * TPB + l, u < UNROLL (rows 2p and
// 2p + 1 as one 16-B load / store per column), fully coalesced per wave instruction; one chunk per block.
//   load(u, p)  stages pair p into the kernel's own register arrays, slot u; all of a lane's loads are
//               issued before any pair is computed, each under its guard (gm_keys.hpp, ld_stream);
//   pair(u, p)  computes pair p from slot u and stores it;
//   tail(i)     the odd last row i = n - 1, on lane 0 of block 0.
// The two Z3 key kernels with LDS-staged bins (k_z3_index_key, k_z3_key_arrow_v) have this shape written
// out: they measured slower on the skeleton (profiles/stream_skeleton_ab.txt).
template <int TPB, int UNROLL, class Load, class Pair, class Tail>
__device__ __forceinline__ void pair_stream(int64_t n, Load load, Pair pair, Tail tail) {
  const int64_t npairs = n >> 1;
  const int64_t base = (int64_t)blockIdx.x * (TPB * UNROLL) + threadIdx.x;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int64_t p = base + (int64_t)u * TPB;
    if (p < npairs) load(u, p);
  }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int64_t p = base + (int64_t)u * TPB;
    if (p < npairs) pair(u, p);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) tail(n - 1);
}

// Row shape: row(i) for every i < n, grid-stride (the grid is stride_grid's, clamped).
template <int TPB, class Row>
__device__ __forceinline__ void row_stream(int64_t n, Row row) {
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) row(i);
}

// Status epilogues.  `store` is the kernel's STATUS template flag (folded) or, in the Arrow and legacy
// kernels, `status != nullptr`.
__device__ __forceinline__ void finish_row(bool store, uint8_t* __restrict__ status, int64_t* __restrict__ err,
                                           int64_t i, uint8_t s) {
  if (store) status[i] = s;
  if (s) report_error(err, i, s);
}
__device__ __forceinline__ void finish_pair(bool store, uchar2* __restrict__ status, int64_t* __restrict__ err,
                                            int64_t p, uint8_t s0, uint8_t s1) {
  if (store) status[p] = make_uchar2(s0, s1);
  if (s0) report_error(err, 2 * p, s0);
  if (s1) report_error(err, 2 * p + 1, s1);
}

// grid of a row_stream kernel: one lane per unit, at most `cap` blocks
inline unsigned stride_grid(int64_t units, int tpb, int64_t cap) {
  const int64_t b = (units + tpb - 1) / tpb;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace gm
