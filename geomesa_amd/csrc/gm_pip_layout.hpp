// gm_pip_layout.hpp -- the bytes of the polygon index (gm_pip.hpp): the location codes, the ring /
// slab records, the cell-word encoding, the blob records, and the order of the exported arrays and
// counters.  No HIP include: the host build (gm_pip_build_host.hpp) and its host-only check
// (tools/pip_host_build_check.cpp) compile with a plain C++ compiler and see the definitions the
// kernels see.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GM_HOST_DEVICE __host__ __device__
#else
#define GM_HOST_DEVICE
#endif

namespace gm {

enum : int { LOC_EXTERIOR = 0, LOC_BOUNDARY = 1, LOC_INTERIOR = 2 };

struct RingDev {
  double minx, miny, maxx, maxy;  // ring envelope (empty ring: +inf/-inf)
  double y0, inv_h;               // slab(y) = clamp(floor((y - y0) * inv_h), 0, ns - 1)
  int32_t ns, slab_base;          // slab_off[slab_base .. slab_base + ns]
};

struct Edge {
  double p1x, p1y, p2x, p2y;  // countSegment(p1 = ring[i], p2 = ring[i-1])
};

#ifndef GM_CF_LOG
#define GM_CF_LOG 3
#endif
#ifndef GM_MAX_CELLS_LOG
#define GM_MAX_CELLS_LOG 26
#endif
constexpr int CF_LOG = GM_CF_LOG;   // coarse cell = 8 x 8 fine cells: the coarse table (<= 4 MB) stays L2-resident

// cell word kinds (2 high bits; 30-bit payload)
enum : uint32_t { CELL_INTERIOR = 0, CELL_BOUNDARY = 1, CELL_LIST = 2, CELL_EMPTY = 3 };
// BOUNDARY payload: bit 29 set = compact blob index, else generic blob offset (16-B units)
constexpr uint32_t BLOB_COMPACT = 1u << 29;
// LIST payload: list_ent offset << 4 | count; count 15 = long list whose count is list_ent[offset]
constexpr int LIST_LONG = 15;

// Compact blob (single-ring polygon, 4 * segments + breakpoints <= 30 in the cell): one or two
// 128-B lines of 16 words in `compact`, addressed by line index.
//   w0: int32 polygon | int32 meta (segments | lines << 8), w1: parity bits,
//   segment j (p1x p1y p2x p2y) at words CSEG[j] = 2, 6, 10 (line 0), 16, 20, 24, 28 (line 1);
//   every other word of the record is a breakpoint slot (+inf when unused).
// The breakpoint count k = #(slots <= y) does not depend on slot order, so the record is evaluated
// with static indexing, line by line: crossings = parity bit k + segment crossings, exactly the
// RayCrossingCounter walk of a generic one-ring blob.
constexpr int CSEG_MAX = 7;
GM_HOST_DEVICE constexpr int cseg_word(int j) { return j < 3 ? 2 + 4 * j : 16 + 4 * (j - 3); }

// Generic blob (16-B aligned in `blob`): w0 = int32 polygon | int32 rings, then per ring a RingHdr
// word, a parity word (a slab-walk ring, flags & 2: its ring id), n_edge segments of 4 words and
// n_brk breakpoints; flags & 1 = the ring is a part's shell
struct RingHdr {
  int16_t n_edge, n_brk, flags, pad;
};

// the device arrays of an index in gm_pip_index_layout order (bytes[k], gm_pip_index_copy_array's k)
enum : int { ARR_RINGS = 0, ARR_SLAB_OFF, ARR_SLAB_EDGES, ARR_CELL_WORD, ARR_COARSE_WORD, ARR_COMPACT, ARR_LIST_ENT,
             ARR_BLOB, ARR_COUNT };
// the counters of an index in gm_pip_index_layout.stats order; gm_pip_index_stats reports the first ST_PUBLIC
enum : int { ST_CELLS = 0, ST_ENTRIES, ST_BOUNDARY, ST_RECORDS, ST_SLOW, ST_BLOB_BYTES, ST_COMPACT,
             ST_MAX_BND_PER_CELL,   // most BOUNDARY (cell, polygon) entries of any cell
             ST_MAX_ENT_PER_CELL,   // most (cell, polygon) entries of any cell
             ST_COUNT, ST_PUBLIC = ST_COMPACT + 1 };

}  // namespace gm
