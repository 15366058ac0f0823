// gm_ranges.hpp -- what the batched-ranges units share: the per-query status codes, the batch output
// that the walk kernels (gm_ranges_z.hip, gm_ranges_xz.hip) append to, and the interface of the host
// batch driver (gm_ranges.hip).
#pragma once

#include <functional>

#include "gm_internal.hpp"

namespace gm {

#ifndef GM_RTPB
#define GM_RTPB 512
#endif
constexpr int RTPB = GM_RTPB;   // threads per workgroup of the Z walk (one query each) and of the gather
constexpr int MAXB = 256;       // zbounds / windows per query
#ifndef GM_LDS_SORT
#define GM_LDS_SORT 4096
#endif
constexpr int LDS_SORT = GM_LDS_SORT;  // ranges sorted in LDS; larger lists sort in global memory

enum : int32_t { QS_OK = 0, QS_OUT_OF_BOUNDS = 1, QS_UNORDERED = 3, QS_CAPACITY = 4, QS_TOO_MANY_BOUNDS = 5 };

// Batch output: every query's merged ranges are appended to one device buffer (one atomic per query)
// with their (start, count) recorded by query index; the host driver then scans the counts and
// gathers the buffer into query order.  Phase 2 re-runs the queries whose first-pass workspace
// overflowed, through qmap.
struct BatchOut {
  const int32_t* qmap;           // block -> query index (phase 2), null: q0 + block
  int64_t q_base;                // the batch's first query: start / count / status are indexed by q - q_base
  gm_range* dbuf;                // batch buffer
  int64_t dcap;
  unsigned long long* total;
  int64_t* start;                // per query of the batch
  int32_t* count;
  int32_t* status;
};

__device__ __forceinline__ int64_t batch_query(const BatchOut& bo, int64_t q0, int64_t qc) {
  return bo.qmap ? (int64_t)bo.qmap[qc] : q0 + qc;
}

// record query q's result: its m ranges start at `start` of the batch buffer (one thread calls it)
__device__ __forceinline__ void batch_record(const BatchOut& bo, int64_t q, int64_t start, int64_t m, int status) {
  const int64_t i = q - bo.q_base;
  bo.start[i] = start;
  bo.count[i] = status == QS_OK ? (int32_t)m : 0;
  bo.status[i] = status;
}

// What a curve family hands the driver.  The driver runs every query with small workspaces first and
// the overflowing ones again with the worst-case caps, in chunks that fit a memory budget: it asks
// per_query for a chunk's workspace bytes per query and calls launch once per chunk.
struct RangesFamily {
  int64_t fcap, rcap;   // worst-case frontier / range-list capacity of one query
  std::function<int64_t(int64_t fc, int64_t rc)> per_query;
  // queries [q0, q0 + m) (or bo.qmap[0, m) when set) with caps (fc, rc) in the workspace `ws`
  std::function<void(int64_t q0, int64_t m, int64_t fc, int64_t rc, char* ws, const BatchOut& bo)> launch;
};

// the output arguments of a ranges entry point (include/geomesa_hip.h)
struct RangesOut {
  int64_t* off;           // [nq + 1]
  gm_range* out;          // cap ranges, device or host memory
  int64_t cap;
  int64_t* needed;        // may be null, and so may query_status [nq]
  int32_t* query_status;
};

int run_ranges(gm_ctx* ctx, int64_t nq, const RangesFamily& fam, const RangesOut& o);

// the answer of a ranges entry point to nq == 0
inline int empty_ranges(int64_t* out_off, int64_t* needed) { out_off[0] = 0; if (needed) *needed = 0; return GM_OK; }

// a stream-ordered input copy of one entry point into *d, freed by `tmp` on every return path
template <class T>
int to_dev(gm_ctx* ctx, DevTemps& tmp, const T* h, size_t n, const T** d) {
  T* p = nullptr;
  const int rc = tmp.alloc_async(n * sizeof(T), &p);
  *d = p;
  return rc ? rc : copy_h2d(ctx, p, h, n * sizeof(T));
}

inline int stop_of(int max_ranges) { return max_ranges <= 0 ? INT32_MAX : max_ranges; }

}  // namespace gm
