// gm_internal.hpp -- context, error plumbing and launch helpers shared by the libgeomesa_hip units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/geomesa_hip.h"
#include "gm_device.hpp"
#include "gm_dispatch.hpp"

struct gm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int64_t* d_err = nullptr;        // [0] error count, [1] packed (first index << 8 | code)
  int64_t* d_scratch = nullptr;    // small device scratch: counters
  int64_t* h_pinned = nullptr;     // pinned host mirror for summaries / counters
  char* h_stage = nullptr;         // pinned staging for copies to / from pageable host memory (2 halves)
  void* ws[4] = {nullptr, nullptr, nullptr, nullptr};   // reusable device workspaces (see ctx_workspace)
  size_t ws_cap[4] = {0, 0, 0, 0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int64_t join_chunk = 0;          // GM_PARAM_JOIN_CHUNK: rows per join pass (0 = default, 2^31)
  int64_t index_build = 0;         // GM_PARAM_INDEX_BUILD: 0 = device build of the join index, 1 = host build
  int64_t ranges_hint = 0;         // largest batched-ranges output seen (sizes the device batch buffer)
  int64_t ranges_chunk = 0;        // GM_PARAM_RANGES_CHUNK: queries per pipelined chunk (0 = default)
  int64_t sort_last = 0;           // GM_PARAM_SORT_LAST (read-only): the last sort's digit passes | 256 if ranked locally
  int64_t sort_mode = 0;           // GM_PARAM_SORT_MODE: 0 = auto (prefix passes + local ranks), 1 = digit passes only
  int64_t index_coarse = -1;       // GM_PARAM_INDEX_COARSE: the join's coarse sub-block masks (-1 = automatic)
  int64_t hist_grid = 0;           // GM_PARAM_HIST_GRID: Z3Histogram LDS-kernel workgroups (0 = default)
  int64_t relate_rows64 = 0;       // GM_PARAM_RELATE_ROWS64: the row predicate's 64-bit-row kernel always
  uint32_t fault_calls = 0;        // FC_* bits: the entry points that enqueued reference-checked kernels
                                   // since the fault word was last read (take_fault names them)
  hipStream_t copy_stream = nullptr;   // result copies overlapping the next chunk's kernels (lazy)
  hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
};

namespace gm {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define GM_HIP(expr)                                   \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return gm::hip_fail(_e, #expr); \
  } while (0)

#define GM_CHECK_LAUNCH() GM_HIP(hipGetLastError())

// device-side element error report: called only by failing lanes (rare path)
__device__ __forceinline__ void report_error(int64_t* err, int64_t idx, uint8_t code) {
  atomicAdd((unsigned long long*)&err[0], 1ull);
  atomicMin((long long*)&err[1], (long long)((idx << 8) | code));
}

// Host <-> device copies of caller host memory.  Pinned (hipHostMalloc'd / registered) memory is
// copied directly; pageable memory goes through the context's pinned staging buffer in
// double-buffered pieces (direct DMA to pageable memory degrades badly on this stack: a 256 MB
// result copy took 0.3-7 s and grew from call to call, against 80 ms through pinned memory).
// Both synchronise the context stream.
int copy_d2h(gm_ctx* ctx, void* host, const void* dev, size_t bytes);
int copy_h2d(gm_ctx* ctx, void* dev, const void* host, size_t bytes);

// A device workspace owned by the context, grown on demand and reused by later calls (calls on
// one context are stream-ordered, so reuse is safe).  Large per-call temporaries come from here
// rather than hipMallocAsync: on this stack multi-GB pool allocations were re-mapped on every call
// (0.7-6 s stalls between launches).  slot: 0 = range batches, 1 = sort, 2 = scans, 3 = join.
enum : int { WS_RANGES = 0, WS_SORT = 1, WS_SCAN = 2, WS_JOIN = 3 };
int ctx_workspace(gm_ctx* ctx, int slot, size_t bytes, void** p);

// Region offsets of one workspace request: take() returns the region's offset and advances `total` by
// its size rounded up to `align`, so the sum asked of ctx_workspace and the pointers formed from its
// base come from the same calls.
struct Carve {
  size_t align, total = 0;
  constexpr size_t take(size_t bytes) {
    const size_t at = total;
    total += (bytes + align - 1) / align * align;
    return at;
  }
};
namespace carve_check {
constexpr Carve a16{16}, a256{256};
constexpr size_t offs(Carve c, size_t x, size_t y, size_t z, int k) {
  const size_t o[4] = {c.take(x), c.take(y), c.take(z), c.total};
  return o[k];
}
static_assert(offs(a16, 1, 16, 17, 0) == 0 && offs(a16, 1, 16, 17, 1) == 16 && offs(a16, 1, 16, 17, 2) == 32 &&
                  offs(a16, 1, 16, 17, 3) == 64, "sizes round up to the alignment");
static_assert(offs(a256, 8, 257, 256, 1) == 256 && offs(a256, 8, 257, 256, 2) == 768 &&
                  offs(a256, 8, 257, 256, 3) == 1024, "256-B regions");
static_assert(offs(a16, 0, 8, 0, 1) == 0 && offs(a16, 0, 8, 0, 2) == 16 && offs(a16, 0, 8, 0, 3) == 16,
              "an empty region takes no bytes");
static_assert(offs(a16, 3, 5, 7, 3) % 16 == 0 && offs(a256, 3, 5, 7, 3) % 256 == 0, "totals stay aligned");
}  // namespace carve_check

// Owner of one call's device temporaries: every buffer it hands out is freed when it goes out of
// scope, so no return path (the ones inside GM_HIP / GM_CHECK_LAUNCH included) leaks.  alloc buffers
// leave through hipFree, which waits for the device; alloc_async buffers come from the stream's pool
// and leave stream-ordered.  Either is safe after work enqueued on the stream.  Buffers that outlive
// the call (index arrays) are not allocated here.
class DevTemps {
 public:
  explicit DevTemps(hipStream_t s) : s_(s) {}
  DevTemps(const DevTemps&) = delete;
  DevTemps& operator=(const DevTemps&) = delete;
  ~DevTemps() {
    for (const Buf& b : bufs_) (void)(b.async ? hipFreeAsync(b.p, s_) : hipFree(b.p));
  }
  template <class T>
  int alloc(size_t bytes, T** p) {
    GM_HIP(hipMalloc((void**)p, bytes < 16 ? 16 : bytes));
    bufs_.push_back(Buf{*p, false});
    return GM_OK;
  }
  template <class T>
  int alloc_async(size_t bytes, T** p) {
    GM_HIP(hipMallocAsync((void**)p, bytes < 16 ? 16 : bytes, s_));
    bufs_.push_back(Buf{*p, true});
    return GM_OK;
  }

 private:
  struct Buf {
    void* p;
    bool async;
  };
  hipStream_t s_;
  std::vector<Buf> bufs_;
};

// one int64 of device memory (a scan's total, a counter) through h_pinned[0]; synchronises the stream
inline int read_i64(gm_ctx* ctx, const void* dev, int64_t* host) {
  GM_HIP(hipMemcpyAsync(ctx->h_pinned, dev, 8, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(hipStreamSynchronize(ctx->stream));
  *host = ctx->h_pinned[0];
  return GM_OK;
}

bool host_pinned(const void* p);
bool device_memory(const void* p);   // device (hipMalloc) memory, as opposed to host memory
int ctx_copy_stream(gm_ctx* ctx);   // creates copy_stream and its events on first use

// The context's sticky reference-fault word (d_scratch[SCRATCH_FAULT]): the polygon-index kernels OR
// PIP_FAULT_* bits into it, stream-ordered; take_fault (a synchronising call: a join that returns its
// pair count, a query scan, gm_ctx_sync) reads and clears it and returns GM_E_INDEX when set.
// A stream-ordered call (gm_pip_relate, a join without n_pairs) leaves its bits for a later
// synchronising call, so each call that enqueues checked kernels records itself (note_fault_call) and
// the error text names every such call since the last read, not only the call that read the word.
constexpr int SCRATCH_FAULT = 63;
enum : uint32_t { FC_JOIN = 1, FC_JOIN_ARROW = 2, FC_RELATE = 4, FC_QUERY = 8 };
inline void note_fault_call(gm_ctx* ctx, uint32_t fc) { ctx->fault_calls |= fc; }
int take_fault(gm_ctx* ctx, const char* what);

// reset the error summary before a call that reports one
int begin_summary(gm_ctx* ctx, gm_batch_status* summary);
// read the summary back (synchronises the stream).  GM_E_ELEMENT when an element failed and the
// caller gave no status[] to find it in; GM_OK otherwise, and always without a summary (asynchronous)
int end_summary(gm_ctx* ctx, gm_batch_status* summary, const uint8_t* status);

// Resident block count of `kernel` at `block` threads per block on `device`: occupancy x CUs,
// computed once per (kernel, device) under a lock (contexts on different devices and concurrent
// callers are safe); `fallback_per_cu` when the occupancy query fails.
int resident_blocks(const void* kernel, int device, int block, int fallback_per_cu);

template <unsigned N>
inline bool aligned_to(const void* p) { return ((uintptr_t)p & (N - 1)) == 0; }   // a null pointer is aligned
inline bool aligned16(const void* p) { return aligned_to<16>(p); }

inline unsigned grid_for(int64_t n, int64_t per_block) {
  int64_t b = (n + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b);
}

// grid of a pair kernel (one lane per two rows); a single row still gets its block
inline unsigned pair_grid(int64_t n, int64_t pairs_per_block) {
  return grid_for((n >> 1) > 0 ? (n >> 1) : 1, pairs_per_block);
}

// the answer of an indexing entry point to n == 0
inline int empty_batch(gm_batch_status* summary) {
  if (summary) *summary = gm_batch_status{0, -1, 0, 0};
  return GM_OK;
}

}  // namespace gm
