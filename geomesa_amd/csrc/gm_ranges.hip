// gm_ranges.hip -- host driver of the batched range decompositions (gm_ranges.hpp): runs a curve
// family's walk kernel (gm_ranges_z.hip: Z2 / Z3, gm_ranges_xz.hip: XZ2 / XZ3) over a batch of queries
// and delivers the ranges in query order, into device memory, host memory or, pipelined in query
// chunks, pinned host memory.
#include <string.h>

#include <algorithm>
#include <vector>

#include "gm_ranges.hpp"
#include "gm_scan.hpp"

namespace gm {

// gather every query's ranges from the batch buffer into query order (one block per query)
__global__ __launch_bounds__(RTPB) void k_gather_ranges(const gm_range* __restrict__ buf, const int64_t* __restrict__ start,
                                                        const int64_t* __restrict__ off, int64_t nq,
                                                        gm_range* __restrict__ out) {
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const int64_t a = off[q], n = off[q + 1] - a, s = start[q];
    for (int64_t j = threadIdx.x; j < n; j += RTPB) out[a + j] = buf[s + j];
  }
}

namespace {

inline int64_t next_pow2(int64_t v) { int64_t p = 1; while (p < v) p <<= 1; return p; }

// What run_batch computed, in the context's scan workspace (valid until the next batch): the batch
// buffer, every query's start in it and the query-order offsets.
struct Batch {
  int64_t total = 0;        // ranges of the batch
  const gm_range* dbuf = nullptr;
  const int64_t *dstart = nullptr, *doff = nullptr;
  bool failed = false;      // a query's status is not QS_OK
};

// One batch, queries [q_base, q_base + nq).  Phase 1 runs every query with small workspaces (frontier /
// range lists of P1CAP, sorted in LDS), chunked only by a memory budget and launched back to back (the
// chunks reuse one stream-ordered workspace, no host round trip).  Phase 2 re-runs the queries that
// overflowed it (status QS_CAPACITY) with the worst-case caps.  Then the counts are scanned on the
// device into the query-order offsets (out_off, host) and the statuses are read back.
constexpr int64_t P1CAP = LDS_SORT;

int run_batch(gm_ctx* ctx, const RangesFamily& fam, int64_t q_base, int64_t nq, int64_t* out_off, int64_t cap,
              int32_t* query_status, Batch& b) {
  const int64_t fcap = fam.fcap, rcap = next_pow2(std::max<int64_t>(fam.rcap, 16));
  size_t free_b = 0, total_b = 0;
  int64_t budget = (int64_t)2 << 30;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
    budget = std::max<int64_t>(budget, std::min<int64_t>((int64_t)16 << 30, (int64_t)(free_b / 4)));
  // batch buffer: sized from the largest output seen on this context (at least 64 ranges a query),
  // bounded by the caller's capacity and the budget; a batch whose ranges overflow it but fit `cap`
  // runs once more with the exact size
  int64_t dcap = std::min<int64_t>(std::max<int64_t>({(int64_t)1 << 20, nq * 64, ctx->ranges_hint}),
                                   budget / (int64_t)sizeof(gm_range));
  dcap = std::max<int64_t>(1, std::min<int64_t>(cap, dcap));
  std::vector<int32_t> stats((size_t)nq);
  for (int attempt = 0;; ++attempt) {
    // batch arrays (scan workspace): buffer | start | offsets | count | status | qmap | scan partials | total
    Carve c{16};
    const size_t o_buf = c.take((size_t)dcap * sizeof(gm_range)), o_start = c.take((size_t)nq * 8),
                 o_off = c.take((size_t)(nq + 1) * 8), o_count = c.take((size_t)nq * 4), o_status = c.take((size_t)nq * 4),
                 o_qmap = c.take((size_t)nq * 4), o_parts = c.take((size_t)scan_partials_len(nq) * 8), o_total = c.take(16);
    char* wb = nullptr;
    int wrc = ctx_workspace(ctx, WS_SCAN, c.total, (void**)&wb);
    if (wrc) return wrc;
    gm_range* dbuf = (gm_range*)(wb + o_buf);
    int64_t *dstart = (int64_t*)(wb + o_start), *doff = (int64_t*)(wb + o_off), *dparts = (int64_t*)(wb + o_parts);
    int32_t *dcount = (int32_t*)(wb + o_count), *dstatus = (int32_t*)(wb + o_status), *dqmap = (int32_t*)(wb + o_qmap);
    unsigned long long* dtotal = (unsigned long long*)(wb + o_total);
    GM_HIP(hipMemsetAsync(dtotal, 0, 8, ctx->stream));
    // one pass over a query list with caps (fc, rc); qmap null = queries [q_base, q_base + count).  The
    // family's workspace is per_query(fc, rc) bytes per query, chunked by the memory budget
    auto pass = [&](int64_t count, const int32_t* qmap, int64_t fc, int64_t rc) -> int {
      const int64_t per_q = std::max<int64_t>(16, fam.per_query(fc, rc));
      int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, budget / per_q));
      chunk = std::min<int64_t>(chunk, (int64_t)1 << 20);
      const int64_t m_max = std::min(chunk, count);
      void* base = nullptr;
      int wrc = ctx_workspace(ctx, WS_RANGES, (size_t)(m_max * per_q), &base);
      if (wrc) return wrc;
      for (int64_t q0 = 0; q0 < count; q0 += chunk) {
        const int64_t m = std::min(chunk, count - q0);
        const BatchOut bo{qmap ? qmap + q0 : nullptr, q_base, dbuf, dcap, dtotal, dstart, dcount, dstatus};
        fam.launch(qmap ? 0 : q_base + q0, m, fc, rc, (char*)base, bo);
        GM_CHECK_LAUNCH();
      }
      return GM_OK;
    };
    int rc = pass(nq, nullptr, std::min<int64_t>(fcap, P1CAP), std::min<int64_t>(rcap, P1CAP));
    if (rc) return rc;
    if (fcap > P1CAP || rcap > P1CAP) {
      rc = copy_d2h(ctx, stats.data(), dstatus, (size_t)nq * 4);
      if (rc) return rc;
      std::vector<int32_t> redo;
      for (int64_t i = 0; i < nq; ++i)
        if (stats[i] == QS_CAPACITY) redo.push_back((int32_t)(q_base + i));
      if (!redo.empty()) {
        rc = copy_h2d(ctx, dqmap, redo.data(), redo.size() * 4);
        if (!rc) rc = pass((int64_t)redo.size(), dqmap, fcap, rcap);
        if (rc) return rc;
      }
    }
    // device scan of the counts -> query-order offsets (total in out_off[nq])
    launch_excl_scan(ctx->stream, dcount, nq, doff, dparts, doff + nq);
    GM_CHECK_LAUNCH();
    rc = copy_d2h(ctx, out_off, doff, (size_t)(nq + 1) * 8);
    if (!rc) rc = copy_d2h(ctx, stats.data(), dstatus, (size_t)nq * 4);
    if (rc) return rc;
    const int64_t total = out_off[nq];
    ctx->ranges_hint = std::max(ctx->ranges_hint, std::min(total, cap));
    if (total > dcap && total <= cap && attempt == 0) {
      dcap = total;
      continue;
    }
    if (query_status) memcpy(query_status, stats.data(), (size_t)nq * 4);
    b = Batch{total, dbuf, dstart, doff, std::any_of(stats.begin(), stats.end(), [](int32_t st) { return st != QS_OK; })};
    return GM_OK;
  }
}

// the batch's ranges in query order into dst (device memory, b.total ranges), on the context stream
int gather(gm_ctx* ctx, const Batch& b, int64_t nq, gm_range* dst) {
  hipLaunchKernelGGL(k_gather_ranges, dim3((unsigned)std::min<int64_t>(nq, 65536)), dim3(RTPB), 0, ctx->stream, b.dbuf,
                     b.dstart, b.doff, nq, dst);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

// all nq queries as one batch: *needed and GM_E_CAPACITY from its total
int whole_batch(gm_ctx* ctx, const RangesFamily& fam, int64_t nq, const RangesOut& o, Batch& b) {
  const int rc = run_batch(ctx, fam, 0, nq, o.off, o.cap, o.query_status, b);
  if (rc) return rc;
  if (o.needed) *o.needed = b.total;
  return b.total > o.cap ? GM_E_CAPACITY : GM_OK;
}

// device output (ranges consumed on the device): gathered in place
int to_device(gm_ctx* ctx, const RangesFamily& fam, int64_t nq, const RangesOut& o, Batch& b) {
  int rc = whole_batch(ctx, fam, nq, o, b);
  if (rc || b.total == 0) return rc;
  rc = gather(ctx, b, nq, o.out);
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(ctx->stream));
  return GM_OK;
}

// host output in one batch: gathered into the range workspace (free again after the walk), one copy
int to_host(gm_ctx* ctx, const RangesFamily& fam, int64_t nq, const RangesOut& o, Batch& b) {
  int rc = whole_batch(ctx, fam, nq, o, b);
  if (rc || b.total == 0) return rc;
  void* dout = nullptr;
  rc = ctx_workspace(ctx, WS_RANGES, (size_t)b.total * sizeof(gm_range), &dout);
  if (!rc) rc = gather(ctx, b, nq, (gm_range*)dout);
  return rc ? rc : copy_d2h(ctx, o.out, dout, (size_t)b.total * sizeof(gm_range));
}

// The pipelined path's two device result buffers, reused every other chunk once their copy is done
// (ev_copied).  They are used across two streams, so they come from hipMalloc and not the stream's
// pool; leaving the scope on any path waits for the copy stream and frees them.
struct ResultBufs {
  hipStream_t copy_stream;
  gm_range* p[2] = {nullptr, nullptr};
  int64_t cap[2] = {0, 0};
  bool used[2] = {false, false};
  ~ResultBufs() {
    (void)hipStreamSynchronize(copy_stream);
    for (int k = 0; k < 2; ++k) if (p[k]) (void)hipFree(p[k]);
  }
  // room for n ranges in buffer k (its last copy is done); the stream `s` is drained before a regrow
  int reserve(int k, int64_t n, hipStream_t s) {
    if (cap[k] >= n) return GM_OK;
    GM_HIP(hipStreamSynchronize(s));
    if (p[k]) (void)hipFree(p[k]);
    p[k] = nullptr; cap[k] = 0;
    GM_HIP(hipMalloc(&p[k], (size_t)n * sizeof(gm_range)));
    cap[k] = n;
    return GM_OK;
  }
};

// Pinned host output with enough queries: the queries run in chunks of qc and chunk k's result copy (a
// second stream) overlaps chunk k + 1's kernels: the copy back of 10^7-10^8 ranges costs as much as
// their computation.  The output is identical to one batch's.  `sum` takes the total and the failure flag.
int to_pinned(gm_ctx* ctx, const RangesFamily& fam, int64_t nq, int64_t qc, const RangesOut& o, Batch& sum) {
  int rc = ctx_copy_stream(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream, cs = ctx->copy_stream;
  int64_t base = 0;
  {
    ResultBufs res{cs};
    std::vector<int64_t> off_c;
    int k = 0;
    for (int64_t c0 = 0; c0 < nq; c0 += qc, k ^= 1) {
      const int64_t m = std::min(qc, nq - c0);
      off_c.assign((size_t)m + 1, 0);
      Batch b;
      rc = run_batch(ctx, fam, c0, m, off_c.data(), INT64_MAX / 32, o.query_status ? o.query_status + c0 : nullptr, b);
      if (rc) return rc;
      sum.failed = sum.failed || b.failed;
      if (b.total > 0 && base + b.total <= o.cap) {   // past the capacity: counting only
        if (res.used[k]) GM_HIP(hipStreamWaitEvent(s, ctx->ev_copied[k], 0));   // its last copy is done
        rc = res.reserve(k, b.total, s);
        if (!rc) rc = gather(ctx, b, m, res.p[k]);
        if (rc) return rc;
        GM_HIP(hipEventRecord(ctx->ev_ready[k], s));
        GM_HIP(hipStreamWaitEvent(cs, ctx->ev_ready[k], 0));
        GM_HIP(hipMemcpyAsync(o.out + base, res.p[k], (size_t)b.total * sizeof(gm_range), hipMemcpyDeviceToHost, cs));
        GM_HIP(hipEventRecord(ctx->ev_copied[k], cs));
        res.used[k] = true;
      }
      // the host's share of the chunk after its gather and copy are enqueued
      for (int64_t i = 0; i <= m; ++i) o.off[c0 + i] = base + off_c[(size_t)i];
      base += b.total;
    }
  }
  if (hipGetLastError() != hipSuccess) return hip_fail(hipErrorLaunchFailure, "batched ranges copy");
  if (o.needed) *o.needed = base;
  ctx->ranges_hint = std::max(ctx->ranges_hint, std::min(base, o.cap) / std::max<int64_t>(1, (nq + qc - 1) / qc));
  sum.total = base;
  return base > o.cap ? GM_E_CAPACITY : GM_OK;
}

}  // namespace

// A query that failed (non-zero status) is reported as GM_E_ELEMENT when the caller gave no
// query_status to find it in: offsets, ranges and *needed are delivered all the same, and
// GM_E_CAPACITY (or any other failure) takes precedence.
int run_ranges(gm_ctx* ctx, int64_t nq, const RangesFamily& fam, const RangesOut& o) {
  const int64_t qc = ctx->ranges_chunk > 0 ? ctx->ranges_chunk : (nq < 16384 ? nq : std::max<int64_t>(8192, (nq + 7) / 8));
  Batch b;   // the one batch, or the pipelined chunks' total and failure flag
  int rc;
  if (o.out && device_memory(o.out)) rc = to_device(ctx, fam, nq, o, b);
  else if (qc >= nq || !o.out || !host_pinned(o.out)) rc = to_host(ctx, fam, nq, o, b);
  else rc = to_pinned(ctx, fam, nq, qc, o, b);
  if (rc == GM_OK && b.failed && !o.query_status) {
    set_error("at least one query failed; pass query_status to see which");
    return GM_E_ELEMENT;
  }
  return rc;
}

}  // namespace gm
