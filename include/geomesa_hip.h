/*
 * geomesa_hip.h -- C ABI of the MI355X-native GeoMesa hot path (libgeomesa_hip.so, gfx950).
 *
 * Drop-in boundary for the Scala/JVM surface of liyq0307/geomesa's spatio-temporal
 * index-and-filter path.  Every entry point names the reference interface it replaces
 * (paths abbreviated: z3/ = geomesa-z3/src/main/scala/org/locationtech/geomesa/,
 *  idx/ = geomesa-index-api/src/main/scala/org/locationtech/geomesa/index/).
 * A JVM binding (JNI or Java FFM) is sketched in INTEGRATION.md.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Array arguments are DEVICE pointers (hipMalloc'd, or
 *    any device allocation of the caller) unless the parameter says "host".  Buffers are
 *    caller-owned; the library never retains a pointer past the call (or past gm_ctx_sync()
 *    for the asynchronous entry points).
 *  - Every call returns an int status: GM_OK (0) or a negative GM_E_* code.
 *  - Per-element failures mirror the JVM exceptions: an optional device uint8 status[] gets
 *    GM_ST_* per element, and an optional host gm_batch_status receives the error count and
 *    the first failing element, so a shim can throw the same IllegalArgumentException the
 *    Scala code throws on the first bad element.
 *  - The element-failure rule.  An index call returns GM_E_ELEMENT when summary != NULL,
 *    status == NULL and at least one element failed.  The summary is still filled, every output
 *    row is still written, and failed rows get the documented zeros.  With status != NULL the
 *    return code stays GM_OK: the caller has the codes.  With summary == NULL the call stays
 *    asynchronous on the context's stream and returns GM_OK: a caller passing neither status nor
 *    summary has opted out of failure reporting.  A ranges call returns GM_E_ELEMENT when
 *    query_status == NULL and some query has a non-zero status.  Offsets, ranges and *needed are
 *    still delivered, and GM_E_CAPACITY takes precedence when both apply.
 *  - Thread safety: one gm_ctx per thread; calls on different contexts are independent.
 *  - Asynchrony: beside the entry points whose own comment says asynchronous or stream-ordered, these only
 *    enqueue work on the context's stream and return: gm_z3_invert, gm_z2_invert, gm_legacy_z3_invert,
 *    gm_legacy_z2_invert, gm_z3_key_bytes, gm_z2_key_bytes, gm_arrow_points_to_columns, gm_gen_points.
 *  - Configuration knobs the Scala code reads from system properties
 *    (geomesa.scan.ranges.target, geomesa.scan.ranges.recurse, XZ precision g, ...) are
 *    explicit parameters here, never globals.
 */
#ifndef GEOMESA_HIP_H
#define GEOMESA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: gm_scan_filter gained its last member, polys.  A shim compiled against version 1 passes a shorter
   struct and must be rebuilt. */
#define GM_ABI_VERSION 2

/* return codes */
#define GM_OK 0
#define GM_E_INVALID (-1)     /* bad argument (null pointer, bad period/precision, malformed filter) */
#define GM_E_HIP (-2)         /* HIP runtime failure; see gm_last_error() */
#define GM_E_CAPACITY (-3)    /* output capacity too small; the needed size is reported */
#define GM_E_ELEMENT (-4)     /* at least one element failed and the caller gave nothing to find it in: an index
                                 call with summary != NULL and status == NULL, or a ranges call with
                                 query_status == NULL (the element-failure rule above); every output is
                                 still written */
#define GM_E_INDEX (-5)       /* a device-side reference check of a join failed (corrupt or mismatched index,
                                 or a broken internal invariant); the call's output is not valid */

/* per-element status codes */
/* BinnedTime periods (TimePeriod, z3/curve/BinnedTime.scala:283-291) */
#define GM_PERIOD_DAY 0
#define GM_PERIOD_WEEK 1
#define GM_PERIOD_MONTH 2
#define GM_PERIOD_YEAR 3

#define GM_ST_OK 0
#define GM_ST_OUT_OF_BOUNDS 1 /* Z3SFC/Z2SFC/XZ2SFC/XZ3SFC require(...) -> IllegalArgumentException */
#define GM_ST_BAD_TIME 2      /* BinnedTime require(...): before 1970-01-01 or past the period's max date */
#define GM_ST_UNORDERED 3     /* XZ require(xmin <= xmax ...) / ZRange require(min <= max) */
#define GM_ST_NULL_GEOM 4     /* toIndexKey: "Null geometry in feature" (Z3IndexKeySpace.scala:66-68) */

/* query_status values of the ranges entry points only (gm_z3_ranges, gm_z2_ranges, gm_zranges, gm_xz2_ranges,
   gm_xz3_ranges), beside GM_ST_OUT_OF_BOUNDS and GM_ST_UNORDERED.  They are limits of this library, not
   exceptions of the Scala code, and they are never written to a per-element status[].  The values are those of
   GM_ST_NULL_GEOM and the next free one: in a query_status, 4 is GM_QS_CAPACITY and never means a null
   geometry.  A query with either status delivers no ranges and does not count in *needed; the other queries
   of the batch are not affected. */
#define GM_QS_CAPACITY 4         /* range workspace capacity exceeded: an unbounded (max_ranges <= 0) query, or one
                                    with a budget past the unbounded caps, whose walk outgrew its workspace */
#define GM_QS_TOO_MANY_BOUNDS 5  /* more than 256 z-bounds (boxes x intervals) or windows in one query */

/* TimePeriod (z3/curve/BinnedTime.scala:283-291) */
#define GM_DAY 0
#define GM_WEEK 1
#define GM_MONTH 2
#define GM_YEAR 3

typedef struct gm_ctx gm_ctx;

typedef struct {
  int64_t n_errors;     /* number of failed elements */
  int64_t first_index;  /* index of the first failed element, -1 if none */
  int32_t first_code;   /* GM_ST_* of that element */
  int32_t reserved;
} gm_batch_status;

/* IndexRange (z3/zorder/sfcurve/package.scala:45-76): CoveredRange when contained = 1 */
typedef struct {
  int64_t lower;
  int64_t upper;
  int32_t contained;
  int32_t reserved;
} gm_range;

/* ------------------------------------------------------------------ context */
int gm_abi_version(void);
/* stream: the hipStream_t every call of this context launches on (NULL = the default null stream,
   which is also PyTorch's default stream) */
int gm_ctx_create(int device, void* stream, gm_ctx** out);
/* same, on a new non-blocking stream owned (and destroyed) by the context */
int gm_ctx_create_owned(int device, gm_ctx** out);
int gm_ctx_destroy(gm_ctx* ctx);
/* waits for the context stream; GM_E_INDEX when a stream-ordered polygon-index call since the last
   check failed its device reference checks (gm_pip_join without n_pairs, gm_pip_relate) */
int gm_ctx_sync(gm_ctx* ctx);
void* gm_ctx_stream(gm_ctx* ctx);
const char* gm_last_error(void);
/* per-context tuning parameters (library defaults when unset) */
#define GM_PARAM_JOIN_CHUNK 1   /* points per pass of the join (0 = default 2^31; odd values are rounded
                                   down to even, at least 2); smaller values only add passes -- the
                                   pair set never changes */
#define GM_PARAM_INDEX_BUILD 2  /* where gm_pip_index_create builds the join index: 0 (default) = on the
                                   device (same arrays, byte for byte), 1 = on the host */
#define GM_PARAM_RANGES_CHUNK 3 /* queries per chunk of a batched ranges call whose output is pinned host
                                   memory: chunk k's result copy runs while chunk k + 1 computes (0 =
                                   default: one batch below 16384 queries, else about nq / 8 per chunk);
                                   the output never changes */
#define GM_PARAM_SORT_MODE 4    /* gm_sort_keys: 0 (default) = one to four digit passes over the top
                                   ~log2(n) - 1 varying key bits, then every run of equal prefixes ranked
                                   in LDS (digit passes over every varying byte when a run exceeds 256
                                   rows); 1 = digit passes over every varying byte.  The output never
                                   changes */
#define GM_PARAM_SORT_LAST 5    /* read-only (gm_ctx_get_param): how the context's last gm_sort_keys ran:
                                   digit passes, plus 256 when the runs were ranked locally */
#define GM_PARAM_INDEX_COARSE 6 /* the join's coarse-cell sub-block masks, chosen when a polygon index is
                                   built or imported on this context: -1 (default) = automatic (with
                                   fewer than 2^14 polygons 8 sub-blocks with EMPTY and INTERIOR-of-one-
                                   polygon bits, else 16 EMPTY bits), 0 = EMPTY bits, 1 = EMPTY and
                                   INTERIOR bits.  Results never change */
#define GM_PARAM_INDEX_CORE_RETIRED 7 /* ABI change (round 5): gm_pip_index_core and its parameter 7
                                   (the row predicate's per-polygon core rectangles) were removed with the
                                   rectangles.  Kept for one release as an accepted no-op: setting it
                                   succeeds and changes nothing, reading it returns 0 */
#define GM_PARAM_HIST_GRID 8    /* gm_z3_histogram: workgroups of the LDS-counter kernel (0 = default: one
                                   resident wave of workgroups); fewer workgroups each count more features
                                   and drain their packed counters more often.  Results never change */
#define GM_PARAM_RELATE_ROWS64 9 /* gm_pip_relate: 1 = always the kernel with 64-bit queue rows and the
                                   join's coarse bitmap (the one calls of 2^32 rows or more take);
                                   0 (default) = 32-bit queue rows and the finer bitmap below 2^32 rows.
                                   Results never change */
int gm_ctx_set_param(gm_ctx* ctx, int param, int64_t value);
int gm_ctx_get_param(gm_ctx* ctx, int param, int64_t* value);
/* device memory helpers for callers without their own allocator (e.g. a JNI shim) */
int gm_device_alloc(gm_ctx* ctx, size_t bytes, void** ptr);
int gm_device_free(gm_ctx* ctx, void* ptr);
int gm_copy_to_device(gm_ctx* ctx, void* dst, const void* host_src, size_t bytes);
int gm_copy_to_host(gm_ctx* ctx, void* host_dst, const void* src, size_t bytes);
/* device-to-device copy on the context stream (asynchronous): 16 B per lane with non-temporal loads and
   stores when both pointers are 16-B aligned -- the streaming copy the benchmark calibrates HBM against */
int gm_device_copy(gm_ctx* ctx, void* dst, const void* src, size_t bytes);
/* HIP-event timing on the context stream: brackets any sequence of calls */
int gm_timer_start(gm_ctx* ctx);
int gm_timer_stop(gm_ctx* ctx, float* ms);

/* ------------------------------------------------------------------ Z-curve keys */
/* Z3SFC.index(x, y, t, lenient) (z3/curve/Z3SFC.scala:37-52), t = offset within the period
   (BinnedTime units).  precision = bits per dimension, 1..21 (StandardZ3Dimensions, :92-99). */
int gm_z3_index(gm_ctx* ctx, const double* x, const double* y, const int64_t* t, int64_t n, int period,
                int precision, int lenient, int64_t* z, uint8_t* status, gm_batch_status* summary);

/* Z3IndexKeySpace.toIndexKey lines 71-76 (idx/index/z3/Z3IndexKeySpace.scala): epoch millis ->
   BinnedTime.timeToBinnedTime(period) (z3/curve/BinnedTime.scala:73-86) -> Z3SFC(period).index.
   Produces the [bin][z] key columns (the row key is [shard?][bin BE16][z BE64][id], :81-92). */
int gm_z3_index_key(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n,
                    int period, int lenient, int16_t* bin, int64_t* z, uint8_t* status,
                    gm_batch_status* summary);

/* Z3SFC.invert (z3/curve/Z3SFC.scala:54-57) */
int gm_z3_invert(gm_ctx* ctx, const int64_t* z, int64_t n, int period, int precision, double* x, double* y,
                 int64_t* t);

/* Z2SFC.index / invert (z3/curve/Z2SFC.scala:26-45); precision 1..31 (Z2SFC object uses 31) */
int gm_z2_index(gm_ctx* ctx, const double* x, const double* y, int64_t n, int precision, int lenient,
                int64_t* z, uint8_t* status, gm_batch_status* summary);
int gm_z2_invert(gm_ctx* ctx, const int64_t* z, int64_t n, int precision, double* x, double* y);

/* BinnedTime.timeToBinnedTime(period) (z3/curve/BinnedTime.scala:73-86) */
int gm_binned_time(gm_ctx* ctx, const int64_t* t_ms, int64_t n, int period, int16_t* bin, int64_t* offset,
                   uint8_t* status, gm_batch_status* summary);

/* XZ2SFC(g).index(xmin, ymin, xmax, ymax, lenient) (z3/curve/XZ2SFC.scala:54-77) */
int gm_xz2_index(gm_ctx* ctx, const double* xmin, const double* ymin, const double* xmax, const double* ymax,
                 int64_t n, int g, int lenient, int64_t* out, uint8_t* status, gm_batch_status* summary);
/* XZ3SFC(g, period).index(xmin, ymin, zmin, xmax, ymax, zmax, lenient) (z3/curve/XZ3SFC.scala:53-76) */
int gm_xz3_index(gm_ctx* ctx, const double* xmin, const double* ymin, const double* zmin, const double* xmax,
                 const double* ymax, const double* zmax, int64_t n, int g, int period, int lenient,
                 int64_t* out, uint8_t* status, gm_batch_status* summary);
/* XZ3IndexKeySpace.toIndexKey (idx/index/z3/XZ3IndexKeySpace.scala:60-95) over envelope + dtg columns:
   bin = BinnedTime(period)(dtg) (t_ms NULL = every dtg null -> 0; a bad date fails even when lenient),
   xz = XZ3SFC(g, period).index(xmin, ymin, offset, xmax, ymax, offset, lenient); a failed row gets
   bin 0 and xz 0 and its status */
int gm_xz3_index_key(gm_ctx* ctx, const double* xmin, const double* ymin, const double* xmax, const double* ymax,
                     const int64_t* t_ms, int64_t n, int g, int period, int lenient, int16_t* bin, int64_t* xz,
                     uint8_t* status, gm_batch_status* summary);

/* ------------------------------------------------------------------ range decomposition */
/* Batched ZN.zranges (z3/zorder/sfcurve/ZN.scala:110-242) as reached from Z3SFC.ranges
   (z3/curve/Z3SFC.scala:59-67) and Z2SFC.ranges (z3/curve/Z2SFC.scala:47-52).
   Host inputs, one query per entry of query_off: query q owns boxes [box_off[q], box_off[q+1]) of
   xy (host, 4 doubles each) and, for Z3, times [time_off[q], time_off[q+1]) of t (host, 2 int64
   each, offsets within the period).  The z-bounds of a query are the cross product, as in
   Z3SFC.ranges.  max_ranges <= 0 means None; max_recurse < 0 means the default (Z3:
   Int.MaxValue, Z2: ZN.DefaultRecurse = 7).  Output: ranges of query q are
   out[out_off[q] .. out_off[q+1]) (out_off host); capacity in ranges.  `out` is host memory
   (pageable or pinned; pinned output is copied back chunk by chunk, overlapping the next chunk's
   kernels) or device memory (the ranges stay in HBM for a device-side consumer: no copy).  Returns
   GM_E_CAPACITY with *needed set when cap is too small.  The same output rules hold for
   gm_z2_ranges, gm_zranges, gm_xz2_ranges and gm_xz3_ranges. */
int gm_z3_ranges(gm_ctx* ctx, int64_t n_queries, const int32_t* box_off, const double* xy,
                 const int32_t* time_off, const int64_t* t, int period, int precision, int range_precision,
                 int max_ranges, int max_recurse, int64_t* out_off, gm_range* out, int64_t cap,
                 int64_t* needed, int32_t* query_status);
int gm_z2_ranges(gm_ctx* ctx, int64_t n_queries, const int32_t* box_off, const double* xy, int precision,
                 int range_precision, int max_ranges, int max_recurse, int64_t* out_off, gm_range* out,
                 int64_t cap, int64_t* needed, int32_t* query_status);
/* ZN.zranges(zbounds: Array[ZRange], precision, maxRanges, maxRecurse) (z3/zorder/sfcurve/ZN.scala:110-242)
   on raw z bounds, as Z3.zranges (dims = 3) / Z2.zranges (dims = 2), batched: query q owns the bounds
   [bound_off[q], bound_off[q+1]) of zbounds (host, (min, max) int64 pairs).  max_ranges <= 0 = None;
   max_recurse < 0 = the Scala default Some(ZN.DefaultRecurse) = 7 (ZN.scala:113).  A bound with
   min > max gets query status GM_ST_UNORDERED (ZRange's require, z3/zorder/sfcurve/package.scala:24).
   Outputs as gm_z3_ranges. */
int gm_zranges(gm_ctx* ctx, int dims, int64_t n_queries, const int32_t* bound_off, const int64_t* zbounds,
               int range_precision, int max_ranges, int max_recurse, int64_t* out_off, gm_range* out, int64_t cap,
               int64_t* needed, int32_t* query_status);
/* Batched XZ2SFC.ranges / XZ3SFC.ranges (z3/curve/XZ2SFC.scala:130-252, XZ3SFC.scala:139-262);
   windows as above (4 or 6 doubles each, user space). */
int gm_xz2_ranges(gm_ctx* ctx, int64_t n_queries, const int32_t* win_off, const double* windows, int g,
                  int max_ranges, int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed,
                  int32_t* query_status);
int gm_xz3_ranges(gm_ctx* ctx, int64_t n_queries, const int32_t* win_off, const double* windows, int g,
                  int period, int max_ranges, int64_t* out_off, gm_range* out, int64_t cap, int64_t* needed,
                  int32_t* query_status);

/* ------------------------------------------------------------------ filter scans */
/* Z3Filter.inBounds over columnar keys (idx/filters/Z3Filter.scala:26-62), RowFilterIterator's
   per-row call (geomesa-accumulo-iterators/.../RowFilterIterator.scala:57) as one pass.
   filter_bytes (host) is exactly Z3Filter.serializeToBytes (Z3Filter.scala:112-137).
   bin_ranges (host, n_bin_ranges pairs of int16, inclusive) restricts the scan to the query's
   epochs (the bins Z3IndexKeySpace.getRanges scans, Z3IndexKeySpace.scala:161-194);
   n_bin_ranges = 0 scans every bin.
   Outputs (device, each optional): mask = 1 bit per row (bit i%64 of word i/64, exactly ceil(n/64)
   words; the bits at and above n of the last word are zero, so a popcount of the mask is the match
   count), ids = compacted matching row indices (ids_cap entries, in ascending order; no entry past
   ids_cap is written, and ids != NULL with ids_cap < 0 is GM_E_INVALID).
   *n_match (host) receives the match count (this call synchronises when n_match != NULL);
   GM_E_CAPACITY when ids is given and the matches exceed ids_cap.  The same output rules hold for
   every scan below.
   Waits.  The four scans that take filter_bytes (this one, gm_z2filter_scan and the two _rows forms) wait
   for the context stream once before their kernel is launched, whatever n_match is: the filter's
   descriptor is uploaded from pageable host memory and that copy is waited for.  With n_match == NULL
   they return without waiting for their own kernels; gm_strict_scan, and gm_query_scan without a geometry
   term, do not wait at all then.  gm_query_scan with a geometry term always synchronises (it reports its
   reference check itself). */
int gm_z3filter_scan(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const int16_t* bin_ranges,
                     int n_bin_ranges, const int16_t* bin, const int64_t* z, int64_t n, uint64_t* mask,
                     int64_t* ids, int64_t ids_cap, int64_t* n_match);
/* Z2Filter.inBounds (idx/filters/Z2Filter.scala:20-35) */
int gm_z2filter_scan(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const int64_t* z, int64_t n,
                     uint64_t* mask, int64_t* ids, int64_t ids_cap, int64_t* n_match);
/* RowFilter.inBounds(buf, offset) on row-key BYTES (idx/filters/RowFilter.scala:11-13), the loop of
   RowFilterIterator.findTop (geomesa-accumulo-iterators/.../RowFilterIterator.scala:52-66) and
   Z3HBaseFilter as one pass: row i is rows[row_off[i] .. row_off[i+1]) (device bytes; device int64
   offsets, n + 1 of them) and its key starts at key_offset (RowFilterIterator.RowOffsetKey, the
   shard / table-sharing prefix length).  Z3Filter.inBounds (Z3Filter.scala:26-28) reads the
   big-endian short epoch at key_offset and the long z at key_offset + 2; Z2Filter.inBounds
   (Z2Filter.scala:22-35) the long at key_offset.  A row shorter than its key never matches and is
   counted in *n_short (host, optional; the JVM read throws ArrayIndexOutOfBoundsException).
   Outputs as gm_z3filter_scan (no bin restriction: the scan ranges already chose the rows). */
int gm_z3filter_scan_rows(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const uint8_t* rows,
                          const int64_t* row_off, int key_offset, int64_t n, uint64_t* mask, int64_t* ids,
                          int64_t ids_cap, int64_t* n_match, int64_t* n_short);
int gm_z2filter_scan_rows(gm_ctx* ctx, const uint8_t* filter_bytes, size_t filter_len, const uint8_t* rows,
                          const int64_t* row_off, int key_offset, int64_t n, uint64_t* mask, int64_t* ids,
                          int64_t ids_cap, int64_t* n_match, int64_t* n_short);
/* Strict full-filter evaluation on raw columns (useFullFilter, Z3IndexKeySpace.scala:240-254):
   GeoTools BBOX on a point (geomesa-filter/.../GeometryProcessing.scala:129, inclusive) AND
   FastDuring (geomesa-filter/.../FastTemporalOperator.scala:123-126, exclusive at both ends, ms).
   bbox (host) = xmin, ymin, xmax, ymax; has_during = 0 skips the time test. */
int gm_strict_scan(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n,
                   const double* bbox, int has_during, int64_t during_lo_ms, int64_t during_hi_ms,
                   uint64_t* mask, int64_t* ids, int64_t ids_cap, int64_t* n_match);

/* ------------------------------------------------------------------ st_contains join */
/* Polygon set in CSR form (host arrays): polygon -> parts (a MultiPolygon's components; a
   Polygon has one) -> rings (first ring of each part is the shell, the rest are holes) ->
   vertices.  Rings are closed (first vertex == last vertex), as JTS LinearRings are. */
typedef struct {
  int32_t n_polys;
  const int32_t* poly_part_off; /* [n_polys + 1] */
  const int32_t* part_ring_off; /* [n_parts + 1] */
  const int32_t* ring_vert_off; /* [n_rings + 1] */
  const double* vx;             /* [n_verts] */
  const double* vy;             /* [n_verts] */
} gm_polyset;

typedef struct gm_pip_index gm_pip_index;

/* Uploads the polygon set and builds the device-side join index (uniform grid over polygon
   envelopes -- the analogue of RelationUtils.grid, geomesa-spark-sql/.../RelationUtils.scala:30-157 --
   plus per-ring y-slab edge buckets). */
int gm_pip_index_create(gm_ctx* ctx, const gm_polyset* polys, gm_pip_index** out);
/* same with an explicit grid density: ~cells_per_poly grid cells per polygon over the set's
   envelope (0 = default 16384, at most 2^26 cells; a coarse 8x8-cell table in front of it stays
   L2-resident) */
int gm_pip_index_create_ex(gm_ctx* ctx, const gm_polyset* polys, int cells_per_poly, gm_pip_index** out);
int gm_pip_index_destroy(gm_pip_index* index);
/* index statistics: stats[0..6] = cells, (cell, polygon) entries, boundary entries, ring records,
   ring records that fall back to the slab walk, boundary blob bytes, compact (one-line) blobs */
int gm_pip_index_stats(const gm_pip_index* index, int64_t* stats);
/* Diagnostic (no reference counterpart): how the join's lookup chain resolves the device points
   px / py, stage by stage -- counters[20] = points, outside the grid, coarse EMPTY, coarse INTERIOR,
   points in mixed coarse cells before the sub-block masks, fine lookups, fine EMPTY, fine INTERIOR,
   fine line entries, fine compact blobs, fine generic blobs, fine lists, list entries, list entries
   that are blobs, line entries that decide, line entries that fall back to the blob, fine words with
   inline lines, inline words that fall back to the blob, coarse-table gathers (points the LDS
   EMPTY bitmap does not answer), fine words with two inline lines. */
int gm_pip_join_census(gm_ctx* ctx, const gm_pip_index* index, const double* px, const double* py, int64_t n,
                       int64_t* counters);

/* A built index as device arrays, for shipping it to the other GPUs of a join (RCCL broadcast) instead
   of rebuilding it on every rank -- the broadcast side of GeoMesaJoinRelation's join
   (geomesa-spark-sql/.../GeoMesaJoinRelation.scala:41-91).  gm_pip_index_export fills the layout
   (array sizes + grid scalars, plain host data); gm_pip_index_copy_array copies device array k into a
   caller buffer of layout.bytes[k] bytes (stream-ordered); gm_pip_index_import builds an index on
   ctx's device from the layout and device copies of the arrays (the library copies them: the caller
   keeps ownership of `arrays`). */
#define GM_PIP_INDEX_ARRAYS 8
#define GM_PIP_LAYOUT_VERSION 1
typedef struct {
  int32_t version;                       /* GM_PIP_LAYOUT_VERSION */
  int32_t dims[4];                       /* grid columns, rows, coarse columns, polygons */
  int32_t reserved;
  double grid[6];                        /* grid envelope x0 y0 x1 y1, inverse cell width / height */
  int64_t stats[9];                      /* gm_pip_index_stats[0..6], most boundary / all entries of a cell */
  int64_t bytes[GM_PIP_INDEX_ARRAYS];    /* device bytes of each array */
} gm_pip_index_layout;
int gm_pip_index_export(const gm_pip_index* index, gm_pip_index_layout* layout);
int gm_pip_index_copy_array(gm_ctx* ctx, const gm_pip_index* index, int k, void* dst);
int gm_pip_index_import(gm_ctx* ctx, const gm_pip_index_layout* layout, void* const* arrays, gm_pip_index** out);

/* ST_Contains(polygon, point) = JTS Geometry.contains (geomesa-spark-jts/.../udf/
   SpatialRelationFunctions.scala:29), evaluated for every (point, polygon) pair -- the result of
   GeoMesaJoinRelation.sweeplineJoin + OverlapAction (geomesa-spark-sql/.../GeoMesaJoinRelation.scala:41-91,
   OverlapAction.scala:25-41) as one batch.  Points are device columns.  Matching pairs go to
   pt_ids / poly_ids (device, cap entries; point ids are id_base + row); order within the output is
   unspecified (the reference returns an unordered RDD).  *n_pairs (host) receives the pair count;
   when it exceeds cap, GM_E_CAPACITY is returned and no pair beyond cap is written.  With
   pt_ids = poly_ids = NULL the call only counts.  With n_pairs = NULL the call is stream-ordered
   (asynchronous); with n_pairs it synchronises the context stream.  A device reference check of the
   index that fails (a corrupt or mismatched imported index) makes the output invalid and is reported
   as GM_E_INDEX by the next synchronising call on the context (this join with n_pairs, gm_query_scan,
   gm_ctx_sync). */
int gm_pip_join(gm_ctx* ctx, const gm_pip_index* index, const double* px, const double* py, int64_t n,
                int64_t id_base, int64_t* pt_ids, int32_t* poly_ids, int64_t cap, int64_t* n_pairs);

/* join strategies for gm_pip_join_ex.  Both run the staged direct pass over the point columns; a
   band-partitioned and a two-pass variant measured slower on MI355X and were
   removed, and any other value returns GM_E_INVALID */
#define GM_JOIN_AUTO 0
#define GM_JOIN_DIRECT 1
/* gm_pip_join with an explicit strategy */
int gm_pip_join_ex(gm_ctx* ctx, const gm_pip_index* index, const double* px, const double* py, int64_t n,
                   int64_t id_base, int64_t* pt_ids, int32_t* poly_ids, int64_t cap, int64_t* n_pairs, int mode);

/* gm_pip_join_ex with the join's predicate: GM_SPATIAL_CONTAINS (st_contains(polygon, point) /
   st_within(point, polygon): the point in the interior) or GM_SPATIAL_INTERSECTS (st_intersects /
   st_covers: boundary included).  GeoMesaJoinRelation takes any (Geometry, Geometry) => Boolean UDF of
   the join condition (GeoMesaJoinRelation.scala:67-79, SQLRules.scala:186-190); these are the ones with
   a non-empty result over (polygon, point) pairs besides st_touches. */
int gm_pip_join_pred(gm_ctx* ctx, const gm_pip_index* index, const double* px, const double* py, int64_t n,
                     int64_t id_base, int64_t* pt_ids, int32_t* poly_ids, int64_t cap, int64_t* n_pairs, int mode,
                     int predicate);

/* ------------------------------------------------------------------ fused query filter */
/* spatial terms of gm_query_scan */
#define GM_SPATIAL_NONE 0
#define GM_SPATIAL_INTERSECTS 1  /* INTERSECTS(geom, P): JTS P.intersects(point), boundary included */
#define GM_SPATIAL_CONTAINS 2    /* CONTAINS(P, geom) / WITHIN(geom, P): JTS P.contains(point), interior only */
/* The full filter of a point query in one pass (useFullFilter, Z3IndexKeySpace.scala:240-254):
   BBOX (inclusive, geomesa-filter/.../GeometryProcessing.scala:129) AND during (exclusive ms,
   FastTemporalOperator.scala:123-126) AND the OR over the polygons of `geoms` of the spatial term
   (GeometryProcessing.process turns a split query geometry into an OR of its parts, :104-136).
   bbox (host xmin, ymin, xmax, ymax) NULL = no BBOX term; has_during = 0 = no time term;
   spatial_op GM_SPATIAL_NONE = no geometry term (geoms may be NULL).  geoms is any polygon index
   (gm_pip_index_create_ex; a denser grid, e.g. 65536 cells for one query polygon, makes more rows
   resolve in one lookup).  Outputs as gm_strict_scan: mask bits, ids ascending, *n_match. */
int gm_query_scan(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n,
                  const double* bbox, int has_during, int64_t during_lo_ms, int64_t during_hi_ms,
                  const gm_pip_index* geoms, int spatial_op, uint64_t* mask, int64_t* ids, int64_t ids_cap,
                  int64_t* n_match);

/* ------------------------------------------------------------------ row-wise predicates (UDF path) */
/* Spark SQL's st_* relation UDFs evaluated row by row (SpatialRelationFunctions.scala:29-37, null in
   -> null out via nullableUDF, SQLFunctionHelper.scala:27-33): row i relates polygon poly[i] of the
   index with point (px[i], py[i]) and gets PointLocator's location of the point in the polygon.
   For an areal geometry and a point every DE-9IM predicate follows from it:
     st_contains(P, pt) = st_within(pt, P) = INTERIOR;  st_covers / st_intersects = not EXTERIOR;
     st_touches = BOUNDARY;  st_disjoint = EXTERIOR;  st_crosses / st_overlaps / st_equals = false.
   poly[i] < 0 or >= the polygon count marks a null row (GM_LOC_NULL).  Device arrays. */
#define GM_LOC_EXTERIOR 0
#define GM_LOC_BOUNDARY 1
#define GM_LOC_INTERIOR 2
#define GM_LOC_NULL 255
/* Stream-ordered; a failed device reference check is reported as for gm_pip_join (GM_E_INDEX at the
   next synchronising call: the locations are then invalid).  gm_query_scan checks its geometry term
   the same way and reports it itself. */
int gm_pip_relate(gm_ctx* ctx, const gm_pip_index* index, const int32_t* poly, const double* px, const double* py,
                  int64_t n, uint8_t* loc);

/* ------------------------------------------------------------------ Arrow columnar input */
/* GeoMesa's Arrow geometry vectors (geomesa-arrow-jts) as zero-copy device input.  A point column is
   a FixedSizeList(2) of Float8 (PointVector) or Float4 (PointFloatVector) whose tuples hold [y, x]
   by default and [x, y] when the vector's flipAxisOrder is set (AbstractPointVector.java:52-79);
   line, polygon and multi-geometry columns nest List offsets around the same tuples
   (AbstractLineStringVector.java, AbstractPolygonVector.java:56-84 -- rings, the first one the
   shell --, AbstractMultiPolygonVector.java:61-95 -- polygons, rings).  Dates are Arrow int64 epoch
   milliseconds.  Null slots come from the Arrow validity bitmaps (LSB bit order). */
#define GM_GEOM_POINT 0
#define GM_GEOM_LINESTRING 1      /* offsets[0]: slot -> tuples */
#define GM_GEOM_POLYGON 2         /* offsets[0]: slot -> rings, offsets[1]: ring -> tuples */
#define GM_GEOM_MULTIPOINT 3      /* offsets[0]: slot -> tuples */
#define GM_GEOM_MULTILINESTRING 4 /* offsets[0]: slot -> lines, offsets[1]: line -> tuples */
#define GM_GEOM_MULTIPOLYGON 5    /* offsets[0]: slot -> polygons, [1]: polygon -> rings, [2]: ring -> tuples */
/* The seventh vector: WKBGeometryVector (geomesa-arrow-jts WKBGeometryVector.java:27-93), what an
   attribute declared geom:Geometry is written as (geomesa-arrow-gt ArrowAttributeWriter.scala:266-267; read
   at ArrowAttributeReader.scala:432 and through GeometryFields.java:40).  An Arrow Binary column, one JTS
   WKBWriter blob per slot, any geometry class in any slot.  As a gm_geom_column:
     coords        the Binary value buffer (bytes, any alignment)
     offsets[0]    the int32 value offsets, n + 1 entries: slot i is bytes [offsets[0][i], offsets[0][i+1]);
                   offsets[1], offsets[2] unused
     validity, validity_offset   as for the typed columns
     ordinal_bits  64 (WKB ordinates are doubles); anything else is GM_E_INVALID
     flip_axis     ignored: WKB is always x then y (the vector stores its flipAxisOrder flag but never
                   applies it to the bytes, WKBGeometryVector.java:66-75, 122-129)
   The blob grammar -- the OGC / ISO WKB layout plus the EWKB flag bits -- is this rule, and the rule is
   the definition.  JTS is outside the reference tree, so agreement with JTS 1.20's WKBReader itself is
   PARITY UNPINNED.
     geometry := order:u8 (0 = big-endian, 1 = little-endian; anything else is malformed)
                 typeInt:u32 in that order
                 [srid:u32 if typeInt & 0x20000000]   (skipped)
                 body
     code = (typeInt & 0xffff) % 1000          iso = (typeInt & 0xffff) / 1000
     hasZ = typeInt & 0x80000000 or iso in {1, 3};  hasM = typeInt & 0x40000000 or iso in {2, 3}
     tuple = (2 + hasZ + hasM) doubles; x, y are the first two; Z and M are skipped
     1 Point            one tuple; a NaN x or y = the empty point
     2 LineString       count:u32, count tuples
     3 Polygon          rings:u32, each ring count:u32 + tuples; ring 0 is the shell
     4 MultiPoint / 5 MultiLineString / 6 MultiPolygon / 7 GeometryCollection
                        count:u32, then count complete geometries, each with its own order byte and
                        typeInt; an element of a Multi* must have the matching single code
   Each nested geometry carries its own byte order and orders may differ inside one blob (JTS's own
   writer emits big-endian 2-D blobs without SRID: POINT (0 20) is 00 00000001 0000000000000000
   4034000000000000).  Collections (codes 4 .. 7) nest to at most GM_WKB_MAX_DEPTH levels; that is this
   library's limit.  Bytes after the top-level geometry are ignored.  Ordinates are read as 64-bit
   patterns: NaN payloads and -0.0 arrive as written.
   A MALFORMED SLOT IS TREATED EXACTLY AS A NULL SLOT.  A slot is malformed when the order byte or the
   code is unknown, when a header or a tuple run would end past the slot's end, when a Multi* element has
   the wrong code, or when collections nest deeper than the limit (WKBGeometryVector.get throws there,
   WKBGeometryVector.java:78-92; the entries below have no per-slot error channel besides the key entries'
   status).  No byte outside [offsets[0][i], offsets[0][i+1]) is read, whatever the headers claim.
   Entries that take the type: gm_arrow_envelopes, gm_xz2_index_key_arrow, gm_xz3_index_key_arrow,
   gm_arrow_points_to_columns, gm_table_scan_geom.  Every other entry with a gm_geom_column argument
   returns GM_E_INVALID for it (gm_last_error names the type). */
#define GM_GEOM_WKB 16
#define GM_WKB_MAX_DEPTH 8

typedef struct {
  int32_t type;              /* GM_GEOM_* */
  int32_t ordinal_bits;      /* 64 (Float8 vectors, WKB) or 32 (Float4 "...FloatVector"s) */
  int32_t flip_axis;         /* 0: [y, x] tuples (the default), 1: [x, y] */
  int32_t reserved;
  const void* coords;        /* tuple ordinates, tuple j at [2j], [2j + 1] (already advanced by the
                                innermost child array's offset); GM_GEOM_WKB: the value bytes */
  const uint8_t* validity;   /* top-level validity bitmap, NULL = no nulls */
  int64_t validity_offset;   /* bit index of slot 0 in validity (the Arrow array offset) */
  const int32_t* offsets[3]; /* List offsets, outermost first, each advanced by its array's offset;
                                unused levels NULL */
} gm_geom_column;

typedef struct {
  const int64_t* millis;     /* epoch ms (Arrow Timestamp(ms) / Date(ms) / Int64) */
  const uint8_t* validity;   /* NULL = no nulls */
  int64_t validity_offset;
} gm_time_column;

/* Z3IndexKeySpace.toIndexKey over an Arrow batch (idx/index/z3/Z3IndexKeySpace.scala:63-95):
   point column + date column (dtg NULL or a null slot -> time 0, :70).  A null geometry is
   GM_ST_NULL_GEOM (the IllegalArgumentException of :66-68).  Device arrays, as gm_z3_index_key. */
int gm_z3_index_key_arrow(gm_ctx* ctx, const gm_geom_column* geom, const gm_time_column* dtg, int64_t n,
                          int period, int lenient, int16_t* bin, int64_t* z, uint8_t* status,
                          gm_batch_status* summary);
/* Z2IndexKeySpace.toIndexKey (idx/index/z2/Z2IndexKeySpace.scala:48-75): Z2SFC.index of a point column */
int gm_z2_index_key_arrow(gm_ctx* ctx, const gm_geom_column* geom, int64_t n, int lenient, int64_t* z,
                          uint8_t* status, gm_batch_status* summary);
/* XZ2IndexKeySpace.toIndexKey (idx/index/z2/XZ2IndexKeySpace.scala:48-76): XZ2SFC(g).index of each
   geometry's JTS envelope (Geometry.getEnvelopeInternal: a polygon's envelope is its shell's, a multi
   geometry's the union of its parts'; an empty geometry has the null envelope -> GM_ST_UNORDERED). */
int gm_xz2_index_key_arrow(gm_ctx* ctx, const gm_geom_column* geom, int64_t n, int g, int lenient, int64_t* xz,
                           uint8_t* status, gm_batch_status* summary);
/* XZ3IndexKeySpace.toIndexKey (idx/index/z3/XZ3IndexKeySpace.scala:60-95): bin + XZ3SFC(g, period).index
   of (envelope, offset) with the time from dtg (NULL / null slot -> 0) */
int gm_xz3_index_key_arrow(gm_ctx* ctx, const gm_geom_column* geom, const gm_time_column* dtg, int64_t n, int g,
                           int period, int lenient, int16_t* bin, int64_t* xz, uint8_t* status,
                           gm_batch_status* summary);
/* Geometry.getEnvelopeInternal of every slot as four device columns (a null slot and an empty geometry:
   the JTS null envelope, 0, 0, -1, -1): the envelope columns of gm_scan_filter.  Asynchronous.
   GM_GEOM_WKB: a collection's envelope is the merge of its elements', null ones skipped; a malformed slot
   reads as a null slot.  The two XZ key entries above index the same envelope (GM_ST_NULL_GEOM for a null
   or malformed slot, GM_ST_UNORDERED for an empty geometry). */
int gm_arrow_envelopes(gm_ctx* ctx, const gm_geom_column* geom, int64_t n, double* xmin, double* ymin,
                       double* xmax, double* ymax);
/* A point column as x / y device columns (null slots -> NaN): the adapter for every other entry.
   GM_GEOM_WKB: x, y of a slot whose top-level geometry is a Point; a null or malformed slot, the empty
   point and every other class (a one-element MultiPoint included) are NaN, NaN. */
int gm_arrow_points_to_columns(gm_ctx* ctx, const gm_geom_column* geom, int64_t n, double* x, double* y);
/* gm_pip_join_pred over an Arrow point column (null points never match): the direct pass reads the
   tuples in place */
int gm_pip_join_arrow(gm_ctx* ctx, const gm_pip_index* index, const gm_geom_column* points, int64_t n,
                      int64_t id_base, int64_t* pt_ids, int32_t* poly_ids, int64_t cap, int64_t* n_pairs, int mode,
                      int predicate);
/* gm_pip_index_create_ex from an Arrow POLYGON or MULTIPOLYGON column given in HOST memory (the
   broadcast side of the join is collected on the host); a null slot is an empty polygon */
int gm_pip_index_create_arrow(gm_ctx* ctx, const gm_geom_column* polys, int32_t n, int cells_per_poly,
                              gm_pip_index** out);

/* ------------------------------------------------------------------ sorted key table */
/* The row-key prefix [shard?][bin BE16][z BE64] of Z3IndexKeySpace.toIndexKey (idx/index/z3/
   Z3IndexKeySpace.scala:81-92; ByteArrays.writeShort / writeLong, geomesa-utils/.../index/
   ByteArrays.scala:51,90-99) for n rows: out (device) gets n * key_len bytes, key_len = 11 with a
   shard column (device uint8, ShardStrategy.scala:75-80), 10 when shard = NULL.  The feature id
   the store appends after the prefix is the caller's. */
int gm_z3_key_bytes(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                    uint8_t* out);

/* The row-key prefix of the key spaces without a time bin: [shard?][z BE64] for Z2IndexKeySpace
   (idx/index/z2/Z2IndexKeySpace.scala:48-76) and XZ2IndexKeySpace (idx/index/z2/XZ2IndexKeySpace.scala:
   48-76, z = the XZ2 value): n * key_len bytes, key_len = 9 with a shard column, 8 without. */
int gm_z2_key_bytes(gm_ctx* ctx, const uint8_t* shard, const int64_t* z, int64_t n, uint8_t* out);

/* Sorts key columns into the table's row order -- the byte order of the row keys above: shard,
   then bin as an unsigned big-endian short, then z as an unsigned big-endian long (what Accumulo /
   HBase keep sorted).  Stable; perm_out[i] = the input row of table row i.  shard / shard_out may
   be NULL together (unsharded table); bin / bin_out may be NULL together (a key space without a time
   bin: Z2, XZ2).  n < 2^32.  Device temporaries: about 32.5 B per row (+ 4 B without a bin).
   Synchronises the context stream: the sort's plan reads the keys' varying bits back. */
int gm_sort_keys(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                 uint8_t* shard_out, int16_t* bin_out, int64_t* z_out, int64_t* perm_out);

/* Key-range partitioning of a table over GPUs (configs[2]: the table split into contiguous key ranges,
   one per rank, as a sorted store splits a table into tablets / regions, the shard prefix of
   ShardStrategy.scala:75-80 staying the key's first byte; it replaces the Spark shuffle of
   RelationUtils.scala:30-33, groupByKey(new IndexPartitioner(...))).  A key is the pair
   key_hi = shard << 16 | bin as u16 (0 <= key_hi < 2^24), key_lo = z as u64, compared unsigned
   lexicographically -- the byte order of [shard][bin BE16][z BE64].

   gm_key_sample: n_samples (<= 65536) keys of the UNSORTED columns at rows floor((2i+1) n / (2 n_samples))
   into key_hi / key_lo (host arrays).  Synchronises the context stream. */
int gm_key_sample(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n, int32_t n_samples,
                  uint64_t* key_hi, uint64_t* key_lo);
/* gm_key_partition: every row's destination d = the number of the n_split (< 256) ascending splitter keys
   (host arrays) <= its key; the rows are written grouped by destination (d ascending), keeping their
   input order within a destination, into shard_out / bin_out / z_out (device; shard and shard_out NULL
   together), with their source in ids_out (device, optional: ids[row] when ids (device) is given, else
   id_base + row) and / or rows_out (device, optional: the input row).  dest_counts (host, n_split + 1)
   receives each destination's row count; destination d's rows start at the sum of the counts before it.
   n < 2^32.  Synchronises the context stream. */
int gm_key_partition(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                     const uint64_t* split_hi, const uint64_t* split_lo, int32_t n_split, const int64_t* ids,
                     int64_t id_base, uint8_t* shard_out, int16_t* bin_out, int64_t* z_out, int64_t* ids_out,
                     uint32_t* rows_out, int64_t* dest_counts);

/* A scan range over the key prefix, inclusive at both ends in table order: what getRangeBytes
   makes of a ScanRange (idx/index/z3/Z3IndexKeySpace.scala:196-238), [toBytes(lo),
   toBytesFollowingPrefix(hi)) = every row whose [shard][bin][z] prefix lies in [lo, hi].
   BoundedRange(bin, lo, hi): bin_lo = bin_hi = bin; LowerBoundedRange: z_hi/bin_hi = all ones;
   UpperBoundedRange: bin_lo = z_lo = 0; UnboundedRange: both.  bin and z compare unsigned. */
typedef struct {
  int64_t z_lo;
  int64_t z_hi;
  int16_t bin_lo;
  int16_t bin_hi;
  uint8_t shard;       /* 0 for an unsharded table */
  uint8_t reserved[3];
} gm_key_range;

/* Seek-and-filter over a sorted table (gm_sort_keys order): every row inside any of the ranges
   (host array; sorted and merged here the way a BatchScanner merges overlapping ranges), then
   Z3Filter.inBounds on each (idx/filters/Z3Filter.scala:26-62, RowFilterIterator.scala:52-66) when
   filter_bytes (host, Z3Filter.serializeToBytes) is not NULL.  ids (device, optional) receives the
   matching rows in table order, mapped through perm (device, optional) to input rows.
   *n_match / *n_scanned (host) receive the match and candidate counts; GM_E_CAPACITY when the
   matches exceed ids_cap.  Synchronises the context stream. */
int gm_key_range_scan(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                      const gm_key_range* ranges, int64_t n_ranges, const uint8_t* filter_bytes, size_t filter_len,
                      const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned);

/* The filters a table scan applies to its candidates (all optional; zero-initialise the struct):
   - the row filter the tablet server runs on each key (RowFilterIterator.scala:52-66): z3filter
     (host, Z3Filter.serializeToBytes: Z3Filter.inBounds on (bin, z), idx/filters/Z3Filter.scala:26-62)
     OR z2filter (host, Z2Filter.serializeToBytes: Z2Filter.inBounds on z, idx/filters/Z2Filter.scala:
     20-35), not both;
   - the full filter on the feature, which the XZ key spaces always apply (useFullFilter = true,
     XZ2IndexKeySpace.scala:122-125, XZ3IndexKeySpace.scala:247-250): with n_boxes > 0 the feature's
     envelope (xmin / ymin / xmax / ymax: device columns, reached through rows) intersects at least
     one of the boxes (host, n_boxes x (xmin, ymin, xmax, ymax); JTS Envelope.intersects, inclusive; a
     null envelope -- maxx < minx, JTS Envelope.isNull, on either side -- never intersects; the y
     ends and NaN take no part in that rule), and with during != 0 the feature's dtg (t_ms: device, same
     order as the envelopes) lies in (t_lo, t_hi), exclusive (FastDuring,
     FastTemporalOperator.scala:116-129).  For a rectangular geometry the envelope test is GeoTools
     BBOX exactly; for other geometries it is BBOX's envelope pre-check, and gm_table_scan_geom applies
     BBOX itself, on the feature geometry;
   - rows (device, optional): the column row of each table row, i.e. where table row r's envelope and
     dtg are found (xmin[rows[r]], ...).  NULL: gm_table_scan's perm argument maps them (columns in
     INPUT order); both NULL: the columns are in table order.  rows only reaches the full filter's
     columns; the ids that come back are mapped by perm alone;
   - polys (host, optional; gm_table_scan_geom only): the query geometry as polygons instead of boxes, see
     gm_table_scan_geom.  NULL: boxes, as before the member existed.  With polys, boxes must be NULL and
     n_boxes 0; gm_table_scan refuses a filter with polys (GM_E_INVALID). */
typedef struct {
  const uint8_t* z3filter;
  size_t z3filter_len;
  const uint8_t* z2filter;
  size_t z2filter_len;
  const double* xmin;
  const double* ymin;
  const double* xmax;
  const double* ymax;
  const double* boxes;
  int32_t n_boxes;
  int32_t during;
  const int64_t* t_ms;
  int64_t t_lo;
  int64_t t_hi;
  const int64_t* rows;
  const gm_polyset* polys;
} gm_scan_filter;
/* the most ring tuples (closing tuples included) a query polygon set may hold: its edges, bucketed by
   y-slab with at most 2 entries per edge, go to the device once per call, 40 B per entry (5 MiB at the
   cap) */
#define GM_POLY_QUERY_MAX_VERTICES 65536
/* Seek-and-filter over any sorted key table (gm_sort_keys order): Z3 and XZ3 tables ([shard][bin][z]),
   Z2 and XZ2 tables (bin = NULL: [shard][z]).  Every row inside any of the ranges (host array, merged as
   gm_key_range_scan merges them; for bin = NULL give bin_lo = bin_hi = 0, XZ2IndexKeySpace.getRangeBytes
   :104-120), then the filters of f (NULL = none).  ids (device, optional) receives the matching rows in
   table order, mapped through perm (device, optional) to input rows; *n_match / *n_scanned (host) the
   match and candidate counts; GM_E_CAPACITY when the matches exceed ids_cap.  Synchronises. */
int gm_table_scan(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                  const gm_key_range* ranges, int64_t n_ranges, const gm_scan_filter* f, const int64_t* perm,
                  int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned);

/* gm_table_scan with the full filter on the feature GEOMETRY: a candidate must pass everything
   gm_table_scan asks of it and its geometry (slot of geom, any GM_GEOM_* kind) must meet at least one of
   f's boxes, each box [xmin, xmax] x [ymin, ymax] a closed set, a segment or a point included: GeoTools
   BBOX on the geometry (geomesa-filter/.../GeometryProcessing.scala:104-136), i.e. JTS Geometry.intersects
   with the rectangle (RectangleIntersects).  A point or multipoint has a point in the box; a line has a
   segment meeting it; a polygon has a ring segment (shell or hole) meeting it or holds the box (inside the
   shell and inside no hole, SimplePointInAreaLocator).  A null slot, an empty geometry and a null box
   (xmax < xmin) never match.  Required, else GM_E_INVALID with a gm_last_error text: f, f->n_boxes > 0,
   f->boxes, f's four envelope columns, geom with ordinal_bits 64 or 32, a GM_GEOM_* type and the coords and
   List offsets of that type.  f's envelope columns must hold the slots' JTS envelopes (gm_arrow_envelopes
   writes them): the envelope test stays the prefilter and decides the slots it can decide.  Table row r's
   slot is found as its envelope is: f->rows, else perm, else the identity.  *n_envelope (host, optional)
   receives the candidates that pass the row filter, during and the envelope test -- gm_table_scan's *n_match
   for the same arguments.  ids, ids_cap, *n_match, *n_scanned, GM_E_CAPACITY and the synchronisation are
   gm_table_scan's.
   A GM_GEOM_WKB slot (ordinal_bits 64, coords and offsets[0]) is decided per class in the same way: a
   collection matches iff any element does, a LineString of one tuple is that point, and a malformed slot
   never matches -- its envelope column holds the null envelope, which is what keeps it from the walk.

   INTERSECTS against query polygons: f->polys (host) in place of the boxes (f->boxes NULL, f->n_boxes 0,
   else GM_E_INVALID).  Each polygon of the set has parts, each part a shell and holes, rings closed.  A part
   is the closed set "inside or on the shell, and not strictly inside a hole"; slot G matches iff G and at
   least one part share a point.  A null slot, an empty geometry and a malformed WKB slot never match, a
   collection matches iff any element does, a LineString of one tuple is that point.  The decision:
     1. the envelope prefilter, unchanged, with the JTS envelope of each part (of its shell) as the boxes,
        derived here; *n_envelope reports its survivors;
     2. contact: a segment of G meets a ring segment of a part (shell or hole), decided as
        RobustLineIntersector.computeIntersect decides hasIntersection: the segments' envelopes overlap,
        the orientation signs of one segment's ends about the other are not both positive or both negative,
        either way round, and with all four zero an endpoint lies in the other segment's envelope;
     3. containment, reached only without contact, when every connected piece of G (each point, line and
        polygon shell) lies wholly inside or wholly outside each part: the first tuple of a piece is not
        exterior to some part (RayCrossingCounter ring by ring; inside or on the shell and strictly inside
        no hole -- not Mod-2 over the rings; for a point this is also where "on the boundary" is found), or,
        for a polygon of G, the first shell vertex of some part is inside that polygon by the same rule over
        its rings.
   Every query ring is closed, has at least 4 tuples and finite ordinates, the set has at least one part and
   at most GM_POLY_QUERY_MAX_VERTICES tuples, else GM_E_INVALID with a gm_last_error text -- never a
   fallback.  A self-intersecting query polygon is answered by the procedure as written; its parity with
   JTS is unpinned.  JTS 1.20 answers a non-rectangular intersects through RelateOp, which is not in the
   reference tree: parity beyond this closed-set definition is unpinned. */
int gm_table_scan_geom(gm_ctx* ctx, const uint8_t* shard, const int16_t* bin, const int64_t* z, int64_t n,
                       const gm_key_range* ranges, int64_t n_ranges, const gm_scan_filter* f,
                       const gm_geom_column* geom, const int64_t* perm, int64_t* ids, int64_t ids_cap,
                       int64_t* n_match, int64_t* n_scanned, int64_t* n_envelope);

/* ------------------------------------------------------------------ legacy curves (reading / deleting old data) */
/* LegacyZ3SFC(period) (z3/curve/LegacyZ3SFC.scala:18-49): SemiNormalizedDimension lon/lat (2^21-1) and
   time (2^20-1) (NormalizedDimension.scala:83-97), ceil-based normalize, lenientIndex clamped from
   below only; LegacyYearZ3SFC (LegacyYearZ3SFC.scala:17-46): the 21-bit curve with the 52-week time
   max, offsets in (52 weeks, maxOffset(Year)] indexed as the max.  Device arrays, as gm_z3_index. */
#define GM_LEGACY_Z3 0
#define GM_LEGACY_YEAR_Z3 1
int gm_legacy_z3_index(gm_ctx* ctx, const double* x, const double* y, const int64_t* t, int64_t n, int curve,
                       int period, int lenient, int64_t* z, uint8_t* status, gm_batch_status* summary);
/* LegacyZ3SFC.invert = Z3SFC.invert with SemiNormalizedDimension.denormalize (curve GM_LEGACY_Z3 only) */
int gm_legacy_z3_invert(gm_ctx* ctx, const int64_t* z, int64_t n, int curve, int period, double* x, double* y,
                        int64_t* t);
/* LegacyZ2SFC (z3/curve/LegacyZ2SFC.scala:14-26): 2^31-1 semi-normalized lon/lat */
int gm_legacy_z2_index(gm_ctx* ctx, const double* x, const double* y, int64_t n, int lenient, int64_t* z,
                       uint8_t* status, gm_batch_status* summary);
int gm_legacy_z2_invert(gm_ctx* ctx, const int64_t* z, int64_t n, double* x, double* y);

/* ------------------------------------------------------------------ statistics */
/* Z3Histogram.observe / unobserve over a batch of point features (utils/stats/Z3Histogram.scala:101-128;
   a point's safeCentroid is the point): toKey (:80-86) = BinnedTime(period) + Z3SFC(period).index,
   lenient only for unobserve; a feature whose toKey throws is skipped (the Scala code logs a warning)
   and counted in tally[0].  The bin is LongBinning(length, (minZ, maxZ)).directIndex
   (utils/stats/BinnedArray.scala:185-201).  The histogram's binMap is the dense block
   counts[(timeBin - bin_lo) * length + i] (int64) for time bins bin_lo .. bin_lo + n_bins - 1 with
   present[timeBin - bin_lo] != 0 marking the bins binMap holds (observe sets it: getOrElseUpdate;
   unobserve only touches present bins: binMap.get(..).foreach).  Features whose time bin lies outside
   the window are counted in tally[1] and not added, so a caller can widen the window and re-run them.
   counts, present and tally (int64[2]) are device arrays and are accumulated into, never cleared; the
   call is asynchronous on the context stream. */
int gm_z3_histogram(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n, int period,
                    int length, int unobserve, int bin_lo, int n_bins, uint8_t* present, int64_t* counts,
                    int64_t* tally);

/* ------------------------------------------------------------------ density (heatmap) scan */
/* DensityScan over point features (idx/iterators/DensityScan.scala:29-49, 201-212): every feature that
   passed the scan's filters is rendered into a RenderingGrid of width x height pixels over an envelope
   (geomesa-utils/.../geotools/RenderingGrid.scala:43-49), in FP64 with the JVM's semantics:
     GridSnap(env, width, height) (geomesa-utils/.../geotools/GridSnap.scala:32-36):
       dx = (xmax - xmin) / width, dy = (ymax - ymin) / height;
     GridSnap.i(x) (GridSnap.scala:60-66): -1 when x < xmin || x > xmax, else
       floor((x - xmin) / dx).toInt (a true division; toInt saturates) clamped to width - 1; j(y) likewise
       (GridSnap.scala:74-80);
     RenderingGrid.render(Point, w) (RenderingGrid.scala:43-49): j = j(y); when j != -1, pixel (i, j) += w
       for every i of translate(x);
     translate / widen (RenderingGrid.scala:299-330): below xmin, xt = x + 360 * ceil((xmin - x) / 360),
       nothing when xt > xmax; above xmax, xt = x - 360 * ceil((x - xmax) / 360), nothing when xt < xmin;
       when xmax - xmin > 360 the grid renders copies: xup = xt - 360 * floor((xt - xmin) / 360),
       while (xup <= xmax) { i(xup); xup += 360 }; otherwise the one column i(xt).  No multiply-add is fused;
     the weight (DensityScan.scala:247-259) is 1.0 (EqualWeight, weight = NULL) or a numeric column
       (WeightByNumber); a null weight is 0.0, which the caller writes.
   A MultiPoint renders every one of its points with the slot's weight (RenderingGrid.scala:57-64).

   Three places where the dense grid cannot follow the reference's map of pixels, each counted in
   tally (device int64[3], accumulated into):
     tally[0]  unrenderable rows, skipped: a null Arrow slot (the reference throws a
               NullPointerException), a non-finite x or y, |x| > 2^31.  In the reference a NaN ordinate
               fails both range checks of GridSnap and lands in column or row 0, and an infinite or huge x
               makes xt NaN or widen's loop endless (xup += 360 is absorbed).  gm_arrow_points_to_columns
               writes NaN for null slots, so this is also the null rule of x / y columns.  For a MultiPoint
               a null slot counts once and every such tuple counts;
     tally[1]  pixel additions whose column came out -1, dropped: xt and xup are rounded and can land an
               ulp below xmin, where the reference adds to the map key (-1, j), a pixel outside the grid;
     tally[2]  entries of ids outside [0, n), skipped and never read through.

   The grid description.  workgroups: 0 = the default launch (one resident wave of workgroups), else the
   launch's workgroup count (raised when a workgroup's counters could otherwise wrap).  path: 0 =
   automatic, 1 = workgroup-private counters in LDS, flushed with one device atomic per nonzero pixel,
   2 = one FP64 device atomic per addition.  Both exist so tests reach every path; an unweighted grid never
   changes with them (integer sums below 2^53 are exact in any order), a weighted one only in the
   order of its FP64 additions. */
typedef struct {
  double xmin, ymin, xmax, ymax;
  int32_t width, height;
  int32_t workgroups;
  int32_t path;
} gm_density_grid;

/* Renders rows 0 .. n-1 of the device columns x / y (weight: NULL = 1.0) into grid (device, FP64,
   pixel (i, j) at [j * width + i]).  Selection, at most one of: mask (bit r%64 of word r/64 set = render
   row r; ceil(n/64) words, as the filter scans write them; bits at and above n are ignored) or ids (n_ids
   rows to render, in any order; a row named twice renders twice), as a table query returns them.
   grid and tally are accumulated into and never cleared, and the call is stream-ordered, as
   gm_z3_histogram: batches, and the grids of several ranks, add.  Columns, mask, ids, grid and tally need
   8-B alignment; x, y and weight all 16-B aligned take the vector-load kernel.
   GM_E_INVALID, with a gm_last_error text: a NULL ctx, g, grid or tally; x or y NULL with n > 0; n < 0;
   width < 1 or height < 1; width * height > 2^31 - 1; xmax <= xmin or ymax <= ymin (the reference's 0/0 for
   a flat envelope is an accident and is not reproduced); a bound that is not finite or beyond 2^31 in
   magnitude; xmax - xmin > 360 * 64 (inside this domain widen's loop runs at most
   floor((xmax - xmin) / 360) + 2 times, which bounds the device loop); mask and ids both given; path
   outside 0..2, or path 1 for a grid that does not fit (more than 8 passes of 40,704 pixels, 20,352 with
   weights); workgroups < 0; a misaligned pointer. */
int gm_density_points(gm_ctx* ctx, const double* x, const double* y, const double* weight, int64_t n,
                      const uint64_t* mask, const int64_t* ids, int64_t n_ids, const gm_density_grid* g,
                      double* grid, int64_t* tally);
/* gm_density_points over the n slots of an Arrow GM_GEOM_POINT or GM_GEOM_MULTIPOINT column (64- or 32-bit
   ordinates, either axis order), read in place; weight, mask and ids are per slot. */
int gm_density_arrow(gm_ctx* ctx, const gm_geom_column* geom, const double* weight, int64_t n, const uint64_t* mask,
                     const int64_t* ids, int64_t n_ids, const gm_density_grid* g, double* grid, int64_t* tally);
/* Line features.  gm_density_points over the n slots of an Arrow GM_GEOM_LINESTRING or
   GM_GEOM_MULTILINESTRING column (64- or 32-bit ordinates, either axis order), read in place; weight, mask
   and ids are per slot.  Same grid description, validation, paths and accumulation as gm_density_points
   (every path valid there for a grid is valid here; an unweighted grid does not depend on path or
   workgroups); any other geometry type is GM_E_INVALID.  Stream-ordered; a GM_GEOM_MULTILINESTRING call
   waits for the stream once, to read the column's part count (its last slot offset).
   Polygons and GeometryCollections are not rendered: the reference fills them with java.awt's fillPolygon
   (RenderingGrid.scala:189-206), which has no restatement here.

   One linestring with vertices p[0 .. N-1] and weight w is RenderingGrid.render(LineString, weight)
   (RenderingGrid.scala:72-142) operation for operation; a MultiLineString renders each of its parts so
   (RenderingGrid.scala:150-157), every part starting afresh.
     Per vertex: I(p) = translate(p.x) (RenderingGrid.scala:299-330), the list of columns above -- one entry,
       one per turn for an envelope wider than 360, none when the wrapped x falls outside -- and
       J(p) = GridSnap.j(p.y) (GridSnap.scala:74-80).
     State: (iN, jN) = (-1, -1) at the start of the linestring (RenderingGrid.scala:74); segments
       n = 1 .. N-1 (p0 = p[n-1], p1 = p[n]) are taken in order (RenderingGrid.scala:85-92, 138).
     In-grid segment (I(p0), I(p1) not empty, J(p0), J(p1) != -1; RenderingGrid.scala:106-135): walk
       B = GridSnap.bresenhamLine(I(p0).head, J(p0), I(p1).head, J(p1)) (GridSnap.scala:94-126).  B is the
       single start pixel when both ends share a pixel; otherwise max(dX, dY) pixels from the start pixel,
       the end pixel left out (take(deltaX), GridSnap.scala:111, 123; GridSnapTest.scala:79-97 pins the
       lengths 9, 9, 9, 1, 9).  The minor axis steps by the reference's running FP64 error --
       deltaError = minor.toDouble / major; per pixel error += deltaError, and when error >= 0.5 the minor
       step is taken and error -= 1 (GridSnap.scala:101-110, 113-122) -- replayed as written: it is not the
       rational Bresenham ((dX, dY) = (10, 3) steps at x = 6, the rational walk at x = 5).
       The first pixel of B is written unless it equals (iN, jN) (RenderingGrid.scala:109-115); every later
       pixel is written (RenderingGrid.scala:120-134).  A write at (i, j) adds w there and at
       (i - I(p0).head + c, j) for every further entry c of I(p0), the start vertex's copies
       (RenderingGrid.scala:112-114, 124-126).  Afterwards (iN, jN) is the last pixel of B, written or not
       (RenderingGrid.scala:116-118, 129-131).  Every written pixel gets the whole w.
     Clipped segment (any other; RenderingGrid.scala:94-105): the reference renders
       createLineString(p0, p1).intersection(envelope) (JTS 1.20) as a fresh Point or LineString and leaves
       (iN, jN) alone.  Here the intersection is defined, on the raw ordinates (no translate), a = p0,
       b = p1, the rectangle the closed envelope:
         1. empty when the segment's own envelope misses the rectangle;
         2. an endpoint inside the closed rectangle is kept bit for bit;
         3. an endpoint e outside is replaced by a crossing, both ordinates from a, in unfused FP64 in the
            written order: with the vertical side X (xmin when e.x < xmin, xmax when e.x > xmax),
            (X, a.y + (X - a.x) * ((b.y - a.y) / (b.x - a.x))), valid when its y lies in [ymin, ymax]; with
            the horizontal side Y chosen likewise, (a.x + (Y - a.y) * ((b.x - a.x) / (b.y - a.y)), Y), valid
            when its x lies in [xmin, xmax]; the vertical one when both are valid, empty when none is;
         4. equal resulting ends are a Point, rendered by render(Point) above (RenderingGrid.scala:43-49);
         5. unequal ends are the two-vertex linestring a' -> b', in the segment's direction, rendered with
            a fresh (iN, jN); both ends lie in the envelope, so it is an in-grid segment.
       Parity-unpinned against JTS: the last-ulp rounding of a crossing (it moves a pixel only within an
       ulp of a pixel edge) and the direction of the piece (JTS may return b' -> a', which moves the
       left-out end pixel to the other end) are this definition's, not measured against
       LineString.intersection.
   What the dense grid leaves out, in the same tally:
     tally[0]  parts skipped whole, once per part: a null slot; a linestring part with any non-finite
               ordinate or any |x| > 2^31 (the other parts of the same MultiLineString still render);
     tally[1]  additions whose column falls outside [0, width): a -1 column of an ulp-low translate, as
               for points, and the copies of it;
     tally[2]  ids outside [0, n).
   A linestring of 0 or 1 vertices renders nothing and counts nothing. */
int gm_density_lines(gm_ctx* ctx, const gm_geom_column* geom, const double* weight, int64_t n, const uint64_t* mask,
                     const int64_t* ids, int64_t n_ids, const gm_density_grid* g, double* grid, int64_t* tally);
/* The grid as the sparse matrix DensityScan.encodeResult writes (DensityScan.scala:95-106): the cells
   with w != 0.0 into the device arrays i / j / w (cap entries each), ordered by column i, then row j --
   the order encodeResult groups by.  *n_cells (host) receives the cell count; GM_E_CAPACITY when it
   exceeds cap (no entry past cap is written; cap = 0 only counts, and i / j / w may then be NULL).
   Synchronises the context stream.  A pixel whose weights sum to zero is not reported; the reference's
   map would keep it with 0.0. */
int gm_density_sparse(gm_ctx* ctx, const double* grid, int32_t width, int32_t height, int64_t cap, int32_t* i,
                      int32_t* j, double* w, int64_t* n_cells);

/* ------------------------------------------------------------------ BIN track-record scan */
/* BinAggregatingScan (idx/iterators/BinAggregatingScan.scala:129-168): every feature that passed the
   scan's filters becomes little-endian records in one buffer (geomesa-utils/.../bin/
   BinaryOutputCallback.scala:28-41), 16 B, or 24 B with a label:
     offset 0   int32   trackId   convertToTrack (geomesa-utils/.../bin/BinaryOutputEncoder.scala:149-150)
     offset 4   int32   (dtg / 1000).toInt: Long division, truncating toward zero (-1 ms -> 0, -1999 ms
                        -> -1); toInt keeps the low 32 bits (it wraps); a null date is 0 (:153-154)
     offset 8   float32 lat       p.getY.toFloat (:295-301), the JVM's d2f: round to nearest even, overflow
     offset 12  float32 lon       p.getX.toFloat  to +-Inf, float denormals and -0.0 kept; under
                                  AxisOrder.LatLon lat = x and lon = y (:281-286)
     offset 16  int64   label     convertToLabel (:156-168), 24-B records only
   A point feature gives one record (ToValuesPoints[Labels], :326-343); a LineString one per vertex, in vertex
   order, with the feature's track, label and date (ToValuesLines[Labels], :345-377) or, given a date list,
   with dates(i) for vertex i, min(vertices, dates) records (ToValuesLinesDates[Labels], :379-419; a null
   list is empty, :317-320).  Polygons (safeCentroid) are not encoded.

   gm_bin_track / gm_bin_label turn an attribute column into the int32 track / int64 label column the
   encode reads (a track column is hashed once per table; a BIN query runs many times over it).  A null
   slot gives 0.  track = hashCode: GM_ATTR_INT32 the value; GM_ATTR_INT64 (int)(v ^ (v >>> 32));
   GM_ATTR_FLOAT64 the same fold over doubleToLongBits (every NaN is 0x7ff8000000000000 first; -0.0 keeps
   its sign bit); GM_ATTR_UTF8 String.hashCode, s[0] * 31^(n-1) + ... over UTF-16 code units in wrapping
   int32, a 4-byte UTF-8 sequence being two surrogate units.  With no track attribute the track is the hash
   of the feature id string (:247-250): the caller hashes its id column.  label: Number.longValue
   (GM_ATTR_INT32 sign-extends; GM_ATTR_FLOAT64 is the JVM's saturating d2l, NaN -> 0); GM_ATTR_UTF8 the
   first 8 UTF-8 bytes, byte i at bits 8i (a multi-byte character may be cut).  UTF-8 input is well
   formed (Arrow's contract); a malformed or truncated sequence gives an unspecified value and never
   reads outside the slot's bytes.  Device arrays, naturally aligned; stream-ordered; one lane per slot. */
#define GM_ATTR_INT32 1
#define GM_ATTR_INT64 2
#define GM_ATTR_FLOAT64 3
#define GM_ATTR_UTF8 4      /* Arrow Utf8: int32 offsets [n + 1] + bytes */
#define GM_ATTR_FLOAT32 5   /* the stats scans (gm_frequency_attr, gm_histogram_attr, gm_minmax_attr); gm_bin_track / gm_bin_label reject it */
typedef struct {
  int32_t type;              /* GM_ATTR_* */
  int32_t reserved;
  const void* values;        /* the values; GM_ATTR_UTF8: the bytes */
  const int32_t* offsets;    /* GM_ATTR_UTF8 only: slot i is bytes [offsets[i], offsets[i + 1]) */
  const uint8_t* validity;   /* NULL = no nulls */
  int64_t validity_offset;
} gm_attr_column;

int gm_bin_track(gm_ctx* ctx, const gm_attr_column* col, int64_t n, int32_t* track);
int gm_bin_label(gm_ctx* ctx, const gm_attr_column* col, int64_t n, int64_t* label);

typedef struct {
  int32_t sort;        /* 0: scan order; 1: by BinSorter.compare, stable */
  int32_t lat_lon;     /* 0: AxisOrder.LonLat (the default); 1: LatLon */
  int32_t reserved[2];
} gm_bin_opts;

/* Encodes rows 0 .. n-1 of the device columns x / y / t_ms (NULL: date 0) / track / label (NULL: 16-B
   records) into out (device, cap records).  Selection as gm_density_points: at most one of mask (bits at
   and above n are ignored) or ids (n_ids rows, in any order, a row named twice encoded twice; entries
   outside [0, n) are skipped and counted).
   Order.  Without sort: ascending row (no selection, mask) or the order of ids -- a table query returns its
   ids in table order, the reference's scan order -- and vertex order within a line.  With sort: by
   BinSorter.compare (idx/utils/bin/BinSorter.scala:38-79), the int32 at offset 4 compared signed, stable.
   The reference's quickSort (:155) leaves the order among equal seconds unspecified, so any tie order is
   its; the stable one makes the result fixed, and the stable sort of left ++ right, both sorted, is byte
   for byte BinSorter.mergeSort(left, right) (:115-145), which takes from left on ties.
   tally (device int64[3], accumulated into):
     tally[0]  records not written because the geometry is null (the reference throws a
               NullPointerException) or an ordinate is NaN (the float payload of a NaN after d2f is not
               portable); gm_arrow_points_to_columns writes NaN for null slots, so this is also the null
               rule of x / y columns.  +-Inf and values outside the float range are encoded;
     tally[1]  entries of ids outside [0, n), skipped and never read through;
     tally[2]  selected line slots whose date list length differs from the vertex count (the reference
               logs a warning and uses the minimum; so does this).
   *n_records (host) receives the full record count; GM_E_CAPACITY when it exceeds cap, and then out is
   not written; cap = 0 with out = NULL only counts.  Nothing past cap records is ever written; what out
   holds past *n_records records is unspecified.  The call synchronises the context stream for that
   readback, as gm_density_sparse.  Without a mask, and with room for every selected row (cap >= n, or
   n_ids), the records are first written in one pass on the assumption that every selected row gives one;
   a null geometry, a NaN or a bad id among them makes the count -> scan -> write passes run after it,
   and the result is the same.  Pointers need 8-B alignment; x, y, t_ms and label all 16-B aligned take
   the vector-load kernel, a 16-B aligned out 16-B stores.
   GM_E_INVALID, with a gm_last_error text: a NULL ctx, o, tally or n_records; x, y or track NULL with
   n > 0 (without a track attribute, hash the feature ids with gm_bin_track); n, n_ids or cap negative; a
   NULL out with cap > 0; mask and ids both given; sort or lat_lon outside 0..1; more than 2^32 - 1
   records with sort; a misaligned pointer. */
int gm_bin_points(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, const int32_t* track,
                  const int64_t* label, int64_t n, const uint64_t* mask, const int64_t* ids, int64_t n_ids,
                  const gm_bin_opts* o, uint8_t* out, int64_t cap, int64_t* n_records, int64_t* tally);
/* gm_bin_points over the n slots of an Arrow GM_GEOM_POINT or GM_GEOM_LINESTRING column (64- or 32-bit
   ordinates, either axis order), read in place; dtg (NULL, or a null slot: date 0), track, label, mask and
   ids are per slot.  date_off / dates (both NULL: the slot's single date) give a line column its date
   list: slot i's dates are dates[date_off[i] .. date_off[i + 1]) (a null element is date 0; a null list
   has no entries).  Also GM_E_INVALID: another geometry type; exactly one of date_off / dates; dates with
   a GM_GEOM_POINT column.  A null line slot counts once in tally[0], a NaN vertex once each.  A line
   column takes a second readback (the vertices its selection asks for). */
int gm_bin_arrow(gm_ctx* ctx, const gm_geom_column* geom, const gm_time_column* dtg, const int32_t* date_off,
                 const gm_time_column* dates, const int32_t* track, const int64_t* label, int64_t n,
                 const uint64_t* mask, const int64_t* ids, int64_t n_ids, const gm_bin_opts* o, uint8_t* out,
                 int64_t cap, int64_t* n_records, int64_t* tally);
/* The stable sort by BinSorter.compare of n_records records of record_bytes (16 or 24) each, in (device)
   into out (device, another buffer).  A concatenation of sorted batches comes out as their merge
   (BinSorter.mergeSort, BinSorter.scala:85-145), so the batches of several ranks combine through it.
   GM_E_INVALID: record_bytes other than 16 / 24; n_records negative or above 2^32 - 1; NULL, misaligned or
   aliased buffers.  Device temporaries: 24 B per record plus gm_sort_keys's.  Synchronises the
   context stream, as gm_sort_keys. */
int gm_bin_sort(gm_ctx* ctx, const uint8_t* in, int64_t n_records, int32_t record_bytes, uint8_t* out);

/* ------------------------------------------------------------------ Frequency / Z3Frequency (count-min) */
/* The two count-min stats of a stats scan (idx/iterators/StatsScan.scala:94-109), which the stats-based cost
   estimator reads (idx/stats/StatsBasedEstimator.scala:310-324): Frequency
   (geomesa-utils/.../stats/Frequency.scala) and Z3Frequency (.../stats/Z3Frequency.scala), each a map from a
   time bin to a CountMinSketch (geomesa-utils/.../clearspring/CountMinSketch.scala).  All integer, 64-bit
   wrapping as the JVM.
     The sketch (CountMinSketch.scala:181-203): depth rows of width Long counters and a size; width =
       ceil(2 / eps).toInt, depth = ceil(-ln(1 - confidence) / ln 2).toInt, hashA(i) =
       new java.util.Random(-27).nextInt(Int.MaxValue) for i < depth (Frequency.scala:213).  The caller
       computes the three (the library does no floating point for the sketch); the defaults eps 0.005,
       confidence 0.95 give width 400, depth 5, hashA 575626169, 278924161, 1519804117, 1200401393, 783957587.
     hash(item, i) (CountMinSketch.scala:48-57): h = hashA(i) * item, wrapping; h += h >> 32, an arithmetic
       shift; h &= 2^31 - 1; the bucket is h.toInt % width.
     add(item, 1) (:59-73): table(i)(hash(item, i)) += 1 for every i < depth, size += 1.
     estimateCount(item) (:96-105): the minimum over i of table(i)(hash(item, i)).
     The mask of the curve keys (Frequency.scala:284-287): Long.MaxValue << (64 - precision), precision within
       0..64; the JVM takes the count mod 64, so precision 0 gives Long.MaxValue, as 64 does.
   The map of sketches is the dense block table[(bin - bin_lo) * depth * width + i * width + bucket] and
   size[bin - bin_lo] (device int64) over the time bins bin_lo .. bin_lo + n_bins - 1 -- per bin exactly what
   a JVM caller copies into sketch.table(i) and sketch._size, and what the serializer writes for a bin with
   size > 0 (geomesa-utils/.../stats/StatSerializer.scala:487-507, 546-567).  Merging (Frequency.scala:180-187,
   Z3Frequency.scala:127-131, CountMinSketch.scala:118-135) adds tables and sizes bin by bin; a sketch is a sum
   of per-row increments, so any row order, workgroup split or rank split gives the same block.

   workgroups, path: as gm_density_grid's.  path 1 = workgroup-private uint32 counters in LDS (depth * width + 1
   per time bin, 32,768 per pass, as many passes over the rows as the window needs), flushed with one device
   atomic per nonzero counter; path 2 = one 64-bit device atomic per increment; 0 = automatic: path 1 up to 64
   passes, path 2 beyond that and when one bin alone does not fit.  The result never depends on either. */
#define GM_CMS_MAX_DEPTH 32
typedef struct {
  int32_t depth, width;          /* 1..GM_CMS_MAX_DEPTH, >= 1 */
  int32_t bin_lo, n_bins;        /* the window of time bins, as gm_z3_histogram's */
  int32_t workgroups, path;
  int64_t hash_a[GM_CMS_MAX_DEPTH];
} gm_cms;

/* Z3Frequency.observe (Z3Frequency.scala:54-60, 104-115) over rows 0 .. n-1 of the device columns x / y / t_ms:
   (bin, offset) = BinnedTime(period)(t_ms), z = Z3SFC(period).index(x, y, offset) (not lenient) & mask, and
   add(z, 1) on that bin's sketch.  Selection (mask / ids / n_ids) exactly as gm_density_points.
   table, size and tally (device int64[3]) are accumulated into and never cleared, and the call is
   stream-ordered: batches, and the blocks of several ranks, add.
     tally[0]  rows skipped because the reference's toKey throws (a date BinnedTime rejects, a point outside
               the curve's bounds; Z3Frequency logs a warning and moves on) or an ordinate is NaN (which fails
               the bounds check; gm_arrow_points_to_columns writes NaN for null slots, so this is also the
               null rule of x / y columns);
     tally[1]  rows whose time bin lies outside the window: not added, so a caller can widen the window and
               run the new bins alone, as with gm_z3_histogram.  A row counts in tally[0] before it can here;
     tally[2]  entries of ids outside [0, n), skipped and never read through.
   Pointers need 8-B alignment; x, y and t_ms all 16-B aligned take the vector-load kernel.
   GM_E_INVALID, with a gm_last_error text: a NULL ctx, cms, table, size or tally; a column NULL with n > 0;
   n < 0; an unknown period; depth outside 1..GM_CMS_MAX_DEPTH; width < 1; n_bins < 1; a window outside the
   Short range (bin_lo < -32768 or bin_lo + n_bins > 32768); n_bins * depth * width > 2^31 - 1; the selection
   errors of gm_density_points (n_ids < 0, mask and ids both given); path outside 0..2, or path 1 when one
   bin's depth * width + 1 counters exceed 32,768; workgroups < 0; precision outside 0..64; a misaligned
   pointer. */
int gm_z3_frequency(gm_ctx* ctx, const double* x, const double* y, const int64_t* t_ms, int64_t n,
                    const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                    const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally);
/* Frequency.observe (Frequency.scala:159-168) of an attribute column.  The time bin is
   BinnedTime(period)(dtg).bin, and Frequency.DefaultTimeBin = 0 without a dtg column (NULL) or at a null
   date slot.  The key by the column's type (Frequency.scala:302-306):
     GM_ATTR_INT32    (long)(v / precision): Int division, truncating toward zero (-7 / 2 = -3)
     GM_ATTR_INT64    v / precision: Long division (java.lang.Long, and a Date as its epoch milliseconds)
     GM_ATTR_FLOAT32  Math.round(v * (float)precision): the float32 product, then the closest int
     GM_ATTR_FLOAT64  Math.round(v * (double)precision): the FP64 product, then the closest long
   Math.round takes ties toward +Infinity (-0.5 -> 0, 2.5 -> 3, 0.49999999999999994 -> 0), maps NaN to 0 and
   saturates; the product is not fused with anything.  A null attribute slot is not observed and counts
   nowhere.  Frequency.observe has no try: a date BinnedTime rejects makes the reference's scan throw; here
   the row is skipped and counted in tally[0].  tally[1], tally[2], selection, accumulation and the errors as
   gm_z3_frequency (precision there aside); also GM_E_INVALID: a NULL col; GM_ATTR_UTF8 (a string key hashes
   through com.clearspring's MurmurHash, which the reference tree does not hold) and unknown types; an
   integer column with precision < 1 (0 throws in the reference; negative divisors are not reproduced);
   values or millis NULL with n > 0 or not naturally aligned.  8-byte columns whose values and millis are
   16-B aligned take the vector-load kernel; 4-byte columns always take scalar loads. */
int gm_frequency_attr(gm_ctx* ctx, const gm_attr_column* col, const gm_time_column* dtg, int64_t n,
                      const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                      const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally);
/* Frequency.observe of a point geometry attribute (Frequency.scala:289-293): the key is
   Z2SFC.index(x, y) (not lenient) & mask, the time bin as gm_frequency_attr's.  The reference throws for a
   point outside the curve's bounds; here the row is skipped and counted in tally[0], as is a NaN ordinate
   and a rejected date.  Everything else as gm_z3_frequency. */
int gm_frequency_points(gm_ctx* ctx, const double* x, const double* y, const gm_time_column* dtg, int64_t n,
                        const uint64_t* mask, const int64_t* ids, int64_t n_ids, int period, int precision,
                        const gm_cms* cms, int64_t* table, int64_t* size, int64_t* tally);
/* estimateCount of n keys (device int64), one lane per key, into out (device int64).  bins NULL: the sum over
   the window's sketches -- Frequency.count(value), countDirect(value) (Frequency.scala:78, 117-118); else
   (device int16, as gm_z3_index_key writes them) the estimate in bins[i]'s sketch, 0 for a bin outside the
   window (:87, :128-129; Z3Frequency.scala:81).  Stream-ordered.  GM_E_INVALID: a NULL ctx, cms or table;
   n < 0; the sketch and window errors above; keys or out NULL with n > 0; a misaligned pointer. */
int gm_cms_estimate(gm_ctx* ctx, const gm_cms* cms, const int64_t* table, const int64_t* keys, const int16_t* bins,
                    int64_t n, int64_t* out);

/* ------------------------------------------------------------------ Histogram / MinMax of an attribute */
/* The two per-attribute stats the planner costs a strategy with: Histogram
   (geomesa-utils/.../stats/Histogram.scala over BinnedArray.scala) and MinMax (.../stats/MinMax.scala with
   clearspring/HyperLogLog.scala).  Bindings: Integer = GM_ATTR_INT32, Long and Date (epoch ms) =
   GM_ATTR_INT64, Float = GM_ATTR_FLOAT32, Double = GM_ATTR_FLOAT64.  String and Geometry bindings are not
   restated (GM_ATTR_UTF8 is GM_E_INVALID).  Nothing is fused (-ffp-contract=off) and every division is the
   correctly rounded IEEE one, float32 included.

   Binning (BinnedArray.scala:185-201, :284-350), `length` bins over the bounds [lo, hi], lo < hi:
     whole numbers  binSize = (double)(hi - lo) / length, the Long difference wrapping;
                    indexOf(v) = -1 when v < lo || v > hi, else i = d2i(floor((double)(v - lo) / binSize)), v - lo
                    wrapping, d2i the JVM's saturating conversion (NaN -> 0);
     float          the same in float32: binSize = (hi - lo) / (float)length, i = d2i(floor((double)((v - lo) /
                    binSize)));
     double         the same in FP64;
     then i < 0 || i > length gives -1 and i == length gives length - 1.
   A NaN passes both comparisons and floor(NaN) converts to 0: it counts in bin 0 and never expands.  An
   infinity expands to an infinite bound, after which the quotients are NaN and land in bin 0; no special case.
     bounds(i)      whole: lo' = lo + d2l(ceil(binSize * i)), hi' = max(lo', lo + d2l(floor(binSize * (i + 1)))),
                    lo' <= lo gives lo and hi' >= hi gives hi (an Int binding truncates with toInt);
                    float / double: (lo + binSize * i, lo + binSize * (i + 1)).
     medianValue(i) whole: lo + Math.round(binSize / 2 + binSize * i), hi when that exceeds hi;
                    float / double: lo + binSize / 2 + binSize * i.
   observe (Histogram.scala:74-89): counts(indexOf(v)) += 1; when indexOf(v) is -1, expandBins (:226-232) first:
   bounds (min(v, lo), max(v, hi)), the same length, copyInto(new, old), then add(v).  unobserve subtracts.
   copyInto (:260-292): for every source bin with count > 0, lo = toIndex(bounds(i).min), hi =
   toIndex(bounds(i).max), toIndex(x) = indexOf(x) in the target, or 0 / length - 1 for an x below / above it;
   lo == hi adds the count there, else size = hi - lo + 1, every bin of lo..hi gets count / size and bin
   lo + size / 2 gets count % size more (size <= 0 throws, and observe then drops the feature with a warning).
   So a histogram depends on which rows came before each expansion: ORDER IS PART OF THE CONTRACT.  The rows
   that expand are those whose indexOf under the running bounds is -1: a value below every earlier value and
   lo, or above every earlier value and hi (and, once a Long span has wrapped, values the wrapped arithmetic
   rejects).  gm_histogram_attr finds these records with a prefix-extrema scan, counts every row under the
   bounds that held when the reference saw it, and replays the expansions on the host.

   MinMax (MinMax.scala:51-62, :149-182): min and max by compareTo -- for Float and Double the total order
   with -0.0 < 0.0 and NaN above +Infinity -- and a HyperLogLog(10) of the values.  A float or double travels
   as the order key of its double: key = bits ^ ((bits >> 63) & INT64_MAX), its own inverse, every NaN first
   made 0x7ff8000000000000; Float widens to double exactly, which keeps the order.
   HyperLogLog (clearspring/HyperLogLog.scala:99-131, :168-178): 1,024 Int registers; for the 32-bit hash h
   of a value, j = h >>> 22, r = numberOfLeadingZeros((h << 10) | 513) + 1 (the source's `1 << 9 + 1`
   or-ed in whole), register[j] = max(register[j], r).  cardinality() sums 1.0 / (1 << register) in register
   order, counts the zero registers, estimate = (0.7213 / (1 + 1.079 / 1024)) * 1024 * 1024 / sum; an estimate
   <= 2.5 * 1024 gives Math.round(1024 * ln(1024 / zeros)), else Math.round(estimate).
   The hash is com.clearspring.analytics.hash.MurmurHash.hash(Object), outside the reference tree: PARITY
   UNPINNED, defined here as hashLong(key), key = the sign-extended Integer, the Long, doubleToRawLongBits,
   or floatToRawIntBits sign-extended, in wrapping 32-bit arithmetic:
     m = 0x5bd1e995; h = 0
     k = (int)key * m;          k ^= k >>> 24;  h ^= k * m
     k = (int)(key >> 32) * m;  k ^= k >>> 24;  h *= m;  h ^= k * m
     h ^= h >>> 13;  h *= m;  h ^= h >>> 15
   A Date's cardinality hashes Date.toString and is not restated. */
typedef struct {
  int32_t type;      /* GM_ATTR_INT32 / INT64 / FLOAT32 / FLOAT64 */
  int32_t length;    /* bins, >= 1 */
  int64_t lo, hi;    /* the bounds of a whole-number binding */
  double flo, fhi;   /* the bounds of a float (exactly widened) or double binding */
} gm_hist_state;
#define GM_HIST_MAX_SEGMENTS 256   /* records one round of gm_histogram_attr replays */
#define GM_HIST_LDS_BINS 16384     /* longest histogram the workgroup-private counters hold */

/* MinMax.observe over the selected, non-null rows of an attribute column (selection exactly as
   gm_frequency_attr: none, mask, or ids in the caller's order with repeats; a reduction, so order does not
   matter).  minmax (device int64[2], in/out): {min, max}, a whole number as itself, a float / double as its
   order key; the caller starts them at the binding's defaults.max / defaults.min.  registers (device
   int32[1024], in/out) or NULL for no cardinality.  tally (device int64[3], accumulated): {rows observed,
   unused, ids outside [0, n)}.  Stream-ordered, no readback.  GM_E_INVALID: a NULL ctx, col, minmax or
   tally; GM_ATTR_UTF8 or an unknown type; values NULL with n > 0 or not naturally aligned; n < 0; the
   selection errors; a misaligned output. */
int gm_minmax_attr(gm_ctx* ctx, const gm_attr_column* col, int64_t n, const uint64_t* mask, const int64_t* ids,
                   int64_t n_ids, int64_t* minmax, int32_t* registers, int64_t* tally);
/* Histogram.observe (sign +1) / unobserve (sign -1) over the selected, non-null rows of an attribute column, in
   selection order: ascending rows, or the order of ids.  state (host, in/out): the binding (col->type must
   equal state->type), the length and the bounds, which come back expanded.  counts (device int64[length],
   in/out).  tally (device int64[3], accumulated): {rows observed, expansions, ids outside [0, n)}.
   path: 0 automatic, 1 workgroup-private uint32 counters in LDS (length <= GM_HIST_LDS_BINS), 2 device atomics;
   the result never depends on it.  Works in rounds of at most GM_HIST_MAX_SEGMENTS records; a sorted column
   is a record per row and stays correct and slow, as in the reference.  Synchronises the context stream: it
   reads the record count back, and with records the counts.  GM_E_INVALID, with a gm_last_error text: a NULL
   ctx, col, state, counts or tally; GM_ATTR_UTF8, an unknown type or one that differs from the state's;
   length < 1; bounds with lo >= hi; sign other than +1 / -1; path outside 0..2, or path 1 with a longer
   histogram; values NULL with n > 0 or not naturally aligned; n < 0; the selection errors; a misaligned
   output. */
int gm_histogram_attr(gm_ctx* ctx, const gm_attr_column* col, int64_t n, const uint64_t* mask, const int64_t* ids,
                      int64_t n_ids, int sign, int path, gm_hist_state* state, int64_t* counts, int64_t* tally);
/* The host half, no context and no GPU (all pointers host).  values: n values of the binding's type.
   gm_hist_index_of: indexOf of each value into index[n].  gm_hist_bin_bounds / gm_hist_median: bounds(i) into
   out's bounds fields (type and length copied) / medianValue(i) into *iv or *fv; 0 <= i <= length as the
   reference allows.  gm_hist_copy_into: copyInto(to, from); GM_E_INVALID with to_counts untouched where the
   reference throws.  gm_hist_merge: a += b (Histogram.scala:123-154, checkEndpoints / getActualBounds
   :238-253); a_counts holds max(a->length, b->length) entries, a comes back with the merged bounds and
   length.  GM_E_INVALID: NULL pointers, a bad state, differing types, an index out of range. */
int gm_hist_index_of(const gm_hist_state* state, const void* values, int64_t n, int32_t* index);
int gm_hist_bin_bounds(const gm_hist_state* state, int32_t i, gm_hist_state* out);
int gm_hist_median(const gm_hist_state* state, int32_t i, int64_t* iv, double* fv);
int gm_hist_copy_into(const gm_hist_state* to, int64_t* to_counts, const gm_hist_state* from,
                      const int64_t* from_counts);
int gm_hist_merge(gm_hist_state* a, int64_t* a_counts, const gm_hist_state* b, const int64_t* b_counts);

/* ------------------------------------------------------------------ synthetic data (bench/tests) */
/* SplitMix64 keyed by (seed, index): lon U[lon0,lon1), lat U[lat0,lat1), t_ms U[t0,t1).  Each of x, y and
   t_ms is optional (NULL = that column is not generated; the others get the same values either way);
   all three NULL with n > 0 is GM_E_INVALID */
int gm_gen_points(gm_ctx* ctx, uint64_t seed, int64_t n, int64_t index_base, double lon0, double lon1,
                  double lat0, double lat1, int64_t t0, int64_t t1, double* x, double* y, int64_t* t_ms);

/* ------------------------------------------------------------------ attribute index table */
/* The attribute index (`attr`, version 8; att/ = idx/index/attribute/) of an attribute with index=true
   (AttributeIndex.defaults, att/AttributeIndex.scala:84-95) for the fixed-width bindings.  A row is
   [shard 1 B, if sharded][UTF-8 of the lexicoded value][0x00][tier bytes][feature id]
   (AttributeIndexKeySpace.toIndexKey, att/AttributeIndexKeySpace.scala:68-137); a null attribute writes no
   row.  The tier is the secondary key space the index was created with (att/AttributeIndex.scala:49-69):
     GM_ATTR_TIER_NONE  no tier bytes
     GM_ATTR_TIER_DATE  ByteArrays.toOrderedBytes(dtg ms): 8 B, sign bit flipped, big-endian; a null date is
                        Long.MinValue (att/DateIndexKeySpace.scala:48-56)
     GM_ATTR_TIER_Z3    [bin BE16][z BE64] of Z3IndexKeySpace.toIndexKey without its shard
                        (idx/index/z3/Z3IndexKeySpace.scala:63-95)
   The lexicoders.  AttributeIndexKey.typeEncode (att/AttributeIndexKey.scala:41,67) delegates to
   org.calrissian.mango 3.0.0 LexiTypeEncoders, which is outside the reference tree; this table is the
   definition here.  The key text is the ordered value v in lower-case hex digits, zero padded:
     Integer                       GM_ATTR_INT32    v = (uint32)(x ^ 0x80000000)              8 digits
     Long; Date, Timestamp (ms)    GM_ATTR_INT64    v = (uint64)(x ^ 0x8000000000000000)      16 digits
     Float                         GM_ATTR_FLOAT32  b = floatToIntBits(x) (every NaN 0x7fc00000);
                                                    v = b < 0 ? ~b : b ^ 0x80000000           8 digits
     Double                        GM_ATTR_FLOAT64  the same over doubleToLongBits            16 digits
   The Integer row is pinned by the reference's DefaultSplitterTest.scala:134-188 ("80000000", "8000000c",
   "7ffffff7").  Long, Float and Double are PARITY UNPINNED: nothing in the reference tree states their text.
   By the definition the byte order of the key text is the unsigned order of v; -0.0 sorts immediately below
   +0.0 and is a different key; NaN sorts above +infinity.
   Not built, GM_E_INVALID with a gm_last_error text: GM_ATTR_UTF8 (String: variable-length keys), List
   attributes, the XZ3 / Z2 / XZ2 tiers, the legacy index versions (legacy/AttributeIndexV2-V7), the join
   index and attribute-level visibility.
   Every entry takes the context and runs on its stream.  gm_attr_key_bytes only enqueues (asynchronous); the
   other three synchronise the context stream. */
#define GM_ATTR_TIER_NONE 0
#define GM_ATTR_TIER_DATE 1
#define GM_ATTR_TIER_Z3 2

/* toIndexKey's value part (att/AttributeIndexKeySpace.scala:112-117) over a column, its validity and
   validity_offset honoured: v_out (device, n entries) receives the ordered value of every NON-NULL slot in
   input order, rows_out (device, n entries) that slot's input row, *n_rows (host) their number; the entries
   past *n_rows are not written.  A null slot produces nothing (:113-114).  values need natural alignment,
   v_out and rows_out 8 B.  Synchronises the context stream: the row count is read back. */
int gm_attr_index_key(gm_ctx* ctx, const gm_attr_column* col, int64_t n, uint64_t* v_out, int64_t* rows_out,
                      int64_t* n_rows);

/* The row-key prefix of m table rows (att/AttributeIndexKeySpace.scala:116-134): out (device) gets
   m * key_len bytes, [shard, if shard != NULL][hex text of v: 8 B for the 32-bit types, else 16][0x00][tier].
   tier_kind GM_ATTR_TIER_DATE: t = epoch ms, 8 B; GM_ATTR_TIER_Z3: bin and t = z, 10 B; GM_ATTR_TIER_NONE: bin
   and t are not read.  key_len is constant per table, 9 to 28.  Asynchronous. */
int gm_attr_key_bytes(gm_ctx* ctx, int type, const uint8_t* shard, const uint64_t* v, int tier_kind,
                      const int16_t* bin, const int64_t* t, int64_t m, uint8_t* out);

/* Sorts the key columns into table order, the byte order of the rows above: shard, then v unsigned, then the
   tier -- bin as u16 then t as u64 (Z3: t = z; date: t = the ordered long, ms ^ 2^63, bin NULL; no tier: bin
   and t NULL).  Stable: rows of equal keys keep their input order, which stands for the feature id the store
   appends.  perm_out[i] = the input row of table row i.  shard / shard_out, bin / bin_out and t / t_out are
   each NULL together; bin needs t.  m < 2^32.  With a tier this is two stable gm_sort_keys passes, by tier
   and by (shard, v), with a gather between them and the permutations composed: device temporaries are
   gm_sort_keys's and 32 B per row from the stream's pool (+ 2 B with a bin, + 1 B with a shard).  Without a
   tier it is one gm_sort_keys.  Synchronises the context stream, as gm_sort_keys does. */
int gm_attr_sort(gm_ctx* ctx, const uint8_t* shard, const uint64_t* v, const int16_t* bin, const int64_t* t, int64_t m,
                 uint8_t* shard_out, uint64_t* v_out, int16_t* bin_out, int64_t* t_out, int64_t* perm_out);

/* A scan range over the key prefix, inclusive at both ends, compared lexicographically as (shard, v, b, t),
   every field unsigned: what getRangeBytes and the tier combination make of a query
   (att/AttributeIndexKeySpace.scala:150-190, 224-343; idx/api/GeoMesaFeatureIndex.scala:298-356), one per
   shard.  The fields of a column the table does not have (b without the Z3 tier, t without a tier) are not
   compared. */
typedef struct {
  uint64_t v_lo, v_hi;   /* ordered attribute value */
  uint64_t t_lo, t_hi;   /* tier low word: z, or the ordered date; 0 / all ones without a tier */
  uint16_t b_lo, b_hi;   /* tier high word: bin (Z3 tier); 0 / 0xffff otherwise */
  uint8_t  shard;
  uint8_t  reserved[3];
} gm_attr_range;

/* Seek-and-filter over a sorted attribute table (gm_attr_sort order).  The ranges (host array) are merged as
   gm_table_scan merges them, each one's row interval is found by binary search on the composite key, and the
   secondary filter runs on every candidate through gm_scan_filter's full filter: n_boxes > 0 with xmin = xmax
   = the features' x and ymin = ymax = y is, for point features, GeoTools BBOX (inclusive); during tests t_ms
   in (t_lo, t_hi), exclusive; rows maps a table row to its column row, else perm does.  A filter with
   z3filter, z2filter or polys is GM_E_INVALID here.  ids (device, optional) receives the matching rows in
   table order, mapped through perm (device, optional) to input rows; *n_match / *n_scanned (host) the match
   and candidate counts.  GM_E_CAPACITY, the NULL rules, ids_cap < 0 (GM_E_INVALID) and the synchronisation are
   gm_table_scan's; v, t, perm and ids need 8-B alignment. */
int gm_attr_table_scan(gm_ctx* ctx, const uint8_t* shard, const uint64_t* v, const int16_t* bin, const int64_t* t,
                       int64_t m, const gm_attr_range* ranges, int64_t n_ranges, const gm_scan_filter* f,
                       const int64_t* perm, int64_t* ids, int64_t ids_cap, int64_t* n_match, int64_t* n_scanned);

#ifdef __cplusplus
}
#endif
#endif /* GEOMESA_HIP_H */
