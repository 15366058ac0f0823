// gm_density.hip -- the density (heatmap) scan over point and line features on gfx950.
//
// Reference: DensityScan (idx/iterators/DensityScan.scala:29-49, 201-212) renders every feature that passed
// the scan's filters into a RenderingGrid: RenderingGrid.render(Point, weight)
// (geomesa-utils/.../geotools/RenderingGrid.scala:43-49) snaps y to a row with GridSnap.j
// (geomesa-utils/.../geotools/GridSnap.scala:74-80), turns x into the columns of translate / widen
// (RenderingGrid.scala:299-330: the 360-degree wrap and, for an envelope wider than 360, one copy per turn),
// each through GridSnap.i (GridSnap.scala:60-66), and adds the weight to those pixels.  The contract, with
// the three places where a dense grid cannot follow the reference's map, is in include/geomesa_hip.h.
//
// Shape: k_z3_hist_lds (gm_stats.hip) with a shorter read -- 16 B/row (24 with weights, + n/8 B of mask),
// 16-B non-temporal pair loads, one resident wave of workgroups.  Every workgroup keeps a block of pixel
// rows in LDS (uint32 counters unweighted, FP64 cells weighted: ds_add_u32 / ds_add_f64, no returning
// atomic) and flushes the nonzero ones with one global_atomic_add_f64 each.  A grid of more pixels than
// one LDS block takes up to DENS_MAX_PASSES passes over the rows, one block of pixel rows each (a row
// outside the pass's block leaves after the y snap); beyond that, and when the caller asks for it, every
// addition is a device atomic on the grid itself.  Measured on MI355X over 1B points (tools/
// density_scan_probe.py, profiles/density_scan_probe.json): an LDS pass 3.2 ms unweighted, 4.2 ms weighted;
// scattered FP64 device atomics 22.4 G/s (44.5 ms), the rate gm_stats.hip records for 64-bit integer ones.
// So every pass costs what atomics for about 8 % of the rows cost, and a selection decides the automatic
// path with the grid: ids take LDS counters only when one pass holds the grid (every pass gathers again);
// a mask's popcount is taken on the device and both forms are enqueued, each leaving at once unless the
// count falls on its side of DENS_PASS_SHARE x (passes - 1) x n (the call stays stream-ordered).
// The selection is gm_scan.hpp's RowSel (sel_row per entry, mask_pair per pair of rows; sel_check for the
// entry points' shared argument errors); gm_density_sparse's count -> scan -> total is its CountScan.
//
// Line features (gm_density_lines): RenderingGrid.render(LineString / MultiLineString, weight)
// (RenderingGrid.scala:72-157) with GridSnap.bresenhamLine (GridSnap.scala:94-126), a lane per segment, in
// the same kernel with another row loop (line_items) -- the same pixel block, passes, gate and flush.  A
// segment that leaves the envelope is clipped by the definition of include/geomesa_hip.h, which stands in
// for JTS's LineString.intersection(envelope): the last-ulp rounding of a crossing and the direction of
// the clipped piece are parity-unpinned against JTS.  Measured over 1B vertices (tools/
// density_lines_probe.py, profiles/density_lines_probe.json): device atomics 21.5-29.4 G additions/s, the
// point scan's rate; one LDS pass 18.6 ms over 20-vertex tracks of 1-3 pixels per step, 34 ms over
// segments of tens of pixels (261 G additions/s).
#include <algorithm>
#include <cmath>

#include "gm_arrow.hpp"
#include "gm_keys.hpp"
#include "gm_scan.hpp"

namespace gm {

constexpr int DTPB = 1024;
// LDS of the pixel block: the 160 KB of a workgroup less the kernel's few statics
constexpr int DENS_LDS_BYTES = 160 * 1024 - 1024;
constexpr int DENS_MAX_PASSES = 8;
constexpr double DENS_PASS_SHARE = 0.08;   // selected share of the rows at which one more LDS pass pays
// a thread of the multipoint kernel drains the workgroup's counters itself after this many additions of
// its own (see k_density): 1024 threads x 2^19 stays below the 2^32 a uint32 counter holds
constexpr uint32_t DENS_THREAD_DRAIN = 1u << 19;
static_assert((uint64_t)DTPB * DENS_THREAD_DRAIN < (1ull << 32), "thread drain: a counter could wrap");

enum : int { SRC_COLS = 0, SRC_POINT = 1, SRC_MULTI = 2, SRC_LINE = 3 };

struct DensArgs {
  RowSel sel;       // over the rows (columns) or slots (Arrow)
  double xmin, ymin, xmax, ymax;
  double dx, dy;    // GridSnap.scala:32-33
  double rdx, rdy;  // fl(1 / dx), fl(1 / dy): the quotient's estimate (grid_snap)
  int width, height;
  int wide;         // xMax - xMin > 360 (RenderingGrid.scala:33)
  int copies;       // bound of widen's loop: floor((xmax - xmin) / 360) + 2
  int row_lo, row_n;  // this pass adds into pixel rows [row_lo, row_lo + row_n)
  int first;        // this pass reports unrenderable rows and bad ids (each addition belongs to one pass,
                    // each row to all of them)
  // automatic path under a mask: the mask's popcount (device), and the count from which the LDS form runs
  const unsigned long long* gate;
  unsigned long long gate_min;
};

struct DensSrc {
  const double* x;
  const double* y;
  const double* w;      // per row / per slot; unread when unweighted
  ArrowPts pts;
  const int32_t* o0;    // multipoint, linestring: slot -> tuples; multilinestring: slot -> parts
  const int32_t* o1;    // multilinestring: part -> tuples
  const uint8_t* bad;   // lines: 1 for a part k_density_line_parts found unrenderable (linestring: part = slot)
  int multi;            // lines: a multilinestring column
};

// GridSnap.i / GridSnap.j (GridSnap.scala:60-80): -1 outside [lo, hi], else floor((v - lo) / d).toInt
// clamped to size - 1.  The quotient is the reference's division.  q = (v - lo) * fl(1 / d) only
// estimates it: both q and fl((v - lo) / d) lie within 3 * 2^-53 relative, i.e. (the quotient is at most
// size < 2^31) within 2^-20, of the real quotient, so when q is farther than 2^-16 from every integer
// no integer lies between the two and their floors are equal; otherwise (about 2^-15 of the rows, and
// every row on a cell edge) the division decides.  An infinite or NaN estimate (d underflowed to a
// denormal or 0) fails the comparison and takes the division as well.
__device__ __forceinline__ int grid_snap(double v, double lo, double hi, double d, double rd, int size) {
  if (v < lo || v > hi) return -1;
  const double t = v - lo;
  double q = t * rd;
  if (!(fabs(q - rint(q)) > 0x1p-16)) q = t / d;
  const int i = jvm_d2i(floor(q));
  return i >= size ? size - 1 : i;
}

// RenderingGrid.render(Point, weight) (RenderingGrid.scala:43-49) with translate / widen (:299-330)
// operation for operation; emit(i, j) is `pixels(i, j) += weight`.  skip: the rows the dense grid does
// not render (tally[0]); drop: additions whose column came out -1 (tally[1]).
template <class Emit>
__device__ __forceinline__ void render_point(double x, double y, const DensArgs& a, long long& skip, long long& drop,
                                             Emit emit) {
  if (!(fabs(x) <= 2147483648.0) || !(fabs(y) < INFINITY)) { ++skip; return; }
  const int j = grid_snap(y, a.ymin, a.ymax, a.dy, a.rdy, a.height);
  if (j < a.row_lo || j >= a.row_lo + a.row_n) return;   // j == -1, or a row of another pass
  double xt = x;
  if (x < a.xmin) {
    xt = x + 360.0 * ceil((a.xmin - x) / 360.0);
    if (xt > a.xmax) return;
  } else if (x > a.xmax) {
    xt = x - 360.0 * ceil((x - a.xmax) / 360.0);
    if (xt < a.xmin) return;
  }
  if (a.wide) {
    double xup = xt - 360.0 * floor((xt - a.xmin) / 360.0);
    for (int k = 0; k < a.copies && xup <= a.xmax; ++k) {
      const int i = grid_snap(xup, a.xmin, a.xmax, a.dx, a.rdx, a.width);
      if (i < 0) ++drop; else emit(i, j);
      xup += 360.0;
    }
  } else {
    const int i = grid_snap(xt, a.xmin, a.xmax, a.dx, a.rdx, a.width);
    if (i < 0) ++drop; else emit(i, j);
  }
}

// ------------------------------------------------------------------ line features
// RenderingGrid.render(LineString, weight) (RenderingGrid.scala:72-142), one lane per segment.  The
// segments of a linestring are coupled only through (iN, jN), the last pixel of the nearest earlier
// in-grid segment, which suppresses the first pixel of the next in-grid one.  That pixel never has to be
// carried: a walk of more than one pixel ends one major-axis step before its end vertex, so after an
// in-grid segment the next start pixel (the shared vertex) equals (iN, jN) exactly when that segment
// stayed in one pixel -- one more vertex to snap.  Only a segment that follows a clipped one looks
// further back (reenters_last_pixel), walking the vertices behind it until two in a row are in the grid.

// what the reference keeps of a vertex: translate(x) (RenderingGrid.scala:299-330) and GridSnap.j(y)
struct VSnap {
  bool ok;      // translate(x) is not empty and j != -1: a segment between two such vertices is in-grid
  int head;     // translate(x).head, -1 when x came out an ulp below xmin
  int j;
  double xup;   // the x of head; widen's further copies are xup + 360, + 360, ... while <= xmax
};

__device__ __forceinline__ VSnap snap_vertex(double x, double y, const DensArgs& a) {
  VSnap v{false, -1, grid_snap(y, a.ymin, a.ymax, a.dy, a.rdy, a.height), x};
  if (x < a.xmin) {
    v.xup = x + 360.0 * ceil((a.xmin - x) / 360.0);
    if (v.xup > a.xmax) return v;
  } else if (x > a.xmax) {
    v.xup = x - 360.0 * ceil((x - a.xmax) / 360.0);
    if (v.xup < a.xmin) return v;
  }
  if (a.wide) {
    v.xup = v.xup - 360.0 * floor((v.xup - a.xmin) / 360.0);
    if (!(v.xup <= a.xmax)) return v;
  }
  v.head = grid_snap(v.xup, a.xmin, a.xmax, a.dx, a.rdx, a.width);
  v.ok = v.j != -1;
  return v;
}

// GridSnap.bresenhamLine (GridSnap.scala:94-126): the start pixel alone when both ends share it, else
// max(dX, dY) pixels from the start, the end pixel left out (take(deltaX), :111, :123).  The minor axis
// steps by the reference's running FP64 error, replayed as written (for (dX, dY) = (10, 3) it steps a
// pixel later than the rational walk).  px(i, j) for every pixel but, when skip_first, the first.
template <class Px>
__device__ __forceinline__ void bresenham(int x0, int y0, int x1, int y1, bool skip_first, Px px) {
  const int dX = abs(x1 - x0), dY = abs(y1 - y0);
  if (dX == 0 && dY == 0) {
    if (!skip_first) px(x0, y0);
    return;
  }
  const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
  const bool xmajor = dX > dY;
  const int major = xmajor ? dX : dY;
  const double de = xmajor ? (double)dY / (double)dX : (double)dX / (double)dY;
  double err = 0.0;
  int x = x0, y = y0;
  for (int k = 0; k < major; ++k) {
    if (k > 0 || !skip_first) px(x, y);
    err += de;
    if (err >= 0.5) {
      err -= 1.0;
      x += sx;
      y += sy;
    } else if (xmajor) {
      x += sx;
    } else {
      y += sy;
    }
  }
}

// the pixels of an in-grid segment and the start vertex's copies of them (RenderingGrid.scala:107-135):
// copy k of pixel (i, j) is (i - head + i(xup + 360 k), j); add(i, j) sees columns outside the grid too
template <class Add>
__device__ __forceinline__ void draw_segment(const VSnap& p0, const VSnap& p1, bool skip_first, const DensArgs& a,
                                             Add add) {
  bresenham(p0.head, p0.j, p1.head, p1.j, skip_first, add);
  if (!a.wide) return;
  double xu = p0.xup + 360.0;
  for (int k = 1; k < a.copies && xu <= a.xmax; ++k) {
    const int off = grid_snap(xu, a.xmin, a.xmax, a.dx, a.rdx, a.width) - p0.head;
    bresenham(p0.head, p0.j, p1.head, p1.j, skip_first, [&](int i, int j) { add(i + off, j); });
    xu += 360.0;
  }
}

// vertex t of a line column
template <bool F32>
__device__ __forceinline__ VSnap line_vertex(const DensSrc& s, const DensArgs& a, int64_t t) {
  double x, y;
  arrow_tuple<F32>(s.pts.c, t, s.pts.flip, x, y);
  return snap_vertex(x, y, a);
}

// Segment t (vertices t - 1, t) is in-grid and segment t - 1 was clipped: is (iN, jN) the pixel (i0, j0)
// of vertex t - 1?  (iN, jN) is the last pixel of the nearest in-grid segment before t - 1 in the part
// [ps, ..); without one it still is (-1, -1), which no in-grid vertex has.
template <bool F32>
__device__ __forceinline__ bool reenters_last_pixel(const DensSrc& s, const DensArgs& a, int64_t ps, int64_t t,
                                                    int i0, int j0) {
  VSnap next{false, -1, -1, 0.0};   // vertex m + 1; t - 2 is outside, or segment t - 1 were in-grid
  for (int64_t m = t - 3; m >= ps; --m) {
    const VSnap cur = line_vertex<F32>(s, a, m);
    if (cur.ok && next.ok) {
      int li = cur.head, lj = cur.j;
      bresenham(cur.head, cur.j, next.head, next.j, false, [&](int i, int j) { li = i; lj = j; });
      return li == i0 && lj == j0;
    }
    next = cur;
  }
  return false;
}

// One end of the clipped segment a -> b (include/geomesa_hip.h, "the clipped segment"): e itself inside the
// closed envelope, else its crossing with the vertical side it lies beyond, else with the horizontal one;
// both ordinates from a, unfused (the unit is built with -ffp-contract=off).  false: no valid crossing.
__device__ __forceinline__ bool clip_end(double ex, double ey, double ax, double ay, double bx, double by,
                                         const DensArgs& a, double& ox, double& oy) {
  if (ex >= a.xmin && ex <= a.xmax && ey >= a.ymin && ey <= a.ymax) { ox = ex; oy = ey; return true; }
  if (ex < a.xmin || ex > a.xmax) {
    const double X = ex < a.xmin ? a.xmin : a.xmax;
    const double y = ay + (X - ax) * ((by - ay) / (bx - ax));
    if (y >= a.ymin && y <= a.ymax) { ox = X; oy = y; return true; }
  }
  if (ey < a.ymin || ey > a.ymax) {
    const double Y = ey < a.ymin ? a.ymin : a.ymax;
    const double x = ax + (Y - ay) * ((bx - ax) / (by - ay));
    if (x >= a.xmin && x <= a.xmax) { ox = x; oy = Y; return true; }
  }
  return false;
}

// segment t (vertices t - 1 -> t, t > ps) of the renderable part that starts at tuple ps
// (RenderingGrid.scala:85-138); add(i, j) is `pixels(i, j) += weight` before the grid's bounds
template <bool F32, class Add>
__device__ __forceinline__ void render_segment(const DensSrc& s, const DensArgs& a, int64_t ps, int64_t t,
                                               long long& drop, Add add) {
  double x0, y0, x1, y1;
  arrow_tuple<F32>(s.pts.c, t - 1, s.pts.flip, x0, y0);
  arrow_tuple<F32>(s.pts.c, t, s.pts.flip, x1, y1);
  const VSnap v0 = snap_vertex(x0, y0, a), v1 = snap_vertex(x1, y1, a);
  const int row_hi = a.row_lo + a.row_n;
  if (v0.ok && v1.ok) {
    if (max(v0.j, v1.j) < a.row_lo || min(v0.j, v1.j) >= row_hi) return;   // rows of other passes
    bool same = false;   // the start pixel is (iN, jN)
    if (t - 1 > ps) {
      const VSnap vp = line_vertex<F32>(s, a, t - 2);
      same = vp.ok ? vp.head == v0.head && vp.j == v0.j : reenters_last_pixel<F32>(s, a, ps, t, v0.head, v0.j);
    }
    draw_segment(v0, v1, same, a, add);
    return;
  }
  // RenderingGrid.scala:94-105: the piece of the raw segment inside the closed envelope, rendered as a
  // fresh Point or two-vertex LineString; (iN, jN) stays
  if (fmax(x0, x1) < a.xmin || fmin(x0, x1) > a.xmax || fmax(y0, y1) < a.ymin || fmin(y0, y1) > a.ymax) return;
  double ax, ay, bx, by;
  if (!clip_end(x0, y0, x0, y0, x1, y1, a, ax, ay) || !clip_end(x1, y1, x0, y0, x1, y1, a, bx, by)) return;
  if (ax == bx && ay == by) {
    long long none = 0;
    render_point(ax, ay, a, none, drop, add);
  } else {
    const VSnap c0 = snap_vertex(ax, ay, a), c1 = snap_vertex(bx, by, a);
    if (c0.ok && c1.ok) draw_segment(c0, c1, false, a, add);
  }
}

// The vertices of the selected slots, one per lane.  A wave takes 64 entries of the selection at a time,
// one per lane, scans their vertex counts and deals the vertices of all of them out 64 at a time, so
// short linestrings share a wave and a long one spreads over its lanes; a lane finds the slot of its
// vertex in the scanned counts (6 shuffles) and, in a multilinestring, the part in the slot's offsets.
// item(slot, part, ps, t): vertex t of the part that starts at tuple ps.  nulls: selected null slots;
// bad: ids outside [0, n).
template <int SEL, class Item>
__device__ __forceinline__ void line_items(const DensSrc& s, const RowSel& sel, long long& nulls, long long& bad,
                                           Item item) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (DTPB / 64);
  for (int64_t base = ((int64_t)blockIdx.x * (DTPB / 64) + (threadIdx.x >> 6)) * 64; base < sel.units;
       base += nwaves * 64) {
    const int64_t u = base + lane;
    int64_t r = 0;
    const int k = u < sel.units ? sel_row<SEL>(sel, u, r) : 0;
    if (k < 0) ++bad;
    bool live = k > 0;
    if (live && !arrow_valid(s.pts.valid, s.pts.voff, r)) { ++nulls; live = false; }
    int32_t pa = 0, pb = 0;
    int64_t t0 = 0, cnt = 0;
    if (live) {
      pa = s.o0[r];
      pb = s.o0[r + 1];
      t0 = s.multi ? s.o1[pa] : pa;
      cnt = (s.multi ? s.o1[pb] : pb) - t0;
      if (cnt < 0) cnt = 0;
    }
    int64_t inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    const int64_t total = __shfl(inc, 63, 64), first = t0 - (inc - cnt);   // vertex q of the wave is tuple first + q
    for (int64_t q0 = 0; q0 < total; q0 += 64) {
      const int64_t q = min(q0 + lane, total - 1);
      int o = 0;   // the lanes whose scanned count is <= q: the owner of vertex q
#pragma unroll
      for (int step = 32; step > 0; step >>= 1)
        if (__shfl(inc, o + step - 1, 64) <= q) o += step;
      const int64_t t = __shfl(first, o, 64) + q, rr = __shfl(r, o, 64);
      int32_t lo = __shfl(pa, o, 64), hi = __shfl(pb, o, 64);
      if (q0 + lane >= total) continue;
      if (!s.multi) {
        item(rr, rr, (int64_t)lo, t);
      } else {
        while (hi - lo > 1) {   // the last part that starts at or before t: empty parts start where it does
          const int32_t m = lo + ((hi - lo) >> 1);
          if (s.o1[m] <= t) lo = m; else hi = m;
        }
        item(rr, (int64_t)lo, (int64_t)s.o1[lo], t);
      }
    }
  }
}

// SRC: x / y columns, an Arrow point column, an Arrow multipoint column or an Arrow linestring /
// multilinestring column (F32: Float4 ordinates).
// SEL: every row, the rows of a mask, or the rows ids names (gm_scan.hpp's RowSel).  LDS: the pass's pixel rows live in LDS
// (uint32 counters, or FP64 cells when WEIGHTED) and are flushed at the end; else every addition is a
// device atomic.  VEC (columns, no ids): 16-B pair loads, software-pipelined as k_z3_hist_lds.
//
// A uint32 counter cannot wrap: a row adds at most a.copies times, and launch_density sizes the launch so
// a workgroup sees fewer than 2^31 / copies rows.  A multipoint slot has no such bound (one slot can
// hold 2^31 tuples), nor has a linestring (it can cross one pixel any number of times), so there a thread
// that has added DENS_THREAD_DRAIN times drains every counter itself with atomic exchanges: between two
// exchanges of a counter no thread adds to it more often than that.
template <int SRC, int SEL, bool WEIGHTED, bool LDS, bool VEC, bool F32>
__global__ __launch_bounds__(DTPB) void k_density(DensSrc s, DensArgs a, double* __restrict__ grid,
                                                  unsigned long long* __restrict__ tally) {
  if (a.gate && (*a.gate >= a.gate_min) != LDS) return;   // the other form runs (uniform: before any barrier)
  extern __shared__ uint64_t dens_lds[];
  uint32_t* cnt = (uint32_t*)dens_lds;   // [row_n * width] (!WEIGHTED)
  double* cell = (double*)dens_lds;      // [row_n * width] (WEIGHTED)
  __shared__ unsigned long long s_tally[3];
  const int total = LDS ? a.row_n * a.width : 0;
  if (WEIGHTED) for (int i = threadIdx.x; i < total; i += DTPB) cell[i] = 0.0;
  else for (int i = threadIdx.x; i < total; i += DTPB) cnt[i] = 0u;
  if (threadIdx.x < 3) s_tally[threadIdx.x] = 0ull;
  __syncthreads();
  double* gpass = grid + (int64_t)a.row_lo * a.width;   // the pass's pixel rows
  long long skip = 0, drop = 0, bad = 0;
  uint32_t since = 0;
  auto emit = [&](int i, int j, double w) {
    if (LDS) {
      const int c = (j - a.row_lo) * a.width + i;
      if (WEIGHTED) {
        atomicAdd(&cell[c], w);
      } else {
        atomicAdd(&cnt[c], 1u);
        if ((SRC == SRC_MULTI || SRC == SRC_LINE) && ++since == DENS_THREAD_DRAIN) {
          for (int k = 0; k < total; ++k) {
            const uint32_t v = atomicExch(&cnt[k], 0u);
            if (v) atomicAdd(&gpass[k], (double)v);
          }
          since = 0;
        }
      }
    } else {
      double* p = &grid[(int64_t)j * a.width + i];
      if (!WEIGHTED) atomicAdd(p, 1.0);
      else if (w != 0.0) atomicAdd(p, w);
    }
  };
  auto point = [&](double x, double y, double w) {
    render_point(x, y, a, skip, drop, [&](int i, int j) { emit(i, j, w); });
  };
  auto row = [&](int64_t r) {   // 0 <= r < a.sel.n
    if (SRC == SRC_COLS) {
      point(s.x[r], s.y[r], WEIGHTED ? s.w[r] : 1.0);
    } else {
      if (!arrow_valid(s.pts.valid, s.pts.voff, r)) { ++skip; return; }   // the reference throws an NPE
      const double w = WEIGHTED ? s.w[r] : 1.0;
      double x, y;
      if (SRC == SRC_POINT) {
        arrow_tuple<F32>(s.pts.c, r, s.pts.flip, x, y);
        point(x, y, w);
      } else {   // RenderingGrid.render(MultiPoint, weight), RenderingGrid.scala:57-64
        for (int64_t t = s.o0[r], e = s.o0[r + 1]; t < e; ++t) {
          arrow_tuple<F32>(s.pts.c, t, s.pts.flip, x, y);
          point(x, y, w);
        }
      }
    }
  };
  const int64_t stride = (int64_t)gridDim.x * DTPB;
  if constexpr (SRC == SRC_LINE) {
    // RenderingGrid.render(LineString / MultiLineString, weight) (RenderingGrid.scala:72-157): every part
    // starts afresh; its first vertex has no segment and reports the part when it is unrenderable
    line_items<SEL>(s, a.sel, skip, bad, [&](int64_t r, int64_t p, int64_t ps, int64_t t) {
      const bool out = s.bad[p];
      if (t == ps) skip += out;
      if (t == ps || out) return;
      const double w = WEIGHTED ? s.w[r] : 1.0;
      render_segment<F32>(s, a, ps, t, drop, [&](int i, int j) {
        if (j < a.row_lo || j >= a.row_lo + a.row_n) return;   // a row of another pass
        if ((unsigned)i >= (unsigned)a.width) ++drop; else emit(i, j, w);
      });
    });
  } else if constexpr (VEC) {
    const dv2* x2 = (const dv2*)s.x;
    const dv2* y2 = (const dv2*)s.y;
    const dv2* w2 = (const dv2*)s.w;
    const int64_t np = a.sel.n >> 1;
    constexpr int HU = 2;
    dv2 xa[HU], ya[HU], wa[HU];
    uint64_t ma[HU];
    // pair q = rows 2q and 2q + 1, both in mask word q >> 5.  Unconditional (clamped) loads, so the
    // compiler can count them and bin the current pairs under the next ones' latency (k_z3_hist_lds)
    auto load = [&](int64_t q, dv2& xv, dv2& yv, dv2& wv, uint64_t& mv) {
      const int64_t qc = q < np ? q : np - 1;
      xv = ld_stream(&x2[qc]);
      yv = ld_stream(&y2[qc]);
      if (WEIGHTED) wv = ld_stream(&w2[qc]);
      if (SEL == SEL_MASK) mv = a.sel.mask[qc >> 5];
    };
    const int64_t p0 = (int64_t)blockIdx.x * DTPB;
    if (p0 < np) {
#pragma unroll
      for (int u = 0; u < HU; ++u) load(p0 + threadIdx.x + u * stride, xa[u], ya[u], wa[u], ma[u]);
    }
    for (int64_t pb = p0; pb < np; pb += HU * stride) {
      const int64_t p = pb + threadIdx.x, pn = p + HU * stride;
      dv2 xb[HU], yb[HU], wb[HU];
      uint64_t mb[HU];
#pragma unroll
      for (int u = 0; u < HU; ++u) load(pn + u * stride, xb[u], yb[u], wb[u], mb[u]);
#pragma unroll
      for (int u = 0; u < HU; ++u) {
        const int64_t q = p + u * stride;
        if (q < np) {
          bool se = true, so = true;
          if (SEL == SEL_MASK) mask_pair(ma[u], q, se, so);
          if (se) point(xa[u].x, ya[u].x, WEIGHTED ? wa[u].x : 1.0);
          if (so) point(xa[u].y, ya[u].y, WEIGHTED ? wa[u].y : 1.0);
        }
        xa[u] = xb[u]; ya[u] = yb[u]; wa[u] = wb[u]; ma[u] = mb[u];
      }
    }
    if ((a.sel.n & 1) && blockIdx.x == 0 && threadIdx.x == 0 && (SEL != SEL_MASK || mask_bit(a.sel.mask, a.sel.n - 1)))
      row(a.sel.n - 1);
  } else {
    for (int64_t u = (int64_t)blockIdx.x * DTPB + threadIdx.x; u < a.sel.units; u += stride) {
      int64_t r;
      const int k = sel_row<SEL>(a.sel, u, r);
      if (k > 0) row(r); else if (k < 0) ++bad;
    }
  }
  if (skip) atomicAdd(&s_tally[0], (unsigned long long)skip);
  if (drop) atomicAdd(&s_tally[1], (unsigned long long)drop);
  if (bad) atomicAdd(&s_tally[2], (unsigned long long)bad);
  __syncthreads();
  if (LDS) {
    // integer partial sums below 2^53 are exact in any order: the unweighted grid is reproducible
    for (int i = threadIdx.x; i < total; i += DTPB) {
      if (WEIGHTED) { if (cell[i] != 0.0) atomicAdd(&gpass[i], cell[i]); }
      else if (cnt[i]) atomicAdd(&gpass[i], (double)cnt[i]);
    }
  }
  if (threadIdx.x == 0) {
    if (a.first && s_tally[0]) atomicAdd(&tally[0], s_tally[0]);
    if (s_tally[1]) atomicAdd(&tally[1], s_tally[1]);
    if (a.first && s_tally[2]) atomicAdd(&tally[2], s_tally[2]);
  }
}

// rows a mask selects: the popcount of its first n bits
__global__ __launch_bounds__(256) void k_density_mask_count(const uint64_t* __restrict__ mask, int64_t n,
                                                            unsigned long long* __restrict__ count) {
  const int64_t words = (n + 63) >> 6;
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
    uint64_t m = mask[i];
    if (i == words - 1 && (n & 63)) m &= (1ull << (n & 63)) - 1;
    c += __popcll(m);
  }
  if (c) atomicAdd(count, c);
}

// Marks the parts of the selected slots that the dense grid does not render: any ordinate not finite, or
// |x| > 2^31 (render_point's rule, for the whole part).  bad[part] is cleared before; lanes that find the
// same part store the same byte.
template <int SEL, bool F32>
__global__ __launch_bounds__(DTPB) void k_density_line_parts(DensSrc s, RowSel sel, uint8_t* __restrict__ bad) {
  long long nulls = 0, ids = 0;
  line_items<SEL>(s, sel, nulls, ids, [&](int64_t, int64_t p, int64_t, int64_t t) {
    double x, y;
    arrow_tuple<F32>(s.pts.c, t, s.pts.flip, x, y);
    if (!(fabs(x) <= 2147483648.0) || !(fabs(y) < INFINITY)) bad[p] = 1;
  });
}

// pixel rows one LDS pass holds, and the passes a grid takes (DENS_MAX_PASSES + 1: it does not fit)
inline int dens_rows(const gm_density_grid* g, bool weighted) {
  const int cells = DENS_LDS_BYTES / (weighted ? 8 : 4);
  return std::min(g->height, cells / g->width);
}
inline int dens_passes(const gm_density_grid* g, bool weighted) {
  const int rows = dens_rows(g, weighted);
  if (rows < 1) return DENS_MAX_PASSES + 1;
  return std::min((g->height + rows - 1) / rows, DENS_MAX_PASSES + 1);
}

// parts: the parts of a line column (SRC_LINE), for the marks of the unrenderable ones
int launch_density(gm_ctx* ctx, int src, bool f32, DensSrc s, RowSel rows, const gm_density_grid* g, double* grid,
                   int64_t* tally, int64_t parts = 0) {
  DensArgs a;
  a.sel = rows;
  a.xmin = g->xmin; a.ymin = g->ymin; a.xmax = g->xmax; a.ymax = g->ymax;
  a.width = g->width; a.height = g->height;
  a.dx = (g->xmax - g->xmin) / g->width;
  a.dy = (g->ymax - g->ymin) / g->height;
  a.rdx = 1.0 / a.dx;
  a.rdy = 1.0 / a.dy;
  a.wide = g->xmax - g->xmin > 360.0;
  a.copies = (int)std::floor((g->xmax - g->xmin) / 360.0) + 2;
  const bool weighted = s.w != nullptr;
  const int sel = sel_of(rows);
  const int fit = dens_passes(g, weighted);
  const int64_t n = a.sel.n, units = a.sel.units;
  // the automatic path (see the head of this file); gated: decided on the device by the mask's popcount
  const bool lds = g->path == 1 || (g->path == 0 && fit <= DENS_MAX_PASSES && (sel != SEL_IDS || fit == 1));
  const bool gated = g->path == 0 && sel == SEL_MASK && fit > 1 && fit <= DENS_MAX_PASSES;
  DevTemps tmp(ctx->stream);
  a.gate = nullptr;
  a.gate_min = 0;
  if (gated) {
    unsigned long long* count;
    const int rc = tmp.alloc_async(16, &count);
    if (rc) return rc;
    GM_HIP(hipMemsetAsync(count, 0, 16, ctx->stream));
    hipLaunchKernelGGL(k_density_mask_count, dim3(grid_for((n + 63) >> 6, 256 * 16)), dim3(256), 0, ctx->stream,
                       a.sel.mask, n, count);
    GM_CHECK_LAUNCH();
    a.gate = count;
    a.gate_min = (unsigned long long)(DENS_PASS_SHARE * (fit - 1) * (double)n);
  }
  const bool vec = src == SRC_COLS && sel != SEL_IDS && aligned16(s.x) && aligned16(s.y) && aligned16(s.w);
  int cus = 256;
  GM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (src == SRC_LINE) {   // once per call: every pass and both forms of a gated call read the marks
    uint8_t* bad;
    const int rc = tmp.alloc_async((size_t)parts, &bad);
    if (rc) return rc;
    GM_HIP(hipMemsetAsync(bad, 0, (size_t)std::max<int64_t>(parts, 1), ctx->stream));
    s.bad = bad;
    const int64_t wgs = std::min<int64_t>((int64_t)cus * 2, std::max<int64_t>((units + DTPB - 1) / DTPB, 1));
    const int prc = with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) {
      return with_flags([&](auto F) -> int {
        hipLaunchKernelGGL((k_density_line_parts<E(), F()>), dim3((unsigned)wgs), dim3(DTPB), 0, ctx->stream, s,
                           a.sel, bad);
        GM_CHECK_LAUNCH();
        return GM_OK;
      }, f32);
    });
    if (prc) return prc;
  }
  auto run = [&](bool in_lds) -> int {
    const int rows = in_lds ? dens_rows(g, weighted) : g->height;
    const int passes = (g->height + rows - 1) / rows;
    for (int k = 0; k < passes; ++k) {
      a.row_lo = k * rows;
      a.row_n = std::min(rows, g->height - a.row_lo);
      a.first = k == 0;
      const size_t bytes = in_lds ? std::max<size_t>((size_t)a.row_n * a.width * (weighted ? 8 : 4), 8) : 0;
      const int per_cu = bytes <= 72 * 1024 ? 2 : 1;   // 2 x 1024 threads is the CU's wave limit
      // a workgroup's rows x copies stay below 2^31, so neither a uint32 LDS counter nor a pixel's count wraps
      const int64_t need = units / ((int64_t)(1u << 30) / a.copies) + 1;
      int64_t wgs = std::min<int64_t>((int64_t)cus * per_cu, std::max<int64_t>((units + DTPB - 1) / DTPB, 1));
      if (g->workgroups > 0) wgs = g->workgroups;
      wgs = std::max(wgs, need);
      auto go = [&](auto kern) -> int {
        GM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(DTPB), bytes, ctx->stream, s, a, grid,
                           (unsigned long long*)tally);
        GM_CHECK_LAUNCH();
        return GM_OK;
      };
      // the switches that exist for a source: vector loads for columns, Float4 for Arrow tuples
      const int rc = with_value<SRC_COLS, SRC_POINT, SRC_MULTI, SRC_LINE>(src, [&](auto S) {
        return with_value<SEL_NONE, SEL_MASK, SEL_IDS>(sel, [&](auto E) {
          return with_flags([&](auto W, auto L, auto V, auto F) {
            if constexpr (S() == SRC_COLS) return go(k_density<SRC_COLS, E(), W(), L(), V() && E() != SEL_IDS, false>);
            else return go(k_density<S(), E(), W(), L(), false, F()>);
          }, weighted, in_lds, vec, f32);
        });
      });
      if (rc) return rc;
    }
    return GM_OK;
  };
  // a gated call enqueues the LDS passes, then the device-atomic form: one of the two runs
  const int rc = run(lds);
  return rc || !gated ? rc : run(false);
}

inline bool dens_bound_ok(double v) { return std::isfinite(v) && std::fabs(v) <= 2147483648.0; }

// every GM_E_INVALID of the density entries that does not depend on the source
int density_check(const char* who, gm_ctx* ctx, int64_t n, const void* weight, const uint64_t* mask, const int64_t* ids,
                  int64_t n_ids, const gm_density_grid* g, const double* grid, const int64_t* tally) {
  auto fail = [&](const char* why) {
    set_error(std::string(who) + ": " + why);
    return (int)GM_E_INVALID;
  };
  if (!ctx) return fail("NULL context");
  if (!g) return fail("NULL grid description");
  if (!grid || !tally) return fail("NULL grid or tally output");
  if (n < 0) return fail("negative row count");
  if (g->width < 1 || g->height < 1) return fail("width and height must be at least 1");
  if ((int64_t)g->width * g->height > 2147483647LL) return fail("width * height exceeds 2^31 - 1");
  if (!dens_bound_ok(g->xmin) || !dens_bound_ok(g->xmax) || !dens_bound_ok(g->ymin) || !dens_bound_ok(g->ymax))
    return fail("envelope bounds must be finite and within 2^31 in magnitude");
  if (!(g->xmax > g->xmin) || !(g->ymax > g->ymin)) return fail("flat or inverted envelope");
  if (g->xmax - g->xmin > 360.0 * 64) return fail("envelope wider than 64 turns");
  if (const char* why = sel_check(mask, ids, n_ids)) return fail(why);
  if (g->path < 0 || g->path > 2) return fail("path must be 0, 1 or 2");
  if (g->path == 1 && dens_passes(g, weight != nullptr) > DENS_MAX_PASSES)
    return fail("path 1: the grid does not fit workgroup-private counters");
  if (g->workgroups < 0) return fail("negative workgroups");
  if (!aligned_to<8>(weight) || !aligned_to<8>(grid) || !aligned_to<8>(tally))
    return fail("columns and outputs need 8-B alignment");
  return GM_OK;
}

// ------------------------------------------------------------------ dense grid -> sparse cells
// Cells in the order encodeResult groups them by (DensityScan.scala:95-106): column i, then row j.
// Block b owns cells k = i * height + j of [b * SP_CELLS, +SP_CELLS), SP_PER consecutive ones per thread.
constexpr int SP_PER = 16;
constexpr int SP_CELLS = SCAN_TPB * SP_PER;

template <bool WRITE>
__global__ __launch_bounds__(SCAN_TPB) void k_density_sparse(const double* __restrict__ grid, int width, int height,
                                                             int32_t* __restrict__ counts,
                                                             const int64_t* __restrict__ offsets, int64_t cap,
                                                             int32_t* __restrict__ oi, int32_t* __restrict__ oj,
                                                             double* __restrict__ ow) {
  const int64_t cells = (int64_t)width * height;
  const int64_t k0 = (int64_t)blockIdx.x * SP_CELLS + (int64_t)threadIdx.x * SP_PER;
  double v[SP_PER];
  int64_t c = 0;
#pragma unroll
  for (int u = 0; u < SP_PER; ++u) {
    const int64_t k = k0 + u;
    v[u] = k < cells ? grid[(k % height) * width + k / height] : 0.0;
    c += v[u] != 0.0;
  }
  int64_t tot;
  int64_t at = block_excl_scan(c, &tot);
  if (!WRITE) {
    if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)tot;
    return;
  }
  at += offsets[blockIdx.x];
#pragma unroll
  for (int u = 0; u < SP_PER; ++u) {
    if (v[u] != 0.0) {
      if (at < cap) {
        const int64_t k = k0 + u;
        oi[at] = (int32_t)(k / height);
        oj[at] = (int32_t)(k % height);
        ow[at] = v[u];
      }
      ++at;
    }
  }
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_density_points(gm_ctx* ctx, const double* x, const double* y, const double* weight, int64_t n,
                      const uint64_t* mask, const int64_t* ids, int64_t n_ids, const gm_density_grid* g,
                      double* grid, int64_t* tally) {
  const int rc = density_check("gm_density_points", ctx, n, weight, mask, ids, n_ids, g, grid, tally);
  if (rc) return rc;
  if (n == 0 && !ids) return GM_OK;
  if (n > 0 && (!x || !y || !aligned_to<8>(x) || !aligned_to<8>(y))) {
    set_error("gm_density_points: x and y must be given, 8-B aligned");
    return GM_E_INVALID;
  }
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  DensSrc s{x, y, weight, ArrowPts{nullptr, nullptr, 0, 0, 0}, nullptr};
  return launch_density(ctx, SRC_COLS, false, s, row_sel(n, mask, ids, n_ids), g, grid, tally);
}

int gm_density_arrow(gm_ctx* ctx, const gm_geom_column* geom, const double* weight, int64_t n, const uint64_t* mask,
                     const int64_t* ids, int64_t n_ids, const gm_density_grid* g, double* grid, int64_t* tally) {
  const int rc = density_check("gm_density_arrow", ctx, n, weight, mask, ids, n_ids, g, grid, tally);
  if (rc) return rc;
  if (rejects_wkb(geom, "gm_density_arrow", true)) return GM_E_INVALID;
  if (n == 0 && !ids) return GM_OK;
  if (n > 0 && (!geom_col_ok(geom) || (geom->type != GM_GEOM_POINT && geom->type != GM_GEOM_MULTIPOINT))) {
    set_error("gm_density_arrow: geom must be a GM_GEOM_POINT or GM_GEOM_MULTIPOINT column of 64- or 32-bit ordinates");
    return GM_E_INVALID;
  }
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  DensSrc s{nullptr, nullptr, weight, ArrowPts{nullptr, nullptr, 0, 0, 0}, nullptr};
  int src = SRC_POINT;
  bool f32 = false;
  if (n > 0) {
    s.pts = ArrowPts{geom->coords, geom->validity, geom->validity_offset, geom->flip_axis, geom->ordinal_bits == 32};
    s.o0 = geom->offsets[0];
    src = geom->type == GM_GEOM_POINT ? SRC_POINT : SRC_MULTI;
    f32 = geom->ordinal_bits == 32;
  }
  return launch_density(ctx, src, f32, s, row_sel(n, mask, ids, n_ids), g, grid, tally);
}

int gm_density_lines(gm_ctx* ctx, const gm_geom_column* geom, const double* weight, int64_t n, const uint64_t* mask,
                     const int64_t* ids, int64_t n_ids, const gm_density_grid* g, double* grid, int64_t* tally) {
  const int rc = density_check("gm_density_lines", ctx, n, weight, mask, ids, n_ids, g, grid, tally);
  if (rc) return rc;
  if (rejects_wkb(geom, "gm_density_lines", false)) return GM_E_INVALID;
  if (n == 0 && !ids) return GM_OK;
  if (n > 0 && (!geom_col_ok(geom) || (geom->type != GM_GEOM_LINESTRING && geom->type != GM_GEOM_MULTILINESTRING))) {
    set_error("gm_density_lines: geom must be a GM_GEOM_LINESTRING or GM_GEOM_MULTILINESTRING column of 64- or 32-bit "
              "ordinates");
    return GM_E_INVALID;
  }
  if (ids && n_ids == 0) return GM_OK;
  GM_HIP(hipSetDevice(ctx->device));
  DensSrc s{nullptr, nullptr, weight, ArrowPts{nullptr, nullptr, 0, 0, 0}, nullptr, nullptr, nullptr, 0};
  bool f32 = false;
  int64_t parts = 0;
  if (n > 0) {
    s.pts = ArrowPts{geom->coords, geom->validity, geom->validity_offset, geom->flip_axis, geom->ordinal_bits == 32};
    s.o0 = geom->offsets[0];
    s.o1 = geom->offsets[1];
    s.multi = geom->type == GM_GEOM_MULTILINESTRING;
    f32 = geom->ordinal_bits == 32;
    parts = n;
    if (s.multi) {   // the column's part count is its last slot offset, on the device: the one wait of the call
      int32_t* last = (int32_t*)ctx->h_pinned;
      GM_HIP(hipMemcpyAsync(last, s.o0 + n, 4, hipMemcpyDeviceToHost, ctx->stream));
      GM_HIP(hipStreamSynchronize(ctx->stream));
      parts = *last;
      if (parts < 0) {
        set_error("gm_density_lines: negative slot offset");
        return GM_E_INVALID;
      }
    }
  }
  return launch_density(ctx, SRC_LINE, f32, s, row_sel(n, mask, ids, n_ids), g, grid, tally, parts);
}

int gm_density_sparse(gm_ctx* ctx, const double* grid, int32_t width, int32_t height, int64_t cap, int32_t* i,
                      int32_t* j, double* w, int64_t* n_cells) {
  if (!ctx || !grid || !n_cells || width < 1 || height < 1 || (int64_t)width * height > 2147483647LL || cap < 0 ||
      (cap > 0 && (!i || !j || !w))) {
    set_error("gm_density_sparse: NULL argument, bad grid size or negative capacity");
    return GM_E_INVALID;
  }
  GM_HIP(hipSetDevice(ctx->device));
  const int64_t cells = (int64_t)width * height, nb = (cells + SP_CELLS - 1) / SP_CELLS;
  DevTemps tmp(ctx->stream);
  CountScan cs;
  int rc = cs.alloc(tmp, nb);
  if (rc) return rc;
  hipLaunchKernelGGL(k_density_sparse<false>, dim3((unsigned)nb), dim3(SCAN_TPB), 0, ctx->stream, grid, width, height,
                     cs.counts, (const int64_t*)nullptr, cap, i, j, w);
  GM_CHECK_LAUNCH();
  if ((rc = cs.scan(ctx))) return rc;
  if (cap > 0) {   // the cells, before the count is waited for: one wait covers both
    hipLaunchKernelGGL(k_density_sparse<true>, dim3((unsigned)nb), dim3(SCAN_TPB), 0, ctx->stream, grid, width, height,
                       cs.counts, (const int64_t*)cs.offsets, cap, i, j, w);
    GM_CHECK_LAUNCH();
  }
  if ((rc = cs.total(ctx, n_cells))) return rc;
  return *n_cells > cap ? GM_E_CAPACITY : GM_OK;
}

}  // extern "C"
