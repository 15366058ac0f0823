// gm_geom_filter.hip -- the XZ tables' full filter on the feature GEOMETRY: geometry meets query box (k_refine
// with BoxPred and its visitor MeetsBox, below) and geometry meets query polygons (k_poly_refine, further
// down, with its own notes).  In k_refine the kernel owns the survivors, a predicate owns the query, and a
// visitor of the slot's walk (arrow_walk, gm_arrow.hpp; wkb_walk, gm_wkb.hpp) owns the decision per point,
// line and ring, over typed and WKB columns alike.
//
// The XZ key spaces always apply the full filter (XZ2IndexKeySpace.scala:122-125,
// XZ3IndexKeySpace.scala:247-250); for bbox(geom, ...) it is GeoTools BBOXImpl on the feature's geometry
// (GeometryProcessing.scala:104-136), i.e. JTS Geometry.intersects against the query rectangle.  The
// contract here is the closed-set one: slot G matches box B iff G and B share a point.  JTS 1.20
// RectangleIntersects gets there by an envelope check, GeometryContainsPointVisitor over the
// rectangle's corners and RectangleLineIntersector per segment; so does the box predicate:
//   * the envelope test is the mask pass of the scan (k_range_mask, gm_filter.hip); its survivors come
//     here as compacted candidate indices, one 64-lane wave per survivor;
//   * lanes stride over the slot's segments (segments_any: consecutive tuples, one contiguous run per wave
//     step, each tuple loaded once, a segment's second end taken from the next lane).
//     RectangleLineIntersector: segment envelope, an endpoint in the box, else the segment ordered by
//     (x, y) against the diagonal of opposite slope, decided by four orientation signs
//     (RobustLineIntersector; jts_orientation, gm_device.hpp) -- reached only when both endpoints are
//     outside and the envelopes overlap;
//   * a polygon also matches when the box lies inside it.  When no ring segment meets the box the box
//     touches no ring, so its four corners have one location and the corner (xmin, ymin) stands for all
//     of them: the same pass over a ring counts that corner's crossings (RayCrossingCounter.countSegment,
//     gm_pip.hpp), a ballot gives the ring's parity, and SimplePointInAreaLocator's rule decides
//     (inside the shell and inside no hole; not Mod-2 over the rings);
//   * a survivor that meets no box clears its bit of the candidate mask; k_mask_recount then takes the
//     per-block counts again and the scan's compaction runs as after pass A.
// Two shortcuts follow from the definition and skip the walk: a slot envelope inside the box, and a
// LineString / Polygon (one connected component reaching all four sides of its envelope) whose x- or
// y-range lies within the box's.  Neither holds for the union envelope of a multi geometry.
#include <algorithm>

#include "gm_arrow.hpp"
#include "gm_pip.hpp"
#include "gm_scan.hpp"
#include "gm_wkb.hpp"

namespace gm {

constexpr int GTPB = 256;   // 4 waves per block, one survivor per wave

struct Box {
  double x0, y0, x1, y1;
};

__device__ __forceinline__ bool pt_in_box(double x, double y, const Box& q) {
  return x >= q.x0 && x <= q.x1 && y >= q.y0 && y <= q.y1;
}

// Envelope.intersects(p1, p2, q): q in the envelope of the segment p1-p2
__device__ __forceinline__ bool pt_in_seg_env(double ax, double ay, double bx, double by, double qx, double qy) {
  return qx >= (ax < bx ? ax : bx) && qx <= (ax > bx ? ax : bx) && qy >= (ay < by ? ay : by) &&
         qy <= (ay > by ? ay : by);
}

// RobustLineIntersector.computeIntersect(p1, p2, q1, q2).hasIntersection() past its envelope test
__device__ __forceinline__ bool segs_cross(double ax, double ay, double bx, double by, double cx, double cy,
                                           double dx, double dy) {
  const int pq1 = jts_orientation(ax, ay, bx, by, cx, cy);
  const int pq2 = jts_orientation(ax, ay, bx, by, dx, dy);
  if ((pq1 > 0 && pq2 > 0) || (pq1 < 0 && pq2 < 0)) return false;
  const int qp1 = jts_orientation(cx, cy, dx, dy, ax, ay);
  const int qp2 = jts_orientation(cx, cy, dx, dy, bx, by);
  if ((qp1 > 0 && qp2 > 0) || (qp1 < 0 && qp2 < 0)) return false;
  if ((pq1 | pq2 | qp1 | qp2) == 0)   // computeCollinearIntersection
    return pt_in_seg_env(ax, ay, bx, by, cx, cy) || pt_in_seg_env(ax, ay, bx, by, dx, dy) ||
           pt_in_seg_env(cx, cy, dx, dy, ax, ay) || pt_in_seg_env(cx, cy, dx, dy, bx, by);
  return true;
}

__device__ __forceinline__ bool seg_meets_seg(double ax, double ay, double bx, double by, double cx, double cy,
                                              double dx, double dy) {
  if ((ax < bx ? ax : bx) > (cx > dx ? cx : dx) || (ax > bx ? ax : bx) < (cx < dx ? cx : dx) ||
      (ay < by ? ay : by) > (cy > dy ? cy : dy) || (ay > by ? ay : by) < (cy < dy ? cy : dy))
    return false;
  return segs_cross(ax, ay, bx, by, cx, cy, dx, dy);
}

// RectangleLineIntersector.intersects(p0, p1) for a non-null box: its two cheap tests, then the segment
// against a diagonal, whose envelope is the box (so seg_meets_seg's envelope test is the first one here)
__device__ __forceinline__ bool seg_meets_box(double ax, double ay, double bx, double by, const Box& q) {
  const double sx0 = ax < bx ? ax : bx, sx1 = ax > bx ? ax : bx;
  const double sy0 = ay < by ? ay : by, sy1 = ay > by ? ay : by;
  if (q.x0 > sx1 || q.x1 < sx0 || q.y0 > sy1 || q.y1 < sy0) return false;
  if (pt_in_box(ax, ay, q) || pt_in_box(bx, by, q)) return true;
  // Coordinate.compareTo order, then the diagonal of opposite slope
  if (ax > bx || (ax == bx && ay > by)) {
    double t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const bool up = by > ay;
  return segs_cross(ax, ay, bx, by, q.x0, up ? q.y1 : q.y0, q.x1, up ? q.y0 : q.y1);
}

__device__ __forceinline__ double uniform(double v) {   // v, the same in every lane, as a scalar
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), lo);
}

// the tuples [0, n) as points, spread over the lanes: f(x, y) of some point
template <class SRC, class F>
__device__ __forceinline__ bool points_any(const SRC& t, int32_t n, int lane, const F& f) {
  for (int32_t j0 = 0; j0 < n; j0 += 64) {
    const int32_t j = j0 + lane;
    bool h = false;
    if (j < n) {
      double x, y;
      t.tuple(j, x, y);
      h = f(x, y);
    }
    if (__any(h)) return true;
  }
  return false;
}

// the tuples [0, n) as a line or a ring: f(ax, ay, bx, by) of some segment (j, j + 1), 0 <= j < n - 1.  A
// wave step reads one contiguous run of 64 tuples, one per lane, and takes each segment's second end from
// the next lane, so a step covers 63 segments and no tuple is loaded twice within it.  f keeps what a ring's
// pass counts (crossings) in its own state, one count per lane
template <class SRC, class F>
__device__ __forceinline__ bool segments_any(const SRC& t, int32_t n, int lane, F& f) {
  for (int32_t j0 = 0; j0 < n - 1; j0 += 63) {
    const int32_t left = n - j0;   // wave-uniform: the lanes compare against it, the index stays base + lane
    double ax = 0.0, ay = 0.0;
    if (lane < left) t.tuple(j0 + lane, ax, ay);
    const double bx = __shfl_down(ax, 1, 64), by = __shfl_down(ay, 1, 64);
    bool h = false;
    if (lane < 63 && lane < left - 1) h = f(ax, ay, bx, by);
    if (__any(h)) return true;
  }
  return false;
}

// a segment against the box; RING also counts the crossings of the corner (q.x0, q.y0) (on a segment: a hit)
template <bool RING>
struct BoxSeg {
  const Box& q;
  int cross;
  __device__ __forceinline__ bool operator()(double ax, double ay, double bx, double by) {
    bool h = seg_meets_box(ax, ay, bx, by, q);
    if (RING && !h) h = count_segment(ax, ay, bx, by, q.x0, q.y0, cross);
    return h;
  }
};

// A slot against the box, the whole wave on it (UNI walks): a collection by any of its elements; the walk
// stops at the first hit
struct MeetsBox {
  Box q;
  int lane;
  bool in_shell, in_hole;
  template <class T>
  __device__ __forceinline__ bool point(const T& t) {
    double x, y;
    t.tuple(0, x, y);
    return pt_in_box(x, y, q);
  }
  template <class T>
  __device__ __forceinline__ bool points(const T& t, int32_t n) {
    const auto in = [&](double x, double y) __attribute__((always_inline)) { return pt_in_box(x, y, q); };
    return points_any(t, n, lane, in);
  }
  // A WKB LineString of one tuple is that point.  A typed one has no segment and meets nothing here; alone
  // in its slot it matches all the same, by the envelope shortcut (its envelope is the point)
  template <class T>
  __device__ __forceinline__ bool line(const T& t, int32_t n) {
    if (T::WKB && n == 1) return point(t);
    BoxSeg<false> f{q, 0};
    return segments_any(t, n, lane, f);
  }
  __device__ __forceinline__ void polygon_begin() { in_shell = in_hole = false; }
  template <class T>
  __device__ __forceinline__ bool ring(uint32_t r, const T& t, int32_t n) {
    BoxSeg<true> f{q, 0};
    if (segments_any(t, n, lane, f)) return true;
    const bool in = __popcll(__ballot(f.cross & 1)) & 1;
    if (r == 0) in_shell = in; else in_hole |= in;
    return false;
  }
  // no ring segment met the box: its corner inside the shell and inside no hole
  // (SimplePointInAreaLocator.locatePointInPolygon)
  __device__ __forceinline__ bool polygon_end() { return in_shell && !in_hole; }
};

// The box filter as k_refine's predicate: the box loop and the two envelope shortcuts
struct BoxPred {
  const double* boxes;   // nbox x (xmin, ymin, xmax, ymax)
  int nbox;
  template <bool F32, bool WKB>
  __device__ __forceinline__ bool meets(const ArrowGeom& g, int64_t r, double ex0, double ey0, double ex1, double ey1,
                                        int lane, uint32_t* rem) const {
    // one connected component: by the column's type, and for WKB by the slot's own top-level code (a
    // malformed slot never matches; its envelope column holds the null envelope besides)
    bool connected = g.type == GM_GEOM_LINESTRING || g.type == GM_GEOM_POLYGON;
    if (WKB) {
      WkbCur top = wkb_slot(g, r);
      WkbHead h;
      if (!wkb_head<true>(top, h)) return false;
      connected = h.code == WKB_LINESTRING || h.code == WKB_POLYGON;
    }
    bool hit = false;
    for (int k = 0; k < nbox && !hit; ++k) {
      const double* b = boxes + 4 * k;
      if (!env_intersects(ex0, ey0, ex1, ey1, b)) continue;
      // in scalar registers: as vector ones the box is what takes the typed kernel past 80 VGPRs (6 waves)
      const Box q{uniform(b[0]), uniform(b[1]), uniform(b[2]), uniform(b[3])};
      const bool xin = ex0 >= q.x0 && ex1 <= q.x1, yin = ey0 >= q.y0 && ey1 <= q.y1;
      hit = (xin && yin) || (connected && (xin || yin));
      if (hit) continue;
      MeetsBox v{q, lane, false, false};
      hit = geom_walk<true, F32, WKB>(g, r, rem, GTPB / 64, v) == WKB_STOP;
    }
    return hit;
  }
};

// ------------------------------------------------------------------ geometry meets query polygons
// NOT merged into k_refine and the shared walk: as a predicate with a visitor under arrow_walk / wkb_walk and
// run_meets_a over segments_any it gave the same ids with 112-114 VGPRs for 105-107 and took 3.5% longer where
// it dominates ("Geometry walks and visitors").  Its kernel, typed switch and WKB visitor stay; the
// price is a second tuple source for a typed column (ArrowColumn) and a second scalar offset read (uoff).
//
// k_poly_refine: INTERSECTS(geom, polygons), the contract of geomesa_hip.h.  Still one wave per envelope
// survivor.  The query (PolyQuery, gm_scan.hpp) is its ring edges bucketed by y-slab; while the entries fit
// PQ_LDS_ENTRIES they are staged in LDS once per workgroup, else read from global memory (L2).  Per tuple
// run of G (a line, or a ring) the pair space is G's segments x the query's entries, in one of two shapes:
//   * run_meets_a, more than 64 tuples: lanes stride over G's segments (segments_any's read pattern) and each
//     lane loops the entries of the slabs its own segment's y-range overlaps;
//   * run_meets_b, fewer segments than a wave: the run sits in registers, one tuple per lane; lanes stride
//     over the entries of the slabs the SLOT's y-range overlaps (one contiguous run) and loop G's
//     segments, each taken from its lanes by readlane.
// A ring's pass also counts, for up to PQ_GROUP parts at once, the crossings of the part's first shell
// vertex (RayCrossingCounter.countSegment) -- "Q's part inside G" -- as the box kernel counts its corner's.
// Parts past the first PQ_GROUP take further passes over the rings, contact off, and only after contact
// failed.  Without contact a line, or a polygon's shell, lies wholly inside or outside each part, and its
// first tuple decides (pq_locate: the tuple's one slab, ring by ring, parts by the shell / hole rule).
constexpr int PQ_LDS_ENTRIES = 2040;   // just under 64 KiB of entries per workgroup (the WKB stack follows them)
constexpr int PQ_GROUP = 4;
constexpr int PQ_MAX_BLOCKS = 1024;    // a staging workgroup strides over the survivors: 4 per CU

extern __shared__ __attribute__((aligned(16))) char pq_smem[];

// a List offset every lane of the wave reads alike, as a scalar
__device__ __forceinline__ int32_t uoff(const int32_t* o, int64_t i) { return __builtin_amdgcn_readfirstlane(o[i]); }

// the whole typed column as a tuple source, indexed from its tuple 0 (ArrowTuples carries a run's base)
template <bool F32>
struct ArrowColumn {
  const void* c;
  int flip;
  __device__ __forceinline__ void tuple(int64_t j, double& x, double& y) const { arrow_tuple<F32>(c, j, flip, x, y); }
};

template <bool LDS>
struct QEdges {
  const double* g;
  __device__ __forceinline__ void get(int32_t e, double& ax, double& ay, double& bx, double& by) const {
    const dv2* s = (LDS ? (const dv2*)pq_smem : (const dv2*)g) + 2 * (int64_t)e;
    const dv2 a = s[0], b = s[1];
    ax = a.x; ay = a.y; bx = b.x; by = b.y;
  }
};

__device__ __forceinline__ int pq_slab(double y, const PolyQuery& q) {   // polyq::slab_of
  const double c = floor(__dmul_rn(__dsub_rn(y, q.y0), q.inv_h));
  return (int)__builtin_fmin(__builtin_fmax(c, 0.0), (double)(q.ns - 1));
}

// one survivor's view of the query: the slot's envelope, the entries of the slabs it overlaps, and the
// group of parts whose first shell vertex this walk counts (act: those inside the slot's envelope)
template <bool LDS>
struct PolyCtx {
  PolyQuery q;
  QEdges<LDS> ed;
  int lane;
  int32_t be0, be1;
  bool contact;            // this walk tests contact and locates first tuples (the first group's)
  int p0;                  // the group's first part
  uint32_t act;
  double vx[PQ_GROUP], vy[PQ_GROUP];
};

// the point is not exterior to some part.  Every lane for itself: the entries of the point's slab in
// order, a ring's crossings closed when the ring changes and a part's rule when the part does
template <bool LDS>
__device__ __forceinline__ bool pq_locate(const PolyCtx<LDS>& c, double px, double py) {
  const PolyQuery& q = c.q;
  if (!(px >= q.x0 && px <= q.x1 && py >= q.y0 && py <= q.y1)) return false;
  const int s = pq_slab(py, q);
  const int32_t e1 = q.soff[s + 1];
  bool hit = false, shell_ok = false, hole_in = false, shell = false, on = false;
  int32_t cur_r = -1, cur_p = -1;
  int cr = 0;
  for (int32_t e = q.soff[s]; e < e1; ++e) {
    const int32_t r = q.ering[e], pw = q.epart[e];
    if (r != cur_r) {
      if (cur_r >= 0) {
        if (shell) shell_ok = on || (cr & 1); else hole_in |= !on && (cr & 1);
      }
      if ((pw >> 1) != cur_p) {
        hit |= shell_ok && !hole_in;
        cur_p = pw >> 1;
        shell_ok = hole_in = false;
      }
      cur_r = r;
      shell = pw & 1;
      cr = 0;
      on = false;
    }
    if (!on) {
      double ax, ay, bx, by;
      c.ed.get(e, ax, ay, bx, by);
      on = count_segment(ax, ay, bx, by, px, py, cr);
    }
  }
  if (cur_r >= 0) {
    if (shell) shell_ok = on || (cr & 1); else hole_in |= !on && (cr & 1);
  }
  return hit || (shell_ok && !hole_in);
}

// a lane's segment against the entries of the slabs its y-range overlaps
template <bool LDS>
__device__ __forceinline__ bool seg_meets_query(const PolyCtx<LDS>& c, double ax, double ay, double bx, double by) {
  const PolyQuery& q = c.q;
  const double sy0 = ay < by ? ay : by, sy1 = ay > by ? ay : by;
  if (sy1 < q.y0 || sy0 > q.y1 || (ax > bx ? ax : bx) < q.x0 || (ax < bx ? ax : bx) > q.x1) return false;
  const int32_t e1 = q.soff[pq_slab(sy1, q) + 1];
  for (int32_t e = q.soff[pq_slab(sy0, q)]; e < e1; ++e) {
    double cx, cy, dx, dy;
    c.ed.get(e, cx, cy, dx, dy);
    if (seg_meets_seg(ax, ay, bx, by, cx, cy, dx, dy)) return true;
  }
  return false;
}

// the first-vertex crossings of the group's active parts over one segment of a ring of G; true: on it
template <bool LDS>
__device__ __forceinline__ bool count_group(const PolyCtx<LDS>& c, double ax, double ay, double bx, double by,
                                            int (&cross)[PQ_GROUP]) {
  bool on = false;
#pragma unroll
  for (int k = 0; k < PQ_GROUP; ++k)
    if ((c.act >> k) & 1u) on |= count_segment(ax, ay, bx, by, c.vx[k], c.vy[k], cross[k]);
  return on;
}

// the tuples [a, b), b - a >= 2, as a line or a ring: some segment meets a query edge (when c.contact); a
// RING also gives the parities of the group's crossings in par (true as well when a first vertex is on it)
template <bool RING, bool LDS, class SRC>
__device__ __forceinline__ bool run_meets_a(const SRC& g, int32_t a, int32_t b, const PolyCtx<LDS>& c, uint32_t& par) {
  int cross[PQ_GROUP] = {0, 0, 0, 0};
  for (int32_t j0 = a; j0 < b - 1; j0 += 63) {
    const int32_t j = j0 + c.lane;
    double ax = 0.0, ay = 0.0;
    if (j < b) g.tuple(j, ax, ay);
    const double bx = __shfl_down(ax, 1, 64), by = __shfl_down(ay, 1, 64);
    bool h = false;
    if (c.lane < 63 && j < b - 1) {
      if (c.contact) h = seg_meets_query(c, ax, ay, bx, by);
      if (RING && !h) h = count_group(c, ax, ay, bx, by, cross);
    }
    if (__any(h)) return true;
  }
  par = 0;
  if (RING) {
#pragma unroll
    for (int k = 0; k < PQ_GROUP; ++k) par |= (uint32_t)(__popcll(__ballot(cross[k] & 1)) & 1) << k;
  }
  return false;
}

__device__ __forceinline__ double lane_of(double v, int k) {   // v of lane k, k wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

// the same for 2 <= b - a <= 64: the run in registers, lanes over the query's entries.  Lane k < PQ_GROUP
// counts part k's first vertex, once, in the first step over the entries
template <bool RING, bool LDS, class SRC>
__device__ __forceinline__ bool run_meets_b(const SRC& g, int32_t a, int32_t b, const PolyCtx<LDS>& c, uint32_t& par) {
  double tx = 0.0, ty = 0.0;
  if (a + c.lane < b) g.tuple(a + c.lane, tx, ty);
  const int nseg = b - a - 1;
  const bool counts = RING && c.lane < PQ_GROUP && ((c.act >> c.lane) & 1u);
  double vx = 0.0, vy = 0.0;
  if (counts) {   // an active part's: from memory, since a lane-indexed c.vx[] would put c into scratch
    vx = c.q.pv0[2 * (c.p0 + c.lane)];
    vy = c.q.pv0[2 * (c.p0 + c.lane) + 1];
  }
  int cross = 0;
  int32_t e0 = c.contact ? c.be0 : c.be1;
  bool first = true;
  do {
    const int32_t e = e0 + c.lane;
    const bool have = e < c.be1;
    double cx = 0.0, cy = 0.0, dx = 0.0, dy = 0.0;
    if (have) c.ed.get(e, cx, cy, dx, dy);
    bool h = false;
    for (int k = 0; k < nseg; ++k) {
      const double ax = lane_of(tx, k), ay = lane_of(ty, k), bx = lane_of(tx, k + 1), by = lane_of(ty, k + 1);
      if (have && !h) h = seg_meets_seg(ax, ay, bx, by, cx, cy, dx, dy);
      if (counts && first && !h) h = count_segment(ax, ay, bx, by, vx, vy, cross);
    }
    if (__any(h)) return true;
    first = false;
    e0 += 64;
  } while (e0 < c.be1);
  par = RING ? (uint32_t)__ballot(cross & 1) & ((1u << PQ_GROUP) - 1u) : 0u;
  return false;
}

template <bool RING, bool LDS, class SRC>
__device__ __forceinline__ bool run_meets(const SRC& g, int32_t a, int32_t b, const PolyCtx<LDS>& c, uint32_t& par) {
  return b - a <= 64 ? run_meets_b<RING>(g, a, b, c, par) : run_meets_a<RING>(g, a, b, c, par);
}

template <bool LDS, class SRC>
__device__ __forceinline__ bool first_tuple_in(const SRC& g, int64_t a, const PolyCtx<LDS>& c) {
  double x, y;
  g.tuple(a, x, y);
  return pq_locate(c, x, y);
}

// a line: contact, else its first tuple (one tuple: that point)
template <bool LDS, class SRC>
__device__ __forceinline__ bool line_meets_polys(const SRC& g, int32_t a, int32_t b, const PolyCtx<LDS>& c) {
  if (!c.contact || b <= a) return false;
  uint32_t unused;
  if (b - a >= 2 && run_meets<false>(g, a, b, c, unused)) return true;
  return first_tuple_in(g, a, c);
}

// one ring of a polygon of G: contact; the shell's first tuple; the group's parities into in_shell / in_hole
template <bool LDS, class SRC>
__device__ __forceinline__ bool ring_meets_polys(const SRC& g, int32_t a, int32_t b, bool is_shell, const PolyCtx<LDS>& c,
                                 uint32_t& in_shell, uint32_t& in_hole) {
  if (b <= a) return false;
  uint32_t par = 0;
  if (b - a >= 2 && (c.contact || c.act) && run_meets<true>(g, a, b, c, par)) return true;
  if (is_shell) in_shell = par; else in_hole |= par;
  return is_shell && c.contact && first_tuple_in(g, a, c);
}

template <bool LDS, class SRC>
__device__ __forceinline__ bool polygon_meets_polys(const SRC& g, const int32_t* __restrict__ ro, int32_t r0, int32_t r1,
                                    const PolyCtx<LDS>& c) {
  uint32_t in_shell = 0, in_hole = 0;
  for (int32_t r = r0; r < r1; ++r)
    if (ring_meets_polys(g, uoff(ro, r), uoff(ro, r + 1), r == r0, c, in_shell, in_hole)) return true;
  return (in_shell & ~in_hole & c.act) != 0;
}

template <bool LDS, class SRC>
__device__ __forceinline__ bool points_meet_polys(const SRC& g, int32_t a, int32_t b, const PolyCtx<LDS>& c) {
  if (!c.contact) return false;
  for (int32_t j0 = a; j0 < b; j0 += 64) {
    const int32_t j = j0 + c.lane;
    bool h = false;
    if (j < b) h = first_tuple_in(g, j, c);
    if (__any(h)) return true;
  }
  return false;
}

// slot i meets a part (wave-uniform), for the group of parts c holds
template <bool F32, bool LDS>
__device__ __forceinline__ bool geom_meets_polys(const ArrowGeom& g, int64_t i, const PolyCtx<LDS>& c) {
  const ArrowColumn<F32> ts{g.c, g.flip};
  switch (g.type) {
    case GM_GEOM_POINT:
      return c.contact && first_tuple_in(ts, i, c);
    case GM_GEOM_MULTIPOINT:
      return points_meet_polys(ts, uoff(g.o0, i), uoff(g.o0, i + 1), c);
    case GM_GEOM_LINESTRING:
      return line_meets_polys(ts, uoff(g.o0, i), uoff(g.o0, i + 1), c);
    case GM_GEOM_POLYGON:
      return polygon_meets_polys(ts, g.o1, uoff(g.o0, i), uoff(g.o0, i + 1), c);
    case GM_GEOM_MULTILINESTRING: {
      const int32_t l1 = uoff(g.o0, i + 1);
      for (int32_t l = uoff(g.o0, i); l < l1; ++l)
        if (line_meets_polys(ts, uoff(g.o1, l), uoff(g.o1, l + 1), c)) return true;
      return false;
    }
    default: {   // GM_GEOM_MULTIPOLYGON
      const int32_t p1 = uoff(g.o0, i + 1);
      for (int32_t p = uoff(g.o0, i); p < p1; ++p)
        if (polygon_meets_polys(ts, g.o2, uoff(g.o1, p), uoff(g.o1, p + 1), c)) return true;
      return false;
    }
  }
}

// the visitor of a WKB slot, beside WkbMeets: each class decided as geom_meets_polys decides it
template <bool LDS>
struct WkbMeetsPolys {
  const PolyCtx<LDS>& c;
  uint32_t in_shell, in_hole;
  __device__ __forceinline__ bool point(const WkbTuples& t) { return c.contact && first_tuple_in(t, 0, c); }
  __device__ __forceinline__ bool line(const WkbTuples& t, uint32_t n) { return line_meets_polys(t, 0, (int32_t)n, c); }
  __device__ __forceinline__ void polygon_begin() { in_shell = in_hole = 0; }
  __device__ __forceinline__ bool ring(uint32_t r, const WkbTuples& t, uint32_t n) {
    return ring_meets_polys(t, 0, (int32_t)n, r == 0, c, in_shell, in_hole);
  }
  __device__ __forceinline__ bool polygon_end() { return (in_shell & ~in_hole & c.act) != 0; }
};

template <bool F32, bool WKB, bool LDS>
__global__ __launch_bounds__(GTPB) void k_poly_refine(ArrowGeom g, GeomRefine a, PolyQuery q) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * (GTPB / 64);
  if (LDS) {
    for (int32_t i = threadIdx.x; i < 2 * q.entries; i += GTPB) ((dv2*)pq_smem)[i] = ((const dv2*)q.edge)[i];
    __syncthreads();
  }
  // wkb_walk's stack, one column per wave, behind the staged entries
  uint32_t* s_rem = (uint32_t*)(pq_smem + (LDS ? (size_t)q.entries * 32 : 0));
  const bool areal = WKB || g.type == GM_GEOM_POLYGON || g.type == GM_GEOM_MULTIPOLYGON;
  PolyCtx<LDS> c;
  c.q = q;
  c.ed = QEdges<LDS>{q.edge};
  c.lane = lane;
  for (int64_t s = (int64_t)blockIdx.x * (GTPB / 64) + wave; s < a.n_surv; s += nwaves) {
    const int64_t cand = a.surv[s];
    const int64_t row = cand_row(a.coff, a.start, a.nr, cand);
    const int64_t r = a.rows ? a.rows[row] : row;
    bool hit = false;
    if (arrow_valid(g.valid, g.voff, r)) {
      const double ex0 = a.xmin[r], ey0 = a.ymin[r], ex1 = a.xmax[r], ey1 = a.ymax[r];
      // a null envelope (an empty or malformed slot) overlaps no slab and holds no first vertex
      const bool any = ex1 >= ex0 && !(ey1 < q.y0 || ey0 > q.y1 || ex1 < q.x0 || ex0 > q.x1);
      c.be0 = any ? q.soff[pq_slab(ey0, q)] : 0;
      c.be1 = any ? q.soff[pq_slab(ey1, q) + 1] : 0;
      const int groups = any ? (areal ? (q.n_parts + PQ_GROUP - 1) / PQ_GROUP : 1) : 0;
      for (int gi = 0; gi < groups && !hit; ++gi) {
        c.contact = gi == 0;
        c.p0 = gi * PQ_GROUP;
        c.act = 0;
#pragma unroll
        for (int k = 0; k < PQ_GROUP; ++k) {
          const int p = gi * PQ_GROUP + k;
          c.vx[k] = c.vy[k] = 0.0;
          if (areal && p < q.n_parts) {
            c.vx[k] = q.pv0[2 * p];
            c.vy[k] = q.pv0[2 * p + 1];
            if (c.vx[k] >= ex0 && c.vx[k] <= ex1 && c.vy[k] >= ey0 && c.vy[k] <= ey1) c.act |= 1u << k;
          }
        }
        if (!c.contact && !c.act) continue;
        if (WKB) {
          WkbMeetsPolys<LDS> v{c, 0, 0};
          hit = wkb_walk<true>(wkb_slot(g, r), s_rem + wave, GTPB / 64, v) == WKB_STOP;
        } else {
          hit = geom_meets_polys<F32>(g, r, c);
        }
      }
    }
    if (!hit && lane == 0) atomicAnd((unsigned long long*)&a.mask[cand >> 6], ~(1ull << (cand & 63)));
  }
}

// ------------------------------------------------------------------ the kernels
// One wave per survivor: candidate -> table row -> column row, a null slot never matches, else the
// predicate P (BoxPred) decides on the slot and its envelope; a miss clears the candidate's bit.  WKB: the
// column is GM_GEOM_WKB (F32 false)
template <bool F32, bool WKB, class P>
__global__ __launch_bounds__(GTPB) void k_refine(ArrowGeom g, GeomRefine a, P p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * (GTPB / 64);
  __shared__ uint32_t s_rem[WKB ? WKB_DEPTH * (GTPB / 64) : 1];   // wkb_walk's stack, one column per wave
  uint32_t* rem = s_rem + wave;
  for (int64_t s = (int64_t)blockIdx.x * (GTPB / 64) + wave; s < a.n_surv; s += nwaves) {
    const int64_t c = a.surv[s];
    const int64_t row = cand_row(a.coff, a.start, a.nr, c);
    const int64_t r = a.rows ? a.rows[row] : row;
    const bool hit = arrow_valid(g.valid, g.voff, r) &&
                     p.template meets<F32, WKB>(g, r, a.xmin[r], a.ymin[r], a.xmax[r], a.ymax[r], lane, rem);
    if (!hit && lane == 0) atomicAnd((unsigned long long*)&a.mask[c >> 6], ~(1ull << (c & 63)));
  }
}

// per-block match counts of a candidate mask (the block_counts of pass A), one wave per block
__global__ __launch_bounds__(64) void k_mask_recount(const uint64_t* __restrict__ mask, int64_t total,
                                                     int32_t* __restrict__ counts) {
  int c = 0;
  for (int w = threadIdx.x; w < FROWS / 64; w += 64) {
    const int64_t word = (int64_t)blockIdx.x * (FROWS / 64) + w;
    if ((word << 6) < total) c += __popcll(mask[word]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// Geometry.getEnvelopeInternal of every slot, one lane per slot; a null slot, and a malformed WKB one,
// reads as the null envelope
template <bool F32, bool WKB>
__global__ __launch_bounds__(GTPB) void k_envelopes(ArrowGeom g, int64_t n, double* __restrict__ xmin,
                                                    double* __restrict__ ymin, double* __restrict__ xmax,
                                                    double* __restrict__ ymax) {
  __shared__ uint32_t s_rem[WKB ? WKB_DEPTH * GTPB : 1];   // wkb_walk's stack, one column per lane
  for (int64_t i = (int64_t)blockIdx.x * GTPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GTPB) {
    Env e = env_null();
    if (arrow_valid(g.valid, g.voff, i)) slot_envelope<F32, WKB>(g, i, s_rem + threadIdx.x, GTPB, e);
    xmin[i] = e.minx;
    ymin[i] = e.miny;
    xmax[i] = e.maxx;
    ymax[i] = e.maxy;
  }
}

static ArrowGeom to_geom(const gm_geom_column* c) {
  return ArrowGeom{c->coords, c->validity, c->validity_offset, c->offsets[0], c->offsets[1], c->offsets[2], c->type,
                   c->flip_axis};
}

// f(F32, WKB) as template flags; a WKB column holds doubles
template <class F>
static void with_column_form(const gm_geom_column* geom, F&& f) {
  const bool wkb = geom->type == GM_GEOM_WKB;
  with_flags([&](auto F32, auto WKB) {
    if constexpr (!(F32() && WKB())) f(F32, WKB);
  }, geom->ordinal_bits == 32 && !wkb, wkb);
}

int geom_refine(gm_ctx* ctx, const gm_geom_column* geom, const GeomRefine& a, const PolyQuery* q) {
  const ArrowGeom g = to_geom(geom);
  const bool lds = q && q->entries <= PQ_LDS_ENTRIES;
  const int64_t blocks = std::min<int64_t>((a.n_surv + GTPB / 64 - 1) / (GTPB / 64), lds ? PQ_MAX_BLOCKS : 1 << 20);
  // the polygon kernel's dynamic LDS: the staged entries, then the WKB stack (the box kernel's is static)
  const size_t smem = !q ? 0 : (lds ? (size_t)q->entries * 32 : 0) +
                                   (geom->type == GM_GEOM_WKB ? WKB_DEPTH * (GTPB / 64) * sizeof(uint32_t) : 0);
  with_column_form(geom, [&](auto F32, auto WKB) {
    if (!q) {
      hipLaunchKernelGGL((k_refine<decltype(F32)::value, decltype(WKB)::value, BoxPred>), dim3((unsigned)blocks),
                         dim3(GTPB), 0, ctx->stream, g, a, BoxPred{a.boxes, a.nbox});
    } else {
      with_flags([&](auto LDS) {
        hipLaunchKernelGGL((k_poly_refine<decltype(F32)::value, decltype(WKB)::value, decltype(LDS)::value>),
                           dim3((unsigned)blocks), dim3(GTPB), smem, ctx->stream, g, a, *q);
      }, lds);
    }
  });
  GM_CHECK_LAUNCH();
  const int64_t nblocks = (a.total + FROWS - 1) / FROWS;
  hipLaunchKernelGGL(k_mask_recount, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, a.mask, a.total, a.counts);
  GM_CHECK_LAUNCH();
  return GM_OK;
}

int upload_polys(gm_ctx* ctx, DevTemps& tmp, const polyq::HostQuery& h, PolyQuery& q) {
  // [entries x 4 f64][parts x 2 f64][slab offsets][entry rings][entry parts]
  const size_t nb = (size_t)h.entries(), np = (size_t)h.n_parts, no = h.soff.size();
  std::vector<double> buf(nb * 4 + np * 2 + (no + 2 * nb + 1) / 2);
  int32_t* words = (int32_t*)(buf.data() + nb * 4 + np * 2);
  std::copy(h.edge.begin(), h.edge.end(), buf.begin());
  std::copy(h.pv0.begin(), h.pv0.end(), buf.begin() + nb * 4);
  std::copy(h.soff.begin(), h.soff.end(), words);
  std::copy(h.ering.begin(), h.ering.end(), words + no);
  std::copy(h.epart.begin(), h.epart.end(), words + no + nb);
  double* d = nullptr;
  int rc = tmp.alloc_async(buf.size() * 8, &d);
  if (!rc) rc = copy_h2d(ctx, d, buf.data(), buf.size() * 8);
  if (rc) return rc;
  const int32_t* dw = (const int32_t*)(d + nb * 4 + np * 2);
  q = PolyQuery{d, dw + no, dw + no + nb, dw, d + nb * 4, h.n_parts, h.ns, (int32_t)nb, h.x0, h.y0, h.x1, h.y1, h.inv_h};
  return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_arrow_envelopes(gm_ctx* ctx, const gm_geom_column* geom, int64_t n, double* xmin, double* ymin, double* xmax,
                       double* ymax) {
  if (!ctx || n < 0) return GM_E_INVALID;
  if (n == 0) return GM_OK;
  if (!geom_col_ok(geom) || !xmin || !ymin || !xmax || !ymax) return GM_E_INVALID;
  GM_HIP(hipSetDevice(ctx->device));
  const ArrowGeom g = to_geom(geom);
  const int64_t blocks = std::min<int64_t>((n + GTPB - 1) / GTPB, 256 * 32);
  with_column_form(geom, [&](auto F32, auto WKB) {
    hipLaunchKernelGGL((k_envelopes<decltype(F32)::value, decltype(WKB)::value>), dim3((unsigned)blocks), dim3(GTPB),
                       0, ctx->stream, g, n, xmin, ymin, xmax, ymax);
  });
  GM_CHECK_LAUNCH();
  return GM_OK;
}

}  // extern "C"
