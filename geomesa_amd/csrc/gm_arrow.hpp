// gm_arrow.hpp -- device access to GeoMesa's Arrow geometry vectors (geomesa-arrow-jts): validity
// bits and ordinate tuples.  A tuple is [y, x] unless the vector's flipAxisOrder is set
// (AbstractPointVector.java:52-79, AbstractPolygonVector.java:72-79); Float4 vectors
// (PointFloatVector, ...FloatVector) widen their floats to double on read (readOrdinal).  Also the nested
// geometry column as a kernel argument (ArrowGeom), its tuple runs (ArrowTuples), the walk of one slot
// (arrow_walk) and the JTS envelope as a visitor (Env, EnvelopeOf), shared by the XZ key kernels
// (gm_arrow.hip) and the geometry full filter (gm_geom_filter.hip).  A GM_GEOM_WKB column
// travels in the same ArrowGeom (c: the value bytes, o0: the value offsets) and is read by gm_wkb.hpp only.
#pragma once

#include "gm_internal.hpp"

namespace gm {

// Arrow validity bitmap, LSB bit order; NULL = every slot valid
__device__ __forceinline__ bool arrow_valid(const uint8_t* __restrict__ v, int64_t off, int64_t i) {
  if (!v) return true;
  const int64_t b = off + i;
  return (v[b >> 3] >> (b & 7)) & 1u;
}

// tuple j of an ordinate buffer -> (x, y)
template <bool F32>
__device__ __forceinline__ void arrow_tuple(const void* __restrict__ c, int64_t j, int flip, double& x, double& y) {
  double o0, o1;
  if (F32) {
    const float2 f = ((const float2*)c)[j];
    o0 = (double)f.x;
    o1 = (double)f.y;
  } else {
    const dv2 d = ((const dv2*)c)[j];
    o0 = d.x;
    o1 = d.y;
  }
  x = flip ? o0 : o1;
  y = flip ? o1 : o0;
}

// a point column as a kernel argument
struct ArrowPts {
  const void* c;
  const uint8_t* valid;
  int64_t voff;
  int32_t flip;
  int32_t f32;
};

// ------------------------------------------------------------------ envelopes (XZ keys)
// org.locationtech.jts.geom.Envelope: expandToInclude(x, y) initialises a null envelope and
// otherwise widens with strict compares (a NaN ordinate never widens); expandToInclude(Envelope)
// skips a null envelope.  The null envelope reads back as (minx 0, maxx -1, miny 0, maxy -1).
struct Env {
  double minx, maxx, miny, maxy;
  bool null_;
};

__device__ __forceinline__ Env env_null() { return Env{0.0, -1.0, 0.0, -1.0, true}; }

__device__ __forceinline__ void env_expand(Env& e, double x, double y) {
  if (e.null_) { e = Env{x, x, y, y, false}; return; }
  if (x < e.minx) e.minx = x;
  if (x > e.maxx) e.maxx = x;
  if (y < e.miny) e.miny = y;
  if (y > e.maxy) e.maxy = y;
}

__device__ __forceinline__ void env_merge(Env& e, const Env& o) {
  if (o.null_) return;
  if (e.null_) { e = o; return; }
  if (o.minx < e.minx) e.minx = o.minx;
  if (o.maxx > e.maxx) e.maxx = o.maxx;
  if (o.miny < e.miny) e.miny = o.miny;
  if (o.maxy > e.maxy) e.maxy = o.maxy;
}

struct ArrowGeom {
  const void* c;
  const uint8_t* valid;
  int64_t voff;
  const int32_t* o0;
  const int32_t* o1;
  const int32_t* o2;
  int32_t type;
  int32_t flip;
};

// the tuples of a typed column from tuple `c` on, as a tuple source (a WKB run is the other one: WkbTuples,
// gm_wkb.hpp); a visitor sees either as (tuples, n) and reads tuple j, 0 <= j < n
template <bool F32>
struct ArrowTuples {
  static constexpr bool WKB = false;
  const void* c;
  int flip;
  __device__ __forceinline__ void tuple(int64_t j, double& x, double& y) const { arrow_tuple<F32>(c, j, flip, x, y); }
};

// Walks slot i of a typed column: the switch over the typed kinds (the polygon filter keeps its own), wkb_walk's
// (gm_wkb.hpp) counterpart.  The visitor's calls return true to stop the walk, which then returns true:
//   point(t)        the tuple of a Point
//   points(t, n)    the n tuples of a MultiPoint, one run (a WKB MultiPoint's points carry a header each and
//                   arrive one per point(); only this walk makes the call)
//   line(t, n)      the n tuples of a LineString
//   polygon_begin() then ring(r, t, n) for each ring, shell first, then polygon_end()
// with t an ArrowTuples<F32>; n is signed and an offset pair that runs backwards reads as no tuples.
// UNI as in wkb_walk: the whole wave is on slot i and the offsets go through readfirstlane, so the walk's
// control flow stays scalar; otherwise each lane walks its own slot with plain loads.
template <bool UNI, bool F32, class V>
__device__ __forceinline__ bool arrow_walk(const ArrowGeom& g, int64_t i, V& v) {
  const auto off = [](const int32_t* __restrict__ o, int64_t k) __attribute__((always_inline)) {
    return UNI ? __builtin_amdgcn_readfirstlane(o[k]) : o[k];
  };
  const auto run = [&](int64_t a) __attribute__((always_inline)) {
    return ArrowTuples<F32>{(const char*)g.c + a * (F32 ? 8 : 16), g.flip};
  };
  const auto polygon = [&](const int32_t* __restrict__ ro, int32_t r0, int32_t r1) __attribute__((always_inline)) {
    v.polygon_begin();
    for (int32_t r = r0; r < r1; ++r) {
      const int32_t a = off(ro, r);
      if (v.ring((uint32_t)(r - r0), run(a), off(ro, r + 1) - a)) return true;
    }
    return v.polygon_end();
  };
  const bool nested = g.type != GM_GEOM_POINT;   // a Point column has no offsets
  const int32_t a = nested ? off(g.o0, i) : 0, b = nested ? off(g.o0, i + 1) : 0;
  switch (g.type) {
    case GM_GEOM_POINT: return v.point(run(i));
    case GM_GEOM_MULTIPOINT: return v.points(run(a), b - a);
    case GM_GEOM_LINESTRING: return v.line(run(a), b - a);
    case GM_GEOM_POLYGON: return polygon(g.o1, a, b);
    case GM_GEOM_MULTILINESTRING:
      for (int32_t l = a; l < b; ++l) {
        const int32_t t0 = off(g.o1, l);
        if (v.line(run(t0), off(g.o1, l + 1) - t0)) return true;
      }
      return false;
    default:   // GM_GEOM_MULTIPOLYGON
      for (int32_t p = a; p < b; ++p)
        if (polygon(g.o2, off(g.o1, p), off(g.o1, p + 1))) return true;
      return false;
  }
}

// Geometry.getEnvelopeInternal as a visitor of either walk: every element's own envelope
// (CoordinateSequence.expandEnvelope: the first tuple initialises, strict compares after it), merged
// skipping null ones (GeometryCollection.computeEnvelopeInternal); a polygon's is its shell's
// (Polygon.computeEnvelopeInternal).  It never stops the walk
struct EnvelopeOf {
  Env e;
  template <class T>
  __device__ __forceinline__ static Env of(const T& t, int32_t n) {
    Env r = env_null();
    for (int32_t j = 0; j < n; ++j) {
      double x, y;
      t.tuple(j, x, y);
      env_expand(r, x, y);
    }
    return r;
  }
  // A WKB Point with a NaN x or y is the empty point (WKBWriter's encoding of it) and is skipped; a typed
  // Point's tuple is taken as it is, NaN included, so such a slot's XZ key status differs by column form
  template <class T>
  __device__ __forceinline__ bool point(const T& t) {
    double x, y;
    t.tuple(0, x, y);
    if (!T::WKB || (x == x && y == y)) env_merge(e, Env{x, x, y, y, false});
    return false;
  }
  template <class T>
  __device__ __forceinline__ bool points(const T& t, int32_t n) { return line(t, n); }
  template <class T>
  __device__ __forceinline__ bool line(const T& t, int32_t n) {
    env_merge(e, of(t, n));
    return false;
  }
  __device__ __forceinline__ void polygon_begin() {}
  template <class T>
  __device__ __forceinline__ bool ring(uint32_t r, const T& t, int32_t n) { return r == 0 && line(t, n); }
  __device__ __forceinline__ bool polygon_end() { return false; }
};

// the List offsets a geometry type needs, outermost first
inline int offset_levels(int type) {
  switch (type) {
    case GM_GEOM_POINT: return 0;
    case GM_GEOM_LINESTRING: case GM_GEOM_MULTIPOINT: return 1;
    case GM_GEOM_POLYGON: case GM_GEOM_MULTILINESTRING: return 2;
    case GM_GEOM_MULTIPOLYGON: return 3;
    default: return -1;
  }
}

inline bool geom_col_ok(const gm_geom_column* g) {
  if (!g || !g->coords || (g->ordinal_bits != 64 && g->ordinal_bits != 32)) return false;
  if (g->type == GM_GEOM_WKB) return g->ordinal_bits == 64 && g->offsets[0];   // value bytes, value offsets
  const int lv = offset_levels(g->type);
  if (lv < 0) return false;
  for (int k = 0; k < lv; ++k)
    if (!g->offsets[k]) return false;
  return true;
}

// The entries that read typed columns only: true (and the gm_last_error text) for a GM_GEOM_WKB column.
// A point entry names the adapter that takes such a column's points to x / y columns.
inline bool rejects_wkb(const gm_geom_column* g, const char* who, bool point_entry) {
  if (!g || g->type != GM_GEOM_WKB) return false;
  set_error(std::string(who) + ": a GM_GEOM_WKB column is not read here" +
            (point_entry ? "; gm_arrow_points_to_columns gives its points as x / y columns" : ""));
  return true;
}

}  // namespace gm
