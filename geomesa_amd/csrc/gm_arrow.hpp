// gm_arrow.hpp -- device access to GeoMesa's Arrow geometry vectors (geomesa-arrow-jts): validity
// bits and ordinate tuples.  A tuple is [y, x] unless the vector's flipAxisOrder is set
// (AbstractPointVector.java:52-79, AbstractPolygonVector.java:72-79); Float4 vectors
// (PointFloatVector, ...FloatVector) widen their floats to double on read (readOrdinal).  Also the nested
// geometry column as a kernel argument (ArrowGeom) and its JTS envelope walk (Env, geom_envelope), shared by
// the XZ key kernels (gm_arrow.hip) and the geometry full filter (gm_geom_filter.hip).  A GM_GEOM_WKB column
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

// CoordinateSequence.expandEnvelope over tuples [a, b)
template <bool F32>
__device__ __forceinline__ Env env_tuples(const ArrowGeom& g, int64_t a, int64_t b) {
  Env e = env_null();
  for (int64_t j = a; j < b; ++j) {
    double x, y;
    arrow_tuple<F32>(g.c, j, g.flip, x, y);
    env_expand(e, x, y);
  }
  return e;
}

// Geometry.getEnvelopeInternal of slot i: a polygon's is its shell's (Polygon.computeEnvelopeInternal),
// a multi geometry's the merge of its parts' (GeometryCollection.computeEnvelopeInternal)
template <bool F32>
__device__ Env geom_envelope(const ArrowGeom& g, int64_t i) {
  switch (g.type) {
    case GM_GEOM_POINT: {
      Env e = env_null();
      double x, y;
      arrow_tuple<F32>(g.c, i, g.flip, x, y);
      env_expand(e, x, y);
      return e;
    }
    case GM_GEOM_LINESTRING:
    case GM_GEOM_MULTIPOINT:
      return env_tuples<F32>(g, g.o0[i], g.o0[i + 1]);
    case GM_GEOM_POLYGON: {
      const int32_t r0 = g.o0[i], r1 = g.o0[i + 1];
      if (r1 <= r0) return env_null();
      return env_tuples<F32>(g, g.o1[r0], g.o1[r0 + 1]);
    }
    case GM_GEOM_MULTILINESTRING: {
      Env e = env_null();
      for (int32_t l = g.o0[i]; l < g.o0[i + 1]; ++l) env_merge(e, env_tuples<F32>(g, g.o1[l], g.o1[l + 1]));
      return e;
    }
    default: {   // GM_GEOM_MULTIPOLYGON
      Env e = env_null();
      for (int32_t p = g.o0[i]; p < g.o0[i + 1]; ++p) {
        const int32_t r0 = g.o1[p], r1 = g.o1[p + 1];
        if (r1 > r0) env_merge(e, env_tuples<F32>(g, g.o2[r0], g.o2[r0 + 1]));
      }
      return e;
    }
  }
}

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
