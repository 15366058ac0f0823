// gm_wkb.hpp -- device access to a GM_GEOM_WKB column: GeoMesa's WKBGeometryVector (geomesa-arrow-jts
// WKBGeometryVector.java:27-93), an Arrow Binary column holding one JTS WKBWriter blob per slot, any
// geometry class in any slot.  The blob grammar is the one geomesa_hip.h states (OGC / ISO WKB plus the
// EWKB flag bits); this file is its only reader on the device:
//   * WkbCur: a slot's bytes [p, end).  Every read goes through wkb_head / wkb_count / wkb_run, which
//     compare what the header claims with the bytes that remain (count * stride in 64 bits) BEFORE the
//     cursor moves, so no byte outside the slot is ever read, whatever the blob says;
//   * wkb_walk: the traversal, shared by its uses (envelopes and XZ keys, the exact box and polygon
//     filters), with the visitor protocol of arrow_walk (gm_arrow.hpp): a decision can be written once, as a
//     visitor templated on the tuple source, and serves both column forms.  Collections are walked with
//     an explicit stack of the element counts still to read, GM_WKB_MAX_DEPTH levels deep, kept in LDS (a
//     register array indexed by the depth would live in scratch); the code a Multi*'s elements must carry
//     takes 4 bits per level of one register.  A visitor sees each point, line and ring as a WkbTuples
//     (first byte, stride in bytes, byte order) with its tuple count, and may stop the walk;
//   * UNI: the caller is a whole wave on one slot; headers and counts then go through readfirstlane so
//     the walk's control flow stays scalar.
// Ordinates are moved as 64-bit integers from unaligned addresses (memcpy: slots start at any byte),
// byte-swapped when big-endian, then bit-cast: NaN payloads and -0.0 arrive as they were written.
// A malformed slot (wkb_walk's WKB_BAD) is treated by every caller exactly as a null slot.
#pragma once

#include "gm_arrow.hpp"

namespace gm {

constexpr int WKB_DEPTH = GM_WKB_MAX_DEPTH;

enum : uint32_t { WKB_POINT = 1, WKB_LINESTRING = 2, WKB_POLYGON = 3, WKB_MULTIPOINT = 4, WKB_COLLECTION = 7 };
enum : int { WKB_BAD = 0, WKB_END = 1, WKB_STOP = 2 };   // malformed; walked to its end; stopped by the visitor

template <bool UNI>
__device__ __forceinline__ uint32_t wkb_uni(uint32_t v) {
  if constexpr (UNI) return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  return v;
}

__device__ __forceinline__ uint32_t wkb_u32(const uint8_t* p, bool le) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return le ? v : __builtin_bswap32(v);
}

__device__ __forceinline__ double wkb_f64(const uint8_t* p, bool le) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  if (!le) v = __builtin_bswap64(v);
  double d;
  __builtin_memcpy(&d, &v, 8);
  return d;
}

struct WkbCur {
  const uint8_t* p;
  const uint8_t* end;
  __device__ __forceinline__ int64_t left() const { return end - p; }
};

// the bytes of slot i (a slot whose offsets run backwards has none, and so is malformed)
__device__ __forceinline__ WkbCur wkb_slot(const ArrowGeom& g, int64_t i) {
  const uint8_t* b = (const uint8_t*)g.c;
  return WkbCur{b + g.o0[i], b + g.o0[i + 1]};
}

struct WkbHead {
  uint32_t code;     // 1 .. 7
  uint32_t stride;   // bytes per tuple: 16, 24 (Z or M) or 32 (ZM)
  bool le;
};

// order byte, typeInt and the SRID when flagged; false: malformed
template <bool UNI>
__device__ __forceinline__ bool wkb_head(WkbCur& c, WkbHead& h) {
  if (c.left() < 5) return false;
  const uint32_t order = wkb_uni<UNI>(c.p[0]);
  if (order > 1) return false;
  h.le = order == 1;
  const uint32_t t = wkb_uni<UNI>(wkb_u32(c.p + 1, h.le));
  c.p += 5;
  if (t & 0x20000000u) {
    if (c.left() < 4) return false;
    c.p += 4;
  }
  const uint32_t lo = t & 0xffffu, iso = lo / 1000u;
  h.code = lo % 1000u;
  const uint32_t z = (t >> 31) | (uint32_t)(iso == 1 || iso == 3);
  const uint32_t m = ((t >> 30) & 1u) | (uint32_t)(iso == 2 || iso == 3);
  h.stride = 8u * (2u + z + m);
  return h.code >= WKB_POINT && h.code <= WKB_COLLECTION;
}

template <bool UNI>
__device__ __forceinline__ bool wkb_count(WkbCur& c, bool le, uint32_t& n) {
  if (c.left() < 4) return false;
  n = wkb_uni<UNI>(wkb_u32(c.p, le));
  c.p += 4;
  return true;
}

// a run of n items of `stride` bytes: its first byte, and the cursor past it; false when the run
// would end past the slot (nothing is read and the cursor stays)
__device__ __forceinline__ bool wkb_run(WkbCur& c, uint32_t n, uint32_t stride, const uint8_t*& base) {
  const uint64_t bytes = (uint64_t)n * stride;
  if (bytes > (uint64_t)c.left()) return false;
  base = c.p;
  c.p += bytes;
  return true;
}

// a tuple run as a tuple source, from its first byte on (a typed column's: ArrowTuples, gm_arrow.hpp)
struct WkbTuples {
  static constexpr bool WKB = true;
  const uint8_t* base;
  uint32_t stride;
  bool le;
  __device__ __forceinline__ void tuple(int64_t j, double& x, double& y) const {
    const uint8_t* t = base + j * (int64_t)stride;
    x = wkb_f64(t, le);
    y = wkb_f64(t + 8, le);
  }
};

// Walks one slot.  rem[k * rs], k < WKB_DEPTH, is this walker's stack (LDS).  The visitor's point / line /
// ring / polygon_end return true to stop the walk (WKB_STOP); the protocol is arrow_walk's (gm_arrow.hpp),
// so one visitor serves both column forms:
//   point(t)        the tuple of a Point (a MultiPoint's points arrive here too, one per call)
//   line(t, n)      the n tuples of a LineString
//   polygon_begin() then ring(r, t, n) for each ring, shell first, then polygon_end()
// with t a WkbTuples and n < 2^27 (the slot's bytes bound it), handed over signed.  The shortest geometry is
// 9 bytes (an empty LineString, Polygon or collection) and the shortest ring 4, so a count that cannot fit in
// the bytes left is malformed before its elements are looked at; that also bounds the walk by the slot's
// length.
template <bool UNI, class V>
__device__ __forceinline__ int wkb_walk(WkbCur c, uint32_t* rem, int rs, V& v) {
  int depth = 0;        // collections around the geometry being read
  uint32_t need = 0;    // 4 bits per level: the code a Multi*'s elements must have, 0 = any
  uint32_t left = 1;    // geometries still to read at this level
  for (;;) {
    while (left == 0) {
      if (depth == 0) return WKB_END;
      --depth;
      left = wkb_uni<UNI>(rem[depth * rs]);
    }
    --left;
    WkbHead h;
    if (!wkb_head<UNI>(c, h)) return WKB_BAD;
    const uint32_t want = depth ? (need >> (4 * (depth - 1))) & 15u : 0u;
    if (want && h.code != want) return WKB_BAD;
    const uint8_t* base;
    uint32_t n;
    if (h.code == WKB_POINT) {
      if (!wkb_run(c, 1, h.stride, base)) return WKB_BAD;
      if (v.point(WkbTuples{base, h.stride, h.le})) return WKB_STOP;
    } else if (h.code == WKB_LINESTRING) {
      if (!wkb_count<UNI>(c, h.le, n) || !wkb_run(c, n, h.stride, base)) return WKB_BAD;
      if (v.line(WkbTuples{base, h.stride, h.le}, (int32_t)n)) return WKB_STOP;
    } else if (h.code == WKB_POLYGON) {
      uint32_t nr;
      if (!wkb_count<UNI>(c, h.le, nr) || (uint64_t)nr * 4 > (uint64_t)c.left()) return WKB_BAD;
      v.polygon_begin();
      for (uint32_t r = 0; r < nr; ++r) {
        if (!wkb_count<UNI>(c, h.le, n) || !wkb_run(c, n, h.stride, base)) return WKB_BAD;
        if (v.ring(r, WkbTuples{base, h.stride, h.le}, (int32_t)n)) return WKB_STOP;
      }
      if (v.polygon_end()) return WKB_STOP;
    } else {   // MultiPoint, MultiLineString, MultiPolygon, GeometryCollection
      if (!wkb_count<UNI>(c, h.le, n) || (uint64_t)n * 9 > (uint64_t)c.left()) return WKB_BAD;
      if (depth == WKB_DEPTH) return WKB_BAD;
      rem[depth * rs] = left;
      const uint32_t elem = h.code == WKB_COLLECTION ? 0u : h.code - 3u;
      need = (need & ~(15u << (4 * depth))) | (elem << (4 * depth));
      ++depth;
      left = n;
    }
  }
}

// slot i of either column form through one call (rem / rs are unused by a typed column, whose slots are
// never malformed)
template <bool UNI, bool F32, bool WKB, class V>
__device__ __forceinline__ int geom_walk(const ArrowGeom& g, int64_t i, uint32_t* rem, int rs, V& v) {
  if constexpr (WKB) return wkb_walk<UNI>(wkb_slot(g, i), rem, rs, v);
  else return arrow_walk<UNI, F32>(g, i, v) ? WKB_STOP : WKB_END;
}

// ------------------------------------------------------------------ envelopes
// Geometry.getEnvelopeInternal of slot i of either column form, one lane per slot (EnvelopeOf,
// gm_arrow.hpp); false: a malformed WKB slot (e is then the null envelope)
template <bool F32, bool WKB>
__device__ __forceinline__ bool slot_envelope(const ArrowGeom& g, int64_t i, uint32_t* rem, int rs, Env& e) {
  EnvelopeOf v{env_null()};
  const bool ok = geom_walk<false, F32, WKB>(g, i, rem, rs, v) != WKB_BAD;
  e = ok ? v.e : env_null();
  return ok;
}

}  // namespace gm
