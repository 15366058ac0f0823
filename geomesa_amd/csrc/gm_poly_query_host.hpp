// gm_poly_query_host.hpp -- the query polygons of gm_table_scan_geom (gm_scan_filter.polys) as the exact
// filter reads them (k_poly_refine, gm_geom_filter.hip): validation and the y-slab buckets over the ring
// edges.  Host-only and free of HIP, so that a plain C++ program (tools/poly_query_check.cpp) compiles the
// same builder the library runs.
//
// The query's y-range [y0, y1] is cut into ns slabs by slab_of, a non-decreasing function of y.  An edge is
// entered into every slab from slab_of(its lower y) to slab_of(its upper y), so two segments whose closed
// y-ranges share a y share a slab, whatever the rounding of slab_of: a feature segment that visits the
// slabs of its own y-range sees every edge it can meet, and a point sees in its one slab every edge whose
// y-range holds its y -- the only ones RayCrossingCounter.countSegment can count or find it on.  The
// entries are stored slab by slab with their coordinates (an edge crossing k slabs is stored k times), in
// ring order within a slab: the slabs a y-range overlaps are ONE contiguous run of entries, and the
// entries of one ring, and of one part, are contiguous within a slab.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/geomesa_hip.h"

namespace gm {
namespace polyq {

constexpr int MAX_SLABS = 4096;
constexpr int DUP_MAX = 2;   // bucket entries <= DUP_MAX x edges: the slab count is halved until they are

inline int slab_of(double y, double y0, double inv_h, int ns) {
  const double c = floor((y - y0) * inv_h);
  if (!(c >= 0.0)) return 0;   // below the range, or NaN
  return c > (double)(ns - 1) ? ns - 1 : (int)c;
}

struct HostQuery {
  int32_t n_parts = 0, n_rings = 0, n_edges = 0, ns = 1;
  double x0 = 0, y0 = 0, x1 = -1, y1 = -1, inv_h = 0;   // the envelope of all parts; the slab scale
  std::vector<double> penv;     // n_parts x (xmin, ymin, xmax, ymax): each part's envelope (its shell's)
  std::vector<double> pv0;      // n_parts x (x, y): each part's first shell vertex
  std::vector<int32_t> pring;   // n_parts + 1: each part's ring range
  std::vector<int32_t> soff;    // ns + 1: slab s holds the entries [soff[s], soff[s + 1])
  std::vector<double> edge;     // entries x (ax, ay, bx, by)
  std::vector<int32_t> eid;     // entries: the edge's index in ring order (the checker's; not uploaded)
  std::vector<int32_t> ering;   // entries: the edge's ring
  std::vector<int32_t> epart;   // entries: the edge's part * 2 + (1 when the ring is the part's shell)
  int64_t entries() const { return (int64_t)ering.size(); }
};

// what makes a query polygon set unusable, or null: the CSR arrays, at least one part, every ring closed
// with at least 4 tuples and finite ordinates, at most GM_POLY_QUERY_MAX_VERTICES tuples in all
inline const char* validate(const gm_polyset* ps) {
  if (!ps || ps->n_polys < 0 || !ps->poly_part_off || !ps->part_ring_off || !ps->ring_vert_off)
    return "the polygon set's offset arrays are required";
  const int32_t np = ps->poly_part_off[ps->n_polys];
  if (ps->poly_part_off[0] != 0 || np <= 0) return "at least one query polygon part is required";
  for (int32_t p = 0; p < ps->n_polys; ++p)
    if (ps->poly_part_off[p + 1] < ps->poly_part_off[p]) return "polygon offsets run backwards";
  if (ps->part_ring_off[0] != 0) return "ring offsets must start at 0";
  for (int32_t p = 0; p < np; ++p)
    if (ps->part_ring_off[p + 1] <= ps->part_ring_off[p]) return "a query polygon part without a shell";
  const int32_t nr = ps->part_ring_off[np];
  if (ps->ring_vert_off[0] != 0) return "vertex offsets must start at 0";
  for (int32_t r = 0; r < nr; ++r) {
    const int64_t n = (int64_t)ps->ring_vert_off[r + 1] - ps->ring_vert_off[r];
    if (n < 4) return "a query ring has fewer than 4 tuples";
    if (ps->ring_vert_off[r + 1] > GM_POLY_QUERY_MAX_VERTICES)
      return "the query polygons hold more than GM_POLY_QUERY_MAX_VERTICES tuples";
  }
  if (!ps->vx || !ps->vy) return "the polygon set's vertex arrays are required";
  for (int32_t r = 0; r < nr; ++r) {
    const int32_t a = ps->ring_vert_off[r], b = ps->ring_vert_off[r + 1];
    for (int32_t v = a; v < b; ++v)
      if (!isfinite(ps->vx[v]) || !isfinite(ps->vy[v])) return "a query ring has a NaN or infinite ordinate";
    if (ps->vx[a] != ps->vx[b - 1] || ps->vy[a] != ps->vy[b - 1]) return "a query ring is not closed";
  }
  return nullptr;
}

// the device arrays' host images of a validated set
inline void build(const gm_polyset* ps, HostQuery& q) {
  q = HostQuery();
  q.n_parts = ps->poly_part_off[ps->n_polys];
  q.n_rings = ps->part_ring_off[q.n_parts];
  q.n_edges = ps->ring_vert_off[q.n_rings] - q.n_rings;
  q.pring.assign(ps->part_ring_off, ps->part_ring_off + q.n_parts + 1);
  for (int32_t p = 0; p < q.n_parts; ++p) {
    const int32_t r = ps->part_ring_off[p], a = ps->ring_vert_off[r], b = ps->ring_vert_off[r + 1];
    double e[4] = {ps->vx[a], ps->vy[a], ps->vx[a], ps->vy[a]};
    for (int32_t v = a + 1; v < b; ++v) {
      if (ps->vx[v] < e[0]) e[0] = ps->vx[v];
      if (ps->vy[v] < e[1]) e[1] = ps->vy[v];
      if (ps->vx[v] > e[2]) e[2] = ps->vx[v];
      if (ps->vy[v] > e[3]) e[3] = ps->vy[v];
    }
    q.penv.insert(q.penv.end(), e, e + 4);
    q.pv0.push_back(ps->vx[a]);
    q.pv0.push_back(ps->vy[a]);
  }
  // every ring's y takes part in the slab range (a hole outside its shell is still walked)
  q.x0 = q.x1 = ps->vx[0];
  q.y0 = q.y1 = ps->vy[0];
  for (int32_t v = 1; v < ps->ring_vert_off[q.n_rings]; ++v) {
    if (ps->vx[v] < q.x0) q.x0 = ps->vx[v];
    if (ps->vx[v] > q.x1) q.x1 = ps->vx[v];
    if (ps->vy[v] < q.y0) q.y0 = ps->vy[v];
    if (ps->vy[v] > q.y1) q.y1 = ps->vy[v];
  }
  auto span = [&](int32_t v, int& s0, int& s1) {
    const double lo = ps->vy[v] < ps->vy[v + 1] ? ps->vy[v] : ps->vy[v + 1];
    const double hi = ps->vy[v] < ps->vy[v + 1] ? ps->vy[v + 1] : ps->vy[v];
    s0 = slab_of(lo, q.y0, q.inv_h, q.ns);
    s1 = slab_of(hi, q.y0, q.inv_h, q.ns);
  };
  auto each_edge = [&](auto fn) {
    int32_t id = 0;
    for (int32_t p = 0; p < q.n_parts; ++p)
      for (int32_t r = ps->part_ring_off[p]; r < ps->part_ring_off[p + 1]; ++r)
        for (int32_t v = ps->ring_vert_off[r]; v < ps->ring_vert_off[r + 1] - 1; ++v)
          fn(id++, v, r, p * 2 + (r == ps->part_ring_off[p] ? 1 : 0));
  };
  int ns = q.n_edges / 2 < 1 ? 1 : (q.n_edges / 2 > MAX_SLABS ? MAX_SLABS : q.n_edges / 2);
  const double height = q.y1 - q.y0;
  for (;; ns /= 2) {
    q.ns = height > 0.0 ? ns : 1;
    q.inv_h = height > 0.0 ? (double)q.ns / height : 0.0;
    q.soff.assign((size_t)q.ns + 1, 0);
    each_edge([&](int32_t, int32_t v, int32_t, int32_t) {
      int s0, s1;
      span(v, s0, s1);
      for (int s = s0; s <= s1; ++s) ++q.soff[(size_t)s + 1];
    });
    for (int s = 0; s < q.ns; ++s) q.soff[(size_t)s + 1] += q.soff[(size_t)s];
    if (q.ns == 1 || q.soff[(size_t)q.ns] <= (int64_t)DUP_MAX * q.n_edges) break;
  }
  const size_t nb = (size_t)q.soff[(size_t)q.ns];
  q.edge.resize(nb * 4);
  q.eid.resize(nb);
  q.ering.resize(nb);
  q.epart.resize(nb);
  std::vector<int32_t> at(q.soff.begin(), q.soff.end() - 1);
  each_edge([&](int32_t id, int32_t v, int32_t r, int32_t pw) {
    int s0, s1;
    span(v, s0, s1);
    for (int s = s0; s <= s1; ++s) {
      const size_t e = (size_t)at[(size_t)s]++;
      q.edge[4 * e] = ps->vx[v];
      q.edge[4 * e + 1] = ps->vy[v];
      q.edge[4 * e + 2] = ps->vx[v + 1];
      q.edge[4 * e + 3] = ps->vy[v + 1];
      q.eid[e] = id;
      q.ering[e] = r;
      q.epart[e] = pw;
    }
  });
}

}  // namespace polyq
}  // namespace gm
