// gm_pip_build_host.hpp -- the host side of the polygon index build, as plain C++ (no HIP include, no
// device memory): the host restatement of the JTS point locator, prepare() = rings, slabs, polygon
// envelopes and the grid (the BuildPlan both builds work from), and classify() = the host build of
// the cell words, lists and blobs (GM_PARAM_INDEX_BUILD = 1, and every set the device build
// declines).  Compiled into gm_pip_build.hip, and on its own by tools/pip_host_build_check.cpp.
// Reference: RelationUtils.grid (RelationUtils.scala:30-157).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/geomesa_hip.h"
#include "gm_pip_layout.hpp"

namespace gm {
namespace host {

// ------------------------------------------------------------------ host-side JTS (index build)
inline int sgn(double x) { return x > 0 ? 1 : (x < 0 ? -1 : 0); }

// CGAlgorithmsDD.orientationIndex (filter + DD), host copy for the index build
inline int orientation(double p1x, double p1y, double p2x, double p2y, double qx, double qy) {
  volatile double detleft = (p1x - qx) * (p2y - qy);
  volatile double detright = (p1y - qy) * (p2x - qx);
  double det = detleft - detright, detsum;
  if (detleft > 0.0) {
    if (detright <= 0.0) return sgn(det);
    detsum = detleft + detright;
  } else if (detleft < 0.0) {
    if (detright >= 0.0) return sgn(det);
    detsum = -detleft - detright;
  } else {
    return sgn(det);
  }
  double errbound = 1e-15 * detsum;
  if ((det >= errbound) || (-det >= errbound)) return sgn(det);
  auto add_d = [](double hi, double lo, double y, double& rhi, double& rlo) {
    double S = hi + y, e = S - hi, s = S - e;
    s = (y - e) + (hi - s);
    double f = s + lo, H = S + f, h = f + (S - H);
    rhi = H + h;
    rlo = h + (H - rhi);
  };
  auto mul = [](double hi, double lo, double yhi, double ylo, double& rhi, double& rlo) {
    const double SPLIT = 134217729.0;
    double C = SPLIT * hi, hx = C - hi, c = SPLIT * yhi;
    hx = C - hx;
    double tx = hi - hx, hy = c - yhi;
    C = hi * yhi;
    hy = c - hy;
    double ty = yhi - hy;
    c = ((((hx * hy - C) + hx * ty) + tx * hy) + tx * ty) + (hi * ylo + lo * yhi);
    double zhi = C + c;
    hx = C - zhi;
    rhi = zhi;
    rlo = c + hx;
  };
  double a1, a2, b1, b2, c1, c2, d1, d2, ah, al, bh, bl;
  add_d(p2x, 0.0, -p1x, a1, a2);
  add_d(p2y, 0.0, -p1y, b1, b2);
  add_d(qx, 0.0, -p2x, c1, c2);
  add_d(qy, 0.0, -p2y, d1, d2);
  mul(a1, a2, d1, d2, ah, al);
  mul(b1, b2, c1, c2, bh, bl);
  double yhi = -bh, ylo = -bl;
  double S = ah + yhi, T = al + ylo, e = S - ah, f = T - al, s = S - e, t = T - f;
  s = (yhi - e) + (ah - s);
  t = (ylo - f) + (al - t);
  e = s + T;
  double H = S + e, h = e + (S - H);
  e = t + h;
  double zhi = H + e, zlo = e + (H - zhi);
  if (zhi > 0.0) return 1;
  if (zhi < 0.0) return -1;
  if (zlo > 0.0) return 1;
  if (zlo < 0.0) return -1;
  return 0;
}

inline int locate_ring(const double* vx, const double* vy, int n, double px, double py) {
  if (n < 1) return LOC_EXTERIOR;
  double mnx = vx[0], mxx = vx[0], mny = vy[0], mxy = vy[0];
  for (int i = 1; i < n; ++i) {
    mnx = std::min(mnx, vx[i]); mxx = std::max(mxx, vx[i]);
    mny = std::min(mny, vy[i]); mxy = std::max(mxy, vy[i]);
  }
  if (!(px >= mnx && px <= mxx && py >= mny && py <= mxy)) return LOC_EXTERIOR;
  int crossings = 0;
  for (int i = 1; i < n; ++i) {
    double p1x = vx[i], p1y = vy[i], p2x = vx[i - 1], p2y = vy[i - 1];
    if (p1x < px && p2x < px) continue;
    if (px == p2x && py == p2y) return LOC_BOUNDARY;
    if (p1y == py && p2y == py) {
      double mn = std::min(p1x, p2x), mx = std::max(p1x, p2x);
      if (px >= mn && px <= mx) return LOC_BOUNDARY;
      continue;
    }
    if (((p1y > py) && (p2y <= py)) || ((p2y > py) && (p1y <= py))) {
      int o = orientation(p1x, p1y, p2x, p2y, px, py);
      if (o == 0) return LOC_BOUNDARY;
      if (p2y < p1y) o = -o;
      if (o == 1) crossings++;
    }
  }
  return (crossings & 1) ? LOC_INTERIOR : LOC_EXTERIOR;
}

inline int locate_poly(const gm_polyset* ps, int poly, double px, double py) {
  bool is_in = false;
  int nb = 0;
  for (int p = ps->poly_part_off[poly]; p < ps->poly_part_off[poly + 1]; ++p) {
    const int r0 = ps->part_ring_off[p], r1 = ps->part_ring_off[p + 1];
    if (r1 <= r0) continue;
    const int v0 = ps->ring_vert_off[r0], v1 = ps->ring_vert_off[r0 + 1];
    int loc = locate_ring(ps->vx + v0, ps->vy + v0, v1 - v0, px, py);
    if (loc == LOC_INTERIOR) {
      for (int r = r0 + 1; r < r1; ++r) {
        const int h0 = ps->ring_vert_off[r], h1 = ps->ring_vert_off[r + 1];
        const int hl = locate_ring(ps->vx + h0, ps->vy + h0, h1 - h0, px, py);
        if (hl == LOC_INTERIOR) { loc = LOC_EXTERIOR; break; }
        if (hl == LOC_BOUNDARY) { loc = LOC_BOUNDARY; break; }
      }
    }
    if (loc == LOC_INTERIOR) is_in = true;
    if (loc == LOC_BOUNDARY) nb++;
  }
  if (nb & 1) return LOC_BOUNDARY;
  if (nb > 0 || is_in) return LOC_INTERIOR;
  return LOC_EXTERIOR;
}

inline int cell_of(double v, double v0, double inv, int g) {
  volatile double t = (v - v0) * inv;  // keep the exact device op order (sub, mul, floor)
  double c = floor(t);
  if (!(c >= 0.0)) return 0;
  if (c >= (double)g) return g - 1;
  return (int)c;
}

// ------------------------------------------------------------------ threads
// host threads of the index build: GM_BUILD_THREADS, else OMP_NUM_THREADS (16 on the GPU boxes),
// else the machine's, at most 64
inline int build_threads() {
  for (const char* v : {"GM_BUILD_THREADS", "OMP_NUM_THREADS"}) {
    const char* s = getenv(v);
    if (s && atoi(s) > 0) return std::min(64, atoi(s));
  }
  const unsigned hc = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(64u, hc ? hc : 1u));
}

// fn(i) for i in [0, n) over the build threads (contiguous blocks of items per thread)
template <class F>
void parallel_for(int n, F fn) {
  const int nth = std::max(1, std::min(build_threads(), n / 64));
  if (nth <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
  std::atomic<int> next{0};
  auto work = [&]() {
    for (;;) {
      const int b = next.fetch_add(64);
      if (b >= n) break;
      for (int i = b; i < std::min(n, b + 64); ++i) fn(i);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nth; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ------------------------------------------------------------------ the prepared plan
// What both builds start from, computed once by prepare(): the ring / slab arrays of the fallback
// walk (index arrays 0-2), the polygon envelopes, and the grid.
struct BuildPlan {
  std::vector<RingDev> rings;
  std::vector<int32_t> slab_off;
  std::vector<Edge> slab_edges;
  std::vector<double> env;        // 4 per polygon (empty polygon: +inf / -inf)
  double G[4];                    // the set's envelope x0 y0 x1 y1 (nothing to match: 0 0 -1 -1)
  int gx, gy, gxc;                // grid columns, rows, coarse columns
  double inv_cw, inv_ch, epsx, epsy;   // inverse cell width / height; the cells' inflation
  bool any, degenerate;           // a polygon has an envelope; the set's envelope has no width or height
  int64_t ncell;
};

inline void prepare(const gm_polyset* ps, int cells_per_poly_in, BuildPlan& plan) {
  const int P = ps->n_polys;
  const int n_parts = P ? ps->poly_part_off[P] : 0;
  const int n_rings = n_parts ? ps->part_ring_off[n_parts] : 0;
  const int n_verts = n_rings ? ps->ring_vert_off[n_rings] : 0;
  const double* vx = ps->vx;
  const double* vy = ps->vy;

  // ---- rings: envelopes + y-slab segment buckets (fallback walk); segments by end vertex
  std::vector<RingDev>& rings = plan.rings;
  std::vector<int32_t>& slab_off = plan.slab_off;
  std::vector<Edge>& slab_edges = plan.slab_edges;
  rings.assign((size_t)n_rings, RingDev{});
  std::vector<Edge> segs((size_t)std::max(n_verts, 1));  // segs: segment ending at vertex i
  // per ring: envelope and slab count (parallel over rings), then flat counting-sort of the
  // segments into their slabs (two passes over each ring, no per-slab vectors)
  std::vector<int64_t> ring_slab_base((size_t)n_rings + 1, 0), ring_edge_base((size_t)n_rings + 1, 0);
  // the slabs [s0, s1] of ring rd that the segment ending at vertex i meets
  auto slab_range = [&](const RingDev& rd, int i, int& s0, int& s1) {
    s0 = cell_of(std::min(vy[i], vy[i - 1]), rd.y0, rd.inv_h, rd.ns);
    s1 = cell_of(std::max(vy[i], vy[i - 1]), rd.y0, rd.inv_h, rd.ns);
  };
  auto ring_env = [&](int r) {
    const int v0 = ps->ring_vert_off[r], v1 = ps->ring_vert_off[r + 1];
    RingDev& rd = rings[r];
    rd.minx = rd.miny = INFINITY;
    rd.maxx = rd.maxy = -INFINITY;
    for (int v = v0; v < v1; ++v) {
      rd.minx = std::min(rd.minx, vx[v]); rd.maxx = std::max(rd.maxx, vx[v]);
      rd.miny = std::min(rd.miny, vy[v]); rd.maxy = std::max(rd.maxy, vy[v]);
    }
    for (int i = v0 + 1; i < v1; ++i) segs[i] = Edge{vx[i], vy[i], vx[i - 1], vy[i - 1]};
    const int nseg = std::max(0, v1 - v0 - 1);
    int ns = std::max(1, std::min(4096, nseg / 2));
    const double hgt = rd.maxy - rd.miny;
    if (!(hgt > 0.0) || nseg == 0) ns = 1;
    rd.y0 = nseg ? rd.miny : 0.0;
    rd.inv_h = (ns > 1) ? (double)ns / hgt : 0.0;
    rd.ns = ns;
    int64_t ne = 0;   // (segment, slab) pairs of the ring
    for (int i = v0 + 1; i < v1; ++i) {
      int s0, s1;
      slab_range(rd, i, s0, s1);
      ne += s1 - s0 + 1;
    }
    ring_edge_base[r + 1] = ne;
    ring_slab_base[r + 1] = ns;
  };
  parallel_for(n_rings, ring_env);
  for (int r = 0; r < n_rings; ++r) {
    ring_slab_base[r + 1] += ring_slab_base[r];
    ring_edge_base[r + 1] += ring_edge_base[r];
    rings[r].slab_base = (int32_t)ring_slab_base[r];
  }
  slab_off.assign((size_t)ring_slab_base[n_rings] + 1, 0);
  slab_edges.assign((size_t)ring_edge_base[n_rings], Edge{});
  auto ring_fill = [&](int r) {
    const int v0 = ps->ring_vert_off[r], v1 = ps->ring_vert_off[r + 1];
    const RingDev& rd = rings[r];
    const int ns = rd.ns;
    int32_t* so = slab_off.data() + ring_slab_base[r];
    std::vector<int32_t> cnt((size_t)ns + 1, 0);
    for (int i = v0 + 1; i < v1; ++i) {
      int s0, s1;
      slab_range(rd, i, s0, s1);
      for (int k = s0; k <= s1; ++k) cnt[k + 1]++;
    }
    for (int k = 0; k < ns; ++k) cnt[k + 1] += cnt[k];
    for (int k = 0; k < ns; ++k) so[k] = (int32_t)(ring_edge_base[r] + cnt[k]);
    Edge* out = slab_edges.data() + ring_edge_base[r];
    for (int i = v0 + 1; i < v1; ++i) {   // segments in vertex order within each slab
      int s0, s1;
      slab_range(rd, i, s0, s1);
      for (int k = s0; k <= s1; ++k) out[cnt[k]++] = segs[i];
    }
  };
  parallel_for(n_rings, ring_fill);
  slab_off[(size_t)ring_slab_base[n_rings]] = (int32_t)slab_edges.size();

  // ---- polygon envelopes (JTS: Polygon envelope = shell envelope; MultiPolygon = union)
  plan.env.assign((size_t)std::max(P, 1) * 4, 0.0);
  double* G = plan.G;
  G[0] = G[1] = INFINITY;
  G[2] = G[3] = -INFINITY;
  for (int p = 0; p < P; ++p) {
    double e[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (int q = ps->poly_part_off[p]; q < ps->poly_part_off[p + 1]; ++q) {
      const int r0 = ps->part_ring_off[q];
      if (ps->part_ring_off[q + 1] <= r0) continue;
      const RingDev& rd = rings[r0];
      e[0] = std::min(e[0], rd.minx); e[1] = std::min(e[1], rd.miny);
      e[2] = std::max(e[2], rd.maxx); e[3] = std::max(e[3], rd.maxy);
    }
    memcpy(&plan.env[4 * (size_t)p], e, sizeof e);
    if (e[0] <= e[2]) {
      G[0] = std::min(G[0], e[0]); G[1] = std::min(G[1], e[1]);
      G[2] = std::max(G[2], e[2]); G[3] = std::max(G[3], e[3]);
    }
  }
  const bool any = G[0] <= G[2];
  if (!any) { G[0] = G[1] = 0.0; G[2] = G[3] = -1.0; }  // nothing can match

  // ---- grid: ~cells_per_poly cells per polygon over the set's envelope
  const double W = any ? G[2] - G[0] : 0.0, H = any ? G[3] - G[1] : 0.0;
  const int64_t cells_per_poly = cells_per_poly_in > 0 ? cells_per_poly_in : 16384;
  int64_t target = std::min<int64_t>(std::max<int64_t>((int64_t)P * cells_per_poly, 64), (int64_t)1 << GM_MAX_CELLS_LOG);
  int gx = 1, gy = 1;
  const bool degenerate = !(W > 0 && H > 0);
  if (!degenerate) {
    gx = (int)std::max<double>(1.0, std::floor(std::sqrt((double)target * W / H)));
    gy = (int)std::max<int64_t>(1, target / gx);
  }
  plan.any = any;
  plan.degenerate = degenerate;
  plan.gx = gx;
  plan.gy = gy;
  plan.gxc = (gx + (1 << CF_LOG) - 1) >> CF_LOG;
  plan.inv_cw = degenerate ? 0.0 : (double)gx / W;
  plan.inv_ch = degenerate ? 0.0 : (double)gy / H;
  plan.epsx = W > 0 ? W * 1e-9 : 1e-9;
  plan.epsy = H > 0 ? H * 1e-9 : 1e-9;
  plan.ncell = (int64_t)gx * gy;
}

// ------------------------------------------------------------------ the host classification
struct BandSeg {
  int32_t seg;   // global vertex id of the segment end (segment = v[seg-1] -> v[seg])
  double minx, maxx, ymin, ymax;
  int32_t vmin, vmax;  // vertex ids holding ymin / ymax
};

// breakpoints of a cell: y values of right-of-cell segment end points inside (yb0, yb1], ascending, unique
inline void collect_breakpoints(const std::vector<const BandSeg*>& right, double yb0, double yb1,
                                std::vector<std::pair<double, int32_t>>& bk) {
  bk.clear();
  for (const BandSeg* sg : right) {
    if (sg->ymin > yb0 && sg->ymin <= yb1) bk.push_back({sg->ymin, sg->vmin});
    if (sg->ymax > yb0 && sg->ymax <= yb1) bk.push_back({sg->ymax, sg->vmax});
  }
  std::sort(bk.begin(), bk.end(),
            [](const std::pair<double, int32_t>& x, const std::pair<double, int32_t>& y) { return x.first < y.first; });
  bk.erase(std::unique(bk.begin(), bk.end(),
                       [](const std::pair<double, int32_t>& x, const std::pair<double, int32_t>& y) {
                         return x.first == y.first;
                       }),
           bk.end());
}

// parity of right-of-cell segments straddling y (ymin <= y < ymax) at each breakpoint interval's left end
inline uint64_t right_parity(const std::vector<const BandSeg*>& right, double yb0,
                             const std::vector<std::pair<double, int32_t>>& bk) {
  uint64_t parity = 0;
  for (size_t j = 0; j <= bk.size(); ++j) {
    const double yk = j == 0 ? yb0 : bk[j - 1].first;
    int c = 0;
    for (const BandSeg* sg : right) c += (sg->ymin <= yk && yk < sg->ymax);
    if (c & 1) parity |= 1ull << j;
  }
  return parity;
}

// index arrays 3-7 and the counters, as the host build leaves them
struct HostCells {
  std::vector<uint32_t> cell_word, coarse_word, list_ent;
  std::vector<double> compact, blob;
  int64_t stat[ST_COUNT] = {};
  int rc = GM_OK;               // GM_E_CAPACITY: `error` says which capacity (the caller reports it)
  const char* error = nullptr;
  double t_classify = 0, t_merge = 0;   // now_s() at the end of those phases (GM_PIP_DEBUG)
};

struct Ent { int64_t cell; uint32_t e; };
struct ChunkOut {
  std::vector<Ent> ents;
  std::vector<double> blob;      // 8-byte words; each blob starts 16-byte aligned (even length kept)
  std::vector<double> compact;   // 16-word (128-B) compact blobs
  int64_t n_slow = 0, n_boundary = 0, n_records = 0, n_compact = 0;
};
struct RingRef { int32_t ring; bool shell; };
constexpr int PCH = 4;   // polygons per work item
struct Scratch {   // a thread's working vectors, kept across its chunks
  std::vector<RingRef> ring_list;
  std::vector<std::vector<BandSeg>> band;  // per ring of the polygon, segments meeting the row band
  std::vector<int32_t> a_edges;
  std::vector<const BandSeg*> right;
  std::vector<std::pair<double, int32_t>> bk;
};

// (cell, polygon) classification + boundary blobs of the polygons of chunk ch.  The entries carry
// chunk-local blob / compact offsets
inline void classify_chunk(const gm_polyset* ps, const BuildPlan& plan, int ch, Scratch& t, ChunkOut& o) {
  const int P = ps->n_polys;
  const double* vx = ps->vx;
  const double* vy = ps->vy;
  const double* G = plan.G;
  const double inv_cw = plan.inv_cw, inv_ch = plan.inv_ch, epsx = plan.epsx, epsy = plan.epsy;
  const int gx = plan.gx, gy = plan.gy;
  const bool degenerate = plan.degenerate;
  auto& [ring_list, band, a_edges, right, bk] = t;
  std::vector<Ent>& ents = o.ents;
  std::vector<double>& blob = o.blob;
  std::vector<double>& compact = o.compact;
  auto put_i32x2 = [&](int32_t a, int32_t b) {
    double w; int32_t v[2] = {a, b}; memcpy(&w, v, 8); blob.push_back(w);
  };
  auto put_u64 = [&](uint64_t u) { double w; memcpy(&w, &u, 8); blob.push_back(w); };
  for (int p = ch * PCH; p < std::min(P, (ch + 1) * PCH); ++p) {
    const double* e = &plan.env[4 * (size_t)p];
    if (!(e[0] <= e[2])) continue;
    ring_list.clear();
    for (int q = ps->poly_part_off[p]; q < ps->poly_part_off[p + 1]; ++q)
      for (int r = ps->part_ring_off[q]; r < ps->part_ring_off[q + 1]; ++r)
        ring_list.push_back(RingRef{r, r == ps->part_ring_off[q]});
    const int nr = (int)ring_list.size();
    band.resize((size_t)nr);
    const int cx0 = cell_of(e[0], G[0], inv_cw, gx), cx1 = cell_of(e[2], G[0], inv_cw, gx);
    const int cy0 = cell_of(e[1], G[1], inv_ch, gy), cy1 = cell_of(e[3], G[1], inv_ch, gy);
    for (int cy = cy0; cy <= cy1; ++cy) {
      const double yb0 = degenerate ? -INFINITY : G[1] + (double)cy / inv_ch - epsy;
      const double yb1 = degenerate ? INFINITY : G[1] + (double)(cy + 1) / inv_ch + epsy;
      for (int k = 0; k < nr; ++k) {
        band[k].clear();
        const int r = ring_list[k].ring;
        for (int i = ps->ring_vert_off[r] + 1; i < ps->ring_vert_off[r + 1]; ++i) {
          const double ya = vy[i - 1], yb = vy[i];
          const double ymin = std::min(ya, yb), ymax = std::max(ya, yb);
          if (ymax < yb0 || ymin > yb1) continue;
          band[k].push_back(BandSeg{i, std::min(vx[i - 1], vx[i]), std::max(vx[i - 1], vx[i]), ymin, ymax,
                                    ya <= yb ? i - 1 : i, ya <= yb ? i : i - 1});
        }
      }
      int run_loc = -1;
      for (int cx = cx0; cx <= cx1; ++cx) {
        const int64_t cell = (int64_t)cy * gx + cx;
        const double xb0 = degenerate ? -INFINITY : G[0] + (double)cx / inv_cw - epsx;
        const double xb1 = degenerate ? INFINITY : G[0] + (double)(cx + 1) / inv_cw + epsx;
        bool bnd = degenerate;
        for (int k = 0; k < nr && !bnd; ++k)
          for (const BandSeg& sg : band[k])
            if (sg.maxx >= xb0 && sg.minx <= xb1) { bnd = true; break; }
        if (!bnd) {
          if (run_loc < 0) {
            // any point of the cell: its nominal centre, checked to map back to the cell
            const double cxm = G[0] + ((double)cx + 0.5) / inv_cw;
            const double cym = G[1] + ((double)cy + 0.5) / inv_ch;
            if (cell_of(cxm, G[0], inv_cw, gx) != cx || cell_of(cym, G[1], inv_ch, gy) != cy) bnd = true;
            else run_loc = locate_poly(ps, p, cxm, cym);
          }
          if (!bnd) {
            if (run_loc == LOC_EXTERIOR) continue;
            if (run_loc == LOC_INTERIOR) {
              ents.push_back(Ent{cell, (CELL_INTERIOR << 30) | (uint32_t)p});
              continue;
            }
            bnd = true;  // a boundary location cannot occur in a segment-free cell; stay exact anyway
          }
        }
        run_loc = -1;
        // ---- compact blob: single-ring polygon, <= 2 segments, <= 4 breakpoints -> one 128-B line
        if (nr == 1 && !degenerate) {
          a_edges.clear(); right.clear(); bk.clear();
          for (const BandSeg& sg : band[0]) {
            if (sg.maxx >= xb0 && sg.minx <= xb1) a_edges.push_back(sg.seg);
            else if (sg.minx > xb1) right.push_back(&sg);
          }
          collect_breakpoints(right, yb0, yb1, bk);
          if (4 * a_edges.size() + bk.size() <= 30) {
            const int E = (int)a_edges.size(), B = (int)bk.size();
            const int lines = (4 * E + B <= 14 && E <= 3) ? 1 : 2;
            const uint64_t ci = compact.size() / 16;   // chunk-local line index
            double rec[32];
            for (double& w : rec) w = INFINITY;
            { int32_t v[2] = {p, E | (lines << 8)}; memcpy(&rec[0], v, 8); }
            { const uint64_t par = right_parity(right, yb0, bk); memcpy(&rec[1], &par, 8); }
            bool used[32] = {};
            used[0] = used[1] = true;
            for (int j = 0; j < E; ++j) {
              const int32_t i = a_edges[j];
              double* eg = rec + cseg_word(j);
              eg[0] = vx[i]; eg[1] = vy[i]; eg[2] = vx[i - 1]; eg[3] = vy[i - 1];
              for (int q = 0; q < 4; ++q) used[cseg_word(j) + q] = true;
            }
            int w = 2;
            for (int j = 0; j < B; ++j) {
              while (used[w]) ++w;
              rec[w] = bk[j].first;
              used[w] = true;
            }
            compact.insert(compact.end(), rec, rec + 16 * lines);
            o.n_boundary++;
            o.n_compact++;
            ents.push_back(Ent{cell, (CELL_BOUNDARY << 30) | BLOB_COMPACT | (uint32_t)ci});
            continue;
          }
        }
        // ---- boundary blob
        if (blob.size() & 1) blob.push_back(0.0);
        const uint64_t boff = blob.size() / 2;   // chunk-local, 16-B units
        put_i32x2(p, nr);
        for (int k = 0; k < nr; ++k) {
          a_edges.clear(); right.clear(); bk.clear();
          for (const BandSeg& sg : band[k]) {
            if (sg.maxx >= xb0 && sg.minx <= xb1) a_edges.push_back(sg.seg);
            else if (sg.minx > xb1) right.push_back(&sg);
          }
          collect_breakpoints(right, yb0, yb1, bk);
          const int r = ring_list[k].ring;
          const bool slow = degenerate || a_edges.size() > 4096 || bk.size() > 63;
          RingHdr rh{};
          rh.flags = (int16_t)((ring_list[k].shell ? 1 : 0) | (slow ? 2 : 0));
          rh.n_edge = slow ? 0 : (int16_t)a_edges.size();
          rh.n_brk = slow ? 0 : (int16_t)bk.size();
          { double w; memcpy(&w, &rh, 8); blob.push_back(w); }
          uint64_t parity = 0;
          if (!slow) {
            parity = right_parity(right, yb0, bk);
          } else {
            o.n_slow++;
            parity = (uint32_t)r;
          }
          put_u64(parity);
          if (!slow) {
            for (int32_t i : a_edges) {
              blob.push_back(vx[i]); blob.push_back(vy[i]); blob.push_back(vx[i - 1]); blob.push_back(vy[i - 1]);
            }
            for (auto& b : bk) blob.push_back(b.first);
          }
          o.n_records++;
        }
        o.n_boundary++;
        ents.push_back(Ent{cell, (CELL_BOUNDARY << 30) | (uint32_t)boff});
      }
    }
  }
  if (blob.size() & 1) blob.push_back(0.0);
}

// (cell, polygon) classification + boundary blobs, in parallel over chunks of polygons; the chunks
// are concatenated in polygon order afterwards (so cell lists keep polygons ascending) and their
// offsets rebased.  Then the cell words, the lists and the coarse words.
inline HostCells classify(const gm_polyset* ps, const BuildPlan& plan) {
  HostCells hc;
  const int P = ps->n_polys;
  const int gx = plan.gx, gy = plan.gy;
  const int64_t ncell = plan.ncell;
  const int nchunks = (P + PCH - 1) / PCH;
  std::vector<ChunkOut> outs((size_t)std::max(nchunks, 1));
  std::atomic<int> next_chunk{0};
  auto work = [&]() {
    Scratch t;
    for (;;) {
      const int ch = next_chunk.fetch_add(1);
      if (ch >= nchunks || !plan.any) break;
      classify_chunk(ps, plan, ch, t, outs[(size_t)ch]);
    }
  };
  {
    const int nth = std::max(1, std::min(build_threads(), nchunks));
    std::vector<std::thread> th;
    for (int t = 1; t < nth; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
  }
  hc.t_classify = now_s();
  // concatenate the chunks in polygon order, rebasing blob / compact offsets
  std::vector<Ent> ents;
  std::vector<double>& blob = hc.blob;
  std::vector<double>& compact = hc.compact;
  {
    size_t ne = 0, nbw = 0, ncw = 0;
    for (const ChunkOut& o : outs) { ne += o.ents.size(); nbw += o.blob.size(); ncw += o.compact.size(); }
    if (nbw / 2 >= (size_t)BLOB_COMPACT || ncw / 16 >= (size_t)BLOB_COMPACT) {
      hc.error = "gm_pip_index_create: boundary blobs too large (lower cells_per_poly)";
      hc.rc = GM_E_CAPACITY;
      return hc;
    }
    ents.reserve(ne); blob.reserve(nbw); compact.reserve(ncw);
    for (ChunkOut& o : outs) {
      const uint32_t bb = (uint32_t)(blob.size() / 2), cb = (uint32_t)(compact.size() / 16);
      for (const Ent& en : o.ents) {
        uint32_t e = en.e;
        if ((e >> 30) == CELL_BOUNDARY) e += (e & BLOB_COMPACT) ? cb : bb;
        ents.push_back(Ent{en.cell, e});
      }
      blob.insert(blob.end(), o.blob.begin(), o.blob.end());
      compact.insert(compact.end(), o.compact.begin(), o.compact.end());
      hc.stat[ST_SLOW] += o.n_slow; hc.stat[ST_BOUNDARY] += o.n_boundary;
      hc.stat[ST_RECORDS] += o.n_records; hc.stat[ST_COMPACT] += o.n_compact;
      std::vector<Ent>().swap(o.ents); std::vector<double>().swap(o.blob); std::vector<double>().swap(o.compact);
    }
  }
  std::vector<int32_t> per_cell((size_t)ncell, 0), bnd_cell((size_t)ncell, 0);
  for (const Ent& en : ents) {
    per_cell[en.cell]++;
    if ((en.e >> 30) == CELL_BOUNDARY) bnd_cell[en.cell]++;
  }
  hc.t_merge = now_s();
  if (blob.empty()) blob.push_back(0.0);
  // ---- cell words: single entries inline, multi-entry cells through a list (polygons ascending)
  std::vector<uint32_t>& cell_word = hc.cell_word;
  std::vector<uint32_t>& list_ent = hc.list_ent;
  cell_word.assign((size_t)ncell, 0xffffffffu);
  {
    std::vector<int32_t> start((size_t)ncell + 1, 0);
    for (int64_t c = 0; c < ncell; ++c) start[c + 1] = start[c] + per_cell[c];
    std::vector<uint32_t> all(ents.size());
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (const Ent& en : ents) all[fill[en.cell]++] = en.e;
    for (int64_t c = 0; c < ncell; ++c) {
      const int k = per_cell[c];
      if (k == 1) cell_word[c] = all[start[c]];
      else if (k > 1) {
        // payload = (list offset / 4) << 4 | count (15 = long list: true count in the first slot);
        // lists start 16-B aligned so one uint4 load brings the first four slots
        while (list_ent.size() & 3) list_ent.push_back(0);
        const size_t off = list_ent.size() / 4;
        if (off + k + 1 >= ((size_t)1 << 26)) {
          hc.error = "gm_pip_index_create: cell lists too large";
          hc.rc = GM_E_CAPACITY;
          return hc;
        }
        cell_word[c] = (CELL_LIST << 30) | (uint32_t)(off << 4) | (uint32_t)std::min(k, LIST_LONG);
        if (k >= LIST_LONG) list_ent.push_back((uint32_t)k);
        for (int j = 0; j < k; ++j) list_ent.push_back(all[start[c] + j]);
      }
    }
  }
  while (list_ent.size() < 4 || (list_ent.size() & 3)) list_ent.push_back(0);
  // coarse words: EMPTY when every fine cell is empty, the fine word when all fine cells carry the
  // same INTERIOR word, otherwise CELL_LIST ("read the fine word")
  const int gxc = plan.gxc, gyc = (gy + (1 << CF_LOG) - 1) >> CF_LOG;
  hc.coarse_word.assign((size_t)gxc * gyc, 0xffffffffu);
  for (int yc = 0; yc < gyc; ++yc)
    for (int xc = 0; xc < gxc; ++xc) {
      uint32_t w = 0xffffffffu;
      bool first = true, mixed = false;
      for (int yy = yc << CF_LOG; yy < std::min(gy, (yc + 1) << CF_LOG) && !mixed; ++yy)
        for (int xx = xc << CF_LOG; xx < std::min(gx, (xc + 1) << CF_LOG); ++xx) {
          const uint32_t f = cell_word[(size_t)yy * gx + xx];
          if (first) { w = f; first = false; }
          else if (f != w) { mixed = true; break; }
        }
      const uint32_t kind = w >> 30;
      hc.coarse_word[(size_t)yc * gxc + xc] =
          (!mixed && (kind == CELL_EMPTY || kind == CELL_INTERIOR)) ? w : (CELL_LIST << 30);
    }
  hc.stat[ST_MAX_BND_PER_CELL] = ncell ? *std::max_element(bnd_cell.begin(), bnd_cell.end()) : 0;
  hc.stat[ST_MAX_ENT_PER_CELL] = ncell ? *std::max_element(per_cell.begin(), per_cell.end()) : 0;
  hc.stat[ST_ENTRIES] = (int64_t)ents.size();
  hc.stat[ST_CELLS] = ncell;
  hc.stat[ST_BLOB_BYTES] = (int64_t)(blob.size() + compact.size()) * 8;
  if (compact.empty()) compact.assign(16, 0.0);   // after the byte count: an index without compact blobs reports none
  return hc;
}

}  // namespace host
}  // namespace gm
