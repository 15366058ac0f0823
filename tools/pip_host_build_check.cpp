// pip_host_build_check.cpp -- host-only check of the polygon index's host build
// (geomesa_amd/csrc/gm_pip_build_host.hpp over gm_pip_layout.hpp): prepare() and classify() on a few
// tiny polygon sets, and the invariants of the arrays they return -- every reference inside its
// array, lists aligned and ascending, coarse words true to their fine cells, non-boundary entries
// agreeing with the point locator at the cell centre, counters equal to what the arrays hold.
// Prints "bad 0" on success.  Run with GM_BUILD_THREADS=4 for the threaded classification.
//   c++ -std=c++17 -pthread -o pip_host_build_check tools/pip_host_build_check.cpp && ./pip_host_build_check
#include <cstdio>
#include <string>

#include "../geomesa_amd/csrc/gm_pip_build_host.hpp"
#include "../geomesa_amd/csrc/gm_pip_layout.hpp"
#include "../include/geomesa_hip.h"

using namespace gm;

namespace {

typedef std::vector<std::pair<double, double>> Ring;
typedef std::vector<std::vector<Ring>> Polygon;   // parts of rings, shell first

struct PolySet {
  std::vector<int32_t> ppo{0}, pro{0}, rvo{0};
  std::vector<double> vx, vy;
  gm_polyset c{};
  explicit PolySet(const std::vector<Polygon>& polys) {
    for (const Polygon& poly : polys) {
      for (const std::vector<Ring>& part : poly) {
        for (Ring r : part) {
          if (!r.empty() && r.front() != r.back()) r.push_back(r.front());   // closed, as JTS LinearRing requires
          for (const auto& v : r) { vx.push_back(v.first); vy.push_back(v.second); }
          rvo.push_back((int32_t)vx.size());
        }
        pro.push_back((int32_t)rvo.size() - 1);
      }
      ppo.push_back((int32_t)pro.size() - 1);
    }
    c.n_polys = (int32_t)polys.size();
    c.poly_part_off = ppo.data(); c.part_ring_off = pro.data(); c.ring_vert_off = rvo.data();
    c.vx = vx.data(); c.vy = vy.data();
  }
};

Ring box(double x0, double y0, double x1, double y1) { return Ring{{x0, y0}, {x1, y0}, {x1, y1}, {x0, y1}}; }

int bad = 0;
std::string set_name;
#define EXPECT(cond, ...)                                   \
  do {                                                      \
    if (!(cond)) {                                          \
      if (++bad <= 20) {                                    \
        std::printf("%s: %s: ", set_name.c_str(), #cond);   \
        std::printf(__VA_ARGS__);                           \
        std::printf("\n");                                  \
      }                                                     \
    }                                                       \
  } while (0)

struct Tally {
  int64_t entries = 0, boundary = 0, compact = 0, records = 0, slow = 0, blob_words = 0, compact_words = 0;
};

// one INTERIOR / BOUNDARY entry of cell c: its references and records; returns its polygon (-1: broken)
int check_entry(const host::HostCells& hc, const host::BuildPlan& plan, const gm_polyset* ps, int64_t c, uint32_t e,
                Tally& t) {
  const uint32_t kind = e >> 30, ref = e & 0x3fffffffu;
  ++t.entries;
  if (kind == CELL_INTERIOR) {
    EXPECT((int)ref < ps->n_polys, "cell %lld polygon %u", (long long)c, ref);
    return (int)ref < ps->n_polys ? (int)ref : -1;
  }
  EXPECT(kind == CELL_BOUNDARY, "cell %lld entry kind %u", (long long)c, kind);
  if (kind != CELL_BOUNDARY) return -1;
  ++t.boundary;
  int32_t h[2];
  if (ref & BLOB_COMPACT) {
    const size_t w0 = 16 * (size_t)(ref & (BLOB_COMPACT - 1));
    EXPECT(w0 + 16 <= hc.compact.size(), "cell %lld compact line %zu of %zu words", (long long)c, w0 / 16, hc.compact.size());
    if (w0 + 16 > hc.compact.size()) return -1;
    memcpy(h, &hc.compact[w0], 8);
    const int E = h[1] & 0xff, lines = (h[1] >> 8) & 0xff;
    EXPECT((lines == 1 || lines == 2) && w0 + 16 * (size_t)lines <= hc.compact.size(), "cell %lld compact lines %d",
           (long long)c, lines);
    EXPECT(E <= CSEG_MAX && (E == 0 || cseg_word(E - 1) + 4 <= 16 * lines), "cell %lld compact segments %d in %d lines",
           (long long)c, E, lines);
    ++t.compact;
    t.compact_words += 16 * lines;
  } else {
    size_t w = 2 * (size_t)ref;
    EXPECT(w < hc.blob.size(), "cell %lld blob offset %zu of %zu words", (long long)c, w, hc.blob.size());
    if (w >= hc.blob.size()) return -1;
    memcpy(h, &hc.blob[w], 8);
    const size_t w0 = w++;
    for (int r = 0; r < h[1]; ++r) {
      EXPECT(w + 2 <= hc.blob.size(), "cell %lld ring record %d beyond the blob", (long long)c, r);
      if (w + 2 > hc.blob.size()) return -1;
      RingHdr rh;
      memcpy(&rh, &hc.blob[w], 8);
      ++t.records;
      if (rh.flags & 2) {
        ++t.slow;
        uint64_t ring;
        memcpy(&ring, &hc.blob[w + 1], 8);
        EXPECT(rh.n_edge == 0 && rh.n_brk == 0 && ring < plan.rings.size(), "cell %lld slab-walk ring %llu", (long long)c,
               (unsigned long long)ring);
      }
      EXPECT(rh.n_edge >= 0 && rh.n_brk >= 0 && rh.n_brk <= 63, "cell %lld record %d: %d edges %d breakpoints", (long long)c,
             r, rh.n_edge, rh.n_brk);
      w += 2 + 4 * (size_t)rh.n_edge + (size_t)rh.n_brk;
    }
    EXPECT(w <= hc.blob.size(), "cell %lld blob ends at %zu of %zu words", (long long)c, w, hc.blob.size());
    t.blob_words += (int64_t)(((w - w0) + 1) & ~(size_t)1);   // blobs keep 16-byte alignment
  }
  EXPECT(h[0] >= 0 && h[0] < ps->n_polys, "cell %lld blob polygon %d", (long long)c, h[0]);
  return h[0] >= 0 && h[0] < ps->n_polys ? h[0] : -1;
}

void check_set(const char* name, const std::vector<Polygon>& polys, int cells_per_poly) {
  set_name = std::string(name) + " @" + std::to_string(cells_per_poly);
  const PolySet set(polys);
  const gm_polyset* ps = &set.c;
  host::BuildPlan plan;
  host::prepare(ps, cells_per_poly, plan);
  const host::HostCells hc = host::classify(ps, plan);
  EXPECT(hc.rc == GM_OK, "classify returned %d (%s)", hc.rc, hc.error ? hc.error : "");
  if (hc.rc) return;
  const int gx = plan.gx, gy = plan.gy, P = ps->n_polys;
  const int64_t ncell = (int64_t)gx * gy;
  EXPECT(plan.ncell == ncell && (int64_t)hc.cell_word.size() == ncell, "%lld cells, %zu cell words", (long long)ncell,
         hc.cell_word.size());
  EXPECT(plan.rings.size() == (size_t)set.rvo.size() - 1 && plan.slab_off.back() == (int32_t)plan.slab_edges.size(),
         "rings %zu, slab_off ends at %d of %zu edges", plan.rings.size(), plan.slab_off.back(), plan.slab_edges.size());
  EXPECT(hc.list_ent.size() >= 4 && hc.list_ent.size() % 4 == 0, "list_ent has %zu slots", hc.list_ent.size());
  Tally t;
  int64_t max_ent = 0, max_bnd = 0;
  size_t next_list = 0;   // lists follow one another, each from a multiple of 4
  std::vector<int8_t> kind_of((size_t)std::max(P, 1));   // per polygon, this cell's entry: -1 none, else the kind
  for (int64_t c = 0; c < ncell; ++c) {
    const uint32_t w = hc.cell_word[(size_t)c];
    std::fill(kind_of.begin(), kind_of.end(), (int8_t)-1);
    int64_t n_ent = 0, n_bnd = 0;
    auto entry = [&](uint32_t e, int prev) {
      const int p = check_entry(hc, plan, ps, c, e, t);
      if (p >= 0) kind_of[(size_t)p] = (int8_t)(e >> 30);
      EXPECT(p > prev, "cell %lld: polygon %d after %d", (long long)c, p, prev);
      ++n_ent;
      n_bnd += (e >> 30) == CELL_BOUNDARY;
      return p;
    };
    if ((w >> 30) == CELL_EMPTY) {
      EXPECT(w == 0xffffffffu, "cell %lld EMPTY word %08x", (long long)c, w);
    } else if ((w >> 30) == CELL_LIST) {
      const size_t off = 4 * (size_t)((w & 0x3fffffffu) >> 4);
      size_t k = w & 15u, q = off;
      EXPECT(off == next_list && off < hc.list_ent.size(), "cell %lld list at %zu, expected %zu", (long long)c, off, next_list);
      if (off >= hc.list_ent.size()) continue;
      if (k == (size_t)LIST_LONG) {
        k = hc.list_ent[q++];
        EXPECT(k >= (size_t)LIST_LONG, "cell %lld long list counts %zu", (long long)c, k);
      }
      EXPECT(k >= 2 && q + k <= hc.list_ent.size(), "cell %lld list of %zu at %zu of %zu", (long long)c, k, q,
             hc.list_ent.size());
      if (q + k > hc.list_ent.size()) continue;
      int prev = -1;
      for (size_t j = 0; j < k; ++j) prev = entry(hc.list_ent[q + j], prev);
      next_list = (q + k + 3) & ~(size_t)3;
      for (size_t j = q + k; j < next_list && j < hc.list_ent.size(); ++j)
        EXPECT(hc.list_ent[j] == 0u, "cell %lld list padding %08x", (long long)c, hc.list_ent[j]);
    } else {
      entry(w, -1);
    }
    max_ent = std::max(max_ent, n_ent);
    max_bnd = std::max(max_bnd, n_bnd);
    // the locator at the cell centre: INTERIOR entries inside, polygons without an entry outside
    if (!plan.degenerate) {
      const int cx = (int)(c % gx), cy = (int)(c / gx);
      const double cxm = plan.G[0] + ((double)cx + 0.5) / plan.inv_cw, cym = plan.G[1] + ((double)cy + 0.5) / plan.inv_ch;
      for (int p = 0; p < P; ++p) {
        if (kind_of[(size_t)p] == (int8_t)CELL_BOUNDARY) continue;
        const int loc = host::locate_poly(ps, p, cxm, cym);
        const int want = kind_of[(size_t)p] < 0 ? LOC_EXTERIOR : LOC_INTERIOR;
        EXPECT(loc == want, "cell %lld polygon %d: centre located %d, entry says %d", (long long)c, p, loc, want);
      }
    } else {
      EXPECT(n_ent == n_bnd, "cell %lld: a degenerate grid holds boundary entries only", (long long)c);
    }
  }
  // coarse words
  const int gxc = plan.gxc, gyc = (gy + (1 << CF_LOG) - 1) >> CF_LOG;
  EXPECT(gxc == (gx + (1 << CF_LOG) - 1) >> CF_LOG && hc.coarse_word.size() == (size_t)gxc * gyc, "%d x %d coarse cells, %zu words",
         gxc, gyc, hc.coarse_word.size());
  if (hc.coarse_word.size() == (size_t)gxc * gyc)
    for (int yc = 0; yc < gyc; ++yc)
      for (int xc = 0; xc < gxc; ++xc) {
        const uint32_t cw = hc.coarse_word[(size_t)yc * gxc + xc], f0 = hc.cell_word[(size_t)(yc << CF_LOG) * gx + (xc << CF_LOG)];
        bool same = true;
        for (int yy = yc << CF_LOG; yy < std::min(gy, (yc + 1) << CF_LOG); ++yy)
          for (int xx = xc << CF_LOG; xx < std::min(gx, (xc + 1) << CF_LOG); ++xx) same &= hc.cell_word[(size_t)yy * gx + xx] == f0;
        const bool uniform = same && ((f0 >> 30) == CELL_EMPTY || (f0 >> 30) == CELL_INTERIOR);
        EXPECT(cw == (uniform ? f0 : (CELL_LIST << 30)), "coarse cell (%d, %d) word %08x over fine %08x (%s)", xc, yc, cw, f0,
               same ? "uniform" : "mixed");
      }
  // counters
  const int64_t want[ST_COUNT] = {ncell, t.entries, t.boundary, t.records, t.slow,
                                  (std::max<int64_t>(t.blob_words, 1) + t.compact_words) * 8, t.compact, max_bnd, max_ent};
  static const char* const names[ST_COUNT] = {"cells", "entries", "boundary", "records", "slow", "blob_bytes", "compact",
                                              "max_bnd_per_cell", "max_ent_per_cell"};
  for (int k = 0; k < ST_COUNT; ++k)
    EXPECT(hc.stat[k] == want[k], "counter %s = %lld, the arrays hold %lld", names[k], (long long)hc.stat[k], (long long)want[k]);
  EXPECT((int64_t)hc.blob.size() == std::max<int64_t>(t.blob_words, 1), "blob has %zu words, its records %lld", hc.blob.size(),
         (long long)t.blob_words);
  EXPECT((int64_t)hc.compact.size() == std::max<int64_t>(t.compact_words, 16), "compact has %zu words, its records %lld",
         hc.compact.size(), (long long)t.compact_words);
  std::printf("%-34s %4d x %-4d cells  %7lld entries  %6lld boundary (%lld compact)  %5lld records (%lld slow)  lists %zu\n",
              set_name.c_str(), gx, gy, (long long)t.entries, (long long)t.boundary, (long long)t.compact, (long long)t.records,
              (long long)t.slow, hc.list_ent.size());
}

}  // namespace

int main() {
  // shell (0,0)-(34,18) with 512 square holes of side 0.5 centred in the unit cells of a 32 x 16 lattice:
  // one ring more than the device build takes
  std::vector<Ring> lattice{box(0, 0, 34, 18)};
  for (int k = 0; k < 512; ++k) lattice.push_back(box(1.25 + k % 32, 1.25 + k / 32, 1.75 + k % 32, 1.75 + k / 32));
  // twenty squares over one another, each shifted a little: long cell lists, five chunks of polygons
  std::vector<Polygon> stack;
  for (int k = 0; k < 20; ++k) stack.push_back(Polygon{{box(0.01 * k, 0.02 * k, 3 + 0.01 * k, 3 + 0.02 * k)}});
  // six squares with a hole each, side by side: generic blobs from more than one chunk of polygons
  std::vector<Polygon> holed;
  for (int k = 0; k < 6; ++k) holed.push_back(Polygon{{box(5 * k, 0, 5 * k + 4, 3), box(5 * k + 1, 1, 5 * k + 2.5, 2)}});
  for (int cells : {0, 512}) {
    check_set("square with a hole", {Polygon{{box(0, 0, 4, 3), box(1, 1, 2.5, 2)}}}, cells);
    check_set("two squares sharing an edge", {Polygon{{box(0, 0, 2, 2)}}, Polygon{{box(2, 0, 4, 2)}}}, cells);
    check_set("513 rings", {Polygon{lattice}}, cells);
  }
  check_set("six squares with holes", holed, 512);
  check_set("twenty stacked squares", stack, 64);
  check_set("twenty stacked squares", stack, 512);
  check_set("zero height", {Polygon{{Ring{{0, 0}, {1, 0}, {2, 0}}}}}, 0);
  check_set("zero width", {Polygon{{Ring{{0, 0}, {0, 1}, {0, 2}}}}}, 0);
  check_set("three equal points", {Polygon{{Ring{{1, 1}, {1, 1}, {1, 1}}}}}, 0);
  check_set("no polygons", {}, 0);
  check_set("polygons without rings", {Polygon{}, Polygon{{}}}, 0);
  check_set("an empty polygon beside a square", {Polygon{}, Polygon{{box(0, 0, 4, 3)}}}, 0);
  std::printf("bad %d\n", bad);
  return bad != 0;
}
