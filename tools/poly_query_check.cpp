// poly_query_check.cpp -- runs the query-polygon builder of gm_table_scan_geom (csrc/gm_poly_query_host.hpp,
// plain C++) on polygon sets read from a text file and prints what it built, for
// tests/test_geom_poly_reference.py to hold against its own restatement.
//
// Input, whitespace separated: the number of sets; per set the number of parts; per part the number of
// rings; per ring the number of tuples and then x y pairs (strtod: hexadecimal floats are exact).  Every
// part is a polygon of its own.  Output per set: "invalid <text>" or "set <parts> <edges> <slabs>
// <entries>", then one line per slab with the ring-order index of each entry's edge, then "parts" and one
// line per part: its envelope and first shell vertex (%a).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../geomesa_amd/csrc/gm_poly_query_host.hpp"

static bool next(FILE* f, double& v) {
  char tok[64];
  if (fscanf(f, "%63s", tok) != 1) return false;
  v = strtod(tok, nullptr);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s FILE\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return perror(argv[1]), 2;
  double v;
  if (!next(f, v)) return 2;
  const int nsets = (int)v;
  for (int s = 0; s < nsets; ++s) {
    std::vector<int32_t> ppo{0}, pro{0}, rvo{0};
    std::vector<double> vx, vy;
    if (!next(f, v)) return 2;
    const int np = (int)v;
    for (int p = 0; p < np; ++p) {
      if (!next(f, v)) return 2;
      const int nr = (int)v;
      for (int r = 0; r < nr; ++r) {
        if (!next(f, v)) return 2;
        const int n = (int)v;
        for (int i = 0; i < n; ++i) {
          double x, y;
          if (!next(f, x) || !next(f, y)) return 2;
          vx.push_back(x);
          vy.push_back(y);
        }
        rvo.push_back((int32_t)vx.size());
      }
      pro.push_back((int32_t)rvo.size() - 1);
      ppo.push_back((int32_t)pro.size() - 1);
    }
    const gm_polyset ps{np, ppo.data(), pro.data(), rvo.data(), vx.data(), vy.data()};
    if (const char* bad = gm::polyq::validate(&ps)) {
      printf("invalid %s\n", bad);
      continue;
    }
    gm::polyq::HostQuery q;
    gm::polyq::build(&ps, q);
    printf("set %d %d %d %lld\n", q.n_parts, q.n_edges, q.ns, (long long)q.entries());
    for (int k = 0; k < q.ns; ++k) {
      for (int32_t e = q.soff[k]; e < q.soff[k + 1]; ++e) {
        // an entry carries its edge's own coordinates, ring and part
        const int32_t v0 = q.eid[e] + q.ering[e];   // ring r's edges start r tuples behind its vertices
        const int32_t r = q.ering[e], p = q.epart[e] >> 1;
        if (r < 0 || r >= q.n_rings || p < 0 || p >= q.n_parts || v0 < rvo[r] || v0 + 1 >= rvo[r + 1] ||
            pro[p] > r || pro[p + 1] <= r || (q.epart[e] & 1) != (pro[p] == r) || q.edge[4 * e] != vx[v0] ||
            q.edge[4 * e + 1] != vy[v0] || q.edge[4 * e + 2] != vx[v0 + 1] || q.edge[4 * e + 3] != vy[v0 + 1])
          return printf("bad entry %d\n", e), 1;
        printf("%d%c", q.eid[e], e + 1 < q.soff[k + 1] ? ' ' : '\n');
      }
      if (q.soff[k] == q.soff[k + 1]) printf("\n");
    }
    printf("parts\n");
    for (int p = 0; p < q.n_parts; ++p)
      printf("%a %a %a %a %a %a\n", q.penv[4 * p], q.penv[4 * p + 1], q.penv[4 * p + 2], q.penv[4 * p + 3],
             q.pv0[2 * p], q.pv0[2 * p + 1]);
  }
  fclose(f);
  return 0;
}
