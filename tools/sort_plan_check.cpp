// sort_plan_check -- prints the digit plan gm_sort_keys makes (plan_sort, gm_sort_plan.hpp) for each
// input line, so that tests/test_sort_plan.py can compare it with an independent restatement.
//
//   g++ -O2 -std=c++17 -o sort_plan_check tools/sort_plan_check.cpp && ./sort_plan_check < cases.txt
//
// stdin:  or_z or_bs and_z and_bs sharded n mode     (one case per line; 0x.. or decimal;
//                                                      bs = bin | shard << 16 of the caller's columns)
// stdout: prefix npre pw pofs0 pofs1 pofs2 pofs3 sq binhi lsd...   (one line per case)
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../geomesa_amd/csrc/gm_sort_plan.hpp"

int main() {
  char line[512];
  long lineno = 0;
  while (fgets(line, sizeof line, stdin)) {
    ++lineno;
    unsigned long long h[4];
    int sharded = 0, mode = 0;
    long long n = 0;
    char* p = line;
    char* e = nullptr;
    bool ok = true;
    for (int k = 0; k < 4 && ok; ++k) { h[k] = strtoull(p, &e, 0); ok = e != p; p = e; }
    if (ok) { sharded = (int)strtol(p, &e, 0); ok = e != p; p = e; }
    if (ok) { n = strtoll(p, &e, 0); ok = e != p; p = e; }
    if (ok) { mode = (int)strtol(p, &e, 0); ok = e != p; }
    if (!ok) {
      fprintf(stderr, "sort_plan_check: line %ld: expected or_z or_bs and_z and_bs sharded n mode\n", lineno);
      return 2;
    }
    const unsigned long long h_raw[4] = {h[0], h[1], h[2], h[3]};
    const gm::SortPlan s = gm::plan_sort(h_raw, sharded != 0, (int64_t)n, mode);
    printf("%d %d %d %d %d %d %d %d %" PRIu32, s.prefix ? 1 : 0, s.npre, s.pw, s.pofs[0], s.pofs[1], s.pofs[2], s.pofs[3],
           s.sq, s.binhi);
    for (int o : s.lsd) printf(" %d", o);
    printf("\n");
  }
  return 0;
}
