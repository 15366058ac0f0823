"""Times the attribute index table over resident columns and writes profiles/attr_table_probe.json.

In one process, over n rows (an int64 attribute with about 1M distinct values, the Z3 tier, generated points):
the streaming copy (gm_device_copy) as the rate everything is a share of; Z3Table construction (gm_z3_index_key +
gm_sort_keys) for the same points and one gm_sort_keys of (bin, z) as yardsticks; gm_attr_index_key,
gm_attr_sort and gm_attr_key_bytes; AttributeTable.query for an equality, a 1 %-of-values range (both with bbox
and during) and an unbounded scan; Z3Table.query with the same bbox and during.  Wall-clock around each call
with a device synchronise (the calls synchronise themselves), after one warm-up call.  No pass or fail
threshold: the file records what was found.

    python tools/attr_table_probe.py [--n 250000000] [--out profiles/attr_table_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geomesa_amd import _lib  # noqa: E402
from geomesa_amd import attribute as A  # noqa: E402
from geomesa_amd.keyspace import during  # noqa: E402
from geomesa_amd.table import Z3Table  # noqa: E402
from bench import SEED, T2020, T2021  # noqa: E402

P = _lib.ptr
DISTINCT = 1_000_000


def timed(f, reps=3):
    """(best ms of `reps` calls after one warm-up, the last result)."""
    out = f()
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_table_probe.json"))
    a = ap.parse_args()
    n = a.n
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    torch.manual_seed(SEED)
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    _lib.check(lib.gm_gen_points(h, SEED, n, 0, -180.0, 180.0, -90.0, 90.0, T2020, T2021, P(x), P(y), P(t)), "gm_gen_points")
    values = torch.empty(n, dtype=torch.int64, device="cuda")
    step = 1 << 26
    for lo in range(0, n, step):
        k = min(step, n - lo)
        values[lo:lo + k] = torch.randint(0, DISTINCT, (k,), dtype=torch.int64, device="cuda")
    res = {"n": n, "device": torch.cuda.get_device_name(0), "distinct_values": DISTINCT, "rows": []}

    def note(name, ms, **kw):
        row = dict(name=name, ms=round(ms, 3), rows_per_s=round(n / ms * 1e3), **kw)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        return ms

    scratch = torch.empty(n, dtype=torch.int64, device="cuda")
    ms, _ = timed(lambda: _lib.check(lib.gm_device_copy(h, P(scratch), P(values), n * 8), "gm_device_copy"))
    note("gm_device_copy 8 B rows", ms, gb_per_s=round(16 * n / ms / 1e6, 1))
    del scratch

    # yardsticks: the Z3 table of the same points, and its sort alone
    ms, z3 = timed(lambda: Z3Table.from_points(x, y, t), reps=2)
    note("Z3Table.from_points (gm_z3_index_key + gm_sort_keys)", ms)
    bins, z = z3.ks.sfc.index_keys(x, y, t)
    ob, oz, op = torch.empty_like(bins), torch.empty_like(z), torch.empty(n, dtype=torch.int64, device="cuda")
    sort_ms, _ = timed(lambda: _lib.check(lib.gm_sort_keys(h, None, P(bins), P(z), n, None, P(ob), P(oz), P(op)),
                                          "gm_sort_keys"), reps=2)
    note("gm_sort_keys (bin, z)", sort_ms)
    del ob, oz, op

    # the attribute table's entries, one at a time
    col = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, values.data_ptr(), None, None, 0)
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    rows = torch.empty(n, dtype=torch.int64, device="cuda")
    m = ctypes.c_int64()
    ms, _ = timed(lambda: _lib.check(lib.gm_attr_index_key(h, ctypes.byref(col), n, P(v), P(rows), ctypes.byref(m)),
                                     "gm_attr_index_key"))
    note("gm_attr_index_key int64, no nulls", ms)
    del rows
    sv, sb, st = torch.empty_like(v), torch.empty_like(bins), torch.empty_like(z)
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    attr_ms, _ = timed(lambda: _lib.check(lib.gm_attr_sort(h, None, P(v), P(bins), P(z), n, None, P(sv), P(sb), P(st), P(perm)),
                                          "gm_attr_sort"), reps=2)
    note("gm_attr_sort (v, bin, z)", attr_ms, sort_keys_calls=round(attr_ms / sort_ms, 2))
    pv = torch.empty(n, dtype=torch.int64, device="cuda")
    pp = torch.empty(n, dtype=torch.int64, device="cuda")
    ms, _ = timed(lambda: _lib.check(lib.gm_sort_keys(h, None, None, P(v), n, None, None, P(pv), P(pp)), "gm_sort_keys"), reps=2)
    note("gm_sort_keys (v alone): the primary pass without its gathers", ms)
    del pv, pp
    out = torch.empty((n, 27), dtype=torch.uint8, device="cuda")
    ms, _ = timed(lambda: _lib.check(lib.gm_attr_key_bytes(h, _lib.GM_ATTR_INT64, None, P(sv), _lib.GM_ATTR_TIER_Z3, P(sb),
                                                           P(st), n, P(out)), "gm_attr_key_bytes"))
    note("gm_attr_key_bytes 27 B rows", ms, gb_per_s=round((18 + 27) * n / ms / 1e6, 1))
    del out, v, sv, sb, st, perm, bins, z

    # queries through the two tables
    table = A.AttributeTable(values, "long", x=x, y=y, t_ms=t, tier="z3")
    box = [(-80.0, 30.0, -70.0, 40.0)]
    week = [during(T2020 + 10 * 86400000, T2020 + 17 * 86400000)]
    for name, bounds, bb, iv in (("equality + bbox + during", [(4242, True, 4242, True)], box, week),
                                 ("1 % of values + bbox + during", [(500000, True, 509999, True)], box, week),
                                 ("equality alone", [(4242, True, 4242, True)], None, None),
                                 ("unbounded", [], None, None)):
        ms, (ids, nm, ns) = timed(lambda: table.query(bounds, bb, iv))
        note("AttributeTable.query " + name, ms, n_match=nm, n_scanned=ns)
    ms, (ids, nm, ns) = timed(lambda: z3.query(box, week))
    note("Z3Table.query bbox + during (loose: Z3Filter only)", ms, n_match=nm, n_scanned=ns)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
