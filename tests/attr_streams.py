"""The stream-order cases of the four attribute-table entries (gm_attr_index_key, gm_attr_key_bytes, gm_attr_sort,
gm_attr_table_scan), added to the case table of tests/stream_order.py through its own add():
tests/test_gpu_streams.py then runs them with every other entry (held stream on a caller's stream and on
Context.owned, the shuffled table), and tests/test_abi.py finds every new symbol covered.  Imported by
tests/test_gpu_attr_table.py, which pytest collects before either of them.
"""
import ctypes
import functools

import numpy as np

import attr_ref as R
import stream_order as SO
from geomesa_amd import _lib

I16, I64, U8, U64, F64 = np.int16, np.int64, np.uint8, np.uint64, np.float64
N = 2 * 4096 + 5      # two blocks of the validity scan (FROWS = 4096) and an odd tail
VOFF = 3


def _key_cols(n, seed):
    """(shard, v, bin, t) with ties in every prefix: 4 shards, ~50 values, 2 bins, t from a small set or random."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << 63, 50, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    t = np.where(rng.random(n) < 0.5, rng.integers(0, 8, n), rng.integers(0, 1 << 62, n)).astype(I64)
    return (rng.integers(0, 4, n).astype(U8), vals[rng.integers(0, 50, n)], rng.choice([2296, 2297], n).astype(I16), t)


def table_order(sh, v, b, t):
    """The stable sort by (shard, v, bin as u16, t as u64): numpy.lexsort, last key first."""
    return np.lexsort((t.view(U64), b.view(np.uint16), v, sh))


def _index_key_case(scale):
    valid = np.random.default_rng(41).random(N) < 0.75

    def bitmap():
        bits = np.zeros(VOFF + N, U8)
        bits[VOFF:] = valid
        return np.packbits(bits, bitorder="little")

    def ins(seed):
        return {"values": np.random.default_rng(4100 + seed).integers(-(1 << 62), 1 << 62, N), "valid": bitmap()}

    def call(lib, h, p, host):
        host["col"] = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, p["values"].value, None, p["valid"].value, VOFF)
        host["n_rows"] = ctypes.c_int64(-7)
        return lib.gm_attr_index_key(h, ctypes.byref(host["col"]), N, p["v"], p["rows"], ctypes.byref(host["n_rows"]))

    def expect(O, d):
        rows = np.flatnonzero(valid).astype(I64)
        v = d["values"][rows].view(U64) ^ np.uint64(1 << 63)
        return {"dev": {"v": v, "rows": rows}, "host": {"n_rows": len(rows)}, "elems": v}
    return SO.Case(ins, {"v": 8 * N, "rows": 8 * N}, call, expect)


def _key_bytes_case(scale):
    n = 2 * 256 + 5       # k_attr_key_bytes: STPB = 256 rows per block

    def ins(seed):
        sh, v, b, t = _key_cols(n, 4200 + seed)
        return {"shard": sh, "v": v, "bin": b, "t": t}

    def call(lib, h, p, host):
        return lib.gm_attr_key_bytes(h, _lib.GM_ATTR_INT64, p["shard"], p["v"], _lib.GM_ATTR_TIER_Z3, p["bin"], p["t"], n,
                                     p["out"])

    def expect(O, d):
        rows = np.array([list(bytes([d["shard"][i]]) + format(int(d["v"][i]), "016x").encode() + b"\x00" +
                              R.tier_z3(d["bin"][i], d["t"][i])) for i in range(n)], U8)
        return {"dev": {"out": rows}, "elems": rows}
    return SO.Case(ins, {"out": n * 28}, call, expect)


def _sort_case(scale):
    n = N * scale

    def ins(seed):
        sh, v, b, t = _key_cols(n, 4300 + seed)
        return {"shard": sh, "v": v, "bin": b, "t": t}

    def call(lib, h, p, host):
        return lib.gm_attr_sort(h, p["shard"], p["v"], p["bin"], p["t"], n, p["shard_out"], p["v_out"], p["bin_out"],
                                p["t_out"], p["perm"])

    def expect(O, d):
        o = table_order(d["shard"], d["v"], d["bin"], d["t"])
        return {"dev": {"shard_out": d["shard"][o], "v_out": d["v"][o], "bin_out": d["bin"][o], "t_out": d["t"][o],
                        "perm": o.astype(I64)}, "elems": o.astype(I64)}
    return SO.Case(ins, {"shard_out": n, "v_out": 8 * n, "bin_out": 2 * n, "t_out": 8 * n, "perm": 8 * n}, call, expect)


def _scan_case(scale):
    """A sorted table is structural (the same keys in A and B); the decoy differs in perm and in the secondary
    filter's columns, so ids and the matches themselves differ."""
    n = N * scale
    box = np.array([-180.0, -90.0, 0.0, 90.0])

    @functools.lru_cache(maxsize=None)
    def table():
        sh, v, b, t = _key_cols(n, 4400)
        o = table_order(sh, v, b, t)
        sh, v, b, t = sh[o], v[o], b[o], t[o]
        rng = np.random.default_rng(44)
        arr = np.zeros(12 * scale, _lib.ATTR_RANGE_DTYPE)
        for k in range(len(arr)):
            i, j = sorted(rng.integers(0, n, 2))
            j = min(j, i + n // 8)
            s = sh[i]
            j = max(np.flatnonzero(sh[:j + 1] == s)[-1], i)
            arr[k] = (v[i], v[j], t.view(U64)[i], t.view(U64)[j], b.view(np.uint16)[i], b.view(np.uint16)[j], s, (0, 0, 0))
        return sh, v, b, t, arr

    def ins(seed):
        sh, v, b, t, _ = table()
        rng = np.random.default_rng(4500 + seed)
        return {"shard": sh, "v": v, "bin": b, "t": t, "perm": rng.permutation(n).astype(I64),
                "x": rng.uniform(-180, 180, n), "y": rng.uniform(-90, 90, n)}

    def call(lib, h, p, host):
        arr = table()[4]
        host["n_match"], host["n_scanned"] = ctypes.c_int64(-7), ctypes.c_int64(-7)
        f = _lib.ScanFilter()
        f.xmin, f.ymin, f.xmax, f.ymax = p["x"].value, p["y"].value, p["x"].value, p["y"].value
        f.boxes, f.n_boxes = box.ctypes.data, 1
        host["f"] = f
        return lib.gm_attr_table_scan(h, p["shard"], p["v"], p["bin"], p["t"], n, arr.ctypes.data, len(arr),
                                      ctypes.byref(f), p["perm"], p["ids"], n, ctypes.byref(host["n_match"]),
                                      ctypes.byref(host["n_scanned"]))

    def expect(O, d):
        sh, v, b, t, arr = table()
        cand = candidates(sh, v, b, t, arr)
        inside = (d["x"] >= box[0]) & (d["x"] <= box[2]) & (d["y"] >= box[1]) & (d["y"] <= box[3])
        keep = cand & inside[d["perm"]]
        ids = d["perm"][np.flatnonzero(keep)]
        assert n // 16 < len(ids) < n
        return {"dev": {"ids": ids}, "host": {"n_match": len(ids), "n_scanned": int(cand.sum())},
                "elems": np.where(keep, d["perm"], -1)[cand]}
    return SO.Case(ins, {"ids": 8 * n}, call, expect)


def candidates(sh, v, b, t, arr):
    """Rows inside any gm_attr_range row of arr: (shard, v, b, t) compared lexicographically, every field unsigned."""
    keys = list(zip(sh.tolist(), v.tolist(), b.view(np.uint16).tolist(), t.view(U64).tolist()))
    out = np.zeros(len(keys), bool)
    for r in arr:
        lo = (int(r["shard"]), int(r["v_lo"]), int(r["b_lo"]), int(r["t_lo"]))
        hi = (int(r["shard"]), int(r["v_hi"]), int(r["b_hi"]), int(r["t_hi"]))
        out |= np.fromiter((lo <= k <= hi for k in keys), bool, len(keys))
    return out


if "gm_attr_index_key" not in SO.TABLE:
    # include/geomesa_hip.h, the attribute index table section: "gm_attr_key_bytes only enqueues (asynchronous);
    # the other three synchronise the context stream"
    SO.add("gm_attr_index_key", "gm_attr_index_key", True, _index_key_case)
    SO.add("gm_attr_key_bytes", "gm_attr_key_bytes", False, _key_bytes_case)
    SO.add("gm_attr_sort", "gm_attr_sort", True, _sort_case)
    SO.add("gm_attr_table_scan", "gm_attr_table_scan", True, _scan_case)
