"""Times the entries that read a GM_GEOM_WKB column against the typed LineString column of the same
geometries and writes profiles/wkb_probe.json.

    python tools/wkb_probe.py [--n 6000000] [--out profiles/wkb_probe.json]
                              [--typed-ab parent=FILE,FILE tree=FILE,FILE]

n lines of 20 vertices (the shape of tools/density_lines_probe.py: a random walk; here every step is up to a
degree either way, so a line spans a few degrees and most of the envelopes that meet the 6 x 4 degree query
box are wider and taller than it: the exact filter has to walk them), built on the device twice: as a
LineString column ([x, y] tuples, int32 List offsets: 4 + 320 B per slot) and as a WKB column (little-endian
2-D blobs, 9 + 320 B per slot, so consecutive slots start at every residue mod 8).  int32 value offsets
bound a WKB column at 2^31 bytes, 6.5 M such slots; calls are repeated to pass half a second.  Timed on each, with device events after a warm-up call:
  gm_arrow_envelopes, gm_xz2_index_key_arrow (asynchronous forms), and XZ2Table.query(exact=True) of one box
  (events around the whole call, its host steps and count read-backs included),
beside gm_device_copy of the typed column's bytes in the same run.  Every row states its bytes read, GB/s
and the share of the copy rate; `ratio` is WKB time over typed time.  The results of the two columns are
compared (envelopes by bit pattern, keys, ids) before anything is written.

--typed-ab takes the outputs of tools/geom_scan_probe.py run on a build of the parent commit and on this
tree, back to back on one machine, and records the typed path's times of both."""
import argparse
import ctypes
import json
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geomesa_amd import _lib  # noqa: E402
from geomesa_amd import arrow as A  # noqa: E402
from geomesa_amd.table import XZ2Table  # noqa: E402

PER = 20
HEAD = 9                       # order byte, typeInt, count
BOX = (-10.0, 30.0, -4.0, 34.0)
P = _lib.ptr


def timed(f, floor_s=0.5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    first = e0.elapsed_time(e1)
    reps = max(3, int(math.ceil(floor_s * 1000.0 / max(first, 1e-3))))
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def make_lines(n, seed=11):
    """[x, y] tuples (n * PER, 2): random walks of PER vertices about uniform centres."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.rand((n, 1, 2), device="cuda", dtype=torch.float64, generator=g)
    c[..., 0] = c[..., 0] * 340 - 170
    c[..., 1] = c[..., 1] * 160 - 80
    step = (torch.rand((n, PER, 2), device="cuda", dtype=torch.float64, generator=g) - 0.5) * 2.0
    return (c + torch.cumsum(step, 1)).reshape(n * PER, 2).contiguous()


def column(kind, n, coords, offsets):
    """A GeometryColumn over buffers already on the device."""
    col = A.GeometryColumn.__new__(A.GeometryColumn)
    col.kind, col.n, col.flip_axis, col.ordinal_bits = kind, n, True, 64
    col._coords, col._valid, col._offs, col._voff = coords, None, [offsets], 0
    col._c = A.GeomColumnC(A.KINDS[kind], 64, 1, 0, coords.data_ptr(), None, 0,
                           (ctypes.c_void_p * 3)(offsets.data_ptr(), None, None))
    return col


def parse_geom_scan(path):
    """The per-call times a tools/geom_scan_probe.py output states."""
    text = open(path).read()
    a = re.search(r"\(a\) gm_table_scan\s+tree\s+ms per call, rounds: (.*)", text)
    b = re.search(r"\(b\) gm_table_scan_geom\s+ms per call, rounds: (.*)", text)
    bad = re.search(r"intersects_restated: (\d+) disagreements", text)
    return {"file": os.path.basename(path), "envelope_filter_ms": [float(v) for v in a.group(1).split()],
            "exact_filter_ms": [float(v) for v in b.group(1).split()], "disagreements": int(bad.group(1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wkb_probe.json"))
    ap.add_argument("--typed-ab", nargs="*", default=[])
    args = ap.parse_args()
    n = args.n
    assert n * (HEAD + PER * 16) < 2 ** 31, "int32 value offsets: at most 6.5 M slots of 329 B"
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle

    xy = make_lines(n)
    t_off = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * PER).to(torch.int32)
    blob = torch.empty((n, HEAD + PER * 16), dtype=torch.uint8, device="cuda")
    blob[:, :HEAD] = torch.tensor([1, 2, 0, 0, 0, PER, 0, 0, 0], dtype=torch.uint8, device="cuda")
    blob[:, HEAD:] = xy.view(torch.uint8).view(n, PER * 16)
    w_off = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * (HEAD + PER * 16)).to(torch.int32)
    cols = {"typed": column("linestring", n, xy, t_off), "wkb": column("wkb", n, blob, w_off)}
    read = {"typed": n * (4 + PER * 16), "wkb": n * (4 + HEAD + PER * 16)}      # offsets + slot bytes

    res = {"device": torch.cuda.get_device_name(0), "slots": n, "vertices_per_slot": PER, "box": BOX,
           "bytes_read_per_slot": {k: v // n for k, v in read.items()}, "rows": []}
    dst = torch.empty_like(xy)
    copy = lambda: _lib.check(lib.gm_device_copy(h, P(dst), P(xy), xy.numel() * 8), "gm_device_copy")  # noqa: E731
    copy()
    ms, reps = timed(copy)
    copy_gbs = 2.0 * xy.numel() * 8 / ms / 1e6
    res["copy"] = {"ms": round(ms, 4), "reps": reps, "gb_per_s": round(copy_gbs, 1), "bytes": "read + written"}
    del dst

    env = {k: torch.empty((4, n), dtype=torch.float64, device="cuda") for k in cols}
    key = {k: torch.empty(n, dtype=torch.int64, device="cuda") for k in cols}
    tables, ids = {}, {}

    def note(entry, kind, ms, reps, out_bytes):
        row = {"entry": entry, "column": kind, "ms": round(ms, 4), "reps": reps,
               "gb_per_s_read": round(read[kind] / ms / 1e6, 1),
               "share_of_copy_rate": round((read[kind] + out_bytes) / ms / 1e6 / copy_gbs, 3)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        return row

    for kind, col in cols.items():
        cs = ctypes.byref(col.c_struct())
        f = lambda: _lib.check(lib.gm_arrow_envelopes(h, cs, n, *[P(env[kind][k]) for k in range(4)]),  # noqa: E731
                               "gm_arrow_envelopes")
        f()
        note("gm_arrow_envelopes", kind, *timed(f), 32 * n)
        f = lambda: _lib.check(lib.gm_xz2_index_key_arrow(h, cs, n, 12, 1, P(key[kind]), None, None),  # noqa: E731
                               "gm_xz2_index_key_arrow")
        f()
        note("gm_xz2_index_key_arrow", kind, *timed(f), 8 * n)
    assert torch.equal(env["typed"].view(torch.int64), env["wkb"].view(torch.int64)), "envelopes differ"
    assert torch.equal(key["typed"], key["wkb"]), "keys differ"
    del env, key
    for kind, col in cols.items():
        tables[kind] = XZ2Table.from_geometries(col, kind, lenient=True)
        f = lambda: tables[kind].query([BOX], exact=True)  # noqa: E731
        ids[kind], nm, scanned = f()
        ms, reps = timed(f)
        e = tables[kind].env
        meets = ~((e[2] < BOX[0]) | (e[0] > BOX[2]) | (e[3] < BOX[1]) | (e[1] > BOX[3]) | (e[2] < e[0]))
        short = ((e[0] >= BOX[0]) & (e[2] <= BOX[2])) | ((e[1] >= BOX[1]) & (e[3] <= BOX[3]))   # BoxPred's shortcuts
        row = {"entry": "XZ2Table.query(exact=True)", "column": kind, "ms": round(ms, 4), "reps": reps,
               "matches": int(nm), "envelope_survivors": int(tables[kind].n_envelope), "scanned": int(scanned),
               "survivors_walked": int((meets & ~short).sum().item())}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    assert torch.equal(torch.sort(ids["typed"])[0], torch.sort(ids["wkb"])[0]), "query results differ"

    by = {(r["entry"], r["column"]): r["ms"] for r in res["rows"]}
    res["ratio_wkb_over_typed"] = {e: round(by[(e, "wkb")] / by[(e, "typed")], 3) for e, k in by if k == "wkb"}
    for spec in args.typed_ab:
        name, files = spec.split("=", 1)
        res.setdefault("typed_path_geom_scan_probe", {})[name] = [parse_geom_scan(f) for f in files.split(",")]
    print(json.dumps(res["ratio_wkb_over_typed"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
