"""Times XZ2Table.query(polygons=...) -- INTERSECTS against query polygons, k_poly_refine -- beside the box
query of the exact box filter, and writes profiles/geom_poly_probe.json.

    python tools/geom_poly_probe.py [--n 6000000] [--out profiles/geom_poly_probe.json]

The table is tools/wkb_probe.py's: n lines of 20 vertices, random walks about uniform centres, as a typed
LineString column.  The queries, each timed with device events after a warm-up call (events around the
whole call, its host steps, the query's upload and the count read-backs included):
  box          the probe's box as a box: k_refine with BoxPred, the baseline;
  rect5        the same rectangle as a 5-tuple polygon;
  ring65       a 65-tuple polygon of the same envelope (an ellipse touching the box's four sides);
  ring1000     a 1,000-tuple polygon of the same envelope;
  large65      a 65-tuple ellipse 80 x 50 degrees about the box's centre: most survivors lie inside it and
               are decided by containment.
Each query is also run with exact=False over the same boxes (the parts' envelopes): `refine_ms` is the exact
query's time less that one's, what the geometry filter adds.  gm_device_copy of the column's bytes is timed
in the same run.  rect5's ids must equal box's, and a strided sample of every polygon query is held to
tests/geom_poly_ref.intersects_restated, before anything is written."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from geomesa_amd import _lib  # noqa: E402
from geomesa_amd.table import XZ2Table  # noqa: E402
from wkb_probe import BOX, PER, column, make_lines, timed  # noqa: E402

P = _lib.ptr


def ellipse(m, a, b):
    """A closed ring of m tuples on the ellipse of half-axes a, b about the box's centre; its four extreme
    points are among them, exactly, so a = 3, b = 2 gives the box's own envelope."""
    cx, cy = (BOX[0] + BOX[2]) / 2, (BOX[1] + BOX[3]) / 2
    k = m - 1 - 4
    th = {0.0: (cx + a, cy), 0.5: (cx, cy + b), 1.0: (cx - a, cy), 1.5: (cx, cy - b)}
    for i in range(k):
        t = 2.0 * (i + 0.37) / k
        th[t] = (cx + a * math.cos(math.pi * t), cy + b * math.sin(math.pi * t))
    pts = [th[t] for t in sorted(th)]
    assert len(pts) == m - 1
    return pts + [pts[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_poly_probe.json"))
    args = ap.parse_args()
    n = args.n
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    xy = make_lines(n)
    off = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * PER).to(torch.int32)
    tb = XZ2Table.from_geometries(column("linestring", n, xy, off), "linestring", lenient=True)

    res = {"device": torch.cuda.get_device_name(0), "slots": n, "vertices_per_slot": PER, "box": BOX, "rows": []}
    dst = torch.empty_like(xy)
    copy = lambda: _lib.check(lib.gm_device_copy(h, P(dst), P(xy), xy.numel() * 8), "gm_device_copy")  # noqa: E731
    copy()
    ms, reps = timed(copy)
    res["copy"] = {"ms": round(ms, 4), "reps": reps, "gb_per_s": round(2.0 * xy.numel() * 8 / ms / 1e6, 1),
                   "bytes": "read + written"}
    del dst

    hw, hh = (BOX[2] - BOX[0]) / 2, (BOX[3] - BOX[1]) / 2
    rect = [(BOX[0], BOX[1]), (BOX[2], BOX[1]), (BOX[2], BOX[3]), (BOX[0], BOX[3]), (BOX[0], BOX[1])]
    queries = [("box", None), ("rect5", rect), ("ring65", ellipse(65, hw, hh)), ("ring1000", ellipse(1000, hw, hh)),
               ("large65", ellipse(65, 40.0, 25.0))]
    import geom_poly_ref as G
    ids = {}
    for name, ring in queries:
        if ring is None:
            boxes = [BOX]
            f = lambda: tb.query(boxes)  # noqa: E731
        else:
            xs, ys = [p[0] for p in ring], [p[1] for p in ring]
            boxes = [(min(xs), min(ys), max(xs), max(ys))]
            f = lambda: tb.query(polygons=[[[ring]]])  # noqa: E731
        got, nm, scanned = f()
        ids[name] = torch.sort(got)[0]
        n_env = tb.n_envelope
        ms, reps = timed(f)
        env_ms, _ = timed(lambda: tb.query(boxes, exact=False))
        row = {"query": name, "ring_tuples": len(ring) if ring else None, "envelope": boxes[0], "ms": round(ms, 4),
               "reps": reps, "envelope_filter_ms": round(env_ms, 4), "refine_ms": round(ms - env_ms, 4),
               "matches": int(nm), "envelope_survivors": int(n_env), "scanned": int(scanned)}
        if ring is not None:      # a strided sample of the survivors' neighbourhood against the reference
            q = G.Query([[ring]])
            e = [c.cpu().numpy() for c in tb.env]
            near = np.nonzero(~((e[2] < boxes[0][0]) | (e[0] > boxes[0][2]) | (e[3] < boxes[0][1]) | (e[1] > boxes[0][3])))[0]
            sample = near[::max(1, len(near) // 400)]
            hit = np.isin(sample, got.cpu().numpy())
            rows = xy.view(n, PER, 2)[torch.from_numpy(sample).cuda()].cpu().tolist()
            bad = sum(G.intersects_restated([tuple(t) for t in r], "linestring", q) != bool(g) for r, g in zip(rows, hit))
            row["sample"], row["sample_disagreements"] = len(sample), int(bad)
            assert bad == 0, (name, bad)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    assert torch.equal(ids["box"], ids["rect5"]), "the rectangle as a polygon must give the box's ids"
    base = res["rows"][0]["refine_ms"]
    for row in res["rows"]:
        row["refine_over_box"] = round(row["refine_ms"] / base, 2) if base > 0 else None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
