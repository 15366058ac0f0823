"""The WKB columns of test_wkb_reference.py and test_gpu_wkb.py, as lists of blobs (None: a null slot).  What
every slot should give comes from wkb_ref.parse of the slot's own bytes, so a column may hold anything.

  mixed_column()      LANE_SLOTS + slots around the query BOXES: all seven codes in every encoding style;
                      collections nested 1, 2 and 8 deep and 9 deep (malformed); Multi* and collections of
                      zero elements; empty points, lines and polygons; lines of 1, 2, 63, 64, 65 and 130
                      tuples; null slots.  Thin diagonal lines and L-shaped polygons (some with a hole in
                      the corner) placed within reach of a box, so that many envelopes meet a box the
                      geometry misses and many geometries meet a box their envelope is not inside.
  special_column()    NaN (with payloads), +-Inf and -0.0 ordinates in both byte orders.
  malformed_column()  slots the grammar rejects, each laid out so that the bytes after it complete a valid
                      geometry of another envelope: every proper prefix B[:k] of a blob B is followed by the
                      slot B[k:], so a reader that ran past the slot's end would see all of B.
"""
import struct

import numpy as np

import wkb_ref as W

LANE_SLOTS = 2 * 256 + 5          # two full blocks of the lane-per-slot kernels and a tail
LINE_TUPLES = [1, 2, 63, 64, 65, 130]
BOXES = [(-10.0, -10.0, -9.0, -9.0), (5.0, 5.0, 6.5, 6.0), (8.0, -7.0, 8.5, -6.5)]
QUERIES = {"a": BOXES[:1], "b": BOXES[1:2], "c": BOXES[2:], "all": BOXES}

STYLES = [W.BE, W.LE, W.Style(False, "z"), W.Style(True, "z", iso=True), W.Style(True, "m"),
          W.Style(False, "m", iso=True), W.Style(False, "zm"), W.Style(True, "zm", iso=True),
          W.Style(False, srid=4326), W.Style(True, "z", srid=3857)]


def alternate(path, geom):
    """Nested geometries in alternating byte order, every third with Z."""
    k = sum(path) + len(path)
    return W.Style(bool(k & 1), "z" if k % 3 == 0 else "")


def diagonal(c, m, anti=False):
    """A straight thin line of m tuples through c, 6 x 6 across (m = 1: the point c)."""
    if m == 1:
        return [c]
    t = np.linspace(-3.0, 3.0, m)
    return list(zip((c[0] + t).tolist(), (c[1] + (-t if anti else t)).tolist()))


def ell(c, hole):
    """An L-shaped polygon with its inner corner at c - 1.5, arms 1.5 wide and 6 long; hole: a square hole in
    the corner block."""
    x, y = c
    rings = [[(x - 3, y - 3), (x + 3, y - 3), (x + 3, y - 1.5), (x - 1.5, y - 1.5), (x - 1.5, y + 3), (x - 3, y + 3),
              (x - 3, y - 3)]]
    if hole:
        rings.append([(x - 2.75, y - 2.75), (x - 1.75, y - 2.75), (x - 1.75, y - 1.75), (x - 2.75, y - 1.75),
                      (x - 2.75, y - 2.75)])
    return rings


def nest(geom, depth):
    """geom inside `depth` GeometryCollections."""
    for _ in range(depth):
        geom = ("collection", [geom])
    return geom


def near(rng, i):
    b = BOXES[i % len(BOXES)]
    return ((b[0] + b[2]) / 2 + float(rng.uniform(-2.5, 2.5)), (b[1] + b[3]) / 2 + float(rng.uniform(-2.5, 2.5)))


def feature(rng, i):
    """Slot i's geometry, by i mod 16."""
    c, k = near(rng, i), i % 16
    m = LINE_TUPLES[(i // 16) % len(LINE_TUPLES)]
    if k == 0:
        b = BOXES[i % len(BOXES)]
        return ("point", (float(rng.uniform(b[0] - 0.5, b[2] + 0.5)), float(rng.uniform(b[1] - 0.5, b[3] + 0.5))))
    if k in (1, 2, 3):
        return ("linestring", diagonal(c, m, anti=k == 3))
    if k in (4, 5, 6):
        return ("polygon", ell(c, hole=k != 4))
    if k == 7:
        return ("multipoint", [near(rng, i) for _ in range(int(rng.integers(1, 5)))])
    if k == 8:
        return ("multilinestring", [diagonal(c, m), diagonal(near(rng, i), 2, anti=True)])
    if k == 9:
        return ("multipolygon", [ell(c, True), ell(near(rng, i), False)])
    if k == 10:
        return ("collection", [("linestring", diagonal(c, m)), ("point", near(rng, i)), ("polygon", ell(near(rng, i), True))])
    if k == 11:
        return nest(("multilinestring", [diagonal(c, 2), diagonal(c, m, anti=True)]), 1)     # depth 2
    if k == 12:
        return nest(("polygon", ell(c, True)), W.MAX_DEPTH)                                  # depth 8
    if k == 13:
        return nest(("multipoint", [c, near(rng, i)]), W.MAX_DEPTH - 1)                      # depth 8, a Multi* innermost
    if k == 14:
        return ("collection", [W.EMPTY_POINT, ("linestring", []), ("polygon", ell(c, False)), ("collection", [])])
    return [W.EMPTY_POINT, ("linestring", []), ("polygon", []), ("multipoint", []), ("multilinestring", []),
            ("multipolygon", []), ("collection", []), nest(("point", c), W.MAX_DEPTH + 1),   # depth 9: malformed
            nest(("multipoint", [c]), W.MAX_DEPTH), ("polygon", [[]]), ("linestring", [c]), None][(i // 16) % 12]


def mixed_column(seed=5, n=LANE_SLOTS + 123):
    rng = np.random.default_rng(seed)
    blobs = []
    for i in range(n):
        g = feature(rng, i)
        if g is None:
            blobs.append(None)
            continue
        style = STYLES[(i // 3) % len(STYLES)]
        b = W.write(g, style, alternate if i % 5 == 0 else None)
        blobs.append(b + bytes(range(i % 4)) if i % 7 == 0 else b)      # trailing bytes are ignored
    return blobs


def special_column():
    nan1 = struct.unpack(">d", bytes.fromhex("7ff8000000abc123"))[0]
    nan2 = struct.unpack(">d", bytes.fromhex("fff4000000000007"))[0]
    inf = float("inf")
    geoms = [("point", (-0.0, 0.0)), ("point", (nan1, 1.0)), ("point", (1.0, nan2)), ("point", (inf, -inf)),
             ("linestring", [(nan1, nan2), (1.0, 2.0), (3.0, -4.0)]), ("linestring", [(1.0, 2.0), (nan2, nan1), (-0.0, 5.0)]),
             ("linestring", [(-0.0, -0.0), (0.0, 0.0)]), ("linestring", [(0.0, 0.0), (-0.0, -0.0)]),
             ("linestring", [(-inf, 1.0), (inf, 2.0)]), ("multipoint", [(nan1, 0.0), (2.0, -0.0)]),
             ("polygon", [[(0.0, 0.0), (inf, 0.0), (0.0, nan1), (0.0, 0.0)]]),
             ("collection", [("linestring", [(nan2, 7.0), (1.0, 1.0)]), ("point", (-0.0, 3.0))])]
    return [W.write(g, s) for g in geoms for s in (W.BE, W.LE, W.Style(True, "zm"))]


def line_header(le, count, code=2):
    e = "<" if le else ">"
    return struct.pack("B", le) + struct.pack(e + "II", code, count)


def malformed_column():
    """(blobs, the indices that must be malformed).  The other slots are whatever wkb_ref.parse makes of them."""
    blobs, bad = [], []

    def prefixes(b):
        for k in range(len(b)):
            bad.append(len(blobs))
            blobs.extend([b[:k], b[k:]])
    prefixes(W.write(("linestring", diagonal((3.0, 4.0), 5)), W.BE))
    prefixes(W.write(("collection", [("multipoint", [(1.0, 2.0), (30.0, 40.0)]),
                                     ("collection", [("polygon", ell((7.0, 7.0), True)), ("point", (50.0, -60.0))])]),
                     W.LE, alternate))
    prefixes(W.write(("point", (11.0, 12.0)), W.Style(True, "z", srid=4326)))
    tail = b"".join(struct.pack("<dd", 100.0 + k, -50.0 - k) for k in range(1000))
    cases = [line_header(True, 0xffffffff) + tail[:160],                       # rejected by the length alone
             line_header(True, 1000) + tail[:16 * 999],                        # one tuple short ...
             tail[16 * 999:] + W.write(("point", (1.0, 1.0))),                 # ... which the next slot holds
             line_header(False, 3) + struct.pack(">dd", 1.0, 2.0),
             struct.pack(">dddd", 5.0, 6.0, 7.0, 8.0),
             W.write(("multipoint", [(1.0, 2.0)]))[:9] + W.write(("linestring", diagonal((0.0, 0.0), 2))),   # wrong element
             W.write(("multipolygon", [ell((0.0, 0.0), False)]))[:9] + W.write(("point", (1.0, 2.0))),
             W.write(("multilinestring", [diagonal((0.0, 0.0), 2)]))[:9] + W.write(("polygon", ell((0.0, 0.0), False))),
             b"\x02" + W.write(("point", (1.0, 2.0)))[1:],                     # order byte 2
             b"\x00\x00\x00\x00\x00" + struct.pack(">dd", 1.0, 2.0),           # code 0
             b"\x01\x08\x00\x00\x00" + struct.pack("<dd", 1.0, 2.0),           # code 8
             b"\x00\x00\x00\x03\xe8" + struct.pack(">dd", 1.0, 2.0),           # ISO 1000: Z of code 0
             W.write(("polygon", [[(0.0, 0.0), (1.0, 1.0)]]))[:9] + struct.pack(">I", 900) + struct.pack(">dd", 1.0, 2.0),
             W.write(("polygon", []))[:5] + struct.pack(">I", 0xffffffff)]
    for k, b in enumerate(cases):
        if k != 2 and k != 4:      # 2 and 4 are the continuations of their predecessors
            bad.append(len(blobs))
        blobs.append(b)
    return blobs, bad


def check_shortcut_coverage(geoms, boxes):
    """On the reference alone: of the envelope survivors at least a quarter fail the exact test and at least a
    quarter pass it with an envelope inside none of the boxes.  Returns (envelope hits, matches)."""
    env_hit, exp = W.env_scan(geoms, boxes), W.scan(geoms, boxes)
    assert not (exp & ~env_hit).any()
    inside = np.array([any(W.env_inside(g, b) for b in boxes) for g in geoms], bool)
    surv = int(env_hit.sum())
    assert surv >= 2 * 4 + 1
    assert 4 * int((env_hit & ~exp).sum()) >= surv, (int((env_hit & ~exp).sum()), surv)
    assert 4 * int((exp & ~inside).sum()) >= surv, (int((exp & ~inside).sum()), surv)
    return env_hit, exp
