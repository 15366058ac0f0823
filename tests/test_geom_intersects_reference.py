"""The two host references of the exact full filter agree (tests/geom_intersects_ref.py): the kernel's route
(RectangleLineIntersector's diagonal rule on orientation signs, RayCrossingCounter for one box corner) equals
the closed-set definition in exact rational arithmetic, on inputs built to sit on every edge case, and both
give the reference's answers for its own test features."""
import math

import numpy as np
import pytest

import geom_intersects_ref as R

MIN_CASES = 20


def lat(rng, lo, hi, size=None):
    """1/8-lattice ordinates in [lo / 8, hi / 8]."""
    return rng.integers(lo, hi + 1, size) / 8.0


def lattice_box(rng, span=4):
    x = np.sort(rng.choice(np.arange(-span, span + 1), 2, replace=False)) / 8.0
    y = np.sort(rng.choice(np.arange(-span, span + 1), 2, replace=False)) / 8.0
    return (x[0], y[0], x[1], y[1])


def nudge(rng, v):
    """v moved 0-3 ulps, either way.  A zero ordinate moves by ulps of the lattice step (2^-55), not by
    its own 5e-324: next to a subnormal ordinate the products of JTS's double-double orientation
    (CGAlgorithmsDD) underflow, so neither JTS nor its restatement is exact there.  With zero moved by 5e-324 one of this
    module's 6000 nudged segments disagrees; test_subnormal_ordinates_stay_unpinned keeps that case."""
    k = int(rng.integers(0, 4))
    to = math.inf if rng.random() < 0.5 else -math.inf
    if v == 0.0:
        return math.copysign(k * math.ulp(0.125), to)
    for _ in range(k):
        v = math.nextafter(v, to)
    return v


def star_ring(rng, span=8):
    """A closed ring through 3-8 distinct lattice points, ordered by angle about their mean."""
    k = int(rng.integers(3, 9))
    pts = set()
    while len(pts) < k:
        pts.add((float(lat(rng, -span, span)), float(lat(rng, -span, span))))
    pts = list(pts)
    cx, cy = sum(p[0] for p in pts) / k, sum(p[1] for p in pts) / k
    pts.sort(key=lambda p: math.atan2(p[1] - cy, p[0] - cx))
    return pts + [pts[0]]


def cross(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])   # exact on the lattice


def on_segment(a, b, p):
    return cross(a, b, p) == 0 and R._in_seg_env(a, b, p)


def corners(b):
    return ((b[0], b[1]), (b[2], b[1]), (b[2], b[3]), (b[0], b[3]))


def on_boundary(p, b):
    return R._pt_in_box(p[0], p[1], b) and (p[0] in (b[0], b[2]) or p[1] in (b[1], b[3]))


def both(row, kind, box):
    e, r = R.intersects_exact(row, kind, box), R.intersects_restated(row, kind, box)
    assert e == r, (kind, row, box, e, r)
    return e


def test_segments_on_the_lattice_and_nudged(oracle):
    """Lines against proper lattice boxes: through a corner, along an edge, touching at an endpoint; then
    the same inputs with every ordinate moved 0-3 ulps."""
    rng = np.random.default_rng(1)
    seen = dict(corner_pass=0, on_edge=0, endpoint_touch=0, envelope_hit_miss=0, hit=0, nudged=0, nudged_flip=0)
    for _ in range(6000):
        a = (float(lat(rng, -6, 6)), float(lat(rng, -6, 6)))
        b = (float(lat(rng, -6, 6)), float(lat(rng, -6, 6)))
        box = lattice_box(rng)
        m = both([a, b], "linestring", box)
        ends_in = R._pt_in_box(*a, box) or R._pt_in_box(*b, box)
        seen["hit"] += m
        seen["corner_pass"] += (not ends_in) and any(on_segment(a, b, c) for c in corners(box))
        seen["on_edge"] += a != b and ((a[0] == b[0] and a[0] in (box[0], box[2]) and
                                        max(min(a[1], b[1]), box[1]) < min(max(a[1], b[1]), box[3])) or
                                       (a[1] == b[1] and a[1] in (box[1], box[3]) and
                                        max(min(a[0], b[0]), box[0]) < min(max(a[0], b[0]), box[2])))
        seen["endpoint_touch"] += on_boundary(a, box) != on_boundary(b, box) and not (
            R._pt_in_box(*a, box) and R._pt_in_box(*b, box))
        env_hit = not (box[0] > max(a[0], b[0]) or box[2] < min(a[0], b[0]) or box[1] > max(a[1], b[1]) or
                       box[3] < min(a[1], b[1]))
        seen["envelope_hit_miss"] += env_hit and not m
        na, nb = tuple(nudge(rng, v) for v in a), tuple(nudge(rng, v) for v in b)
        nbox = tuple(nudge(rng, v) for v in box)
        seen["nudged"] += 1
        seen["nudged_flip"] += both([na, nb], "linestring", nbox) != m
    assert all(v >= MIN_CASES for v in seen.values()), seen


def test_rings_on_the_lattice_and_nudged(oracle):
    """Polygons against lattice boxes: box corners on ring vertices and on ring edges, boxes inside a ring
    with no segment near (the corner rule alone), and the nudged copies."""
    rng = np.random.default_rng(2)
    seen = dict(corner_on_vertex=0, corner_on_edge=0, corner_rule_alone=0, miss=0, nudged=0)
    for _ in range(2500):
        ring = star_ring(rng)
        box = lattice_box(rng, 6)
        m = both([ring], "polygon", box)
        cs = corners(box)
        seen["corner_on_vertex"] += any(c in ring for c in cs)
        seen["corner_on_edge"] += any(on_segment(a, b, c) and c != a and c != b
                                      for a, b in zip(ring, ring[1:]) for c in cs)
        seen["corner_rule_alone"] += m and not any(R.seg_meets_box(a, b, box) for a, b in zip(ring, ring[1:]))
        seen["miss"] += not m
        nring = [tuple(nudge(rng, v) for v in p) for p in ring[:-1]]
        both([nring + [nring[0]]], "polygon", tuple(nudge(rng, v) for v in box))
        seen["nudged"] += 1
    assert all(v >= MIN_CASES for v in seen.values()), seen


def test_degenerate_boxes(oracle):
    """Zero-width, zero-height and point boxes against lattice lines, rings and points."""
    rng = np.random.default_rng(3)
    seen = dict(zero_width=0, zero_height=0, point=0, zero_width_hit=0, zero_height_hit=0, point_hit=0)
    for i in range(3000):
        x, y = float(lat(rng, -4, 4)), float(lat(rng, -4, 4))
        y1, x1 = y + float(lat(rng, 1, 6)), x + float(lat(rng, 1, 6))
        name, box = (("zero_width", (x, y, x, y1)), ("zero_height", (x, y, x1, y)), ("point", (x, y, x, y)))[i % 3]
        k = i % 4
        if k == 0:
            m = both([(float(lat(rng, -6, 6)), float(lat(rng, -6, 6))) for _ in range(2)], "linestring", box)
        elif k == 1:
            m = both([star_ring(rng, 6)], "polygon", box)
        elif k == 2:
            m = both([(float(lat(rng, -4, 4)), float(lat(rng, -4, 4))) for _ in range(3)], "multipoint", box)
        else:
            m = both([[(float(lat(rng, -6, 6)), float(lat(rng, -6, 6))) for _ in range(3)] for _ in range(2)],
                     "multilinestring", box)
        seen[name] += 1
        seen[name + "_hit"] += m
    assert all(v >= MIN_CASES for v in seen.values()), seen


def square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def test_holes_and_shared_edges(oracle):
    """The shell / hole rule: a box inside a hole misses, inside the shell's body matches, across a hole edge
    matches; MultiPolygons of two squares sharing an edge; empty geometries and the null box never match."""
    rng = np.random.default_rng(4)
    poly = [square(-2.0, -2.0, 2.0, 2.0), square(-1.0, -1.0, 1.0, 1.0)]
    seen = dict(in_hole=0, in_body=0, across_hole_edge=0, shared_edge=0, empty=0, null_box=0)
    for _ in range(40):
        w, h = float(lat(rng, 0, 6)), float(lat(rng, 0, 6))
        x, y = float(lat(rng, -7, 7 - int(w * 8))), float(lat(rng, -7, 7 - int(h * 8)))
        assert not both(poly, "polygon", (x, y, x + w, y + h))            # strictly inside the hole
        assert not both([poly], "multipolygon", (x, y, x + w, y + h))
        seen["in_hole"] += 1
        bx = float(lat(rng, 9, 15 - int(w * 8)))                           # x in (1, 2): the body, right of the hole
        assert both(poly, "polygon", (bx, y, bx + w, y + h))
        seen["in_body"] += 1
        ex = float(lat(rng, 1, 8))                                         # from inside the hole across x = 1
        assert both(poly, "polygon", (1.0 - ex, y, 1.0 + float(lat(rng, 0, 7)), y + h))
        seen["across_hole_edge"] += 1
    two = [[square(0.0, 0.0, 1.0, 1.0)], [square(1.0, 0.0, 2.0, 1.0)]]
    for _ in range(60):
        y = float(lat(rng, -4, 12))
        box = (1.0 - float(lat(rng, 0, 4)), y, 1.0 + float(lat(rng, 0, 4)), y + float(lat(rng, 0, 4)))
        assert both(two, "multipolygon", box) == (box[1] <= 1.0 and box[3] >= 0.0)
        seen["shared_edge"] += 1
    empties = [("linestring", []), ("multipoint", []), ("polygon", []), ("multilinestring", []), ("multipolygon", []),
               ("multipolygon", [[]]), ("multilinestring", [[]]), ("point", None)]
    for i in range(24):
        kind, row = empties[i % len(empties)]
        assert not both(row, kind, lattice_box(rng)) and not both(row, kind, (-180.0, -90.0, 180.0, 90.0))
        seen["empty"] += 1
    rows = [("linestring", [(0.0, 0.0), (1.0, 1.0)]), ("polygon", [square(-1.0, -1.0, 1.0, 1.0)]), ("point", (0.0, 0.0))]
    for i in range(24):
        kind, row = rows[i % 3]
        assert not both(row, kind, (1.0, -1.0, -1.0 - i, 1.0))
        seen["null_box"] += 1
    assert all(v >= MIN_CASES for v in seen.values()), seen


@pytest.mark.parametrize("fn", [R.intersects_exact, R.intersects_restated])
def test_reference_known_answers(oracle, fn):
    """XZ2IdxStrategyTest's polygons and bbox queries (XZ2IdxStrategyTest.scala:74-79, 88-93, 102-107, 132-136)
    and XZ3IndexTest's lines (XZ3IndexTest.scala:38-47, 54-64) come out with the reference's ids."""
    ids, rows, queries = R.xz2_strategy_polygons()
    for box, exp in queries:
        assert [i for i, r in zip(ids, rows) if fn(r, "polygon", box)] == exp
    rows, t, queries = R.xz3_index_linestrings()
    for box, (lo, hi), exp in queries:
        assert [i for i, r in enumerate(rows) if fn(r, "linestring", box) and lo < t[i] < hi] == exp


def test_the_issue_examples(oracle):
    """LINESTRING(0 0, 10 10) against bbox(8, 0, 10, 2): the envelopes meet, the geometries do not; an L-shaped
    polygon whose notch holds the box likewise."""
    assert not both([(0.0, 0.0), (10.0, 10.0)], "linestring", (8.0, 0.0, 10.0, 2.0))
    ell = [[(0.0, 0.0), (10.0, 0.0), (10.0, 2.0), (2.0, 2.0), (2.0, 10.0), (0.0, 10.0), (0.0, 0.0)]]
    assert not both(ell, "polygon", (5.0, 5.0, 8.0, 8.0)) and both(ell, "polygon", (0.5, 5.0, 1.0, 8.0))


def test_subnormal_ordinates_stay_unpinned(oracle):
    """The known disagreement, kept in sight: next to subnormal ordinates (a zero moved by its own ulp,
    5e-324) the products of JTS's double-double orientation underflow, and the restatement -- JTS's route, and
    the kernel's -- no longer equals the rationals.  This line and box are apart by exact arithmetic and meeting
    by the orientation signs.  The same inputs with the subnormals back at zero are decided alike.  If this
    test ever fails because the two agree, the orientation has become exact there and nudge() can move zeros
    by their own ulp."""
    line = [(0.7499999999999999, -5e-324), (-0.6249999999999999, 0.0)]
    box = (0.125, -0.5000000000000002, 0.24999999999999997, -5e-324)
    assert not R.intersects_exact(line, "linestring", box)
    assert R.intersects_restated(line, "linestring", box)
    flat = [(line[0][0], 0.0), line[1]]
    assert both(flat, "linestring", box[:3] + (0.0,))
