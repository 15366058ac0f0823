"""Two host references for "geometry meets query box", the XZ tables' exact full filter (GeoTools BBOX on the
feature geometry, GeometryProcessing.scala:104-136: JTS Geometry.intersects with the rectangle).

A geometry row is what oracle.arrow_rows gives: None (null slot), (x, y) for a point, nested lists of
(x, y) for the other kinds (rings shell first, closed as stored).  A box is (xmin, ymin, xmax, ymax), a
closed set; xmax < xmin is the null box.

  intersects_exact     the definition, in fractions.Fraction: the row and the box share a point.  Segments
                       are clipped exactly (Liang-Barsky); a polygon also matches when a box corner is not
                       exterior to it, located exactly ring by ring with the shell / hole rule of JTS
                       SimplePointInAreaLocator (exterior to the shell: exterior; else interior to a hole:
                       exterior; on a ring: boundary) -- not Mod-2 over the rings.
  intersects_restated  the kernel's route: JTS RectangleIntersects' steps with compares and
                       oracle.orientation_index (RectangleLineIntersector's diagonal rule decided by
                       RobustLineIntersector's four signs), and RayCrossingCounter for the box corner
                       (xmin, ymin) ring by ring.  One corner stands for the four: when no ring segment
                       meets the box the box touches no ring, so its corners share one location.
"""
from fractions import Fraction as Fr

import oracle as O


def _parts(row, kind):
    """(points, lines, polygons) of a non-null row: loose points, open tuple runs, lists of rings."""
    if kind == "point":
        return [row], [], []
    if kind == "multipoint":
        return list(row), [], []
    if kind == "linestring":
        return [], [row], []
    if kind == "multilinestring":
        return [], list(row), []
    if kind == "polygon":
        return [], [], [row]
    if kind == "multipolygon":
        return [], [], list(row)
    raise ValueError(kind)


def null_box(b):
    return b[2] < b[0]


# ---------------------------------------------------------------- exact
def _pt_in_box(x, y, b):
    return b[0] <= x <= b[2] and b[1] <= y <= b[3]


def _seg_box_exact(p, q, b):
    """The closed segment p-q meets the closed box (Liang-Barsky over Fractions)."""
    x0, y0, x1, y1 = Fr(p[0]), Fr(p[1]), Fr(q[0]), Fr(q[1])
    t0, t1 = Fr(0), Fr(1)
    for d, lo, hi, s in ((x1 - x0, Fr(b[0]), Fr(b[2]), x0), (y1 - y0, Fr(b[1]), Fr(b[3]), y0)):
        if d == 0:
            if s < lo or s > hi:
                return False
            continue
        ta, tb = (lo - s) / d, (hi - s) / d
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return False
    return True


def _locate_ring_exact(ring, px, py):
    """0 exterior, 1 boundary, 2 interior of the point in the closed ring (stored segments only)."""
    px, py = Fr(px), Fr(py)
    inside = False
    for (ax, ay), (bx, by) in zip(ring, ring[1:]):
        ax, ay, bx, by = Fr(ax), Fr(ay), Fr(bx), Fr(by)
        cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        if cr == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return 1
        if (ay > py) != (by > py):
            xi = ax + (py - ay) * (bx - ax) / (by - ay)   # the edge's x at the point's y
            if xi > px:
                inside = not inside
    return 2 if inside else 0


def _locate_polygon_exact(rings, px, py):
    if not rings:
        return 0
    loc = _locate_ring_exact(rings[0], px, py)
    if loc != 2:
        return loc
    for hole in rings[1:]:
        h = _locate_ring_exact(hole, px, py)
        if h == 1:
            return 1
        if h == 2:
            return 0
    return 2


def intersects_exact(row, kind, box):
    if row is None or null_box(box):
        return False
    pts, lines, polys = _parts(row, kind)
    if any(_pt_in_box(x, y, box) for x, y in pts):
        return True
    for line in lines + [r for p in polys for r in p]:
        if any(_seg_box_exact(a, b, box) for a, b in zip(line, line[1:])):
            return True
    corners = ((box[0], box[1]), (box[2], box[1]), (box[2], box[3]), (box[0], box[3]))
    return any(_locate_polygon_exact(p, cx, cy) != 0 for p in polys for cx, cy in corners)


# ---------------------------------------------------------------- restated (the kernel's route)
def _in_seg_env(a, b, q):
    return min(a[0], b[0]) <= q[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= q[1] <= max(a[1], b[1])


def seg_meets_box(a, b, box):
    """RectangleLineIntersector.intersects(p0, p1)."""
    if box[0] > max(a[0], b[0]) or box[2] < min(a[0], b[0]) or box[1] > max(a[1], b[1]) or box[3] < min(a[1], b[1]):
        return False
    if _pt_in_box(a[0], a[1], box) or _pt_in_box(b[0], b[1], box):
        return True
    if a[0] > b[0] or (a[0] == b[0] and a[1] > b[1]):
        a, b = b, a
    up = b[1] > a[1]
    d0 = (box[0], box[3] if up else box[1])
    d1 = (box[2], box[1] if up else box[3])
    pq1, pq2 = O.orientation_index(*a, *b, *d0), O.orientation_index(*a, *b, *d1)
    if (pq1 > 0 and pq2 > 0) or (pq1 < 0 and pq2 < 0):
        return False
    qp1, qp2 = O.orientation_index(*d0, *d1, *a), O.orientation_index(*d0, *d1, *b)
    if (qp1 > 0 and qp2 > 0) or (qp1 < 0 and qp2 < 0):
        return False
    if pq1 == 0 and pq2 == 0 and qp1 == 0 and qp2 == 0:
        return _in_seg_env(a, b, d0) or _in_seg_env(a, b, d1) or _in_seg_env(d0, d1, a) or _in_seg_env(d0, d1, b)
    return True


def count_segment(p1, p2, p):
    """RayCrossingCounter.countSegment: (on the segment, crossings added)."""
    if p1[0] < p[0] and p2[0] < p[0]:
        return False, 0
    if p[0] == p2[0] and p[1] == p2[1]:
        return True, 0
    if p1[1] == p[1] and p2[1] == p[1]:
        return min(p1[0], p2[0]) <= p[0] <= max(p1[0], p2[0]), 0
    if (p1[1] > p[1] and p2[1] <= p[1]) or (p2[1] > p[1] and p1[1] <= p[1]):
        o = O.orientation_index(*p1, *p2, *p)
        if o == 0:
            return True, 0
        if p2[1] < p1[1]:
            o = -o
        return False, 1 if o == 1 else 0
    return False, 0


def _ring_restated(ring, box):
    """(a segment meets the box or holds its corner, the corner's crossing parity)."""
    corner, cross = (box[0], box[1]), 0
    for a, b in zip(ring, ring[1:]):
        if seg_meets_box(a, b, box):
            return True, False
        on, c = count_segment(a, b, corner)
        if on:
            return True, False
        cross += c
    return False, bool(cross & 1)


def intersects_restated(row, kind, box):
    if row is None or null_box(box):
        return False
    pts, lines, polys = _parts(row, kind)
    if any(_pt_in_box(x, y, box) for x, y in pts):
        return True
    for line in lines:
        if any(seg_meets_box(a, b, box) for a, b in zip(line, line[1:])):
            return True
    for rings in polys:
        in_shell = in_hole = False
        for k, ring in enumerate(rings):
            hit, inside = _ring_restated(ring, box)
            if hit:
                return True
            if k == 0:
                in_shell = inside
            else:
                in_hole = in_hole or inside
        if in_shell and not in_hole:
            return True
    return False


def scan(rows, kind, boxes, fn=intersects_restated):
    """The full filter over every feature: row i meets any of the boxes."""
    import numpy as np
    return np.array([any(fn(r, kind, b) for b in boxes) for r in rows], bool)


# ---------------------------------------------------------------- the reference's own test features
def xz2_strategy_polygons():
    """XZ2IdxStrategyTest.scala:40-45: features 10-19, POLYGON((40 3k, 42 3k, 42 2k, 40 2k, 40 3k)), and
    its bbox queries with the ids they return (:74-79, :88-93, :102-107, :132-136)."""
    rows = [[[(40.0, 30.0 + k), (42.0, 30.0 + k), (42.0, 20.0 + k), (40.0, 20.0 + k), (40.0, 30.0 + k)]]
            for k in range(10)]
    queries = [((35.0, 29.0, 45.0, 31.0), list(range(10, 20))), ((35.0, 38.0, 45.0, 40.0), [18, 19]),
               ((39.999, 21.999, 40.001, 22.001), [10, 11, 12]), ((35.0, 22.0, 45.0, 24.0), [10, 11, 12, 13, 14])]
    return list(range(10, 20)), rows, queries


def xz3_index_linestrings():
    """XZ3IndexTest.scala:38-47: 32 two-point lines with their dtg (epoch ms), and the two queries (:54-64):
    (box, (lo, hi) of the DURING, expected ids)."""
    import calendar

    def ms(day, hour):
        return calendar.timegm((2020, 12, day, hour, 0, 0)) * 1000
    rows, t = [], []
    for i in range(10):
        rows.append([(40.0 + i, 60.0), (40.0 + i, 61.0)]); t.append(ms(7, i))
    for i in range(10, 20):
        rows.append([(30.0 + i, 60.0), (30.0 + i, 61.0)]); t.append(ms(i, i))
    for i in range(20, 30):
        rows.append([(40.0 + i, 60.0), (40.0 + i, 61.0)]); t.append(ms(i, i - 10))
    for i in range(30, 32):
        rows.append([(i - 20.0, 60.0), (i - 20.0, 61.0)]); t.append(ms(i, i - 10))
    end = ms(31, 23) + 59 * 60_000 + 59_999
    queries = [((0.0, 55.0, 70.0, 65.0), (ms(1, 0), end), list(range(32))),
               ((9.0, 59.0, 12.0, 61.0), (ms(31, 0), end), [31])]
    return rows, t, queries
