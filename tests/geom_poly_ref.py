"""Two host references for "geometry meets query polygons", the XZ tables' INTERSECTS full filter
(gm_scan_filter.polys), and the queries and features its tests share.

A geometry row is what oracle.arrow_rows gives (geom_intersects_ref).  A query is a list of PARTS, each part
a list of closed rings of (x, y), shell first; a part is the closed set "inside or on the shell, and not
strictly inside a hole", and a row matches iff it shares a point with some part.

  intersects_exact     the definition, in fractions.Fraction: a segment of the row meets a ring segment of
                       the part (exact signs), or ANY vertex of the row is in the part, or ANY vertex of the
                       part is in a polygon of the row (the same rule over the row's rings).
  intersects_restated  the kernel's route (geomesa_hip.h): contact as RobustLineIntersector decides it --
                       envelopes, then oracle.orientation_index signs, then the collinear rule; without
                       contact the FIRST tuple of each piece (point, line, polygon shell) located with
                       RayCrossingCounter ring by ring, and for a polygon the part's FIRST shell vertex
                       located in it.

Both skip segment pairs whose envelopes are disjoint with numpy compares (exact on doubles) so that a scan of
a few thousand features takes seconds; decide() names the step of the procedure that settled a row.
"""
import functools
from fractions import Fraction as Fr

import numpy as np

import geom_intersects_ref as R
import oracle as O


def _segs(run):
    a = np.asarray(run, np.float64).reshape(-1, 2)
    return np.hstack([a[:-1], a[1:]]) if len(a) >= 2 else np.zeros((0, 4))


class Query:
    """The parts with their ring segments as arrays (n x (ax, ay, bx, by)) and each part's shell envelope."""

    def __init__(self, parts):
        self.parts = [[[(float(x), float(y)) for x, y in ring] for ring in part] for part in parts]
        self.segs = [[_segs(ring) for ring in part] for part in self.parts]
        self.boxes = [(min(x for x, _ in p[0]), min(y for _, y in p[0]), max(x for x, _ in p[0]),
                       max(y for _, y in p[0])) for p in self.parts]
        self.all = np.vstack([s for part in self.segs for s in part])

    def polygon_set(self):
        """As join.PolygonSet.from_polygons takes it: every part a polygon of its own."""
        return [[part] for part in self.parts]


def _overlap_pairs(gs, qs):
    """Index pairs (i, j) of segments whose envelopes overlap (Envelope.intersects(p1, p2, q1, q2))."""
    if not len(gs) or not len(qs):
        return []
    gx0, gx1 = np.minimum(gs[:, 0], gs[:, 2])[:, None], np.maximum(gs[:, 0], gs[:, 2])[:, None]
    gy0, gy1 = np.minimum(gs[:, 1], gs[:, 3])[:, None], np.maximum(gs[:, 1], gs[:, 3])[:, None]
    qx0, qx1 = np.minimum(qs[:, 0], qs[:, 2])[None], np.maximum(qs[:, 0], qs[:, 2])[None]
    qy0, qy1 = np.minimum(qs[:, 1], qs[:, 3])[None], np.maximum(qs[:, 1], qs[:, 3])[None]
    ok = ~((gx0 > qx1) | (gx1 < qx0) | (gy0 > qy1) | (gy1 < qy0))
    return np.argwhere(ok).tolist()


def _y_span(segs, py):
    """The segments whose closed y-range holds py: the only ones a crossing count can count or find py on."""
    return segs[(np.minimum(segs[:, 1], segs[:, 3]) <= py) & (np.maximum(segs[:, 1], segs[:, 3]) >= py)].tolist()


# ---------------------------------------------------------------- exact
def _sign(v):
    return (v > 0) - (v < 0)


def _orient_exact(ax, ay, bx, by, cx, cy):
    return _sign((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))


def seg_seg_exact(s, t):
    ax, ay, bx, by = (Fr(v) for v in s)
    cx, cy, dx, dy = (Fr(v) for v in t)
    o1, o2 = _orient_exact(ax, ay, bx, by, cx, cy), _orient_exact(ax, ay, bx, by, dx, dy)
    o3, o4 = _orient_exact(cx, cy, dx, dy, ax, ay), _orient_exact(cx, cy, dx, dy, bx, by)
    if o1 == o2 == o3 == o4 == 0:      # collinear: they meet iff their ranges overlap on both axes
        return (max(min(ax, bx), min(cx, dx)) <= min(max(ax, bx), max(cx, dx)) and
                max(min(ay, by), min(cy, dy)) <= min(max(ay, by), max(cy, dy)))
    return o1 * o2 <= 0 and o3 * o4 <= 0


def _locate_pairs_exact(pairs, px, py):
    """0 exterior, 1 boundary, 2 interior of the point in the ring these segments are of."""
    px, py = Fr(px), Fr(py)
    inside = False
    for s in pairs:
        ax, ay, bx, by = (Fr(v) for v in s)
        cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        if cr == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return 1
        if (ay > py) != (by > py):
            if ax + (py - ay) * (bx - ax) / (by - ay) > px:
                inside = not inside
    return 2 if inside else 0


def in_part_exact(ring_segs, px, py):
    """The closed-set rule: inside or on the shell, and strictly inside no hole."""
    if not ring_segs or _locate_pairs_exact(_y_span(ring_segs[0], py), px, py) == 0:
        return False
    return all(_locate_pairs_exact(_y_span(h, py), px, py) != 2 for h in ring_segs[1:])


def _in_box(x, y, b):
    return b[0] <= x <= b[2] and b[1] <= y <= b[3]


def intersects_exact(row, kind, q):
    if row is None:
        return False
    pts, lines, polys = R._parts(row, kind)
    runs = [r for r in lines if r] + [r for p in polys for r in p if r]
    verts = list(pts) + [v for r in runs for v in r]
    gsegs = np.vstack([_segs(r) for r in runs]) if runs else np.zeros((0, 4))
    if any(seg_seg_exact(gsegs[i], q.all[j]) for i, j in _overlap_pairs(gsegs, q.all)):
        return True
    for part, box in zip(q.segs, q.boxes):
        if any(_in_box(x, y, box) and in_part_exact(part, x, y) for x, y in verts):
            return True
    for poly in polys:
        rs = [_segs(r) for r in poly if r]
        if rs and any(in_part_exact(rs, x, y) for part in q.parts for ring in part for x, y in ring):
            return True
    return False


# ---------------------------------------------------------------- restated (the kernel's route)
def seg_meets_seg(s, t):
    """RobustLineIntersector.computeIntersect(p1, p2, q1, q2).hasIntersection()."""
    a, b, c, d = (s[0], s[1]), (s[2], s[3]), (t[0], t[1]), (t[2], t[3])
    if (min(a[0], b[0]) > max(c[0], d[0]) or max(a[0], b[0]) < min(c[0], d[0]) or
            min(a[1], b[1]) > max(c[1], d[1]) or max(a[1], b[1]) < min(c[1], d[1])):
        return False
    pq1, pq2 = O.orientation_index(*a, *b, *c), O.orientation_index(*a, *b, *d)
    if (pq1 > 0 and pq2 > 0) or (pq1 < 0 and pq2 < 0):
        return False
    qp1, qp2 = O.orientation_index(*c, *d, *a), O.orientation_index(*c, *d, *b)
    if (qp1 > 0 and qp2 > 0) or (qp1 < 0 and qp2 < 0):
        return False
    if pq1 == 0 and pq2 == 0 and qp1 == 0 and qp2 == 0:
        return R._in_seg_env(a, b, c) or R._in_seg_env(a, b, d) or R._in_seg_env(c, d, a) or R._in_seg_env(c, d, b)
    return True


def _ring_count(segs, p):
    """RayCrossingCounter over a ring's segments: (on the ring, crossings odd)."""
    cross = 0
    for s in _y_span(segs, p[1]):
        on, c = R.count_segment((s[0], s[1]), (s[2], s[3]), p)
        if on:
            return True, False
        cross += c
    return False, bool(cross & 1)


def in_part_restated(ring_segs, p):
    on, odd = _ring_count(ring_segs[0], p)
    if not (on or odd):
        return False
    for h in ring_segs[1:]:
        on, odd = _ring_count(h, p)
        if odd and not on:
            return False
    return True


def _located(p, q):
    return any(in_part_restated(part, p) for part in q.segs)


def _contact(run, q):
    gs = _segs(run)
    return any(seg_meets_seg(gs[i], q.all[j]) for i, j in _overlap_pairs(gs, q.all))


def decide(row, kind, q):
    """None: no match; else the step that settled it: "contact", "g_in_q" (a piece's first tuple in a part) or
    "q_in_g" (a part's first shell vertex in a polygon of the row)."""
    if row is None:
        return None
    pts, lines, polys = R._parts(row, kind)
    how = None
    for p in pts:
        if _located(p, q):
            return "g_in_q"
    for line in lines:
        if line and _contact(line, q):
            return "contact"
    for rings in polys:
        if any(ring and _contact(ring, q) for ring in rings):
            return "contact"
    for line in lines:
        if line and _located(line[0], q):
            return "g_in_q"
    for rings in polys:
        if rings and rings[0] and _located(rings[0][0], q):
            how = how or "g_in_q"
    if how:
        return how
    for rings in polys:
        rs = [_segs(r) for r in rings]
        if not rings or not rings[0]:
            continue
        for part in q.parts:
            counts = [_ring_count(r, part[0][0]) if len(r) else (False, False) for r in rs]
            if any(on for on, _ in counts):       # on a ring of the row (contact finds it first)
                return "q_in_g"
            if counts[0][1] and not any(odd for _, odd in counts[1:]):
                return "q_in_g"
    return None


def intersects_restated(row, kind, q):
    return decide(row, kind, q) is not None


def envelope_hit(env, q):
    """The prefilter: the feature's JTS envelope meets a part's (oracle.envelope_scan's rule)."""
    return O.envelope_scan(*env, q.boxes)


def scan(rows, kind, q, env, fn=intersects_restated):
    """The full filter over every feature; the envelope prefilter first, as the definition allows."""
    hit = envelope_hit(env, q)
    return np.array([bool(h) and fn(r, kind, q) for r, h in zip(rows, hit)], bool)


# ---------------------------------------------------------------- what sits wholly in a hole
def _all_vertices(row, kind):
    pts, lines, polys = R._parts(row, kind)
    return list(pts) + [v for r in lines for v in r] + [v for p in polys for r in p for v in r]


def wholly_in_hole_of_query(row, kind, q):
    """Every vertex of the row strictly inside ONE hole ring of the query (and the row does not match)."""
    vs = _all_vertices(row, kind) if row is not None else []
    return bool(vs) and any(all(_locate_pairs_exact(_y_span(h, y), x, y) == 2 for x, y in vs)
                            for part in q.segs for h in part[1:])


def part_wholly_in_hole_of_row(row, kind, q):
    """The shell of some part strictly inside ONE hole ring of a polygon of the row.  For a row that does
    not match (the callers'): none of its rings touches the part, so the part's shell, one connected piece,
    is wholly where its first vertex is."""
    if row is None or kind not in ("polygon", "multipolygon"):
        return False
    holes = [_segs(h) for p in R._parts(row, kind)[2] for h in p[1:] if len(h) >= 4]
    return any(_locate_pairs_exact(_y_span(h, part[0][0][1]), *part[0][0]) == 2 for part in q.parts for h in holes)


# ---------------------------------------------------------------- the queries
CENTRE = (0.0, 0.0)
RAD = 8.0                                   # every central part fits the disc of radius 9.5 about CENTRE
S1, S2, S3 = (-2.0, 0.0), (2.0, 0.0), (0.0, 2.75)   # small planted features; S1 and S2 sit in `holed`'s holes
FAR_B, FAR_C = (40.0, 20.0), (-40.0, -25.0)          # `multi`'s far part and second polygon
WORLD = (-180.0, -90.0, 180.0, 90.0)
RECT = (-7.0, -5.0, 7.0, 5.5)
LDS_ENTRIES = 2040                           # gm_geom_filter.hip's PQ_LDS_ENTRIES


def star(c, rad, m, seed, lo=0.55):
    """A star-shaped closed ring of m tuples about c, radii in [lo, 1] rad."""
    rng = np.random.default_rng(seed)
    th = np.sort(rng.uniform(0, 2 * np.pi, m - 1))
    r = rad * rng.uniform(lo, 1.0, m - 1)
    pts = list(zip((c[0] + r * np.cos(th)).tolist(), (c[1] + r * np.sin(th)).tolist()))
    return pts + [pts[0]]


def _rect_ring(b):
    return [(b[0], b[1]), (b[2], b[1]), (b[2], b[3]), (b[0], b[3]), (b[0], b[1])]


@functools.lru_cache(maxsize=None)
def queries():
    q = {
        "tri": [[[(-8.0, -5.0), (8.0, -5.0), (0.0, 8.0), (-8.0, -5.0)]]],
        "concave": [[[(-7.0, -6.0), (7.0, -6.0), (7.0, 1.25), (3.5, 1.25), (3.5, 6.0), (-7.0, 6.0), (-7.0, -6.0)]]],
        "c64": [[star(CENTRE, RAD, 64, 64)]], "c65": [[star(CENTRE, RAD, 65, 65)]],
        "c66": [[star(CENTRE, RAD, 66, 66)]], "c129": [[star(CENTRE, RAD, 129, 129)]],
        "c1000": [[star(CENTRE, RAD, 1000, 1000)]],
        # past the entries the kernel stages in LDS: its edges are read from global memory
        "c2000": [[star(CENTRE, RAD, 2000, 2000)]],
        "holed": [[star(CENTRE, RAD, 129, 7),
                   [(S1[0] - 1.25, S1[1]), (S1[0], S1[1] - 1.25), (S1[0] + 1.25, S1[1]), (S1[0], S1[1] + 1.25),
                    (S1[0] - 1.25, S1[1])],
                   star(S2, 1.5, 65, 8)]],
        "multi": [[star(CENTRE, RAD, 65, 9)], [star(FAR_B, 3.0, 33, 10)], [star(FAR_C, 3.0, 5, 11)]],
        "rect": [[_rect_ring(RECT)]],
        "world": [[_rect_ring(WORLD)]],
    }
    return {k: Query(v) for k, v in q.items()}


def multi_as_polygons():
    """`multi` as the set it stands for: a polygon of two parts far apart, and a second polygon."""
    p = queries()["multi"].parts
    return [[p[0], p[1]], [p[2]]]


# ---------------------------------------------------------------- the features
def _small(rng, kind, site, gen):
    """A feature within 0.45 of the site."""
    c = (site[0] + float(rng.uniform(-0.1, 0.1)), site[1] + float(rng.uniform(-0.1, 0.1)))
    if kind == "point":
        return c
    m = int(rng.choice([2, 3, 5, 9]))
    if kind == "multipoint":
        return gen.arc(rng, c, 0.3, m, False, False)
    if kind == "linestring":
        return gen.arc(rng, c, 0.3, m, False, False)
    if kind == "multilinestring":
        return [gen.arc(rng, c, 0.3, m, False, False), gen.arc(rng, c, 0.2, 2, False, False)]
    ring = gen.arc(rng, c, 0.3, max(m, 5), False, True)
    return [ring] if kind == "polygon" else [[ring]]


def _big(rng, kind, gen, hole):
    """A polygon about CENTRE that holds the disc of radius 9.9: in its body, or (hole) in a hole of it."""
    m = int(rng.choice([64, 65, 129, 200]))
    if hole:
        rings = [gen.arc(rng, CENTRE, float(rng.uniform(38.0, 42.0)), m, False, True),
                 gen.arc(rng, CENTRE, float(rng.uniform(18.0, 20.0)), int(rng.choice([64, 65, 129])), False, True)]
    else:
        rings = [gen.arc(rng, CENTRE, float(rng.uniform(18.0, 22.0)), m, False, True)]
    return rings if kind == "polygon" else [rings]


@functools.lru_cache(maxsize=None)
def features(kind, seed=500, f32=False, n_random=None):
    """test_gpu_geom_scan.make_rows (random features about the centre, a third on the 1/4 lattice, the
    planted features of the box sites, null and empty slots) plus what the polygon conditions need: 60 small
    features at each of S1, S2, S3 and 20 at each far part; for lines, 12 long ones through the centre; for
    lines and multipoints, 60 that go round a corner of RECT without touching it; for polygons, 60 that hold
    every central part in their body and 60 that hold it in a hole."""
    import test_gpu_geom_scan as G
    rows = G.make_rows(kind, seed, False, n_random)
    rng = np.random.default_rng(seed + 1)
    for site, n in ((S1, 60), (S2, 60), (S3, 60), (FAR_B, 20), (FAR_C, 20)):
        rows += [_small(rng, kind, site, G) for _ in range(n)]
    if kind in ("linestring", "multilinestring"):
        for _ in range(12):
            th = rng.uniform(0, np.pi)
            t = np.sort(np.concatenate([[-1.0, 1.0], rng.uniform(-1, 1, 298)])) * 12.0
            line = list(zip((t * np.cos(th)).tolist(), (t * np.sin(th) + 0.3).tolist()))
            rows.append(line if kind == "linestring" else [line])
    if kind in ("multipoint", "linestring", "multilinestring"):
        # 60 two-segment lines (three points) around a corner of RECT: the envelopes overlap, nothing touches
        for _ in range(60):
            sx, cy = RECT[2] if rng.random() < 0.5 else RECT[0], RECT[3]
            d = rng.uniform(0.1, 0.4, 3)
            run = [(sx - sx / abs(sx) * 0.5, cy + d[0]), (sx + sx / abs(sx) * d[1], cy + d[0]),
                   (sx + sx / abs(sx) * d[1], cy - d[2])]
            rows.append([run] if kind == "multilinestring" else run)
    if kind in ("polygon", "multipolygon"):
        rows += [_big(rng, kind, G, hole) for hole in (False, True) for _ in range(60)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    if f32:
        def r32(v, depth):
            if depth == 0:
                return (float(np.float32(v[0])), float(np.float32(v[1])))
            return [r32(c, depth - 1) for c in v]
        rows = [None if r is None else r32(r, G.DEPTH[kind]) for r in rows]
    return rows


@functools.lru_cache(maxsize=None)
def envelopes(kind, seed=500, f32=False, n_random=None):
    import test_gpu_geom_scan as G
    return G.envelopes_of(O, features(kind, seed, f32, n_random), kind)


@functools.lru_cache(maxsize=None)
def decided(kind, name, seed=500, f32=False, n_random=None):
    """decide() over every feature of the kind, the envelope prefilter first: a list of None / step names."""
    q = queries()[name]
    hit = envelope_hit(envelopes(kind, seed, f32, n_random), q)
    return [decide(r, kind, q) if h else None for r, h in zip(features(kind, seed, f32, n_random), hit)]


def expected(kind, name, seed=500, f32=False, n_random=None):
    return np.array([d is not None for d in decided(kind, name, seed, f32, n_random)], bool)


def segment_counts(row, kind):
    """The segment count of each tuple run of a row."""
    _, lines, polys = R._parts(row, kind)
    return [len(r) - 1 for r in lines + [r for p in polys for r in p] if len(r) >= 2]


# ---------------------------------------------------------------- the bucket builder, restated
def slab_of(y, y0, inv_h, ns):
    c = np.floor((y - y0) * inv_h)
    if not c >= 0.0:
        return 0
    return ns - 1 if c > ns - 1 else int(c)


def buckets(q, max_slabs=4096, dup_max=2):
    """gm_poly_query_host.hpp's build: (ns, offsets, the edge ids of each slab in order)."""
    edges = [tuple(s) for part in q.segs for ring in part for s in ring.tolist()]
    ys = [v for e in edges for v in (e[1], e[3])]
    y0, y1 = min(ys), max(ys)
    n = len(edges)
    ns = min(max(n // 2, 1), max_slabs)
    while True:
        k = ns if y1 > y0 else 1
        inv_h = np.float64(k) / np.float64(y1 - y0) if y1 > y0 else 0.0
        slabs = [[] for _ in range(k)]
        for i, e in enumerate(edges):
            for s in range(slab_of(min(e[1], e[3]), y0, inv_h, k), slab_of(max(e[1], e[3]), y0, inv_h, k) + 1):
                slabs[s].append(i)
        if k == 1 or sum(len(s) for s in slabs) <= dup_max * n:
            return k, slabs
        ns //= 2
