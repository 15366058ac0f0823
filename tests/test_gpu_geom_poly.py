"""GPU parity of INTERSECTS against query polygons: gm_table_scan_geom with gm_scan_filter.polys, through
XZ2Table / XZ3Table.query(polygons=...) and through the C ABI.

Every result equals geom_poly_ref.intersects_restated over EVERY feature (a full scan, which also proves the
ranges planned from the parts' envelopes cover), ANDed with FastDuring where a query has an interval.  The
inputs -- features, queries and the cases they hold -- are geom_poly_ref's; tests/test_geom_poly_reference.py
holds them to the exact reference and counts the cases without a GPU.  The queries' ring tuple counts are
where the lanes-over-edges loop changes shape (64, 65, 66, 129), 1,000, and 2,000: past the entries the
kernel stages in LDS."""
import ctypes
import functools

import numpy as np
import pyarrow as pa
import pytest

import geom_poly_ref as P
from abi_buffers import Guarded, untouched
from test_gpu_geom_scan import KINDS, T0, WEEK_MS, as_np, to_arrow

pytestmark = pytest.mark.gpu


def polygons_of(name):
    return P.multi_as_polygons() if name == "multi" else P.queries()[name].polygon_set()


@functools.lru_cache(maxsize=None)
def xz2_case(kind):
    from geomesa_amd.table import XZ2Table
    rows = P.features(kind)
    sh = (np.arange(len(rows)) * 2654435761 % 4).astype(np.uint8)
    return XZ2Table.from_geometries(to_arrow(rows, kind), kind, shard=sh, shards=4)


def check(tb, got, exp, env_hit):
    ids, nm, scanned = got
    assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
    assert tb.n_envelope == env_hit.sum() and nm <= tb.n_envelope <= scanned


# ---------------------------------------------------------------- XZ2, all kinds x queries
@pytest.mark.parametrize("name", list(P.queries()))
@pytest.mark.parametrize("kind", KINDS)
def test_xz2_polygon_query(gpu, oracle, kind, name):
    tb, q = xz2_case(kind), P.queries()[name]
    exp, env_hit = P.expected(kind, name), P.envelope_hit(P.envelopes(kind), q)
    assert exp.sum() >= 50 and not (exp & ~env_hit).any()
    if kind not in ("point", "multipoint"):     # both kernel shapes, from the inputs
        runs = [n for r, h in zip(P.features(kind), env_hit) if h for n in P.segment_counts(r, kind)]
        assert any(n < 64 for n in runs) and any(n > 128 for n in runs)
    check(tb, tb.query(polygons=polygons_of(name)), exp, env_hit)
    if name in ("rect", "world"):               # the box kernel as an independent witness
        box = P.RECT if name == "rect" else P.WORLD
        ids, nm, _ = tb.query(bboxes=[box])
        assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
    if name == "concave":                       # full_filter=False is still the bare range scan
        ids, nm, scanned = tb.query(polygons=polygons_of(name), full_filter=False)
        assert nm == scanned >= env_hit.sum() and set(np.nonzero(env_hit)[0]) <= set(as_np(ids).tolist())


def test_polygons_as_wkt_and_as_a_polygon_set(gpu, oracle):
    from geomesa_amd.join import PolygonSet
    tb, exp = xz2_case("linestring"), P.expected("linestring", "concave")
    ring = P.queries()["concave"].parts[0][0]
    wkt = "POLYGON((%s))" % ", ".join("%r %r" % p for p in ring)
    for arg in ([wkt], PolygonSet.from_wkt([wkt]), PolygonSet.from_polygons([[[ring[:-1]]]])):   # closed on the way in
        ids, nm, _ = tb.query(polygons=arg)
        assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])


# ---------------------------------------------------------------- XZ3
@functools.lru_cache(maxsize=None)
def xz3_case(kind, sharded):
    from geomesa_amd.table import XZ3Table
    rows = P.features(kind)
    rng = np.random.default_rng(31)
    t = T0 + rng.integers(WEEK_MS // 4, 6 * WEEK_MS, len(rows))
    t[:300] = T0 + 1500 + np.arange(300) % 3 - 1          # at and around an exclusive bound
    sh = (np.arange(len(rows)) * 2654435761 % 4).astype(np.uint8) if sharded else None
    return t, XZ3Table.from_geometries(to_arrow(rows, kind), t, kind, shard=sh, shards=4 if sharded else None)


@pytest.mark.parametrize("name", ["concave", "holed", "multi"])
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("kind", ["linestring", "polygon", "multipolygon"])
def test_xz3_polygon_query(gpu, oracle, kind, sharded, name):
    t, tb = xz3_case(kind, sharded)
    q, iv = P.queries()[name], (T0 + 1500, T0 + 5 * WEEK_MS + 999)
    during = (t > iv[0]) & (t < iv[1])
    exp = P.expected(kind, name) & during
    env_hit = oracle.envelope_scan(*P.envelopes(kind), q.boxes, t, iv)
    assert exp.sum() >= 50 and (P.expected(kind, name) & ~during).sum() >= 50
    check(tb, tb.query(polygons=polygons_of(name), interval=iv), exp, env_hit)
    check(tb, tb.query(polygons=polygons_of(name)), P.expected(kind, name), P.envelope_hit(P.envelopes(kind), q))


# ---------------------------------------------------------------- Float4 columns and flipAxisOrder
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("kind", ["linestring", "multipolygon"])
def test_xz2_float4_and_flip(gpu, oracle, kind, flip):
    from geomesa_amd.table import XZ2Table
    rows = P.features(kind, 55, True, 500)
    tb = XZ2Table.from_geometries(to_arrow(rows, kind, True, flip), kind, flip_axis=flip)
    for name in ("concave", "holed", "c65"):
        exp = P.expected(kind, name, 55, True, 500)
        assert 50 <= exp.sum() < len(rows) - 50
        check(tb, tb.query(polygons=polygons_of(name)), exp, P.envelope_hit(P.envelopes(kind, 55, True, 500), P.queries()[name]))


# ---------------------------------------------------------------- WKB columns
def wkb_array(rows, kind):
    import wkb_ref as W
    return pa.array([None if r is None else W.write((kind, r), W.LE if i & 1 else W.BE) for i, r in enumerate(rows)],
                    pa.binary())


@pytest.mark.parametrize("kind", ["linestring", "polygon", "multipolygon"])
def test_wkb_column_gives_the_typed_columns_ids(gpu, oracle, kind):
    from geomesa_amd.table import XZ2Table
    tb = XZ2Table.from_geometries(wkb_array(P.features(kind), kind), "wkb")
    for name in ("tri", "holed", "multi", "c2000"):
        check(tb, tb.query(polygons=polygons_of(name)), P.expected(kind, name),
              P.envelope_hit(P.envelopes(kind), P.queries()[name]))


# ---------------------------------------------------------------- the segment loop's step boundaries
STEP_SIZES = (2, 3, 64, 65, 127, 128)     # tuples: within a step, exactly one step (63 segments), one segment
STEP_HITS = (0, 62, 63, 125, 126)         # into the second, the third step's edge; hits at the steps' ends
STEP_BOX = (-0.5, -1.5, 0.5, 1.5)         # about (0, 0), inside the concave query; narrower than a joining
                                          # segment's x-extent, so no envelope shortcut settles a feature


STEP_THROUGH, STEP_AROUND, STEP_ASIDE = (-1.0, 1.0), (9.0, 11.0), (-50.0, 10.0)


def step_line(m, k, join):
    """m tuples on two rails, y = -20 and y = 20, far from both queries; segment k alone joins the rails, from
    (join[0], -20) to (join[1], 20): STEP_THROUGH runs it through the box and the concave query, STEP_ASIDE
    clear of both on their left, under the feature's envelope all the same."""
    return [(join[0] - 0.5 * (k - j), -20.0) if j <= k else (join[1] + 0.5 * (j - k - 1), 20.0) for j in range(m)]


def step_ring(m, k, join):
    """A closed ring of m >= 4 tuples: the same joining segment as segment k, the upper rail back to x = -80
    and the lower rail from there.  It encloses what lies left of the joining segment, between the rails:
    STEP_AROUND puts both queries inside with no segment near them, STEP_ASIDE both outside."""
    n, nu = m - 1, (m - 2) // 2
    nl = n - 2 - nu
    w = [(join[0], -20.0), (join[1], 20.0)]
    w += [(join[1] + (-80.0 - join[1]) * (i + 1) / nu, 20.0) for i in range(nu)]
    w += [(-80.0 + (join[0] + 80.0) * i / nl, -20.0) for i in range(nl)]
    ring = [w[(j - k) % n] for j in range(n)]
    return ring + [ring[0]]


@functools.lru_cache(maxsize=None)
def step_rows(kind):
    """(row, how many of its segments meet a query, match expected).  Rings of 2 and 3 tuples have no segment
    of their own to single out ([a, a]; [a, b, a]): they go in with every segment a hit."""
    rows = []
    for m in STEP_SIZES:
        hits = sorted({k for k in STEP_HITS + (m - 2,) if k <= m - 2})
        if kind == "linestring":
            rows += [(step_line(m, k, STEP_THROUGH), 1, True) for k in hits]
            rows.append((step_line(m, hits[-1], STEP_ASIDE), 0, False))
        elif m == 2:
            rows.append(([[(0.25, 0.25), (0.25, 0.25)]], 1, True))
        elif m == 3:
            rows.append(([[(-1.0, -20.0), (1.0, 20.0), (-1.0, -20.0)]], 2, True))
        else:   # and polygons that hold the queries, the one crossing counted at each of the same segments
            rows += [([step_ring(m, k, STEP_THROUGH)], 1, True) for k in hits]
            rows += [([step_ring(m, k, STEP_AROUND)], 0, True) for k in hits]
            rows.append(([step_ring(m, m - 2, STEP_ASIDE)], 0, False))
    return rows


@pytest.mark.parametrize("form", ["typed", "wkb"])
@pytest.mark.parametrize("kind", ["linestring", "polygon"])
def test_one_hit_at_each_step_boundary(gpu, oracle, kind, form):
    """Lines and single-ring polygons whose tuple counts sit at the edges of the 63-segment wave step, one
    segment alone meeting the query, at segment 0, at a step's last and next step's first segment, and at the
    final one; polygons that meet nothing and hold the box's corner / the query's first shell vertex, whose one
    crossing is counted at each of those segments in turn.  The box filter sends every run through the shared
    segment loop; the polygon filter only runs of more than 64 tuples (65, 127, 128 here), the shorter ones
    going lanes-over-entries.  Only the [a, a] ring is settled by an envelope shortcut (it is a point)."""
    import geom_intersects_ref as R
    from geomesa_amd.table import XZ2Table
    case = step_rows(kind)
    rows = [r for r, _, _ in case]
    q = P.queries()["concave"]
    runs = [r if kind == "linestring" else r[0] for r in rows]
    for run, (_, n_meet, exp) in zip(runs, case):      # the inputs, by the references alone
        segs = list(zip(run, run[1:]))
        assert sum(R.seg_meets_box(a, b, STEP_BOX) for a, b in segs) == n_meet
        assert sum(P._contact([a, b], q) for a, b in segs) == n_meet or len(run) == 2   # [a, a] inside: no contact
    exp = np.array([e for _, _, e in case])
    assert np.array_equal(R.scan(rows, kind, [STEP_BOX]), exp)
    assert np.array_equal(np.array([P.intersects_restated(r, kind, q) for r in rows]), exp)
    arr, col = (to_arrow(rows, kind), kind) if form == "typed" else (wkb_array(rows, kind), "wkb")
    tb = XZ2Table.from_geometries(arr, col)
    for got in (tb.query([STEP_BOX]), tb.query(polygons=q.polygon_set())):
        assert got[1] == exp.sum() and np.array_equal(np.sort(as_np(got[0])), np.nonzero(exp)[0])
        assert tb.n_envelope == len(rows)              # every feature reaches the walk


def collection_query():
    """Parts about the three sites of wkb_cases' mixed column: a star, a star with a hole, a rectangle; then
    six more small parts away from them, so that a polygon's first-vertex passes come in two groups."""
    import wkb_cases as C
    c = [((b[0] + b[2]) / 2, (b[1] + b[3]) / 2) for b in C.BOXES]
    parts = [[P.star(c[0], 2.5, 9, 1)], [P.star(c[1], 3.0, 33, 2), P.star(c[1], 1.0, 5, 3)],
             [[(c[2][0] - 1, c[2][1] - 1), (c[2][0] + 1, c[2][1] - 1), (c[2][0] + 1, c[2][1] + 1.5), (c[2][0] - 1, c[2][1] + 1.5),
               (c[2][0] - 1, c[2][1] - 1)]]]
    parts += [[P.star((c[k % 3][0] + 2.0 + 0.3 * k, c[k % 3][1] - 2.0), 0.2, 5, 10 + k)] for k in range(6)]
    return P.Query(parts)


def test_wkb_geometry_collections(gpu, oracle):
    """A column of every class, collections nested, every byte order and dimension: wkb_ref's reader plus the
    reference."""
    import wkb_cases as C
    import wkb_ref as W
    from geomesa_amd.table import XZ2Table
    blobs = C.mixed_column()
    geoms = [W.parse(b) for b in blobs]
    q = collection_query()
    exp = W.scan(geoms, [q], P.intersects_restated)
    env_hit = oracle.envelope_scan(*W.envelopes(geoms), q.boxes)
    assert sum(g is not None and g[0] == "collection" for g in geoms) >= 30
    assert exp.sum() >= 50 and (env_hit & ~exp).sum() >= 50 and not (exp & ~env_hit).any()
    tb = XZ2Table.from_geometries(pa.array(blobs, pa.binary()), "wkb")
    check(tb, tb.query(polygons=q.polygon_set()), exp, env_hit)


def test_wkb_malformed_slots_never_match(gpu, oracle):
    import wkb_cases as C
    import wkb_ref as W
    from geomesa_amd.table import XZ2Table
    blobs, bad = C.malformed_column()
    geoms = [W.parse(b) for b in blobs]
    tb = XZ2Table.from_geometries(pa.array(blobs, pa.binary()), "wkb")
    for q in (P.queries()["world"], P.Query([[P.star((4.0, 4.0), 6.0, 17, 5)]])):
        exp = W.scan(geoms, [q], P.intersects_restated)
        ids, nm, _ = tb.query(polygons=q.polygon_set())
        assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
        assert not set(as_np(ids).tolist()) & set(bad)
    assert W.scan(geoms, [P.queries()["world"]], P.intersects_restated).sum() >= 8


# ---------------------------------------------------------------- the C ABI
def raw_set(rings):
    """A PolygonSet of one part with these rings, as given: nothing closed or checked on the way."""
    from geomesa_amd.join import PolygonSet
    off = np.cumsum([0] + [len(r) for r in rings])
    xy = np.array([p for r in rings for p in r], np.float64).reshape(-1, 2)
    return PolygonSet([0, 1], [0, len(rings)], off, xy[:, 0], xy[:, 1])


def scan_c(ctx, tb, kr, f, ids=None, cap=None, geom=True):
    """gm_table_scan_geom (or gm_table_scan) as called from C: (rc, n_match, n_scanned, n_envelope)."""
    from geomesa_amd._lib import ptr
    nm, ns, ne = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    head = (ctx.handle, ptr(tb.shard), ptr(tb.bin), ptr(tb.z), tb.n, kr.ctypes.data, len(kr), ctypes.byref(f))
    tail = (ptr(tb.perm), ids, tb.n if cap is None else cap, ctypes.byref(nm), ctypes.byref(ns))
    if geom:
        rc = ctx.lib.gm_table_scan_geom(*head, ctypes.byref(tb.geom.c_struct()), *tail, ctypes.byref(ne))
    else:
        rc = ctx.lib.gm_table_scan(*head, *tail)
    return rc, nm.value, ns.value, ne.value


def test_abi_polys(gpu, oracle):
    from geomesa_amd import _lib
    from geomesa_amd.join import PolygonSet
    from geomesa_amd.table import _full_filter, key_ranges
    tb, q = xz2_case("polygon"), P.queries()["holed"]
    exp = np.nonzero(P.expected("polygon", "holed"))[0]
    kr, _ = key_ranges(tb.ks.get_ranges(tb.ks.get_index_values(q.boxes)), tb.shards)

    def filt(ps, **kw):
        f, keep = _full_filter(tb.env, None, perm=tb.perm, polys=ps)
        for k, v in kw.items():
            setattr(f, k, v)
        return f, keep
    good = PolygonSet.from_polygons(q.polygon_set())
    out = Guarded(8 * tb.n)
    f, keep = filt(good)
    rc, nm, ns, ne = scan_c(gpu, tb, kr, f, out.ptr)
    ids = out.read(np.int64)
    assert rc == 0 and nm == len(exp) <= ne <= ns and np.array_equal(np.sort(ids[:nm]), exp)
    assert untouched(ids[nm:])
    out.check("full capacity")
    # a short ids[]: the true count, a correct prefix, nothing past ids_cap
    cap = nm // 2
    short = Guarded(8 * cap)
    rc, nm2, _, ne2 = scan_c(gpu, tb, kr, f, short.ptr, cap)
    assert rc == _lib.GM_E_CAPACITY and nm2 == nm and ne2 == ne and np.array_equal(short.read(np.int64), ids[:cap])
    short.check("short capacity")
    rc, nm3, _, _ = scan_c(gpu, tb, kr, f, None)
    assert rc == 0 and nm3 == nm
    # every refusal is GM_E_INVALID with a text that names the entry
    box = np.array([P.RECT], np.float64)
    n_cap = _lib.GM_POLY_QUERY_MAX_VERTICES
    big = P.star(P.CENTRE, 8.0, n_cap + 1, 3)
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    cases = [(filt(good, boxes=box.ctypes.data, n_boxes=1), True, "polys and boxes together"),
             (filt(good), False, "polys needs the geometry column"),
             (filt(raw_set([sq + [(0.0, 0.5)]])), True, "not closed"),
             (filt(raw_set([[(0.0, 0.0), (1.0, 0.0), (0.0, 0.0)]])), True, "fewer than 4 tuples"),
             (filt(raw_set([sq[:2] + [(float("nan"), 1.0)] + sq[3:] + sq[:1]])), True, "NaN or infinite"),
             (filt(raw_set([big])), True, "more than GM_POLY_QUERY_MAX_VERTICES"),
             (filt(PolygonSet([0], [0], [0], [], [])), True, "at least one query polygon part")]
    for (f, keep), geom, text in cases:
        before = out.read(np.int64).copy()
        rc, *_ = scan_c(gpu, tb, kr, f, out.ptr, geom=geom)
        assert rc == _lib.GM_E_INVALID, text
        who = "gm_table_scan_geom: " if geom else "gm_table_scan: "
        assert _lib.last_error().startswith(who) and text in _lib.last_error(), (text, _lib.last_error())
        assert np.array_equal(out.read(np.int64), before)
    # exactly at the cap the set is taken
    f, keep = filt(raw_set([P.star(P.CENTRE, 8.0, n_cap, 3)]))
    rc, nm4, _, _ = scan_c(gpu, tb, kr, f, out.ptr)
    assert rc == 0 and nm4 > 0
    out.check("after the refusals")


# ---------------------------------------------------------------- Python
def test_python_argument_errors(gpu, oracle):
    from geomesa_amd.curve import IllegalArgumentException
    from geomesa_amd.table import XZ2Table
    tb, polys = xz2_case("linestring"), polygons_of("tri")
    with pytest.raises(IllegalArgumentException):
        tb.query(bboxes=[P.RECT], polygons=polys)
    with pytest.raises(IllegalArgumentException):
        tb.query(polygons=polys, exact=False)
    with pytest.raises(IllegalArgumentException):
        tb.query(polygons=[])
    env_only = XZ2Table(*(np.array(c) for c in ([0.0, 1.0], [0.0, 1.0], [2.0, 3.0], [2.0, 3.0])))
    with pytest.raises(IllegalArgumentException):
        env_only.query(polygons=polys)
    outside = [[[[(200.0, 0.0), (210.0, 0.0), (205.0, 10.0), (200.0, 0.0)]]]]
    ids, nm, scanned = tb.query(polygons=outside)
    assert ids.numel() == 0 and nm == 0 and scanned == 0
    # one part outside the world, one inside: the one inside answers
    ids, nm, _ = tb.query(polygons=outside + polys)
    exp = P.expected("linestring", "tri")
    assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])


def test_query_under_another_current_stream(gpu, oracle):
    import torch
    from geomesa_amd.table import XZ2Table
    rows, exp = P.features("polygon"), P.expected("polygon", "holed")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tb = XZ2Table.from_geometries(to_arrow(rows, "polygon"), "polygon")
        ids, nm, _ = tb.query(polygons=polygons_of("holed"))
        got = np.sort(as_np(ids))
    side.synchronize()
    assert nm == exp.sum() and np.array_equal(got, np.nonzero(exp)[0])
