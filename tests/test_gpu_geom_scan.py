"""GPU parity of the exact full filter: gm_arrow_envelopes, gm_table_scan_geom and the XZ tables built from
geometries (XZ2Table / XZ3Table.from_geometries, query(exact=...)).

Every query result equals geom_intersects_ref.intersects_restated over EVERY feature (a full scan), ANDed
with FastDuring where a query has an interval -- which also proves the ranges cover every matching key.
The features carry the tuple counts at which the kernel's walk changes shape (one lane, a partial wave,
exactly one 64-segment step, several strides), rings with holes, multi geometries, null slots and empty
geometries; a third of them sit on a 1/4 lattice the query boxes share, so segments run through box corners
and along box edges.

For each kind and query the INPUTS are first checked against the reference alone: at least 50 features
whose envelope meets the box while the geometry does not, and at least 50 that match.  Two counts are
impossible by the definition and left out: a point is its own envelope (no envelope-only hits), and nothing
non-empty misses the whole world.  Every other (kind, query) pair has both, by planting where chance does
not give them: around each of the two small-box sites 60 features that surround the box without touching
it (rings of lines and points; polygons with the box in a hole) and 60 that meet it (lines through it, a
point in it, polygons holding it in their body, where the corner rule alone decides)."""
import ctypes
import functools

import numpy as np
import pyarrow as pa
import pytest

import geom_intersects_ref as R

pytestmark = pytest.mark.gpu

KINDS = ["point", "linestring", "polygon", "multipoint", "multilinestring", "multipolygon"]
DEPTH = {"point": 0, "linestring": 1, "multipoint": 1, "polygon": 2, "multilinestring": 2, "multipolygon": 3}
COUNTS = [2, 3, 4, 5, 63, 64, 65, 128, 129, 1000]
SITE_A, SITE_B = (24.0, 0.0), (-24.0, 0.0)      # the two small-box sites of the planted features
WORLD = (-180.0, -90.0, 180.0, 90.0)
QUERIES = {
    "one": [(-1.5, -1.0, 0.75, 1.25)],
    "two": [(-9.0, -6.0, -7.0, -4.25), (5.0, 1.0, 7.5, 3.0)],
    "five": [(-12.0, 3.0, -10.0, 5.0), (-2.0, -8.0, 0.0, -6.5), (0.5, -5.0, 2.5, -3.0), (9.0, -4.0, 11.0, -1.25),
             (-6.25, 5.0, -4.0, 7.0)],
    "interior": [(SITE_A[0] - 0.1, -0.1, SITE_A[0] + 0.1, 0.1)],
    "hole": [(SITE_B[0] - 0.1, -0.1, SITE_B[0] + 0.1, 0.1)],
    "zero_width": [(1.25, -2.0, 1.25, 1.5)],
    "world": [WORLD],
}
WEEK_MS = 604800000
T0 = 2600 * WEEK_MS


def as_np(t):
    return t.detach().cpu().numpy()


def arrow_type(kind, f32):
    t = pa.list_(pa.float32() if f32 else pa.float64(), 2)
    for _ in range(DEPTH[kind]):
        t = pa.list_(t)
    return t


def to_arrow(rows, kind, f32=False, flip=False):
    """Rows of (x, y) nests (None: a null slot) -> the geomesa-arrow-jts vector ([y, x] tuples unless flip)."""
    def conv(v, depth):
        if depth == 0:
            return [v[0], v[1]] if flip else [v[1], v[0]]
        return [conv(c, depth - 1) for c in v]
    return pa.array([None if r is None else conv(r, DEPTH[kind]) for r in rows], arrow_type(kind, f32))


def draw_count(rng):
    return 1000 if rng.random() < 0.01 else int(rng.choice(COUNTS[:-1]))


def arc(rng, c, rad, m, snap, closed):
    """m tuples around c: an arc of up to 0.9 pi (a line) or a star-shaped ring (closed: first = last)."""
    if closed and m < 4:      # a degenerate ring: [a, a] or [a, b, a]
        a = (c[0] + rad, c[1])
        return [a, a] if m == 2 else [a, (c[0], c[1] + rad), a]
    k = m - 1 if closed else m
    th = np.sort(rng.uniform(0, 2 * np.pi, k)) if closed else rng.uniform(0, 2 * np.pi) + np.sort(
        rng.uniform(0, rng.uniform(0.05, 0.9) * np.pi, k))
    r = rad * rng.uniform(0.55, 1.0, k)
    x, y = c[0] + r * np.cos(th), c[1] + r * np.sin(th)
    if snap:
        x, y = np.round(x * 4) / 4, np.round(y * 4) / 4
    pts = list(zip(x.tolist(), y.tolist()))
    return pts + [pts[0]] if closed else pts


def polygon(rng, c, rad, snap, holes):
    rings = [arc(rng, c, rad, draw_count(rng), snap, True)]
    if len(rings[0]) < 63:      # few vertices: the shell's chords cut inside its inner radius, no room for holes
        holes = 0
    for h in range(holes):      # holes inside the shell's inner radius (0.55 rad), apart from each other
        a = 2 * np.pi * h / 3
        hc = (c[0] + 0.25 * rad * np.cos(a), c[1] + 0.25 * rad * np.sin(a))
        rings.append(arc(rng, hc, 0.15 * rad, draw_count(rng), False, True))
    return rings


def feature(rng, kind, c, rad, snap):
    if kind == "point":
        return (round(c[0] * 4) / 4, round(c[1] * 4) / 4) if snap else c
    if kind == "multipoint":
        return arc(rng, c, rad, draw_count(rng), snap, False)
    if kind == "linestring":
        return arc(rng, c, rad, draw_count(rng), snap, False)
    if kind == "polygon":
        return polygon(rng, c, rad, snap, int(rng.integers(0, 4)))
    parts = []
    for p in range(int(rng.integers(1, 5))):
        pc = (c[0] + (p % 2) * 0.9 * rad, c[1] + (p // 2) * 0.9 * rad)
        parts.append(arc(rng, pc, 0.6 * rad, draw_count(rng), snap, False) if kind == "multilinestring"
                     else polygon(rng, pc, 0.4 * rad, snap, int(rng.integers(0, 3))))
    return parts


def planted(rng, kind, site, through):
    """A feature of radius 2.75 - 8 around a site whose small box no ring of it comes near.  through: it meets
    the box all the same -- a polygon by holding it in its body, a line by running straight through the site,
    a multipoint by a point on the site; else it surrounds the box: a polygon with a hole of radius >= 0.8
    about the site, a closed ring of segments or of points."""
    rad, m = rng.uniform(5.0, 8.0), int(rng.choice([64, 65, 129]))
    ring = arc(rng, site, rad, m, False, True)
    if kind in ("polygon", "multipolygon"):
        rings = [ring] if through else [ring, arc(rng, site, rng.uniform(1.5, 2.5), 64, False, True)]
        return rings if kind == "polygon" else [rings]
    if kind == "multipoint":
        return ring + [site] if through else ring
    if through:
        th, m = rng.uniform(0, np.pi), int(rng.choice([2, 3, 64, 65, 129]))
        t = np.sort(np.concatenate([[-1.0, 1.0], rng.uniform(-1, 1, m - 2)])) * rad
        ring = list(zip((site[0] + t * np.cos(th)).tolist(), (site[1] + t * np.sin(th)).tolist()))
    return ring if kind == "linestring" else [ring]


# random features per kind: enough for 50 envelope-only hits and 50 matches of every query's small boxes
N_RANDOM = {"point": 8000, "linestring": 3000, "polygon": 1800, "multipoint": 1800, "multilinestring": 1800,
            "multipolygon": 1900}


def make_rows(kind, seed, f32=False, n_random=None):
    rng = np.random.default_rng(seed)
    rows = []
    n_random = n_random or N_RANDOM[kind]
    for i in range(n_random):
        if rng.random() < 0.03:
            rows.append(None if (kind == "point" or rng.random() < 0.6) else [])   # null slot / empty geometry
            continue
        c = (rng.uniform(-15, 15), rng.uniform(-10, 10))
        rows.append(feature(rng, kind, c, rng.uniform(2.0, 9.0), rng.random() < 0.33))
    if kind == "multipoint":    # one point on the zero-width box, the others around it
        rows += [arc(rng, (1.25, 0.0), rng.uniform(3.0, 6.0), 5, False, False) + [(1.25, float(y))]
                 for y in rng.uniform(-2.0, 1.5, 60)]
    if kind == "point":
        rows += [(1.25, float(y)) for y in rng.uniform(-2.5, 2.0, 80)]            # on the zero-width box's line
        rows += [(s[0] + float(dx), float(dy)) for s in (SITE_A, SITE_B) for dx, dy in rng.uniform(-0.1, 0.1, (60, 2))]
    else:
        rows += [planted(rng, kind, s, through) for s in (SITE_A, SITE_B) for through in (False, True)
                 for _ in range(60)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    if f32:     # the values a Float4 vector holds
        def r32(v, depth):
            if depth == 0:
                return (float(np.float32(v[0])), float(np.float32(v[1])))
            return [r32(c, depth - 1) for c in v]
        rows = [None if r is None else r32(r, DEPTH[kind]) for r in rows]
    return rows


def envelopes_of(oracle, rows, kind):
    e = np.array([(0.0, 0.0, -1.0, -1.0) if r is None else oracle.jts_envelope(r, kind) for r in rows])
    return e[:, 0], e[:, 1], e[:, 2], e[:, 3]


@functools.lru_cache(maxsize=None)
def xz2_case(kind):
    """One table per kind, shared by its queries: (rows, envelope columns, XZ2Table)."""
    import oracle as O
    from geomesa_amd.table import XZ2Table
    rows = make_rows(kind, 100 + KINDS.index(kind))
    arr = to_arrow(rows, kind)
    assert O.arrow_rows(arr, kind) == rows
    n = len(rows)
    sh = (np.arange(n) * 2654435761 % 4).astype(np.uint8)
    return rows, envelopes_of(O, rows, kind), XZ2Table.from_geometries(arr, kind, shard=sh, shards=4)


def check_inputs(kind, q, env_hit, exp, rows, boxes):
    """The conditions on the inputs (reference only): at least 50 envelope-only hits and 50 matches."""
    miss, hit = int((env_hit & ~exp).sum()), int(exp.sum())
    if kind != "point" and q != "world":      # a point is its own envelope; nothing misses the world
        assert miss >= 50, (kind, q, miss)
    assert hit >= 50, (kind, q, hit)
    if q in ("interior", "hole") and kind in ("polygon", "multipolygon"):
        # the corner rule alone: matches none of whose ring segments meets the box
        alone = sum(1 for r, e in zip(rows, exp) if e and not any(
            R.seg_meets_box(a, b, boxes[0]) for p in (r if kind == "multipolygon" else [r]) for ring in p
            for a, b in zip(ring, ring[1:])))
        assert alone >= 50, (kind, q, alone)


# ---------------------------------------------------------------- gm_arrow_envelopes
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_arrow_envelopes(gpu, oracle, kind, f32, flip):
    """gm_arrow_envelopes = oracle.jts_envelope per slot (null and empty slots: 0, 0, -1, -1), Float8 and
    Float4, both axis orders, and a sliced array whose offset is not zero."""
    from geomesa_amd import arrow as A
    rows = make_rows(kind, 7, f32, n_random=300)
    for arr, rr in ((to_arrow(rows, kind, f32, flip), rows), (to_arrow(rows, kind, f32, flip).slice(37, 211), rows[37:248])):
        got = np.stack([as_np(c) for c in A.envelopes(arr, kind, flip_axis=flip)], 1)
        exp = np.stack(envelopes_of(oracle, rr, kind), 1)
        assert got.shape == exp.shape and np.array_equal(got, exp)


# ---------------------------------------------------------------- XZ2 tables, all kinds x queries
@pytest.mark.parametrize("q", list(QUERIES))
@pytest.mark.parametrize("kind", KINDS)
def test_xz2_from_geometries_query(gpu, oracle, kind, q):
    rows, env, tb = xz2_case(kind)
    boxes = QUERIES[q]
    exp = R.scan(rows, kind, boxes)
    env_hit = oracle.envelope_scan(*env, boxes)
    assert not (exp & ~env_hit).any()
    check_inputs(kind, q, env_hit, exp, rows, boxes)
    ids, nm, scanned = tb.query(boxes)
    assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
    assert tb.n_envelope == env_hit.sum() and nm <= tb.n_envelope <= scanned
    ids, nm, _ = tb.query(boxes, exact=False)      # the envelope filter is still there, unchanged
    assert nm == env_hit.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(env_hit)[0])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("kind", ["linestring", "multipolygon"])
def test_xz2_float4_and_flip(gpu, oracle, kind, flip):
    """Float4 ordinates (widened on read) and flipAxisOrder through the table."""
    from geomesa_amd.table import XZ2Table
    rows = make_rows(kind, 55, True, n_random=500)
    tb = XZ2Table.from_geometries(to_arrow(rows, kind, True, flip), kind, flip_axis=flip)
    for q in ("one", "five", "hole"):
        exp = R.scan(rows, kind, QUERIES[q])
        ids, nm, _ = tb.query(QUERIES[q])
        assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])


# ---------------------------------------------------------------- XZ3 tables and the C ABI
def scan_geom(ctx, tb, arr, f, geom, perm, ids_cap=None, want_ids=True):
    """gm_table_scan_geom as called from C: (rc, ids, n_match, n_scanned, n_envelope)."""
    import torch
    from geomesa_amd._lib import ptr
    cap = tb.n if ids_cap is None else ids_cap
    ids = torch.full((max(tb.n, 1) + 8,), -7, dtype=torch.int64, device="cuda")
    nm, ns, ne = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = ctx.lib.gm_table_scan_geom(ctx.handle, ptr(tb.shard), ptr(tb.bin), ptr(tb.z), tb.n,
                                    arr.ctypes.data if len(arr) else None, len(arr),
                                    ctypes.byref(f) if f is not None else None,
                                    ctypes.byref(geom) if geom is not None else None, ptr(perm),
                                    ptr(ids) if want_ids else None, cap, ctypes.byref(nm), ctypes.byref(ns),
                                    ctypes.byref(ne))
    return rc, as_np(ids), nm.value, ns.value, ne.value


@functools.lru_cache(maxsize=None)
def xz3_rows(kind):
    import oracle as O
    rows = make_rows(kind, 300 + KINDS.index(kind))
    rng = np.random.default_rng(31)
    t = T0 + rng.integers(WEEK_MS // 4, 6 * WEEK_MS, len(rows))
    t[:300] = T0 + 1500 + np.arange(300) % 3 - 1          # at and around an exclusive bound
    return rows, t, to_arrow(rows, kind), envelopes_of(O, rows, kind)


@functools.lru_cache(maxsize=None)
def xz3_case(kind, sharded):
    from geomesa_amd.table import XZ3Table
    rows, t, arr, env = xz3_rows(kind)
    sh = (np.arange(len(rows)) * 2654435761 % 4).astype(np.uint8) if sharded else None
    return rows, t, arr, env, XZ3Table.from_geometries(arr, t, kind, shard=sh, shards=4 if sharded else None)


# each query's DURING: ms edges at T0 + 1500, several bins, one without a dtg term
XZ3_DURING = {"one": (T0 + 1500, T0 + 6 * WEEK_MS), "two": (T0 + 1500, T0 + 5 * WEEK_MS + 999),
              "five": (T0 + WEEK_MS // 8, T0 + 6 * WEEK_MS), "interior": (T0 + 1500, T0 + 6 * WEEK_MS), "hole": None,
              "zero_width": (T0 + 1500, T0 + 6 * WEEK_MS), "world": (T0 + 2 * WEEK_MS, T0 + 3 * WEEK_MS)}


@pytest.mark.parametrize("q", list(QUERIES))
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("kind", ["linestring", "polygon", "multipolygon"])
def test_xz3_from_geometries_query(gpu, oracle, kind, sharded, q):
    """XZ3Table.from_geometries(...).query with during, on inputs that hold the same counts once the dtg term
    is applied; then the same scan through the C ABI with the columns reached the other two ways: f.rows set
    and perm NULL (ids are table rows), and both NULL over columns put into table order."""
    import torch
    from geomesa_amd import arrow as A
    from geomesa_amd.keyspace import during
    from geomesa_amd.table import _full_filter, key_ranges
    rows, t, arr, env, tb = xz3_case(kind, sharded)
    boxes, iv = QUERIES[q], XZ3_DURING[q]
    exp = R.scan(rows, kind, boxes)
    env_hit = oracle.envelope_scan(*env, boxes, t, iv)
    if iv is not None:
        exp &= (t > iv[0]) & (t < iv[1])
    check_inputs(kind, q, env_hit, exp, rows, boxes)
    ids, nm, scanned = tb.query(boxes, iv)
    assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
    assert tb.n_envelope == env_hit.sum()
    # f.rows = perm, perm NULL: the ids are table rows, in table order
    v = tb.ks.get_index_values(boxes, [during(*iv)] if iv is not None else None)
    kr, _ = key_ranges(tb.ks.get_ranges(v), tb.shards)
    f, keep = _full_filter(tb.env, v.spatialBounds, iv, tb.t, tb.perm)
    rc, tids, nm2, _, ne2 = scan_geom(gpu, tb, kr, f, tb.geom.c_struct(), None)
    perm = as_np(tb.perm)
    assert rc == 0 and nm2 == nm and ne2 == env_hit.sum()
    assert np.all(np.diff(tids[:nm2]) > 0) and np.array_equal(np.sort(perm[tids[:nm2]]), np.nonzero(exp)[0])
    # columns in table order, rows and perm NULL
    tarr = arr.take(pa.array(perm))
    tcol = A.GeometryColumn(tarr, kind)
    tenv = A.envelopes(tcol, kind)
    tt = torch.from_numpy(t[perm]).cuda()
    f, keep = _full_filter(tenv, v.spatialBounds, iv, tt, None)
    rc, tids3, nm3, _, ne3 = scan_geom(gpu, tb, kr, f, tcol.c_struct(), None)
    assert rc == 0 and nm3 == nm and ne3 == ne2 and np.array_equal(tids3[:nm3], tids[:nm2])


def test_abi_contract(gpu, oracle):
    """n_envelope is gm_table_scan's n_match; a short ids[] gives GM_E_CAPACITY with the true count and a
    correct prefix, nothing written past ids_cap; ids NULL counts; a query whose envelope pass keeps nothing."""
    from geomesa_amd import _lib
    from geomesa_amd.table import _full_filter, key_ranges
    rows, env, tb = xz2_case("polygon")
    boxes = QUERIES["two"]
    exp = np.nonzero(R.scan(rows, "polygon", boxes))[0]
    v = tb.ks.get_index_values(boxes)
    kr, _ = key_ranges(tb.ks.get_ranges(v), tb.shards)
    f, keep = _full_filter(tb.env, v.spatialBounds, perm=tb.perm)
    g = tb.geom.c_struct()
    _, n_env_scan, _ = tb.table_scan(kr, f)
    rc, ids, nm, ns, ne = scan_geom(gpu, tb, kr, f, g, tb.perm)
    assert rc == 0 and ne == n_env_scan and nm == len(exp) <= ne <= ns
    assert np.array_equal(np.sort(ids[:nm]), exp) and np.all(ids[nm:] == -7)
    cap = nm // 2
    rc, short, nm2, _, ne2 = scan_geom(gpu, tb, kr, f, g, tb.perm, ids_cap=cap)
    assert rc == _lib.GM_E_CAPACITY and nm2 == nm and ne2 == ne
    assert np.array_equal(short[:cap], ids[:cap]) and np.all(short[cap:] == -7)
    rc, untouched, nm3, _, _ = scan_geom(gpu, tb, kr, f, g, tb.perm, want_ids=False)
    assert rc == 0 and nm3 == nm and np.all(untouched == -7)
    # zero survivors of the envelope pass: a box in the scanned key space that no envelope meets
    far = [(100.0, 50.0, 101.0, 51.0)]
    assert not oracle.envelope_scan(*env, far).any()
    v = tb.ks.get_index_values(far)
    kr2, _ = key_ranges(tb.ks.get_ranges(v), tb.shards)
    f2, keep2 = _full_filter(tb.env, far, perm=tb.perm)
    rc, ids4, nm4, ns4, ne4 = scan_geom(gpu, tb, np.concatenate([kr, kr2]), f2, g, tb.perm)
    assert rc == 0 and nm4 == 0 and ne4 == 0 and ns4 > 0 and np.all(ids4 == -7)


def test_abi_invalid_arguments(gpu):
    """Every GM_E_INVALID precondition of gm_table_scan_geom, each with a gm_last_error text."""
    from geomesa_amd import _lib
    from geomesa_amd.table import _full_filter, key_ranges
    rows, env, tb = xz2_case("linestring")
    kr, _ = key_ranges([("bounded", (0, 0), (0, -1))], tb.shards)
    good, keep = _full_filter(tb.env, QUERIES["one"], perm=tb.perm)
    g = tb.geom.c_struct()

    def copy_of(s, **kw):
        c = type(s)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(s), ctypes.sizeof(s))
        for k, val in kw.items():
            setattr(c, k, val)
        return c
    assert scan_geom(gpu, tb, kr, good, g, tb.perm)[0] == 0
    buf = ctypes.create_string_buffer(8)
    both = dict(z3filter=ctypes.addressof(buf), z3filter_len=8, z2filter=ctypes.addressof(buf), z2filter_len=8)
    cols = "the boxes and the four envelope columns"
    col = {c: (copy_of(good, **{c: None}), g, cols) for c in ("xmin", "ymin", "xmax", "ymax", "boxes")}
    cases = [(None, g, "the filter"), col["xmin"], (copy_of(good, n_boxes=0), g, "at least one query box"), col["ymin"],
             (good, None, "the geometry column"), col["xmax"], (good, copy_of(g, ordinal_bits=16), "ordinal_bits"),
             col["ymax"], (good, copy_of(g, type=6), "unknown geometry type"), col["boxes"],
             (good, copy_of(g, type=-1), "unknown geometry type"), (good, copy_of(g, coords=None), "coords"),
             (copy_of(good, **both), g, "a Z3Filter and a Z2Filter together")]   # from the body the entries share
    # no two neighbours share a text, so a case that set none would be caught on its predecessor's
    assert all(a[2] != b[2] for a, b in zip(cases, cases[1:]))
    for f, gc, text in cases:
        assert scan_geom(gpu, tb, kr, f, gc, tb.perm)[0] == _lib.GM_E_INVALID
        assert _lib.last_error().startswith("gm_table_scan_geom: ") and text in _lib.last_error(), (text, _lib.last_error())


# ---------------------------------------------------------------- the reference's own features
def test_xz2_strategy_polygons_through_the_table(gpu):
    """XZ2IdxStrategyTest.scala:74-79, 88-93, 102-107, 132-136 through XZ2Table.from_geometries."""
    from geomesa_amd.table import XZ2Table
    ids, rows, queries = R.xz2_strategy_polygons()
    tb = XZ2Table.from_geometries(to_arrow(rows, "polygon"), "polygon")
    for box, exp in queries:
        got, nm, _ = tb.query([box])
        assert sorted(ids[i] for i in as_np(got)) == exp and nm == len(exp)


def test_xz3_index_linestrings_through_the_table(gpu):
    """XZ3IndexTest.scala:38-47, 54-64 (a yearly period) through XZ3Table.from_geometries."""
    from geomesa_amd.table import XZ3Table
    rows, t, queries = R.xz3_index_linestrings()
    tb = XZ3Table.from_geometries(to_arrow(rows, "linestring"), np.array(t, np.int64), "linestring", period="year")
    for box, iv, exp in queries:
        got, nm, _ = tb.query([box], iv)
        assert sorted(as_np(got).tolist()) == exp and nm == len(exp)


# ---------------------------------------------------------------- the default did not move
def test_envelope_table_keeps_the_envelope_filter(gpu, oracle):
    """XZ2Table(xmin, ...) without geometries still answers with oracle.envelope_scan: LINESTRING(0 0, 10 10)
    against bbox(8, 0, 10, 2) comes back from the envelope table and not from the geometry table, and
    exact=True on the envelope table is an IllegalArgumentException."""
    from geomesa_amd.curve import IllegalArgumentException
    from geomesa_amd.table import XZ2Table
    rows = [[(0.0, 0.0), (10.0, 10.0)], [(8.5, 0.5), (9.0, 1.0)], [(20.0, 0.0), (30.0, 10.0)]]
    box = [(8.0, 0.0, 10.0, 2.0)]
    env = envelopes_of(oracle, rows, "linestring")
    tb = XZ2Table(*env)
    ids, nm, _ = tb.query(box)
    exp = np.nonzero(oracle.envelope_scan(*env, box))[0]
    assert exp.tolist() == [0, 1] and nm == 2 and np.array_equal(np.sort(as_np(ids)), exp)
    with pytest.raises(IllegalArgumentException):
        tb.query(box, exact=True)
    ids, nm, _ = XZ2Table.from_geometries(to_arrow(rows, "linestring"), "linestring").query(box)
    assert nm == 1 and as_np(ids).tolist() == [1]
