"""The WKB reference (wkb_ref.py) and the test columns (wkb_cases.py) on the host, and the buffers a "wkb"
GeometryColumn points at.

The grammar is the one geomesa_hip.h states (OGC / ISO WKB plus the EWKB flag bits); agreement with JTS 1.20's
WKBReader itself is parity unpinned (JTS is outside the reference tree).  What the reference tree does pin: the
vector is an Arrow Binary column of WKBWriter output (WKBGeometryVector.java:27-93), and WKBWriter's default
is big-endian, two dimensions, no SRID -- the standard blobs of GeometryVectorTest.java:565-567's geometries."""
import math
import struct

import numpy as np
import pyarrow as pa
import pytest

import geom_intersects_ref as R
import wkb_cases as C
import wkb_ref as W

# GeometryVectorTest.java:565-567
POINT = ("point", (0.0, 20.0))
LINE = ("linestring", [(30.0, 10.0), (10.0, 30.0), (40.0, 45.0), (55.0, 60.0), (56.0, 60.0)])
POLYGON = ("polygon", [[(35.0, 10.0), (45.0, 45.0), (15.0, 40.0), (10.0, 20.0), (35.0, 10.0)],
                       [(20.0, 30.0), (35.0, 35.0), (30.0, 20.0), (20.0, 30.0)]])


def same(a, b):
    """Geometries equal with NaN == NaN."""
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack(">d", a) == struct.pack(">d", b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_standard_blobs_of_the_vector_tests_geometries():
    assert W.write(POINT).hex() == "00" + "00000001" + "0000000000000000" + "4034000000000000"
    assert len(W.write(POINT)) == 21
    line = W.write(LINE)
    assert line[:9].hex() == "00" + "00000002" + "00000005" and len(line) == 9 + 5 * 16
    assert line[9:25] == struct.pack(">dd", 30.0, 10.0) and line[-16:] == struct.pack(">dd", 56.0, 60.0)
    poly = W.write(POLYGON)
    assert poly[:13].hex() == "00" + "00000003" + "00000002" + "00000005" and len(poly) == 9 + 4 + 80 + 4 + 64
    assert poly[93:97].hex() == "00000004" and poly[97:113] == struct.pack(">dd", 20.0, 30.0)
    for g in (POINT, LINE, POLYGON):
        assert W.read(W.write(g)) == g
    assert W.envelope(LINE) == (10.0, 10.0, 56.0, 60.0) and W.envelope(POLYGON) == (10.0, 10.0, 45.0, 45.0)


def depth(g):
    """Collection levels: 0 for a Point, LineString or Polygon, 1 + its deepest element for codes 4 .. 7."""
    if g[0] in W.ELEMENT:
        return 1
    return 1 + max([depth(e) for e in g[1]] + [0]) if g[0] == "collection" else 0


@pytest.mark.parametrize("style", range(len(C.STYLES)))
def test_round_trips_in_every_style(style):
    s = C.STYLES[style]
    rng = np.random.default_rng(style)
    geoms = [g for g in (C.feature(rng, i) for i in range(16 * 12)) if g is not None]
    assert any(depth(g) > W.MAX_DEPTH for g in geoms)
    for pick in (None, C.alternate):
        for g in geoms:
            b = W.write(g, s, pick)
            if depth(g) > W.MAX_DEPTH:
                assert W.parse(b) is None
            else:
                assert same(W.read(b), g), (g, s.__dict__)
                assert same(W.read(b + b"\x09\x09\x09"), g)          # trailing bytes


def test_header_bits():
    z = W.write(POINT, W.Style(True, "z"))
    assert z[:5].hex() == "0101000080" and len(z) == 5 + 24
    assert W.write(POINT, W.Style(False, "zm", iso=True))[:5].hex() == "0000000bb9"
    assert W.write(POINT, W.Style(False, "m", iso=True))[:5].hex() == "00000007d1"
    s = W.write(POINT, W.Style(True, srid=4326))
    assert s[:9].hex() == "0101000020" + "e6100000" and len(s) == 9 + 16
    mixed = W.write(("collection", [POINT, LINE]), W.LE, C.alternate)
    assert mixed[0] == 1 and mixed[9] == 1 and mixed[9 + 21] == 0        # path (0,): k = 1, path (1,): k = 2
    assert W.read(mixed) == ("collection", [POINT, LINE])


def test_depth_limit():
    p = ("point", (1.0, 2.0))
    for d in (1, 2, W.MAX_DEPTH):
        assert W.read(W.write(C.nest(p, d))) == C.nest(p, d)
    assert W.parse(W.write(C.nest(p, W.MAX_DEPTH + 1))) is None
    assert W.parse(W.write(C.nest(("multipoint", []), W.MAX_DEPTH))) is None      # the Multi* is the ninth level
    assert W.read(W.write(C.nest(("multipoint", []), W.MAX_DEPTH - 1)))[0] == "collection"


def test_envelope_rules():
    nan = math.nan
    assert W.envelope(None) == W.NULL_ENV and W.envelope(W.EMPTY_POINT) == W.NULL_ENV
    for empty in ("linestring", "polygon", "multipoint", "multilinestring", "multipolygon", "collection"):
        assert W.envelope((empty, [])) == W.NULL_ENV
    assert W.envelope(("point", (3.0, nan))) == W.NULL_ENV
    # the first tuple initialises, a later NaN never widens
    e = W.envelope(("linestring", [(nan, 1.0), (5.0, 2.0)]))
    assert math.isnan(e[0]) and math.isnan(e[2]) and e[1] == 1.0 and e[3] == 2.0
    assert W.envelope(("linestring", [(5.0, 2.0), (nan, 1.0)])) == (5.0, 1.0, 5.0, 2.0)
    # a polygon's envelope is its shell's; a collection skips its null elements
    assert W.envelope(("polygon", [[(0.0, 0.0), (1.0, 1.0), (0.0, 0.0)], [(-9.0, -9.0), (9.0, 9.0), (-9.0, -9.0)]])) == \
        (0.0, 0.0, 1.0, 1.0)
    assert W.envelope(("collection", [W.EMPTY_POINT, ("linestring", []), ("point", (2.0, 3.0)), ("collection", [])])) == \
        (2.0, 3.0, 2.0, 3.0)
    # the typed rules and these agree on typed rows
    import oracle as O
    rows = [[(1.0, 2.0), (-3.0, 4.0)], [], [(0.0, 0.0)]]
    for r in rows:
        assert W.envelope(("linestring", r)) == O.jts_envelope(r, "linestring")


def test_intersects_rules():
    box = (0.0, 0.0, 1.0, 1.0)
    assert W.intersects(("linestring", [(0.5, 0.5)]), box) and not W.intersects(("linestring", [(2.0, 0.5)]), box)
    assert not W.intersects(None, box) and not W.intersects(W.EMPTY_POINT, box)
    far, hit = ("point", (5.0, 5.0)), ("linestring", [(-1.0, 0.5), (2.0, 0.5)])
    assert W.intersects(("collection", [far, C.nest(hit, 3)]), box) and not W.intersects(("collection", [far, far]), box)
    assert not W.intersects(("collection", []), box)
    for fn in (R.intersects_exact, R.intersects_restated):
        assert W.intersects(("polygon", C.ell((1.0, 1.0), False)), (-1.6, -1.6, -1.0, -1.0), fn)       # in the corner block
        assert not W.intersects(("polygon", C.ell((1.0, 1.0), False)), (0.0, 0.0, 1.0, 1.0), fn)       # in the notch
        assert not W.intersects(("polygon", C.ell((1.0, 1.0), True)), (-1.6, -1.6, -1.0, -1.0), fn)    # in the hole


def test_mixed_column_holds_what_the_gpu_tests_need():
    blobs = C.mixed_column()
    geoms = [W.parse(b) for b in blobs]
    assert len(blobs) >= C.LANE_SLOTS
    tops = {g[0] for g in geoms if g is not None}
    assert tops == set(W.CODES)
    assert {1, 2, W.MAX_DEPTH} <= {depth(g) for g in geoms if g is not None}
    assert sum(1 for b, g in zip(blobs, geoms) if b is not None and g is None) >= 2          # depth 9
    assert sum(1 for b in blobs if b is None) >= 2
    lines = {len(g[1]) for g in geoms if g is not None and g[0] == "linestring"}
    assert set(C.LINE_TUPLES) | {0} <= lines
    for empty in (W.EMPTY_POINT, ("polygon", []), ("multipoint", []), ("multilinestring", []), ("multipolygon", []),
                  ("collection", [])):
        assert any(same(g, empty) for g in geoms)
    starts = np.cumsum([0] + [len(b or b"") for b in blobs])[:-1]
    assert set((starts % 8).tolist()) == set(range(8))
    assert {b[0] for b in blobs if b} == {0, 1}


@pytest.mark.parametrize("q", list(C.QUERIES))
def test_mixed_column_keeps_the_shortcuts_from_hiding_the_walk(q):
    """Of a query's envelope survivors at least a quarter fail the exact test, and at least a quarter pass it
    although their envelope is inside none of the boxes; both references agree on every slot."""
    geoms = [W.parse(b) for b in C.mixed_column()]
    boxes = C.QUERIES[q]
    C.check_shortcut_coverage(geoms, boxes)
    assert np.array_equal(W.scan(geoms, boxes), W.scan(geoms, boxes, R.intersects_exact))


def test_malformed_column():
    blobs, bad = C.malformed_column()
    for i in bad:
        assert W.parse(blobs[i]) is None, i
    # every truncated slot is followed by the bytes that complete it
    whole = [W.parse(blobs[i] + blobs[i + 1]) for i in bad[:50]]
    assert all(g is not None and W.envelope(g) != W.NULL_ENV for g in whole)
    assert sum(len(b) for b in blobs) < 1 << 20


def test_wkb_column_buffers_of_a_sliced_array_with_nulls():
    from geomesa_amd import _lib
    from geomesa_amd.arrow import KINDS, arrow_buffers
    from geomesa_amd.curve import IllegalArgumentException
    assert KINDS["wkb"] == 16 == _lib.GM_GEOM_WKB
    blobs = [W.write(POINT), None, W.write(LINE), b"", W.write(POLYGON, W.LE), None, W.write(POINT, W.LE) + b"xyz"]
    arr = pa.array(blobs, pa.binary())
    for a, b in [(0, 7), (1, 6), (2, 3), (4, 4)]:
        s = arr.slice(a, b - a)
        data, bits, valid, voff, offs = arrow_buffers(s, "wkb")
        assert bits == 64 and len(offs) == 1 and offs[0].dtype == np.int32 and len(offs[0]) == b - a + 1
        assert data.dtype == np.uint8
        got = []
        for i in range(b - a):
            ok = valid is None or (valid[(voff + i) >> 3] >> ((voff + i) & 7)) & 1
            got.append(bytes(data[offs[0][i]:offs[0][i + 1]]) if ok else None)
        assert got == blobs[a:b]
    with pytest.raises(IllegalArgumentException):
        arrow_buffers(pa.array(blobs, pa.large_binary()), "wkb")
    with pytest.raises(IllegalArgumentException):
        arrow_buffers(pa.array(["a"], pa.string()), "wkb")
