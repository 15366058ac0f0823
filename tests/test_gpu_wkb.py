"""GPU parity of GM_GEOM_WKB columns (WKBGeometryVector as gm_geom_column type 16): gm_arrow_envelopes,
gm_xz2_index_key_arrow / gm_xz3_index_key_arrow, gm_arrow_points_to_columns and the exact box filter
gm_table_scan_geom through XZ2Table / XZ3Table.from_geometries(..., "wkb").

  * differential: the typed suites' own features (test_gpu_geom_scan.make_rows: every tuple count at which
    the typed walk changes shape, holes, multi geometries, null slots, empty geometries, a lattice the boxes
    share) written as WKB give bit-identical envelopes, identical keys and statuses, and the same ids,
    n_match and n_envelope for every query of that suite.  Its input conditions (50 envelope-only hits and
    50 matches per kind and query) are asserted there;
  * the columns of wkb_cases.py against wkb_ref.py: all seven codes in one column, nesting 1, 2, 8 and 9
    deep, every encoding style, every slot start mod 8, 2 * 256 + 5 slots and more, lines of 1 .. 130 tuples,
    null slots and a validity offset, special ordinates by bit pattern, and malformed slots whose following
    bytes would complete a valid geometry.  Each refine query first asserts, from the reference alone, that
    a quarter of its envelope survivors fail the exact test and a quarter pass it with an envelope that is
    inside no box (wkb_cases.check_shortcut_coverage), so the shortcuts cannot hide the walk.
"""
import ctypes
import functools

import numpy as np
import pyarrow as pa
import pytest

import test_gpu_geom_scan as G
import wkb_cases as C
import wkb_ref as W

pytestmark = pytest.mark.gpu

WORLD = [(-180.0, -90.0, 180.0, 90.0)]
T0 = G.T0


def as_np(t):
    return t.detach().cpu().numpy()


def bits(cols):
    """Device float64 columns -> one uint64 array, for comparison by bit pattern."""
    return np.stack([as_np(c).view(np.uint64) for c in cols], 1)


def wkb_array(blobs):
    return pa.array(blobs, pa.binary())


def typed_as_wkb(rows, kind):
    """The rows of a typed column as WKB slots, byte order alternating."""
    return wkb_array([None if r is None else W.write((kind, r), W.LE if i & 1 else W.BE) for i, r in enumerate(rows)])


def times(n):
    return T0 + (np.arange(n, dtype=np.int64) * 7919 % 4) * (G.WEEK_MS // 5)


# ---------------------------------------------------------------- differential: typed column vs WKB column
@pytest.mark.parametrize("kind", G.KINDS)
def test_typed_and_wkb_columns_agree_xz2(gpu, kind):
    from geomesa_amd import arrow as A
    from geomesa_amd.table import XZ2Table
    rows, _, tb = G.xz2_case(kind)
    typed, wkb = tb.geom, A.GeometryColumn(typed_as_wkb(rows, kind), "wkb")
    assert np.array_equal(bits(A.envelopes(wkb, "wkb")), bits(A.envelopes(typed, kind)))
    for lenient in (False, True):
        zt, st = A.xz2_index_keys(typed, kind, lenient=lenient, status=True)
        zw, sw = A.xz2_index_keys(wkb, "wkb", lenient=lenient, status=True)
        assert np.array_equal(as_np(zw), as_np(zt)) and np.array_equal(as_np(sw), as_np(st))
    t = pa.array(times(len(rows)))
    for got, exp in zip(A.xz3_index_keys(wkb, t, "wkb", status=True), A.xz3_index_keys(typed, t, kind, status=True)):
        assert np.array_equal(as_np(got), as_np(exp))
    assert {0, W.NULL_GEOM} <= set(as_np(sw).tolist()) and (kind == "point" or W.UNORDERED in as_np(sw))
    sh = (np.arange(len(rows)) * 2654435761 % 4).astype(np.uint8)
    wt = XZ2Table.from_geometries(wkb, "wkb", shard=sh, shards=4)
    for q, boxes in G.QUERIES.items():
        ids, nm, _ = tb.query(boxes)
        wids, wnm, _ = wt.query(boxes)
        assert wnm == nm and wt.n_envelope == tb.n_envelope, (kind, q)
        assert np.array_equal(np.sort(as_np(wids)), np.sort(as_np(ids))), (kind, q)


@pytest.mark.parametrize("kind", ["linestring", "polygon", "multipolygon"])
def test_typed_and_wkb_columns_agree_xz3(gpu, kind):
    from geomesa_amd.table import XZ3Table
    rows, t, _, _, tb = G.xz3_case(kind, False)
    wt = XZ3Table.from_geometries(typed_as_wkb(rows, kind), t, "wkb")
    for q, boxes in G.QUERIES.items():
        ids, nm, _ = tb.query(boxes, G.XZ3_DURING[q])
        wids, wnm, _ = wt.query(boxes, G.XZ3_DURING[q])
        assert wnm == nm and wt.n_envelope == tb.n_envelope, (kind, q)
        assert np.array_equal(np.sort(as_np(wids)), np.sort(as_np(ids))), (kind, q)


# ---------------------------------------------------------------- the mixed column against wkb_ref
@functools.lru_cache(maxsize=None)
def mixed():
    blobs = C.mixed_column()
    return blobs, [W.parse(b) for b in blobs]


def expect_points(geoms):
    xy = np.full((len(geoms), 2), np.nan)
    for i, g in enumerate(geoms):
        if g is not None and g[0] == "point" and not (np.isnan(g[1][0]) or np.isnan(g[1][1])):
            xy[i] = g[1]
    return xy


def check_column(blobs, geoms, g=12):
    """Envelopes, XZ2 / XZ3 keys and statuses and the point adapter of a column against the reference."""
    from geomesa_amd import arrow as A
    col = A.GeometryColumn(wkb_array(blobs), "wkb")
    exp = np.stack(W.envelopes(geoms), 1)
    assert np.array_equal(bits(A.envelopes(col, "wkb")), exp.view(np.uint64))
    z, st = A.xz2_index_keys(col, "wkb", g=g, status=True)
    ez, est = W.xz2_keys(geoms, g=g)
    assert np.array_equal(as_np(st), est) and np.array_equal(as_np(z), ez)
    t = times(len(blobs))
    for got, e in zip(A.xz3_index_keys(col, pa.array(t), "wkb", g=g, status=True), W.xz3_keys(geoms, t, g=g)):
        assert np.array_equal(as_np(got), e)
    x, y = A.points_to_columns(col)
    assert np.array_equal(bits((x, y)), expect_points(geoms).view(np.uint64))
    return col


def test_mixed_column_envelopes_keys_and_points(gpu, oracle):
    blobs, geoms = mixed()
    assert len(blobs) >= C.LANE_SLOTS
    check_column(blobs, geoms)
    # a slice: value offsets and validity bits that do not start at zero
    assert any(b is None for b in blobs[37:300])
    from geomesa_amd import arrow as A
    got = bits(A.envelopes(wkb_array(blobs).slice(37, 263), "wkb"))
    assert np.array_equal(got, np.stack(W.envelopes(geoms[37:300]), 1).view(np.uint64))
    x, y = A.points_to_columns(wkb_array(blobs).slice(37, 263), kind="wkb")
    assert np.array_equal(bits((x, y)), expect_points(geoms[37:300]).view(np.uint64))


@functools.lru_cache(maxsize=None)
def mixed_table(dim):
    from geomesa_amd.table import XZ2Table, XZ3Table
    blobs, _ = mixed()
    sh = (np.arange(len(blobs)) * 2654435761 % 4).astype(np.uint8)
    if dim == 2:
        return XZ2Table.from_geometries(wkb_array(blobs), "wkb", shard=sh, shards=4)
    return XZ3Table.from_geometries(wkb_array(blobs), times(len(blobs)), "wkb")


@pytest.mark.parametrize("q", list(C.QUERIES))
@pytest.mark.parametrize("dim", [2, 3])
def test_mixed_column_queries(gpu, dim, q):
    _, geoms = mixed()
    boxes = C.QUERIES[q]
    env_hit, exp = C.check_shortcut_coverage(geoms, boxes)
    tb = mixed_table(dim)
    if dim == 3:
        iv = (T0 - 1, T0 + G.WEEK_MS)
        t = times(len(geoms))
        keep = (t > iv[0]) & (t < iv[1])
        assert keep.all()
        ids, nm, scanned = tb.query(boxes, iv)
    else:
        ids, nm, scanned = tb.query(boxes)
    assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
    assert tb.n_envelope == env_hit.sum() and nm <= tb.n_envelope <= scanned
    ids, nm, _ = tb.query(boxes, exact=False) if dim == 2 else tb.query(boxes, iv, exact=False)
    assert np.array_equal(np.sort(as_np(ids)), np.nonzero(env_hit)[0])


def test_special_ordinates_by_bit_pattern(gpu, oracle):
    blobs = C.special_column()
    geoms = [W.parse(b) for b in blobs]
    assert all(g is not None for g in geoms)
    from geomesa_amd import arrow as A
    col = A.GeometryColumn(wkb_array(blobs), "wkb")
    exp = np.stack(W.envelopes(geoms), 1).view(np.uint64)
    assert np.array_equal(bits(A.envelopes(col, "wkb")), exp)
    assert 0x7ff8000000abc123 in exp and 0xfff4000000000007 in exp and 0x8000000000000000 in exp   # they got through
    x, y = A.points_to_columns(col)
    assert np.array_equal(bits((x, y)), expect_points(geoms).view(np.uint64))


# ---------------------------------------------------------------- malformed slots
def test_malformed_slots_are_null_slots(gpu, oracle):
    """Null envelope, GM_ST_NULL_GEOM, NaN from the adapter, never a match -- and every neighbour, whose bytes
    a reader running past a malformed slot's end would take, is what the reference makes of it alone."""
    from geomesa_amd.table import XZ2Table
    blobs, bad = C.malformed_column()
    geoms = [W.parse(b) for b in blobs]
    assert all(geoms[i] is None for i in bad) and sum(g is not None for g in geoms) >= 8
    col = check_column(blobs, geoms)
    tb = XZ2Table.from_geometries(col, "wkb")
    for boxes in (WORLD, [(0.0, 0.0, 8.0, 8.0)], [(99.0, -60.0, 101.0, -49.0), (49.0, -61.0, 51.0, -59.0)]):
        exp = W.scan(geoms, boxes)
        ids, nm, _ = tb.query(boxes)
        assert nm == exp.sum() and np.array_equal(np.sort(as_np(ids)), np.nonzero(exp)[0])
        assert not set(as_np(ids).tolist()) & set(bad)
    assert W.scan(geoms, WORLD).sum() == sum(g is not None and W.envelope(g) != W.NULL_ENV for g in geoms)


# ---------------------------------------------------------------- the ABI's rejections
def copy_of(s, **kw):
    c = type(s)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(s), ctypes.sizeof(s))
    for k, val in kw.items():
        setattr(c, k, val)
    return c


def test_invalid_wkb_columns(gpu):
    """ordinal_bits 32, offsets[0] NULL and coords NULL are GM_E_INVALID for the new type in the five entries
    that take it; types 6 and -1 stay unknown."""
    import torch
    from geomesa_amd import _lib
    from geomesa_amd.table import _full_filter, key_ranges
    tb = mixed_table(2)
    g = tb.geom.c_struct()
    n = tb.geom.n
    out = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    z = torch.zeros(n, dtype=torch.int64, device="cuda")
    b = torch.zeros(n, dtype=torch.int16, device="cuda")
    o = [out[k].data_ptr() for k in range(4)]
    kr, _ = key_ranges([("bounded", (0, 0), (0, -1))], tb.shards)
    f, keep = _full_filter(tb.env, C.BOXES, perm=tb.perm)
    lib, h = gpu.lib, gpu.handle

    def calls(c):
        p = ctypes.byref(c)
        return [lib.gm_arrow_envelopes(h, p, n, *o), lib.gm_xz2_index_key_arrow(h, p, n, 12, 0, z.data_ptr(), None, None),
                lib.gm_xz3_index_key_arrow(h, p, None, n, 12, 1, 0, b.data_ptr(), z.data_ptr(), None, None),
                lib.gm_arrow_points_to_columns(h, p, n, o[0], o[1]), G.scan_geom(gpu, tb, kr, f, c, tb.perm)[0]]
    assert calls(g) == [0] * 5
    bad = [copy_of(g, ordinal_bits=32), copy_of(g, offsets=(ctypes.c_void_p * 3)(None, None, None)),
           copy_of(g, coords=None), copy_of(g, type=6), copy_of(g, type=-1), copy_of(g, type=15), copy_of(g, type=17)]
    for c in bad:
        assert calls(c) == [_lib.GM_E_INVALID] * 5, (c.type, c.ordinal_bits)
    for c, text in ((bad[0], "ordinal_bits must be 64 for a GM_GEOM_WKB column"), (bad[1], "offsets"), (bad[2], "coords"),
                    (bad[3], "unknown geometry type"), (bad[4], "unknown geometry type")):
        assert G.scan_geom(gpu, tb, kr, f, c, tb.perm)[0] == _lib.GM_E_INVALID
        assert _lib.last_error().startswith("gm_table_scan_geom: ") and text in _lib.last_error()


def test_entries_that_do_not_take_wkb(gpu):
    """The seven typed-only entries return GM_E_INVALID for type 16 with a text that names the type and, for
    the point entries, the adapter.  Each is reached through its wrapper with a typed column that is valid
    for it in every other respect, its type code alone set to GM_GEOM_WKB."""
    from geomesa_amd import _lib
    from geomesa_amd import arrow as A
    from geomesa_amd.bin import BinEncoder
    from geomesa_amd.curve import IllegalArgumentException
    from geomesa_amd.density import RenderingGrid
    rows = {"point": [(3.0, 1.0), (9.0, 9.0)], "linestring": [[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0), (3.0, 1.0)]],
            "polygon": [[[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 0.0)]]]}
    cols = {k: A.GeometryColumn(G.to_arrow(r, k), k) for k, r in rows.items()}
    index = A.ArrowPolygonIndex(cols["polygon"])
    assert index.join(cols["point"], count_only=True) == 1          # valid before the type changes
    for k in ("point", "linestring"):
        cols[k]._c.type = _lib.GM_GEOM_WKB
    grid = RenderingGrid((-10.0, -10.0, 10.0, 10.0), 16, 16)
    point_entries = {
        "gm_z3_index_key_arrow": lambda: A.z3_index_keys(cols["point"]),
        "gm_z2_index_key_arrow": lambda: A.z2_index_keys(cols["point"]),
        "gm_pip_join_arrow": lambda: index.join(cols["point"], count_only=True),
        "gm_density_arrow": lambda: grid.render_arrow(cols["point"]),
        "gm_bin_arrow": lambda: BinEncoder().encode_arrow(cols["point"], track=np.zeros(2, np.int32)),
    }
    other_entries = {"gm_density_lines": lambda: grid.render_lines(cols["linestring"])}
    for name, call in list(point_entries.items()) + list(other_entries.items()):
        with pytest.raises(_lib.GeomesaHipError) as e:
            call()
        text = str(e.value)
        assert name in text and "rc=%d" % _lib.GM_E_INVALID in text and "GM_GEOM_WKB" in text, text
        assert ("gm_arrow_points_to_columns" in text) == (name in point_entries), text
    hs = cols["polygon"].host_struct()
    hs.type = _lib.GM_GEOM_WKB
    out = ctypes.c_void_p()
    assert gpu.lib.gm_pip_index_create_arrow(gpu.handle, ctypes.byref(hs), 1, 0, ctypes.byref(out)) == _lib.GM_E_INVALID
    assert _lib.last_error().startswith("gm_pip_index_create_arrow: ") and "GM_GEOM_WKB" in _lib.last_error()
    assert "gm_arrow_points_to_columns" not in _lib.last_error() and not out.value
    # the wrappers of the point keys name the adapter before the ABI is reached
    wkb = A.GeometryColumn(wkb_array([W.write(("point", (1.0, 2.0)))]), "wkb")
    for fn in (A.z3_index_keys, A.z2_index_keys):
        with pytest.raises(IllegalArgumentException, match="points_to_columns"):
            fn(wkb)
    with pytest.raises(IllegalArgumentException):
        A.GeometryColumn(pa.array([b"x"], pa.large_binary()), "wkb")


# ---------------------------------------------------------------- a stream of its own
def test_wkb_entries_on_an_owned_stream(gpu):
    """gm_arrow_envelopes and gm_xz2_index_key_arrow over a WKB column on a Context.owned stream, compared after
    gm_ctx_sync with what the default context gives."""
    import torch
    from geomesa_amd import _lib
    from geomesa_amd import arrow as A
    blobs, _ = mixed()
    col = A.GeometryColumn(wkb_array(blobs), "wkb")
    n = col.n
    exp_env = bits(A.envelopes(col, "wkb"))
    ez, es = A.xz2_index_keys(col, "wkb", status=True)
    env = torch.full((4, n), 7.0, dtype=torch.float64, device="cuda")
    z = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx = _lib.Context.owned(0)
    try:
        p = ctypes.byref(col.c_struct())
        assert ctx.stream != 0
        assert ctx.lib.gm_arrow_envelopes(ctx.handle, p, n, *[env[k].data_ptr() for k in range(4)]) == 0
        assert ctx.lib.gm_xz2_index_key_arrow(ctx.handle, p, n, 12, 0, z.data_ptr(), st.data_ptr(), None) == 0
        ctx.sync()
        assert np.array_equal(bits([env[k] for k in range(4)]), exp_env)
        assert np.array_equal(as_np(z), as_np(ez)) and np.array_equal(as_np(st), as_np(es))
    finally:
        ctx.close()
