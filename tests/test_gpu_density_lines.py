"""GPU parity of the density scan over line features (gm_density_lines, RenderingGrid.render_lines) with
tests/density_lines_ref.render_lines_numpy, which test_density_lines_reference.py holds equal to the Scala
read line by line and whose input classes it counts.

Grids and the three tallies are compared bit for bit (unweighted and dyadic weights) on every accumulation
path the grid allows (0 automatic, 1 LDS counters, 2 device atomics), with the default launch and with one
workgroup.  The kernel deals vertices out 64 at a time per wave (gm_density.hip: line_items), and a lane
drains the LDS counters after 2^19 additions of its own (DENS_THREAD_DRAIN)."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

import density_lines_ref as L
from abi_buffers import Guarded, untouched
from test_gpu_density import as_np, fits, grid_c, paths, same

pytestmark = pytest.mark.gpu

THREAD_DRAIN = 1 << 19


def tuples_type(f32):
    return pa.list_(pa.float32() if f32 else pa.float64(), 2)


def to_arrow(rows, kind, f32=False, flip=False):
    """Rows (None: a null slot) -> the geomesa-arrow-jts vector ([y, x] tuples unless flip)."""
    def line(pts):
        return [[x, y] if flip else [y, x] for (x, y) in pts]
    if kind == "linestring":
        return pa.array([None if r is None else line(r) for r in rows], pa.list_(tuples_type(f32)))
    return pa.array([None if r is None else [line(p) for p in r] for r in rows], pa.list_(pa.list_(tuples_type(f32))))


def arrow_line_of(x, y, f32=False):
    """One LineString slot per row of the 2-D arrays x / y (rows x vertices), from numpy: [y, x] tuples."""
    flat = np.stack([y, x], -1).reshape(-1).astype(np.float32 if f32 else np.float64)
    tup = pa.FixedSizeListArray.from_arrays(pa.array(flat), 2)
    off = (np.arange(x.shape[0] + 1) * x.shape[1]).astype(np.int32)
    return pa.ListArray.from_arrays(pa.array(off), tup)


def column(arr, kind, flip=False):
    from geomesa_amd.arrow import GeometryColumn
    return GeometryColumn(arr, kind, flip)


def gpu_lines(env, w, h, col, weight=None, mask=None, ids=None, path=0, workgroups=0, into=None):
    from geomesa_amd.density import RenderingGrid
    g = into if into is not None else RenderingGrid(env, w, h, path=path, workgroups=workgroups)
    g.render_lines(col, weight, mask=mask, ids=ids)
    return as_np(g.grid), np.array(g.tally, np.int64), g


@functools.lru_cache(maxsize=None)
def case(k):
    """The line set of envelope k: rows, its device column, the reference grid and tally."""
    name, env, w, h = L.LINE_ENVELOPES[k]
    rows = L.line_set(env, w, h, 5 + k)
    grid, tally = L.render_lines_numpy(env, w, h, rows)
    assert grid.sum() >= 1000
    return env, w, h, rows, column(to_arrow(rows, "linestring"), "linestring"), grid, tally


@functools.lru_cache(maxsize=None)
def weighted_case(k):
    env, w, h, rows, col, _, _ = case(k)
    wt = np.random.default_rng(9 + k).integers(-1024, 1025, len(rows)) / 8.0
    return (wt,) + L.render_lines_numpy(env, w, h, rows, wt)


CASES = [(k, p, wg) for k, e in enumerate(L.LINE_ENVELOPES) for p in paths(e[2], e[3]) for wg in (0, 1)]


@pytest.mark.parametrize("k,path,workgroups", CASES,
                         ids=["%s-path%d-wg%d" % (L.LINE_ENVELOPES[k][0], p, wg) for (k, p, wg) in CASES])
def test_grids_and_paths(gpu, k, path, workgroups):
    """Every input class (test_density_lines_reference.py counts them) on 8 x 8, 64 x 64 (one LDS pass),
    256 x 256 (2 passes), 500 x 500 (7 passes) and the wide and fractional-xmin envelopes, on every path."""
    env, w, h, rows, col, want, tally = case(k)
    got, t, _ = gpu_lines(env, w, h, col, path=path, workgroups=workgroups)
    assert same(got, want) and np.array_equal(t, tally)


WCASES = [(k, p) for k, e in enumerate(L.LINE_ENVELOPES) for p in ([0, 1, 2] if fits(e[2], e[3], True) else [0, 2])]


@pytest.mark.parametrize("k,path", WCASES, ids=["%s-path%d" % (L.LINE_ENVELOPES[k][0], p) for (k, p) in WCASES])
def test_dyadic_weights_are_bit_equal_on_every_path(gpu, k, path):
    """Weights k / 8, |k| <= 1024: every partial sum is exact, so no order of the additions shows
    (256 x 256 takes 4 weighted LDS passes)."""
    env, w, h, rows, col, _, _ = case(k)
    wt, want, tally = weighted_case(k)
    for workgroups in (0, 1):
        got, t, _ = gpu_lines(env, w, h, col, wt, path=path, workgroups=workgroups)
        assert same(got + 0.0, want + 0.0) and np.array_equal(t, tally)


@pytest.mark.parametrize("kind", ["linestring", "multilinestring"])
@pytest.mark.parametrize("f32", [False, True], ids=["float8", "float4"])
@pytest.mark.parametrize("flip", [False, True], ids=["yx", "xy"])
def test_arrow_columns(gpu, kind, f32, flip):
    """LineString and MultiLineString, Float8 and Float4, both axis orders; unselected, masked and by ids,
    weighted and not.  A Float4 vector renders the widened floats."""
    k = 1
    name, env, w, h = L.LINE_ENVELOPES[k]
    rows = case(k)[3]
    if kind == "multilinestring":
        rows = L.as_multi(rows, 3)
        assert any(r == [[]] for r in rows) and any(r is not None and len(r) == 3 for r in rows)
    if f32:
        rows = L.in_float32(rows)
    col = column(to_arrow(rows, kind, f32, flip), kind, flip)
    n = len(rows)
    rng = np.random.default_rng(21)
    wt = rng.integers(-1024, 1025, n) / 8.0
    mask = rng.random(n) < 0.5
    ids = np.concatenate([rng.permutation(n)[:n // 2], [3, 3, -1, n]]).astype(np.int64)
    for weight in (None, wt):
        for sel in ({}, {"mask": mask}, {"ids": ids}):
            want, tally = L.render_lines_numpy(env, w, h, rows, weight, **sel)
            for path in (0, 2):
                got, t, _ = gpu_lines(env, w, h, col, weight, path=path, **sel)
                assert same(got + 0.0, want + 0.0) and np.array_equal(t, tally), (weight is None, list(sel), path)
    assert tally[0] > 20 and tally[2] == 2


def test_pyarrow_array_and_bad_kind(gpu):
    from geomesa_amd.density import RenderingGrid
    env, w, h, rows, col, want, tally = case(0)
    g = RenderingGrid(env, w, h).render_lines(to_arrow(rows, "linestring"))
    assert same(as_np(g.grid), want) and g.tally == tally.tolist()
    pts = pa.array([[1.0, 1.0]], tuples_type(False))
    with pytest.raises(ValueError):
        RenderingGrid(env, w, h).render_lines(pts, kind="point")
    with pytest.raises(ValueError):                       # render_arrow keeps refusing lines
        RenderingGrid(env, w, h).render_arrow(col)


# ------------------------------------------------------------------ structure

def test_one_linestring_of_100k_vertices(gpu):
    """A part far longer than the 64 vertices a wave takes per step, between short ones: a random walk of
    steps up to 3 pixels that leaves the 500 x 500 envelope now and then."""
    env, w, h = (-1.0, 33.0, 6.0, 40.0), 500, 500
    rng = np.random.default_rng(5)
    n = 100_000
    d = 7.0 / 500
    x = 2.5 + np.cumsum(rng.uniform(-3, 3, n) * d)
    y = 36.5 + np.cumsum(rng.uniform(-3, 3, n) * d)
    x, y = -2.0 + (x + 2.0) % 9.0, 32.0 + (y - 32.0) % 9.0      # folded over the envelope and a margin of 1
    long = list(zip(x.tolist(), y.tolist()))
    short = case(3)[3][:40]
    rows = short[:20] + [long] + short[20:]
    want, tally = L.render_lines_numpy(env, w, h, rows)
    assert want.sum() > 100_000
    col = column(to_arrow(rows, "linestring"), "linestring")
    for path, workgroups in ((0, 0), (1, 1), (2, 0)):
        got, t, _ = gpu_lines(env, w, h, col, path=path, workgroups=workgroups)
        assert same(got, want) and np.array_equal(t, tally), (path, workgroups)
    multi = [rows[:21], None, rows[21:]]
    col = column(to_arrow(multi, "multilinestring"), "multilinestring")
    got, t, _ = gpu_lines(env, w, h, col)
    assert same(got, want) and t.tolist() == [tally[0] + 1, tally[1], 0]


def zigzag(segments, row_y):
    """One LineString zigzagging between the centres of columns 0 and 63 of a 64-column grid over (0, 64)."""
    x = np.where(np.arange(segments + 1) % 2 == 0, 0.5, 63.5)
    return x[None, :], np.full((1, segments + 1), row_y)


def test_one_linestring_past_the_thread_drain(gpu):
    """One linestring whose lanes each add more than DENS_THREAD_DRAIN times (the LDS counters are drained
    in between) and that hits one pixel more often than that: 600,000 segments of 63 pixels over one row.
    Segment k writes columns 0..62 (even k) or 63..1 (odd k); the closed form is held against the
    reference at 1,001 segments."""
    env, w, h = (0.0, 0.0, 64.0, 64.0), 64, 64

    def closed_form(s):
        want = np.zeros((h, w))
        want[10, :] = s
        want[10, 0], want[10, 63] = (s + 1) // 2, s // 2
        return want
    x, y = zigzag(1001, 10.5)
    rows = [list(zip(x[0].tolist(), y[0].tolist()))]
    assert same(L.render_lines_numpy(env, w, h, rows)[0], closed_form(1001))
    s = 600_000
    assert s * 63 // 64 > THREAD_DRAIN and s > THREAD_DRAIN
    x, y = zigzag(s, 10.5)
    col = column(arrow_line_of(x, y), "linestring")
    for path, workgroups in ((1, 1), (1, 0), (2, 0)):
        got, t, _ = gpu_lines(env, w, h, col, path=path, workgroups=workgroups)
        assert same(got, closed_form(s)) and t.tolist() == [0, 0, 0], (path, workgroups)


def test_two_calls_equal_one_call_over_the_concatenation(gpu):
    env, w, h, rows, col, want, tally = case(2)
    cut = 701
    a, b = column(to_arrow(rows[:cut], "linestring"), "linestring"), column(to_arrow(rows[cut:], "linestring"), "linestring")
    _, _, g = gpu_lines(env, w, h, a)
    got, t, _ = gpu_lines(env, w, h, b, into=g)
    assert same(got, want) and np.array_equal(t, tally)
    i, j, v = g.sparse()
    jj, ii = np.nonzero(want)
    assert len(as_np(v)) == len(ii) and as_np(v).sum() == want.sum()
    assert len(g.decode()[2]) == len(ii)
    g.clear()
    assert g.is_empty() and g.tally == [0, 0, 0]


# ------------------------------------------------------------------ selections

def test_mask_from_strict_scan(gpu, oracle):
    """The mask words gm_strict_scan writes over the lines' first vertices select the slots."""
    import torch
    from geomesa_amd import _lib
    from geomesa_amd.curve import _dev_col
    env, w, h, rows, col, _, _ = case(3)
    n = len(rows)
    first = [r[0] if r else (np.nan, np.nan) for r in rows]
    x, y = np.array([p[0] for p in first]), np.array([p[1] for p in first])
    bbox = (0.5, 34.0, 4.25, 39.0)
    dx, dy = _dev_col(x, torch.float64), _dev_col(y, torch.float64)
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    bb = (ctypes.c_double * 4)(*bbox)
    _lib.check(gpu.lib.gm_strict_scan(gpu.handle, _lib.ptr(dx), _lib.ptr(dy), None, n, bb, 0, 0, 0, _lib.ptr(words),
                                      None, 0, None), "gm_strict_scan")
    keep = oracle.strict_scan(x, y, None, bbox)
    assert 100 < keep.sum() < n - 100 and n % 64 != 0
    want, tally = L.render_lines_numpy(env, w, h, rows, mask=keep)
    for path in (0, 1, 2):
        got, t, _ = gpu_lines(env, w, h, col, mask=words, path=path)
        assert same(got, want) and np.array_equal(t, tally)
    words[-1] |= torch.tensor(-1 << (n % 64), dtype=torch.int64, device="cuda")    # bits at and above n
    got, t, _ = gpu_lines(env, w, h, col, mask=words)
    assert same(got, want) and np.array_equal(t, tally)
    few = np.zeros(n, bool)
    few[::97] = True                                                                # automatic path: atomics
    want, tally = L.render_lines_numpy(env, w, h, rows, mask=few)
    got, t, _ = gpu_lines(env, w, h, col, mask=few)
    assert same(got, want) and np.array_equal(t, tally)


@pytest.mark.parametrize("order", ["ascending", "permuted", "duplicated", "out-of-range"])
@pytest.mark.parametrize("path", [0, 2])
def test_ids(gpu, order, path):
    env, w, h, rows, col, _, _ = case(3)
    n = len(rows)
    rng = np.random.default_rng(4)
    ids = np.flatnonzero(rng.random(n) < 0.4).astype(np.int64)
    if order != "ascending":
        ids = rng.permutation(ids)
    if order == "duplicated":
        ids = np.concatenate([ids, ids[:100], ids[:10], ids[:10]])
    if order == "out-of-range":
        ids = np.concatenate([ids[:50], [-1, n, 1 << 40, -(1 << 62), n + 1], ids[50:], [-1]])
    want, tally = L.render_lines_numpy(env, w, h, rows, ids=ids)
    got, t, _ = gpu_lines(env, w, h, col, ids=ids, path=path)
    assert same(got, want) and np.array_equal(t, tally)
    assert tally[2] == (6 if order == "out-of-range" else 0)
    wt = rng.integers(-1024, 1025, n) / 8.0
    want, tally = L.render_lines_numpy(env, w, h, rows, wt, ids=ids)
    got, t, _ = gpu_lines(env, w, h, col, wt, ids=ids, path=path)
    assert same(got + 0.0, want + 0.0) and np.array_equal(t, tally)


def test_empty_selections_and_no_rows(gpu):
    env, w, h, rows, col, _, _ = case(1)
    zero = np.zeros((h, w))
    for kw in ({"ids": np.zeros(0, np.int64)}, {"mask": np.zeros(len(rows), bool)}):
        got, t, _ = gpu_lines(env, w, h, col, **kw)
        assert same(got, zero) and t.tolist() == [0, 0, 0]
    for kind in ("linestring", "multilinestring"):
        none = column(to_arrow([], kind), kind)
        got, t, _ = gpu_lines(env, w, h, none)
        assert same(got, zero) and t.tolist() == [0, 0, 0]
        got, t, _ = gpu_lines(env, w, h, none, ids=np.array([0, 5, -3]))   # no slots: every id is outside
        assert same(got, zero) and t.tolist() == [0, 0, 3]
    one = column(to_arrow([[(171.0, 1.0), (175.0, 4.0)]], "linestring"), "linestring")
    got, t, _ = gpu_lines(env, w, h, one)
    assert same(got, L.render_lines_numpy(env, w, h, [[(171.0, 1.0), (175.0, 4.0)]])[0]) and got.sum() > 5


def test_ids_of_an_xz2_table_query(gpu):
    """XZ2Table.query over the same column -> render_lines(ids=...): the reference rendering of exactly the
    linestrings the table's exact full filter keeps (geom_intersects_ref)."""
    import geom_intersects_ref as G
    from geomesa_amd.table import XZ2Table
    env, w, h = (-180.0, -90.0, 180.0, 90.0), 256, 256
    rng = np.random.default_rng(8)
    rows = []
    for _ in range(3000):
        c = (rng.uniform(-170, 170), rng.uniform(-80, 80))
        m = int(rng.integers(2, 12))
        rows.append(list(zip((c[0] + np.cumsum(rng.uniform(-2, 2, m))).tolist(),
                             (c[1] + np.cumsum(rng.uniform(-2, 2, m))).tolist())))
    arr = to_arrow(rows, "linestring")
    col = column(arr, "linestring")
    boxes = [(-40.0, 10.0, 40.0, 70.0), (100.0, -50.0, 130.5, -20.0)]
    ids, nm, _ = XZ2Table.from_geometries(col, "linestring").query(boxes)
    keep = G.scan(rows, "linestring", boxes)
    assert nm == keep.sum() > 100
    want, tally = L.render_lines_numpy(env, w, h, rows, mask=keep)
    for path in (0, 2):
        got, t, _ = gpu_lines(env, w, h, col, ids=ids, path=path)
        assert same(got, want) and np.array_equal(t, tally)


# ------------------------------------------------------------------ weights

@pytest.mark.parametrize("k,path", [(0, 1), (0, 2), (1, 1), (3, 2)])
def test_random_weights_within_the_any_order_bound(gpu, k, path):
    """The bound of test_gpu_density.py: a pixel of m addends lies within (m - 1) 2^-53 sum|w| of their sum
    in any order of the additions (each of the m - 1 roundings is at most half an ulp of a partial sum, and
    no partial sum exceeds sum|w|).  The bound is about the real sum, so the sum is taken in rationals here:
    math.fsum rounds it by up to half an ulp more, which the bound does not hold -- lines add one weight to
    one pixel several times, and the addends (-812.76, -294.32, -65.99, -65.99) summed in that order land
    3.4e-13 from their sum (bound 4.1e-13) but 4.5e-13 from fsum."""
    env, w, h, rows, col, _, _ = case(k)
    wt = np.random.default_rng(13).uniform(-1000.0, 1000.0, len(rows))
    pix, wts, tally = L.line_additions(env, w, h, rows, wt)
    order = np.argsort(pix, kind="stable")
    pix, wts = pix[order], wts[order]
    starts = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
    ends = np.r_[starts[1:], len(pix)]
    got, t, _ = gpu_lines(env, w, h, col, wt, path=path)
    got = got.reshape(-1)
    seen = np.zeros(w * h, bool)
    worst = 0.0
    for a, b in zip(starts, ends):
        m = b - a
        exact = sum(Fraction(v) for v in wts[a:b].tolist())
        bound = (m - 1) * Fraction(1, 2 ** 53) * sum(abs(Fraction(v)) for v in wts[a:b].tolist())
        err = abs(Fraction(float(got[pix[a]])) - exact)
        worst = max(worst, float(err / bound) if bound else (0.0 if err == 0 else math.inf))
        assert err <= bound, (int(pix[a]), m, float(err), float(bound))
        seen[pix[a]] = True
    assert not got[~seen].any() and np.array_equal(t, tally)
    print("largest error / bound over %d pixels: %.3g" % (len(starts), worst))


def test_zero_weight_adds_nothing(gpu):
    env, w, h = (0.0, 0.0, 8.0, 8.0), 8, 8
    rows = [[(0.5, 0.5), (4.5, 0.5)], [(0.5, 1.5), (4.5, 1.5)], [(0.5, 1.5), (2.5, 1.5)], [(0.5, 2.5), (3.5, 2.5)]]
    wt = np.array([0.0, 2.0, -2.0, 4.0])
    col = column(to_arrow(rows, "linestring"), "linestring")
    for path in (1, 2):
        got, _, g = gpu_lines(env, w, h, col, wt, path=path)
        assert got[0].tolist() == [0.0] * 8 and got[1, :5].tolist() == [0.0, 0.0, 2.0, 2.0, 0.0]
        assert got[2, :4].tolist() == [4.0, 4.0, 4.0, 0.0]
        i, j, v = g.sparse()
        assert as_np(j).tolist() == [2, 2, 1, 2, 1] and as_np(v).tolist() == [4.0, 4.0, 2.0, 4.0, 2.0]


# ------------------------------------------------------------------ the C ABI

def c_column(kind_code, coords, offs):
    from geomesa_amd.arrow import GeomColumnC
    o = [b.addr for b in offs] + [None] * (3 - len(offs))
    return GeomColumnC(kind_code, 64, 0, 0, coords.addr, None, 0, (ctypes.c_void_p * 3)(*o))


def abi_lines(n=100):
    rng = np.random.default_rng(0)
    yx = np.stack([rng.uniform(33, 40, 4 * n), rng.uniform(-1, 6, 4 * n)], 1)
    rows = [[(float(yx[4 * r + v, 1]), float(yx[4 * r + v, 0])) for v in range(4)] for r in range(n)]
    return Guarded.of(yx), Guarded.of((4 * np.arange(n + 1)).astype(np.int32)), rows


INVALID = {
    "null-ctx": dict(ctx=None),
    "null-grid-description": dict(g=None),
    "null-grid": dict(grid=None),
    "null-tally": dict(tally=None),
    "negative-n": dict(n=-1),
    "width-0": dict(g=dict(w=0)),
    "height-negative": dict(g=dict(h=-1)),
    "too-many-pixels": dict(g=dict(w=65536, h=32768)),
    "xmax-equals-xmin": dict(g=dict(env=(1.0, 33.0, 1.0, 40.0))),
    "ymax-below-ymin": dict(g=dict(env=(-1.0, 40.0, 6.0, 33.0))),
    "nan-bound": dict(g=dict(env=(float("nan"), 33.0, 6.0, 40.0))),
    "infinite-bound": dict(g=dict(env=(-1.0, 33.0, float("inf"), 40.0))),
    "bound-beyond-2^31": dict(g=dict(env=(-1.0, 33.0, 6.0, 3e9))),
    "wider-than-64-turns": dict(g=dict(env=(-12000.0, 33.0, 11040.5, 40.0))),
    "mask-and-ids": dict(both=True),
    "negative-id-count": dict(n_ids=-1),
    "path-3": dict(g=dict(path=3)),
    "path-negative": dict(g=dict(path=-1)),
    "path-1-does-not-fit": dict(g=dict(w=1024, h=1024, path=1)),
    "workgroups-negative": dict(g=dict(workgroups=-1)),
    "null-geom": dict(geom=None),
    "point-column": dict(kind=0),
    "polygon-column": dict(kind=2),
    "multipoint-column": dict(kind=3),
    "multipolygon-column": dict(kind=5),
    "ordinal-bits-16": dict(bits=16),
    "null-coords": dict(coords=None),
    "null-offsets": dict(offsets=None),
    "misaligned-weight": dict(weight_offset=4),
    "misaligned-grid": dict(grid_offset=4),
}


@pytest.mark.parametrize("case_name", sorted(INVALID))
def test_invalid_arguments(gpu, case_name):
    """Every GM_E_INVALID of the contract, on guarded buffers: the code, a gm_last_error text, and no write
    to grid, tally or anything else."""
    from geomesa_amd import _lib
    spec = INVALID[case_name]
    n = 100
    YX, OFF, _ = abi_lines(n)
    M, I = Guarded.of(np.full(2, -1, np.int64)), Guarded.of(np.arange(n, dtype=np.int64))
    W = Guarded.of(np.ones(n + 1), offset=spec.get("weight_offset", 0))
    G, T = Guarded(16 * 16 * 8 + 8, offset=spec.get("grid_offset", 0)), Guarded(24)
    gkw = spec.get("g", {})
    g = None if gkw is None else grid_c(**gkw)
    col = c_column(spec.get("kind", 1), YX, [OFF, OFF, OFF][:{0: 0, 1: 1, 2: 2, 3: 1, 5: 3}[spec.get("kind", 1)]])
    if "bits" in spec:
        col.ordinal_bits = spec["bits"]
    if "coords" in spec:
        col.coords = None
    if "offsets" in spec:
        col.offsets[0] = None
    geom = ctypes.byref(col) if spec.get("geom", 1) is not None else None
    both = bool(spec.get("both"))
    ids = I.ptr if both or "n_ids" in spec else None
    rc = gpu.lib.gm_density_lines(spec.get("ctx", gpu.handle), geom, W.ptr if "weight_offset" in spec else None,
                                  spec.get("n", n), M.ptr if both else None, ids,
                                  spec.get("n_ids", n if both else 0), ctypes.byref(g) if g is not None else None,
                                  spec.get("grid", G.ptr), spec.get("tally", T.ptr))
    assert rc == _lib.GM_E_INVALID
    assert "gm_density_lines" in _lib.last_error()
    gpu.sync()
    assert untouched(G.read()) and untouched(T.read())
    for b in (YX, OFF, M, I, W, G, T):
        b.check(case_name)


@pytest.mark.parametrize("multi", [False, True])
def test_a_valid_call_writes_grid_and_tally_only(gpu, multi):
    from geomesa_amd import _lib
    n = 100
    YX, OFF, rows = abi_lines(n)
    G, T = Guarded(16 * 16 * 8), Guarded(24)
    G.write(np.zeros(16 * 16)); T.write(np.zeros(3, np.int64))
    W = Guarded.of(np.arange(n) / 4.0)
    I = Guarded.of(np.array([5, 7, 7, -1, 99, 100], np.int64))
    g = grid_c()
    if multi:                                     # two lines per slot
        SLOT = Guarded.of((2 * np.arange(n // 2 + 1)).astype(np.int32))
        col, rows, n = c_column(4, YX, [SLOT, OFF]), [rows[2 * r:2 * r + 2] for r in range(n // 2)], n // 2
    else:
        SLOT, col = OFF, c_column(1, YX, [OFF])
    ids = np.array([5, 7, 7, -1, 49, 100], np.int64)
    I = Guarded.of(ids)
    rc = gpu.lib.gm_density_lines(gpu.handle, ctypes.byref(col), W.ptr, n, None, I.ptr, len(ids), ctypes.byref(g),
                                  G.ptr, T.ptr)
    assert rc == _lib.GM_OK
    gpu.sync()
    want, tally = L.render_lines_numpy((-1.0, 33.0, 6.0, 40.0), 16, 16, rows, np.arange(100) / 4.0, ids=ids)
    assert same(G.read(np.float64).reshape(16, 16), want) and T.read(np.int64).tolist() == tally.tolist()
    assert tally[2] == 2 and want.sum() > 0
    for b in (YX, OFF, SLOT, W, I, G, T):
        b.check("valid call")


TWO_CALL_ENV, TWO_CALL_PX = (-1.0, 33.0, 6.0, 40.0), 64
TWO_CALL_LINES = 2 * 1024 + 6      # one lane per segment: 3 x 2054 = 6 blocks of 1024 lanes + 18; even: slots pair up


def two_call_batch(seed, multi):
    """2054 lines of 4 vertices over the envelope and a margin of a tenth of it, two lines per slot if multi:
    (column, its buffers, slots, rows as the reference takes them)."""
    env, n = TWO_CALL_ENV, TWO_CALL_LINES
    rng = np.random.default_rng(1300 + seed)
    mx, my = 0.1 * (env[2] - env[0]), 0.1 * (env[3] - env[1])
    x = rng.uniform(env[0] - mx, env[2] + mx, 4 * n)
    y = rng.uniform(env[1] - my, env[3] + my, 4 * n)
    x[-8 + seed::4] = np.nan           # the last two lines cannot be rendered: the tallies add up too
    YX, OFF = Guarded.of(np.stack([y, x], 1).reshape(-1)), Guarded.of((4 * np.arange(n + 1)).astype(np.int32))
    rows = [[(float(x[4 * r + v]), float(y[4 * r + v])) for v in range(4)] for r in range(n)]
    if not multi:
        return c_column(1, YX, [OFF]), [YX, OFF], n, rows
    SLOT = Guarded.of((2 * np.arange(n // 2 + 1)).astype(np.int32))
    return c_column(4, YX, [SLOT, OFF]), [YX, OFF, SLOT], n // 2, [rows[2 * r:2 * r + 2] for r in range(n // 2)]


@pytest.mark.parametrize("multi", [False, True], ids=["linestring", "multilinestring"])
def test_two_abi_calls_into_one_grid_add_up(gpu, multi):
    """gm_density_lines twice into one grid and tally, two different batches, nothing waited for in between:
    each batch alone equals its reference, and the shared grid equals the sum of both references."""
    from geomesa_amd import _lib
    px = TWO_CALL_PX
    g = grid_c(TWO_CALL_ENV, px, px)
    batches = [two_call_batch(seed, multi) for seed in (0, 1)]
    refs = [L.render_lines_numpy(TWO_CALL_ENV, px, px, b[3]) for b in batches]
    assert all(r[0].sum() > 10000 and r[1].any() for r in refs) and not same(refs[0][0], refs[1][0])

    def fresh():
        G, T = Guarded(px * px * 8), Guarded(24)
        G.write(np.zeros(px * px)); T.write(np.zeros(3, np.int64))
        return G, T

    def render(b, G, T):
        assert gpu.lib.gm_density_lines(gpu.handle, ctypes.byref(b[0]), None, b[2], None, None, 0, ctypes.byref(g), G.ptr,
                                        T.ptr) == _lib.GM_OK, _lib.last_error()

    for k, (b, (want, tally)) in enumerate(zip(batches, refs)):
        G, T = fresh()
        render(b, G, T)
        gpu.sync()
        assert same(G.read(np.float64).reshape(px, px), want) and T.read(np.int64).tolist() == tally.tolist(), k
    G, T = fresh()
    render(batches[0], G, T)
    render(batches[1], G, T)
    gpu.sync()
    assert same(G.read(np.float64).reshape(px, px), refs[0][0] + refs[1][0])
    assert T.read(np.int64).tolist() == (refs[0][1] + refs[1][1]).tolist()
    for buf in batches[0][1] + batches[1][1] + [G, T]:
        buf.check("two calls")
