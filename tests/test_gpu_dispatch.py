"""Every kernel instantiation an entry point can reach, once: the run-time switches that become template
arguments in geomesa_amd/csrc (period, lenient, status given or NULL, all columns 16-B aligned or not, f32,
during, the spatial op) walked as a grid per entry point, each point bit for bit against the C oracle on
guarded buffers (abi_buffers.Guarded).  The other GPU tests vary one switch at a time.

Sizes: an index batch has n = 2 x block + 5 rows with the kernel's own block (the IndexCase blocks of
test_gpu_abi_contract.py), so it crosses a block edge and ends on the odd last row; a scan has
2 x 4096 + 5 rows (FROWS = 4096); the histogram has 2 x 2048 + 5 points (HTPB 1024 lanes x 2 rows), one pass.

Inputs make a wrong instantiation visible, and the `distinct` assertions prove it from the oracle alone:
  lenient   every index batch holds points outside the world: lenient clamps them, strict fails them
  period    epoch-millisecond times of 2020 give four different bins (18262.. / 2609.. / 600.. / 50); every
            such batch also holds a time before 1970, which fails in both modes
  status    the returned array equals the oracle's (a kernel without STATUS leaves the 0xA5 fill); without a
            status the failed rows make the call answer GM_E_ELEMENT
  aligned   "moved" shifts one column by 8 B: same expectation, the kernel without 16-B loads (scalar index
            kernels; the scans' VEC = false instantiations)
  during / op / boxes   the scans' masks differ between neighbouring grid points
The Arrow Z3 key with dtg = NULL indexes every row at time 0, which normalises to the same z in every
period: there the period shows only through the variants that have a dtg column.

The twelve k_range_mask instantiations are walked by test_gpu_table_scan.py::test_every_instantiation.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import test_gpu_abi_contract as A
from abi_buffers import Guarded
from test_gpu_abi_contract import E_ELEMENT, F64, I64, OK, T2020, U8, U64, P

pytestmark = pytest.mark.gpu

PERIODS = (0, 1, 2, 3)
MOVE = 8                    # bytes: 8-B aligned, not 16-B
YEAR_Z3 = 1                 # GM_LEGACY_YEAR_Z3


def differ(a, b):
    """Two oracle expectations ([outputs], status) are not the same answer."""
    return any(not np.array_equal(u, v) for u, v in zip(a[0] + [a[1]], b[0] + [b[1]]))


def distinct(want, keys, what):
    """Expectations of neighbouring grid points differ pairwise."""
    for p, q in itertools.combinations(keys, 2):
        assert differ(want[p], want[q]), "%s: %s and %s expect the same answer" % (what, p, q)


# ---------------------------------------------------------------- index entry points
def _c_legacy_year_z3():
    def call(lib, h, i, n, o, st, sm, period=A.WEEK, lenient=0):
        return lib.gm_legacy_z3_index(h, i[0], i[1], i[2], n, YEAR_Z3, period, lenient, o[0], st, sm)

    def cols(rng, n):      # offsets up to maxOffset(Year), past the curve's 52 weeks of minutes
        import oracle as O
        return [rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.integers(0, O.max_offset(3) + 1, n)]

    def expect(O, c, period=A.WEEK, lenient=False):
        return A.loop_expect(len(c[0]), lambda i: (lambda s, z: (s, [z]))(
            *O.legacy_year_z3_index(c[0][i], c[1][i], int(c[2][i]), lenient)))([I64])
    return A.IndexCase(256, cols, A.spoil_xyt(-1), [I64], call, expect)


CASES = dict(A.INDEX_CASES, gm_legacy_year_z3_index=_c_legacy_year_z3)


@functools.lru_cache(maxsize=None)
def index_batch(name):
    """(case, columns) of one entry point: 2 x block + 5 rows, row 1, a row of the second block and the odd
    last row spoiled (a point outside the world, a bad time where there is one, a second point outside)."""
    case = CASES[name]()
    n = 2 * case.block + 5
    cols = case.cols(np.random.default_rng(977 * len(name) + n), n)
    case.spoil(cols, [1, case.block + 7, n - 1])
    return case, cols


@functools.lru_cache(maxsize=None)
def index_want(name, periods, lenients):
    """{(period, lenient): ([outputs], status)} from the oracle, neighbouring grid points distinct."""
    import oracle as O
    case, cols = index_batch(name)
    want = {(p, le): case.expect(O, cols, p, bool(le)) for p in periods for le in lenients}
    for p in periods:
        distinct(want, [(p, le) for le in lenients], name + " lenient")
    for le in lenients:
        distinct(want, [(p, le) for p in periods], name + " period")
    return want


def run_point(gpu, case, dev_cols, want, period, lenient, with_status, moved=None, what=""):
    """One grid point: the call on guarded buffers (`moved`: the ("in" | "out", k) column shifted by 8 B),
    its return code, summary, status and outputs against the oracle's."""
    exp, est = want
    bound = A.IndexCase(case.block, None, None, case.outs,
                        functools.partial(case.call, period=period, lenient=lenient), None)
    rc, outs, st, sm = A.run_index(gpu, bound, dev_cols, len(est), with_status, True,
                                   {"moved": MOVE} if moved else None, {moved: "moved"} if moved else None)
    fails = np.flatnonzero(est)
    assert rc == (E_ELEMENT if len(fails) and not with_status else OK), (what, rc)
    assert sm == ((len(fails), int(fails[0]), int(est[fails[0]])) if len(fails) else (0, -1, 0)), (what, sm)
    if with_status:
        assert np.array_equal(st, est), (what, np.flatnonzero(st != est)[:8])
    for got, w in zip(outs, exp):
        assert np.array_equal(got, w), (what, np.flatnonzero(got != w)[:8])


INDEX_GRID = {      # entry point: (periods, lenients, moved columns)
    "gm_z3_index_key": (PERIODS, (0, 1), (None, ("in", 0))),
    "gm_z3_index": ((A.WEEK,), (0, 1), (None,)),
    "gm_z2_index": ((A.WEEK,), (0, 1), (None, ("in", 0))),
    "gm_xz2_index": ((A.WEEK,), (0, 1), (None, ("in", 0))),
    "gm_xz3_index": ((A.WEEK,), (0, 1), (None, ("in", 0))),
    "gm_binned_time": (PERIODS, (0,), (None,)),
    "gm_xz3_index_key": (PERIODS, (0, 1), (None,)),
    "gm_legacy_year_z3_index": ((A.WEEK,), (0, 1), (None,)),
}


def index_points(name):
    periods, lenients, moves = INDEX_GRID[name]
    return [(p, le, s, m) for p in periods for le in lenients for s in (True, False) for m in moves]


@pytest.mark.parametrize("name", list(INDEX_GRID))
def test_index_grid(gpu, name):
    """period x lenient x status given / NULL x aligned / one column moved, as far as the entry point has the
    switch: each point equals the oracle's answer for exactly that point."""
    periods, lenients, _ = INDEX_GRID[name]
    case, cols = index_batch(name)
    want = index_want(name, periods, lenients)
    for p, le, s, m in index_points(name):
        run_point(gpu, case, cols, want[(p, le)], p, le, s, m, (name, p, le, s, m))


# ---------------------------------------------------------------- Arrow entry points
def arrow_case(name, f32, dtg):
    """The IndexCase of an Arrow entry point with a Float4 / Float8 point column and with or without dtg."""
    case = A.INDEX_CASES[name]()

    def call(lib, h, i, n, o, st, sm, period=A.WEEK, lenient=0):
        g = A.point_struct(None)
        g.ordinal_bits, g.coords = (32 if f32 else 64), i[0].value
        t = A.time_struct(None)
        t.millis = i[1].value if dtg else None
        gp, tp = ctypes.byref(g), (ctypes.byref(t) if dtg else None)
        if name == "gm_z3_index_key_arrow":
            return lib.gm_z3_index_key_arrow(h, gp, tp, n, period, lenient, o[0], o[1], st, sm)
        if name == "gm_z2_index_key_arrow":
            return lib.gm_z2_index_key_arrow(h, gp, n, lenient, o[0], st, sm)
        if name == "gm_xz2_index_key_arrow":
            return lib.gm_xz2_index_key_arrow(h, gp, n, 12, lenient, o[0], st, sm)
        return lib.gm_xz3_index_key_arrow(h, gp, tp, n, 12, period, lenient, o[0], o[1], st, sm)
    return A.IndexCase(case.block, case.cols, case.spoil, case.outs, call, case.expect)


@functools.lru_cache(maxsize=None)
def arrow_want(name, f32, dtg, periods):
    """(device columns, {(period, lenient): expectation}): Float4 coordinates reach the oracle as the doubles
    they convert to, a missing dtg as time 0."""
    import oracle as O
    case, cols = index_batch(name)
    coords = cols[0].astype(np.float32) if f32 else cols[0]
    t = cols[1] if dtg else np.zeros(len(cols[1]), I64)
    want = {(p, le): case.expect(O, [coords.astype(F64), t], p, bool(le)) for p in periods for le in (0, 1)}
    for p in periods:
        distinct(want, [(p, 0), (p, 1)], name + " lenient")
    if dtg:
        for le in (0, 1):
            distinct(want, [(p, le) for p in periods], name + " period")
    return [coords, t], want


ARROW_GRID = {      # entry point: (periods, [(dtg, moved column)])
    # the four kernels of launch_z3_arrow: vector with dtg, vector without, coordinates moved (pair kernel
    # with vector stores), z moved (pair kernel with scalar stores)
    "gm_z3_index_key_arrow": (PERIODS, [(True, None), (False, None), (True, ("in", 0)), (True, ("out", 1))]),
    "gm_z2_index_key_arrow": ((A.WEEK,), [(True, None), (True, ("out", 0))]),
    "gm_xz2_index_key_arrow": ((A.WEEK,), [(True, None)]),
    "gm_xz3_index_key_arrow": (PERIODS, [(True, None)]),
}


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(ARROW_GRID))
def test_arrow_grid(gpu, name, f32):
    """period x lenient x Float4 / Float8 x the entry point's kernels; status given on every point and NULL on
    the first variant."""
    periods, variants = ARROW_GRID[name]
    for k, (dtg, moved) in enumerate(variants):
        case = arrow_case(name, f32, dtg)
        cols, want = arrow_want(name, f32, dtg, periods)
        for p in periods:
            for le in (0, 1):
                for s in ((True, False) if k == 0 else (True,)):
                    run_point(gpu, case, cols, want[(p, le)], p, le, s, moved, (name, f32, dtg, moved, p, le, s))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_points_to_columns_grid(gpu, f32):
    n = 2 * 256 + 5
    rng = np.random.default_rng(n)
    c = A.interleave_yx(rng.uniform(-180, 180, n), rng.uniform(-90, 90, n))
    c = c.astype(np.float32) if f32 else c
    C, X, Y = Guarded.of(c), Guarded(8 * n), Guarded(8 * n)
    g = A.point_struct(C)
    g.ordinal_bits = 32 if f32 else 64
    assert gpu.lib.gm_arrow_points_to_columns(gpu.handle, ctypes.byref(g), n, X.ptr, Y.ptr) == OK
    A.sync(gpu)
    A.check_all([C, X, Y])
    assert np.array_equal(X.read(F64), c[1::2].astype(F64)) and np.array_equal(Y.read(F64), c[0::2].astype(F64))


# ---------------------------------------------------------------- histogram
HIST_N = 2 * 2048 + 5
HIST_LO = {0: 18262, 1: 2605, 2: 598, 3: 40}      # the window's first bin per period: 50 days of 2020 fit
# (length, n_bins): 32-bit LDS counters (n_bins x (length + 1) <= 32768) and the packed WIDE counters, each with a
# power-of-two length (the TOP path) and another (1000 x 54 is WIDE as 1024 x 54 is, and not a power of two)
HIST_SHAPES = {("int32", True): (512, 53), ("int32", False): (500, 53), ("wide", True): (1024, 54),
               ("wide", False): (1000, 54)}


@functools.lru_cache(maxsize=None)
def hist_points():
    rng = np.random.default_rng(HIST_N)
    x, y = rng.uniform(-180, 180, HIST_N), rng.uniform(-90, 90, HIST_N)
    t = T2020 + rng.integers(0, 50 * 86400000, HIST_N)
    x[1], t[2049], y[HIST_N - 1] = 200.0, -5, -91.0
    return x, y, t


@functools.lru_cache(maxsize=None)
def hist_want(period, unobserve, length, nb):
    """(start state, expected state) as (present, counts, tally): observe from a sparse non-zero state;
    unobserve of the first half from the observed state."""
    import oracle as O
    x, y, t = hist_points()
    p0, c0, t0 = np.zeros(nb, U8), np.zeros((nb, length), I64), np.array([5, 9], I64)
    c0[::3, ::5] = 2
    seen = O.z3_histogram(x, y, t, length, HIST_LO[period], nb, period=period, present=p0.copy(), counts=c0.copy(),
                          tally=t0.copy())
    if not unobserve:
        return (p0, c0, t0), seen
    h = HIST_N // 2
    gone = O.z3_histogram(x[:h], y[:h], t[:h], length, HIST_LO[period], nb, unobserve=True, period=period,
                          present=seen[0].copy(), counts=seen[1].copy(), tally=seen[2].copy())
    assert not np.array_equal(gone[1], seen[1])
    return seen, gone


@pytest.mark.parametrize("counters", ["int32", "wide"])
@pytest.mark.parametrize("period", PERIODS)
def test_histogram_grid(gpu, period, counters):
    """period x observe / unobserve x {aligned with a power-of-two length, aligned without, x moved by 8 B} x
    the two LDS counter layouts: the six k_z3_hist_lds instantiations of each (period, unobserve)."""
    x, y, t = hist_points()
    first = None
    for unobserve in (0, 1):
        for pow2, moved in ((True, 0), (False, 0), (True, MOVE)):
            length, nb = HIST_SHAPES[(counters, pow2)]
            start, want = hist_want(period, unobserve, length, nb)
            first = first if first is not None else want
            h = HIST_N // 2 if unobserve else HIST_N
            ins = [Guarded.of(x[:h], moved), Guarded.of(y[:h]), Guarded.of(t[:h])]
            outs = [Guarded.of(a) for a in start]
            rc = gpu.lib.gm_z3_histogram(gpu.handle, P(ins[0]), P(ins[1]), P(ins[2]), h, period, length, unobserve,
                                         HIST_LO[period], nb, P(outs[0]), P(outs[1]), P(outs[2]))
            A.sync(gpu)
            what = (period, counters, unobserve, pow2, moved)
            assert rc == OK, what
            A.check_all(ins + outs, str(what))
            assert np.array_equal(outs[0].read(U8), want[0]), what
            assert np.array_equal(outs[1].read(I64).reshape(nb, length), want[1]), what
            assert np.array_equal(outs[2].read(I64), want[2]), what
    if period:      # another period counts the same points differently
        assert not np.array_equal(first[1], hist_want(0, 0, *HIST_SHAPES[(counters, True)])[1][1])


# ---------------------------------------------------------------- scans
SCAN_N = 2 * 4096 + 5
BBOX = np.array([-180.0, -90.0, 0.0, 90.0])
DURING = (T2020 + 90 * 86400000, T2020 + 270 * 86400000)


@functools.lru_cache(maxsize=None)
def scan_cols():
    import oracle as O
    x, y, t = A.xyt_ms(np.random.default_rng(SCAN_N), SCAN_N)
    b, z, st = O.z3_index_key_batch(x, y, t, False, A.WEEK)
    z2, st2 = O.z2_index_batch(x, y, False)
    assert not st.any() and not st2.any()
    return x, y, t, b, z, z2


def run_scan(gpu, ins, call, mask, what):
    """call(mask, ids, ids_cap, n_match) -> rc on guarded outputs sized to the oracle's answer."""
    words, ids = A._pack(mask), np.flatnonzero(mask)
    assert 0 < len(ids) < len(mask), what
    M, I = Guarded(len(words) * 8), Guarded(len(ids) * 8)
    nm = ctypes.c_int64(-7)
    rc = call(M.ptr, I.ptr, len(ids), ctypes.byref(nm))
    A.sync(gpu)
    A.check_all(ins + [M, I], str(what))
    assert (rc, nm.value) == (OK, len(ids)), (what, rc, nm.value)
    got = M.read(U64)
    assert np.array_equal(got, words), (what, np.flatnonzero(got != words)[:8])
    assert np.array_equal(I.read(I64), ids), what


def all_differ(masks, what):
    for p, q in itertools.combinations(masks, 2):
        assert not np.array_equal(masks[p], masks[q]), "%s: %s and %s expect the same mask" % (what, p, q)


@functools.lru_cache(maxsize=None)
def strict_masks():
    import oracle as O
    x, y, t = scan_cols()[:3]
    masks = {d: O.strict_scan(x, y, t, BBOX, DURING if d else None) for d in (0, 1)}
    all_differ(masks, "gm_strict_scan during")
    return masks


def test_strict_scan_grid(gpu):
    """during x aligned / x moved: k_strict_mask_v<D, VEC>, all four."""
    x, y, t = scan_cols()[:3]
    masks = strict_masks()
    for d, moved in itertools.product((0, 1), (0, MOVE)):
        ins = [Guarded.of(x, moved), Guarded.of(y), Guarded.of(t)]
        run_scan(gpu, ins, lambda m, i, c, nm: gpu.lib.gm_strict_scan(
            gpu.handle, P(ins[0]), P(ins[1]), P(ins[2]), SCAN_N, BBOX.ctypes.data, d, DURING[0], DURING[1], m, i, c,
            nm), masks[d], ("gm_strict_scan", d, moved))


def _strips(k, bits):
    """k boxes: every other 1/16-wide strip of a `bits`-bit dimension, over the whole of the other one."""
    w = 1 << (bits - 4)
    return [[2 * j * w, 0, (2 * j + 1) * w - 1, (1 << bits) - 1] for j in range(k)]


# five bin ranges (more than FBIN = 4), every other five weeks of 2020's weekly bins 2608..2661
BIN_RANGES = np.array([[2608 + 12 * j, 2612 + 12 * j] for j in range(5)], np.int16)


@functools.lru_cache(maxsize=None)
def filter_masks(entry):
    """({boxes: filter bytes}, {(boxes, bin ranges): mask}) for 2 and 5 boxes and, for Z3, 2 boxes with the
    five BIN_RANGES."""
    import oracle as O
    from geomesa_amd import filters as F
    x, y, t, b, z, z2 = scan_cols()
    z3 = entry == "gm_z3filter_scan"
    fbs, masks = {}, {}
    for k in (2, 5):
        fbs[k] = (F.serialize_to_bytes(F.Z3Filter(_strips(k, 21), [], 32767, -32768)) if z3 else
                  F.z2_serialize_to_bytes(F.Z2Filter(_strips(k, 31))))
        masks[(k, 0)] = O.z3filter_scan(fbs[k], [], b, z) if z3 else O.z2filter_scan(fbs[k], z2)
    if z3:
        masks[(2, 5)] = O.z3filter_scan(fbs[2], BIN_RANGES, b, z)
    all_differ(masks, entry + " boxes and bin ranges")
    return fbs, masks


@pytest.mark.parametrize("entry", ["gm_z3filter_scan", "gm_z2filter_scan"])
def test_filter_scan_grid(gpu, entry):
    """{at most FBOX = 4 boxes, more than 4} x {aligned, z moved}: k_*filter_mask_v<FAST, VEC>, all four; and
    for Z3 more than FBIN = 4 bin ranges on the moved z, the other way to <false, false>."""
    x, y, t, b, z, z2 = scan_cols()
    z3 = entry == "gm_z3filter_scan"
    fbs, masks = filter_masks(entry)
    for k, nbr, moved in ((2, 0, 0), (5, 0, 0), (2, 0, MOVE), (5, 0, MOVE)) + (((2, 5, MOVE),) if z3 else ()):
        fb = np.frombuffer(fbs[k], U8).copy()
        if z3:
            ins = [Guarded.of(b), Guarded.of(z, moved)]
            br = BIN_RANGES.ctypes.data if nbr else None
            call = lambda m, i, c, nm: gpu.lib.gm_z3filter_scan(gpu.handle, fb.ctypes.data, len(fb), br, nbr,  # noqa: E731
                                                                P(ins[0]), P(ins[1]), SCAN_N, m, i, c, nm)
        else:
            ins = [Guarded.of(z2, moved)]
            call = lambda m, i, c, nm: gpu.lib.gm_z2filter_scan(gpu.handle, fb.ctypes.data, len(fb), P(ins[0]),  # noqa: E731
                                                                SCAN_N, m, i, c, nm)
        run_scan(gpu, ins, call, masks[(k, nbr)], (entry, k, nbr, moved))


@pytest.mark.parametrize("entry", ["gm_z3filter_scan_rows", "gm_z2filter_scan_rows"])
def test_filter_rows_scan(gpu, oracle, entry):
    """k_filter_rows_mask<true> and <false>, one case each."""
    s = A.Scan(gpu, oracle, entry)
    assert s.run(gpu, s.m) == (OK, s.m)


QBOX = np.array([1.0, 1.0, 48.0, 9.0])
QDUR = (100, 700)


@functools.lru_cache(maxsize=None)
def query_masks():
    """(points, {(during, op): mask}) over the shapes of test_gpu_query.py, vertex and edge points kept."""
    import oracle as O
    from geomesa_amd.join import PolygonSet
    from test_gpu_query import SHAPES, _points
    ps = PolygonSet.from_wkt(SHAPES)
    qx, qy, qt = _points(SCAN_N, 5, ps)
    k = np.random.default_rng(6).permutation(len(qx))[:SCAN_N]
    qx, qy, qt = qx[k], qy[k], qt[k]
    ops = O.OraclePolySet(*ps.to_arrays())
    masks = {(d, op): O.query_scan(qx, qy, qt, bbox=QBOX, during=QDUR if d else None, polys=ops if op else None,
                                   op=op) for d in (0, 1) for op in (0, 1, 2)}
    all_differ(masks, "gm_query_scan")
    return (qx, qy, qt), masks


def test_query_scan_grid(gpu):
    """aligned / x moved x during x {no geometry term, intersects, contains}: the twelve k_query_mask."""
    _, ix = A._query_polys()
    (qx, qy, qt), masks = query_masks()
    bbox, dur = QBOX, QDUR
    for moved, (d, op) in itertools.product((0, MOVE), masks):
        ins = [Guarded.of(qx, moved), Guarded.of(qy), Guarded.of(qt)]
        run_scan(gpu, ins, lambda m, i, c, nm: gpu.lib.gm_query_scan(
            gpu.handle, P(ins[0]), P(ins[1]), P(ins[2]), SCAN_N, bbox.ctypes.data, d, dur[0], dur[1],
            ix._h if op else None, op, m, i, c, nm), masks[(d, op)], ("gm_query_scan", moved, d, op))


def expectations():
    """Every oracle expectation of this file and its `distinct` assertions, without a GPU."""
    for name, (periods, lenients, _) in INDEX_GRID.items():
        index_want(name, periods, lenients)
    for name, (periods, variants) in ARROW_GRID.items():
        for f32 in (False, True):
            for dtg in {v[0] for v in variants}:
                arrow_want(name, f32, dtg, periods)
    for period in PERIODS:
        for length, nb in HIST_SHAPES.values():
            hist_want(period, 1, length, nb)
    strict_masks()
    filter_masks("gm_z3filter_scan")
    filter_masks("gm_z2filter_scan")
    query_masks()
