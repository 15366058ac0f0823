"""The range kernels (gm_ranges_z.hip, gm_ranges_xz.hip) against what a range list must be, and against the oracle where no
other test varies the parameter.

Sections 1-3 run the kernels under the checkers of ranges_definition.py at the inputs, and with the
no-vacuous-pass conditions, that test_ranges_definition.py has shown the oracle to satisfy: no oracle is
consulted, so a misreading that kernel and oracle shared would still fail here.  Sections 4-5 are exact
list equality with the oracle, as in test_gpu_scan_join_ranges.py: every g, period and precision, lists
long enough for the second phase and the global-memory sort, and the two statuses that are limits of
this library (GM_QS_CAPACITY, GM_QS_TOO_MANY_BOUNDS)."""
import ctypes

import numpy as np
import pytest

import ranges_definition_cases as C

pytestmark = pytest.mark.gpu


def as_np(t):
    return t.detach().cpu().numpy()


class KernelBackend:
    """The entry points under test, in the shape the shared test bodies call."""

    @staticmethod
    def zranges(D, qs, mr, rec):
        from geomesa_amd import ranges as R
        return [r.arr for r in R.zranges(D, qs, 64, mr, rec)]

    @staticmethod
    def z_user_ranges(period, precision, qs, mr):
        from geomesa_amd.curve import Z2SFC, Z3SFC
        if period is None:
            return [r.arr for r in Z2SFC(precision).ranges_batch([b for b, _ in qs], 64, mr)]
        return [r.arr for r in Z3SFC(period, precision).ranges_batch(qs, 64, mr)]

    @staticmethod
    def z_user_index(period, precision, x, y, t):
        from geomesa_amd.curve import Z2SFC, Z3SFC
        if period is None:
            return as_np(Z2SFC(precision).index(x, y))
        return as_np(Z3SFC(period, precision).index(x, y, t))

    @staticmethod
    def xz_ranges(D, g, period, qs, mr):
        from geomesa_amd.curve import XZ2SFC, XZ3SFC
        sfc = XZ2SFC(g) if D == 2 else XZ3SFC(g, period)
        return [r.arr for r in sfc.ranges_batch(qs, mr)]

    @staticmethod
    def xz_index(D, g, period, env):
        from geomesa_amd.curve import XZ2SFC, XZ3SFC
        sfc = XZ2SFC(g) if D == 2 else XZ3SFC(g, period)
        return as_np(sfc.index(*[np.ascontiguousarray(env[:, k]) for k in range(2 * D)]))


K = KernelBackend


# ---------------------------------------------------------------- 1. gm_zranges on an enumerated universe
@pytest.mark.parametrize("setting", C.Z_SETTINGS)
@pytest.mark.parametrize("with_prefix", [0, 1])
@pytest.mark.parametrize("D,bits", C.Z_RAW)
def test_zranges_definition(gpu, D, bits, with_prefix, setting):
    """Z1-Z5 (ranges_definition.check_z_list) on gm_zranges: 24 queries of 1-3 bounds and one of 256
    (MAXB) in one call, with and without a shared high prefix."""
    fails, _ = C.run_z_raw(K.zranges, D, bits, with_prefix, setting)
    assert not fails, fails[:3]


# ---------------------------------------------------------------- 2. gm_z3_ranges / gm_z2_ranges, user space
@pytest.mark.parametrize("budget", C.Z_BUDGETS)
@pytest.mark.parametrize("period,precision", C.Z3_USER + [(None, p) for p in C.Z2_USER])
def test_z_user_space_cover(gpu, period, precision, budget):
    """Cover and soundness (check_cover) of Z3SFC(period, precision) / Z2SFC(precision) ranges over points
    indexed by gm_z3_index / gm_z2_index at the same precision: boxes on +180 / +90 / the period's
    max offset, on the world's minimum, of zero size; points on box edges and cell lines."""
    fails, _ = C.run_z_user(K.z_user_ranges, K.z_user_index, period, precision, budget)
    assert not fails, fails[:3]


# ---------------------------------------------------------------- 3. gm_xz2_ranges / gm_xz3_ranges
@pytest.mark.parametrize("budget", C.XZ_ELEMENT_BUDGETS)
@pytest.mark.parametrize("D,g,period", [(2, g, "week") for g in C.XZ2_ELEMENT_G] +
                         [(3, g, p) for g in C.XZ3_ELEMENT_G for p in C.PERIODS])
def test_xz_elements_definition(gpu, D, g, period, budget):
    """X1-X3 (check_xz_list) against every element of levels 1..g: 20 queries of 1-3 windows, one of 17
    (past the 16 that the first pass stages) and one of 256 (MAXB), in one call."""
    fails, _ = C.run_xz_elements(K.xz_ranges, D, g, period, budget)
    assert not fails, fails[:3]


XZ_END = [(2, g, "week") for g in C.XZ2_END_G] + [(3, g, p) for g in C.XZ3_END_G for p in C.XZ3_END_PERIODS]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("D,g,period", XZ_END)
def test_xz_end_to_end_cover(gpu, D, g, period, which):
    """Cover and soundness over 4,000 envelopes indexed by gm_xz2_index / gm_xz3_index at the same g, up
    to the largest g: zero-size and world-size envelopes, generic coordinates and coordinates on the
    2^-(g+1) lattice (exact ties with element and window edges)."""
    fails, _ = C.run_xz_end(K.xz_ranges, K.xz_index, D, g, period, C.xz_end_budgets(g)[which])
    assert not fails, fails[:3]


# ---------------------------------------------------------------- 4. oracle parity at every g, period, precision
def triples(r):
    return [tuple(x) for x in r]


@pytest.mark.parametrize("D,g,period", [(2, g, "week") for g in C.XZ2_END_G] +
                         [(3, g, p) for g in C.XZ3_END_G for p in C.PERIODS])
def test_xz_ranges_parity_every_g_and_period(gpu, oracle, D, g, period):
    qs = C.xz_parity_queries(D, period, seed=600 + g)
    p = oracle.PERIODS[period]
    for mr in [2000] + ([None] if g <= 6 else []):
        got = K.xz_ranges(D, g, period, qs, mr)
        for q, r in zip(qs, got):
            exp = oracle.xz2_ranges(q, mr, g=g) if D == 2 else oracle.xz3_ranges(q, mr, g=g, period=p)
            assert [(int(a), int(b), bool(c)) for a, b, c, _ in r.tolist()] == exp, (mr, q)


@pytest.mark.parametrize("period,precision", [("day", 21), ("month", 21), ("year", 21),
                                              ("week", 1), ("week", 10), ("week", 20)])
def test_z3_ranges_parity_every_period_and_precision(gpu, oracle, period, precision):
    from geomesa_amd.curve import Z3SFC
    qs = C.parity_queries(80, seed=43, period=period)
    for mr in [2000, 7] + ([None] if precision == 1 else []):
        got = Z3SFC(period, precision).ranges_batch([([b], [t]) for b, t in qs], 64, mr)
        for (b, t), r in zip(qs, got):
            exp = oracle.z3_ranges([b], [t], max_ranges=mr, period=oracle.PERIODS[period], sfc_precision=precision)
            assert triples(r) == exp, (mr, b, t)


@pytest.mark.parametrize("precision", [1, 16, 30])
def test_z2_ranges_parity_every_precision(gpu, oracle, precision):
    from geomesa_amd.curve import Z2SFC
    qs = [b for b, _ in C.parity_queries(80, seed=47)]
    for mr in [1000, 7, None]:
        got = Z2SFC(precision).ranges_batch([[b] for b in qs], 64, mr)
        for b, r in zip(qs, got):
            assert triples(r) == oracle.z2_ranges([b], max_ranges=mr, sfc_precision=precision), (mr, b)


@pytest.mark.parametrize("max_ranges", [5000, 20000])
def test_z2_ranges_long_list_second_phase(gpu, oracle, max_ranges):
    """k_zranges<2> past the first phase's 4,096-range workspace and the LDS sort: the budget fires with
    at least max_ranges ranges held (test_ranges_definition.test_oracle_long_lists_are_long), so the
    query is run again in phase 2 and sorted in global memory.  With Z2SFC's default 7 levels this box
    gives 30 ranges at any budget; the walk here goes to the last level (max_recurse past it), and the
    oracle's is Z2.zranges on the box's corners."""
    from geomesa_amd.curve import Z2SFC
    boxes = [C.TINY[0][0], C.BIG_BOX, C.TINY[1][0]]
    got = Z2SFC().ranges_batch([[b] for b in boxes], 64, max_ranges, max_recurse=C.LARGE)
    for b, r in zip(boxes, got):
        assert triples(r) == oracle.zranges(2, [C.z2_corners(oracle, b)], 64, max_ranges, C.LARGE)
    assert len(got[1]) > 500
    # and the default recursion, which the oracle's z2_ranges has
    got = Z2SFC().ranges_batch([[b] for b in boxes], 64, max_ranges)
    for b, r in zip(boxes, got):
        assert triples(r) == oracle.z2_ranges([b], max_ranges=max_ranges)


def test_z3_ranges_list_past_the_unbounded_floor(gpu, oracle):
    """A budget of 70,000: workspace caps (70,024) above the 65,536 floor that an unbounded call gets, a
    walk that holds 70,000 ranges when it stops, sorted in global memory."""
    from geomesa_amd.curve import Z3SFC
    qs = [C.TINY[0], (C.BIG_BOX, C.BIG_T), C.TINY[1]]
    got = Z3SFC("week").ranges_batch([([b], [t]) for b, t in qs], 64, 70000)
    for (b, t), r in zip(qs, got):
        exp = oracle.z3_ranges([b], [t], max_ranges=70000)
        lo, hi, c = (np.array(v) for v in zip(*exp))
        assert np.array_equal(r.arr["lower"], lo) and np.array_equal(r.arr["upper"], hi)
        assert np.array_equal(r.arr["contained"].astype(bool), c)
    assert len(got[1]) > 30000


# ---------------------------------------------------------------- 5. the two project-limit statuses
QS_CAPACITY, QS_TOO_MANY_BOUNDS = 4, 5
CAP = 1 << 16


def raw(fn, args, nq):
    """One call of a ranges entry point with host outputs: (rc, offsets, ranges, needed, status)."""
    from geomesa_amd import ranges as R
    off = np.full(nq + 1, -1, np.int64)
    out = np.zeros(CAP, R.RANGE_DTYPE)
    need = ctypes.c_int64(-1)
    st = np.full(nq, -1, np.int32)
    rc = fn(*args, off.ctypes.data, out.ctypes.data, CAP, ctypes.byref(need), st.ctypes.data)
    return rc, off, out, need.value, st


def entry(kind, queries, mr, period="week", g=12):
    """(fn, args, keep-alive arrays) of one entry point for `queries`: z3 [(boxes, intervals)], z2 [boxes],
    zranges2 / zranges3 [[(zmin, zmax)]], xz2 / xz3 [windows]."""
    from geomesa_amd import _lib
    from geomesa_amd import ranges as R
    from geomesa_amd.curve import Z3SFC, TimePeriod
    ctx = _lib.context()
    nq = len(queries)
    if kind == "z3":
        fn, args, _, _ = R.prepare_z3(Z3SFC(period), queries, 64, mr)
        return fn, args, ()
    if kind in ("xz2", "xz3"):
        off, w = R._windows(queries, 2 if kind == "xz2" else 3)
        if kind == "xz2":
            return ctx.lib.gm_xz2_ranges, (ctx.handle, nq, off.ctypes.data, w.ctypes.data, g, mr or 0), (off, w)
        return ctx.lib.gm_xz3_ranges, (ctx.handle, nq, off.ctypes.data, w.ctypes.data, g, TimePeriod.of(period),
                                       mr or 0), (off, w)
    width = 4 if kind == "z2" else 2
    flat = [v for q in queries for b in q for v in b]
    off = np.cumsum([0] + [len(q) for q in queries]).astype(np.int32)
    vals = np.asarray(flat, np.float64 if kind == "z2" else np.int64)
    assert len(vals) == width * off[-1]
    if kind == "z2":
        return ctx.lib.gm_z2_ranges, (ctx.handle, nq, off.ctypes.data, vals.ctypes.data, 31, 64, mr or 0, -1), (off, vals)
    return ctx.lib.gm_zranges, (ctx.handle, int(kind[-1]), nq, off.ctypes.data, vals.ctypes.data, 64, mr or 0, -1), \
        (off, vals)


def delivered(off, out, q):
    return [(int(r["lower"]), int(r["upper"]), bool(r["contained"])) for r in out[int(off[q]):int(off[q + 1])]]


@pytest.mark.parametrize("kind", ["z3", "z2", "zranges2", "zranges3", "xz2", "xz3"])
def test_too_many_bounds_is_status_5_and_spares_the_neighbours(gpu, oracle, kind):
    """257 bounds or windows in the middle query of three: that query gets GM_QS_TOO_MANY_BOUNDS and no
    ranges, the call succeeds, *needed counts the other two and they deliver the oracle's lists.  For Z3
    the bounds are the cross product: 257 boxes x 1 interval, and 17 x 16 = 272."""
    from geomesa_amd import _lib
    rng = np.random.default_rng(5)
    (b0, t0), (b1, t1) = C.TINY
    boxes = [(x, y, x + 0.5, y + 0.5) for x, y in zip(rng.uniform(-170, 170, 257), rng.uniform(-80, 80, 257))]
    tt = [(int(t), int(t) + 100) for t in rng.integers(0, 600000, 16)]
    if kind == "z3":
        ends = [([b0], [t0]), ([b1], [t1])]
        mids = [(boxes, [t0]), (boxes[:17], tt)]
        exp = [oracle.z3_ranges(b, t, max_ranges=300) for b, t in ends]
    elif kind == "z2":
        ends, mids = [[b0], [b1]], [boxes]
        exp = [oracle.z2_ranges(b, max_ranges=300) for b in ends]
    elif kind.startswith("zranges"):
        D = int(kind[-1])
        zb = C.z_raw_queries(D, 5, 0, seed=9)
        ends, mids = [zb[1], zb[2]], [zb[-1] + zb[-1][:1]]
        exp = [oracle.zranges(D, b, 64, 300, 7) for b in ends]
    else:
        wins = C.xz_element_queries(int(kind[-1]), "week", seed=10)
        ends, mids = [wins[1], wins[2]], [wins[-1] + wins[-1][:1]]
        exp = [(oracle.xz2_ranges if kind == "xz2" else oracle.xz3_ranges)(w, 300, g=12) for w in ends]
    for mid in mids:
        assert (len(mid[0]) * len(mid[1]) if kind == "z3" else len(mid)) in (257, 272)
        fn, args, keep = entry(kind, [ends[0], mid, ends[1]], 300)
        rc, off, out, need, st = raw(fn, args, 3)
        assert rc == _lib.GM_OK
        assert st.tolist() == [0, QS_TOO_MANY_BOUNDS, 0]
        assert off.tolist() == [0, len(exp[0]), len(exp[0]), len(exp[0]) + len(exp[1])] and need == off[3]
        assert delivered(off, out, 0) == exp[0] and delivered(off, out, 2) == exp[1] and len(exp[0]) > 0
        del keep   # the input arrays, alive across the call


def test_z3_unbounded_past_the_caps_is_status_4(gpu, oracle):
    """An unbounded Z3 query whose walk outgrows the 65,536-range workspace (a budgeted walk of it holds
    70,000 ranges and cells when it stops, test_oracle_long_lists_are_long) gets GM_QS_CAPACITY and no
    ranges; *needed counts only its neighbours, whose lists are the oracle's."""
    from geomesa_amd import _lib
    qs = [C.TINY[0], (C.BIG_BOX, C.BIG_T), C.TINY[1]]
    fn, args, keep = entry("z3", [([b], [t]) for b, t in qs], None)
    rc, off, out, need, st = raw(fn, args, 3)
    del keep   # the input arrays, alive across the call
    exp = [oracle.z3_ranges([b], [t], max_ranges=None) for b, t in (qs[0], qs[2])]
    assert rc == _lib.GM_OK and st.tolist() == [0, QS_CAPACITY, 0]
    assert off.tolist() == [0, len(exp[0]), len(exp[0]), len(exp[0]) + len(exp[1])] and need == off[3]
    assert delivered(off, out, 0) == exp[0] and delivered(off, out, 2) == exp[1] and len(exp[0]) > 0


def test_xz3_unbounded_past_the_caps_is_status_4(gpu, oracle):
    """The whole world, unbounded, at g = 12: the window contains an element only if the element's index is
    at most 2^L - 2 in every dimension, so level L has 8^L - (2^L - 1)^3 overlapping elements, 64,777
    through level 7 and 195,841 more at level 8: past the 65,536 queued elements that the unbounded
    workspace holds.  GM_QS_CAPACITY, no ranges, and the neighbours' lists are the oracle's."""
    from geomesa_amd import _lib
    assert sum(8 ** L - (2 ** L - 1) ** 3 for L in range(1, 8)) == 64777 and 8 ** 8 - (2 ** 8 - 1) ** 3 == 195841
    wins = [[(b[0], b[1], float(t[0]), b[2], b[3], float(t[1]))] for b, t in C.TINY]
    qs = [wins[0], [(-180.0, -90.0, 0.0, 180.0, 90.0, 604800.0)], wins[1]]
    fn, args, keep = entry("xz3", qs, None)
    rc, off, out, need, st = raw(fn, args, 3)
    del keep   # the input arrays, alive across the call
    exp = [oracle.xz3_ranges(q, None, g=12) for q in (qs[0], qs[2])]
    assert rc == _lib.GM_OK and st.tolist() == [0, QS_CAPACITY, 0]
    assert off.tolist() == [0, len(exp[0]), len(exp[0]), len(exp[0]) + len(exp[1])] and need == off[3]
    assert delivered(off, out, 0) == exp[0] and delivered(off, out, 2) == exp[1] and len(exp[0]) > 0
