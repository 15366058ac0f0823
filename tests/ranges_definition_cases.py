"""The inputs of the range definition tests: one set, drawn from fixed seeds, run by the CPU file through
the oracle and by the GPU file through the kernels.  Plain numpy, no oracle, no GPU."""
import numpy as np

import ranges_definition as RD

PERIODS = ("day", "week", "month", "year")
MAX_OFFSET = {"day": 86400000, "week": 604800, "month": 86400 * 31, "year": 1440 * 366 + 10}   # BinnedTime.maxOffset
LARGE = 1000   # a maxRecurse past every level

# ---------------------------------------------------------------- raw ZN.zranges
Z_RAW = [(2, 8), (3, 5)]   # (D, bits): universes of 2^16 and 2^15 z
Z_SETTINGS = [(None, 64), (None, 7), (None, 2), (200, 3), (50, LARGE), (7, LARGE), (1, LARGE)]   # (max_ranges, max_recurse)
Z_NQ = 24


def z_prefix(D, bits, with_prefix, seed=5):
    """0, or random bits above the universe's D * bits (below bit 62 / 63, the curves' widths)."""
    if not with_prefix:
        return 0
    top = (62 if D == 2 else 63) - D * bits
    return int(np.random.default_rng(seed + D).integers(1, 1 << top)) << (D * bits)


def z_raw_queries(D, bits, prefix, seed):
    """Z_NQ queries of 1-3 raw (zmin, zmax) bounds and one of exactly 256: corners drawn per dimension
    (so zmin <= zmax), thin, small and wide boxes, some touching 0 or the dimension's maximum."""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1

    def bound():
        lo, hi = [], []
        for _ in range(D):
            kind = rng.integers(0, 4)
            size = [0, int(rng.integers(0, 4)), int(rng.integers(0, top // 4 + 1)), int(rng.integers(0, top + 1))][kind]
            a = int(rng.integers(0, top + 1 - size))
            if rng.random() < 0.1:
                a = 0
            if rng.random() < 0.1:
                a = top - size
            lo.append(a); hi.append(a + size)
        zlo = prefix | int(RD.interleave([np.int64(v) for v in lo]))
        zhi = prefix | int(RD.interleave([np.int64(v) for v in hi]))
        return (zlo, zhi)

    qs = [[bound() for _ in range(1 + k % 3)] for k in range(Z_NQ)]
    qs.append([bound() for _ in range(256)])
    return qs


# ---------------------------------------------------------------- Z3SFC / Z2SFC, user space
Z3_USER = [(p, prec) for p in PERIODS for prec in (3, 5)]
Z2_USER = [4, 8]
Z_BUDGETS = [None, 20, 1]
Z_NPTS = 3000


def _cell_lines(lo, hi, precision, rng, n):
    """n coordinates on the curve's cell lines lo + (hi - lo) * k / 2^precision (k = 2^precision: the maximum)."""
    k = rng.integers(0, (1 << precision) + 1, n)
    return lo + (hi - lo) * k / float(1 << precision)


def z_user_case(period, precision, seed):
    """(queries, points): queries = [(boxes, intervals)] (intervals None for Z2, period None), among them a
    max corner at exactly +180 / +90 / the period's max offset, a min corner at the world's minimum, a
    zero-size box and a two-box two-interval query; points = (x, y, t int64 offsets), random, on the
    boxes' edges and corners, and on cell lines."""
    rng = np.random.default_rng(seed)
    tmax = MAX_OFFSET[period] if period else 1000   # Z2: the times are drawn and dropped

    def box():
        w, h = 10 ** rng.uniform(0.3, 2.0), 10 ** rng.uniform(0.3, 1.8)
        x0, y0 = rng.uniform(-180, 180 - w), rng.uniform(-90, 90 - h)
        return (x0, y0, x0 + w, y0 + h)

    def interval():
        d = int(tmax * 10 ** rng.uniform(-1.5, -0.2))
        t0 = int(rng.integers(0, tmax - d))
        return (t0, t0 + d)

    qs = [([box()], [interval()]) for _ in range(6)]
    qs.append(([(100.0, 20.0, 180.0, 90.0)], [(tmax - tmax // 3, tmax)]))        # max corner on the world's maximum
    qs.append(([(-180.0, -90.0, -120.0, -30.0)], [(0, tmax // 4)]))              # min corner on the world's minimum
    px, py, pt = rng.uniform(-170, 170), rng.uniform(-80, 80), int(rng.integers(1, tmax))
    qs.append(([(px, py, px, py)], [(pt, pt)]))                                   # zero size
    qs.append(([box(), box()], [interval(), interval()]))
    qs.append(([(-180.0, -90.0, 180.0, 90.0)], [(tmax // 2, tmax // 2 + max(1, tmax // 50))]))   # the world, a slab of time
    # the world less a margin of one cell (from the middle of cell 1 to the middle of the last but one)
    a, b = 1.5 / (1 << precision), 1 - 1.5 / (1 << precision)
    qs.append(([(-180 + 360 * a, -90 + 180 * a, -180 + 360 * b, -90 + 180 * b)], [(int(tmax * a), int(tmax * b))]))
    n = Z_NPTS
    x = rng.uniform(-180, 180, n); y = rng.uniform(-90, 90, n)
    t = rng.integers(0, tmax + 1, n).astype(np.int64)
    # on cell lines
    x[:400] = _cell_lines(-180.0, 180.0, precision, rng, 400)
    y[200:600] = _cell_lines(-90.0, 90.0, precision, rng, 400)
    t[400:800] = np.floor(_cell_lines(0.0, float(tmax), precision, rng, 400)).astype(np.int64)
    # on the boxes' edges and corners, at the intervals' ends
    k = 800
    for boxes, ivs in qs:
        for (x0, y0, x1, y1) in boxes:
            for (t0, t1) in ivs:
                for ex, ey, et in [(x0, y0, t0), (x1, y1, t1), (x0, y1, t1), (x1, y0, t0),
                                   (x0, rng.uniform(y0, y1), int(rng.integers(t0, t1 + 1))),
                                   (rng.uniform(x0, x1), y1, int(rng.integers(t0, t1 + 1))),
                                   (rng.uniform(x0, x1), rng.uniform(y0, y1), t0),
                                   (rng.uniform(x0, x1), rng.uniform(y0, y1), t1)]:
                    x[k], y[k], t[k] = ex, ey, et
                    k += 1
                # inside, so that small boxes are hit too
                for _ in range(12):
                    x[k], y[k], t[k] = rng.uniform(x0, x1), rng.uniform(y0, y1), int(rng.integers(t0, t1 + 1))
                    k += 1
    assert k <= n
    if period is None:
        qs = [(b, None) for b, _ in qs]
        t = None
    return qs, (x, y, t)


def normalize(lo, hi, precision, v):
    """BitNormalizedDimension.normalize (NormalizedDimension.scala:56-72): the maximum maps to the last
    cell, everything else to floor((v - lo) * 2^precision / (hi - lo))."""
    v = np.asarray(v, np.float64)
    bins = 1 << precision
    cell = np.floor((v - lo) * (bins / (hi - lo))).astype(np.int64)
    return np.where(v >= hi, bins - 1, cell)


def z_user_hit_sound(period, precision, query, points, codes):
    """(hit, sound) of one query over the indexed points: hit = the point lies in a box (closed) and, for
    Z3, its time in an interval (closed); sound = the point's cell, read back from its code, lies inside
    the cells of some box x interval (what `contained` can promise for a Z curve)."""
    boxes, ivs = query
    x, y, t = points
    D = 2 if period is None else 3
    dims = RD.deinterleave(codes, D)
    hit_b = np.zeros(len(x), bool)
    for (x0, y0, x1, y1) in boxes:
        hit_b |= (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    hit = hit_b
    if D == 3:
        hit_t = np.zeros(len(x), bool)
        for (t0, t1) in ivs:
            hit_t |= (t >= t0) & (t <= t1)
        hit = hit_b & hit_t
    sound = np.zeros(len(x), bool)
    tmax = float(MAX_OFFSET[period]) if period else 1.0
    for (x0, y0, x1, y1) in boxes:
        cx = (normalize(-180.0, 180.0, precision, x0), normalize(-180.0, 180.0, precision, x1))
        cy = (normalize(-90.0, 90.0, precision, y0), normalize(-90.0, 90.0, precision, y1))
        ok = (dims[0] >= cx[0]) & (dims[0] <= cx[1]) & (dims[1] >= cy[0]) & (dims[1] <= cy[1])
        if D == 2:
            sound |= ok
            continue
        for (t0, t1) in ivs:
            ct = (normalize(0.0, tmax, precision, float(t0)), normalize(0.0, tmax, precision, float(t1)))
            sound |= ok & (dims[2] >= ct[0]) & (dims[2] <= ct[1])
    return hit, sound


# ---------------------------------------------------------------- XZ, element level
XZ2_ELEMENT_G = [1, 2, 3, 5, 6]
XZ3_ELEMENT_G = [1, 2, 3, 4]
XZ_ELEMENT_BUDGETS = [None, 1, 3, 20, 200]
XZ_NQ = 20


def xz_bounds(D, period="week"):
    lo = [-180.0, -90.0, 0.0][:D]
    hi = [180.0, 90.0, float(MAX_OFFSET[period])][:D]
    return np.array(lo), np.array(hi)


def xz_normalize(windows, D, period="week"):
    """Windows [n, 2 * D] (mins then maxs, user space) normalized as the curves do: subtract the minimum,
    divide by the span (normalize, XZ2SFC.scala:318-350, XZ3SFC.scala:338-380)."""
    lo, hi = xz_bounds(D, period)
    w = np.asarray(windows, np.float64).reshape(-1, 2 * D)
    out = np.empty_like(w)
    for d in range(D):
        out[:, d] = (w[:, d] - lo[d]) / (hi[d] - lo[d])
        out[:, D + d] = (w[:, D + d] - lo[d]) / (hi[d] - lo[d])
    return out


def xz_element_queries(D, period, seed):
    """XZ_NQ queries of 1-3 windows, one of 17 and one of 256: random doubles (no edge on a 2^-g line),
    from tiny to most of the world.  Every third query has a window that holds the enlarged level-2 cell
    [0.25, 0.75]^D, the shallowest that a window with edges inside (0, 1) can contain."""
    rng = np.random.default_rng(seed)
    lo, hi = xz_bounds(D, period)

    def window(big=False):
        if big:
            a = rng.uniform(0.05, 0.24, D); b = rng.uniform(0.76, 0.95, D)
        else:
            size = 10 ** rng.uniform(-3, -0.3, D)
            a = rng.uniform(0, 1 - size); b = a + size
        return tuple(lo + a * (hi - lo)) + tuple(lo + b * (hi - lo))

    qs = [[window(big=(k % 3 == 0 and j == 0)) for j in range(1 + k % 3)] for k in range(XZ_NQ)]
    qs.append([window() for _ in range(17)])
    qs.append([window() for _ in range(256)])
    return qs


# ---------------------------------------------------------------- XZ, end to end
XZ2_END_G = [1, 3, 12, 20, 29]
XZ3_END_G = [1, 4, 12, 19]
XZ3_END_PERIODS = ["week", "day"]
XZ_NENV = 4000
XZ_END_NQ = 40


def xz_end_budgets(g):
    return [None if g <= 6 else 2000, 1]


def _snap(v, lo, hi, g):
    """v moved to the 2^-(g+1) lattice of [lo, hi] (exact in doubles for these spans)."""
    n = float(1 << (g + 1))
    return lo + (hi - lo) * (np.round((v - lo) / (hi - lo) * n) / n)


def xz_end_case(D, g, period, seed):
    """(envelopes [XZ_NENV, 2 * D], queries): envelopes from zero size to the whole world, the second half
    snapped to the 2^-(g+1) lattice (exact ties with element edges and with the snapped windows);
    queries of 1-2 windows, every other one snapped, among them the whole world and a point window."""
    rng = np.random.default_rng(seed)
    lo, hi = xz_bounds(D, period)
    span = hi - lo

    def boxes(n, smin, smax):
        size = 10 ** rng.uniform(smin, smax, (n, D))
        a = rng.uniform(0, 1, (n, D)) * (1 - size)
        return np.concatenate([lo + a * span, lo + (a + size) * span], 1)

    env = boxes(XZ_NENV, -6, -0.5)
    env[::50, D:] = env[::50, :D]                       # zero size
    env[7::400, :D] = lo; env[7::400, D:] = hi          # the whole world
    half = XZ_NENV // 2
    for d in range(D):
        env[half:, d] = _snap(env[half:, d], lo[d], hi[d], g)
        env[half:, D + d] = np.maximum(env[half:, d], _snap(env[half:, D + d], lo[d], hi[d], g))
    qs = []
    for k in range(XZ_END_NQ):
        w = boxes(1 + k % 2, -2.5, -0.2)
        if k % 4 == 0:   # holds the enlarged cell [0.25, 0.75]^D
            w[0, :D] = lo + rng.uniform(0.05, 0.24, D) * span
            w[0, D:] = lo + rng.uniform(0.76, 0.95, D) * span
        if k % 2:
            for d in range(D):
                w[:, d] = _snap(w[:, d], lo[d], hi[d], g)
                w[:, D + d] = np.maximum(w[:, d], _snap(w[:, D + d], lo[d], hi[d], g))
        qs.append([tuple(r) for r in w])
    qs.append([tuple(lo) + tuple(hi)])
    p = lo + rng.uniform(0.1, 0.9, D) * span
    qs.append([tuple(p) + tuple(p)])
    return env, qs


def xz_end_hit(env, query, D):
    """Mask over envelopes: intersects some window of the query (closed)."""
    hit = np.zeros(len(env), bool)
    for w in query:
        ok = np.ones(len(env), bool)
        for d in range(D):
            ok &= ~((w[d] > env[:, D + d]) | (w[D + d] < env[:, d]))
        hit |= ok
    return hit


# ---------------------------------------------------------------- oracle parity inputs
def parity_queries(n, seed, period="week"):
    """The boxes and offsets of test_gpu_scan_join_ranges.ranges_queries, t scaled to the period."""
    rng = np.random.default_rng(seed)
    tmax = MAX_OFFSET[period]
    qs = []
    for _ in range(n):
        w = 10 ** rng.uniform(-2, 1.3); h = 10 ** rng.uniform(-2, 1.3)
        cx = rng.uniform(-180 + w, 180 - w); cy = rng.uniform(-90 + h, 90 - h)
        t0 = int(rng.integers(0, 604800)); t1 = int(min(604800, t0 + 10 ** rng.uniform(1, 5.8)))
        qs.append(((cx - w, cy - h, cx + w, cy + h), (t0 * tmax // 604800, t1 * tmax // 604800)))
    return qs


def xz_parity_queries(D, period, seed, n=60):
    """n one-window queries from parity_queries, plus the whole world and a point window."""
    lo, hi = xz_bounds(D, period)
    qs = []
    for b, t in parity_queries(n, seed, period):
        qs.append([b if D == 2 else (b[0], b[1], float(t[0]), b[2], b[3], float(t[1]))])
    qs.append([tuple(lo) + tuple(hi)])
    p = [11.0, 11.0, float(MAX_OFFSET[period] // 3)][:D]
    qs.append([tuple(p) + tuple(p)])
    return qs


BIG_BOX = (-10.0, 35.0, 30.0, 60.0)


def z2_corners(oracle, box):
    """The ZRange of a box under Z2SFC(31) (Z2SFC.scala:50): (index(xmin, ymin), index(xmax, ymax))."""
    (s0, lo), (s1, hi) = oracle.z2_index(box[0], box[1]), oracle.z2_index(box[2], box[3])
    assert s0 == 0 and s1 == 0
    return (lo, hi)


BIG_T = (0, 400000)
TINY = [((b[0], b[1], b[0] + 0.001, b[1] + 0.001), (t[0], t[0] + 60)) for b, t in parity_queries(2, 83)]


# ---------------------------------------------------------------- the test bodies
# Each takes the implementation under test as callables and returns (failures, tally): failures names
# the query and the violations; tally = {"contained", "open", "hits"} feeds the no-vacuous-pass asserts,
# which the bodies make themselves so that the oracle and the kernels are held to the same ones.
def _tally(t, ranges):
    _, _, cont = RD.as_arrays(ranges)
    t["contained"] += int(cont.sum())
    t["open"] += int((~cont).sum())


def run_z_raw(zranges, D, bits, with_prefix, setting):
    """zranges(D, queries, max_ranges, max_recurse) -> one list per query.  Z1-Z4 on every query, Z5 where
    the walk is exact: no budget, and maxRecurse >= bits (a node of depth k is classified at level k, and
    a node of depth `bits` is one z, contained or disjoint; ZN.scala:195-205).
    No vacuous pass: the first query's single bound is one whole top-level cell of the universe, which
    is `contained` at any budget (it is its own common prefix, ZN.scala:183), and unless the walk is
    exact some range of the case is not `contained`."""
    mr, rec = setting
    prefix = z_prefix(D, bits, with_prefix)
    qs = z_raw_queries(D, bits, prefix, seed=97 * D + with_prefix)
    top = (1 << bits) - 1
    corner = [np.int64(top // 2 + 1)] * D, [np.int64(top)] * D
    qs[0] = [(prefix | int(RD.interleave(corner[0])), prefix | int(RD.interleave(corner[1])))]
    lists = zranges(D, qs, mr, rec)
    exact = mr is None and rec >= bits
    uni = RD.z_universe(D, bits, prefix)
    fails, t = [], {"contained": 0, "open": 0, "hits": 0}
    for k, (q, r) in enumerate(zip(qs, lists)):
        v = RD.check_z_list(r, q, D, bits, prefix, exact, universe=uni)
        if v:
            fails.append((k, v))
        _tally(t, r)
    assert len(lists) == len(qs)
    assert RD.as_arrays(lists[0])[2].tolist() == [True], "the whole-cell query is one contained range"
    assert exact or t["open"] > 0, "no range that is not contained"
    return fails, t


def run_z_user(ranges, index, period, precision, budget):
    """ranges(period, precision, queries, max_ranges) and index(period, precision, x, y, t) -> codes; period
    None = Z2.  check_cover per query with hit = point in box and time in interval (closed) and sound =
    the point's cell inside the bounds' cells.
    No vacuous pass: at least 100 hits over the case; without a budget Z3SFC recurses to the last level
    (Z3SFC.scala:72) and Z2SFC's 7 levels cover a precision of 4, so every range is `contained`; with a
    budget of 20 or 1 some range is not `contained`, because the query that is the world less a margin of
    one cell cannot be resolved: all 2^D top cells overlap it, the first of them has one contained and
    2^D - 1 overlapping children (Z2: 4 + 12 after level 2, then 4 children per border cell), and the
    count of ranges and queued cells passes 20 while cells are still queued (ZN.scala:214), which are
    then bottomed out as overlapping (ZN.scala:173-180)."""
    qs, pts = z_user_case(period, precision, seed=1000 + 10 * precision + (PERIODS.index(period) if period else 7))
    codes = index(period, precision, *pts)
    lists = ranges(period, precision, qs, budget)
    fails, t = [], {"contained": 0, "open": 0, "hits": 0}
    for k, (q, r) in enumerate(zip(qs, lists)):
        hit, sound = z_user_hit_sound(period, precision, q, pts, codes)
        assert not (hit & ~sound).any()   # the definition's own consistency
        v = RD.check_cover(r, codes, hit, sound)
        if v:
            fails.append((k, v))
        t["hits"] += int(hit.sum())
        _tally(t, r)
    assert t["hits"] >= 100, t
    if budget is None:
        assert t["contained"] > 0, t
        if period is not None or precision <= 7:
            assert t["open"] == 0, t
    else:
        assert t["open"] > 0, t
    return fails, t


_ELEMENTS = {}


def elements(D, g):
    if (D, g) not in _ELEMENTS:
        _ELEMENTS[(D, g)] = RD.xz_elements(D, g)
    return _ELEMENTS[(D, g)]


def run_xz_elements(ranges, D, g, period, budget):
    """ranges(D, g, period, queries, max_ranges) -> lists.  X1-X3 on every query.
    No vacuous pass: the windows meet at least 100 elements, and some range is not `contained`.  A
    `contained` range is not asked for, because a merged XZ list cannot hold one (see ranges_definition.py:
    "contained" after the merge), although every third query has a window that contains an element."""
    qs = xz_element_queries(D, period, seed=300 + 10 * g + D)
    lists = ranges(D, g, period, qs, budget)
    el = elements(D, g)
    fails, t = [], {"contained": 0, "open": 0, "hits": 0}
    for k, (q, r) in enumerate(zip(qs, lists)):
        wn = xz_normalize(q, D, period)
        v = RD.check_xz_list(r, wn, D, g, elements=el)
        if v:
            fails.append((k, v))
        t["hits"] += int(RD.xz_meets(el[1], el[2], wn, D).sum())
        _tally(t, r)
    assert len(lists) == len(qs)
    assert t["hits"] >= 100 or g == 1, t
    assert t["open"] > 0, t
    return fails, t


def run_xz_end(ranges, index, D, g, period, budget):
    """ranges as in run_xz_elements; index(D, g, period, envelopes) -> codes.  check_cover per query with
    hit = the envelope intersects a window (closed).
    No vacuous pass: at least 100 hits, and a range that is not `contained`.  A `contained` range is not
    asked for (ranges_definition.py: "contained" after the merge), although the whole-world window
    contains the first level-1 element."""
    env, qs = xz_end_case(D, g, period, seed=500 + 10 * g + D)
    codes = index(D, g, period, env)
    lists = ranges(D, g, period, qs, budget)
    fails, t = [], {"contained": 0, "open": 0, "hits": 0}
    for k, (q, r) in enumerate(zip(qs, lists)):
        hit = xz_end_hit(env, q, D)
        v = RD.check_cover(r, codes, hit)
        if v:
            fails.append((k, v))
        t["hits"] += int(hit.sum())
        _tally(t, r)
    assert len(lists) == len(qs)
    assert t["hits"] >= 100, t
    assert t["open"] > 0, t
    return fails, t
