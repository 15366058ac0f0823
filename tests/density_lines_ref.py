"""Host references of the density scan's line rendering, and the inputs its tests share.

ScalarLineGrid is the reference's Scala read line by line (RenderingGrid.render(LineString),
geomesa-utils/.../geotools/RenderingGrid.scala:72-142; render(MultiLineString), RenderingGrid.scala:150-157;
GridSnap.bresenhamLine, geomesa-utils/.../geotools/GridSnap.scala:94-126) on top of density_ref.ScalarGrid: a
dict of pixels, the running FP64 error, (iN, jN) carried from segment to segment, keys outside the grid kept,
and a trace of what happened.  The clipped segment (RenderingGrid.scala:94-105) is the definition of
include/geomesa_hip.h, in FP64 (clip_fp) and in exact rationals (clip_exact).

line_additions / render_lines_numpy are the second form, written independently: all vertices snapped at once,
every segment walked in step (one numpy operation per Bresenham step over all segments), each in-grid
segment's last pixel recorded and compared with the start pixel of the next in-grid segment of its part.
test_density_lines_reference.py holds the two equal on every input class of the GPU tests.

Geometry rows: one entry per slot -- None (null), a list of (x, y) (LineString), or a list of such lists
(MultiLineString).
"""
import math
import operator
from fractions import Fraction

import numpy as np

import density_ref as R


def part_unrenderable(pts):
    return any(R.unrenderable(x, y) for (x, y) in pts)


def rational_line(x0, y0, x1, y1):
    """bresenhamLine with the error kept as an exact rational: what the FP64 walk is compared with."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    if dx == 0 and dy == 0:
        return [(x0, y0)]
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    major, minor = max(dx, dy), min(dx, dy)
    xmajor = dx > dy
    out, err, x, y = [], Fraction(0), x0, y0
    for _ in range(major):
        out.append((x, y))
        err += Fraction(minor, major)
        step = err >= Fraction(1, 2)
        if step:
            err -= 1
        x += sx if (xmajor or step) else 0
        y += sy if (not xmajor or step) else 0
    return out


def _fl(exact, op, a, b):
    """One FP64 operation; exact[0] turns False when its result is not the exact one."""
    r = R.div(a, b) if op is operator.truediv else op(a, b)
    if not (math.isfinite(r) and Fraction(r) == op(Fraction(a), Fraction(b))):
        exact[0] = False
    return r


def clip_fp(a, b, env, exact=None):
    """The clipped segment a -> b of include/geomesa_hip.h in unfused FP64: None (empty) or (a', b').
    exact: a one-entry list that turns False when an operation rounds."""
    xmin, ymin, xmax, ymax = env
    ex = exact if exact is not None else [True]
    (ax, ay), (bx, by) = a, b
    if max(ax, bx) < xmin or min(ax, bx) > xmax or max(ay, by) < ymin or min(ay, by) > ymax:
        return None
    add, sub, mul, div = operator.add, operator.sub, operator.mul, operator.truediv
    ends = []
    for (px, py) in (a, b):
        if xmin <= px <= xmax and ymin <= py <= ymax:
            ends.append((px, py))
            continue
        got = None
        if px < xmin or px > xmax:
            X = xmin if px < xmin else xmax
            y = _fl(ex, add, ay, _fl(ex, mul, _fl(ex, sub, X, ax), _fl(ex, div, _fl(ex, sub, by, ay), _fl(ex, sub, bx, ax))))
            if ymin <= y <= ymax:
                got = (X, y)
        if got is None and (py < ymin or py > ymax):
            Y = ymin if py < ymin else ymax
            x = _fl(ex, add, ax, _fl(ex, mul, _fl(ex, sub, Y, ay), _fl(ex, div, _fl(ex, sub, bx, ax), _fl(ex, sub, by, ay))))
            if xmin <= x <= xmax:
                got = (x, Y)
        if got is None:
            return None
        ends.append(got)
    return ends[0], ends[1]


def clip_exact(a, b, env):
    """The same definition over exact rationals: None or a pair of (Fraction, Fraction)."""
    xmin, ymin, xmax, ymax = (Fraction(v) for v in env)
    (ax, ay), (bx, by) = (tuple(Fraction(v) for v in p) for p in (a, b))
    if max(ax, bx) < xmin or min(ax, bx) > xmax or max(ay, by) < ymin or min(ay, by) > ymax:
        return None
    ends = []
    for (px, py) in ((ax, ay), (bx, by)):
        if xmin <= px <= xmax and ymin <= py <= ymax:
            ends.append((px, py))
            continue
        got = None
        if px < xmin or px > xmax:
            X = xmin if px < xmin else xmax
            y = ay + (X - ax) * ((by - ay) / (bx - ax))
            if ymin <= y <= ymax:
                got = (X, y)
        if got is None and (py < ymin or py > ymax):
            Y = ymin if py < ymin else ymax
            x = ax + (Y - ay) * ((bx - ax) / (by - ay))
            if xmin <= x <= xmax:
                got = (x, Y)
        if got is None:
            return None
        ends.append(got)
    return ends[0], ends[1]


class ScalarLineGrid(R.ScalarGrid):
    """RenderingGrid for lines, as the Scala reads."""

    def __init__(self, env, x_size, y_size):
        super().__init__(env, x_size, y_size)
        self.env = tuple(float(v) for v in env)
        self.clips = []            # (a, b, no operation rounded) of every clipped segment

    def put(self, i, j, weight):
        if i < 0 or i >= self.x_size:
            self.trace["col_out"] += 1
            self.trace["neg_col"] += i == -1
        self.pixels[(i, j)] = self.pixels.get((i, j), 0.0) + weight
        self.trace["added"] += 1

    def bresenham_line(self, x0, y0, x1, y1):                     # GridSnap.scala:94-126
        delta_x, delta_y = abs(x1 - x0), abs(y1 - y0)
        if delta_x == 0 and delta_y == 0:
            yield (x0, y0)
            return
        step_x = 1 if x0 < x1 else -1
        step_y = 1 if y0 < y1 else -1
        x, y, error = x0, y0, 0.0
        if delta_x > delta_y:
            delta_error = float(delta_y) / delta_x
            for _ in range(delta_x):                              # take(deltaX)
                yield (x, y)
                error += delta_error
                if error >= 0.5:
                    error -= 1.0
                    x, y = x + step_x, y + step_y
                else:
                    x = x + step_x
        else:
            delta_error = float(delta_x) / delta_y
            for _ in range(delta_y):
                yield (x, y)
                error += delta_error
                if error >= 0.5:
                    error -= 1.0
                    x, y = x + step_x, y + step_y
                else:
                    y = y + step_y

    def render_point(self, x, y, weight):                         # RenderingGrid.scala:43-49
        j = self.j(y)
        if j != -1:
            for i in self.translate(x):
                self.put(i, j, weight)

    def render_line(self, pts, weight, clipped_piece=False):      # RenderingGrid.scala:72-142
        if len(pts) == 0:
            return
        i_n = j_n = -1
        written = set()
        p1 = pts[0]
        i1, j1 = self.translate(p1[0]), self.j(p1[1])
        after_clip = False
        for n in range(1, len(pts)):
            p0, i0, j0 = p1, i1, j1
            p1 = pts[n]
            i1, j1 = self.translate(p1[0]), self.j(p1[1])
            if len(i0) == 0 or j0 == -1 or len(i1) == 0 or j1 == -1:
                assert not clipped_piece, "a clipped piece lies in the envelope"
                exact = [True]
                piece = clip_fp(p0, p1, self.env, exact)
                self.clips.append((p0, p1, exact[0]))
                if piece is None:
                    self.trace["clip_empty"] += 1
                elif piece[0] == piece[1]:
                    self.trace["clip_point"] += 1
                    self.render_point(piece[0][0], piece[0][1], weight)
                else:
                    self.trace["clip_line"] += 1
                    self.render_line([piece[0], piece[1]], weight, clipped_piece=True)
                after_clip = True
                continue
            line = list(self.bresenham_line(i0[0], j0, i1[0], j1))
            if len(line) == 1:
                self.trace["single_pixel"] += 1
            else:
                dx, dy = i1[0] - i0[0], j1 - j0
                if dx != 0 and dy != 0:
                    self.trace["octant%+d%+d%s" % (np.sign(dx), np.sign(dy), "x" if abs(dx) > abs(dy) else "y")] += 1
                if line != rational_line(i0[0], j0, i1[0], j1):
                    self.trace["fp_walk_differs"] += 1
            for k, (i, j) in enumerate(line):
                if k == 0 and i == i_n and j == j_n:
                    self.trace["first_suppressed"] += 1
                    if after_clip:
                        self.trace["reenter_on_last_pixel"] += 1
                    continue
                self.put(i, j, weight)
                written.add((i, j))
                for c in i0[1:]:
                    self.put(i - i0[0] + c, j, weight)
            i_n, j_n = line[-1]
            after_clip = False
        if not clipped_piece and len(pts) > 1 and len(i1) and j1 != -1 and (i1[0], j1) not in written:
            self.trace["final_pixel_unwritten"] += 1

    def render_geom(self, geom, weight):
        """One slot: None, a LineString's vertices or a MultiLineString's parts."""
        if geom is None:
            self.trace["null"] += 1
            self.trace["skipped"] += 1
            return
        parts = geom if (len(geom) and isinstance(geom[0], list)) else [geom]
        if geom == []:
            parts = [[]]
        for pts in parts:
            pts = [(float(x), float(y)) for (x, y) in pts]
            self.trace["vertices%d" % min(len(pts), 2)] += 1
            if part_unrenderable(pts):
                self.trace["skipped"] += 1
                self.trace["skipped_part"] += 1
                continue
            self.render_line(pts, weight)


def render_scalar(env, width, height, rows, weight=None, mask=None, ids=None):
    """The reference over the selected slots.  Returns (ScalarLineGrid, tally int64[3])."""
    g = ScalarLineGrid(env, width, height)
    sel, bad = R.select(len(rows), mask, ids)
    for r in sel:
        g.render_geom(rows[r], 1.0 if weight is None else float(weight[r]))
    return g, np.array([g.trace["skipped"], g.trace["col_out"], bad], np.int64)


def scalar_dense(g):
    out = np.zeros((g.y_size, g.x_size))
    for (i, j), w in g.pixels.items():
        if 0 <= i < g.x_size:
            out[j, i] = w
    return out


# ------------------------------------------------------------------ the second form

def flatten(rows, sel):
    """(x, y, part offsets, slot of each part, null slots) of the selected slots, in selection order."""
    xs, ys, off, slot, nulls = [], [], [0], [], 0
    for r in sel:
        geom = rows[r]
        if geom is None:
            nulls += 1
            continue
        parts = geom if (len(geom) and isinstance(geom[0], list)) else [geom]
        for pts in parts:
            for (x, y) in pts:
                xs.append(x)
                ys.append(y)
            off.append(len(xs))
            slot.append(r)
    return (np.array(xs, np.float64), np.array(ys, np.float64), np.array(off, np.int64), np.array(slot, np.int64),
            nulls)


class _Snap:
    """translate / widen and GridSnap over arrays: ok (translate not empty and j != -1), head, j, xup."""

    def __init__(self, env, width, height):
        self.xmin, self.ymin, self.xmax, self.ymax = (np.float64(v) for v in env)
        self.width, self.height = width, height
        self.dx = (self.xmax - self.xmin) / np.float64(width)
        self.dy = (self.ymax - self.ymin) / np.float64(height)
        self.wide = bool(self.xmax - self.xmin > 360.0)
        self.copies = int(math.floor((self.xmax - self.xmin) / 360.0)) + 2 if self.wide else 1

    def col(self, x):
        return R._np_index(x, self.xmin, self.xmax, self.dx, self.width)

    def __call__(self, x, y):
        c360 = np.float64(360.0)
        with np.errstate(all="ignore"):
            j = R._np_index(y, self.ymin, self.ymax, self.dy, self.height)
            below, above = x < self.xmin, x > self.xmax
            xt = np.where(below, x + c360 * np.ceil((self.xmin - x) / c360),
                          np.where(above, x - c360 * np.ceil((x - self.xmax) / c360), x))
            some = ~((below & (xt > self.xmax)) | (above & (xt < self.xmin)))
            if self.wide:
                xt = xt - c360 * np.floor((xt - self.xmin) / c360)
                some &= xt <= self.xmax
            head = self.col(xt)
        return some & (j != -1), head, j, xt


def _walk(sn, h0, j0, h1, j1, xup0, w, suppress):
    """All segments walked in step.  Returns (i, j, w) of every addition, copies included, columns outside
    the grid kept, and each segment's last Bresenham pixel."""
    n = len(h0)
    dx, dy = np.abs(h1 - h0), np.abs(j1 - j0)
    sx, sy = np.where(h0 < h1, 1, -1), np.where(j0 < j1, 1, -1)
    xmajor = dx > dy
    major = np.where(xmajor, dx, dy)
    with np.errstate(all="ignore"):
        de = np.where(xmajor, dy.astype(np.float64) / dx, dx.astype(np.float64) / dy)
    x, y, err = h0.copy(), j0.copy(), np.zeros(n)
    li, lj = h0.copy(), j0.copy()
    ev_i, ev_j, ev_s = [], [], []
    steps = int(major.max()) if n else 0
    single = major == 0
    for k in range(max(steps, 1)):
        live = (k < major) | (single & (k == 0))
        if not live.any():
            break
        wr = live & ~(suppress & (k == 0))
        ev_i.append(x[wr]); ev_j.append(y[wr]); ev_s.append(np.flatnonzero(wr))
        li = np.where(live, x, li)
        lj = np.where(live, y, lj)
        err = np.where(live, err + de, err)
        step = live & (err >= 0.5)
        err = np.where(step, err - 1.0, err)
        x = np.where(live & (xmajor | step), x + sx, x)
        y = np.where(live & (~xmajor | step), y + sy, y)
    if not ev_i:
        e = np.zeros(0, np.int64)
        return e, e, np.zeros(0), li, lj
    pi, pj, ps = np.concatenate(ev_i), np.concatenate(ev_j), np.concatenate(ev_s)
    out_i, out_j, out_w = [pi], [pj], [w[ps]]
    xu = xup0.copy()
    for _ in range(1, sn.copies):
        xu = xu + np.float64(360.0)
        have = xu <= sn.xmax
        off = sn.col(xu) - h0
        keep = have[ps]
        out_i.append(pi[keep] + off[ps][keep]); out_j.append(pj[keep]); out_w.append(w[ps][keep])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_w), li, lj


def _clip_np(ax, ay, bx, by, sn):
    """clip over arrays: (kept, a'x, a'y, b'x, b'y)."""
    with np.errstate(all="ignore"):
        kept = ~((np.maximum(ax, bx) < sn.xmin) | (np.minimum(ax, bx) > sn.xmax) |
                 (np.maximum(ay, by) < sn.ymin) | (np.minimum(ay, by) > sn.ymax))
        sv = (by - ay) / (bx - ax)
        sh = (bx - ax) / (by - ay)
        res = []
        for (px, py) in ((ax, ay), (bx, by)):
            inside = (px >= sn.xmin) & (px <= sn.xmax) & (py >= sn.ymin) & (py <= sn.ymax)
            X = np.where(px < sn.xmin, sn.xmin, sn.xmax)
            vy = ay + (X - ax) * sv
            vok = ((px < sn.xmin) | (px > sn.xmax)) & (vy >= sn.ymin) & (vy <= sn.ymax)
            Y = np.where(py < sn.ymin, sn.ymin, sn.ymax)
            hx = ax + (Y - ay) * sh
            hok = ((py < sn.ymin) | (py > sn.ymax)) & (hx >= sn.xmin) & (hx <= sn.xmax)
            kept &= inside | vok | hok
            res.append((np.where(inside, px, np.where(vok, X, hx)), np.where(inside, py, np.where(vok, vy, Y))))
    return kept, res[0][0], res[0][1], res[1][0], res[1][1]


def line_additions(env, width, height, rows, weight=None, mask=None, ids=None):
    """Every pixel addition inside the grid of rendering the selected slots: (flat pixel j * width + i,
    weight) arrays, and the tally int64[3]."""
    sel, bad = R.select(len(rows), mask, ids)
    x, y, off, slot, nulls = flatten(rows, sel)
    sn = _Snap(env, width, height)
    nparts = len(off) - 1
    wpart = np.ones(nparts) if weight is None else np.asarray(weight, np.float64)[slot]
    unr = ~(np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= R.TWO31))
    cum = np.concatenate([[0], np.cumsum(unr)])
    bad_part = (cum[off[1:]] - cum[off[:-1]]) > 0
    tally = np.array([nulls + int(bad_part.sum()), 0, bad], np.int64)
    part_of = np.repeat(np.arange(nparts), np.diff(off))
    t = np.arange(len(x))
    seg = np.flatnonzero((t != off[:-1][part_of]) & ~bad_part[part_of]) if len(x) else np.zeros(0, np.int64)
    xs, ys = np.where(unr, 0.0, x), np.where(unr, 0.0, y)
    ok, head, j, xup = sn(xs, ys)
    a, b = seg - 1, seg
    ingrid = ok[a] & ok[b]
    w = wpart[part_of[seg]]
    # (iN, jN): the last pixel of the previous in-grid segment of the same part
    gi = np.flatnonzero(ingrid)
    h0, j0, h1, j1 = head[a][gi], j[a][gi], head[b][gi], j[b][gi]
    _, _, _, li, lj = _walk(sn, h0, j0, h1, j1, xup[a][gi], w[gi], np.zeros(len(gi), bool))
    prev = np.arange(len(gi)) - 1
    same_part = (prev >= 0) & (part_of[seg[gi]] == part_of[seg[gi[np.maximum(prev, 0)]]])
    suppress = same_part & (li[np.maximum(prev, 0)] == h0) & (lj[np.maximum(prev, 0)] == j0)
    ei, ej, ew, _, _ = _walk(sn, h0, j0, h1, j1, xup[a][gi], w[gi], suppress)
    # clipped segments: raw ordinates
    ci = np.flatnonzero(~ingrid)
    kept, cax, cay, cbx, cby = _clip_np(x[a][ci], y[a][ci], x[b][ci], y[b][ci], sn)
    point = kept & (cax == cbx) & (cay == cby)
    line = kept & ~point
    ppix, pw, _, (_, pdrop) = R.additions(env, width, height, cax[point], cay[point], w[ci][point])
    ok0, ch0, cj0, cxu = sn(cax[line], cay[line])
    ok1, ch1, cj1, _ = sn(cbx[line], cby[line])
    both = ok0 & ok1
    fi, fj, fw, _, _ = _walk(sn, ch0[both], cj0[both], ch1[both], cj1[both], cxu[both], w[ci][line][both],
                             np.zeros(int(both.sum()), bool))
    ai, aj, aw = np.concatenate([ei, fi]), np.concatenate([ej, fj]), np.concatenate([ew, fw])
    inside = (ai >= 0) & (ai < width)
    tally[1] = int((~inside).sum()) + pdrop
    pix = np.concatenate([aj[inside] * width + ai[inside], ppix]).astype(np.int64)
    return pix, np.concatenate([aw[inside], pw]), tally


def render_lines_numpy(env, width, height, rows, weight=None, mask=None, ids=None):
    """(grid float64 [height, width], tally int64[3]): what gm_density_lines adds into a cleared grid and
    tally.  Unweighted and dyadic weights give the same bits in any order of the additions."""
    pix, wts, tally = line_additions(env, width, height, rows, weight, mask, ids)
    grid = np.bincount(pix, weights=wts, minlength=width * height)
    return grid.reshape(height, width), tally


# ------------------------------------------------------------------ inputs

def fp_differing_slopes(limit):
    """(dX, dY), dY <= dX <= limit, at which the FP64 error walk and the rational one differ."""
    g = ScalarLineGrid((0.0, 0.0, 1.0, 1.0), 1, 1)
    return [(a, b) for a in range(1, limit + 1) for b in range(0, a + 1)
            if list(g.bresenham_line(0, 0, a, b)) != rational_line(0, 0, a, b)]


def line_set(env, width, height, seed, tracks=600):
    """LineString rows (None: a null slot) holding every input class of the line tests; the CPU test
    counts the classes from ScalarLineGrid's trace."""
    rng = np.random.default_rng(seed)
    xmin, ymin, xmax, ymax = (float(v) for v in env)
    dx, dy = (xmax - xmin) / width, (ymax - ymin) / height
    rows = []

    def centre(i, j):
        return (xmin + (i + 0.5) * dx, ymin + (j + 0.5) * dy)

    def inside():
        return (rng.uniform(xmin, xmax), rng.uniform(ymin, ymax))

    def outside():
        side = rng.integers(4)
        ox, oy = rng.uniform(0.01, 0.4) * (xmax - xmin), rng.uniform(0.01, 0.4) * (ymax - ymin)
        x, y = inside()
        return [(xmin - ox, y), (xmax + ox, y), (x, ymin - oy), (x, ymax + oy)][side]

    # short tracks: steps of 0 to 3 pixels, a share wandering out of the envelope and back
    for _ in range(tracks):
        x, y = inside()
        pts = [(x, y)]
        for _ in range(int(rng.integers(2, 30))):
            x += rng.uniform(-3, 3) * dx * (rng.random() < 0.8)
            y += rng.uniform(-3, 3) * dy * (rng.random() < 0.8)
            pts.append((x, y))
        rows.append(pts)
    # long segments in every octant, between random pixels
    for _ in range(tracks // 2):
        rows.append([inside() for _ in range(int(rng.integers(2, 5)))])
    # the slopes at which the FP64 error walk leaves the rational one, in all sign combinations
    slopes = [(a, b) for (a, b) in fp_differing_slopes(32) if a < min(width, height)]
    for (a, b) in slopes:
        for (sa, sb, swap) in ((1, 1, 0), (-1, 1, 0), (1, -1, 1), (-1, -1, 1)):
            da, db = ((a, b), (b, a))[swap]
            i0 = int(rng.integers(max(0, -sa * da), min(width, width - sa * da)))
            j0 = int(rng.integers(max(0, -sb * db), min(height, height - sb * db)))
            rows.append([centre(i0, j0), centre(i0 + sa * da, j0 + sb * db), centre(i0, j0)])
    # leave the envelope and come back to the pixel of (iN, jN): after a one-pixel segment and after a
    # walk that ends beside its end vertex
    for k in range(60):
        i, j = int(rng.integers(1, max(width - 3, 2))), int(rng.integers(0, height))
        if width < 4:
            break
        if k % 2:
            rows.append([centre(i, j), centre(i, j), outside(), centre(i, j), inside()])
        else:
            rows.append([centre(i - 1, j), centre(i + 1, j), outside(), centre(i, j), inside(), outside(), outside()])
    # clip results: a line (crossing the edge), a point (from a vertex on the edge outwards), empty (outside)
    for _ in range(60):
        rows.append([inside(), outside(), inside()])
        ex = (xmin, rng.uniform(ymin, ymax)) if rng.random() < 0.5 else (rng.uniform(xmin, xmax), ymax)
        out = (ex[0] - rng.uniform(0.1, 2.0) * dx * 8, ex[1] + rng.uniform(0.1, 2.0) * dy * 8)
        rows.append([inside(), ex, out])
        rows.append([outside(), outside(), outside()])
        rows.append([(xmin - 3 * dx, ymin + 2 * dy), (xmin + 2 * dx, ymin - 3 * dy)])      # across a corner
    # whole turns on either side, vertex by vertex and track by track
    for _ in range(60):
        turn = float(rng.choice([-720.0, -360.0, 360.0, 720.0]))
        pts = [inside() for _ in range(4)]
        rows.append([(x + turn, y) for (x, y) in pts])
        rows.append([pts[0], (pts[1][0] + turn, pts[1][1]), pts[2], (pts[3][0] - turn, pts[3][1])])
    # the -1-column class: fl(xmin + 360 m) and the doubles below it (density_ref.edge_set)
    for m in (-2, -1, 1, 2):
        v = np.float64(xmin) + 360.0 * m
        for _ in range(3):
            for _ in range(12):
                rows.append([(float(v), rng.uniform(ymin, ymax)), inside()])
                rows.append([inside(), (float(v), rng.uniform(ymin, ymax))])
            v = R.ulp_down(v)
    # parts the dense grid skips, null slots, 0- and 1-vertex parts
    for bad in (np.nan, np.inf, -np.inf, 3e9, -3e9):
        for _ in range(5):
            pts = [inside() for _ in range(5)]
            pts[int(rng.integers(5))] = (bad, pts[0][1])
            rows.append(pts)
            pts = [inside() for _ in range(3)]
            if bad != 3e9 and bad != -3e9:
                pts[1] = (pts[1][0], bad)
                rows.append(pts)
    for _ in range(25):
        rows.append(None)
        rows.append([])
        rows.append([inside()])
    order = rng.permutation(len(rows))
    return [rows[k] for k in order]


def as_multi(lines, seed):
    """MultiLineString rows of 0 to 3 parts each out of line_set's rows (its nulls stay null slots)."""
    rng = np.random.default_rng(seed)
    rows, k = [], 0
    while k < len(lines):
        if lines[k] is None:
            rows.append(None)
            k += 1
            continue
        m = int(rng.integers(0, 4))
        parts = []
        while m and k < len(lines) and lines[k] is not None:
            parts.append(lines[k])
            k += 1
            m -= 1
        rows.append(parts if parts else [[]])
        if not parts and rng.random() < 0.5:
            rows[-1] = [[], []]
    return rows


def in_float32(rows):
    """The rows as a Float4 vector holds them."""
    def r(p):
        return (float(np.float32(p[0])), float(np.float32(p[1])))

    def line(pts):
        return [r(p) for p in pts]
    return [None if g is None else ([line(p) for p in g] if len(g) and isinstance(g[0], list) else line(g))
            for g in rows]


# the envelopes of the line tests: (name, (xmin, ymin, xmax, ymax), width, height)
LINE_ENVELOPES = [
    ("8x8", (0.0, 0.0, 8.0, 8.0), 8, 8),
    ("antimeridian-64", (170.0, -10.0, 190.0, 10.0), 64, 64),
    ("world-256", (-180.0, -90.0, 180.0, 90.0), 256, 256),
    ("dx-not-dyadic-500", (-1.0, 33.0, 6.0, 40.0), 500, 500),
    ("wide", (-200.0, -90.0, 600.0, 90.0), 256, 64),
    ("wide-fractional-xmin", (-170.7, -90.0, 600.1, 90.0), 64, 64),
    ("narrow-fractional-xmin", (-1.3, 33.0, 6.1, 40.0), 64, 64),
    ("wide-fractional-xmin-3x1000", (-170.7, -90.0, 600.1, 90.0), 3, 1000),   # density_ref.EDGE_ENVELOPES' grid
]


def dyadic_clip_set(seed, n=400):
    """Two-vertex lines over the envelope (0, 0, 8, 8) whose clip rounds nowhere: ordinates k / 8, run and
    rise powers of two, so the slope, its product and the sum are exact in FP64."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        ax, ay = rng.integers(-32, 97) / 8.0, rng.integers(-32, 97) / 8.0
        run = float(2.0 ** rng.integers(-2, 4)) * rng.choice([-1.0, 1.0])
        rise = float(2.0 ** rng.integers(-2, 4)) * rng.choice([-1.0, 1.0])
        rows.append([(ax, ay), (ax + run, ay + rise)])
    return rows


DYADIC_ENV = (0.0, 0.0, 8.0, 8.0)
