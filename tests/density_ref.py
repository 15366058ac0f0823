"""Host references of the density scan's point rendering, and the inputs its tests share.

render_scalar is the reference's Scala read line by line (RenderingGrid.render(Point), translate, widen:
geomesa-utils/.../geotools/RenderingGrid.scala:43-49, 299-330; GridSnap.i / j: geomesa-utils/.../geotools/
GridSnap.scala:60-80): a dict of pixels, the literal `while`, the map key (-1, j) kept.  render_numpy is the
vectorised form the GPU tests compare with: a dense grid and the three tallies of include/geomesa_hip.h.
test_density_reference.py holds the two equal on every input class below.

Both leave out the rows the C ABI declares unrenderable (non-finite x or y, |x| > 2^31: the Scala code
would put a NaN into row / column 0 and never leave widen's loop for an infinite x) and count them.
"""
import math
from collections import Counter

import numpy as np

INT_MAX, INT_MIN = 2147483647, -2147483648
TWO31 = 2147483648.0


def to_int(q):
    """Scala's Double.toInt (JLS 5.1.3): NaN -> 0, saturating."""
    if q != q:
        return 0
    if q >= INT_MAX:
        return INT_MAX
    if q <= INT_MIN:
        return INT_MIN
    return int(q)


def floor(q):
    return float(math.floor(q)) if math.isfinite(q) else q


def ceil(q):
    return float(math.ceil(q)) if math.isfinite(q) else q


def div(a, b):
    """IEEE double division (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b))


def unrenderable(x, y):
    return not (math.isfinite(x) and math.isfinite(y) and abs(x) <= TWO31)


class ScalarGrid:
    """RenderingGrid + GridSnap for points, as the Scala reads."""

    def __init__(self, env, x_size, y_size):
        self.x_min, self.y_min, self.x_max, self.y_max = (float(v) for v in env)
        self.x_size, self.y_size = x_size, y_size
        with np.errstate(all="ignore"):
            self.dx = div(self.x_max - self.x_min, x_size)      # GridSnap.scala:32-33
            self.dy = div(self.y_max - self.y_min, y_size)
        self.wide = self.x_max - self.x_min > 360.0             # RenderingGrid.scala:33
        self.pixels = {}
        self.trace = Counter()

    def i(self, x):                                             # GridSnap.scala:60-66
        if x < self.x_min or x > self.x_max:
            return -1
        with np.errstate(all="ignore"):
            i = to_int(floor(div(x - self.x_min, self.dx)))
        if i >= self.x_size:
            self.trace["clamped"] += 1
            return self.x_size - 1
        return i

    def j(self, y):                                             # GridSnap.scala:74-80
        if y < self.y_min or y > self.y_max:
            return -1
        with np.errstate(all="ignore"):
            i = to_int(floor(div(y - self.y_min, self.dy)))
        if i >= self.y_size:
            return self.y_size - 1
        return i

    def translate(self, x):                                     # RenderingGrid.scala:299-309
        if x < self.x_min:
            self.trace["below"] += 1
            xt = x + (360.0 * ceil((self.x_min - x) / 360))
            if xt > self.x_max:
                self.trace["empty"] += 1
                return []
            return self.widen(xt)
        elif x > self.x_max:
            self.trace["above"] += 1
            xt = x - (360.0 * ceil((x - self.x_max) / 360))
            if xt < self.x_min:
                self.trace["empty"] += 1
                return []
            return self.widen(xt)
        return self.widen(x)

    def widen(self, x):                                         # RenderingGrid.scala:317-330
        if self.wide:
            seq = []
            xup = x - 360.0 * floor((x - self.x_min) / 360)
            while xup <= self.x_max:
                seq.append(self.i(xup))
                xup += 360.0
            self.trace["copies%d" % len(seq)] += 1
            return seq
        return [self.i(x)]

    def render(self, x, y, weight):                             # RenderingGrid.scala:43-49
        if unrenderable(x, y):
            self.trace["skipped"] += 1
            return
        j = self.j(y)
        if j != -1:
            for i in self.translate(x):
                if i == -1:
                    self.trace["neg_col"] += 1
                self.pixels[(i, j)] = self.pixels.get((i, j), 0.0) + weight
                self.trace["added"] += 1
        else:
            self.trace["row_out"] += 1


def render_scalar(env, width, height, x, y, weight=None):
    """The reference over rows of x / y (weight None = EqualWeight's 1.0).  Returns the ScalarGrid: .pixels
    is the reference's map, (-1, j) keys included; .trace counts what happened."""
    g = ScalarGrid(env, width, height)
    for k in range(len(x)):
        g.render(float(x[k]), float(y[k]), 1.0 if weight is None else float(weight[k]))
    return g


def scalar_dense(g):
    """(grid, dropped) of a ScalarGrid: the dense [height, width] array of the pixels inside the grid, and
    how many additions went to a (-1, j) key."""
    out = np.zeros((g.y_size, g.x_size))
    for (i, j), w in g.pixels.items():
        if i >= 0:
            out[j, i] = w
    return out, g.trace["neg_col"]


def _np_index(v, lo, hi, d, size):
    with np.errstate(all="ignore"):
        q = np.floor((v - lo) / d)
        q = np.clip(np.where(np.isnan(q), 0.0, q), float(INT_MIN), float(INT_MAX)).astype(np.int64)
    return np.where((v < lo) | (v > hi), -1, np.minimum(q, size - 1))


def additions(env, width, height, x, y, weight=None):
    """Every pixel addition of rendering rows x / y, in row order per copy: (flat pixel j * width + i,
    weight, source row) arrays, and (skipped, dropped)."""
    xmin, ymin, xmax, ymax = (np.float64(v) for v in env)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    w = np.ones(len(x)) if weight is None else np.asarray(weight, np.float64)
    with np.errstate(all="ignore"):
        dx = (xmax - xmin) / np.float64(width)
        dy = (ymax - ymin) / np.float64(height)
        ok = np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= TWO31)
        skipped = int((~ok).sum())
        j = _np_index(y, ymin, ymax, dy, height)
        live = ok & (j != -1)
        below, above = x < xmin, x > xmax
        xt = np.where(below, x + np.float64(360.0) * np.ceil((xmin - x) / np.float64(360.0)),
                      np.where(above, x - np.float64(360.0) * np.ceil((x - xmax) / np.float64(360.0)), x))
        live &= ~((below & (xt > xmax)) | (above & (xt < xmin)))
        pix, wts, src = [], [], []
        dropped = 0
        rows = np.arange(len(x))
        if xmax - xmin > 360.0:
            xup = xt - np.float64(360.0) * np.floor((xt - xmin) / np.float64(360.0))
            copies = int(math.floor((xmax - xmin) / 360.0)) + 2
        else:
            xup, copies = xt, 1
        for _ in range(copies):
            if copies > 1:
                live = live & (xup <= xmax)
            i = _np_index(xup, xmin, xmax, dx, width)
            neg = live & (i == -1)
            dropped += int(neg.sum())
            sel = live & (i != -1)
            pix.append(j[sel] * width + i[sel])
            wts.append(w[sel])
            src.append(rows[sel])
            xup = xup + np.float64(360.0)
    return np.concatenate(pix), np.concatenate(wts), np.concatenate(src), (skipped, dropped)


def select(n, mask=None, ids=None):
    """(rows to render, bad id count) of a selection over n rows: a bool mask or ids in any order."""
    if ids is not None:
        ids = np.asarray(ids, np.int64)
        good = (ids >= 0) & (ids < n)
        return ids[good], int((~good).sum())
    if mask is not None:
        return np.flatnonzero(np.asarray(mask, bool)[:n]), 0
    return np.arange(n), 0


def render_numpy(env, width, height, x, y, weight=None, mask=None, ids=None):
    """(grid float64 [height, width], tally int64[3]) of rendering the selected rows of x / y: what
    gm_density_points adds into a cleared grid and tally.  The FP64 additions run in row order; for
    unweighted and dyadic weights every order gives the same bits."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    rows, bad = select(len(x), mask, ids)
    w = None if weight is None else np.asarray(weight, np.float64)[rows]
    pix, wts, _, (skipped, dropped) = additions(env, width, height, x[rows], y[rows], w)
    grid = np.zeros(width * height)
    np.add.at(grid, pix, wts)
    return grid.reshape(height, width), np.array([skipped, dropped, bad], np.int64)


def render_rows(env, width, height, rows, weight=None, mask=None, ids=None):
    """render_numpy over per-slot geometry rows (oracle.arrow_rows of a point or multipoint column: None,
    (x, y), or a list of (x, y)); a null slot counts as skipped, every point of a slot gets its weight."""
    sel, bad = select(len(rows), mask, ids)
    xs, ys, ws, nulls = [], [], [], 0
    for r in sel:
        v = rows[r]
        if v is None:
            nulls += 1
            continue
        pts = [v] if isinstance(v, tuple) else v
        for (px, py) in pts:
            xs.append(px)
            ys.append(py)
            ws.append(1.0 if weight is None else float(weight[r]))
    grid, tally = render_numpy(env, width, height, np.array(xs, np.float64), np.array(ys, np.float64),
                               None if weight is None else np.array(ws, np.float64))
    tally[0] += nulls
    tally[2] = bad
    return grid, tally


def ulp_up(v):
    return np.nextafter(v, np.inf)


def ulp_down(v):
    return np.nextafter(v, -np.inf)


def edge_set(env, width, height):
    """x / y columns of the edge classes of one envelope: the envelope's edges and one ulp outside them,
    every cell edge xmin + k dx and +-1 ulp (at most 600 of them, spread over the grid), whole turns outside
    (+-360, +-720), fl(xmin + 360 k) -- the -1-column class --, and NaN, +-inf and |x| > 2^31 rows; every
    class at least 20 times."""
    xmin, ymin, xmax, ymax = (np.float64(v) for v in env)
    dx = (xmax - xmin) / np.float64(width)
    dy = (ymax - ymin) / np.float64(height)
    ymid = ymin + (ymax - ymin) * 0.37
    xmid = xmin + (xmax - xmin) * 0.41
    xs, ys = [], []

    def put(x, y):
        xs.extend(np.atleast_1d(x).tolist())
        ys.extend(np.broadcast_to(y, np.atleast_1d(x).shape).tolist())
    ys_in = ymin + (ymax - ymin) * np.linspace(0.0, 1.0, 21)     # both corners included
    xs_in = xmin + (xmax - xmin) * np.linspace(0.02, 0.98, 21)
    for e in (xmin, xmax):
        for v in (e, ulp_down(e), ulp_up(e)):
            put(np.full(21, v), ys_in)
    for e in (ymin, ymax):
        for v in (e, ulp_down(e), ulp_up(e)):
            put(xs_in, np.full(21, v))
    kx = np.unique(np.linspace(0, width, min(width, 600) + 1).astype(np.int64))
    cx = xmin + kx * dx
    for v in (cx, ulp_down(cx), ulp_up(cx)):
        put(v, ymid)
    ky = np.unique(np.linspace(0, height, min(height, 600) + 1).astype(np.int64))
    cy = ymin + ky * dy
    for v in (cy, ulp_down(cy), ulp_up(cy)):
        put(np.full(len(v), xmid), v)
    inside = xmin + (xmax - xmin) * np.linspace(0.0, 1.0, 41)
    for turn in (-720.0, -360.0, 360.0, 720.0):
        put(inside + turn, ymid)
    for k in range(-40, 41):
        if k:
            put([xmin + 360.0 * k, xmax + 360.0 * k], ymid)
    # the -1-column class: fl(xmin + 360 m) and the doubles just below it, at every row of ys_in.  In a
    # narrow envelope xt = x - 360 m lands below xmin; in a wide one xup does when (x - xmin) / 360 still
    # rounds to m
    for m in (-2, -1, 1, 2):
        v = xmin + 360.0 * m
        for _ in range(3):
            put(np.full(21, v), ys_in)
            v = ulp_down(v)
    bad = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, ulp_up(TWO31), -ulp_up(TWO31)])
    for yv in ys_in[3:6]:
        put(bad, np.full(len(bad), yv))
    put([TWO31, -TWO31], ymid)                                   # the last renderable magnitude
    for yv in (np.nan, np.inf, -np.inf):
        put(xs_in[:7], np.full(7, yv))
    return np.array(xs, np.float64), np.array(ys, np.float64)


# the envelopes of the edge set: (name, (xmin, ymin, xmax, ymax), width, height)
EDGE_ENVELOPES = [
    ("dx-not-dyadic-500", (-1.0, 33.0, 6.0, 40.0), 500, 500),
    ("dx-not-dyadic-100", (0.0, 0.0, 10.0, 10.0), 100, 100),
    ("dx-dyadic", (-180.0, -90.0, 180.0, 90.0), 256, 256),
    ("antimeridian", (170.0, -10.0, 190.0, 10.0), 64, 64),
    ("wide", (-200.0, -90.0, 600.0, 90.0), 256, 64),
    ("wide-fractional-xmin", (-170.7, -90.0, 600.1, 90.0), 3, 1000),
    ("narrow-fractional-xmin", (-1.3, 33.0, 6.1, 40.0), 64, 64),
]


def density_iterator_points(seed):
    """DensityIteratorTest's 15 features (DensityIteratorTest.scala:71-86): lon = i / 3 + 1 +
    (random - 0.5) / 1000, lat 37; the random is numpy's here."""
    rng = np.random.default_rng(seed)
    lon = np.array([(i // 3) + 1 + (rng.random() - 0.5) / 1000.0 for i in range(15)])
    return lon, np.full(15, 37.0)
