"""The density (heatmap) scan: point and line features rendered into a grid of pixels.

Mirrors DensityScan (geomesa-index-api/.../iterators/DensityScan.scala:29-49, 201-212) over batches of point
features: every feature the scan kept is snapped into a pixel of a width x height grid over an envelope and
its weight is added there (RenderingGrid.render, geomesa-utils/.../geotools/RenderingGrid.scala:43-49, with
GridSnap.i / j, geomesa-utils/.../geotools/GridSnap.scala:60-80, and the 360-degree translate / widen,
RenderingGrid.scala:299-330); LineString and MultiLineString features by the Bresenham walk of
RenderingGrid.scala:72-157 (render_lines, gm_density_lines).  The per-row work runs in the gm_density_points /
gm_density_arrow / gm_density_lines kernels; RenderingGrid keeps the pixels as a dense float64 device tensor.  GridSnap is the host-side class, in numpy
float64 with the reference's arithmetic.  The contract, and the three places where the dense grid departs
from the reference's map of pixels (.skipped, .dropped, .bad_ids), are stated in include/geomesa_hip.h.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr

INT_MAX = 2147483647


def _to_int(q):
    """Scala's Double.toInt over an array: NaN -> 0, saturating (JLS 5.1.3)."""
    q = np.asarray(q, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.where(np.isnan(q), 0.0, q), -2147483648.0, 2147483647.0)
    return r.astype(np.int64)


class GridSnap:
    """GridSnap(env, xSize, ySize) (GridSnap.scala:23-82); env = (xmin, ymin, xmax, ymax).  Scalars in,
    scalars out; arrays in, arrays out."""

    def __init__(self, env, width, height):
        self.xmin, self.ymin, self.xmax, self.ymax = (np.float64(v) for v in env)
        self.width, self.height = int(width), int(height)
        with np.errstate(all="ignore"):
            self.dx = (self.xmax - self.xmin) / np.float64(self.width)     # GridSnap.scala:32-33
            self.dy = (self.ymax - self.ymin) / np.float64(self.height)
            self.x_offset = self.xmin + self.dx / np.float64(2)            # GridSnap.scala:35-36
            self.y_offset = self.ymin + self.dy / np.float64(2)

    @staticmethod
    def _index(v, lo, hi, d, size):
        a = np.asarray(v, np.float64)
        with np.errstate(all="ignore"):
            q = _to_int(np.floor((a - lo) / d))
        out = np.where((a < lo) | (a > hi), -1, np.minimum(q, size - 1))
        return int(out) if out.ndim == 0 else out

    def i(self, x):
        """GridSnap.i (GridSnap.scala:60-66)."""
        return self._index(x, self.xmin, self.xmax, self.dx, self.width)

    def j(self, y):
        """GridSnap.j (GridSnap.scala:74-80)."""
        return self._index(y, self.ymin, self.ymax, self.dy, self.height)

    def x(self, i):
        """GridSnap.x (GridSnap.scala:44)."""
        r = self.x_offset + self.dx * np.asarray(i, np.float64)
        return float(r) if r.ndim == 0 else r

    def y(self, j):
        """GridSnap.y (GridSnap.scala:52)."""
        r = self.y_offset + self.dy * np.asarray(j, np.float64)
        return float(r) if r.ndim == 0 else r

    def snap(self, x, y):
        """GridSnap.snap (GridSnap.scala:82)."""
        return self.x(self.i(x)), self.y(self.j(y))


class RenderingGrid:
    """RenderingGrid(env, xSize, ySize) for point and line features (RenderingGrid.scala:25-157), the pixels a dense
    float64 [height, width] device tensor; env = (xmin, ymin, xmax, ymax).

    render / render_arrow / render_lines add a batch; batches add up, and so do the grids of several ranks (any
    all-reduce of .grid).  A batch is every row, or the rows a scan or a table query kept:

        ids, _, _ = table.query(bboxes, intervals)          # Z3Table, Z2Table, XZ2Table, XZ3Table
        grid.render(x, y, ids=ids)
        mask, _, _ = filters.query_scan(x, y, t_ms, bbox=bbox, during=during)
        grid.render(x, y, mask=mask)

    (x, y the columns the table was built from, in input order; the tables themselves are untouched.)
    .skipped, .dropped and .bad_ids count what the dense grid leaves out (geomesa_hip.h): unrenderable
    rows (null, non-finite, |x| > 2^31), additions whose column came out -1, and ids outside [0, n).
    path and workgroups reach gm_density_grid's fields of those names (tests; results do not change)."""

    def __init__(self, env, width, height, device=None, path=0, workgroups=0):
        import torch
        self.snap = GridSnap(env, width, height)
        self.env = tuple(float(v) for v in env)
        self.width, self.height = int(width), int(height)
        self._device = device
        self.path, self.workgroups = int(path), int(workgroups)
        ctx = _lib.context(device)
        dev = torch.device("cuda", ctx.device)
        if self.width < 1 or self.height < 1 or self.width * self.height > INT_MAX:
            raise ValueError("width and height must be at least 1 and width * height at most 2^31 - 1")
        self.grid = torch.zeros((self.height, self.width), dtype=torch.float64, device=dev)
        self._tally = torch.zeros(3, dtype=torch.int64, device=dev)

    def _c(self):
        return _lib.DensityGrid(self.env[0], self.env[1], self.env[2], self.env[3], self.width, self.height,
                                self.workgroups, self.path)

    def render(self, x, y, weight=None, mask=None, ids=None):
        """RenderingGrid.render(Point, weight) for rows of x / y columns (weight: None = 1.0, or a column)."""
        import torch
        from .curve import _dev_col, _selection
        x = _dev_col(x, torch.float64)
        y = _dev_col(y, torch.float64)
        w = _dev_col(weight, torch.float64) if weight is not None else None
        n = x.numel()
        if y.numel() != n or (w is not None and w.numel() != n):
            raise ValueError("x, y and weight must have one entry per row")
        mask, ids, n_ids = _selection(n, mask, ids, self.grid.device)
        ctx = _lib.context(self._device)
        g = self._c()
        check(ctx.lib.gm_density_points(ctx.handle, ptr(x), ptr(y), ptr(w), n, ptr(mask), ptr(ids), n_ids,
                                        ctypes.byref(g), ptr(self.grid), ptr(self._tally)), "gm_density_points")
        return self

    def render_arrow(self, col, weight=None, mask=None, ids=None, kind="point", flip_axis=False):
        """render over an Arrow Point or MultiPoint column (an arrow.GeometryColumn, or a pyarrow array of
        `kind`); every point of a MultiPoint gets the slot's weight (RenderingGrid.scala:57-64)."""
        import torch
        from .arrow import _as_geom
        from .curve import _dev_col, _selection
        col = _as_geom(col, kind, flip_axis)
        if col.kind not in ("point", "multipoint"):
            raise ValueError("the density scan renders Point and MultiPoint columns")
        n = col.n
        w = _dev_col(weight, torch.float64) if weight is not None else None
        if w is not None and w.numel() != n:
            raise ValueError("weight must have one entry per slot")
        mask, ids, n_ids = _selection(n, mask, ids, self.grid.device)
        ctx = _lib.context(self._device)
        g = self._c()
        cs = col.c_struct()
        check(ctx.lib.gm_density_arrow(ctx.handle, ctypes.byref(cs), ptr(w), n, ptr(mask), ptr(ids), n_ids,
                                       ctypes.byref(g), ptr(self.grid), ptr(self._tally)), "gm_density_arrow")
        return self

    def render_lines(self, col, weight=None, mask=None, ids=None, kind="linestring", flip_axis=False):
        """RenderingGrid.render(LineString / MultiLineString, weight) (RenderingGrid.scala:72-157) over an
        Arrow LineString or MultiLineString column (an arrow.GeometryColumn, or a pyarrow array of `kind`):
        every pixel of a line's Bresenham walk gets the slot's whole weight; a segment that leaves the
        envelope is clipped to it (include/geomesa_hip.h states the walk and the clip).  Polygons are not
        rendered.  The slots a table query kept:

            ids, _, _ = xz2table.query(bboxes)               # XZ2Table / XZ3Table over the same column
            grid.render_lines(col, ids=ids)

        .skipped counts null slots and parts with a non-finite ordinate or |x| > 2^31, once each."""
        import torch
        from .arrow import _as_geom
        from .curve import _dev_col, _selection
        col = _as_geom(col, kind, flip_axis)
        if col.kind not in ("linestring", "multilinestring"):
            raise ValueError("render_lines renders LineString and MultiLineString columns")
        n = col.n
        w = _dev_col(weight, torch.float64) if weight is not None else None
        if w is not None and w.numel() != n:
            raise ValueError("weight must have one entry per slot")
        mask, ids, n_ids = _selection(n, mask, ids, self.grid.device)
        ctx = _lib.context(self._device)
        g = self._c()
        cs = col.c_struct()
        check(ctx.lib.gm_density_lines(ctx.handle, ctypes.byref(cs), ptr(w), n, ptr(mask), ptr(ids), n_ids,
                                       ctypes.byref(g), ptr(self.grid), ptr(self._tally)), "gm_density_lines")
        return self

    @property
    def tally(self):
        return [int(v) for v in self._tally.cpu().tolist()]

    @property
    def skipped(self):
        return self.tally[0]

    @property
    def dropped(self):
        return self.tally[1]

    @property
    def bad_ids(self):
        return self.tally[2]

    def is_empty(self):
        """RenderingGrid.isEmpty, for the pixels sparse() reports."""
        return not bool((self.grid != 0).any())

    def sparse(self, cap=None):
        """(i, j, w) device tensors of the pixels with w != 0.0, ordered by column i then row j -- the groups
        DensityScan.encodeResult writes (DensityScan.scala:95-106)."""
        import torch
        ctx = _lib.context(self._device)
        dev = self.grid.device
        n = ctypes.c_int64()
        if cap is None:
            rc = ctx.lib.gm_density_sparse(ctx.handle, ptr(self.grid), self.width, self.height, 0, None, None, None,
                                           ctypes.byref(n))
            if rc != _lib.GM_E_CAPACITY:
                check(rc, "gm_density_sparse")
            cap = n.value
        i = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        j = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        w = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
        check(ctx.lib.gm_density_sparse(ctx.handle, ptr(self.grid), self.width, self.height, cap, ptr(i), ptr(j),
                                        ptr(w), ctypes.byref(n)), "gm_density_sparse")
        k = n.value
        return i[:k], j[:k], w[:k]

    def decode(self):
        """(x, y, w) host arrays as DensityScan.decodeResult yields them (DensityScan.scala:118-136): the
        pixel centres GridSnap.x(i), GridSnap.y(j) of sparse()'s cells and their weights."""
        i, j, w = self.sparse()
        return self.snap.x(i.cpu().numpy()), self.snap.y(j.cpu().numpy()), w.cpu().numpy()

    def clear(self):
        """RenderingGrid.clear (RenderingGrid.scala:290); the tallies start again as well."""
        self.grid.zero_()
        self._tally.zero_()


__all__ = ["GridSnap", "RenderingGrid"]
