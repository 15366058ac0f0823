"""Host reference for GM_GEOM_WKB columns (WKBGeometryVector: an Arrow Binary column, one WKB blob per slot).

A geometry is (kind, row): kind one of the six of geom_intersects_ref with its row form (a point (x, y),
nested lists of (x, y) for the others, rings shell first), or ("collection", [geometry, ...]).  The empty
point is ("point", (nan, nan)).

  write(geom, style)   a WKB writer over the grammar geomesa_hip.h states: both byte orders, Z / M / ZM in
                       the EWKB flag style and the ISO thousands style, SRID, and -- through `pick` -- a
                       style of its own for every nested geometry (orders mixed inside one collection).
                       Z and M ordinates are written as FILL, so a reader that did not skip them shows.
  read(blob)           an independent reader (struct, recursive) back to that form; Malformed for a slot the
                       grammar rejects.  parse(blob) is read() with None for a malformed or null slot.
  envelope(geom)       the JTS envelope rules restated: a tuple run's first tuple initialises and strict
                       compares widen; a polygon's is its shell's; a collection's the merge of its elements',
                       null ones skipped; an empty geometry gives (0, 0, -1, -1).
  intersects(geom, b)  geom_intersects_ref per element, any() over a collection; a LineString of one tuple
                       is that point.
  xz2_keys / xz3_keys  the oracle's XZ index of those envelopes, with the key entries' statuses.
"""
import math
import struct

import numpy as np

import geom_intersects_ref as R

MAX_DEPTH = 8
NULL_ENV = (0.0, 0.0, -1.0, -1.0)
NULL_GEOM, UNORDERED = 4, 3
FILL = 777.25
CODES = {"point": 1, "linestring": 2, "polygon": 3, "multipoint": 4, "multilinestring": 5, "multipolygon": 6,
         "collection": 7}
ELEMENT = {"multipoint": "point", "multilinestring": "linestring", "multipolygon": "polygon"}
EMPTY_POINT = ("point", (math.nan, math.nan))


class Malformed(Exception):
    pass


class Style:
    """le: little-endian; dims: "", "z", "m" or "zm"; iso: the thousands style instead of the flag bits;
    srid: None or the SRID to write."""

    def __init__(self, le=False, dims="", iso=False, srid=None):
        self.le, self.dims, self.iso, self.srid = le, dims, iso, srid

    def type_int(self, code):
        z, m = "z" in self.dims, "m" in self.dims
        t = code + 1000 * (z + 2 * m) if self.iso else code | (0x80000000 * z) | (0x40000000 * m)
        return t | (0x20000000 if self.srid is not None else 0)


BE, LE = Style(False), Style(True)


def typed(rows, kind):
    """Rows of one typed kind (None: a null slot) as geometries."""
    return [None if r is None else (kind, r) for r in rows]


# ---------------------------------------------------------------- writer
def write(geom, style=BE, pick=None, _path=()):
    """pick(path, geom) -> Style or None for a nested geometry at `path` (indices from the top)."""
    kind, row = geom
    s = (pick(_path, geom) if pick and _path else None) or style
    e = "<" if s.le else ">"
    out = [struct.pack("B", 1 if s.le else 0), struct.pack(e + "I", s.type_int(CODES[kind]))]
    if s.srid is not None:
        out.append(struct.pack(e + "I", s.srid))

    def tuples(ts):
        a = np.full((len(ts), 2 + len(s.dims)), FILL, e + "f8")
        if len(ts):
            a[:, :2] = ts
        return a.tobytes()
    if kind == "point":
        out.append(tuples([row]))
    elif kind == "linestring":
        out += [struct.pack(e + "I", len(row)), tuples(row)]
    elif kind == "polygon":
        out.append(struct.pack(e + "I", len(row)))
        for ring in row:
            out += [struct.pack(e + "I", len(ring)), tuples(ring)]
    else:
        elems = row if kind == "collection" else [(ELEMENT[kind], r) for r in row]
        out.append(struct.pack(e + "I", len(elems)))
        out += [write(g, s, pick, _path + (k,)) for k, g in enumerate(elems)]
    return b"".join(out)


# ---------------------------------------------------------------- reader
def _read(b, at, depth, want):
    def take(fmt, at):
        n = struct.calcsize(fmt)
        if at + n > len(b):
            raise Malformed("past the slot's end")
        return struct.unpack_from(fmt, b, at), at + n
    (order,), at = take("B", at)
    if order > 1:
        raise Malformed("order byte %d" % order)
    e = "<" if order else ">"
    (t,), at = take(e + "I", at)
    if t & 0x20000000:
        _, at = take(e + "I", at)
    code, iso = (t & 0xffff) % 1000, (t & 0xffff) // 1000
    nd = 2 + bool(t & 0x80000000 or iso in (1, 3)) + bool(t & 0x40000000 or iso in (2, 3))
    if not 1 <= code <= 7:
        raise Malformed("code %d" % code)
    if want is not None and code != want:
        raise Malformed("element code %d in a Multi* of %d" % (code, want))

    def run(at):
        (n,), at = take(e + "I", at)
        if at + n * 8 * nd > len(b):
            raise Malformed("a tuple run past the slot's end")
        v = np.frombuffer(b, e + "f8", n * nd, at).reshape(n, nd)
        return [(float(x), float(y)) for x, y in v[:, :2]], at + n * 8 * nd
    if code == 1:
        v, at = take(e + "%dd" % nd, at)
        return ("point", (v[0], v[1])), at
    if code == 2:
        ts, at = run(at)
        return ("linestring", ts), at
    if code == 3:
        (nr,), at = take(e + "I", at)
        rings = []
        for _ in range(nr):
            ts, at = run(at)
            rings.append(ts)
        return ("polygon", rings), at
    if depth == MAX_DEPTH:
        raise Malformed("nested deeper than %d" % MAX_DEPTH)
    (n,), at = take(e + "I", at)
    elems = []
    for _ in range(n):
        g, at = _read(b, at, depth + 1, None if code == 7 else code - 3)
        elems.append(g)
    kind = [k for k, c in CODES.items() if c == code][0]
    return (kind, elems if code == 7 else [g[1] for g in elems]), at


def read(blob):
    return _read(bytes(blob), 0, 0, None)[0]


def parse(blob):
    if blob is None:
        return None
    try:
        return read(blob)
    except Malformed:
        return None


# ---------------------------------------------------------------- envelopes
def _run_env(ts):
    e = None
    for x, y in ts:
        if e is None:
            e = [x, x, y, y]
            continue
        if x < e[0]: e[0] = x
        if x > e[1]: e[1] = x
        if y < e[2]: e[2] = y
        if y > e[3]: e[3] = y
    return e


def _merge(e, o):
    if o is None:
        return e
    if e is None:
        return list(o)
    if o[0] < e[0]: e[0] = o[0]
    if o[1] > e[1]: e[1] = o[1]
    if o[2] < e[2]: e[2] = o[2]
    if o[3] > e[3]: e[3] = o[3]
    return e


def _env(geom):
    kind, row = geom
    if kind == "point":
        return None if (math.isnan(row[0]) or math.isnan(row[1])) else [row[0], row[0], row[1], row[1]]
    if kind == "linestring":
        return _run_env(row)
    if kind == "polygon":
        return _run_env(row[0]) if row else None
    elems = row if kind == "collection" else [(ELEMENT[kind], r) for r in row]
    e = None
    for g in elems:
        e = _merge(e, _env(g))
    return e


def envelope(geom):
    """(minx, miny, maxx, maxy); a null / malformed slot (None) and an empty geometry: (0, 0, -1, -1)."""
    e = None if geom is None else _env(geom)
    return NULL_ENV if e is None else (e[0], e[2], e[1], e[3])


def envelopes(geoms):
    e = np.array([envelope(g) for g in geoms], np.float64).reshape(-1, 4)
    return e[:, 0], e[:, 1], e[:, 2], e[:, 3]


# ---------------------------------------------------------------- geometry meets box
def intersects(geom, box, fn=R.intersects_restated):
    if geom is None:
        return False
    kind, row = geom
    if kind == "collection":
        return any(intersects(g, box, fn) for g in row)
    if kind == "multilinestring":
        return any(intersects(("linestring", r), box, fn) for r in row)
    if kind == "linestring" and len(row) == 1:
        kind, row = "point", row[0]
    return fn(row, kind, box)


def scan(geoms, boxes, fn=R.intersects_restated):
    return np.array([any(intersects(g, b, fn) for b in boxes) for g in geoms], bool)


def env_scan(geoms, boxes):
    """The envelope filter: the slot's envelope meets a box (JTS Envelope.intersects; a null one never)."""
    def hit(e, b):
        return not (e[2] < e[0] or b[2] < b[0] or b[0] > e[2] or b[2] < e[0] or b[1] > e[3] or b[3] < e[1])
    return np.array([any(hit(envelope(g), b) for b in boxes) for g in geoms], bool)


def env_inside(geom, box):
    e = envelope(geom)
    return e[2] >= e[0] and e[0] >= box[0] and e[2] <= box[2] and e[1] >= box[1] and e[3] <= box[3]


# ---------------------------------------------------------------- XZ keys of the envelopes
def xz2_keys(geoms, g=12, lenient=False):
    import oracle as O
    z, st = np.zeros(len(geoms), np.int64), np.zeros(len(geoms), np.uint8)
    for i, gm in enumerate(geoms):
        if gm is None:
            st[i] = NULL_GEOM
            continue
        st[i], z[i] = O.xz2_index(*envelope(gm), lenient=lenient, g=g)
        if st[i]:
            z[i] = 0
    return z, st


def xz3_keys(geoms, t_ms, g=12, period=1, lenient=False):
    """period: oracle.WEEK by default, as arrow.xz3_index_keys."""
    import oracle as O
    n = len(geoms)
    b, z, st = np.zeros(n, np.int16), np.zeros(n, np.int64), np.zeros(n, np.uint8)
    for i, (gm, t) in enumerate(zip(geoms, t_ms)):
        if gm is None:
            st[i] = NULL_GEOM
            continue
        s, bb, off = O.binned_time(period, int(t))
        if not s:
            x0, y0, x1, y1 = envelope(gm)
            s, zz = O.xz3_index(x0, y0, float(off), x1, y1, float(off), lenient=lenient, g=g, period=period)
        st[i] = s
        if not s:
            b[i], z[i] = bb, zz
    return b, z, st
