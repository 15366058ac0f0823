"""The attribute index restated in plain Python over `bytes`, independent of geomesa_amd/attribute.py.

From geomesa-index-api (idx/ = src/main/scala/org/locationtech/geomesa/index/):
  * the lexicoders: the written definition of include/geomesa_hip.h (Integer pinned by DefaultSplitterTest.scala:
    134-188; Long, Float, Double parity unpinned);
  * toIndexKey's row bytes (idx/index/attribute/AttributeIndexKeySpace.scala:68-137) and the tier encodings
    (none; DateIndexKeySpace.scala:48-56; Z3IndexKeySpace.scala:63-95 without a shard);
  * getRanges (:150-190), getRangeBytes (:192-285), lower / upper / tieredUpper (:294-343), DateIndexKeySpace's
    getRanges / getRangeBytes (:61-104), Z3IndexKeySpace.getRangeBytes (:196-213) and the tier combination of
    GeoMesaFeatureIndex.scala:298-356, line for line;
  * a reference store: rows sorted by their bytes (equal bytes keep input order, standing in for the feature id
    the store appends), a scan is lo <= row < hi by byte comparison over merged ranges, then the exact
    secondary filter;
  * the definitional answer: non-null rows whose value satisfies a bound and whose point and date satisfy the
    boxes and the interval, in table order.
A value satisfies a bound in the order of the key text, which is numeric order except that -0.0 sorts below
+0.0 and NaN above +infinity.
"""
import collections

import numpy as np

HEX = {"int": 8, "long": 16, "date": 16, "float": 8, "double": 16}
MIN_LONG = -(1 << 63)
UNB_LO, UNB_HI = b"", b"\xff\xff\xff"


# ---------------------------------------------------------------- lexicoders
def ordered(value, binding):
    if binding == "int":
        return int(np.array([value], np.int32).view(np.uint32)[0]) ^ 0x80000000
    if binding in ("long", "date"):
        return int(np.array([value], np.int64).view(np.uint64)[0]) ^ (1 << 63)
    if binding == "float":
        f = np.array([value], np.float32)
        b = 0x7fc00000 if np.isnan(f[0]) else int(f.view(np.uint32)[0])
        return (b ^ 0xffffffff) if b & 0x80000000 else (b | 0x80000000)
    d = np.array([value], np.float64)
    b = 0x7ff8000000000000 if np.isnan(d[0]) else int(d.view(np.uint64)[0])
    return (b ^ 0xffffffffffffffff) if b & (1 << 63) else (b | (1 << 63))


def encode(value, binding):
    return format(ordered(value, binding), "0%dx" % HEX[binding])


def decode(binding, text):
    v = int(text, 16)
    if binding == "int":
        return int(np.array([v ^ 0x80000000], np.uint32).view(np.int32)[0])
    if binding in ("long", "date"):
        return int(np.array([v ^ (1 << 63)], np.uint64).view(np.int64)[0])
    if binding == "float":
        b = (v & 0x7fffffff) if v & 0x80000000 else v ^ 0xffffffff
        return float(np.array([b], np.uint32).view(np.float32)[0])
    b = (v & ((1 << 63) - 1)) if v >> 63 else v ^ 0xffffffffffffffff
    return float(np.array([b], np.uint64).view(np.float64)[0])


def ordered_column(values, binding):
    return np.array([ordered(x, binding) for x in values], np.uint64)


# ---------------------------------------------------------------- row bytes
def ordered_long(ms):                                   # ByteArrays.toOrderedBytes(long)
    return ((int(ms) + (1 << 63)) % (1 << 64)).to_bytes(8, "big")


def tier_none():
    return b""


def tier_date(ms):                                      # a null date: Long.MinValue (DateIndexKeySpace.scala:54)
    return ordered_long(MIN_LONG if ms is None else ms)


def tier_z3(b, z):                                      # ByteArrays.toBytes(bin, z)
    return (int(b) % (1 << 16)).to_bytes(2, "big") + (int(z) % (1 << 64)).to_bytes(8, "big")


def row_key(value, binding, tier=b"", shard=None):
    """toIndexKey without the feature id; None for a null attribute (no row)."""
    if value is None:
        return None
    return (b"" if shard is None else bytes([shard])) + encode(value, binding).encode("utf-8") + b"\x00" + tier


def following_prefix(p):                                # ByteArrays.rowFollowingPrefix
    i = len(p) - 1
    while i >= 0 and p[i] == 0xff:
        i -= 1
    return b"" if i < 0 else p[:i] + bytes([p[i] + 1])


# ---------------------------------------------------------------- ranges
Key = collections.namedtuple("Key", "value inclusive")          # AttributeIndexKey(i, value, inclusive)
BR = collections.namedtuple("BR", "kind lower upper")           # ByteRange; single: the row in lower


def get_ranges(bounds, binding):
    """getRanges: bounds "disjoint", [] (no bounds extracted), or (lower, lower_inclusive, upper, upper_inclusive)s."""
    if bounds == "disjoint":
        return []
    if not bounds:
        return [("Unbounded", Key(None, False), None)]
    out = []
    for lo, li, hi, ui in bounds:
        if lo is None and hi is None:
            out.append(("Unbounded", Key(None, False), None))
        elif hi is None:
            out.append(("LowerBounded", Key(encode(lo, binding), li), None))
        elif lo is None:
            out.append(("UpperBounded", None, Key(encode(hi, binding), ui)))
        elif encode(lo, binding) == encode(hi, binding):
            out.append(("SingleRow", Key(encode(lo, binding), True), None))
        else:
            out.append(("Bounded", Key(encode(lo, binding), li), Key(encode(hi, binding), ui)))
    return out


def _lower(key):
    if key.value is None or key.value == "":
        return b""
    return key.value.encode("utf-8") + (b"\x00" if key.inclusive else b"\x01")


def _upper(key):
    if key.value is None or key.value == "":
        return UNB_HI
    return key.value.encode("utf-8") + (b"\x01" if key.inclusive else b"\x00")


def _tiered_upper(key):
    if key.value is None or not key.inclusive:
        return None
    return key.value.encode("utf-8") + b"\x00"


def get_range_bytes(ranges, tier, shards=0):
    null = Key(None, True)
    out = []
    for kind, lo, hi in ranges:
        if tier:
            if kind == "SingleRow":
                out.append(BR("single", _lower(lo), None))
            elif kind == "Bounded":
                up = _tiered_upper(hi)
                out.append(BR("lower", _lower(lo), _upper(hi)) if up is None else BR("bounded", _lower(lo), up))
            elif kind == "LowerBounded":
                out.append(BR("lower", _lower(lo), _upper(null)))
            elif kind == "UpperBounded":
                up = _tiered_upper(hi)
                out.append(BR("unbounded", _lower(null), _upper(hi)) if up is None else BR("upper", _lower(null), up))
            else:
                out.append(BR("unbounded", _lower(lo), _upper(lo)))
        else:
            a = _lower(null) if kind == "UpperBounded" else _lower(lo)
            b = {"SingleRow": lo, "Bounded": hi, "LowerBounded": null, "UpperBounded": hi, "Unbounded": lo}[kind]
            out.append(BR("bounded", a, _upper(b)))
    if not shards:
        return out
    return [BR(r.kind, bytes([p]) + r.lower, None if r.upper is None else bytes([p]) + r.upper)
            for r in out for p in range(shards)]


def date_ranges(intervals):
    """DateIndexKeySpace.getRanges; intervals: "disjoint", nothing, or (lower, lower_inclusive, upper, upper_inclusive)."""
    if intervals == "disjoint":
        return []
    if not intervals:
        return [("Unbounded", -1, None)]
    out = []
    for lo, li, hi, ui in intervals:
        if lo is not None and lo == hi and li and ui:
            out.append(("SingleRow", lo, None))
        else:
            a = MIN_LONG + 1 if lo is None else (lo if li else lo + 1)
            b = (1 << 63) - 1 if hi is None else (hi + 1 if ui else hi)
            out.append(("Bounded", a, b))
    return out


def date_range_bytes(ranges, tier=True):
    out = []
    for kind, a, b in ranges:
        if kind == "Bounded":
            out.append(BR("bounded", ordered_long(a), ordered_long(b)))
        elif kind == "SingleRow":
            o = ordered_long(a)
            out.append(BR("single", o, None) if tier else BR("bounded", o, following_prefix(o)))
        else:
            out.append(BR("unbounded", ordered_long(MIN_LONG + 1), following_prefix(ordered_long((1 << 63) - 1))))
    return out


def z3_range_bytes(scan_ranges):
    """Z3IndexKeySpace.getRangeBytes, no shard, over (kind, (bin, z) lower, (bin, z) upper) scan ranges."""
    def following(b, z):
        return ((int.from_bytes(tier_z3(b, z), "big") + 1) % (1 << 80)).to_bytes(10, "big")
    out = []
    for kind, lo, hi in scan_ranges:
        if kind == "bounded":
            out.append(BR("bounded", tier_z3(*lo), following(*hi)))
        elif kind == "lower":
            out.append(BR("bounded", tier_z3(*lo), UNB_HI))
        elif kind == "upper":
            out.append(BR("bounded", UNB_LO, following(*hi)))
        else:
            out.append(BR("bounded", UNB_LO, UNB_HI))
    return out


def combine(primary, tiers):
    """GeoMesaFeatureIndex.scala:308-356; tiers None: no secondary filter."""
    if tiers is None or any(t.kind == "unbounded" for t in tiers):
        out = []
        for r in primary:
            if r.kind in ("bounded", "upper"):
                out.append(BR("bounded", r.lower, r.upper + UNB_HI))
            elif r.kind == "single":
                out.append(BR("bounded", r.lower, r.lower + UNB_HI))
            else:
                out.append(BR("bounded", r.lower, r.upper))
        return out
    if not tiers:
        return []
    lows = [t.lower for t in tiers]
    highs = [t.lower if t.kind == "single" else t.upper for t in tiers]
    mn, mx = min(lows), max(highs)
    out = []
    for r in primary:
        if r.kind == "single":
            for t in tiers:
                if t.kind == "single":
                    out.append(BR("single", r.lower + t.lower, None))
                else:
                    out.append(BR("bounded", r.lower + t.lower, r.lower + t.upper))
        elif r.kind == "bounded":
            out.append(BR("bounded", r.lower + mn, r.upper + mx))
        elif r.kind == "lower":
            out.append(BR("bounded", r.lower + mn, r.upper))
        elif r.kind == "upper":
            out.append(BR("bounded", r.lower, r.upper + mx))
        else:
            out.append(BR("bounded", r.lower, r.upper))
    return out


def scan_bounds(byte_ranges):
    """[lo, hi) pairs of bounded / single ranges (a single row: every row with that prefix; an empty hi: no end)."""
    return [(r.lower, following_prefix(r.lower) if r.kind == "single" else r.upper) for r in byte_ranges]


def merged(pairs):
    out = []
    for lo, hi in sorted(pairs, key=lambda p: p[0]):
        if hi != b"" and hi <= lo:
            continue
        if out and (out[-1][1] == b"" or lo <= out[-1][1]):
            if out[-1][1] != b"" and (hi == b"" or hi > out[-1][1]):
                out[-1] = (out[-1][0], hi)
            continue
        out.append((lo, hi))
    return out


def overlaps(pairs):
    """AttributeIndexTest.scala:65-71, 91-97 over the sorted ranges."""
    s = sorted(pairs, key=lambda p: p[0])
    return any(a[0] == b[0] or a[1] == b"" or a[1] > b[0] for a, b in zip(s, s[1:]))


# ---------------------------------------------------------------- the z3 tier on the host
class HostZ3SFC:
    """What keyspace.Z3IndexKeySpace needs of its curve, with ZN.zranges from the CPU oracle."""
    R = collections.namedtuple("R", "lower upper")

    def __init__(self, period):
        from geomesa_amd.curve import Z3SFC
        self._sfc = Z3SFC(period)
        self.period, self.time, self.wholePeriod = self._sfc.period, self._sfc.time, self._sfc.wholePeriod

    def ranges_batch(self, queries, precision=64, max_ranges=None, max_recurse=None):
        import oracle as O
        return [[self.R(lo, hi) for lo, hi, _ in O.z3_ranges(xy, t, precision, max_ranges, period=self.period)]
                for xy, t in queries]


def z3_tier_ranges(period, bboxes, intervals, multiplier, target=2000):
    """The Z3 tier's byte ranges for a secondary filter (Z3IndexKeySpace.getIndexValues / getRanges(values,
    multiplier) / getRangeBytes)."""
    from geomesa_amd.keyspace import Bounds, Z3IndexKeySpace
    ks = Z3IndexKeySpace(period, sfc=HostZ3SFC(period))
    values = ks.get_index_values(bboxes, [Bounds(*_bounds_args(i)) for i in (intervals or [])])
    if values.disjoint:
        return []
    return z3_range_bytes(ks.get_ranges(values, multiplier=multiplier, target=target))


def _bounds_args(i):
    lo, li, hi, ui = i
    return lo, hi, li, ui


# ---------------------------------------------------------------- the store
class Store:
    """Rows (key prefix bytes, None for a null attribute) sorted by their bytes, ties in input order."""

    def __init__(self, keys):
        self.rows = [i for i, k in enumerate(keys) if k is not None]          # the rows written, input order
        self.order = sorted(self.rows, key=lambda i: keys[i])                 # table row -> input row (stable)
        self.keys = [keys[i] for i in self.order]
        self.length = len(self.keys[0]) if self.keys else 0
        self.ordered = None      # input row -> ordered value, filled by definition()

    def candidates(self, byte_ranges):
        """Table rows with lo <= row < hi for a merged range; the bounds never outgrow the key prefix, so the
        feature id behind it takes no part."""
        import bisect
        ms = merged(scan_bounds(byte_ranges))
        assert all(len(lo) <= self.length and len(hi) <= self.length for lo, hi in ms) or not self.keys
        out = []       # the merged ranges are disjoint and ascending, and so are their row intervals
        for lo, hi in ms:
            out.extend(range(bisect.bisect_left(self.keys, lo),
                             len(self.keys) if hi == b"" else bisect.bisect_left(self.keys, hi)))
        return out


def plan(bounds, binding, tier, shards=0, bboxes=None, intervals=None, period=1, target=2000):
    """A query's combined byte ranges: getRanges -> getRangeBytes -> the tier combination."""
    primary = get_range_bytes(get_ranges(bounds, binding), tier is not None, shards)
    if tier is None:
        return primary
    if not bboxes and not intervals:
        return combine(primary, None)
    if tier == "date":
        return combine(primary, date_range_bytes(date_ranges(intervals)))
    mult = max(1, sum(1 for r in primary if r.kind == "single"))
    return combine(primary, z3_tier_ranges(period, bboxes, intervals, mult, target))


def ordered_bounds(bounds, binding):
    """getRanges' bounds with their ends as ordered values."""
    if bounds == "disjoint":
        return "disjoint"
    return [(None if lo is None else ordered(lo, binding), li, None if hi is None else ordered(hi, binding), ui)
            for lo, li, hi, ui in bounds]


def satisfies(v, obounds):
    """v (ordered) against ordered_bounds, in key-text order."""
    if obounds == "disjoint":
        return False
    if not obounds:
        return True
    for a, li, b, ui in obounds:
        if a is not None and a == b:
            if v == a:
                return True
            continue
        if (a is None or v > a or (li and v == a)) and (b is None or v < b or (ui and v == b)):
            return True
    return False


def secondary(x, y, t, bboxes, intervals):
    """The exact secondary filter on one feature: inclusive boxes on the point, the interval on the dtg.  A null
    date (Long.MinValue in the column) satisfies no interval, an open-ended one included."""
    if bboxes and not any(b[0] <= x <= b[2] and b[1] <= y <= b[3] for b in bboxes):
        return False
    if intervals and t == MIN_LONG:
        return False
    for lo, li, hi, ui in (intervals or []):
        if not ((lo is None or t > lo or (li and t == lo)) and (hi is None or t < hi or (ui and t == hi))):
            return False
    return True


def definition(store, values, binding, bounds, x=None, y=None, t_ms=None, bboxes=None, intervals=None):
    """ids in table order: non-null rows whose value satisfies a bound and whose point and date pass."""
    out = []
    ob = ordered_bounds(bounds, binding)
    if store.ordered is None:
        store.ordered = {i: ordered(values[i], binding) for i in store.order}
    for i in store.order:
        if not satisfies(store.ordered[i], ob):
            continue
        if secondary(None if x is None else x[i], None if y is None else y[i], None if t_ms is None else t_ms[i],
                     bboxes, intervals):
            out.append(i)
    return out
