"""The attribute index (`attr`, version 8) for fixed-width bindings: key encoding, range planning with the
secondary tier, and a table resident in HBM beside Z3Table.

Mirrors geomesa-index-api/src/main/scala/org/locationtech/geomesa/index/ (idx/):
  * AttributeIndexKey (idx/index/attribute/AttributeIndexKey.scala:41-84): typeEncode / decode / encodeForQuery.
    The lexicoders themselves (org.calrissian.mango LexiTypeEncoders) are outside the reference tree; the
    definition is the table in include/geomesa_hip.h.  Integer is pinned by DefaultSplitterTest.scala:134-188;
    Long, Float and Double are parity unpinned.
  * AttributeIndexKeySpace.getRanges (idx/index/attribute/AttributeIndexKeySpace.scala:150-190), getRangeBytes
    (:192-285) with lower / upper / tieredUpper (:294-343).
  * DateIndexKeySpace (idx/index/attribute/DateIndexKeySpace.scala:48-104) and Z3IndexKeySpace.getRangeBytes
    without a shard (idx/index/z3/Z3IndexKeySpace.scala:196-213) as the tiers.
  * GeoMesaFeatureIndex.getQueryStrategy's combination of primary and tier byte ranges
    (idx/api/GeoMesaFeatureIndex.scala:298-356): combine_tiers.
Planning is per query and runs on the host; the per-row work -- gm_attr_index_key, gm_attr_sort,
gm_attr_key_bytes, gm_attr_table_scan -- runs on the GPU through libgeomesa_hip.

Not built (NotImplementedError): String bindings (variable-length keys need a different sort), List
attributes, the XZ3 / Z2 / XZ2 tiers, the legacy index versions and the join index, attribute-level visibility.
"""
import ctypes
import math
import struct
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, ptr
from .keyspace import Bounds, Z3IndexKeySpace

# binding -> (GM_ATTR_*, hex digits of the key text)
_BINDINGS = {
    "int": (_lib.GM_ATTR_INT32, 8), "integer": (_lib.GM_ATTR_INT32, 8),
    "long": (_lib.GM_ATTR_INT64, 16), "date": (_lib.GM_ATTR_INT64, 16), "timestamp": (_lib.GM_ATTR_INT64, 16),
    "float": (_lib.GM_ATTR_FLOAT32, 8), "double": (_lib.GM_ATTR_FLOAT64, 16),
}
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1
_NOT_BUILT = "the attribute index is built for Integer, Long, Date, Timestamp, Float and Double bindings; "


def binding_of(binding):
    """(GM_ATTR_* type, hex digits) of a binding name; String and List bindings are not built."""
    b = str(binding).lower()
    if b in ("string", "utf8"):
        raise NotImplementedError(_NOT_BUILT + "String needs variable-length keys and a different sort")
    if b.startswith("list"):
        raise NotImplementedError(_NOT_BUILT + "List attributes write several rows per feature")
    if b not in _BINDINGS:
        raise NotImplementedError(_NOT_BUILT + "not %r" % (binding,))
    return _BINDINGS[b]


class AttributeIndexKey:
    """AttributeIndexKey's lexicoding (AttributeIndexKey.scala:41-84) on the host."""

    @staticmethod
    def ordered(value, binding):
        """The ordered value v of include/geomesa_hip.h's table: unsigned order of v = order of the key text."""
        typ, _ = binding_of(binding)
        if typ == _lib.GM_ATTR_INT32:
            return (int(value) & _M32) ^ 0x80000000
        if typ == _lib.GM_ATTR_INT64:
            return (int(value) & _M64) ^ (1 << 63)
        x = float(value)
        if typ == _lib.GM_ATTR_FLOAT32:
            b = 0x7fc00000 if math.isnan(x) else struct.unpack(">I", struct.pack(">f", x))[0]
            return (~b & _M32) if b >> 31 else b ^ 0x80000000
        b = 0x7ff8000000000000 if math.isnan(x) else struct.unpack(">Q", struct.pack(">d", x))[0]
        return (~b & _M64) if b >> 63 else b ^ (1 << 63)

    @staticmethod
    def type_encode(value, binding):
        """typeEncode (AttributeIndexKey.scala:67): the key text, lower-case hex of the ordered value."""
        _, digits = binding_of(binding)
        return "%0*x" % (digits, AttributeIndexKey.ordered(value, binding))

    @staticmethod
    def decode(binding, text):
        """decode (AttributeIndexKey.scala:84): the value a key text encodes."""
        typ, digits = binding_of(binding)
        if len(text) != digits:
            raise ValueError("a %s key has %d hex digits: %r" % (binding, digits, text))
        v = int(text, 16)
        if typ == _lib.GM_ATTR_INT32:
            u = v ^ 0x80000000
            return u - (1 << 32) if u >> 31 else u
        if typ == _lib.GM_ATTR_INT64:
            u = v ^ (1 << 63)
            return u - (1 << 64) if u >> 63 else u
        if typ == _lib.GM_ATTR_FLOAT32:
            b = v ^ 0x80000000 if v >> 31 else ~v & _M32
            return struct.unpack(">f", struct.pack(">I", b))[0]
        b = v ^ (1 << 63) if v >> 63 else ~v & _M64
        return struct.unpack(">d", struct.pack(">Q", b))[0]

    @staticmethod
    def encode_for_query(value, binding):
        """encodeForQuery (AttributeIndexKey.scala:55-59): null stays null; the value converted to the binding."""
        return None if value is None else AttributeIndexKey.type_encode(value, binding)


# ScanRange[AttributeIndexKey]: kind in single / bounded / lower / upper / unbounded; a key is (text, inclusive)
ScanRange = namedtuple("ScanRange", "kind lower upper")
# ByteRange (idx/api/package.scala:276-318): kind in bounded / single / lower / upper / unbounded; a single
# row keeps its row in `lower`
ByteRange = namedtuple("ByteRange", "kind lower upper")
UNBOUNDED_LOWER = b""                 # ByteRange.UnboundedLowerRange
UNBOUNDED_UPPER = b"\xff\xff\xff"     # ByteRange.UnboundedUpperRange
DISJOINT = "disjoint"                 # FilterValues.disjoint as query()'s bounds


def row_following_prefix(prefix):
    """ByteArrays.rowFollowingPrefix: empty when every byte is 0xff."""
    p = bytes(prefix).rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else b""


def _ordered_long(ms):
    """ByteArrays.toOrderedBytes(long): sign bit flipped, big-endian."""
    return struct.pack(">Q", (int(ms) & _M64) ^ (1 << 63))


class AttributeIndexKeySpace:
    """getRanges / getRangeBytes of AttributeIndexKeySpace for one attribute of a fixed-width binding."""

    def __init__(self, binding, shards=None):
        self.binding = binding
        self.type, self.digits = binding_of(binding)
        self.shards = int(shards) if shards else 0

    def prefixes(self):
        """ShardStrategy.shards: one byte each; none for an unsharded table."""
        return [bytes([s]) for s in range(self.shards)]

    # getRanges (AttributeIndexKeySpace.scala:150-190)
    def get_ranges(self, bounds):
        """bounds: DISJOINT, or a list of (lower, lower_inclusive, upper, upper_inclusive) with None for an
        open end (one tuple is taken as a list of one); an empty list scans every value."""
        enc = lambda v: AttributeIndexKey.encode_for_query(v, self.binding)
        if isinstance(bounds, str) and bounds == DISJOINT:
            return []                                                    # :159-160
        if isinstance(bounds, tuple):
            bounds = [bounds]
        if not bounds:
            return [ScanRange("unbounded", (None, False), None)]         # :156-158
        out = []
        for lower, lower_inc, upper, upper_inc in bounds:
            if lower is None and upper is None:                          # not null (:164-165)
                out.append(ScanRange("unbounded", (None, False), None))
            elif upper is None:
                out.append(ScanRange("lower", (enc(lower), bool(lower_inc)), None))
            elif lower is None:
                out.append(ScanRange("upper", None, (enc(upper), bool(upper_inc))))
            elif enc(lower) == enc(upper):                               # lower == upper (:176-178)
                out.append(ScanRange("single", (enc(lower), True), None))
            else:                                                        # (a PrefixRange needs a String)
                out.append(ScanRange("bounded", (enc(lower), bool(lower_inc)), (enc(upper), bool(upper_inc))))
        return out

    # lower / upper / tieredUpper (:294-343)
    @staticmethod
    def _lower(key):
        text, inclusive = key
        if not text:
            return b""
        return text.encode() + (b"\x00" if inclusive else b"\x01")

    @staticmethod
    def _upper(key):
        text, inclusive = key
        if not text:
            return UNBOUNDED_UPPER
        return text.encode() + (b"\x01" if inclusive else b"\x00")

    @staticmethod
    def _tiered_upper(key):
        text, inclusive = key
        if text is None or not inclusive:
            return None
        return text.encode() + b"\x00"

    # getRangeBytes (:192-285)
    def get_range_bytes(self, ranges, tier):
        empty = (None, True)
        out = []
        for r in ranges:
            if tier:                                                     # getTieredRangeBytes (:224-263)
                if r.kind == "single":
                    out.append(ByteRange("single", self._lower(r.lower), None))
                elif r.kind == "bounded":
                    up = self._tiered_upper(r.upper)
                    out.append(ByteRange("lower", self._lower(r.lower), self._upper(r.upper)) if up is None else
                               ByteRange("bounded", self._lower(r.lower), up))
                elif r.kind == "lower":
                    out.append(ByteRange("lower", self._lower(r.lower), self._upper(empty)))
                elif r.kind == "upper":
                    up = self._tiered_upper(r.upper)
                    out.append(ByteRange("unbounded", self._lower(empty), self._upper(r.upper)) if up is None else
                               ByteRange("upper", self._lower(empty), up))
                else:
                    out.append(ByteRange("unbounded", self._lower(r.lower), self._upper(r.lower)))
            else:                                                        # getStandardRangeBytes (:265-285)
                if r.kind == "single":
                    out.append(ByteRange("bounded", self._lower(r.lower), self._upper(r.lower)))
                elif r.kind == "bounded":
                    out.append(ByteRange("bounded", self._lower(r.lower), self._upper(r.upper)))
                elif r.kind == "lower":
                    out.append(ByteRange("bounded", self._lower(r.lower), self._upper(empty)))
                elif r.kind == "upper":
                    out.append(ByteRange("bounded", self._lower(empty), self._upper(r.upper)))
                else:
                    out.append(ByteRange("bounded", self._lower(r.lower), self._upper(r.lower)))
        prefixes = self.prefixes()
        if not prefixes:
            return out
        return [ByteRange(b.kind, p + b.lower, None if b.upper is None else p + b.upper) for b in out for p in prefixes]


class DateIndexKeySpace:
    """DateIndexKeySpace as a tier (DateIndexKeySpace.scala:48-104): 8 ordered bytes of the dtg."""
    MIN_LOWER = -(1 << 63) + 1      # MinLowerBound: + 1 excludes null dates (:114-115)
    MAX_UPPER = (1 << 63) - 1

    # getRanges (:61-83); intervals: keyspace.Bounds in epoch ms, DISJOINT, or nothing
    def get_ranges(self, intervals):
        if isinstance(intervals, str) and intervals == DISJOINT:
            return []
        if not intervals:
            return [("unbounded", None, None)]
        out = []
        for b in intervals:
            if b.lower is not None and b.lower == b.upper and b.lower_inclusive and b.upper_inclusive:   # isEquals
                out.append(("single", int(b.lower), None))
                continue
            lo = self.MIN_LOWER if b.lower is None else int(b.lower) + (0 if b.lower_inclusive else 1)
            hi = self.MAX_UPPER if b.upper is None else int(b.upper) + (1 if b.upper_inclusive else 0)
            out.append(("bounded", lo, hi))
        return out

    # getRangeBytes (:85-104)
    def get_range_bytes(self, ranges, tier=True):
        out = []
        for kind, lo, hi in ranges:
            if kind == "bounded":
                out.append(ByteRange("bounded", _ordered_long(lo), _ordered_long(hi)))
            elif kind == "single":
                o = _ordered_long(lo)
                out.append(ByteRange("single", o, None) if tier else ByteRange("bounded", o, row_following_prefix(o)))
            else:
                out.append(ByteRange("unbounded", _ordered_long(self.MIN_LOWER),
                                     row_following_prefix(_ordered_long(self.MAX_UPPER))))
        return out


def _bin_z(b, z):
    return struct.pack(">HQ", int(b) & 0xffff, int(z) & _M64)       # ByteArrays.toBytes(bin, z)


def _bin_z_following(b, z):
    k = (((int(b) & 0xffff) << 64) | (int(z) & _M64)) + 1            # toBytesFollowingPrefix: incremented in place
    return (k & ((1 << 80) - 1)).to_bytes(10, "big")


def z3_tier_range_bytes(scan_ranges):
    """Z3IndexKeySpace.getRangeBytes without a shard (Z3IndexKeySpace.scala:196-213) over the tuples of
    keyspace.Z3IndexKeySpace.get_ranges: every one a BoundedByteRange."""
    out = []
    for kind, lo, hi in scan_ranges:
        if kind == "bounded":
            out.append(ByteRange("bounded", _bin_z(*lo), _bin_z_following(*hi)))
        elif kind == "lower":
            out.append(ByteRange("bounded", _bin_z(*lo), UNBOUNDED_UPPER))
        elif kind == "upper":
            out.append(ByteRange("bounded", UNBOUNDED_LOWER, _bin_z_following(*hi)))
        else:
            out.append(ByteRange("bounded", UNBOUNDED_LOWER, UNBOUNDED_UPPER))
    return out


def single_rows(byte_ranges):
    """The multiplier of the tier's getRanges: max(1, the single-row primary ranges) (GeoMesaFeatureIndex.scala:304)."""
    return max(1, sum(1 for b in byte_ranges if b.kind == "single"))


def combine_tiers(primary, tiers):
    """GeoMesaFeatureIndex.scala:308-356 for a tiered index: `primary` from get_range_bytes(.., tier=True);
    `tiers` the tier's byte ranges, or None without a secondary filter.  Returns bounded / single ranges."""
    if tiers is None or any(t.kind == "unbounded" for t in tiers):       # :310-319
        out = []
        for b in primary:
            if b.kind in ("bounded", "upper"):
                out.append(ByteRange("bounded", b.lower, b.upper + UNBOUNDED_UPPER))
            elif b.kind == "single":
                out.append(ByteRange("bounded", b.lower, b.lower + UNBOUNDED_UPPER))
            else:
                out.append(ByteRange("bounded", b.lower, b.upper))
        return out
    if not tiers:                                                        # disjoint secondary filter (:320-322)
        return []
    min_tier = min(t.lower for t in tiers)                               # ByteRange.min / max (:299-317)
    max_tier = max(t.lower if t.kind == "single" else t.upper for t in tiers)
    out = []
    for b in primary:
        if b.kind == "single":                                           # every tier range on the row (:328-333)
            for t in tiers:
                out.append(ByteRange("single", b.lower + t.lower, None) if t.kind == "single" else
                           ByteRange("bounded", b.lower + t.lower, b.lower + t.upper))
        elif b.kind == "bounded":                                        # min / max tier on the end points (:335-337)
            out.append(ByteRange("bounded", b.lower + min_tier, b.upper + max_tier))
        elif b.kind == "lower":
            out.append(ByteRange("bounded", b.lower + min_tier, b.upper))
        elif b.kind == "upper":
            out.append(ByteRange("bounded", b.lower, b.upper + max_tier))
        else:
            out.append(ByteRange("bounded", b.lower, b.upper))
    return out


class KeyLayout:
    """The fixed-length row-key prefix of one table, [shard?][hex text][0x00][tier], as one integer per row:
    shard, v, bin and t packed most significant first, so that integer order is the rows' byte order."""

    def __init__(self, digits, tier=None, sharded=False):
        if tier not in (None, "date", "z3"):
            raise NotImplementedError("the attribute index tiers built are z3, date and none; not %r" % (tier,))
        self.digits, self.tier, self.sharded = digits, tier, bool(sharded)
        self.t_bits = 64 if tier else 0
        self.b_bits = 16 if tier == "z3" else 0
        self.v_bits = 4 * digits
        self.s_bits = 8 if sharded else 0
        self.tier_len = (self.t_bits + self.b_bits) // 8
        self.length = (1 if sharded else 0) + digits + 1 + self.tier_len
        self.total = 1 << (self.s_bits + self.v_bits + self.b_bits + self.t_bits)

    def fields(self, k):
        t = k & ((1 << self.t_bits) - 1)
        k >>= self.t_bits
        b = k & ((1 << self.b_bits) - 1)
        k >>= self.b_bits
        return k >> self.v_bits, k & ((1 << self.v_bits) - 1), b, t

    def key_bytes(self, k):
        s, v, b, t = self.fields(k)
        tier = ((b << self.t_bits) | t).to_bytes(self.tier_len, "big")
        return (bytes([s]) if self.sharded else b"") + ("%0*x" % (self.digits, v)).encode() + b"\x00" + tier

    def ceil_key(self, bound):
        """The smallest row key whose bytes are >= bound (at most `length` bytes; shorter reads as zero padded);
        self.total when there is none."""
        tail = self.b_bits + self.t_bits
        bound = bytes(bound).ljust(self.length, b"\x00")
        s, pos = (bound[0], 1) if self.sharded else (0, 0)
        base = s << self.v_bits
        text = bound[pos:pos + self.digits]
        for i, c in enumerate(text):
            if c in b"0123456789abcdef":
                continue
            head = int(text[:i], 16) if i else 0
            larger = [d for d in b"0123456789abcdef" if d > c]
            if larger:     # the smallest digit past c, then zeros
                v = ((head << 4) | int(chr(min(larger)), 16)) << (4 * (self.digits - i - 1))
            else:          # no digit past c: the text before it moves on by one (a carry may reach the shard)
                v = (head + 1) << (4 * (self.digits - i))
            return (base + v) << tail
        v = int(text, 16)
        if bound[pos + self.digits] != 0:     # past the delimiter: the next value
            return (base + v + 1) << tail
        return ((base + v) << tail) + int.from_bytes(bound[pos + self.digits + 1:self.length], "big")

    def key_interval(self, lower, upper):
        """Rows r with lower <= r + id < upper by byte comparison (id: the non-empty feature id the store
        appends), as an inclusive interval of row keys, or None when empty.  An empty `upper` has no end.  A bound
        longer than the prefix depends on the id and is answered with the prefix that may hold such rows."""
        lo = self.ceil_key(lower[:self.length])
        if not upper:
            hi = self.total - 1
        elif len(upper) <= self.length:
            hi = self.ceil_key(upper) - 1
        else:
            head = upper[:self.length]
            hi = self.ceil_key(head)
            if hi >= self.total or self.key_bytes(hi) != head:
                hi -= 1
        hi = min(hi, self.total - 1)
        return (lo, hi) if lo <= hi else None


def attr_ranges(byte_ranges, layout):
    """Combined byte ranges (bounded / single) as gm_attr_range rows (numpy ATTR_RANGE_DTYPE), one per range
    and shard it covers.  Fields of a column the table lacks get 0 / all ones; the scan does not compare them."""
    rows = []
    below = layout.v_bits + layout.b_bits + layout.t_bits
    for br in byte_ranges:
        upper = row_following_prefix(br.lower) if br.kind == "single" else br.upper
        iv = layout.key_interval(br.lower, upper)
        if iv is None:
            continue
        for s in range(iv[0] >> below, (iv[1] >> below) + 1):
            lo, hi = max(iv[0], s << below), min(iv[1], ((s + 1) << below) - 1)
            _, v0, b0, t0 = layout.fields(lo)
            _, v1, b1, t1 = layout.fields(hi)
            if not layout.t_bits:
                t0, t1 = 0, _M64
            if not layout.b_bits:
                b0, b1 = 0, 0xffff
            rows.append((v0, v1, t0, t1, b0, b1, s, (0, 0, 0)))
    return np.array(rows, _lib.ATTR_RANGE_DTYPE) if rows else np.zeros(0, _lib.ATTR_RANGE_DTYPE)


_TIERS = {None: _lib.GM_ATTR_TIER_NONE, "date": _lib.GM_ATTR_TIER_DATE, "z3": _lib.GM_ATTR_TIER_Z3}
_SIGN = -(1 << 63)


def _during_of(intervals):
    """One interval as the full filter's exclusive (t_lo, t_hi) over epoch ms; None without intervals."""
    if not intervals:
        return None
    if len(intervals) > 1:
        raise NotImplementedError("the secondary filter takes one date interval")
    b = intervals[0]
    lo = _SIGN if b.lower is None else int(b.lower) - (1 if b.lower_inclusive else 0)
    hi = (1 << 63) - 1 if b.upper is None else int(b.upper) + (1 if b.upper_inclusive else 0)
    return lo, hi


class AttributeTable:
    """Sorted (shard?, v, tier) key columns of one GPU's slice of an attribute index table.

    values: the attribute column (n slots) of `binding`; validity: an Arrow validity bitmap (LSB bit order,
    slot 0 at bit validity_offset), None = no nulls.  A null slot writes no row.  x, y, t_ms: the features'
    point and dtg columns (n slots), the tier's input and the secondary filter's columns; a null date of the
    date tier is Long.MinValue in t_ms.  With the Z3 tier a point or date that fails Z3SFC.index raises as
    Z3Table.from_points does (lenient clamps).  Results are input rows."""

    def __init__(self, values, binding, validity=None, x=None, y=None, t_ms=None, tier="z3", shard=None, period="week",
                 validity_offset=0, shards=None, lenient=False):
        import torch
        from .curve import _dev_col
        if tier not in _TIERS:
            raise NotImplementedError("the attribute index tiers built are z3, date and none; not %r" % (tier,))
        self.binding, self.tier = binding, tier
        self.type, self.digits = binding_of(binding)
        self.ctx = _lib.context()
        lib, h = self.ctx.lib, self.ctx.handle
        dt, npdt = {_lib.GM_ATTR_INT32: (torch.int32, np.int32), _lib.GM_ATTR_INT64: (torch.int64, np.int64),
                    _lib.GM_ATTR_FLOAT32: (torch.float32, np.float32),
                    _lib.GM_ATTR_FLOAT64: (torch.float64, np.float64)}[self.type]
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(values, torch.Tensor):
            values = torch.from_numpy(np.array(values, npdt))
        self.values = values.to(dev, dt).contiguous()
        self.n_slots = n = self.values.numel()
        self.x = None if x is None else _dev_col(x, torch.float64)
        self.y = None if y is None else _dev_col(y, torch.float64)
        self.t_ms = None if t_ms is None else _dev_col(t_ms, torch.int64)
        if tier == "z3" and (self.x is None or self.y is None or self.t_ms is None):
            raise ValueError("the z3 tier needs x, y and t_ms")
        if tier == "date" and self.t_ms is None:
            raise ValueError("the date tier needs t_ms")
        vbits = None
        if validity is not None:
            vbits = torch.as_tensor(np.ascontiguousarray(validity, np.uint8)).to(dev)
        col = _lib.AttrColumn(self.type, 0, self.values.data_ptr() if n else None, None,
                              vbits.data_ptr() if vbits is not None else None, int(validity_offset))
        v = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        rows = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        m = ctypes.c_int64()
        check(lib.gm_attr_index_key(h, ctypes.byref(col), n, ptr(v), ptr(rows), ctypes.byref(m)), "gm_attr_index_key")
        self.n = m = m.value
        v, rows = v[:m], rows[:m]
        sh_in = None
        self.shards = 0
        if shard is not None:
            sh = torch.as_tensor(np.asarray(shard, np.uint8) if not isinstance(shard, torch.Tensor) else shard,
                                 dtype=torch.uint8).to(dev)
            self.shards = int(shards) if shards else (int(sh.max().item()) + 1 if n else 1)
            sh_in = sh[rows].contiguous()
        b_in = t_in = None
        if tier == "z3":
            self.z3 = Z3IndexKeySpace(period)
            bins, z = self.z3.sfc.index_keys(self.x, self.y, self.t_ms, lenient=lenient)   # raises on a bad row
            b_in, t_in = bins[rows].contiguous(), z[rows].contiguous()
        elif tier == "date":
            t_in = (self.t_ms[rows] ^ _SIGN).contiguous()      # the ordered long: unsigned order = date order
        self.ks = AttributeIndexKeySpace(binding, self.shards)
        self.layout = KeyLayout(self.digits, tier, shard is not None)
        new = lambda a: None if a is None else torch.empty_like(a)
        self.shard, self.v, self.bin, self.t = new(sh_in), torch.empty_like(v), new(b_in), new(t_in)
        perm = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        check(lib.gm_attr_sort(h, ptr(sh_in), ptr(v), ptr(b_in), ptr(t_in), m, ptr(self.shard), ptr(self.v),
                               ptr(self.bin), ptr(self.t), ptr(perm)), "gm_attr_sort")
        self.perm = rows[perm[:m]].contiguous()       # table row -> input row (slot)

    def key_bytes(self):
        """The table's row-key prefixes in table order, (n, key_len) uint8 (gm_attr_key_bytes)."""
        import torch
        out = torch.empty((self.n, self.layout.length), dtype=torch.uint8, device=self.v.device)
        t = self.t if self.tier != "date" else self.t ^ _SIGN      # back to epoch ms
        check(self.ctx.lib.gm_attr_key_bytes(self.ctx.handle, self.type, ptr(self.shard), ptr(self.v), _TIERS[self.tier],
                                             ptr(self.bin), ptr(t), self.n, ptr(out)), "gm_attr_key_bytes")
        return out

    def scan_filter(self, bboxes=None, intervals=None, map_rows=True):
        """The secondary filter as a ScanFilter over the point and dtg columns (None = no filter); the boxes
        array it points into comes back beside it and must outlive the call."""
        during = _during_of(intervals)
        if not bboxes and during is None:
            return None, None
        f = _lib.ScanFilter()
        boxes = None
        if bboxes:
            if self.x is None or self.y is None:
                raise ValueError("a bbox filter needs the x and y columns")
            boxes = np.ascontiguousarray(np.asarray(bboxes, np.float64).reshape(-1, 4))
            f.xmin = f.xmax = self.x.data_ptr()
            f.ymin = f.ymax = self.y.data_ptr()
            f.boxes, f.n_boxes = boxes.ctypes.data, len(boxes)
        if during is not None:
            if self.t_ms is None:
                raise ValueError("a date filter needs the t_ms column")
            f.during, f.t_ms, f.t_lo, f.t_hi = 1, self.t_ms.data_ptr(), during[0], during[1]
        if not map_rows:
            f.rows = self.perm.data_ptr()     # the columns are in input order whatever the ids are
        return f, boxes

    def table_scan(self, ranges, bboxes=None, intervals=None, map_rows=True, ids_cap=None):
        """gm_attr_table_scan over prepared gm_attr_range rows (numpy ATTR_RANGE_DTYPE): (ids, n_match,
        n_scanned); ids are input rows (map_rows) or table rows, in table order."""
        import torch
        if self.n == 0:      # no row was written: nothing to seek, and the filter's columns may be empty
            return torch.zeros(0, dtype=torch.int64, device=self.v.device), 0, 0
        arr = np.ascontiguousarray(ranges, _lib.ATTR_RANGE_DTYPE)
        flt, keep = self.scan_filter(bboxes, intervals, map_rows)
        cap = self.n if ids_cap is None else ids_cap
        ids = torch.empty(max(cap, 1), dtype=torch.int64, device=self.v.device)
        nm, ns = ctypes.c_int64(), ctypes.c_int64()
        rc = self.ctx.lib.gm_attr_table_scan(
            self.ctx.handle, ptr(self.shard), ptr(self.v), ptr(self.bin), ptr(self.t), self.n,
            arr.ctypes.data if len(arr) else None, len(arr), ctypes.byref(flt) if flt is not None else None,
            ptr(self.perm) if map_rows else None, ptr(ids), cap, ctypes.byref(nm), ctypes.byref(ns))
        del keep
        if rc != _lib.GM_E_CAPACITY:
            check(rc, "gm_attr_table_scan")
        return ids[:min(nm.value, cap)], nm.value, ns.value

    def plan(self, bounds, bboxes=None, intervals=None, target=2000):
        """The query's combined byte ranges (GeoMesaFeatureIndex.scala:298-356)."""
        primary = self.ks.get_range_bytes(self.ks.get_ranges(bounds), self.tier is not None)
        if self.tier is None:
            return primary
        if not bboxes and not intervals:
            return combine_tiers(primary, None)
        if self.tier == "date":
            d = DateIndexKeySpace()
            tiers = d.get_range_bytes(d.get_ranges(intervals), tier=True)
        else:
            values = self.z3.get_index_values(bboxes, intervals)
            sr = [] if values.disjoint else self.z3.get_ranges(values, multiplier=single_rows(primary), target=target)
            tiers = z3_tier_range_bytes(sr)
        return combine_tiers(primary, tiers)

    def query(self, bounds, bboxes=None, intervals=None, target=2000, map_rows=True):
        """`attr <bounds> AND bbox AND dtg <interval>` through the index: the value ranges with the tier's ranges
        on their end points, then the exact secondary filter (inclusive boxes on the point, the interval on the
        dtg) on every candidate.  bounds as AttributeIndexKeySpace.get_ranges takes them; bboxes: (xmin, ymin,
        xmax, ymax) tuples; intervals: keyspace.Bounds in epoch ms (keyspace.during / between).  Returns (ids,
        n_match, n_scanned) like the other tables."""
        return self.table_scan(attr_ranges(self.plan(bounds, bboxes, intervals, target), self.layout), bboxes, intervals,
                               map_rows)
