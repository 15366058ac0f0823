"""Histogram and MinMax of an attribute, restated (include/geomesa_hip.h states the arithmetic).

Histogram twice:
  (a) RefHistogram: the reference's loop, one feature at a time, line for line -- BinnedArray.scala:185-350
      (Binning), Histogram.scala:74-106 (observe / unobserve), :123-154 (+=), :226-232 (expandBins),
      :238-253 (checkEndpoints / getActualBounds), :260-292 (copyInto);
  (b) route_observe: the kernel's route -- the records of the running extrema, vectorised counts per segment
      under the bounds that held there, the expansions replayed through (a)'s copyInto.
MinMax: minmax_ref (compareTo's order through the bit-key map), hash_long, hll_registers, hll_cardinality
(MinMax.scala:51-62, clearspring/HyperLogLog.scala:99-131, :168-178).

Values are Python ints for the whole-number bindings, Python floats for double, numpy float32 for float.
"""
import math
import struct

import numpy as np

WHOLE = ("int", "long", "date")
BINDINGS = WHOLE + ("float", "double")
DTYPE = {"int": np.int32, "long": np.int64, "date": np.int64, "float": np.float32, "double": np.float64}
_M64 = (1 << 64) - 1
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)


def wrap64(v):
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def fdiv(a, b):
    """IEEE a / b of Python floats."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sat(f, lo, hi):
    if f != f:
        return 0
    if f >= hi:
        return hi
    if f <= lo:
        return lo
    return int(f)


def d2i(f):
    return _sat(f, INT_MIN, INT_MAX)


def d2l(f):
    return _sat(f, LONG_MIN, LONG_MAX)


def _floor(f):
    return f if (f != f or math.isinf(f)) else float(math.floor(f))


def _ceil(f):
    return f if (f != f or math.isinf(f)) else float(math.ceil(f))


def jround(a):
    """Math.round(double)."""
    if a != a:
        return 0
    f = _floor(a)
    r = d2l(f)
    return r + 1 if (not math.isinf(a) and a - f >= 0.5 and r != LONG_MAX) else r


def native(binding, v):
    """A value as the binding's Python type."""
    if binding in WHOLE:
        return int(v)
    return np.float32(v) if binding == "float" else float(v)


class Binning:
    """BinnedArray.Binning for one binding (BinnedArray.scala:185-350)."""

    def __init__(self, binding, length, bounds):
        self.binding, self.length = binding, int(length)
        self.lo, self.hi = native(binding, bounds[0]), native(binding, bounds[1])
        if not self.lo < self.hi:
            raise ValueError("Upper bound must be greater than lower bound")
        with np.errstate(all="ignore"):
            if binding in WHOLE:
                self.bin_size = float(wrap64(self.hi - self.lo)) / self.length
            elif binding == "float":
                self.bin_size = (self.hi - self.lo) / np.float32(self.length)
            else:
                self.bin_size = (self.hi - self.lo) / float(self.length)

    @property
    def bounds(self):
        return self.lo, self.hi

    def _clamp(self, i):
        if i < 0 or i > self.length:
            return -1
        return self.length - 1 if i == self.length else i

    def index_of(self, v):
        if v < self.lo or v > self.hi:
            return -1
        if self.binding in WHOLE:
            return self._clamp(d2i(_floor(fdiv(float(wrap64(v - self.lo)), self.bin_size))))
        if self.binding == "float":
            with np.errstate(all="ignore"):
                q = (np.float32(v) - self.lo) / self.bin_size
            return self._clamp(d2i(_floor(float(q))))
        return self._clamp(d2i(_floor(fdiv(v - self.lo, self.bin_size))))

    def is_below(self, v):
        return bool(v < self.lo)

    def _check(self, i):
        if i < 0 or i > self.length:
            raise IndexError(i)

    def _from_long(self, v):
        if self.binding == "int":
            v &= 0xFFFFFFFF
            return v - (1 << 32) if v >> 31 else v
        return v

    def bin_bounds(self, i):
        self._check(i)
        bs = self.bin_size
        if self.binding in WHOLE:
            lo_l = wrap64(self.lo + d2l(_ceil(bs * i)))
            hi_l = max(lo_l, wrap64(self.lo + d2l(_floor(bs * (i + 1)))))
            lo = self.lo if lo_l <= self.lo else self._from_long(lo_l)
            hi = self.hi if hi_l >= self.hi else self._from_long(hi_l)
            return lo, hi
        with np.errstate(all="ignore"):
            if self.binding == "float":
                return self.lo + bs * np.float32(i), self.lo + bs * np.float32(i + 1)
            return self.lo + bs * i, self.lo + bs * (i + 1)

    def median_value(self, i):
        self._check(i)
        bs = self.bin_size
        if self.binding in WHOLE:
            v = wrap64(self.lo + jround(bs / 2 + bs * i))
            return self.hi if v > self.hi else self._from_long(v)
        with np.errstate(all="ignore"):
            if self.binding == "float":
                return self.lo + bs / np.float32(2) + bs * np.float32(i)
            return self.lo + bs / 2 + bs * i


def copy_into(to, to_counts, frm, frm_counts):
    """Histogram.copyInto (Histogram.scala:260-292) on (Binning, list) pairs; ValueError where its require
    fails."""
    def to_index(v):
        i = to.index_of(v)
        return i if i != -1 else (0 if to.is_below(v) else to.length - 1)

    for i in range(frm.length):
        count = frm_counts[i]
        if count > 0:
            mn, mx = frm.bin_bounds(i)
            lo, hi = to_index(mn), to_index(mx)
            if lo == hi:
                to_counts[lo] += count
            else:
                size = hi - lo + 1
                if not size > 0:
                    raise ValueError("Error calculating bounds")
                avg, rem = count // size, count % size
                for j in range(lo, hi + 1):
                    to_counts[j] += avg
                to_counts[lo + size // 2] += rem


def _cmp_key(binding, v):
    """compareTo's order as a sortable key."""
    return v if binding in WHOLE else order_key(float(v))


class RefHistogram:
    """(a): Histogram.scala, one feature at a time."""

    def __init__(self, binding, length, bounds):
        self.binding = binding
        self.bins = Binning(binding, length, bounds)
        self.counts = [0] * self.bins.length
        self.expansions = 0   # expandBins calls, the ones that threw included
        self.observed = 0     # non-null features seen

    @property
    def length(self):
        return self.bins.length

    @property
    def bounds(self):
        return self.bins.bounds

    def _one(self, value, sign):
        self.observed += 1
        value = native(self.binding, value)
        i = self.bins.index_of(value)
        if i == -1:
            self.expansions += 1
            try:
                bins, counts = self._expand(value)
            except ValueError:
                return   # logger.warn
            self.bins, self.counts = bins, counts
            i = self.bins.index_of(value)   # bins.add(value, +-1)
            if i != -1:
                self.counts[i] += sign
        else:
            self.counts[i] += sign

    def _expand(self, value):
        """expandBins (Histogram.scala:226-232)."""
        lo, hi = self.bins.bounds
        mn = value if _cmp_key(self.binding, value) < _cmp_key(self.binding, lo) else lo   # defaults.min(value, lo)
        mx = value if _cmp_key(self.binding, value) > _cmp_key(self.binding, hi) else hi
        bins = Binning(self.binding, self.length, (mn, mx))
        counts = [0] * bins.length
        copy_into(bins, counts, self.bins, self.counts)
        return bins, counts

    def observe(self, values, valid=None, sign=1):
        for k, v in enumerate(values):
            if valid is None or valid[k]:
                self._one(v, sign)
        return self

    def unobserve(self, values, valid=None):
        return self.observe(values, valid, -1)

    def is_empty(self):
        return all(c == 0 for c in self.counts)

    def _actual_bounds(self):
        nz = [i for i, c in enumerate(self.counts) if c != 0]
        min_index = nz[0] if nz else -1
        max_index = nz[-1] if nz else self.length
        mn = self.bins.lo if min_index <= 0 else self.bins.bin_bounds(min_index)[0]
        mx = self.bins.hi if max_index >= self.length - 1 else self.bins.bin_bounds(max_index)[1]
        return mn, mx

    def __iadd__(self, other):
        """+= (Histogram.scala:123-154)."""
        if self.length == other.length and self.bounds == other.bounds:
            self.counts = [a + b for a, b in zip(self.counts, other.counts)]
        elif other.is_empty():
            pass
        elif self.is_empty():
            self.bins = Binning(self.binding, other.length, other.bounds)
            self.counts = list(other.counts)
        else:
            lmn, lmx = self._actual_bounds()
            rmn, rmx = other._actual_bounds()
            key = lambda v: _cmp_key(self.binding, v)
            ends = (rmn if key(lmn) > key(rmn) else lmn, rmx if key(lmx) < key(rmx) else lmx)
            length = max(self.length, other.length)
            if ends != self.bounds or length != self.length:
                bins = Binning(self.binding, length, ends)
                counts = [0] * length
                copy_into(bins, counts, self.bins, self.counts)
                self.bins, self.counts = bins, counts
            copy_into(self.bins, self.counts, other.bins, other.counts)
        return self


# ---------------------------------------------------------------------- (b) the kernel's route
def index_of_array(bins, values):
    """Binning.index_of over a numpy column of the binding's dtype (int32 out), vectorised."""
    b, n = bins.binding, bins.length
    v = np.asarray(values)
    with np.errstate(all="ignore"):
        if b in WHOLE:
            v = v.astype(np.int64)
            out = (v < bins.lo) | (v > bins.hi)
            q = (v - np.int64(bins.lo)).astype(np.float64) / np.float64(bins.bin_size)   # wrapping subtract
        elif b == "float":
            out = (v < bins.lo) | (v > bins.hi)
            q = ((v - bins.lo) / bins.bin_size).astype(np.float64)
        else:
            out = (v < bins.lo) | (v > bins.hi)
            q = (v - np.float64(bins.lo)) / np.float64(bins.bin_size)
        f = np.floor(q)
        i = np.where(np.isnan(f), 0.0, np.clip(f, float(INT_MIN), float(INT_MAX))).astype(np.int64)
    i = np.where((i < 0) | (i > n), -1, np.where(i == n, n - 1, i))
    return np.where(out, -1, i).astype(np.int32)


def find_records(binding, length, bounds, values):
    """The units whose indexOf under the running bounds is -1: below the running minimum or above the running
    maximum of the bounds and everything before (primitive order; NaN never), and for a Long span that has
    wrapped whatever the binning itself refuses."""
    lo, hi = native(binding, bounds[0]), native(binding, bounds[1])
    rec = []
    for k, v in enumerate(values):
        v = native(binding, v)
        if v != v:
            continue
        hit = v < lo or v > hi
        if not hit and binding in WHOLE and wrap64(hi - lo) < 0:
            hit = Binning(binding, length, (lo, hi)).index_of(v) == -1
        if hit:
            rec.append(k)
            lo, hi = min(lo, v), max(hi, v)
    return rec


def route_observe(binding, length, bounds, counts, values, sign=1):
    """(b): (bounds, counts, expansions) after observing the non-null `values` in order."""
    values = np.asarray(values, DTYPE[binding])
    bins = Binning(binding, length, bounds)
    counts = list(counts)
    start, expansions = 0, 0
    while start < len(values):
        chunk = values[start:]
        rec = find_records(binding, length, bins.bounds, chunk.tolist() if binding != "float" else chunk)
        starts = [0] + rec + [len(chunk)]
        seg_bins, rows = [bins], []
        for r in rec:
            lo, hi = seg_bins[-1].bounds
            v = native(binding, chunk[r])
            seg_bins.append(Binning(binding, length, (min(lo, v), max(hi, v))))
        for s, b in enumerate(seg_bins):
            idx = index_of_array(b, chunk[starts[s]:starts[s + 1]])
            rows.append(np.bincount(idx[idx >= 0], minlength=length) * sign)
        counts = [c + int(x) for c, x in zip(counts, rows[0])]
        start += len(chunk)
        for s in range(1, len(seg_bins)):
            expansions += 1
            fresh = [0] * length
            try:
                copy_into(seg_bins[s], fresh, bins, counts)
            except ValueError:
                start = start - len(chunk) + rec[s - 1] + 1   # the feature is dropped; go on behind it
                break
            bins = seg_bins[s]
            counts = [c + int(x) for c, x in zip(fresh, rows[s])]
    return bins.bounds, counts, expansions


# ---------------------------------------------------------------------- MinMax
def order_key(v):
    """Double.compareTo's order as a signed 64-bit key of the double: NaN canonical, then
    bits ^ ((bits >> 63) & Long.MaxValue).  Its own inverse (key_value)."""
    if v != v:
        return 0x7FF8000000000000
    b = struct.unpack("<q", struct.pack("<d", v))[0]
    return b ^ ((b >> 63) & LONG_MAX)


def key_value(k):
    return struct.unpack("<d", struct.pack("<q", k ^ ((k >> 63) & LONG_MAX)))[0]


def minmax_start(binding):
    """(defaults.max, defaults.min) as slots (MinMax.scala:159-182)."""
    if binding == "int":
        return INT_MAX, INT_MIN
    if binding in WHOLE:
        return LONG_MAX, LONG_MIN
    big = float(np.finfo(np.float32).max) if binding == "float" else float(np.finfo(np.float64).max)
    return order_key(big), order_key(-big)


def minmax_ref(binding, values, valid=None, start=None):
    """The (min, max) slots after MinMax.observe of the non-null values, by compareTo."""
    mn, mx = start or minmax_start(binding)
    for k, v in enumerate(values):
        if valid is not None and not valid[k]:
            continue
        key = int(v) if binding in WHOLE else order_key(float(v))
        mn, mx = min(mn, key), max(mx, key)
    return mn, mx


def _i32(v):
    return v & 0xFFFFFFFF


def hash_long(key):
    """MurmurHash.hashLong as include/geomesa_hip.h defines it (parity unpinned), as an unsigned 32-bit value."""
    m = 0x5BD1E995
    k = _i32(_i32(key) * m)
    k ^= k >> 24
    h = _i32(k * m)
    k = _i32(_i32(key >> 32) * m)
    k ^= k >> 24
    h = _i32(h * m)
    h ^= _i32(k * m)
    h ^= h >> 13
    h = _i32(h * m)
    h ^= h >> 15
    return h


def hash_key(binding, v):
    """The Long the value hashes as: the sign-extended Integer, the Long, doubleToRawLongBits,
    floatToRawIntBits sign-extended."""
    if binding in ("int", "long"):
        return int(v)
    if binding == "double":
        return struct.unpack("<q", struct.pack("<d", float(v)))[0]
    if binding == "float":
        return struct.unpack("<i", np.float32(v).tobytes())[0]
    raise NotImplementedError("the cardinality of a %s attribute hashes toString" % binding)


def hll_registers(binding, values, valid=None, registers=None):
    """HyperLogLog(10).offer of the non-null values (HyperLogLog.scala:99-131): 1,024 registers."""
    reg = [0] * 1024 if registers is None else list(registers)
    for k, v in enumerate(values):
        if valid is not None and not valid[k]:
            continue
        h = hash_long(hash_key(binding, v))
        j = h >> 22
        w = _i32(h << 10) | 513
        r = (32 - w.bit_length()) + 1
        reg[j] = max(reg[j], r)
    return reg


def hll_cardinality(registers):
    """HyperLogLog.cardinality (HyperLogLog.scala:168-178)."""
    s, zeros = 0.0, 0.0
    for r in registers:
        s += 1.0 / (1 << r)
        if r == 0:
            zeros += 1
    estimate = ((0.7213 / (1 + 1.079 / 1024)) * 1024 * 1024) * (1 / s)
    if estimate <= (5.0 / 2.0) * 1024:
        return jround(1024 * math.log(1024 / zeros))
    return jround(estimate)
