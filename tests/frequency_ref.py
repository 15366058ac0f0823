"""A numpy restatement of the Frequency / Z3Frequency stats, the reference of test_frequency_reference.py and
test_gpu_frequency.py.

CountMinSketch (geomesa-utils/.../clearspring/CountMinSketch.scala:48-73, 96-105, 118-135, 181-203), the key
rules and the mask of Frequency (geomesa-utils/.../stats/Frequency.scala:159-168, 284-306) and Z3Frequency's
toKey / observe (.../stats/Z3Frequency.scala:54-60, 104-115), in uint64 / int64 arithmetic that wraps as the
JVM's.  Curve keys and time bins come from the C oracle (z3_index_key_batch, z2_index_batch).  hash and
Math.round exist twice -- vectorised, and as scalar pure-Python forms over Python integers and exact
fractions -- so that the two check each other (test_frequency_reference.py).

The dense block and the three tallies are those of include/geomesa_hip.h: table[bin - bin_lo][i][bucket],
size[bin - bin_lo]; tally[0] rows the reference throws for (or with a NaN ordinate), tally[1] rows whose bin
lies outside the window, tally[2] ids outside [0, n).
"""
import math
from fractions import Fraction

import numpy as np

from conftest import JavaRandom

SEED = -27                    # Frequency.Seed, Frequency.scala:213
PRIME = (1 << 31) - 1         # CountMinSketch.PrimeModulus, CountMinSketch.scala:179
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)


def to_long(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def shape(eps=0.005, confidence=0.95):
    """(depth, width), CountMinSketch.scala:186-187."""
    return int(math.ceil(-1 * math.log(1 - confidence) / math.log(2))), int(math.ceil(2 / eps))


def hash_a(depth, seed=SEED):
    """CountMinSketch.scala:197-200."""
    r = JavaRandom(seed)
    return [r.nextInt(INT_MAX) for _ in range(depth)]


def hash_scalar(item, a, width):
    """CountMinSketch.hash (CountMinSketch.scala:48-57) over Python integers."""
    h = to_long(a * item)
    h = to_long(h + (h >> 32))     # Python's >> of a negative int is arithmetic, as the JVM's
    h &= PRIME
    return h % width               # h.toInt is h (31 bits), non-negative: % is the Int remainder


def buckets(keys, hashes, width):
    """hash for every (hash row, key): int64 [depth, n]."""
    k = np.ascontiguousarray(keys, np.int64).view(np.uint64)
    out = np.empty((len(hashes), len(k)), np.int64)
    with np.errstate(over="ignore"):
        for i, a in enumerate(hashes):
            h = np.uint64(a) * k
            h = h + (h.view(np.int64) >> np.int64(32)).view(np.uint64)
            out[i] = (h & np.uint64(PRIME)).astype(np.int64) % width
    return out


def mask(precision):
    """Frequency.getMask (Frequency.scala:284-287); the JVM takes the shift count mod 64."""
    assert 0 <= precision <= 64
    return to_long(LONG_MAX << ((64 - precision) % 64))


def round_scalar(a, single=False):
    """Math.round of one float (float32 when single): exact rational floor(a + 1/2), NaN -> 0, saturating."""
    lo, hi = (INT_MIN, INT_MAX) if single else (LONG_MIN, LONG_MAX)
    a = float(np.float32(a)) if single else float(a)
    if math.isnan(a):
        return 0
    if math.isinf(a):
        return hi if a > 0 else lo
    return max(lo, min(hi, math.floor(Fraction(a) + Fraction(1, 2))))


def round_array(a):
    """Math.round over a float32 / float64 array, int64 out."""
    a = np.asarray(a)
    single = a.dtype == np.float32
    lo, hi = (INT_MIN, INT_MAX) if single else (LONG_MIN, LONG_MAX)
    out = np.zeros(a.shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(a)
        fin = np.isfinite(a) & (np.abs(f) < (2.0 ** 31 if single else 2.0 ** 63))
        out[fin] = f[fin].astype(np.int64) + ((a[fin] - f[fin]) >= 0.5)
        out[~fin & (a > 0)] = hi
        out[~fin & (a < 0)] = lo
    return out


def trunc_div(v, p):
    """Java integer division by p >= 1 (truncating toward zero) over an int64 array."""
    v = np.asarray(v, np.int64)
    q = v // np.int64(p)
    return q + ((v < 0) & (q * np.int64(p) != v))


def attr_keys(kind, values, precision):
    """Frequency.scala:302-306 by attribute class: int, long (and date), float, double."""
    if kind == "int":       # Int division, widened
        return trunc_div(np.asarray(values, np.int32).astype(np.int64), precision)
    if kind == "long":
        return trunc_div(values, precision)
    if kind == "float":     # Float * Int: the Int converts to Float
        with np.errstate(over="ignore", invalid="ignore"):
            return round_array(np.asarray(values, np.float32) * np.float32(precision))
    assert kind == "double"
    with np.errstate(over="ignore", invalid="ignore"):
        return round_array(np.asarray(values, np.float64) * np.float64(precision))


def valid_bits(bitmap, offset, n):
    """An Arrow validity bitmap (LSB first) as n booleans; None: all valid."""
    if bitmap is None:
        return np.ones(n, bool)
    bits = np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")
    return bits[offset:offset + n].astype(bool)


def time_bins(oracle, t_ms, period):
    """(bin, ok) per date: BinnedTime.timeToBinnedTime(period); not ok where its require fails."""
    t = np.ascontiguousarray(t_ms, np.int64)
    z = np.zeros(len(t))
    b, _, st = oracle.z3_index_key_batch(z, z, t, period=period)
    return b.astype(np.int64), st == 0


def selected(n, mask_words=None, ids=None):
    """(rows, bad ids): every row, the rows of the mask's first n bits, or ids with those outside [0, n) counted."""
    if ids is not None:
        ids = np.asarray(ids, np.int64)
        ok = (ids >= 0) & (ids < n)
        return ids[ok], int((~ok).sum())
    if mask_words is not None:
        bits = np.unpackbits(np.ascontiguousarray(mask_words, np.int64).view(np.uint8), bitorder="little")[:n]
        return np.flatnonzero(bits), 0
    return np.arange(n), 0


class Sketches:
    """The dense block of CountMinSketches over the time bins [bin_lo, bin_lo + n_bins)."""

    def __init__(self, depth=5, width=400, bin_lo=0, n_bins=1, hashes=None):
        self.depth, self.width, self.bin_lo, self.n_bins = depth, width, bin_lo, n_bins
        self.hashes = hash_a(depth) if hashes is None else list(hashes)
        self.table = np.zeros((n_bins, depth, width), np.int64)
        self.size = np.zeros(n_bins, np.int64)
        self.tally = np.zeros(3, np.int64)

    def add(self, bins, keys, ok, bad_ids=0):
        """add(key, 1) on bins[r]'s sketch for every row (CountMinSketch.scala:59-73); ok False: the
        reference throws for the row."""
        bins, keys, ok = np.asarray(bins, np.int64), np.asarray(keys, np.int64), np.asarray(ok, bool)
        self.tally[0] += int((~ok).sum())
        self.tally[2] += bad_ids
        rb = bins - self.bin_lo
        inside = ok & (rb >= 0) & (rb < self.n_bins)
        self.tally[1] += int((ok & ~inside).sum())
        rb, keys = rb[inside], keys[inside]
        bk = buckets(keys, self.hashes, self.width)
        for i in range(self.depth):
            np.add.at(self.table, (rb, i, bk[i]), 1)
        np.add.at(self.size, rb, 1)
        return self

    def estimate(self, keys, bins=None):
        """estimateCount (CountMinSketch.scala:96-105) per key: in bins[k]'s sketch (0 outside the window),
        or summed over every sketch (Frequency.scala:78)."""
        keys = np.atleast_1d(np.asarray(keys, np.int64))
        bk = buckets(keys, self.hashes, self.width)
        per_bin = self.table[:, np.arange(self.depth)[:, None], bk].min(axis=1)   # [n_bins, n]
        if bins is None:
            return per_bin.sum(axis=0)
        rb = np.asarray(bins, np.int64) - self.bin_lo
        inside = (rb >= 0) & (rb < self.n_bins)
        return np.where(inside, per_bin[np.clip(rb, 0, self.n_bins - 1), np.arange(len(keys))], 0)

    def merge(self, other):
        """+= (CountMinSketch.scala:118-135) bin by bin; both over the same window."""
        assert (self.depth, self.width, self.bin_lo, self.n_bins) == (other.depth, other.width, other.bin_lo, other.n_bins)
        self.table += other.table
        self.size += other.size
        return self

    # ------------------------------------------------------------------ the three scans
    def observe_z3(self, oracle, x, y, t_ms, period, precision, mask_words=None, ids=None):
        """Z3Frequency.observe (Z3Frequency.scala:104-115): a throwing toKey is logged and skipped."""
        rows, bad = selected(len(x), mask_words, ids)
        b, z, st = oracle.z3_index_key_batch(np.asarray(x)[rows], np.asarray(y)[rows], np.asarray(t_ms)[rows],
                                             period=period)
        return self.add(b, z & np.int64(mask(precision)), st == 0, bad)

    def _bins(self, oracle, rows, t_ms, t_valid, period):
        """Frequency.scala:162-165: bin 0 without dates or at a null date; not ok where timeToBin throws."""
        bins, ok = np.zeros(len(rows), np.int64), np.ones(len(rows), bool)
        if t_ms is not None:
            tb, tok = time_bins(oracle, np.asarray(t_ms)[rows], period)
            has = valid_bits(t_valid, 0, len(t_ms))[rows]
            bins, ok = np.where(has & tok, tb, 0), ~has | tok
        return bins, ok

    def observe_attr(self, oracle, kind, values, precision, t_ms=None, period=1, valid=None, t_valid=None,
                     mask_words=None, ids=None):
        """Frequency.observe (Frequency.scala:159-168): a null value is not observed."""
        rows, bad = selected(len(values), mask_words, ids)
        rows = rows[valid_bits(valid, 0, len(values))[rows]]
        bins, ok = self._bins(oracle, rows, t_ms, t_valid, period)
        return self.add(bins, attr_keys(kind, np.asarray(values)[rows], precision), ok, bad)

    def observe_points(self, oracle, x, y, precision, t_ms=None, period=1, t_valid=None, mask_words=None, ids=None):
        """Frequency.observe of a point attribute: geomToKey (Frequency.scala:289-293); Z2SFC.index throws
        outside the bounds (and fails for a NaN ordinate, the null rule of x / y columns)."""
        rows, bad = selected(len(x), mask_words, ids)
        bins, ok = self._bins(oracle, rows, t_ms, t_valid, period)
        z, st = oracle.z2_index_batch(np.asarray(x)[rows], np.asarray(y)[rows])
        return self.add(bins, z & np.int64(mask(precision)), ok & (st == 0), bad)


def enumerate_ranges(ranges, precision):
    """Frequency.enumerate (Frequency.scala:229-239) over (lower, upper) pairs."""
    shift = (64 - precision) % 64
    out = []
    for lower, upper in ranges:
        c = (upper >> shift) - (lower >> shift)
        out += [to_long(lower + (i << shift)) for i in range(c + 1)]
    return out
