"""Z3Histogram: the statistics caller of the Z3 curve.

Mirrors geomesa-utils/src/main/scala/org/locationtech/geomesa/utils/stats/Z3Histogram.scala
(observe / unobserve :101-128, toKey :80-86, count / directIndex / indexOf :63-72, +=  :145-160,
isEmpty / clear :169-171, splitByTime :95-99, toJsonObject :163-167) over batches of point features:
the per-feature work (BinnedTime + Z3SFC.index + LongBinning.directIndex + the increment) runs in
the gm_z3_histogram kernel; this class keeps the binMap as a dense device block of int64 counters
for a window of time bins [bin_lo, bin_lo + n_bins) plus a per-bin "present" flag (the map's key
set), and widens the window when a batch has features outside it.

Frequency and Z3Frequency, the two count-min stats (Frequency.scala, Z3Frequency.scala over
clearspring/CountMinSketch.scala), keep their map of sketches the same way: a dense device block
table[bin - bin_lo][i][bucket] and sizes[bin - bin_lo] that gm_z3_frequency / gm_frequency_attr /
gm_frequency_points add to and gm_cms_estimate reads (include/geomesa_hip.h states the arithmetic).
"""
import ctypes
import math

import numpy as np

from . import _lib
from ._lib import check, ptr
from .curve import BinnedTime, TimePeriod, Z2SFC, Z3SFC, _dev_col, _selection, _torch

_JSON_FMT = {TimePeriod.Day: "%05d", TimePeriod.Week: "%04d", TimePeriod.Month: "%03d", TimePeriod.Year: "%02d"}
_PERIOD_NAME = {TimePeriod.Day: "day", TimePeriod.Week: "week", TimePeriod.Month: "month", TimePeriod.Year: "year"}
MIN_Z, MAX_Z = 0, (1 << 63) - 1  # Z3Histogram.scala:53-54 for every period (see gm_stats.hip)


def long_binning_index(value, length, lo=MIN_Z, hi=MAX_Z):
    """LongBinning.directIndex (BinnedArray.scala:185-201), scalar host form."""
    if value < lo or value > hi:
        return -1
    bs = float(hi - lo) / length
    i = int(np.floor(float(value - lo) / bs))
    if i < 0 or i > length:
        return -1
    return length - 1 if i == length else i


class Z3Histogram:
    """Stat.Z3Histogram(geom, dtg, period, length) over point columns (x, y, epoch-ms t)."""

    def __init__(self, geom="geom", dtg="dtg", period=TimePeriod.Week, length=1024, device=None):
        self.geom, self.dtg, self.length = geom, dtg, int(length)
        self.period = TimePeriod.of(period)
        self.sfc = Z3SFC(self.period)
        self._device = device
        self.bin_lo = None
        self.n_bins = 0
        self.counts = None    # int64 [n_bins, length] on the device
        self.present = None   # uint8 [n_bins]
        self.skipped = 0      # features whose toKey threw (the Scala code logs a warning per feature)

    # ------------------------------------------------------------------ window management
    def _alloc(self, lo, n):
        torch = _torch()
        dev = torch.device("cuda", _lib.context(self._device).device)
        counts = torch.zeros((n, self.length), dtype=torch.int64, device=dev)
        present = torch.zeros(n, dtype=torch.uint8, device=dev)
        if self.counts is not None:
            off = self.bin_lo - lo
            counts[off:off + self.n_bins] = self.counts
            present[off:off + self.n_bins] = self.present
        self.bin_lo, self.n_bins, self.counts, self.present = lo, n, counts, present

    def _cover(self, t):
        """Widen the window to the valid time bins of batch t (BinnedTime per feature, invalid ones ignored)."""
        b, _, s = BinnedTime.time_to_binned_time(self.period, t, status=True)
        ok = s == 0
        if not bool(ok.any()):
            return
        lo, hi = int(b[ok].min()), int(b[ok].max())
        if self.counts is not None:
            lo, hi = min(lo, self.bin_lo), max(hi, self.bin_lo + self.n_bins - 1)
            if lo == self.bin_lo and hi == self.bin_lo + self.n_bins - 1:
                return
        self._alloc(lo, hi - lo + 1)

    def _run(self, x, y, t, unobserve, counts, present, tally):
        ctx = _lib.context(self._device)
        n = x.numel()
        check(ctx.lib.gm_z3_histogram(ctx.handle, ptr(x), ptr(y), ptr(t), n, self.period, self.length,
                                      int(unobserve), self.bin_lo, self.n_bins, ptr(present), ptr(counts),
                                      ptr(tally)), "gm_z3_histogram")

    def _apply(self, x, y, t_ms, unobserve):
        torch = _torch()
        x = _dev_col(x, torch.float64); y = _dev_col(y, torch.float64); t = _dev_col(t_ms, torch.int64)
        if x.numel() == 0:
            return
        if self.counts is None:
            if unobserve:
                return  # binMap is empty: nothing to take away
            self._cover(t)
            if self.counts is None:  # every feature failed BinnedTime
                self.skipped += x.numel()
                return
        tally = torch.zeros(2, dtype=torch.int64, device=x.device)
        if unobserve:
            # bins outside the window are absent from binMap: unobserve ignores them
            self._run(x, y, t, True, self.counts, self.present, tally)
            self.skipped += int(tally[0])
            return
        # straight into the binMap block: features of bins outside the window are left out and
        # counted in tally[1] (no per-batch scratch block)
        self._run(x, y, t, False, self.counts, self.present, tally)
        self.skipped += int(tally[0])
        if int(tally[1]) > 0:
            # widen to the batch's bins, then add only the features of the new rows: the rows below
            # and above the old window are contiguous row blocks of the dense counts
            lo0, hi0 = self.bin_lo, self.bin_lo + self.n_bins   # [lo0, hi0)
            self._cover(t)
            extra = torch.zeros(2, dtype=torch.int64, device=x.device)
            below, above = lo0 - self.bin_lo, self.bin_lo + self.n_bins - hi0
            if below > 0:
                self._run_rows(x, y, t, self.bin_lo, 0, below, extra)
            if above > 0:
                self._run_rows(x, y, t, hi0, hi0 - self.bin_lo, above, extra)

    def _run_rows(self, x, y, t, bin_lo, row0, rows, tally):
        ctx = _lib.context(self._device)
        check(ctx.lib.gm_z3_histogram(ctx.handle, ptr(x), ptr(y), ptr(t), x.numel(), self.period, self.length, 0,
                                      bin_lo, rows, ptr(self.present[row0:row0 + rows]),
                                      ptr(self.counts[row0:row0 + rows]), ptr(tally)), "gm_z3_histogram")

    # ------------------------------------------------------------------ Stat API
    def observe(self, x, y, t_ms):
        """Z3Histogram.observe for a batch of point features (Z3Histogram.scala:101-111)."""
        self._apply(x, y, t_ms, False)

    def unobserve(self, x, y, t_ms):
        """Z3Histogram.unobserve (Z3Histogram.scala:113-123): lenient toKey, present bins only."""
        self._apply(x, y, t_ms, True)

    def time_bins(self):
        if self.present is None:
            return []
        idx = np.nonzero(self.present.cpu().numpy())[0]
        return [int(i) + self.bin_lo for i in idx]

    def _row(self, time_bin):
        if self.present is None:
            return None
        r = time_bin - self.bin_lo
        if r < 0 or r >= self.n_bins or not int(self.present[r]):
            return None
        return r

    def count(self, time_bin, i):
        r = self._row(time_bin)
        return 0 if r is None else int(self.counts[r, i])

    def bins(self, time_bin):
        """BinnedArray.counts for one time bin (host int64 array) or None when absent."""
        r = self._row(time_bin)
        return None if r is None else self.counts[r].cpu().numpy()

    def direct_index(self, time_bin, z):
        return -1 if self._row(time_bin) is None else long_binning_index(int(z), self.length)

    def index_of(self, x, y, t_ms):
        """indexOf((geom, date)) (Z3Histogram.scala:67-70): non-lenient toKey, then directIndex."""
        b, z = self.sfc.index_keys([x], [y], [t_ms])
        return int(b[0]), self.direct_index(int(b[0]), int(z[0]))

    def median_value(self, time_bin, i):
        """medianValue (Z3Histogram.scala:72, BinnedArray.scala:205-211) -> (x, y, offset in the period)."""
        bs = float(MAX_Z - MIN_Z) / self.length
        v = MIN_Z + int(np.floor(bs / 2 + bs * i + 0.5))  # math.round
        v = min(v, MAX_Z)
        x, y, t = self.sfc.invert([v])
        return float(x[0]), float(y[0]), int(t[0])

    def is_empty(self):
        return self.counts is None or not bool((self.counts != 0).any())

    def clear(self):
        if self.counts is not None:
            self.counts.zero_()

    def __iadd__(self, other):
        """+= (Z3Histogram.scala:145-160): counts of shared bins add, new bins are copied in."""
        if self.length != other.length:
            raise NotImplementedError("Can only add z3 histograms with the same length")
        if other.counts is None:
            return self
        if self.counts is None:
            self._alloc(other.bin_lo, other.n_bins)
        lo = min(self.bin_lo, other.bin_lo)
        hi = max(self.bin_lo + self.n_bins, other.bin_lo + other.n_bins)
        if lo != self.bin_lo or hi != self.bin_lo + self.n_bins:
            self._alloc(lo, hi - lo)
        off = other.bin_lo - self.bin_lo
        self.counts[off:off + other.n_bins] += other.counts * other.present.unsqueeze(1).to(other.counts.dtype)
        self.present[off:off + other.n_bins] |= other.present
        return self

    def __add__(self, other):
        out = Z3Histogram(self.geom, self.dtg, self.period, self.length, self._device)
        out += self
        out += other
        return out

    def all_reduce(self, pg):
        """Merge this rank's histogram with every other rank's (`+=` over the process group, RCCL).
        The merged block comes back on this histogram's device whatever the backend's transport
        device (gloo reduces on the CPU)."""
        from .shard import merge_histograms
        c, p, lo = merge_histograms(pg, self.counts, self.present, self.bin_lo, self.length)
        if c is not None:
            torch = _torch()
            dev = torch.device("cuda", _lib.context(self._device).device)
            self.counts, self.present = c.to(dev).contiguous(), p.to(dev).contiguous()
            self.bin_lo, self.n_bins = lo, c.shape[0]
        return self

    def split_by_time(self):
        out = []
        for b in self.time_bins():
            h = Z3Histogram(self.geom, self.dtg, self.period, self.length, self._device)
            h._alloc(b, 1)
            h.counts[0] = self.counts[b - self.bin_lo]
            h.present[0] = 1
            out.append((b, h))
        return out

    def to_json_object(self):
        """toJsonObject (Z3Histogram.scala:163-167)."""
        name, fmt = _PERIOD_NAME[self.period], _JSON_FMT[self.period]
        return [{("%s-" + fmt) % (name, b): {"bins": [int(c) for c in self.bins(b)]}} for b in self.time_bins()]

    def is_equivalent(self, other):
        if not (self.period == other.period and self.length == other.length):
            return False
        if self.time_bins() != other.time_bins():
            return False
        return all(np.array_equal(self.bins(b), other.bins(b)) for b in self.time_bins())



# ---------------------------------------------------------------------- count-min sketches
FREQUENCY_SEED = -27   # Frequency.Seed (Frequency.scala:213)
DEFAULT_TIME_BIN = 0   # Frequency.DefaultTimeBin (Frequency.scala:216)
_I64 = (1 << 64) - 1


def _to_long(v):
    """A Python int as the JVM Long it wraps to."""
    v &= _I64
    return v - (1 << 64) if v >> 63 else v


def _java_next_ints(seed, bound, count):
    """`count` values of new java.util.Random(seed).nextInt(bound) for a bound that is no power of two (the
    48-bit LCG and the rejection loop of java.util.Random)."""
    assert bound > 0 and bound & (bound - 1)
    state = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)
    out = []
    while len(out) < count:
        state = (state * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        bits = state >> 17                       # next(31)
        val = bits % bound
        if bits - val + (bound - 1) < (1 << 31):
            out.append(val)
    return out


def cms_shape(eps=0.005, confidence=0.95):
    """(depth, width) of CountMinSketch(eps, confidence, seed) (CountMinSketch.scala:186-187).  Where
    -ln(1 - confidence) / ln 2 lands on an integer (confidence 0.5, 0.75, ...) the JVM's StrictMath-free
    Math.log against this platform's libm is parity-unpinned: a last-ulp difference moves the ceiling by
    one, so pass depth / width explicitly there."""
    width = int(math.ceil(2 / eps))
    depth = int(math.ceil(-1 * math.log(1 - confidence) / math.log(2)))
    return depth, width


def cms_hash_a(depth, seed=FREQUENCY_SEED):
    """hashA (CountMinSketch.scala:197-200): depth draws of Random(seed).nextInt(Int.MaxValue)."""
    return _java_next_ints(seed, 2147483647, depth)


def frequency_mask(precision):
    """Frequency.getMask (Frequency.scala:284-287): Long.MaxValue << (64 - precision), the shift count
    taken mod 64 as the JVM does (precision 0 and 64 both give Long.MaxValue)."""
    if not 0 <= precision <= 64:
        raise ValueError("Precision must be in the range [0, 64]")
    return _to_long(((1 << 63) - 1) << ((64 - precision) & 63))


def java_round(a):
    """Math.round over a float32 or float64 array: the closest int / long, ties toward +Infinity, NaN -> 0,
    saturating; int64 out."""
    a = np.asarray(a)
    lo, hi = (-(1 << 31), (1 << 31) - 1) if a.dtype == np.float32 else (-(1 << 63), (1 << 63) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(a)
        up = (a - f) >= a.dtype.type(0.5)          # exact; false for NaN, infinities and |a| past the mantissa
        big, small = f >= a.dtype.type(hi), f <= a.dtype.type(lo)   # hi rounds up to 2^31 / 2^63 as a float
        r = np.where(np.isnan(a) | big | small, 0, f).astype(np.int64)
    r = np.where(big, hi, np.where(small, lo, r))
    return np.where(np.isnan(a), 0, r + up).astype(np.int64)


def _trunc_div(v, p):
    """Java's integer division of an int64 array by p >= 1: truncating toward zero."""
    q = v // p
    return q + ((v < 0) & (q * p != v))


# the attribute bindings Frequency.add knows (Frequency.scala:241-260) -> GM_ATTR_* and the column dtype
_BINDINGS = {"int": (_lib.GM_ATTR_INT32, np.int32), "long": (_lib.GM_ATTR_INT64, np.int64),
             "date": (_lib.GM_ATTR_INT64, np.int64), "float": (_lib.GM_ATTR_FLOAT32, np.float32),
             "double": (_lib.GM_ATTR_FLOAT64, np.float64)}
_DTYPE_BINDING = {"int32": "int", "int64": "long", "float32": "float", "float64": "double"}
_STRING_WHY = ("Frequency over a String attribute is not implemented: its keys hash through "
               "com.clearspring's MurmurHash / Filter.getHashBuckets (CountMinSketch.scala:83), which the "
               "reference tree does not hold")


class _SketchMap:
    """What Frequency and Z3Frequency share: the dense block of sketches over a window of time bins, the
    widening of that window, merge, estimate and the Stat surface that does not depend on the key."""

    def _init_sketches(self, period, precision, eps, confidence, depth, width, device):
        self.period = TimePeriod.of(period)
        self.precision = int(precision)
        self.eps, self.confidence = float(eps), float(confidence)
        d, w = cms_shape(eps, confidence) if depth is None or width is None else (depth, width)
        self.depth = int(d if depth is None else depth)
        self.width = int(w if width is None else width)
        if not 1 <= self.depth <= _lib.GM_CMS_MAX_DEPTH or self.width < 1:
            raise ValueError("depth must be within 1..%d and width at least 1" % _lib.GM_CMS_MAX_DEPTH)
        self.hash_a = cms_hash_a(self.depth)
        self._device = device
        self.bin_lo, self.n_bins = None, 0
        self.table = None    # int64 [n_bins, depth, width] on the device
        self.sizes = None    # int64 [n_bins]
        self.skipped = 0     # rows the reference throws for (tally[0])
        self.bad_ids = 0     # ids outside [0, n) (tally[2])

    def _new(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ window management
    def _dev(self):
        return _torch().device("cuda", _lib.context(self._device).device)

    def _cms(self, lo=None, n=None):
        c = _lib.Cms(self.depth, self.width, self.bin_lo if lo is None else lo, self.n_bins if n is None else n, 0, 0)
        for i, a in enumerate(self.hash_a):
            c.hash_a[i] = a
        return c

    def _alloc(self, lo, n):
        torch = _torch()
        table = torch.zeros((n, self.depth, self.width), dtype=torch.int64, device=self._dev())
        sizes = torch.zeros(n, dtype=torch.int64, device=self._dev())
        if self.table is not None:
            off = self.bin_lo - lo
            table[off:off + self.n_bins] = self.table
            sizes[off:off + self.n_bins] = self.sizes
        self.bin_lo, self.n_bins, self.table, self.sizes = lo, n, table, sizes

    def _widen(self, lo, hi):
        """The window grown to hold the bins lo .. hi."""
        if self.table is not None:
            lo, hi = min(lo, self.bin_lo), max(hi, self.bin_lo + self.n_bins - 1)
            if lo == self.bin_lo and hi == self.bin_lo + self.n_bins - 1:
                return
        self._alloc(lo, hi - lo + 1)

    def _batch_bins(self, t):
        """(lowest, highest) valid time bin of the date column t (None: every row in the default bin); None
        when no date is valid."""
        if t is None:
            return DEFAULT_TIME_BIN, DEFAULT_TIME_BIN
        if t.numel():
            b, _, s = BinnedTime.time_to_binned_time(self.period, t, status=True)
            ok = s == 0
            if bool(ok.any()):
                return int(b[ok].min()), int(b[ok].max())
        return None

    def _observe(self, call, bins):
        """Runs one batch: call(cms, table, sizes, tally) is the entry point over a block of the window's
        bins; bins() the batch's (lowest, highest) bin.  Rows outside the window come back in tally[1]:
        the window widens and only the bins it gained are run again, as Z3Histogram._apply does."""
        torch = _torch()
        if self.table is None:
            w = bins() or (DEFAULT_TIME_BIN, DEFAULT_TIME_BIN)
            self._alloc(w[0], w[1] - w[0] + 1)
        tally = torch.zeros(3, dtype=torch.int64, device=self._dev())
        call(self._cms(), self.table, self.sizes, tally)
        t = tally.cpu().tolist()
        self.skipped += int(t[0])
        self.bad_ids += int(t[2])
        if t[1] > 0:
            lo0, hi0 = self.bin_lo, self.bin_lo + self.n_bins   # [lo0, hi0)
            self._widen(*bins())
            extra = torch.zeros(3, dtype=torch.int64, device=self._dev())   # the same rows: counted already
            below, above = lo0 - self.bin_lo, self.bin_lo + self.n_bins - hi0
            if below > 0:
                call(self._cms(self.bin_lo, below), self.table[:below], self.sizes[:below], extra)
            if above > 0:
                r0 = hi0 - self.bin_lo
                call(self._cms(hi0, above), self.table[r0:], self.sizes[r0:], extra)

    def _estimate(self, keys, bins=None):
        """estimateCount of int64 keys (device or host) in the sketches of `bins` (int16, per key), or summed
        over every sketch; int64 device tensor."""
        torch = _torch()
        keys = _dev_col(keys, torch.int64, self._dev())
        out = torch.zeros(keys.numel(), dtype=torch.int64, device=keys.device)
        if self.table is None or keys.numel() == 0:
            return out
        if bins is not None:
            bins = _dev_col(bins, torch.int16, self._dev())
        ctx = _lib.context(self._device)
        c = self._cms()
        check(ctx.lib.gm_cms_estimate(ctx.handle, ctypes.byref(c), ptr(self.table), ptr(keys), ptr(bins),
                                      keys.numel(), ptr(out)), "gm_cms_estimate")
        return out

    def _counts(self, keys, time_bin, scalar):
        """The estimates of host int64 keys, in one time bin or over all; an int for a scalar query."""
        keys = np.atleast_1d(np.asarray(keys, np.int64))
        bins = None if time_bin is None else np.full(keys.shape, time_bin, np.int16)
        out = self._estimate(keys, bins).cpu().numpy()
        return int(out[0]) if scalar else out

    # ------------------------------------------------------------------ Stat API
    @property
    def size(self):
        """Number of observations (Frequency.scala:136, Z3Frequency.scala:88)."""
        return 0 if self.sizes is None else int(self.sizes.sum())

    def size_of(self, time_bin):
        """size(timeBin) (Frequency.scala:143)."""
        r = None if self.sizes is None else time_bin - self.bin_lo
        return 0 if r is None or not 0 <= r < self.n_bins else int(self.sizes[r])

    def time_bins(self):
        """The time bins with size > 0, ascending.  The reference's key set can also hold cleared sketches,
        which serialisation drops (StatSerializer.scala:487-507)."""
        if self.sizes is None:
            return []
        return [int(i) + self.bin_lo for i in np.nonzero(self.sizes.cpu().numpy())[0]]

    def split_by_time(self):
        """splitByTime (Frequency.scala:151-157, Z3Frequency.scala:96-102)."""
        out = []
        for b in self.time_bins():
            f = self._new()
            f._alloc(b, 1)
            f.table[0] = self.table[b - self.bin_lo]
            f.sizes[0] = self.sizes[b - self.bin_lo]
            out.append((b, f))
        return out

    def is_empty(self):
        return self.sizes is None or not bool((self.sizes != 0).any())

    def clear(self):
        if self.table is not None:
            self.table.zero_()
            self.sizes.zero_()

    def __iadd__(self, other):
        """+= (Frequency.scala:180-187, Z3Frequency.scala:127-131): tables and sizes add bin by bin
        (CountMinSketch.scala:118-135, which throws for sketches of different sizes)."""
        if (self.depth, self.width) != (other.depth, other.width):
            raise ValueError("Can't merge CountMinSketch of different sizes")
        if other.table is None:
            return self
        self._widen(other.bin_lo, other.bin_lo + other.n_bins - 1)
        off = other.bin_lo - self.bin_lo
        self.table[off:off + other.n_bins] += other.table.to(self.table.device)
        self.sizes[off:off + other.n_bins] += other.sizes.to(self.sizes.device)
        return self

    def __add__(self, other):
        out = self._new()
        out += self
        out += other
        return out

    def all_reduce(self, pg):
        """`+=` with every other rank's stat over the process group (RCCL; gloo reduces on the CPU): each
        bin travels as one row of shard.merge_histograms, its table flattened and its size last.  The merged
        block comes back on this stat's device."""
        from .shard import merge_histograms
        torch = _torch()
        counts = present = None
        if self.table is not None:
            counts = torch.cat([self.table.reshape(self.n_bins, -1), self.sizes.reshape(-1, 1)], 1)
            present = (self.sizes > 0).to(torch.uint8)
        c, _, lo = merge_histograms(pg, counts, present, self.bin_lo, self.depth * self.width + 1)
        if c is not None:
            c = c.to(self._dev())
            self.bin_lo, self.n_bins = lo, c.shape[0]
            self.table = c[:, :-1].reshape(self.n_bins, self.depth, self.width).contiguous()
            self.sizes = c[:, -1].contiguous()
        return self

    def _same_sketches(self, other):
        if (self.depth, self.width, self.hash_a) != (other.depth, other.width, other.hash_a):
            return False
        bins = self.time_bins()
        if bins != other.time_bins():
            return False
        return all(self.size_of(b) == other.size_of(b) and
                   bool((self.table[b - self.bin_lo] == other.table[b - other.bin_lo].to(self.table.device)).all())
                   for b in bins)


class Frequency(_SketchMap):
    """Stat.Frequency(attribute, dtg, period, precision) (Frequency.scala:41-208) over attribute columns.

    binding names the attribute's class -- "int", "long", "date", "float", "double", "geometry" -- and decides
    the key (Frequency.scala:302-306); None takes it from the first observed column's dtype.  eps and
    confidence give the sketch's shape as CountMinSketch.apply does (see cms_shape for the confidences where
    that is parity-unpinned); depth / width override it.  .skipped counts the rows for which the reference's
    observe throws (an unindexable date, a point outside the curve): Frequency.observe has no try, so the
    reference's scan fails where this skips and counts.  .bad_ids counts ids outside [0, n)."""

    def __init__(self, attribute, precision, dtg=None, period=TimePeriod.Week, eps=0.005, confidence=0.95,
                 depth=None, width=None, binding=None, device=None):
        self.attribute, self.dtg = attribute, dtg
        if binding is not None:
            binding = binding.lower()
            if binding == "string":
                raise NotImplementedError(_STRING_WHY)
            if binding != "geometry" and binding not in _BINDINGS:
                raise ValueError("No CountMinSketch implementation for class binding %s" % binding)
        self.binding = binding
        self._init_sketches(period, precision, eps, confidence, depth, width, device)
        self._check_precision()

    def _check_precision(self):
        if self.binding == "geometry":
            frequency_mask(self.precision)
        elif self.binding in ("int", "long", "date") and self.precision < 1:
            raise ValueError("an integer attribute needs precision >= 1")

    def _new(self):
        return Frequency(self.attribute, self.precision, self.dtg, self.period, self.eps, self.confidence,
                         self.depth, self.width, self.binding, self._device)

    def _bind(self, binding):
        if self.binding is None:
            self.binding = binding
            self._check_precision()
        elif (self.binding == "geometry") != (binding == "geometry"):
            raise ValueError("a %s attribute cannot observe %s values" % (self.binding, binding))

    def _column(self, values):
        """The values as a device column of the binding's dtype."""
        torch = _torch()
        if not isinstance(values, torch.Tensor):
            values = np.asarray(values)
            if values.dtype.kind in "USO":
                raise NotImplementedError(_STRING_WHY)
        name = str(values.dtype).replace("torch.", "")
        self._bind(_DTYPE_BINDING.get(name) or ("long" if "int" in name else "double"))
        dt = _BINDINGS[self.binding][1]
        if isinstance(values, torch.Tensor):
            return values.to(self._dev()).to(getattr(torch, np.dtype(dt).name)).contiguous()
        return torch.from_numpy(np.ascontiguousarray(values, dt).copy()).to(self._dev())

    def _time(self, t_ms, n):
        """(date column, its gm_time_column), both None without a dtg: the dates are read only with one."""
        from .arrow import TimeColumnC
        if t_ms is None or self.dtg is None:
            return None, None
        t = _dev_col(t_ms, _torch().int64, self._dev())
        if t.numel() != n:
            raise ValueError("values and t_ms must have one entry per row")
        return t, TimeColumnC(t.data_ptr() if n else None, None, 0)

    def observe(self, values, t_ms=None, mask=None, ids=None):
        """Frequency.observe (Frequency.scala:159-168) for a batch of attribute values; t_ms: the dtg column
        (read only when the stat has a dtg).  mask / ids: the rows a scan or a table query kept, exactly as
        RenderingGrid.render takes them.  Columns with null slots go through gm_frequency_attr's validity
        bitmaps (include/geomesa_hip.h); this class takes plain columns."""
        v = self._column(values)
        n = v.numel()
        t, tc = self._time(t_ms, n)
        mask, ids, n_ids = _selection(n, mask, ids, self._dev())
        col = _lib.AttrColumn(_BINDINGS[self.binding][0], 0, v.data_ptr() if n else None, None, None, 0)
        ctx = _lib.context(self._device)

        def call(c, table, sizes, tally):
            check(ctx.lib.gm_frequency_attr(ctx.handle, ctypes.byref(col), ctypes.byref(tc) if tc else None, n,
                                            ptr(mask), ptr(ids), n_ids, self.period, self.precision, ctypes.byref(c),
                                            ptr(table), ptr(sizes), ptr(tally)), "gm_frequency_attr")
        self._observe(call, lambda: self._batch_bins(t))
        return self

    def observe_points(self, x, y, t_ms=None, mask=None, ids=None):
        """Frequency.observe of a point geometry attribute: the key is Z2SFC.index(x, y) & mask
        (Frequency.scala:289-293).  A NaN ordinate is the null rule of x / y columns and counts in .skipped."""
        torch = _torch()
        self._bind("geometry")
        x = _dev_col(x, torch.float64, self._dev())
        y = _dev_col(y, torch.float64, self._dev())
        n = x.numel()
        if y.numel() != n:
            raise ValueError("x and y must have one entry per row")
        t, tc = self._time(t_ms, n)
        mask, ids, n_ids = _selection(n, mask, ids, self._dev())
        ctx = _lib.context(self._device)

        def call(c, table, sizes, tally):
            check(ctx.lib.gm_frequency_points(ctx.handle, ptr(x), ptr(y), ctypes.byref(tc) if tc else None, n,
                                              ptr(mask), ptr(ids), n_ids, self.period, self.precision,
                                              ctypes.byref(c), ptr(table), ptr(sizes), ptr(tally)),
                  "gm_frequency_points")
        self._observe(call, lambda: self._batch_bins(t))
        return self

    def keys(self, values):
        """The Long keys of attribute values (Frequency.scala:289-306), host int64; a geometry value is an
        (x, y) pair or a pair of columns, and a point outside the curve raises as Z2SFC.index does."""
        if self.binding is None:
            raise ValueError("the attribute's binding is not known before the first observe")
        if self.binding == "geometry":
            x, y = values
            z = Z2SFC().index(np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64)))
            return z.cpu().numpy() & np.int64(frequency_mask(self.precision))
        v = np.atleast_1d(np.asarray(values, _BINDINGS[self.binding][1]))
        if self.binding == "int":
            return _trunc_div(v.astype(np.int64), self.precision)
        if self.binding in ("long", "date"):
            return _trunc_div(v, np.int64(self.precision))
        if self.binding == "float":
            return java_round(v * np.float32(self.precision))
        return java_round(v * np.float64(self.precision))

    def count(self, *args):
        """count(value) across all time bins, or count(time_bin, value) (Frequency.scala:78, :87)."""
        time_bin, value = (None,) + args if len(args) == 1 else args
        if self.table is None:
            return 0
        scalar = np.ndim(value[0] if self.binding == "geometry" else value) == 0
        return self._counts(self.keys(value), time_bin, scalar)

    def count_direct(self, *args):
        """countDirect(value: Long) / countDirect(time_bin, value: Long) (Frequency.scala:117-118, 128-129)."""
        time_bin, value = (None,) + args if len(args) == 1 else args
        if isinstance(value, str):
            raise NotImplementedError(_STRING_WHY)
        return self._counts(value, time_bin, np.ndim(value) == 0)

    def to_json_object(self):
        """toJsonObject (Frequency.scala:193)."""
        return {"epsilon": self.eps, "confidence": self.confidence, "size": self.size}

    def is_equivalent(self, other):
        """isEquivalent (Frequency.scala:195-207)."""
        return (isinstance(other, Frequency) and self.attribute == other.attribute and self.dtg == other.dtg and
                self.period == other.period and self.precision == other.precision and self._same_sketches(other))

    @staticmethod
    def enumerate(ranges, precision):
        """Frequency.enumerate (Frequency.scala:229-239): every key of the (lower, upper) ranges at
        `precision` bits, as a generator of Longs."""
        shift = (64 - precision) & 63
        for r in ranges:
            lower, upper = (r.lower, r.upper) if hasattr(r, "lower") else (r[0], r[1])
            c = (upper >> shift) - (lower >> shift)
            for i in range(c + 1):
                yield _to_long(lower + (i << shift))


class Z3Frequency(_SketchMap):
    """Stat.Z3Frequency(geom, dtg, period, precision) (Z3Frequency.scala:32-155) over point columns
    (x, y, epoch-ms t): per time bin a sketch of the Z3 keys cut to `precision` bits.  .skipped counts the
    features whose toKey throws (the Scala code logs a warning per feature)."""

    def __init__(self, geom="geom", dtg="dtg", period=TimePeriod.Week, precision=25, eps=0.005, confidence=0.95,
                 depth=None, width=None, device=None):
        self.geom, self.dtg = geom, dtg
        self._init_sketches(period, precision, eps, confidence, depth, width, device)
        self.mask = frequency_mask(self.precision)
        self.sfc = Z3SFC(self.period)

    def _new(self):
        return Z3Frequency(self.geom, self.dtg, self.period, self.precision, self.eps, self.confidence, self.depth,
                           self.width, self._device)

    def observe(self, x, y, t_ms, mask=None, ids=None):
        """Z3Frequency.observe (Z3Frequency.scala:104-115) for a batch of point features; mask / ids: the
        rows a scan or a table query kept."""
        torch = _torch()
        x = _dev_col(x, torch.float64, self._dev())
        y = _dev_col(y, torch.float64, self._dev())
        t = _dev_col(t_ms, torch.int64, self._dev())
        n = x.numel()
        if y.numel() != n or t.numel() != n:
            raise ValueError("x, y and t_ms must have one entry per row")
        mask, ids, n_ids = _selection(n, mask, ids, self._dev())
        ctx = _lib.context(self._device)

        def call(c, table, sizes, tally):
            check(ctx.lib.gm_z3_frequency(ctx.handle, ptr(x), ptr(y), ptr(t), n, ptr(mask), ptr(ids), n_ids,
                                          self.period, self.precision, ctypes.byref(c), ptr(table), ptr(sizes),
                                          ptr(tally)), "gm_z3_frequency")
        self._observe(call, lambda: self._batch_bins(t))
        return self

    def count(self, x, y, t_ms):
        """count(geom, dtg) (Z3Frequency.scala:69-72): non-lenient toKey, then countDirect."""
        scalar = np.ndim(x) == 0
        b, z = self.sfc.index_keys(np.atleast_1d(x), np.atleast_1d(y), np.atleast_1d(t_ms))
        out = self._estimate(z & self.mask, b).cpu().numpy()
        return int(out[0]) if scalar else out

    def count_direct(self, time_bin, z3):
        """countDirect(bin, z3) (Z3Frequency.scala:81)."""
        return self._counts(z3, time_bin, np.ndim(z3) == 0)

    def to_json_object(self):
        """toJsonObject (Z3Frequency.scala:137-140): eps and confidence of the first sketch, 0.0 without one."""
        e, c = (self.eps, self.confidence) if self.time_bins() else (0.0, 0.0)
        return {"eps": e, "confidence": c, "size": self.size}

    def is_equivalent(self, other):
        """isEquivalent (Z3Frequency.scala:142-154)."""
        return (isinstance(other, Z3Frequency) and self.geom == other.geom and self.dtg == other.dtg and
                self.period == other.period and self.precision == other.precision and self._same_sketches(other))


# ---------------------------------------------------------------------- Histogram, MinMax, Count
_NO_BINDING = ("%s over a %s attribute is not implemented: a String bins base-36 prefixes and a Geometry the Z2 "
               "key of its centroid, their expansion takes a component-wise minimum rather than an order on the "
               "binned value, and their cardinality hashes toString")
_LONG_MAX, _LONG_MIN = (1 << 63) - 1, -(1 << 63)


def _order_key(v):
    """Double.compareTo's order as a signed 64-bit key (include/geomesa_hip.h): its own inverse."""
    b = int(np.float64(v).view(np.int64)) if v == v else 0x7FF8000000000000
    return b ^ ((b >> 63) & _LONG_MAX)


def _key_value(k):
    return float(np.int64(k ^ ((k >> 63) & _LONG_MAX)).view(np.float64))


def _attr_binding(what, binding):
    if binding is None:
        return None
    binding = binding.lower()
    if binding in ("string", "geometry"):
        raise NotImplementedError(_NO_BINDING % (what, binding.capitalize()))
    if binding not in _BINDINGS:
        raise ValueError("no %s for class binding %s" % (what, binding))
    return binding


class _AttrStat:
    """What Histogram and MinMax share: the binding, the device and the column / selection plumbing."""

    def _init_attr(self, what, attribute, binding, device):
        self.attribute = attribute
        self.binding = _attr_binding(what, binding)
        self._what, self._device = what, device
        self.bad_ids = 0   # ids outside [0, n)

    def _dev(self):
        torch = _torch()
        if self._device == "cpu":   # a host-only stat: merges and reads, no observe
            return torch.device("cpu")
        return torch.device("cuda", _lib.context(self._device).device)

    def _column(self, values):
        """(values as a device column of the binding's dtype, its gm_attr_column)."""
        torch = _torch()
        if not isinstance(values, torch.Tensor):
            values = np.asarray(values)
            if values.dtype.kind in "USO":
                raise NotImplementedError(_NO_BINDING % (self._what, "String"))
        if self.binding is None:
            name = str(values.dtype).replace("torch.", "")
            self.binding = _DTYPE_BINDING.get(name) or ("long" if "int" in name else "double")
            self._bound()
        dt = _BINDINGS[self.binding][1]
        if isinstance(values, torch.Tensor):
            v = values.to(self._dev()).to(getattr(torch, np.dtype(dt).name)).contiguous()
        else:
            v = torch.from_numpy(np.ascontiguousarray(values, dt).copy()).to(self._dev())
        n = v.numel()
        return v, _lib.AttrColumn(_BINDINGS[self.binding][0], 0, v.data_ptr() if n else None, None, None, 0)

    def _bound(self):
        pass


class Histogram(_AttrStat):
    """Stat.Histogram(attribute, length, lower, upper) (Histogram.scala:35-178) over attribute columns of the
    bindings "int", "long", "date" (epoch ms), "float" and "double"; None takes the binding from the first
    observed column's dtype.  String and Geometry raise NotImplementedError.

    The result depends on the order of the rows, as the reference's does: observe takes them in ascending row
    order, or in the order of ids.  The counts live on the device; .expansions counts the expandBins calls,
    .bad_ids the ids outside [0, n).  device="cpu" gives a host-only stat for merging and reading."""

    def __init__(self, attribute, length, bounds, binding=None, device=None):
        self._init_attr("Histogram", attribute, binding, device)
        self._length, self._bounds0 = int(length), (bounds[0], bounds[1])
        self._state = None
        self.counts = None    # int64 [length]
        self.expansions = 0
        self.path = 0         # gm_histogram_attr's path: 0 automatic, 1 LDS counters, 2 device atomics
        if self._length < 1:
            raise ValueError("length must be at least 1")
        if self.binding is not None:
            self._bound()

    # ------------------------------------------------------------------ state
    def _bound(self):
        self._state = self._make_state(self._length, self._bounds0)
        self.counts = _torch().zeros(self._length, dtype=_torch().int64, device=self._dev())

    def _make_state(self, length, bounds):
        lo, hi = bounds
        if self.binding in ("int", "long", "date"):
            st = _lib.HistState(_BINDINGS[self.binding][0], length, int(lo), int(hi), 0.0, 0.0)
        else:
            dt = _BINDINGS[self.binding][1]
            st = _lib.HistState(_BINDINGS[self.binding][0], length, 0, 0, float(dt(lo)), float(dt(hi)))
        if not self._lo_hi(st)[0] < self._lo_hi(st)[1]:
            raise ValueError("Upper bound must be greater than lower bound: lower='%s' upper='%s'" % (lo, hi))
        return st

    def _lo_hi(self, st):
        if self.binding in ("int", "long", "date"):
            return int(st.lo), int(st.hi)
        return float(st.flo), float(st.fhi)

    def _need(self):
        if self._state is None:
            raise ValueError("the attribute's binding is not known before the first observe")
        return self._state

    def _new(self, length=None, bounds=None):
        return Histogram(self.attribute, length or self.length, bounds or self.bounds, self.binding, self._device)

    @property
    def length(self):
        return self._length if self._state is None else int(self._state.length)

    @property
    def bounds(self):
        return self._bounds0 if self._state is None else self._lo_hi(self._state)

    # ------------------------------------------------------------------ observe
    def _apply(self, values, mask, ids, sign):
        torch = _torch()
        v, col = self._column(values)
        n = v.numel()
        mask, ids, n_ids = _selection(n, mask, ids, self._dev())
        tally = torch.zeros(3, dtype=torch.int64, device=self._dev())
        ctx = _lib.context(self._device)
        check(ctx.lib.gm_histogram_attr(ctx.handle, ctypes.byref(col), n, ptr(mask), ptr(ids), n_ids, sign, self.path,
                                        ctypes.byref(self._state), ptr(self.counts), ptr(tally)), "gm_histogram_attr")
        t = tally.cpu().tolist()
        self.expansions += int(t[1])
        self.bad_ids += int(t[2])
        return self

    def observe(self, values, mask=None, ids=None):
        """Histogram.observe (Histogram.scala:74-89) for a batch of attribute values; mask / ids: the rows a scan
        or a table query kept, as Frequency.observe takes them."""
        return self._apply(values, mask, ids, 1)

    def unobserve(self, values, mask=None, ids=None):
        """Histogram.unobserve (Histogram.scala:91-106)."""
        return self._apply(values, mask, ids, -1)

    # ------------------------------------------------------------------ reads
    def _host_counts(self):
        return np.ascontiguousarray(self.counts.cpu().numpy())

    def count(self, i):
        return int(self.counts[i])

    def index_of(self, value):
        """indexOf (BinnedArray.scala:195-203, :293-299, :327-333); an int for a scalar, else an int32 array."""
        st = self._need()
        v = np.ascontiguousarray(np.atleast_1d(value), _BINDINGS[self.binding][1])
        out = np.zeros(v.size, np.int32)
        check(_lib.load().gm_hist_index_of(ctypes.byref(st), v.ctypes.data, v.size, out.ctypes.data), "gm_hist_index_of")
        return int(out[0]) if np.ndim(value) == 0 else out

    def direct_index(self, value):
        """directIndex(value: Long): the whole-number binnings' indexOf; -1 for float and double."""
        if self.binding in ("float", "double"):
            return -1
        return self.index_of(value)

    def bin_bounds(self, i):
        """bounds(i) (BinnedArray.scala:213-223, :308-313, :342-347)."""
        out = _lib.HistState()
        check(_lib.load().gm_hist_bin_bounds(ctypes.byref(self._need()), int(i), ctypes.byref(out)), "gm_hist_bin_bounds")
        return self._lo_hi(out)

    def median_value(self, i):
        """medianValue(i) (BinnedArray.scala:205-211, :301-306, :335-340)."""
        iv, fv = ctypes.c_int64(), ctypes.c_double()
        check(_lib.load().gm_hist_median(ctypes.byref(self._need()), int(i), ctypes.byref(iv), ctypes.byref(fv)),
              "gm_hist_median")
        return int(iv.value) if self.binding in ("int", "long", "date") else float(fv.value)

    def is_empty(self):
        return self.counts is None or not bool((self.counts != 0).any())

    def clear(self):
        if self.counts is not None:
            self.counts.zero_()

    # ------------------------------------------------------------------ merges
    def _same_shape(self, other):
        return self.length == other.length and self.bounds == other.bounds

    def _set(self, st, counts):
        self._state = st
        self.counts = _torch().from_numpy(np.ascontiguousarray(counts[:st.length], np.int64).copy()).to(self._dev())

    def _adopt(self, other):
        if self.binding is None:
            self.binding = other.binding
            self._bound()
        if other.binding != self.binding:
            raise ValueError("cannot add a %s histogram to a %s one" % (other.binding, self.binding))

    def __iadd__(self, other):
        """+= (Histogram.scala:123-154): equal shapes add bin by bin; otherwise the bounds become the union of
        the two actual bounds, the length the greater one, and both are copied in by copyInto."""
        if other._state is None:
            return self
        self._adopt(other)
        if self._same_shape(other):
            self.counts += other.counts.to(self.counts.device)
            return self
        a = self._host_counts()
        b = other._host_counts()
        a = np.concatenate([a, np.zeros(max(0, other.length - self.length), np.int64)])
        st = _lib.HistState.from_buffer_copy(self._state)
        check(_lib.load().gm_hist_merge(ctypes.byref(st), a.ctypes.data, ctypes.byref(other._state), b.ctypes.data),
              "gm_hist_merge")
        self._set(st, a)
        return self

    def __add__(self, other):
        out = self._new()
        out += self
        out += other
        return out

    def add_counts_from(self, other):
        """addCountsFrom (Histogram.scala:66-72): as += but this histogram keeps its bounds and length."""
        self._adopt(other)
        if self._same_shape(other):
            self.counts += other.counts.to(self.counts.device)
            return self
        a = self._host_counts()
        b = other._host_counts()
        check(_lib.load().gm_hist_copy_into(ctypes.byref(self._state), a.ctypes.data, ctypes.byref(other._state),
                                            b.ctypes.data), "gm_hist_copy_into")
        self._set(self._state, a)
        return self

    def all_reduce(self, pg):
        """`+=` with every other rank's histogram over the process group.  When every rank has the same bounds
        and length the counts add bin by bin (one all-reduce); otherwise the histograms are gathered and folded
        with += IN RANK ORDER, rank 0 first -- += is not associative, so the order is part of the result, and
        every rank computes the same one."""
        if pg is None:
            return self
        from .shard import _device_of
        torch = _torch()
        mine = (self.binding, self.length, self.bounds) if self._state is not None else None
        shapes = [None] * pg.get_world_size()
        pg.all_gather_object(shapes, mine)
        if all(s is not None and s == shapes[0] for s in shapes):
            c = self.counts.to(_device_of(pg)).contiguous()
            pg.all_reduce(c, op=pg.ReduceOp.SUM)
            self.counts = c.to(self._dev()).contiguous()
            return self
        parts = [None] * len(shapes)
        pg.all_gather_object(parts, None if mine is None else self._host_counts().tolist())
        total = None
        for s, c in zip(shapes, parts):
            if s is None:
                continue
            h = Histogram(self.attribute, s[1], s[2], s[0], self._device)
            h.counts = torch.tensor(c, dtype=torch.int64, device=self._dev())
            if total is None:
                total = h
            else:
                total += h
        if total is not None:
            self.binding, self._state, self.counts = total.binding, total._state, total.counts
        return self

    def to_json_object(self):
        """toJsonObject (Histogram.scala:156-166)."""
        lo, hi = self.bounds
        c = self._host_counts()
        bins = []
        for i in range(self.length):
            b = self.bin_bounds(i)
            bins.append({"index": i, "lower-bound": b[0], "upper-bound": b[1], "count": int(c[i])})
        return {"lower-bound": lo, "upper-bound": hi, "bins": bins}

    def is_equivalent(self, other):
        """isEquivalent (Histogram.scala:172-177)."""
        return (isinstance(other, Histogram) and self.attribute == other.attribute and self.bounds == other.bounds and
                np.array_equal(self._host_counts(), other._host_counts()))


class MinMax(_AttrStat):
    """Stat.MinMax(attribute) (MinMax.scala:29-114): the bounds by compareTo -- for float and double the total
    order with -0.0 < 0.0 and NaN above everything -- and a HyperLogLog(10) cardinality whose hash is the
    header's restated MurmurHash (parity unpinned).  The cardinality of a date attribute hashes Date.toString
    and raises NotImplementedError; its min and max work.  A NaN comes back as the canonical NaN."""

    def __init__(self, attribute, binding=None, device=None):
        self._init_attr("MinMax", attribute, binding, device)
        self._slots = None      # int64 [2] on the device: {minValue, maxValue} as order keys
        self.registers = None   # int32 [1024]
        if self.binding is not None:
            self._bound()

    def _defaults(self):
        """(defaults.max, defaults.min) as slots (MinMax.scala:159-182)."""
        if self.binding == "int":
            return (1 << 31) - 1, -(1 << 31)
        if self.binding in ("long", "date"):
            return _LONG_MAX, _LONG_MIN
        big = float(np.finfo(_BINDINGS[self.binding][1]).max)
        return _order_key(big), _order_key(-big)

    def _bound(self):
        torch = _torch()
        self._slots = torch.tensor(self._defaults(), dtype=torch.int64, device=self._dev())
        if self.binding != "date":
            self.registers = torch.zeros(1024, dtype=torch.int32, device=self._dev())

    def _new(self):
        return MinMax(self.attribute, self.binding, self._device)

    def observe(self, values, mask=None, ids=None):
        """MinMax.observe (MinMax.scala:51-62) for a batch of attribute values; stream-ordered."""
        torch = _torch()
        v, col = self._column(values)
        n = v.numel()
        mask, ids, n_ids = _selection(n, mask, ids, self._dev())
        tally = torch.zeros(3, dtype=torch.int64, device=self._dev())
        ctx = _lib.context(self._device)
        check(ctx.lib.gm_minmax_attr(ctx.handle, ctypes.byref(col), n, ptr(mask), ptr(ids), n_ids, ptr(self._slots),
                                     ptr(self.registers), ptr(tally)), "gm_minmax_attr")
        if ids is not None:
            self.bad_ids += int(tally[2])
        return self

    def unobserve(self, values, mask=None, ids=None):
        """MinMax.unobserve is a no-op (MinMax.scala:65)."""
        return self

    def _host_slots(self):
        return [int(s) for s in self._slots.cpu().tolist()]

    def _value(self, slot):
        if self.binding in ("int", "long", "date"):
            return slot
        v = _key_value(slot)
        return float(np.float32(v)) if self.binding == "float" else v

    def is_empty(self):
        """isEmpty: minValue == defaults.max, so a stat that saw only defaults.max reads as empty."""
        return self._slots is None or self._host_slots()[0] == self._defaults()[0]

    @property
    def min(self):
        s = self._host_slots()
        return self._value(s[1] if self.is_empty() else s[0])

    @property
    def max(self):
        s = self._host_slots()
        return self._value(s[0] if self.is_empty() else s[1])

    @property
    def bounds(self):
        return self.min, self.max

    @property
    def cardinality(self):
        """HyperLogLog.cardinality (HyperLogLog.scala:109-131) of the registers, on the host."""
        if self.binding == "date":
            raise NotImplementedError("the cardinality of a date attribute hashes Date.toString, which is not restated")
        if self.registers is None:
            return 0
        s, zeros = 0.0, 0.0
        for r in self.registers.cpu().tolist():
            s += 1.0 / (1 << r)
            if r == 0:
                zeros += 1
        estimate = ((0.7213 / (1 + 1.079 / 1024)) * 1024 * 1024) * (1 / s)
        if estimate <= (5.0 / 2.0) * 1024:
            return int(java_round(np.float64(1024 * math.log(1024 / zeros))))
        return int(java_round(np.float64(estimate)))

    @property
    def tuple(self):
        return self.min, self.max, self.cardinality

    def clear(self):
        if self._slots is not None:
            self._bound()

    def __iadd__(self, other):
        """+= (MinMax.scala:79-91)."""
        if other._slots is None or other.is_empty():
            return self
        if self.binding is None:
            self.binding = other.binding
            self._bound()
        torch = _torch()
        o = other._slots.to(self._slots.device)
        if self.is_empty():
            self._slots = o.clone()
        else:
            self._slots = torch.stack([torch.minimum(self._slots[0], o[0]), torch.maximum(self._slots[1], o[1])])
        if self.registers is not None and other.registers is not None:
            self.registers = torch.maximum(self.registers, other.registers.to(self.registers.device))
        return self

    def __add__(self, other):
        out = self._new()
        out += self
        out += other
        return out

    def all_reduce(self, pg):
        """min, max and the register-wise maximum over the process group: order-free.  An empty rank sends the
        defaults, which are the reductions' identities."""
        if pg is None:
            return self
        from .shard import _device_of
        if self._slots is None:
            raise ValueError("the attribute's binding is not known before the first observe")
        dev = _device_of(pg)
        s = self._slots.to(dev)
        mn, mx = s[0:1].clone(), s[1:2].clone()
        pg.all_reduce(mn, op=pg.ReduceOp.MIN)
        pg.all_reduce(mx, op=pg.ReduceOp.MAX)
        self._slots = _torch().cat([mn, mx]).to(self._dev())
        if self.registers is not None:
            r = self.registers.to(dev).contiguous()
            pg.all_reduce(r, op=pg.ReduceOp.MAX)
            self.registers = r.to(self._dev())
        return self

    def to_json_object(self):
        """toJsonObject (MinMax.scala:93-98): nulls and 0 when empty."""
        if self.is_empty():
            return {"min": None, "max": None, "cardinality": 0}
        s = self._host_slots()
        return {"min": self._value(s[0]), "max": self._value(s[1]),
                "cardinality": None if self.binding == "date" else self.cardinality}

    def is_equivalent(self, other):
        """isEquivalent (MinMax.scala:108-113)."""
        return (isinstance(other, MinMax) and self.attribute == other.attribute and self.binding == other.binding and
                self._slots is not None and other._slots is not None and self._host_slots() == other._host_slots() and
                (self.binding == "date" or self.cardinality == other.cardinality))


class Count:
    """Stat.Count() (CountStat.scala:18-46).  No kernel: every scan returns its match count, and observe takes
    that number (a scan's n_match, a tally's rows observed)."""

    def __init__(self, count=0):
        self.count = int(count)

    def observe(self, count=1):
        self.count += int(count)
        return self

    def unobserve(self, count=1):
        self.count -= int(count)
        return self

    def __iadd__(self, other):
        self.count += other.count
        return self

    def __add__(self, other):
        return Count(self.count + other.count)

    def all_reduce(self, pg):
        from .shard import all_reduce_scalar
        self.count = int(all_reduce_scalar(pg, self.count, op="sum"))
        return self

    def to_json_object(self):
        return {"count": self.count}

    def is_empty(self):
        return self.count == 0

    def clear(self):
        self.count = 0

    def is_equivalent(self, other):
        return isinstance(other, Count) and self.count == other.count


__all__ = ["Z3Histogram", "long_binning_index", "MIN_Z", "MAX_Z", "Frequency", "Z3Frequency", "cms_shape",
           "cms_hash_a", "frequency_mask", "java_round", "Histogram", "MinMax", "Count"]
