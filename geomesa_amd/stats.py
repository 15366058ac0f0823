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


__all__ = ["Z3Histogram", "long_binning_index", "MIN_Z", "MAX_Z", "Frequency", "Z3Frequency", "cms_shape",
           "cms_hash_a", "frequency_mask", "java_round"]
