"""The reference's BIN encoding, sorting and merging restated in Python / numpy, read line by line from

  geomesa-utils/.../bin/BinaryOutputCallback.scala:28-41       put: the 16-B / 24-B little-endian record
  geomesa-utils/.../bin/BinaryOutputEncoder.scala:149-168      convertToTrack, convertToDate, convertToLabel
  geomesa-utils/.../bin/BinaryOutputEncoder.scala:176-188      decode
  geomesa-utils/.../bin/BinaryOutputEncoder.scala:281-320      pointToXY / pointToYX, lineToXY / lineToYX, dateArray
  geomesa-utils/.../bin/BinaryOutputEncoder.scala:326-419      the six ToValues classes
  geomesa-index-api/.../utils/bin/BinSorter.scala:38-79        compare
  geomesa-index-api/.../utils/bin/BinSorter.scala:115-145      mergeSort(left, right)

with the JVM's value semantics written out: Long division truncates, toInt wraps, Double.toFloat is d2f,
Double.longValue saturates, String.hashCode runs over UTF-16 code units.  BinSorter.quickSort (:155) is not
restated: its output is defined only up to the order of equal seconds.  sort() is the stable order under
compare, which is one of the orders quickSort may produce and the one the library fixes.

A feature is a dict: id (str), track / label (attribute values or None), geom ((x, y) for a point, a list
of (x, y) for a line, None for null), dtg (epoch ms or None), dates (list of epoch ms, or None).  Attribute
values carry their Java class as a Python type: str = String, np.int32 = Integer, int / np.int64 = Long,
float / np.float64 = Double.

scan() adds the library's documented rule on top (include/geomesa_hip.h): a null geometry or a NaN ordinate
writes no record and is counted, where the reference throws or writes a NaN payload.
"""
import functools
import struct

import numpy as np

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1


def to_int(v):
    """Long.toInt / an int32 result of wrapping arithmetic: the low 32 bits, signed."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def to_long(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v


def long_div(a, b):
    """Java's Long division: truncates toward zero."""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def to_float(d):
    """Double.toFloat (d2f): round to nearest even, overflow to +-Inf, denormals and -0.0 kept."""
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(np.float64(d))


def string_hash(s):
    """String.hashCode: s[0] * 31^(n-1) + ... + s[n-1] over UTF-16 code units, in wrapping int32."""
    h = 0
    units = s.encode("utf-16-le", "surrogatepass")
    for k in range(0, len(units), 2):
        h = (31 * h + (units[k] | (units[k + 1] << 8))) & 0xFFFFFFFF
    return to_int(h)


def long_hash(v):
    """Long.hashCode: (int)(value ^ (value >>> 32))."""
    u = v & 0xFFFFFFFFFFFFFFFF
    return to_int(u ^ (u >> 32))


def double_hash(d):
    """Double.hashCode: Long.hashCode(doubleToLongBits(d)); doubleToLongBits makes every NaN canonical."""
    d = float(d)
    bits = 0x7FF8000000000000 if d != d else struct.unpack("<Q", struct.pack("<d", d))[0]
    return to_int(bits ^ (bits >> 32))


def double_to_long(d):
    """Double.longValue (d2l): NaN -> 0, saturating."""
    d = float(d)
    if d != d:
        return 0
    if d >= 9223372036854775808.0:
        return LONG_MAX
    if d <= -9223372036854775808.0:
        return LONG_MIN
    return int(d)


def convert_to_track(track):
    """convertToTrack (BinaryOutputEncoder.scala:150): null -> 0, else hashCode."""
    if track is None:
        return 0
    if isinstance(track, str):
        return string_hash(track)
    if isinstance(track, np.int32):
        return int(track)                      # Integer.hashCode
    if isinstance(track, (int, np.int64)):
        return long_hash(int(track))
    if isinstance(track, (float, np.float64)):
        return double_hash(track)
    raise TypeError(type(track))


def convert_to_date(date):
    """convertToDate (BinaryOutputEncoder.scala:154): null -> 0, else getTime."""
    return 0 if date is None else int(date)


def convert_to_label(label):
    """convertToLabel (BinaryOutputEncoder.scala:157-168)."""
    if label is None:
        return 0
    if isinstance(label, (np.int32, int, np.int64)):
        return int(label)                      # Number.longValue
    if isinstance(label, (float, np.float64)):
        return double_to_long(label)
    total, i = 0, 0
    for b in str(label).encode("utf-8", "surrogatepass")[:8]:
        total += (b & 0xFF) << (8 * i)
        i += 1
    return to_long(total)


def put(track_id, lat, lon, dtg, label=None):
    """ByteStreamCallback / put (BinaryOutputCallback.scala:28-41): trackId, (dtg / 1000).toInt, lat, lon
    [, label], little-endian."""
    out = struct.pack("<ii", to_int(track_id), to_int(long_div(dtg, 1000)))
    out += np.float32(lat).astype("<f4").tobytes() + np.float32(lon).astype("<f4").tobytes()
    if label is not None:
        out += struct.pack("<q", to_long(label))
    return out


class ByteStreamCallback:
    """Collects the records of a scan in one buffer, counting them (BinaryOutputCallback.scala)."""

    def __init__(self):
        self.chunks, self.result = [], 0

    def __call__(self, track_id, lat, lon, dtg, label=None):
        self.chunks.append(put(track_id, lat, lon, dtg, label))
        self.result += 1

    def bytes(self):
        return b"".join(self.chunks)


# pointToXY / pointToYX (BinaryOutputEncoder.scala:295-296): the (lat, lon) pair under each axis order
def point_to_xy(p):
    return to_float(p[0]), to_float(p[1])     # AxisOrder.LatLon


def point_to_yx(p):
    return to_float(p[1]), to_float(p[0])     # AxisOrder.LonLat


def line_to(point_fn):
    """lineToXY / lineToYX (BinaryOutputEncoder.scala:308-315)."""
    return lambda f: [point_fn(p) for p in f["geom"]]


def date_array(f):
    """dateArray (BinaryOutputEncoder.scala:317-320): a null list is empty."""
    return [] if f["dates"] is None else [int(d) for d in f["dates"]]


class ToValuesPoints:
    """BinaryOutputEncoder.scala:326-333."""

    def __init__(self, get_track_id, get_lat_lon):
        self.get_track_id, self.get_lat_lon = get_track_id, get_lat_lon

    def __call__(self, f, callback):
        lat, lon = self.get_lat_lon(f["geom"])
        callback(self.get_track_id(f), lat, lon, convert_to_date(f["dtg"]))


class ToValuesPointsLabels:
    """BinaryOutputEncoder.scala:335-343."""

    def __init__(self, get_track_id, get_lat_lon, get_label):
        self.get_track_id, self.get_lat_lon, self.get_label = get_track_id, get_lat_lon, get_label

    def __call__(self, f, callback):
        lat, lon = self.get_lat_lon(f["geom"])
        callback(self.get_track_id(f), lat, lon, convert_to_date(f["dtg"]), self.get_label(f))


class ToValuesLines:
    """BinaryOutputEncoder.scala:345-359."""

    def __init__(self, get_track_id, get_lat_lon):
        self.get_track_id, self.get_lat_lon = get_track_id, get_lat_lon

    def __call__(self, f, callback):
        track_id = self.get_track_id(f)
        points = self.get_lat_lon(f)
        date = convert_to_date(f["dtg"])
        i = 0
        while i < len(points):
            lat, lon = points[i]
            callback(track_id, lat, lon, date)
            i += 1


class ToValuesLinesLabels:
    """BinaryOutputEncoder.scala:361-377."""

    def __init__(self, get_track_id, get_lat_lon, get_label):
        self.get_track_id, self.get_lat_lon, self.get_label = get_track_id, get_lat_lon, get_label

    def __call__(self, f, callback):
        track_id = self.get_track_id(f)
        points = self.get_lat_lon(f)
        date = convert_to_date(f["dtg"])
        label = self.get_label(f)
        i = 0
        while i < len(points):
            lat, lon = points[i]
            callback(track_id, lat, lon, date, label)
            i += 1


class ToValuesLinesDates:
    """BinaryOutputEncoder.scala:379-397.  mismatched counts the warnings it logs."""

    def __init__(self, get_track_id, get_lat_lon):
        self.get_track_id, self.get_lat_lon = get_track_id, get_lat_lon
        self.mismatched = 0

    def __call__(self, f, callback):
        track_id = self.get_track_id(f)
        points = self.get_lat_lon(f)
        dates = date_array(f)
        if len(points) == len(dates):
            size = len(points)
        else:
            self.mismatched += 1
            size = min(len(points), len(dates))
        i = 0
        while i < size:
            lat, lon = points[i]
            callback(track_id, lat, lon, dates[i])
            i += 1


class ToValuesLinesDatesLabels:
    """BinaryOutputEncoder.scala:399-419."""

    def __init__(self, get_track_id, get_lat_lon, get_label):
        self.get_track_id, self.get_lat_lon, self.get_label = get_track_id, get_lat_lon, get_label
        self.mismatched = 0

    def __call__(self, f, callback):
        track_id = self.get_track_id(f)
        points = self.get_lat_lon(f)
        dates = date_array(f)
        if len(points) == len(dates):
            size = len(points)
        else:
            self.mismatched += 1
            size = min(len(points), len(dates))
        label = self.get_label(f)
        i = 0
        while i < size:
            lat, lon = points[i]
            callback(track_id, lat, lon, dates[i], label)
            i += 1


def to_values(line=False, date_list=False, track=True, label=False, lat_lon=False):
    """toValues (BinaryOutputEncoder.scala:208-293): the ToValues for an encoding.  track False: no track
    field, the feature id's hash (:247-250)."""
    get_track_id = (lambda f: convert_to_track(f["track"])) if track else (lambda f: string_hash(f["id"]))
    get_label = lambda f: convert_to_label(f["label"])   # noqa: E731
    point_fn = point_to_xy if lat_lon else point_to_yx
    if line:
        get = line_to(point_fn)
        if date_list:
            return ToValuesLinesDatesLabels(get_track_id, get, get_label) if label else \
                ToValuesLinesDates(get_track_id, get)
        return ToValuesLinesLabels(get_track_id, get, get_label) if label else ToValuesLines(get_track_id, get)
    return ToValuesPointsLabels(get_track_id, point_fn, get_label) if label else ToValuesPoints(get_track_id, point_fn)


def encode(features, **kw):
    """BinaryOutputEncoder.encode without sort (BinaryOutputEncoder.scala:70-74): the records, in order."""
    tv, cb = to_values(**kw), ByteStreamCallback()
    for f in features:
        tv(f, cb)
    return cb.bytes()


def scan(features, **kw):
    """encode under the library's rule for what the reference cannot encode: (bytes, tally) with tally[0]
    the records not written for a null geometry (one per feature) or a NaN ordinate (one per point or
    vertex), tally[2] the date-list mismatches of the features with a geometry."""
    tv, cb = to_values(**kw), ByteStreamCallback()
    skipped = [0]

    def keep(track_id, lat, lon, dtg, label=None):
        if np.isnan(lat) or np.isnan(lon):
            skipped[0] += 1
        else:
            cb(track_id, lat, lon, dtg, label)
    for f in features:
        if f["geom"] is None:
            skipped[0] += 1
        else:
            tv(f, keep)
    return cb.bytes(), [skipped[0], 0, getattr(tv, "mismatched", 0)]


def _signed(b):
    return b - 256 if b >= 128 else b


def compare(left, left_offset, right, right_offset):
    """BinSorter.compare (BinSorter.scala:38-79): the little-endian int at offset + 4, its top byte signed,
    the lower three unsigned."""
    lo, ro = left_offset + 4, right_offset + 4
    l3, r3 = _signed(left[lo + 3]), _signed(right[ro + 3])
    if l3 < r3:
        return -1
    elif l3 > r3:
        return 1
    l2, r2 = left[lo + 2] & 0xFF, right[ro + 2] & 0xFF
    if l2 < r2:
        return -1
    elif l2 > r2:
        return 1
    l1, r1 = left[lo + 1] & 0xFF, right[ro + 1] & 0xFF
    if l1 < r1:
        return -1
    elif l1 > r1:
        return 1
    l0, r0 = left[lo] & 0xFF, right[ro] & 0xFF
    if l0 == r0:
        return 0
    elif l0 < r0:
        return -1
    return 1


def merge_sort(left, right, bin_size):
    """BinSorter.mergeSort(left, right, binSize) (BinSorter.scala:115-145): takes from left on ties."""
    if len(left) == 0:
        return bytes(right)
    elif len(right) == 0:
        return bytes(left)
    result = bytearray(len(left) + len(right))
    left_index = right_index = result_index = 0
    while left_index < len(left) and right_index < len(right):
        if compare(left, left_index, right, right_index) > 0:
            result[result_index:result_index + bin_size] = right[right_index:right_index + bin_size]
            right_index += bin_size
        else:
            result[result_index:result_index + bin_size] = left[left_index:left_index + bin_size]
            left_index += bin_size
        result_index += bin_size
    while left_index < len(left):
        result[result_index:result_index + bin_size] = left[left_index:left_index + bin_size]
        left_index += bin_size
        result_index += bin_size
    while right_index < len(right):
        result[result_index:result_index + bin_size] = right[right_index:right_index + bin_size]
        right_index += bin_size
        result_index += bin_size
    return bytes(result)


def records(data, bin_size):
    data = bytes(data)
    return [data[k:k + bin_size] for k in range(0, len(data), bin_size)]


def sort(data, bin_size):
    """The stable order under compare: one of the orders BinSorter.quickSort may leave, the one with ties in
    their input order."""
    recs = records(data, bin_size)
    return b"".join(sorted(recs, key=functools.cmp_to_key(lambda a, b: compare(a, 0, b, 0))))


def is_sorted(data, bin_size):
    recs = records(data, bin_size)
    return all(compare(recs[k], 0, recs[k + 1], 0) <= 0 for k in range(len(recs) - 1))


def seconds(data, bin_size):
    """The signed int32 at offset 4 of every record."""
    raw = np.frombuffer(bytes(data), np.uint8).reshape(-1, bin_size)
    return raw[:, 4:8].copy().view("<i4").reshape(-1)


def stable_sort_np(data, bin_size):
    """numpy's stable argsort of the signed seconds, applied to the records."""
    raw = np.frombuffer(bytes(data), np.uint8).reshape(-1, bin_size)
    return raw[np.argsort(seconds(data, bin_size), kind="stable")].tobytes()


def decode(encoded):
    """BinaryOutputEncoder.decode (BinaryOutputEncoder.scala:176-199): (trackId, lat, lon, dtg ms, label),
    label -1 for a 16-B record."""
    track_id, secs, lat, lon = struct.unpack("<iiff", encoded[:16])
    label = struct.unpack("<q", encoded[16:24])[0] if len(encoded) > 16 else -1
    return track_id, lat, lon, secs * 1000, label
