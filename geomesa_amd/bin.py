"""The BIN track-record scan: features encoded as 16-B / 24-B records, sorted by date and merged.

Mirrors BinAggregatingScan (geomesa-index-api/.../iterators/BinAggregatingScan.scala:129-168) over batches of
point or line features: every feature the scan kept becomes little-endian records
(geomesa-utils/.../bin/BinaryOutputCallback.scala:28-41: int32 trackId, int32 seconds, float32 lat, float32
lon[, int64 label]) with the values of BinaryOutputEncoder (geomesa-utils/.../bin/BinaryOutputEncoder.scala:
convertToTrack :149-150, convertToDate :153-154, convertToLabel :156-168, the six ToValues classes :326-419),
in scan order or sorted by BinSorter.compare (geomesa-index-api/.../utils/bin/BinSorter.scala:38-79).  The
per-row work runs in the gm_bin_* kernels; there is no CPU fallback.  The contract, with the three tallies
(.skipped, .bad_ids, .mismatched), is stated in include/geomesa_hip.h.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr
from .curve import _dev_col, _selection

# a decoded record (BinaryOutputEncoder.EncodedValues, BinaryOutputEncoder.scala:107): dtg in ms, label -1
# for 16-B records
DECODED = np.dtype([("track", "<i4"), ("dtg", "<i8"), ("lat", "<f4"), ("lon", "<f4"), ("label", "<i8")])
RECORD16 = np.dtype([("track", "<i4"), ("secs", "<i4"), ("lat", "<f4"), ("lon", "<f4")])
RECORD24 = np.dtype([("track", "<i4"), ("secs", "<i4"), ("lat", "<f4"), ("lon", "<f4"), ("label", "<i8")])


def _utf8_column(strings):
    """(offsets, bytes, validity or None) of a sequence of str / None, as Arrow Utf8 lays them out."""
    enc = [b"" if s is None else s.encode("utf-8", "surrogatepass") for s in strings]
    off = np.zeros(len(enc) + 1, np.int32)
    np.cumsum([len(e) for e in enc], out=off[1:])
    valid = None
    if any(s is None for s in strings):
        valid = np.packbits(np.array([s is not None for s in strings], np.uint8), bitorder="little")
    return off, np.frombuffer(b"".join(enc), np.uint8), valid


class BinEncoder:
    """BinaryOutputEncoder + BinAggregatingScan over device columns; records come back as a uint8 device
    tensor of 16 B each, 24 B with label=True.

    encode / encode_arrow take every row, or the rows a scan or a table query kept:

        ids, _, _ = table.query(bboxes, intervals)          # Z3Table, Z2Table, XZ2Table, XZ3Table
        records = enc.encode(x, y, t_ms, track, ids=ids)    # table order: the reference's scan order
        mask, _, _ = filters.query_scan(x, y, t_ms, bbox=bbox, during=during)
        records = enc.encode(x, y, t_ms, track, mask=mask)  # ascending row

    (x, y, t_ms, track the columns the table was built from, in input order.)  track and label are plain
    int32 / int64 columns: track_of / label_of make them once per table from an attribute column
    (convertToTrack, convertToLabel); with no track attribute, hash the feature ids.  sort=True orders each
    batch by BinSorter.compare, stably; merge() combines sorted batches (of several ranks, say) as
    BinSorter.mergeSort does.  lat_lon=True is AxisOrder.LatLon.  .skipped, .bad_ids and .mismatched count
    records left out for a null geometry or a NaN ordinate, ids outside [0, n), and line slots whose date
    list and vertex counts differ (geomesa_hip.h)."""

    def __init__(self, label=False, sort=False, lat_lon=False, device=None):
        import torch
        self.label, self.sorted, self.lat_lon = bool(label), bool(sort), bool(lat_lon)
        self.record_bytes = 24 if self.label else 16
        self._device = device
        ctx = _lib.context(device)
        self._dev = torch.device("cuda", ctx.device)
        self._tally = torch.zeros(3, dtype=torch.int64, device=self._dev)

    # ------------------------------------------------------------------ attribute columns
    def _attr(self, column, want_label):
        import torch
        ctx = _lib.context(self._device)
        dev = self._dev
        valid = None
        if isinstance(column, (list, tuple)) and all(isinstance(s, (str, type(None))) for s in column):
            column = _utf8_column(column)
        if isinstance(column, tuple):
            off = _dev_col(column[0], torch.int32, dev)
            data = _dev_col(column[1], torch.uint8, dev)
            valid = _dev_col(column[2], torch.uint8, dev) if len(column) > 2 and column[2] is not None else None
            voff = int(column[3]) if len(column) > 3 else 0
            n = off.numel() - 1
            if data.numel() == 0:
                data = torch.zeros(1, dtype=torch.uint8, device=dev)
            c = _lib.AttrColumn(_lib.GM_ATTR_UTF8, 0, data.data_ptr(), off.data_ptr(),
                                valid.data_ptr() if valid is not None else None, voff)
        else:
            if not isinstance(column, torch.Tensor):
                column = np.ascontiguousarray(np.asarray(column))
                column = torch.from_numpy(column if column.flags.writeable else column.copy())
            if column.dtype == torch.int32:
                kind = _lib.GM_ATTR_INT32
            elif column.dtype == torch.int64:
                kind = _lib.GM_ATTR_INT64
            elif column.dtype == torch.float64:
                kind = _lib.GM_ATTR_FLOAT64
            else:
                raise ValueError("an attribute column is int32, int64, float64 or (offsets, bytes[, validity])")
            column = column.to(dev).contiguous()
            n = column.numel()
            c = _lib.AttrColumn(kind, 0, column.data_ptr(), None, None, 0)
        if want_label:
            out = torch.empty(n, dtype=torch.int64, device=dev)
            check(ctx.lib.gm_bin_label(ctx.handle, ctypes.byref(c), n, ptr(out)), "gm_bin_label")
        else:
            out = torch.empty(n, dtype=torch.int32, device=dev)
            check(ctx.lib.gm_bin_track(ctx.handle, ctypes.byref(c), n, ptr(out)), "gm_bin_track")
        return out

    def track_of(self, column):
        """convertToTrack over an attribute column -> int32 device column.  column: a numpy / torch int32,
        int64 or float64 column, strings as Arrow Utf8 (offsets, bytes[, validity bitmap]), or a list of
        str / None."""
        return self._attr(column, False)

    def label_of(self, column):
        """convertToLabel over an attribute column -> int64 device column (columns as track_of)."""
        return self._attr(column, True)

    # ------------------------------------------------------------------ encode
    def _opts(self):
        return _lib.BinOpts(int(self.sorted), int(self.lat_lon))

    def _columns(self, n, track, label):
        import torch
        track = _dev_col(track, torch.int32, self._dev)
        if track is None or track.numel() != n:
            raise ValueError("track must have one entry per row (track_of hashes an attribute or id column)")
        if self.label != (label is not None):
            raise ValueError("a label column goes with BinEncoder(label=True), and only with it")
        label = _dev_col(label, torch.int64, self._dev)
        if label is not None and label.numel() != n:
            raise ValueError("label must have one entry per row")
        return track, label

    def _run(self, call, what, cap):
        """call(out, cap, n_records, tally) with cap records of room; cap None: a counting call first."""
        import torch
        n = ctypes.c_int64()
        if cap is None:
            scratch = torch.zeros(3, dtype=torch.int64, device=self._dev)
            rc = call(None, 0, ctypes.byref(n), scratch)
            if rc != _lib.GM_E_CAPACITY:
                check(rc, what)
            cap = n.value
        out = torch.empty(max(cap, 1) * self.record_bytes, dtype=torch.uint8, device=self._dev)
        check(call(out, cap, ctypes.byref(n), self._tally), what)
        return out[:n.value * self.record_bytes]

    def encode(self, x, y, t_ms, track, label=None, mask=None, ids=None):
        """ToValuesPoints[Labels] over rows of x / y / t_ms (None: date 0) / track / label columns."""
        import torch
        x = _dev_col(x, torch.float64, self._dev)
        y = _dev_col(y, torch.float64, self._dev)
        t = _dev_col(t_ms, torch.int64, self._dev)
        n = x.numel()
        if y.numel() != n or (t is not None and t.numel() != n):
            raise ValueError("x, y and t_ms must have one entry per row")
        track, label = self._columns(n, track, label)
        mask, ids, n_ids = _selection(n, mask, ids, self._dev)
        ctx = _lib.context(self._device)
        o = self._opts()

        def call(out, cap, n_rec, tally):
            return ctx.lib.gm_bin_points(ctx.handle, ptr(x), ptr(y), ptr(t), ptr(track), ptr(label), n, ptr(mask),
                                         ptr(ids), n_ids, ctypes.byref(o), ptr(out), cap, n_rec, ptr(tally))
        return self._run(call, "gm_bin_points", n_ids if ids is not None else n)

    def encode_arrow(self, geom, dtg=None, track=None, label=None, dates=None, mask=None, ids=None, kind="point",
                     flip_axis=False):
        """encode over an Arrow Point or LineString column (an arrow.GeometryColumn, or a pyarrow array of
        `kind`).  dtg: an arrow.TimeColumn or a pyarrow date array (None, or a null slot: date 0).  dates, for
        a LineString column: the List[Date] attribute, as (offsets, millis) host or device columns (a null
        list an empty one) -- vertex i takes dates(i), ToValuesLinesDates[Labels]."""
        import torch
        from .arrow import TimeColumnC, _as_geom, _as_time
        col = _as_geom(geom, kind, flip_axis)
        if col.kind not in ("point", "linestring"):
            raise ValueError("the BIN scan encodes Point and LineString columns")
        n = col.n
        t = _as_time(dtg)
        track, label = self._columns(n, track, label)
        mask, ids, n_ids = _selection(n, mask, ids, self._dev)
        d_off = d_ms = dc = None
        if dates is not None:
            d_off = _dev_col(dates[0], torch.int32, self._dev)
            d_ms = _dev_col(dates[1], torch.int64, self._dev)
            if d_off.numel() != n + 1:
                raise ValueError("dates' offsets need one entry per slot and one more")
            if d_ms.numel() == 0:
                d_ms = torch.zeros(1, dtype=torch.int64, device=self._dev)
            dc = TimeColumnC(d_ms.data_ptr(), None, 0)
        ctx = _lib.context(self._device)
        o = self._opts()
        cs = col.c_struct()
        ts = t.c_struct() if t is not None else None

        def call(out, cap, n_rec, tally):
            return ctx.lib.gm_bin_arrow(ctx.handle, ctypes.byref(cs), ctypes.byref(ts) if ts is not None else None,
                                        ptr(d_off), ctypes.byref(dc) if dc is not None else None, ptr(track),
                                        ptr(label), n, ptr(mask), ptr(ids), n_ids, ctypes.byref(o), ptr(out), cap,
                                        n_rec, ptr(tally))
        cap = None if col.kind == "linestring" else (n_ids if ids is not None else n)
        return self._run(call, "gm_bin_arrow", cap)

    # ------------------------------------------------------------------ order
    def sort(self, records):
        """The records ordered by BinSorter.compare, stably (a new tensor)."""
        import torch
        records = _dev_col(records, torch.uint8, self._dev)
        if records.numel() % self.record_bytes:
            raise ValueError("records are %d bytes each" % self.record_bytes)
        ctx = _lib.context(self._device)
        out = torch.empty(max(records.numel(), 1), dtype=torch.uint8, device=self._dev)
        check(ctx.lib.gm_bin_sort(ctx.handle, ptr(records), records.numel() // self.record_bytes, self.record_bytes,
                                  ptr(out)), "gm_bin_sort")
        return out[:records.numel()]

    def merge(self, chunks):
        """BinSorter.mergeSort over sorted batches (BinSorter.scala:85-145): their concatenation, sorted
        stably, so ties come from the earlier chunk first."""
        import torch
        chunks = [_dev_col(c, torch.uint8, self._dev) for c in chunks]
        if not chunks:
            return torch.empty(0, dtype=torch.uint8, device=self._dev)
        return self.sort(torch.cat(chunks))

    def decode(self, records):
        """BinaryOutputEncoder.decode (BinaryOutputEncoder.scala:176-188) over a buffer of records: a host
        structured array (track, dtg in ms = seconds * 1000, lat, lon, label; label -1 for 16-B records)."""
        import torch
        if isinstance(records, torch.Tensor):
            records = records.cpu().numpy()
        raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        rec = raw.view(RECORD24 if self.label else RECORD16)
        out = np.empty(rec.size, DECODED)
        out["track"], out["lat"], out["lon"] = rec["track"], rec["lat"], rec["lon"]
        out["dtg"] = rec["secs"].astype(np.int64) * 1000
        out["label"] = rec["label"] if self.label else -1
        return out

    # ------------------------------------------------------------------ tallies
    @property
    def tally(self):
        return [int(v) for v in self._tally.cpu().tolist()]

    @property
    def skipped(self):
        return self.tally[0]

    @property
    def bad_ids(self):
        return self.tally[1]

    @property
    def mismatched(self):
        return self.tally[2]

    def clear(self):
        self._tally.zero_()


__all__ = ["BinEncoder", "DECODED", "RECORD16", "RECORD24"]
