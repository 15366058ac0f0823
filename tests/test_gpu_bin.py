"""The BIN track-record scan on the GPU, byte for byte against tests/bin_ref.py (the reference's
BinaryOutputEncoder / BinSorter restated; tests/test_bin_reference.py holds that to the reference's own tests).

Sizes: the encode kernel (k_bin, gm_bin.hip) takes B = 2048 candidate records per block (256 lanes x 4 steps x
a pair of rows), a wave 128 consecutive rows of a step; row counts are 0, 1, 63, 64, 65 and 2 B + 5, and one
line slot has 3 B + 1 vertices.
"""
import ctypes
import functools

import numpy as np
import pytest

import bin_ref as R
from abi_buffers import Guarded, untouched

pytestmark = pytest.mark.gpu

B = 2048
SIZES = [0, 1, 63, 64, 65, 2 * B + 5]


def as_bytes(t):
    return t.cpu().numpy().tobytes()


def shifted(arr, shift):
    """A device copy of a numpy column whose address is `shift` bytes past a 256-B boundary."""
    import torch
    arr = np.ascontiguousarray(arr)
    item = arr.dtype.itemsize
    assert shift % item == 0
    buf = torch.zeros(arr.size + 64, dtype=getattr(torch, arr.dtype.name), device="cuda")
    lead = (-buf.data_ptr() % 256 + shift) // item
    t = buf[lead:lead + arr.size]
    t.copy_(torch.from_numpy(arr.copy()))
    assert arr.size == 0 or t.data_ptr() % 256 == shift
    return t


@functools.lru_cache(maxsize=None)
def columns(n, seed=5):
    rng = np.random.default_rng(seed + n)
    x, y = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    t = rng.integers(-10**12, 2 * 10**12, n)
    track = rng.integers(R.INT_MIN, R.INT_MAX, n).astype(np.int32)
    label = rng.integers(R.LONG_MIN, R.LONG_MAX, n)
    for a in (x, y, t, track, label):
        a.setflags(write=False)
    return x, y, t, track, label


def features(x, y, t, track, label):
    return [{"id": "%d" % i, "track": np.int32(track[i]), "label": int(label[i]),
             "geom": (float(x[i]), float(y[i])), "dtg": None if t is None else int(t[i]), "dates": None}
            for i in range(len(x))]


def want_points(cols, rows, bad=0, **kw):
    """bin_ref over the rows a selection names, in its order."""
    fs = features(*cols)
    data, tally = R.scan([fs[i] for i in rows], **kw)
    tally[1] = bad
    return data, tally


def selections(n, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.5
    ids = rng.integers(0, max(n, 1), n + n // 3) if n else np.zeros(0, np.int64)
    return {"none": ({}, list(range(n))), "mask": ({"mask": mask}, np.flatnonzero(mask).tolist()),
            "ids": ({"ids": ids.astype(np.int64)}, ids.tolist())}


# ------------------------------------------------------------------ 1. points

@pytest.mark.parametrize("lat_lon", [False, True])
@pytest.mark.parametrize("moved", [None, "y"])
@pytest.mark.parametrize("sel", ["none", "mask", "ids"])
@pytest.mark.parametrize("label", [False, True])
def test_points(gpu, label, sel, moved, lat_lon):
    from geomesa_amd.bin import BinEncoder
    for n in SIZES:
        cols = columns(n)
        kw, rows = selections(n, 17 + n)[sel]
        want, tally = want_points(cols, rows, label=label, lat_lon=lat_lon)
        dev = [shifted(c, 8 if moved == name else 0) for c, name in zip(cols, "xytkl")]
        enc = BinEncoder(label=label, lat_lon=lat_lon)
        got = enc.encode(dev[0], dev[1], dev[2], dev[3], dev[4] if label else None, **kw)
        assert as_bytes(got) == want, (n, sel)
        assert enc.tally == tally


@pytest.mark.parametrize("moved", ["x", "t", "k", "l"])
def test_points_each_column_moved(gpu, moved):
    from geomesa_amd.bin import BinEncoder
    n = 2 * B + 5
    cols = columns(n)
    want, _ = want_points(cols, range(n), label=True)
    dev = [shifted(c, 8 if moved == name else 0) for c, name in zip(cols, "xytkl")]
    assert as_bytes(BinEncoder(label=True).encode(*dev)) == want
    out = Guarded(n * 24, offset=8)         # an output that is only 8-B aligned: 8-B stores
    nrec, tally = ctypes.c_int64(), shifted(np.zeros(3, np.int64), 0)
    o = _opts()
    rc = gpu.lib.gm_bin_points(gpu.handle, *[ctypes.c_void_p(d.data_ptr()) for d in dev], n, None, None, 0,
                               ctypes.byref(o), out.ptr, n, ctypes.byref(nrec), ctypes.c_void_p(tally.data_ptr()))
    assert rc == 0 and nrec.value == n and out.read().tobytes() == want
    out.check("8-B aligned output")


def test_points_without_dates(gpu):
    from geomesa_amd.bin import BinEncoder
    x, y, _, track, label = columns(65)
    want, _ = want_points((x, y, None, track, label), range(65))
    assert as_bytes(BinEncoder().encode(x, y, None, track)) == want


# ------------------------------------------------------------------ 2. conversions

ORDINATES = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1e-40, -0.0, 1e39, -1e39, 179.99999999999997, 0.1, -1e-46]
TIMES = [-1, -999, -1000, -1999, (1 << 31) * 1000, R.LONG_MAX, R.LONG_MIN, 0, 1999]


def test_conversion_fixtures(gpu):
    from geomesa_amd.bin import BinEncoder
    n = len(ORDINATES) * len(TIMES)
    x = np.array([ORDINATES[i % len(ORDINATES)] for i in range(n)])
    y = np.array([ORDINATES[(i // len(ORDINATES) + i) % len(ORDINATES)] for i in range(n)])
    t = np.array([TIMES[i // len(ORDINATES)] for i in range(n)], np.int64)
    track, label = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int64)
    for lat_lon in (False, True):
        want, _ = want_points((x, y, t, track, label), range(n), lat_lon=lat_lon)
        enc = BinEncoder(lat_lon=lat_lon)
        got = enc.encode(x, y, t, track)
        assert as_bytes(got) == want and enc.tally == [0, 0, 0]
    rec = BinEncoder().encode(x, y, t, track).cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert rec[:len(ORDINATES), 3].tolist() == [0x3F800000, 0x3F800002, 0x000116C2, 0x80000000, 0x7F800000,
                                                0xFF800000, 0x43340000, 0x3DCCCCCD, 0x80000000]
    secs = rec[::len(ORDINATES), 1].view(np.int32).tolist()
    assert secs[:5] == [0, 0, -1, -1, -(1 << 31)]
    assert secs[5:7] == [R.to_int(R.LONG_MAX // 1000), R.to_int(-((1 << 63) // 1000))]


# ------------------------------------------------------------------ 3. ids and masks

def test_ids_and_masks(gpu):
    import torch
    from geomesa_amd.bin import BinEncoder
    n = 2 * B + 5
    cols = columns(n)
    x, y, t, track, label = cols
    for ids, bad in ((np.arange(n)[::-1], 0), (np.array([5, 5, 5, 0, n - 1, 5]), 0), (np.zeros(0, np.int64), 0),
                     (np.array([3, -1, n, 2, 1 << 40, R.LONG_MIN, 2]), 4)):
        rows = [i for i in ids.tolist() if 0 <= i < n]
        want, tally = want_points(cols, rows, bad=bad, label=True)
        enc = BinEncoder(label=True)
        assert as_bytes(enc.encode(x, y, t, track, label, ids=ids.astype(np.int64))) == want
        assert enc.tally == tally and enc.bad_ids == bad
    # every entry outside [0, n), and no rows at all: nothing is read through
    enc = BinEncoder()
    assert enc.encode(x[:0], y[:0], t[:0], track[:0], ids=np.array([0, 1, -1])).numel() == 0 and enc.bad_ids == 3
    # mask words with bits set at and above n
    keep = np.random.default_rng(3).random(n) < 0.3
    want, _ = want_points(cols, np.flatnonzero(keep).tolist())
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = keep
    bits[n:] = 1
    words = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int64).copy()).cuda()
    assert as_bytes(BinEncoder().encode(x, y, t, track, mask=words)) == want
    assert as_bytes(BinEncoder().encode(x, y, t, track, mask=keep)) == want
    with pytest.raises(ValueError):
        BinEncoder().encode(x, y, t, track, mask=keep, ids=np.array([1]))


# ------------------------------------------------------------------ 4. NaN and null rows

HOLES = [0, 1, 126, 127, 128, 129, 2 * 128 - 1, B - 1, B, B + 1, 2 * B - 2, 2 * B, 2 * B + 4]


@pytest.mark.parametrize("label", [False, True])
def test_nan_rows_shift_the_records_down(gpu, label):
    """NaN rows at lanes 0 and 63, on both sides of a wave's edge (row 128) and of a block's (row B)."""
    from geomesa_amd.bin import BinEncoder
    n = 2 * B + 5
    x, y, t, track, lab = (np.array(c) for c in columns(n))
    x[HOLES[::2]] = np.nan
    y[HOLES[1::2]] = np.nan
    cols = (x, y, t, track, lab)
    for name, (kw, rows) in selections(n, 9).items():
        want, tally = want_points(cols, rows, label=label)
        for shift in (0, 8):
            enc = BinEncoder(label=label)
            got = enc.encode(shifted(x, shift), y, t, track, lab if label else None, **kw)
            assert as_bytes(got) == want, (name, shift)
            assert enc.tally == tally
        if name == "none":
            assert tally[0] == len(HOLES) and len(want) == (n - len(HOLES)) * (24 if label else 16)


# ------------------------------------------------------------------ 5. capacity

def _opts(sort=0, lat_lon=0):
    from geomesa_amd import _lib
    return _lib.BinOpts(sort, lat_lon)


def call_points(gpu, cols, n, out_ptr, cap, o, label=True, mask=None, ids=None, n_ids=0, tally=None, nrec=None, x=0,
                y=0, ctx=0, track=0):
    """gm_bin_points on device tensors (x / y / ctx / track: an override, None included)."""
    p = [ctypes.c_void_p(c.data_ptr()) if c is not None else None for c in cols]
    return gpu.lib.gm_bin_points(gpu.handle if ctx == 0 else ctx, p[0] if x == 0 else x, p[1] if y == 0 else y, p[2],
                                 p[3] if track == 0 else track, p[4] if label else None, n, mask, ids, n_ids,
                                 ctypes.byref(o) if o is not None else None, out_ptr, cap,
                                 ctypes.byref(nrec) if nrec is not None else None,
                                 ctypes.c_void_p(tally.data_ptr()) if tally is not None else None)


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("label", [False, True])
def test_capacity(gpu, label, sort):
    from geomesa_amd import _lib
    n, size = 2 * B + 5, 24 if label else 16
    cols = columns(n)
    dev = [shifted(c, 0) for c in cols]
    want, _ = want_points(cols, range(n), label=label)
    if sort:
        want = R.stable_sort_np(want, size)
    tally, nrec = shifted(np.zeros(3, np.int64), 0), ctypes.c_int64(-1)
    out = Guarded((n - 1) * size)
    rc = call_points(gpu, dev, n, out.ptr, n - 1, _opts(sort), label, tally=tally, nrec=nrec)
    assert rc == _lib.GM_E_CAPACITY and nrec.value == n
    out.check("one record short")
    assert untouched(out.read())
    rc = call_points(gpu, dev, n, None, 0, _opts(sort), label, tally=tally, nrec=nrec)    # counts only
    assert rc == _lib.GM_E_CAPACITY and nrec.value == n
    out = Guarded(n * size)
    rc = call_points(gpu, dev, n, out.ptr, n, _opts(sort), label, tally=tally, nrec=nrec)
    assert rc == 0 and nrec.value == n and out.read().tobytes() == want
    out.check("exact capacity")


# ------------------------------------------------------------------ 6, 7. Arrow

def arrow_points(x, y, f32=False, flip=False, nulls=None):
    import pyarrow as pa
    a, b = (x, y) if flip else (y, x)
    flat = np.stack([a, b], 1).reshape(-1).astype(np.float32 if f32 else np.float64)
    return pa.FixedSizeListArray.from_arrays(pa.array(flat), 2, mask=None if nulls is None else pa.array(nulls))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("f32", [False, True])
def test_arrow_points(gpu, f32, flip):
    import pyarrow as pa
    from geomesa_amd.bin import BinEncoder
    n, lead = 2 * B + 5, 3
    x, y, t, track, label = (np.array(c) for c in columns(n + lead))
    if f32:
        x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(8)
    nulls = rng.random(n + lead) < 0.1
    nulls[[lead, lead + 63, lead + 128, lead + B]] = True
    x[lead + 64] = np.nan
    tnull = rng.random(n + lead) < 0.1
    pts = arrow_points(x, y, f32, flip, nulls).slice(lead)          # a validity bitmap with an offset of 3
    dtg = pa.array(t, pa.int64(), mask=tnull).slice(lead)
    fs = features(x, y, t, track, label)
    for i in range(n + lead):
        if nulls[i]:
            fs[i]["geom"] = None
        if tnull[i]:
            fs[i]["dtg"] = None
    fs = fs[lead:]
    for name, (kw, rows) in selections(n, 12).items():
        for lab in (False, True):
            want, tally = R.scan([fs[i] for i in rows], label=lab)
            enc = BinEncoder(label=lab)
            got = enc.encode_arrow(pts, dtg, track[lead:], label[lead:] if lab else None, flip_axis=flip, **kw)
            assert as_bytes(got) == want, (name, lab)
            assert enc.tally == tally
    assert tally[0] > 100
    want, _ = R.scan([dict(f, dtg=None) for f in fs])
    assert as_bytes(BinEncoder().encode_arrow(pts, None, track[lead:], flip_axis=flip)) == want


LINE_LENGTHS = [0, 1, 2, 63, 64, 65, 300, 3 * B + 1, 5, 0, 7]


@functools.lru_cache(maxsize=None)
def line_rows():
    """Line features: the lengths above (slot 8 null), and date lists equal to, shorter than, longer than the
    line, and null."""
    rng = np.random.default_rng(31)
    fs = []
    for i, m in enumerate(LINE_LENGTHS):
        geom = [(float(a), float(b)) for a, b in zip(rng.uniform(-180, 180, m), rng.uniform(-90, 90, m))]
        nd = {2: m - 1, 4: m + 3, 5: 0, 10: None}.get(i, m)
        dates = None if nd is None else [int(v) for v in rng.integers(-10**9, 10**12, nd)]
        fs.append({"id": "%d" % i, "track": np.int32(rng.integers(R.INT_MIN, R.INT_MAX)), "label": int(rng.integers(-99, 99)),
                   "geom": geom, "dtg": int(rng.integers(0, 10**12)), "dates": dates})
    fs[8]["geom"] = None
    fs[6]["geom"][17] = (float("nan"), 1.0)
    fs[7]["geom"][B] = (2.0, float("nan"))
    return fs


def line_arrays(fs, f32=False, flip=False):
    import pyarrow as pa
    counts = [0 if f["geom"] is None else len(f["geom"]) for f in fs]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    xy = np.array([p for f in fs if f["geom"] for p in f["geom"]], np.float64).reshape(-1, 2)
    geom = pa.ListArray.from_arrays(pa.array(off), arrow_points(xy[:, 0], xy[:, 1], f32, flip),
                                    mask=pa.array([f["geom"] is None for f in fs]))
    dcount = [0 if f["dates"] is None else len(f["dates"]) for f in fs]
    doff = np.concatenate([[0], np.cumsum(dcount)]).astype(np.int32)
    dms = np.array([d for f in fs if f["dates"] for d in f["dates"]], np.int64)
    return geom, (doff, dms)


@pytest.mark.parametrize("date_list", [False, True])
@pytest.mark.parametrize("label", [False, True])
def test_arrow_lines(gpu, label, date_list):
    import pyarrow as pa
    from geomesa_amd.bin import BinEncoder
    fs = line_rows()
    n = len(fs)
    geom, dates = line_arrays(fs)
    dtg = pa.array([f["dtg"] for f in fs], pa.int64())
    track = np.array([f["track"] for f in fs], np.int32)
    lab = np.array([f["label"] for f in fs], np.int64)
    mask = np.array([i % 3 != 1 for i in range(n)])
    ids = np.array([7, 3, 3, -1, 8, 10, 0, 6, n, 2, 4], np.int64)
    sels = {"none": ({}, range(n), 0), "mask": ({"mask": mask}, np.flatnonzero(mask).tolist(), 0),
            "ids": ({"ids": ids}, [i for i in ids.tolist() if 0 <= i < n], 2)}
    for name, (kw, rows, bad) in sels.items():
        want, tally = R.scan([fs[i] for i in rows], line=True, date_list=date_list, label=label)
        tally[1] = bad
        enc = BinEncoder(label=label)
        got = enc.encode_arrow(geom, dtg, track, lab if label else None, dates=dates if date_list else None,
                               kind="linestring", **kw)
        assert as_bytes(got) == want, name
        assert enc.tally == tally, name
        if name == "none":
            assert tally[0] == 3 and tally[2] == (4 if date_list else 0)
    want, _ = R.scan(fs, line=True, date_list=date_list, label=label)
    enc = BinEncoder(label=label, sort=True)
    got = enc.encode_arrow(geom, dtg, track, lab if label else None, dates=dates if date_list else None, kind="linestring")
    assert as_bytes(got) == R.stable_sort_np(want, enc.record_bytes)


def test_arrow_lines_float4_and_flipped(gpu):
    from geomesa_amd.bin import BinEncoder
    fs = [dict(f) for f in line_rows()[:7]]
    for f in fs:
        f["geom"] = [(float(np.float32(a)), float(np.float32(b))) for a, b in f["geom"]]
    track = np.array([f["track"] for f in fs], np.int32)
    want, _ = R.scan(fs, line=True, lat_lon=True)
    for flip in (False, True):
        geom, _ = line_arrays(fs, f32=True, flip=flip)
        got = BinEncoder(lat_lon=True).encode_arrow(geom, None, track, kind="linestring", flip_axis=flip)
        assert as_bytes(got) == R.scan([dict(f, dtg=None) for f in fs], line=True, lat_lon=True)[0]
    assert len(want) == 16 * (sum(LINE_LENGTHS[:7]) - 1)


# ------------------------------------------------------------------ 8. sort and merge

@pytest.mark.parametrize("label", [False, True])
def test_sort_ties_and_signed_seconds(gpu, label):
    from geomesa_amd.bin import BinEncoder
    n, size = 10_000, 24 if label else 16
    rng = np.random.default_rng(77)
    x, y = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    track, lab = np.arange(n, dtype=np.int32), rng.integers(-5, 5, n)
    enc = BinEncoder(label=label, sort=True)
    plain = BinEncoder(label=label)
    secs5 = np.array([-2000, 0, 3000, (1 << 31) * 1000, -(1 << 31) * 1000 - 999])     # the 4th wraps negative
    for t in (secs5[rng.integers(0, 5, n)], rng.integers(-(1 << 42), 1 << 42, n)):
        got = as_bytes(enc.encode(x, y, t, track, lab if label else None))
        unsorted = as_bytes(plain.encode(x, y, t, track, lab if label else None))
        assert R.is_sorted(got, size)
        assert sorted(R.records(got, size)) == sorted(R.records(unsorted, size))
        assert got == R.stable_sort_np(unsorted, size)
        assert as_bytes(enc.sort(plain.encode(x, y, t, track, lab if label else None))) == got
    for k in (0, 1):
        one = plain.encode(x[:k], y[:k], t[:k], track[:k], lab[:k] if label else None)
        assert as_bytes(enc.sort(one)) == as_bytes(one) and one.numel() == k * size
        assert as_bytes(enc.encode(x[:k], y[:k], t[:k], track[:k], lab[:k] if label else None)) == as_bytes(one)


def test_merge_is_merge_sort(gpu, jrandom):
    """merge([left, right]) == BinSorter.mergeSort(left, right) on the BinSorterTest chunks and on random sizes."""
    import torch
    from geomesa_amd.bin import BinEncoder
    from test_bin_reference import sorter_bin
    enc = BinEncoder()

    def dev(b):
        return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    data = sorter_bin(jrandom)
    chunks = [R.sort(data[k:k + 48], 16) for k in range(0, len(data), 48)]
    assert [as_bytes(enc.sort(dev(data[k:k + 48]))) for k in range(0, len(data), 48)] == chunks
    assert as_bytes(enc.merge([dev(chunks[0]), dev(chunks[1])])) == R.merge_sort(chunks[0], chunks[1], 16)
    merged = b""
    for c in chunks:
        merged = R.merge_sort(merged, c, 16)
    assert as_bytes(enc.merge([dev(c) for c in chunks])) == merged
    rng = np.random.default_rng(6)
    enc24 = BinEncoder(label=True)
    for nl, nr in ((0, 5), (7, 0), (1, 1), (300, 77), (2 * B + 5, 1000)):
        parts = []
        for m in (nl, nr):
            secs = rng.integers(-3, 4, m)        # ties inside and across the two sides
            recs = b"".join(R.put(int(rng.integers(0, 1 << 30)), 1.0, 2.0, int(s) * 1000, int(rng.integers(0, 99)))
                            for s in secs)
            parts.append(R.stable_sort_np(recs, 24) if m else b"")
        want = R.merge_sort(parts[0], parts[1], 24)
        assert as_bytes(enc24.merge([dev(p) for p in parts])) == want, (nl, nr)
    assert enc.merge([]).numel() == 0


# ------------------------------------------------------------------ 9. tracks and labels

STRINGS = ["", "abc", "1234-0", "é", "\U0001f600a", "€5", "abcdefghij", None, "ééééé", "name13", None, "abcdefg€",
           "ࠀ￿\U00010000\U0010ffff", "x" * 100_000, "\x7f\x80߿"]


def test_track_and_label_of_strings(gpu):
    from geomesa_amd.bin import BinEncoder, _utf8_column
    enc = BinEncoder()
    want_t = [R.convert_to_track(s) for s in STRINGS]
    want_l = [R.convert_to_label(s) for s in STRINGS]
    assert want_t[:5] == [0, 96354, 1450575205, 233, 54959966] and want_l[3] == 43459 and want_l[6] == 7523094288207667809
    assert enc.track_of(STRINGS).cpu().tolist() == want_t
    assert enc.label_of(STRINGS).cpu().tolist() == want_l
    # offsets that do not start at 0, and a validity bitmap with an offset
    off, data, valid = _utf8_column(STRINGS)
    bits = np.concatenate([[1, 0, 1], np.unpackbits(valid, bitorder="little")[:len(STRINGS)]]).astype(np.uint8)
    col = (off[2:], data, np.packbits(bits, bitorder="little"), 5)
    assert enc.track_of(col).cpu().tolist() == want_t[2:]
    assert enc.label_of(col).cpu().tolist() == want_l[2:]
    assert enc.track_of([]).numel() == 0


def test_track_of_a_truncated_final_sequence_reads_nothing_past_the_slot(gpu):
    """The last slot ends inside a 4-byte sequence and at the end of a guarded buffer: the value is
    unspecified, the reads are not."""
    import torch
    from geomesa_amd import _lib
    data = "ab".encode() + "\U0001f600".encode()[:2]
    g = Guarded.of(np.frombuffer(data, np.uint8))
    off = torch.tensor([0, 2, len(data)], dtype=torch.int32, device="cuda")
    out = Guarded(8)
    col = _lib.AttrColumn(_lib.GM_ATTR_UTF8, 0, g.addr, off.data_ptr(), None, 0)
    assert gpu.lib.gm_bin_track(gpu.handle, ctypes.byref(col), 2, out.ptr) == 0
    assert int(out.read(np.int32)[0]) == R.string_hash("ab")
    out.check("track output")
    lab = Guarded(16)
    assert gpu.lib.gm_bin_label(gpu.handle, ctypes.byref(col), 2, lab.ptr) == 0
    assert lab.read(np.int64).tolist() == [int.from_bytes(b"ab", "little"), int.from_bytes(data[2:], "little")]


def test_track_and_label_of_numbers(gpu):
    from geomesa_amd.bin import BinEncoder
    enc = BinEncoder()
    i32 = np.array([0, 1, -1, R.INT_MIN, R.INT_MAX, 12345], np.int32)
    assert enc.track_of(i32).cpu().tolist() == i32.tolist() == [R.convert_to_track(v) for v in i32]
    assert enc.label_of(i32).cpu().tolist() == i32.tolist()
    i64 = np.array([0, -1, 1 << 32, R.LONG_MIN, R.LONG_MAX, 0x123456789ABCDEF], np.int64)
    assert enc.track_of(i64).cpu().tolist() == [R.convert_to_track(int(v)) for v in i64]
    assert enc.label_of(i64).cpu().tolist() == i64.tolist()
    nan_payload = np.array([0x7FF0000000000123, 0xFFF8000000000001], np.uint64).view(np.float64)
    f64 = np.concatenate([[0.0, -0.0, 1.0, -2.9, np.inf, -np.inf, np.nan, 1e30, -1e30, 2.0 ** 63, 1e-320], nan_payload])
    assert enc.track_of(f64).cpu().tolist() == [R.convert_to_track(float(v)) for v in f64]
    assert enc.track_of(f64).cpu().tolist()[-2:] == [0x7FF80000] * 2
    got = enc.label_of(f64).cpu().tolist()
    assert got == [R.convert_to_label(float(v)) for v in f64]
    assert got[6] == 0 and got[7] == R.LONG_MAX and got[8] == R.LONG_MIN and got[3] == -2


# ------------------------------------------------------------------ 10. composition

@pytest.mark.parametrize("sort", [False, True])
def test_table_query_and_query_scan_compose(gpu, sort):
    from geomesa_amd import filters as F
    from geomesa_amd.bin import BinEncoder
    from geomesa_amd.keyspace import during
    from geomesa_amd.table import Z3Table
    from test_host_planning import ms
    rng = np.random.default_rng(41)
    n = 10_000
    x, y = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    t = rng.integers(1577836800000, 1609459200000, n)
    names = ["track-%d" % (i % 37) for i in range(n)]
    enc = BinEncoder(label=True, sort=sort)
    track, label = enc.track_of(names), enc.label_of(names)
    fs = [{"id": "%d" % i, "track": names[i], "label": names[i], "geom": (float(x[i]), float(y[i])), "dtg": int(t[i]),
           "dates": None} for i in range(n)]
    bbox = (-40.0, 10.0, 40.0, 70.0)
    lo, hi = ms("2020-03-01T00:00:00.000Z"), ms("2020-06-08T12:00:00.000Z")
    tb = Z3Table.from_points(x, y, t)
    ids, nm, _ = tb.query([bbox], [during(lo, hi)])
    assert nm > 50
    want, _ = R.scan([fs[i] for i in ids.cpu().tolist()], label=True)
    got = as_bytes(enc.encode(x, y, t, track, label, ids=ids))
    assert got == (R.stable_sort_np(want, 24) if sort else want)
    mask, _, nk = F.query_scan(x, y, t, bbox=bbox, during=(lo, hi))
    keep = [i for i in range(n) if bbox[0] <= x[i] <= bbox[2] and bbox[1] <= y[i] <= bbox[3] and lo < t[i] < hi]
    assert nk == len(keep) > 50
    want, _ = R.scan([fs[i] for i in keep], label=True)
    got = as_bytes(enc.encode(x, y, t, track, label, mask=mask))
    assert got == (R.stable_sort_np(want, 24) if sort else want)
    assert enc.tally == [0, 0, 0]


# ------------------------------------------------------------------ 11. invalid arguments

def last_error():
    from geomesa_amd import _lib
    return _lib.last_error()


def test_invalid_arguments_of_points(gpu):
    from geomesa_amd import _lib
    n = 65
    dev = [shifted(c, 0) for c in columns(n)]
    tally, nrec, out, o = shifted(np.zeros(3, np.int64), 0), ctypes.c_int64(), Guarded(n * 24), _opts()
    one = ctypes.c_void_p(tally.data_ptr())
    odd = ctypes.c_void_p(dev[0].data_ptr() + 4)
    cases = {
        "null-ctx": dict(ctx=None), "null-opts": dict(o=None), "null-tally": dict(tally=None), "null-n-records": dict(nrec=None),
        "null-x": dict(x=None), "null-y": dict(y=None), "null-track": dict(track=None), "negative-n": dict(n=-1),
        "negative-n-ids": dict(ids=one, n_ids=-1), "negative-cap": dict(cap=-1), "null-out": dict(out_ptr=None),
        "mask-and-ids": dict(mask=one, ids=one, n_ids=1), "sort-2": dict(o=_opts(sort=2)), "sort-negative": dict(o=_opts(sort=-1)),
        "lat-lon-2": dict(o=_opts(lat_lon=2)), "misaligned-x": dict(x=odd), "misaligned-track": dict(track=odd),
        "misaligned-out": dict(out_ptr=ctypes.c_void_p(out.addr + 4)),
    }
    texts = {}
    for name, kw in cases.items():
        args = dict(n=n, out_ptr=out.ptr, cap=n, o=o, tally=tally, nrec=nrec)
        args.update(kw)
        rc = call_points(gpu, dev, args.pop("n"), args.pop("out_ptr"), args.pop("cap"), args.pop("o"), True, **args)
        assert rc == _lib.GM_E_INVALID, name
        texts[name] = last_error()
        assert texts[name].startswith("gm_bin_points: "), name
    assert texts["null-x"] == texts["null-y"] and texts["sort-2"] == texts["sort-negative"]
    distinct = {k: v for k, v in texts.items() if not k.startswith("misaligned") and k not in ("sort-negative", "null-y")}
    assert len(set(distinct.values())) == len(distinct), texts
    assert "alignment" in texts["misaligned-x"] and "alignment" in texts["misaligned-out"]
    out.check("invalid calls")
    assert untouched(out.read()) and tally.cpu().tolist() == [0, 0, 0]


def test_invalid_arguments_of_arrow_and_sort(gpu):
    import pyarrow as pa
    from geomesa_amd import _lib
    from geomesa_amd.arrow import GeometryColumn, TimeColumn, TimeColumnC
    n = 5
    x, y, t, track, label = columns(n)
    pts = GeometryColumn(arrow_points(x, y), "point")
    lines, (doff, dms) = line_arrays(line_rows()[:n])
    lines = GeometryColumn(lines, "linestring")
    poly = GeometryColumn(pa.array([[[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0]]]] * n,
                                   pa.list_(pa.list_(pa.list_(pa.float64(), 2)))), "polygon")
    dtg = TimeColumn(pa.array(t, pa.int64()))
    d_off, d_ms = shifted(doff, 0), shifted(dms, 0)
    dc = TimeColumnC(d_ms.data_ptr(), None, 0)
    trk, tally, nrec, out, o = shifted(track, 0), shifted(np.zeros(3, np.int64), 0), ctypes.c_int64(), Guarded(4096), _opts()

    def call(geom, date_off=None, dates=None, track=trk):
        gs = geom.c_struct()
        return gpu.lib.gm_bin_arrow(gpu.handle, ctypes.byref(gs), ctypes.byref(dtg.c_struct()),
                                    ctypes.c_void_p(date_off.data_ptr()) if date_off is not None else None,
                                    ctypes.byref(dates) if dates is not None else None,
                                    ctypes.c_void_p(track.data_ptr()) if track is not None else None, None, n, None,
                                    None, 0, ctypes.byref(o), out.ptr, 256, ctypes.byref(nrec),
                                    ctypes.c_void_p(tally.data_ptr()))
    texts = []
    for args in ((poly,), (lines, d_off, None), (lines, None, dc), (pts, d_off, dc), (pts, None, None, None)):
        assert call(*args) == _lib.GM_E_INVALID
        texts.append(last_error())
        assert texts[-1].startswith("gm_bin_arrow: ")
    assert len(set(texts)) == 4 and texts[1] == texts[2]
    assert call(pts) == 0 and nrec.value == n
    assert call(lines, d_off, dc) == 0
    # gm_bin_sort
    rec = shifted(np.zeros(48, np.uint8), 0)
    p, q = ctypes.c_void_p(rec.data_ptr()), out.ptr
    bad = [(None, p, 2, 16, q), (gpu.handle, p, 2, 20, q), (gpu.handle, p, -1, 16, q), (gpu.handle, p, 1 << 32, 16, q),
           (gpu.handle, None, 2, 16, q), (gpu.handle, p, 2, 24, p), (gpu.handle, ctypes.c_void_p(rec.data_ptr() + 4), 2, 16, q)]
    texts = []
    for args in bad:
        assert gpu.lib.gm_bin_sort(*args) == _lib.GM_E_INVALID
        texts.append(last_error())
        assert texts[-1].startswith("gm_bin_sort: ")
    assert len(set(texts)) == len(texts)
    assert "2^32 - 1" in texts[3]
    assert gpu.lib.gm_bin_sort(gpu.handle, p, 0, 16, q) == 0
    # gm_bin_track / gm_bin_label
    col = _lib.AttrColumn(9, 0, rec.data_ptr(), None, None, 0)
    assert gpu.lib.gm_bin_track(gpu.handle, ctypes.byref(col), 2, q) == _lib.GM_E_INVALID
    assert last_error().startswith("gm_bin_track: ")
    col = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, rec.data_ptr() + 4, None, None, 0)
    assert gpu.lib.gm_bin_label(gpu.handle, ctypes.byref(col), 2, q) == _lib.GM_E_INVALID
    assert "alignment" in last_error()
    out.check("invalid calls")


# ------------------------------------------------------------------ 12. accumulation

def test_batches_accumulate_and_do_not_see_a_larger_call_s_leftovers(gpu):
    from geomesa_amd.bin import BinEncoder
    big = 2 * B + 5
    x, y, t, track, label = (np.array(c) for c in columns(big))
    x[::7] = np.nan
    enc = BinEncoder()
    ids_big = np.concatenate([np.arange(big), [-1, big]]).astype(np.int64)
    first = enc.encode(x, y, t, track, ids=ids_big)
    want_big, tally_big = want_points((x, y, t, track, label), range(big), bad=2)
    assert as_bytes(first) == want_big and enc.tally == tally_big
    small = 65
    cols = tuple(c[100:100 + small] for c in (x, y, t, track, label))
    want, tally = want_points(cols, range(small))
    assert as_bytes(enc.encode(cols[0], cols[1], cols[2], cols[3])) == want
    assert enc.tally == [a + b for a, b in zip(tally_big, tally)]
    assert enc.skipped == tally_big[0] + tally[0] and enc.bad_ids == 2 and enc.mismatched == 0
    enc.clear()
    assert enc.tally == [0, 0, 0]
