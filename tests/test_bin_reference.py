"""tests/bin_ref.py held to the reference's own tests and to known values (no GPU).

BinaryOutputEncoderTest.scala:35-153 (point and line collections, labels, id tracks, sorting) and
BinSorterTest.scala:27-113 (Random(10) features: sort, chunked merge, 24-B records, the 1..8-permutation edge
cases), with the dates java.util.Random gives; String.hashCode / convertToLabel known answers; compare against
plain signed int32 comparison.
"""
import itertools
import struct

import numpy as np

import bin_ref as R

BASE_DTG = 1388563740000     # 2014-01-01 08:09:00 UTC


def point_features():
    """BinaryOutputEncoderTest.scala:36-47."""
    return [{"id": "%d" % i, "track": "1234-%d" % i, "label": 10 + i, "geom": (45.0, 50.0 + i),
             "dtg": BASE_DTG - 60 * 1000 * i, "dates": None} for i in range(4)]


def line_feature():
    """BinaryOutputEncoderTest.scala:96-107."""
    date = 1388563200000    # 2014-01-01 08:00:00
    return {"id": "0", "track": "1234-0", "label": 10, "geom": [(45.0, 50.0), (46.0, 51.0), (47.0, 52.0), (50.0, 55.0)],
            "dtg": date, "dates": [date + 1000 * (9 - i) for i in range(4)]}


def test_string_hash_of_the_reference_tests():
    assert R.string_hash("1234-0") == 1450575205
    assert R.string_hash("1234-3") == 1450575208
    assert R.string_hash("0") == 48 and R.string_hash("3") == 51


def test_point_collection_with_label():
    enc = R.encode(point_features(), label=True)
    assert len(enc) == 4 * 24
    for i in range(4):
        track, lat, lon, dtg, label = R.decode(enc[i * 24:(i + 1) * 24])
        assert dtg == BASE_DTG - 60 * 1000 * i
        assert lat == 50 + i and lon == 45
        assert track == R.string_hash("1234-%d" % i)
        assert label == R.convert_to_label(10 + i) == 10 + i


def test_point_collection_without_label():
    enc = R.encode(point_features())
    assert len(enc) == 4 * 16
    for i in range(4):
        track, lat, lon, dtg, label = R.decode(enc[i * 16:(i + 1) * 16])
        assert (track, lat, lon, dtg, label) == (R.string_hash("1234-%d" % i), 50 + i, 45, BASE_DTG - 60000 * i, -1)


def test_point_collection_with_id_track():
    enc = R.encode(point_features(), track=False)
    assert [R.decode(enc[i * 16:(i + 1) * 16])[0] for i in range(4)] == [48, 49, 50, 51]


def test_axis_order():
    enc = R.encode(point_features(), lat_lon=True)
    assert [R.decode(enc[i * 16:(i + 1) * 16])[1:3] for i in range(4)] == [(45, 50 + i) for i in range(4)]


def test_line_collection():
    f = line_feature()
    for label, size in ((True, 24), (False, 16)):
        enc = R.encode([f], line=True, date_list=True, label=label)
        assert len(enc) == 4 * size
        for i in range(4):
            track, lat, lon, dtg, lab = R.decode(enc[i * size:(i + 1) * size])
            assert dtg == f["dates"][i]
            assert (lat, lon) == (f["geom"][i][1], f["geom"][i][0])
            assert track == 1450575205 and lab == (10 if label else -1)
    single = R.encode([f], line=True)
    assert [R.decode(single[i * 16:(i + 1) * 16])[3] for i in range(4)] == [f["dtg"]] * 4


def test_line_collection_sorted_comes_back_reversed():
    f = line_feature()
    enc = R.sort(R.encode([f], line=True, date_list=True), 16)
    for i in range(4):
        track, lat, lon, dtg, _ = R.decode(enc[i * 16:(i + 1) * 16])
        assert dtg == f["dates"][3 - i]
        assert (lat, lon) == (f["geom"][3 - i][1], f["geom"][3 - i][0])


def test_line_date_list_mismatch_uses_the_minimum():
    f = dict(line_feature(), dates=[1000, 2000])
    tv, cb = R.to_values(line=True, date_list=True), R.ByteStreamCallback()
    tv(f, cb)
    assert cb.result == 2 and tv.mismatched == 1
    f = dict(line_feature(), dates=None)
    tv(f, cb)
    assert cb.result == 2 and tv.mismatched == 2


def sorter_features(jrandom):
    """BinSorterTest.scala:29-39."""
    r = jrandom(10)
    n = r.nextInt(100) + 1
    return [{"id": "%d" % i, "track": "name%d" % i, "label": None, "geom": (40.0, float("6%d" % i)),
             "dtg": r.nextInt(999999), "dates": None} for i in range(n)]


def sorter_bin(jrandom, label=False):
    cb = R.ByteStreamCallback()
    for f in sorter_features(jrandom):
        y, x = R.to_float(f["geom"][1]), R.to_float(f["geom"][0])
        cb(R.string_hash(f["track"]), y, x, f["dtg"], f["dtg"] * 1000 if label else None)
    return cb.bytes()


def dtgs(data, size):
    return [R.decode(r)[3] for r in R.records(data, size)]


def test_sorter_data_is_random_10(jrandom):
    fs = sorter_features(jrandom)
    assert len(fs) == 14
    assert [f["dtg"] for f in fs[:5]] == [993336, 627846, 724176, 135373, 452899]


def test_sorter_sort_16_and_24(jrandom):
    for label, size in ((False, 16), (True, 24)):
        data = sorter_bin(jrandom, label)
        out = R.sort(data, size)
        d = dtgs(out, size)
        assert d == sorted(d) and R.is_sorted(out, size)
        assert sorted(R.records(out, size)) == sorted(R.records(data, size))
        assert out == R.stable_sort_np(data, size)


def test_sorter_chunked_merge(jrandom):
    data = sorter_bin(jrandom)
    chunks = [R.sort(data[k:k + 48], 16) for k in range(0, len(data), 48)]
    assert len(chunks) == 5
    merged = b""
    for c in chunks:
        merged = R.merge_sort(merged, c, 16)
    assert dtgs(merged, 16) == sorted(dtgs(data, 16))
    assert merged == R.sort(b"".join(chunks), 16)      # taking from the left on ties is the stable order
    two = R.merge_sort(chunks[0], chunks[1], 16)       # "mergesort in place"
    assert dtgs(two, 16) == sorted(dtgs(data[:96], 16))


def test_sorter_edge_cases():
    """BinSorterTest.scala:93-113: every permutation of 1..8 records."""
    bins = [R.put(R.string_hash("name%d" % i), 0.0, 0.0, i * 1000) for i in range(1, 9)]
    for i in range(1, 9):
        want = b"".join(bins[:i])
        for seq in itertools.permutations(bins[:i]):
            assert R.stable_sort_np(b"".join(seq), 16) == want
    for i in range(1, 6):
        for seq in itertools.permutations(bins[:i]):
            assert R.sort(b"".join(seq), 16) == b"".join(bins[:i])


def test_merge_takes_left_on_ties():
    a = R.put(1, 0.0, 0.0, 5000) + R.put(2, 0.0, 0.0, 7000)
    b = R.put(3, 0.0, 0.0, 5000) + R.put(4, 0.0, 0.0, 5999) + R.put(5, 0.0, 0.0, 9000)
    assert [R.decode(r)[0] for r in R.records(R.merge_sort(a, b, 16), 16)] == [1, 3, 4, 2, 5]
    assert R.merge_sort(b"", b, 16) == b and R.merge_sort(a, b"", 16) == a


def test_hash_and_label_known_answers():
    assert R.convert_to_track(None) == 0 and R.convert_to_label(None) == 0
    assert R.string_hash("") == 0
    assert R.string_hash("é") == 233 and R.convert_to_label("é") == 43459
    assert R.string_hash("\U0001f600a") == 54959966      # two surrogate units, then 'a'
    assert R.convert_to_label("abc") == 6513249
    assert R.convert_to_label("abcdefghij") == 7523094288207667809
    assert R.convert_to_track(np.int32(-7)) == -7
    assert R.convert_to_track(1 << 32) == 1 and R.convert_to_track(-1) == 0
    assert R.convert_to_track(1.0) == 1072693248 and R.convert_to_track(-0.0) == to_int32(0x80000000)
    assert R.convert_to_track(float("nan")) == R.convert_to_track(struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000123))[0])
    assert R.convert_to_track(float("nan")) == 0x7FF80000
    assert R.convert_to_label(np.int32(-1)) == -1
    assert R.convert_to_label(1e30) == R.LONG_MAX and R.convert_to_label(-1e30) == R.LONG_MIN
    assert R.convert_to_label(float("nan")) == 0 and R.convert_to_label(-2.9) == -2
    assert R.convert_to_label("ééééé") == int.from_bytes("éééé".encode(), "little", signed=True)
    assert R.convert_to_label("abcdefg€") == int.from_bytes(b"abcdefg\xe2", "little", signed=True)   # '€' is cut


def to_int32(v):
    return R.to_int(v)


def test_put_conversions():
    def secs(ms):
        return struct.unpack("<i", R.put(0, 0.0, 0.0, ms)[4:8])[0]
    assert [secs(v) for v in (-1, -999, -1000, -1999, 1999)] == [0, 0, -1, -1, 1]
    assert secs((1 << 31) * 1000) == -(1 << 31)
    assert secs(R.LONG_MAX) == to_int32(R.LONG_MAX // 1000)
    assert secs(R.LONG_MIN) == to_int32(-((1 << 63) // 1000))

    def f32(d):
        return struct.unpack("<I", R.to_float(d).tobytes())[0]
    assert f32(1 + 2.0 ** -24) == 0x3F800000 and f32(1 + 3 * 2.0 ** -24) == 0x3F800002
    assert f32(1e-40) == 0x000116C2 and f32(-0.0) == 0x80000000
    assert f32(1e39) == 0x7F800000 and f32(-1e39) == 0xFF800000
    assert R.to_float(179.99999999999997) == np.float32(180.0)


def test_compare_is_signed_int32_compare():
    vals = [R.INT_MIN, R.INT_MIN + 1, -(1 << 24), -(1 << 24) - 1, -256, -255, -1, 0, 1, 255, 256, 0x00FFFFFF,
            0x01000000, 0x7F000000, 0x7EFFFFFF, 0x00FF00FF, to_int32(0xFF00FF00), to_int32(0x80FFFFFF), R.INT_MAX]
    recs = {v: struct.pack("<iiff", 7, v, 0.0, 0.0) for v in vals}
    for a in vals:
        for b in vals:
            assert R.compare(b"\0" * 3 + recs[a], 3, recs[b], 0) == (a > b) - (a < b), (a, b)
