"""The Frequency / Z3Frequency restatement (tests/frequency_ref.py) against the reference's own unit tests and
the JVM's integer and rounding rules, and the package's host-side helpers against the restatement.  No GPU."""
import datetime
import math

import numpy as np
import pytest

import frequency_ref as R
from geomesa_amd import stats as S

WEEK = 1
HASH_A = [575626169, 278924161, 1519804117, 1200401393, 783957587]
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)


def ms(s):
    return int(datetime.datetime.fromisoformat(s + "+00:00").timestamp() * 1000)


def test_default_shape_and_hash_multipliers():
    """CountMinSketch.scala:186-187, 197-200 with Frequency.Seed = -27 (Frequency.scala:213)."""
    assert R.shape() == (5, 400)
    assert R.hash_a(5) == HASH_A
    assert S.cms_shape() == (5, 400) and S.cms_hash_a(5) == HASH_A
    assert S.cms_hash_a(32) == R.hash_a(32)
    assert R.shape(0.01, 0.9) == S.cms_shape(0.01, 0.9) == (4, 200)


def test_hash_rows_of_extreme_keys():
    """CountMinSketch.scala:48-57 at the ends of the Long range."""
    for key in (-1, LONG_MAX):
        assert [R.hash_scalar(key, a, 400) for a in HASH_A] == [278, 286, 330, 254, 60]
    assert [R.hash_scalar(LONG_MIN, a, 400) for a in HASH_A] == [0] * 5
    b = R.buckets(np.array([-1, LONG_MAX, LONG_MIN], np.int64), HASH_A, 400)
    assert b.T.tolist() == [[278, 286, 330, 254, 60], [278, 286, 330, 254, 60], [0] * 5]


@pytest.mark.parametrize("width", [400, 1, 7, 20000, 2147483647])
def test_hash_vector_against_scalar(width):
    rng = np.random.default_rng(width)
    keys = np.concatenate([rng.integers(LONG_MIN, LONG_MAX, 2000, dtype=np.int64, endpoint=True),
                           np.array([0, 1, -1, LONG_MAX, LONG_MIN, 1 << 32, -(1 << 32), (1 << 31) - 1], np.int64)])
    hashes = R.hash_a(7) + [0, 1, (1 << 31) - 2]
    b = R.buckets(keys, hashes, width)
    for i, a in enumerate(hashes):
        assert b[i].tolist() == [R.hash_scalar(int(k), a, width) for k in keys]
    assert b.min() >= 0 and b.max() < width


def test_mask():
    """Frequency.getMask (Frequency.scala:284-287): the JVM shifts by the count mod 64."""
    want = {0: LONG_MAX, 1: LONG_MIN, 25: -(1 << 39), 63: -2, 64: LONG_MAX}
    for p, m in want.items():
        assert R.mask(p) == m and S.frequency_mask(p) == m, p
    with pytest.raises(ValueError):
        S.frequency_mask(65)


def test_math_round():
    """Math.round: ties toward +Infinity, NaN -> 0, saturating; 0.49999999999999994 + 0.5 rounds to 1.0 in
    floating point, and the closest long is 0."""
    cases = {0.5: 1, -0.5: 0, 1.5: 2, 2.5: 3, -1.5: -1, -2.5: -2, 0.49999999999999994: 0, 2.0 ** 52 + 1: 2 ** 52 + 1,
             float("nan"): 0, float("inf"): LONG_MAX, float("-inf"): LONG_MIN, 1e19: LONG_MAX, -1e19: LONG_MIN,
             -0.0: 0, 9007199254740993.0: 9007199254740992}
    a = np.array(list(cases), np.float64)
    want = list(cases.values())
    assert [R.round_scalar(v) for v in a] == want
    assert R.round_array(a).tolist() == want
    assert S.java_round(a).tolist() == want
    f = np.array([0.5, -0.5, 1.5, 2.5, 0.49999997, 2.0 ** 23 + 1, np.nan, np.inf, -np.inf, 3e9, -3e9, -2147483648.0],
                 np.float32)
    wf = [1, 0, 2, 3, 0, 2 ** 23 + 1, 0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31]
    assert [R.round_scalar(v, single=True) for v in f] == wf
    assert R.round_array(f).tolist() == wf and S.java_round(f).tolist() == wf


def test_math_round_vector_against_scalar():
    rng = np.random.default_rng(5)
    k = rng.integers(-(1 << 40), 1 << 40, 4000)
    a = np.concatenate([k + 0.5, k - 0.5, np.nextafter(k + 0.5, -np.inf), np.nextafter(k + 0.5, np.inf),
                        rng.normal(0, 1e6, 4000), rng.normal(0, 1e18, 500)])
    assert R.round_array(a).tolist() == [R.round_scalar(v) for v in a]
    f = np.concatenate([(k[:2000] % (1 << 22)) + 0.5, rng.normal(0, 1e5, 2000), rng.normal(0, 1e9, 500)]).astype(np.float32)
    f = np.concatenate([f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))])
    assert R.round_array(f).tolist() == [R.round_scalar(v, single=True) for v in f]
    assert S.java_round(a).tolist() == R.round_array(a).tolist() and S.java_round(f).tolist() == R.round_array(f).tolist()


def test_integer_division_truncates():
    """Frequency.scala:303-304: -7 / 2 == -3 in both widths, and the ends of the ranges."""
    assert R.attr_keys("int", [-7, 7, -8], 2).tolist() == [-3, 3, -4]
    assert R.attr_keys("long", np.array([-7, 7, -8], np.int64), 2).tolist() == [-3, 3, -4]
    i = np.array([-(1 << 31), (1 << 31) - 1], np.int32)
    assert R.attr_keys("int", i, 1).tolist() == [-(1 << 31), (1 << 31) - 1]
    assert R.attr_keys("int", i, 3).tolist() == [-715827882, 715827882]
    l = np.array([LONG_MIN, LONG_MAX], np.int64)
    assert R.attr_keys("long", l, 1).tolist() == [LONG_MIN, LONG_MAX]
    assert R.attr_keys("long", l, 1000).tolist() == [-9223372036854775, 9223372036854775]
    f = S.Frequency("intAttr", 3, binding="int")
    assert f.keys(i).tolist() == [-715827882, 715827882]
    f = S.Frequency("longAttr", 1000, binding="long")
    assert f.keys(l).tolist() == [-9223372036854775, 9223372036854775]


def test_min_value_columns(oracle):
    """Int.MinValue / Long.MinValue columns: the Long.MinValue key hashes to bucket 0 of every row."""
    s = R.Sketches().observe_attr(oracle, "long", np.full(10, LONG_MIN, np.int64), 1)
    assert s.size.tolist() == [10] and s.table[0, :, 0].tolist() == [10] * 5 and s.table.sum() == 50
    assert s.estimate([LONG_MIN]).tolist() == [10]
    s = R.Sketches().observe_attr(oracle, "int", np.full(10, -(1 << 31), np.int32), 1)
    assert s.size.tolist() == [10] and s.estimate([-(1 << 31)]).tolist() == [10]


def test_float_keys_take_a_float_product():
    """floatToKey (Frequency.scala:305): value * precision in float32 (the Int converts), then the closest int."""
    v = np.array([0.1, 16777217.0, -2.5, 1e30, np.nan], np.float32)
    assert R.attr_keys("float", v, 10).tolist() == [1, 167772160, -25, 2 ** 31 - 1, 0]
    assert R.attr_keys("double", v.astype(np.float64), 10).tolist() == [1, 167772160, -25, LONG_MAX, 0]
    f = S.Frequency("floatAttr", 10, binding="float")
    assert f.keys(v).tolist() == [1, 167772160, -25, 2 ** 31 - 1, 0]


def test_frequency_int_attribute(oracle):
    """FrequencyTest.scala:199-205, 231-250 ("correctly bin values", "combine two Frequencies"): the reference
    asserts 1..2, 0 and, merged, 1..3; the restatement pins the exact sets."""
    a = R.Sketches().observe_attr(oracle, "int", np.arange(100, dtype=np.int32), 1)
    assert a.size.sum() == 100 and a.tally.tolist() == [0, 0, 0]
    assert set(a.estimate(np.arange(100)).tolist()) == {1}
    assert a.estimate([200]).tolist() == [0]
    b = R.Sketches().observe_attr(oracle, "int", np.arange(100, 200, dtype=np.int32), 1)
    assert b.size.sum() == 100
    assert set(b.estimate(np.arange(100, 200)).tolist()) == {1}
    assert b.estimate([300]).tolist() == [0]
    a.merge(b)
    assert a.size.sum() == 200
    assert set(a.estimate(np.arange(200)).tolist()) == {1, 2}
    assert a.estimate([300]).tolist() == [0]
    assert b.size.sum() == 100 and set(b.estimate(np.arange(100, 200)).tolist()) == {1}


def weekly_features():
    """FrequencyTest.scala:71-80: longAttr = i, dtg = Epoch + 2340 weeks + 1 hour + (i % 28) days."""
    i = np.arange(28 * 4, dtype=np.int64)
    start = 45 * 52 * 604800000 + 3600000
    return i, start + (i % 28) * 86400000


def test_frequency_weekly_binning(oracle):
    """FrequencyTest.scala:69-103 ("support weekly binning"): four bins 2340..2343, each count 1, and
    splitByTime."""
    v, t = weekly_features()
    s = R.Sketches(bin_lo=2338, n_bins=8).observe_attr(oracle, "long", v, 1, t_ms=t, period=WEEK)
    assert (np.flatnonzero(s.size) + 2338).tolist() == [2340, 2341, 2342, 2343] and s.tally.tolist() == [0, 0, 0]
    for w in range(4):
        vals = np.concatenate([np.arange(o + 7 * w, o + 7 * w + 7) for o in (0, 28, 56, 84)])
        assert s.estimate(vals, np.full(len(vals), 2340 + w)).tolist() == [1] * 28
        split = R.Sketches(bin_lo=2340 + w, n_bins=1)     # splitByTime: that bin's sketch alone
        split.table[0], split.size[0] = s.table[2 + w], s.size[2 + w]
        assert split.estimate(vals).tolist() == [1] * 28
    assert s.estimate([5], [2339]).tolist() == [0] and s.estimate([5], [9999]).tolist() == [0]


def test_enumerate_ranges(oracle):
    """FrequencyTest.scala:61-67 ("enumerate ranges")."""
    lo = oracle.z2_invert(oracle.z2_apply(2, 2))
    hi = oracle.z2_invert(oracle.z2_apply(3, 6))
    ranges = oracle.z2_ranges([(lo[0], lo[1], hi[0], hi[1])])
    want = [12, 13, 14, 15, 36, 37, 38, 39, 44, 45]
    assert sorted(R.enumerate_ranges([(r[0], r[1]) for r in ranges], 64)) == want
    assert sorted(S.Frequency.enumerate([(r[0], r[1]) for r in ranges], 64)) == want
    from geomesa_amd.curve import IndexRange
    assert sorted(S.Frequency.enumerate([IndexRange(*r) for r in ranges], 64)) == want
    # precision 62: keys 4 apart (Frequency.scala:230-236)
    assert list(S.Frequency.enumerate([(8, 19)], 62)) == [8, 12, 16] == R.enumerate_ranges([(8, 19)], 62)


def z3_features():
    """Z3FrequencyTest.scala:30-37: POINT(-i, i / 2) at 2012-01-01T(i % 24):00."""
    i = np.arange(100)
    t = np.array([ms("2012-01-01T%02d:00:00" % (k % 24)) for k in i], np.int64)
    return -i.astype(np.float64), (i // 2).astype(np.float64), t


def test_z3frequency(oracle):
    """Z3FrequencyTest.scala:43-50 ("correctly bin values"): size 100, every count within 1..6 -- here 100
    distinct masked keys with estimates 1..5: the linear hash sends multiples of 2^39 to few buckets."""
    x, y, t = z3_features()
    s = R.Sketches(bin_lo=2191, n_bins=1).observe_z3(oracle, x, y, t, WEEK, 25)
    assert s.size.tolist() == [100] and s.tally.tolist() == [0, 0, 0]
    b, z, st = oracle.z3_index_key_batch(x, y, t, period=WEEK)
    assert set(b.tolist()) == {2191} and not st.any()
    keys = z & np.int64(R.mask(25))
    assert len(set(keys.tolist())) == 100
    est = s.estimate(keys, b)
    assert est.min() == 1 and est.max() == 5
    assert len(set(R.buckets(keys, s.hashes, 400)[0].tolist())) <= 25


def test_tallies_and_selection(oracle):
    """The three tallies of the dense block: a throwing row, a bin outside the window, an id outside [0, n)."""
    x = np.array([0.0, 200.0, np.nan, 10.0, 20.0])
    y = np.array([0.0, 0.0, 0.0, 95.0, 5.0])
    t = np.array([ms("2020-01-01T00:00:00"), ms("2020-01-01T00:00:00"), 5, -1, ms("2021-06-01T00:00:00")], np.int64)
    s = R.Sketches(bin_lo=2608, n_bins=2).observe_z3(oracle, x, y, t, WEEK, 64)
    assert s.tally.tolist() == [3, 1, 0] and s.size.sum() == 1
    s = R.Sketches(bin_lo=2608, n_bins=2).observe_z3(oracle, x, y, t, WEEK, 64, ids=[0, 0, 7, -1, 4])
    assert s.tally.tolist() == [0, 1, 2] and s.size.sum() == 2
    words = np.array([0b10001 | (1 << 40)], np.int64)     # rows 0 and 4; bit 40 lies above n
    s = R.Sketches(bin_lo=2608, n_bins=2).observe_z3(oracle, x, y, t, WEEK, 64, mask_words=words)
    assert s.tally.tolist() == [0, 1, 0] and s.size.sum() == 1
    # Frequency: a null value is not observed at all; a null date is bin 0; a negative date throws
    v = np.array([1, 2, 3, 4], np.int64)
    s = R.Sketches(bin_lo=0, n_bins=1).observe_attr(oracle, "long", v, 1, t_ms=np.array([-5, -5, 9, -5], np.int64),
                                                    valid=np.array([0b1110], np.uint8), t_valid=np.array([0b0101], np.uint8))
    assert s.tally.tolist() == [0, 0, 0] and s.size.tolist() == [3]
    s = R.Sketches(bin_lo=0, n_bins=1).observe_attr(oracle, "long", v, 1, t_ms=np.array([-5, -5, 9, -5], np.int64))
    assert s.tally.tolist() == [3, 0, 0] and s.size.tolist() == [1]


def test_string_attribute_is_not_implemented():
    with pytest.raises(NotImplementedError, match="MurmurHash"):
        S.Frequency("strAttr", 1, binding="string")
    assert math.isclose(S.Frequency("a", 1, binding="long").eps, 0.005)
