"""The attribute index on the host: the lexicoders, the reference's own answers (DefaultSplitterTest,
AttributeIndexTest) through the restatement of tests/attr_ref.py, geomesa_amd.attribute's planning against that
restatement, the byte range -> gm_attr_range map held to byte comparison, and the stand-alone half of the ABI
test.  No GPU."""
import ctypes
import itertools
import math
import re

import numpy as np
import pytest

import attr_ref as R
from geomesa_amd import _lib
from geomesa_amd import attribute as A
from geomesa_amd.keyspace import Bounds

INF, NAN = float("inf"), float("nan")
DENORM32, DENORM64 = float(np.float32(1e-45)), 5e-324
EDGES = {
    "int": [-(1 << 31), -1, 0, 1, (1 << 31) - 1],
    "long": [-(1 << 63), -1, 0, 1, (1 << 63) - 1],
    "date": [-(1 << 63), -1, 0, 1388577600000, (1 << 63) - 1],
    "float": [-INF, -1.5, -DENORM32, -0.0, 0.0, DENORM32, 1.5, INF, NAN],
    "double": [-INF, -1.5, -DENORM64, -0.0, 0.0, DENORM64, 1.5, INF, NAN],
}
BINDINGS = list(EDGES)


def ms(text):
    import datetime
    d = datetime.datetime.strptime(text, "%Y-%m-%dT%H:%M:%S.%fZ").replace(tzinfo=datetime.timezone.utc)
    return int(round(d.timestamp() * 1000))


# ---------------------------------------------------------------- lexicoders
def test_default_splitter_strings():
    """DefaultSplitterTest.scala:134-188: lexicoded Integers in hex."""
    for enc in (R.encode, A.AttributeIndexKey.type_encode):
        assert [enc(i, "int") for i in range(10)] == ["8000000%d" % i for i in range(10)]
        assert [enc(i, "int") for i in (0, 1, 5, 6)] == ["80000000", "80000001", "80000005", "80000006"]
        assert [enc(i, "int") for i in (2, 3, 12, 13)] == ["80000002", "80000003", "8000000c", "8000000d"]
        assert [enc(i, "int") for i in range(80, 90)] == ["8000005%d" % i for i in range(10)]
        assert [enc(i, "int") for i in range(-9, 1)] == [format(0x80000000 + i, "08x") for i in range(-9, 1)]
        assert [enc(i, "int") for i in (-9, -8, -6, -5)] == ["7ffffff7", "7ffffff8", "7ffffffa", "7ffffffb"]
        assert [enc(i, "int") for i in (-13, -12, -3, -2)] == ["7ffffff3", "7ffffff4", "7ffffffd", "7ffffffe"]
        assert enc(80, "int") == "80000050" and enc(89, "int") == "80000059"


@pytest.mark.parametrize("binding", BINDINGS)
def test_lexicoded_order_is_numeric_order(binding):
    """The edge values are listed in numeric order (-0.0 below +0.0, NaN last): their key texts ascend strictly,
    byte order of the text = unsigned order of v, and both implementations agree."""
    texts = [R.encode(v, binding) for v in EDGES[binding]]
    assert texts == [A.AttributeIndexKey.type_encode(v, binding) for v in EDGES[binding]]
    assert all(len(t) == R.HEX[binding] and t == t.lower() for t in texts)
    assert all(a.encode() < b.encode() for a, b in zip(texts, texts[1:]))
    vs = [A.AttributeIndexKey.ordered(v, binding) for v in EDGES[binding]]
    assert vs == [R.ordered(v, binding) for v in EDGES[binding]] == [int(t, 16) for t in texts]
    assert all(a < b for a, b in zip(vs, vs[1:]))


def test_zero_and_nan_consequences():
    for b in ("float", "double"):
        lo, hi = R.ordered(-0.0, b), R.ordered(0.0, b)
        assert hi == lo + 1                                          # immediately below, a different key
        assert R.ordered(NAN, b) > R.ordered(INF, b)
        assert R.encode(-NAN, b) == R.encode(NAN, b)                 # every NaN is the canonical one
    assert R.encode(NAN, "float") == "ffc00000" and R.encode(0.0, "float") == "80000000"


@pytest.mark.parametrize("binding", BINDINGS)
def test_decode_inverts_encode(binding):
    rng = np.random.default_rng(5)
    extra = {"int": rng.integers(-(1 << 31), 1 << 31, 50).tolist(),
             "long": rng.integers(-(1 << 63), (1 << 63) - 1, 50).tolist(),
             "date": rng.integers(0, 1 << 41, 50).tolist(),
             "float": rng.normal(0, 1e6, 50).astype(np.float32).astype(float).tolist(),
             "double": rng.normal(0, 1e6, 50).tolist()}[binding]
    for v in EDGES[binding] + extra:
        for dec, enc in ((R.decode, R.encode), (A.AttributeIndexKey.decode, A.AttributeIndexKey.type_encode)):
            back = dec(binding, enc(v, binding))
            if isinstance(v, float) and math.isnan(v):
                assert math.isnan(back)
            else:
                assert back == v and math.copysign(1, back) == math.copysign(1, v)
    assert A.AttributeIndexKey.encode_for_query(None, binding) is None


def test_bindings_left_out():
    for b in ("String", "List[Int]", "UUID"):
        with pytest.raises(NotImplementedError):
            A.binding_of(b)
    with pytest.raises(NotImplementedError):
        A.KeyLayout(8, "xz3")


# ---------------------------------------------------------------- AttributeIndexTest
NAMES = ["alice", "bill", "bob", "charles"]
AGE = [20, 21, 30, None]
HEIGHT = [10.0, 11.0, 12.0, 12.0]
X, Y = [45.0, 46.0, 47.0, 48.0], [49.0] * 4
DTG = [ms("2012-01-01T12:00:00.000Z"), ms("2013-01-01T12:00:00.000Z"), ms("2014-01-01T12:00:00.000Z"),
       ms("2014-01-01T12:30:00.000Z")]
SHARDS = 4
SHARD = [1, 3, 0, 2]      # any assignment: the results never depend on it


def feature_store(values, binding, tier, shards=SHARDS):
    import oracle as O
    if tier == "z3":
        b, z, st = O.z3_index_key_batch(X, Y, DTG)
        assert not st.any()
        tiers = [R.tier_z3(b[i], z[i]) for i in range(4)]
    elif tier == "date":
        tiers = [R.tier_date(t) for t in DTG]
    else:
        tiers = [b""] * 4
    return R.Store([R.row_key(values[i], binding, tiers[i], SHARD[i] if shards else None) for i in range(4)])


def run(values, binding, tier, bounds, bboxes=None, intervals=None, shards=SHARDS):
    """The reference store's answer, its ranges checked as AttributeIndexTest.scala:91-97 checks them, beside the
    definitional answer."""
    store = feature_store(values, binding, tier, shards)
    ranges = R.plan(bounds, binding, tier, shards, bboxes, intervals)
    pairs = R.scan_bounds(ranges)
    assert not R.overlaps(pairs), pairs
    got = [store.order[r] for r in store.candidates(ranges)
           if R.secondary(X[store.order[r]], Y[store.order[r]], DTG[store.order[r]], bboxes, intervals)]
    assert got == R.definition(store, values, binding, bounds, X, Y, DTG, bboxes, intervals)
    return [NAMES[i] for i in got], ranges


ST_BOX = [(46.9, 48.9, 48.1, 49.1)]
ST_DURING = [(ms("2014-01-01T11:45:00.000Z"), False, ms("2014-01-01T12:15:00.000Z"), False)]


def test_secondary_index_ranges():
    """:83-109: height = 12.0 matches bob and charles, the spatio-temporal filter only bob."""
    names, ranges = run(HEIGHT, "float", "z3", [(12.0, True, 12.0, True)], ST_BOX, ST_DURING)
    assert names == ["bob"]
    prefix = len(R.encode(12.0, "float")) + 2          # shard + value + delimiter
    assert ranges and all(len(r.lower) > prefix for r in ranges)          # z3 ranges behind the equals prefix
    assert run(HEIGHT, "float", "z3", [(12.0, True, 12.0, True)])[0] == ["bob", "charles"]
    assert run(AGE, "int", "z3", [(30, True, 30, True)], ST_BOX, ST_DURING)[0] == ["bob"]
    assert sorted(run(AGE, "int", "z3", [])[0]) == ["alice", "bill", "bob"]      # charles's age is null: no row


def test_one_sided_secondary_filter():
    """:202-221: height = 12.0 AND dtg > 2014-01-01T11:45: every range start is longer than value + delimiter."""
    after = [(ms("2014-01-01T11:45:00.000Z"), False, None, False)]
    names, ranges = run(HEIGHT, "float", "z3", [(12.0, True, 12.0, True)], None, after)
    assert sorted(names) == ["bob", "charles"]
    assert ranges and all(len(r.lower) > 1 + 8 + 1 for r in ranges)


def test_secondary_date_equality():
    """:335-359 on an attr:age:dtg table: the five forms of `dtg = 2014-01-01T12:00` return bob alone."""
    t = ms("2014-01-01T12:00:00.000Z")
    forms = [[(t, True, t, True)],                    # dtg = / tequals / between t and t
             [(t - 1, False, t + 1, False)],          # during t - 1 ms / t + 1 ms
             [(t, True, t + 1, False)]]               # dtg >= t and dtg < t + 1 ms
    for iv in forms:
        names, ranges = run(AGE, "int", "date", [(30, True, 30, True)], None, iv)
        assert names == ["bob"], iv
        assert all(len(r.lower) == 1 + 8 + 1 + 8 for r in ranges)
    assert run(AGE, "int", "date", [(30, True, 30, True)], None, [(t, False, t + 1, False)])[0] == []


# ---------------------------------------------------------------- geomesa_amd.attribute against the restatement
KINDS = {
    "equality": [(7, True, 7, True)],
    "in": [(3, True, 3, True), (7, True, 7, True), (-2, True, -2, True)],
    "lt": [(None, False, 7, False)], "le": [(None, False, 7, True)],
    "gt": [(7, False, None, False)], "ge": [(7, True, None, False)],
    "between": [(3, True, 7, True)], "open": [(3, False, 7, False)], "half": [(3, True, 7, False)],
    "not_null": [(None, False, None, False)], "none": [], "disjoint": "disjoint",
}
T0 = 1388577600000
DATE_TIERS = {
    "no secondary": None, "during": [(T0, False, T0 + 3600000, False)], "equals": [(T0, True, T0, True)],
    "after": [(T0, False, None, False)], "before": [(None, False, T0, True)], "disjoint": "disjoint",
    "two": [(T0, True, T0 + 5, True), (T0 + 100, False, T0 + 200, True)],
}
Z3_SCAN = {    # Z3IndexKeySpace.get_ranges tuples
    "no secondary": None,
    "bounded": [("bounded", (2296, 100), (2296, 200)), ("bounded", (2296, 1 << 40), (2296, (1 << 41) + 5))],
    "lower": [("bounded", (2296, 100), (2296, 200)), ("lower", (2297, 0), None)],
    "upper": [("upper", None, (2295, (1 << 63) - 1)), ("bounded", (2296, 5), (2296, 0xffffffffffff))],
    "unbounded": [("unbounded", None, None)], "disjoint": [],
}


def as_pairs(ranges):
    return [(r.kind, r.lower, r.upper) for r in ranges]


def product_bounds(iv):
    return iv if iv in (None, "disjoint") else [Bounds(lo, hi, li, ui) for lo, li, hi, ui in iv]


@pytest.mark.parametrize("shards", [0, 4])
@pytest.mark.parametrize("kind", list(KINDS))
def test_byte_ranges_equal_the_restatement(kind, shards):
    """Every range kind x tier kind x shards: getRangeBytes and the combined ranges, byte for byte."""
    bounds = KINDS[kind]
    for binding in ("int", "double"):
        ks = A.AttributeIndexKeySpace(binding, shards)
        ref_ranges = R.get_ranges(bounds, binding)
        got_ranges = ks.get_ranges(bounds)
        assert len(got_ranges) == len(ref_ranges)
        for tier in (False, True):
            assert as_pairs(ks.get_range_bytes(got_ranges, tier)) == as_pairs(R.get_range_bytes(ref_ranges, tier, shards))
        primary, ref_primary = ks.get_range_bytes(got_ranges, True), R.get_range_bytes(ref_ranges, True, shards)
        d = A.DateIndexKeySpace()
        for name, iv in DATE_TIERS.items():
            tiers = None if iv is None else d.get_range_bytes(d.get_ranges(product_bounds(iv)))
            ref_tiers = None if iv is None else R.date_range_bytes(R.date_ranges(iv))
            assert as_pairs(A.combine_tiers(primary, tiers)) == as_pairs(R.combine(ref_primary, ref_tiers)), name
        for name, sr in Z3_SCAN.items():
            tiers = None if sr is None else A.z3_tier_range_bytes(sr)
            ref_tiers = None if sr is None else R.z3_range_bytes(sr)
            assert as_pairs(A.combine_tiers(primary, tiers)) == as_pairs(R.combine(ref_primary, ref_tiers)), name
    assert A.single_rows(primary) == max(1, sum(1 for r in ref_primary if r.kind == "single"))


def test_date_tier_without_tiering():
    d = A.DateIndexKeySpace()
    for iv in DATE_TIERS.values():
        if iv is not None:
            assert as_pairs(d.get_range_bytes(d.get_ranges(product_bounds(iv)), tier=False)) == \
                as_pairs(R.date_range_bytes(R.date_ranges(iv), tier=False))


# ---------------------------------------------------------------- byte range -> gm_attr_range
U_VALUES = [-(1 << 31), -3, 7, (1 << 31) - 1]       # 4 values, the smallest and the largest v among them
U_BINS = [0, 2296, 0x7fff]
U_Z = [0, 5, 1 << 40, (1 << 63) - 1]


def struct_member(row, s, v, b, t):
    return int(row["shard"]) == s and (int(row["v_lo"]), int(row["b_lo"]), int(row["t_lo"])) <= (v, b, t) <= \
        (int(row["v_hi"]), int(row["b_hi"]), int(row["t_hi"]))


@pytest.mark.parametrize("shards", [0, 2])
def test_attr_ranges_hold_to_byte_comparison(shards):
    """Over a small universe with the Z3 tier, every inclusive / exclusive combination of every pair of values,
    open ends, the exclusive lower at the largest v (empty), with and without tier ranges: a row is inside the
    gm_attr_range rows iff its bytes are inside the byte ranges."""
    layout = A.KeyLayout(8, "z3", bool(shards))
    ks = A.AttributeIndexKeySpace("int", shards)
    universe = [(s, x, b, z) for s in range(max(shards, 1)) for x in U_VALUES for b in U_BINS for z in U_Z]
    keys = [R.row_key(x, "int", R.tier_z3(b, z), s if shards else None) for s, x, b, z in universe]
    assert all(len(k) == layout.length for k in keys)
    ends = [None] + U_VALUES
    bounds = [(lo, li, hi, ui) for lo in ends for hi in ends for li in (True, False) for ui in (True, False)
              if lo is None or hi is None or lo <= hi]
    tier_sets = [None, [], A.z3_tier_range_bytes(Z3_SCAN["bounded"]), A.z3_tier_range_bytes(Z3_SCAN["lower"]),
                 A.z3_tier_range_bytes(Z3_SCAN["upper"]), A.z3_tier_range_bytes([("bounded", (2296, 5), (2296, 5))])]
    checked = empty = 0
    for bound, tiers in itertools.product(bounds, tier_sets):
        combined = A.combine_tiers(ks.get_range_bytes(ks.get_ranges([bound]), True), tiers)
        arr = A.attr_ranges(combined, layout)
        pairs = R.scan_bounds([R.BR(*c) for c in combined])
        for (s, x, b, z), k in zip(universe, keys):
            by_bytes = any(lo <= k and (hi == b"" or k < hi) for lo, hi in pairs)
            by_struct = any(struct_member(r, s, R.ordered(x, "int"), b, z) for r in arr)
            assert by_bytes == by_struct, (bound, tiers, (s, x, b, z), arr)
            checked += 1
        empty += not len(arr)
    assert checked > 10000 and empty > 0
    top = A.combine_tiers(ks.get_range_bytes(ks.get_ranges([((1 << 31) - 1, False, None, False)]), True), None)
    assert len(A.attr_ranges(top, layout)) == 0      # exclusive lower at the largest v: no key follows
    assert len(A.attr_ranges(A.combine_tiers(ks.get_range_bytes(ks.get_ranges([]), True), None), layout)) == max(shards, 1)


def test_attr_ranges_other_layouts():
    """The date tier and no tier, 16-digit keys: the same membership rule with the fields the table has."""
    for tier, tiers in (("date", [R.tier_date(t) for t in (None, -5, 0, T0)]), (None, [b""])):
        layout = A.KeyLayout(16, tier, False)
        ks = A.AttributeIndexKeySpace("double", 0)
        vals = [-INF, -0.0, 0.0, 2.5, NAN]
        universe = [(x, t) for x in vals for t in tiers]
        d = A.DateIndexKeySpace()
        for lo, hi, li, ui in itertools.product([None] + vals, [None] + vals, (True, False), (True, False)):
            for iv in ([None] if tier is None else [None, [Bounds(-5, T0, True, False)], [Bounds(0, 0, True, True)]]):
                primary = ks.get_range_bytes(ks.get_ranges([(lo, li, hi, ui)]), tier is not None)
                combined = primary if tier is None else A.combine_tiers(
                    primary, None if iv is None else d.get_range_bytes(d.get_ranges(iv)))
                arr = A.attr_ranges(combined, layout)
                pairs = R.scan_bounds([R.BR(*c) for c in combined])
                for x, t in universe:
                    k = R.row_key(x, "double", t)
                    tw = int.from_bytes(t, "big") if t else 0
                    by_bytes = any(a <= k and (b == b"" or k < b) for a, b in pairs)
                    by_struct = any(int(r["v_lo"]) <= R.ordered(x, "double") <= int(r["v_hi"]) and
                                    (int(r["v_lo"]), int(r["t_lo"]) if t else 0) <= (R.ordered(x, "double"), tw) <=
                                    (int(r["v_hi"]), int(r["t_hi"]) if t else 0) for r in arr)
                    assert by_bytes == by_struct, (tier, lo, hi, li, ui, iv, x, t)


# ---------------------------------------------------------------- the host half of the seek, stand-alone
def test_range_check_under_sanitizers(tmp_path):
    """tools/attr_range_check.cpp: the key order, its successor and merge_ranges (csrc/gm_seek.hpp) against a
    brute-force universe, built alone with the address and undefined-behaviour sanitizers."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed to build tools/attr_range_check.cpp")
    exe = str(tmp_path / "attr_range_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(root, "tools", "attr_range_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("bad 0"), out.stdout


# ---------------------------------------------------------------- ABI, the stand-alone half
SYMBOLS = ["gm_attr_index_key", "gm_attr_key_bytes", "gm_attr_sort", "gm_attr_table_scan"]


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)


def test_signatures_present():
    from geomesa_amd import build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    code = header_code()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, code, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s
        assert params.split(",")[0].strip() == "gm_ctx* ctx", s      # every entry takes the context


def test_attr_range_matches_header():
    body = re.search(r"typedef struct \{([^}]*)\}\s*gm_attr_range;", header_code()).group(1)
    fields = [re.sub(r"\[.*\]", "", f) for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    names = ["v_lo", "v_hi", "t_lo", "t_hi", "b_lo", "b_hi", "shard", "reserved"]
    assert fields == [f[0] for f in _lib.AttrRange._fields_] == names == list(_lib.ATTR_RANGE_DTYPE.names)
    assert ctypes.sizeof(_lib.AttrRange) == 40 == _lib.ATTR_RANGE_DTYPE.itemsize
    for n in names:
        assert getattr(_lib.AttrRange, n).offset == _lib.ATTR_RANGE_DTYPE.fields[n][1], n
    assert _lib.AttrRange.t_lo.offset == 16 and _lib.AttrRange.b_lo.offset == 32 and _lib.AttrRange.shard.offset == 36


def test_tier_constants_match_header():
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(GM_ATTR_TIER_[A-Z0-9]+)\s+(\d+)", open(_lib.HEADER).read()))
    assert defs == {"GM_ATTR_TIER_NONE": _lib.GM_ATTR_TIER_NONE, "GM_ATTR_TIER_DATE": _lib.GM_ATTR_TIER_DATE,
                    "GM_ATTR_TIER_Z3": _lib.GM_ATTR_TIER_Z3}
