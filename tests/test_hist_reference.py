"""Histogram / MinMax without a GPU: the two restatements of tests/hist_ref.py against each other, the
reference's own test answers (HistogramTest.scala, MinMaxTest.scala over StatTestHelper's features), the
library's host entries through ctypes against restatement (a), tools/hist_replay_check.cpp under the address
and undefined-behaviour sanitizers, and the host-only side of the Python classes (merges, all_reduce over
gloo)."""
import ctypes
import math
import os
import shutil
import socket
import struct
import subprocess
import sys

import numpy as np
import pytest

import hist_ref as R
from geomesa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 7, 1000]
ATTR = {"int": _lib.GM_ATTR_INT32, "long": _lib.GM_ATTR_INT64, "date": _lib.GM_ATTR_INT64,
        "float": _lib.GM_ATTR_FLOAT32, "double": _lib.GM_ATTR_FLOAT64}


def _ulp_out(binding, lo, hi):
    if binding in R.WHOLE:
        return [lo, hi, hi + 1, lo - 1, lo - 2, hi + 2]
    t = np.float32 if binding == "float" else np.float64
    return [t(lo), t(hi), np.nextafter(t(hi), t(np.inf)), np.nextafter(t(lo), t(-np.inf)),
            np.nextafter(np.nextafter(t(lo), t(-np.inf)), t(-np.inf)), t(hi) * 2]


def inputs(binding, n):
    """name -> (bounds, values): the order cases of the issue for one binding."""
    rng = np.random.default_rng(11)
    dt = R.DTYPE[binding]
    g = rng.normal(0, 1000, n)
    out = {
        "random": ((-100, 100), g.astype(dt)),
        "ascending": ((-100, 100), np.sort(g).astype(dt)),
        "descending": ((-100, 100), np.sort(g)[::-1].astype(dt)),
        "all-equal": ((-100, 100), np.full(n, 250).astype(dt)),
        "alternating": ((-100, 100), np.array([(1 if i & 1 else -1) * (101 + 3 * i) for i in range(n)]).astype(dt)),
        "on-bound": ((-100, 100), np.array(_ulp_out(binding, -100, 100) * 3, dt)),
        "inside": ((-5000, 5000), np.clip(g, -5000, 5000).astype(dt)),
    }
    if binding in ("float", "double"):
        e = g.astype(dt)
        e[3], e[17 % n], e[29 % n] = np.nan, np.nan, -0.0
        out["nan"] = ((-100, 100), e.copy())
        e[11 % n], e[23 % n] = np.inf, -np.inf
        out["inf"] = ((-100, 100), e.copy())
        out["zeros"] = ((0.0, 1.0), np.array([0.0, -0.0, 0.5, -0.0, 1.0, -1e-30, 0.0], dt))
    if binding in ("long", "date"):
        lo, hi = R.LONG_MIN, R.LONG_MAX
        out["near-min"] = ((lo + 50, lo + 90), np.array([lo + 60, lo, lo + 70, 5, hi - 3, 0, hi, lo + 1, -7], dt))
        out["near-max"] = ((hi - 90, hi - 50), np.array([hi - 60, hi, hi - 70, -5, lo + 3, 0, lo, hi - 1, 7], dt))
    if binding == "int":
        out["int-extremes"] = ((R.INT_MAX - 90, R.INT_MAX - 50),
                               np.array([R.INT_MAX, R.INT_MAX - 60, R.INT_MIN, 0, R.INT_MAX], dt))
    return out


def as_list(binding, values):
    return values if binding == "float" else values.tolist()


def same_bounds(a, b):
    return all(x == y and math.copysign(1, float(x)) == math.copysign(1, float(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("binding", R.BINDINGS)
def test_route_equals_reference_loop(binding, length):
    n = 80 if length == 1000 else 400
    for name, (bounds, values) in inputs(binding, n).items():
        a = R.RefHistogram(binding, length, bounds).observe(as_list(binding, values))
        bb, cc, ee = R.route_observe(binding, length, bounds, [0] * length, values)
        assert same_bounds(a.bounds, bb) and a.counts == cc and a.expansions == ee, (name, "observe")
        # unobserve of the first half, onto what observe left, with values that expand again
        back = (values[: len(values) // 2] * 3).astype(values.dtype)
        a.unobserve(as_list(binding, back))
        bb2, cc2, ee2 = R.route_observe(binding, length, bb, cc, back, sign=-1)
        assert same_bounds(a.bounds, bb2) and a.counts == cc2 and a.expansions == ee + ee2, (name, "unobserve")


def test_order_matters():
    v = np.array([5, 50, 500, -700, 20, 3000, 7], np.int64)
    a = R.RefHistogram("long", 7, (0, 100)).observe(v.tolist())
    b = R.RefHistogram("long", 7, (0, 100)).observe(v[::-1].tolist())
    assert a.bounds == b.bounds and a.counts != b.counts


# ---------------------------------------------------------------------- HistogramTest.scala
F1, F2 = list(range(100)), list(range(100, 200))
DAY0 = 1325376000000   # 2012-01-01T00:00:00.000Z
D1 = [DAY0 + (i % 24) * 3600000 for i in range(100)]
D2 = [DAY0 + 86400000 + (i % 24) * 3600000 for i in range(100, 200)]


def hist(binding, n, lo, hi, values=None):
    h = R.RefHistogram(binding, n, (lo, hi))
    return h.observe(values) if values is not None else h


def test_histogram_test_ints():   # HistogramTest.scala:157-296
    s = hist("int", 20, 0, 199, F1)
    assert s.counts == [10] * 10 + [0] * 10
    s.unobserve(F1[:50])
    assert s.counts == [0] * 5 + [10] * 5 + [0] * 10
    s, s2 = hist("int", 20, 0, 199, F1), hist("int", 20, 0, 199, F2)
    assert s2.counts == [0] * 10 + [10] * 10
    s += s2
    assert s.counts == [10] * 20
    s, s2 = hist("int", 20, 0, 99, F1), hist("int", 20, 100, 199, F2)
    assert s.counts == [5] * 20 and s2.counts == [5] * 20
    s += s2
    assert s.bounds == (0, 199) and s.counts == [10] * 20
    s, s2 = hist("int", 20, 0, 199, F1), hist("int", 10, 0, 199, F2)
    assert s2.counts == [0] * 5 + [20] * 5
    s += s2
    assert s.length == 20 and s.bounds == (0, 199) and s.counts == [10] * 20
    s, s2 = hist("int", 20, -100, 300, F1), hist("int", 20, 50, 249, F2)
    assert s.counts == [0] * 5 + [20] * 5 + [0] * 10
    assert s2.counts == [0] * 5 + [10] * 10 + [0] * 5
    s += s2
    assert s.bounds == (0, 199)
    assert s.counts == [6, 8, 12, 8, 12, 8, 12, 8, 12, 8, 16, 10, 10, 10, 10, 10, 10, 10, 10, 10]


def test_histogram_test_longs():   # :298-365
    s, s2 = hist("long", 10, 0, 99, F1), hist("long", 10, 100, 199, F2)
    assert s.counts == [10] * 10 and s2.counts == [10] * 10
    s += s2
    assert s.bounds == (0, 199) and s.counts == [20] * 10 and s2.counts == [10] * 10


@pytest.mark.parametrize("binding", ["float", "double"])
def test_histogram_test_floats_doubles(binding):   # :367-440, :442-515
    assert hist(binding, 10, 0, 99 if binding == "double" else 100, F1).counts == [10] * 10
    s, s2 = hist(binding, 10, 0, 100, F1), hist(binding, 10, 100, 200, F2)
    assert s2.counts == [10] * 10
    s += s2
    assert s.bounds == (0.0, 200.0) and s.counts == [15] + [20] * 8 + [25]
    assert hist(binding, 7, 90, 110).is_empty()


def test_histogram_test_dates():   # :517-624
    s = hist("date", 24, DAY0, DAY0 + 2 * 86400000, D1)
    assert s.counts == [10] * 2 + [8] * 10 + [0] * 12
    s2 = hist("date", 24, DAY0, DAY0 + 2 * 86400000, D2)
    assert s2.counts[:12] == [0] * 12 and s2.counts[15] == 10
    assert all(s2.counts[i] == 8 for i in list(range(12, 14)) + list(range(16, 24)))
    s += s2
    assert all(s.counts[i] == 10 for i in (0, 1, 15))
    assert all(s.counts[i] == 8 for i in list(range(2, 14)) + list(range(16, 24)))
    day = 86400000
    w = hist("date", 4, DAY0, DAY0 + 28 * day - 1, [DAY0 + (i - 1) * day + day // 2 for i in range(1, 29)])
    w2 = hist("date", 5, DAY0, DAY0 + 35 * day - 1, [DAY0 + (i - 1) * day + day // 2 for i in range(29, 36)])
    assert w.counts == [7] * 4 and w2.counts == [0] * 4 + [7]
    w += w2
    assert w.length == 5 and w.counts == [7] * 5


# ---------------------------------------------------------------------- MinMaxTest.scala
CARDINALITY = {"int": (99, 202), "long": (99, 202), "float": (102, 200), "double": (102, 194)}


@pytest.mark.parametrize("binding", ["int", "long", "float", "double"])
def test_minmax_test_answers(binding):
    def bounds(values):
        mn, mx = R.minmax_ref(binding, values)
        return (mn, mx) if binding in R.WHOLE else (R.key_value(mn), R.key_value(mx))
    assert bounds(F1) == (0, 99) and bounds(F2) == (100, 199) and bounds(F1 + F2) == (0, 199)
    assert bounds(range(-100, 0)) == (-100, -1)
    c100 = R.hll_cardinality(R.hll_registers(binding, F1))
    c200 = R.hll_cardinality(R.hll_registers(binding, F2, registers=R.hll_registers(binding, F1)))
    assert (c100, c200) == CARDINALITY[binding]
    assert abs(c100 - 100) <= 5                                        # MinMaxTest.scala: beCloseTo(100L, 5)
    assert abs(c200 - 200) <= (10 if binding == "double" else 5)       # :382 loosens the doubles' to 10
    assert R.hll_cardinality([0] * 1024) == 0


def test_minmax_compare_to_order():
    v = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 3.5]
    mn, mx = R.minmax_ref("double", v)
    assert R.key_value(mn) == -float("inf") and math.isnan(R.key_value(mx))
    mn, mx = R.minmax_ref("double", [0.0, -0.0])
    assert math.copysign(1, R.key_value(mn)) == -1 and math.copysign(1, R.key_value(mx)) == 1
    xs = [-float("inf"), -1e300, -2.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, float("inf"), float("nan")]
    keys = [R.order_key(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)            # Double.compareTo's order
    assert all(R.order_key(R.key_value(k)) == k for k in keys)             # the map is its own inverse
    assert R.order_key(struct.unpack("<d", struct.pack("<q", -1))[0]) == keys[-1]   # every NaN is the canonical one
    # a stat that saw only Int.MaxValue still holds its start value: it reads as empty
    assert R.minmax_ref("int", [R.INT_MAX])[0] == R.minmax_start("int")[0]
    with pytest.raises(NotImplementedError):
        R.hll_registers("date", [1])


# ---------------------------------------------------------------------- the library's host entries
@pytest.fixture(scope="module")
def lib():
    from geomesa_amd import build
    build.build(verbose=False)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gm_hist_index_of", "gm_hist_bin_bounds", "gm_hist_median", "gm_hist_copy_into", "gm_hist_merge"):
        f = getattr(so, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    so.gm_last_error.restype = ctypes.c_char_p
    return so


def state_of(binding, bins):
    if binding in R.WHOLE:
        return _lib.HistState(ATTR[binding], bins.length, int(bins.lo), int(bins.hi), 0.0, 0.0)
    return _lib.HistState(ATTR[binding], bins.length, 0, 0, float(bins.lo), float(bins.hi))


def state_bounds(binding, st):
    return (st.lo, st.hi) if binding in R.WHOLE else (st.flo, st.fhi)


def observed(binding, length, bounds, values):
    return R.RefHistogram(binding, length, bounds).observe(as_list(binding, values))


@pytest.mark.parametrize("binding", R.BINDINGS)
def test_host_entries_match_reference_loop(lib, binding):
    rng = np.random.default_rng(3)
    dt = R.DTYPE[binding]
    for length in LENGTHS:
        for name, (bounds, values) in inputs(binding, 60).items():
            h = observed(binding, length, bounds, values)
            st = state_of(binding, h.bins)
            idx = np.zeros(len(values), np.int32)
            v = np.ascontiguousarray(values)
            assert lib.gm_hist_index_of(ctypes.byref(st), v.ctypes.data, len(v), idx.ctypes.data) == 0
            assert idx.tolist() == [h.bins.index_of(R.native(binding, x)) for x in as_list(binding, values)], name
            for i in sorted({0, 1 % (length + 1), length // 2, length - 1, length}):
                out, iv, fv = _lib.HistState(), ctypes.c_int64(), ctypes.c_double()
                assert lib.gm_hist_bin_bounds(ctypes.byref(st), i, ctypes.byref(out)) == 0
                assert lib.gm_hist_median(ctypes.byref(st), i, ctypes.byref(iv), ctypes.byref(fv)) == 0
                lo, hi = h.bins.bin_bounds(i)
                med = h.bins.median_value(i)
                got = state_bounds(binding, out)
                want = (float(lo), float(hi)) if binding not in R.WHOLE else (lo, hi)
                assert all(a == b or (a != a and b != b) for a, b in zip(got, want)), (name, length, i)
                gm = iv.value if binding in R.WHOLE else fv.value
                assert gm == med or (gm != gm and med != med), (name, length, i)
            # copyInto and += against another histogram of another shape
            other = observed(binding, int(rng.integers(1, 30)), (40, 900), rng.normal(300, 400, 80).astype(dt))
            to_counts = np.array([int(c) for c in rng.integers(0, 50, length)], np.int64)
            want = to_counts.tolist()
            try:
                R.copy_into(h.bins, want, other.bins, other.counts)
            except ValueError:
                want = None
            so = state_of(binding, other.bins)
            oc = np.array(other.counts, np.int64)
            rc = lib.gm_hist_copy_into(ctypes.byref(st), to_counts.ctypes.data, ctypes.byref(so), oc.ctypes.data)
            assert (rc == 0) == (want is not None) and (want is None or to_counts.tolist() == want), name
            a = np.array(h.counts + [0] * max(0, other.length - length), np.int64)
            sa = state_of(binding, h.bins)
            try:
                h += other
            except ValueError:
                h = None
            rc = lib.gm_hist_merge(ctypes.byref(sa), a.ctypes.data, ctypes.byref(so), oc.ctypes.data)
            assert (rc == 0) == (h is not None), name
            if h is not None:
                assert sa.length == h.length and a[:sa.length].tolist() == h.counts, name
                assert same_bounds(state_bounds(binding, sa), [float(b) if binding not in R.WHOLE else b for b in h.bounds])


def test_host_entries_reject(lib):
    st = _lib.HistState(_lib.GM_ATTR_INT64, 4, 10, 10, 0.0, 0.0)
    out = _lib.HistState()
    assert lib.gm_hist_bin_bounds(ctypes.byref(st), 0, ctypes.byref(out)) == _lib.GM_E_INVALID
    assert b"upper bound must be greater" in lib.gm_last_error()
    st = _lib.HistState(_lib.GM_ATTR_INT64, 0, 0, 10, 0.0, 0.0)
    assert lib.gm_hist_bin_bounds(ctypes.byref(st), 0, ctypes.byref(out)) == _lib.GM_E_INVALID
    assert b"length must be at least 1" in lib.gm_last_error()
    st = _lib.HistState(_lib.GM_ATTR_UTF8, 4, 0, 10, 0.0, 0.0)
    assert lib.gm_hist_bin_bounds(ctypes.byref(st), 0, ctypes.byref(out)) == _lib.GM_E_INVALID
    assert b"GM_ATTR_UTF8" in lib.gm_last_error()
    st = _lib.HistState(_lib.GM_ATTR_INT64, 4, 0, 10, 0.0, 0.0)
    assert lib.gm_hist_bin_bounds(ctypes.byref(st), 5, ctypes.byref(out)) == _lib.GM_E_INVALID
    assert b"index out of range" in lib.gm_last_error()


def test_replay_check_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed to build tools/hist_replay_check.cpp")
    exe = str(tmp_path / "hist_replay_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "hist_replay_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("bad 0"), out.stdout


# ---------------------------------------------------------------------- the Python classes, host side
def cpu_hist(binding, length, bounds, values):
    """A host-only stats.Histogram holding what restatement (a) computes."""
    import torch
    from geomesa_amd.stats import Histogram
    ref = observed(binding, length, bounds, np.asarray(values, R.DTYPE[binding]))
    h = Histogram("attr", length, ref.bounds, binding, device="cpu")
    h.counts = torch.tensor(ref.counts, dtype=torch.int64)
    return h, ref


@pytest.mark.parametrize("binding", R.BINDINGS)
def test_class_merges_match_reference_loop(lib, binding):
    a, ra = cpu_hist(binding, 20, (-100, 300), F1)
    b, rb = cpu_hist(binding, 10, (50, 249), F2)
    plus = a + b
    a.add_counts_from(b)
    kept = list(ra.counts)
    R.copy_into(ra.bins, kept, rb.bins, rb.counts)
    assert a.bounds == ra.bounds and a.counts.tolist() == kept
    ra += rb
    assert plus.length == ra.length and plus.counts.tolist() == ra.counts
    assert same_bounds(plus.bounds, [float(x) if binding not in R.WHOLE else x for x in ra.bounds])
    assert plus.bin_bounds(3) == tuple(float(x) if binding not in R.WHOLE else x for x in ra.bins.bin_bounds(3))
    assert plus.median_value(3) == ra.bins.median_value(3)
    assert plus.index_of(120) == ra.bins.index_of(R.native(binding, 120))
    assert plus.direct_index(120) == (-1 if binding in ("float", "double") else ra.bins.index_of(120))
    j = plus.to_json_object()
    assert [x["count"] for x in j["bins"]] == ra.counts and j["bins"][3]["index"] == 3
    assert plus.is_equivalent(plus) and not plus.is_equivalent(a) and not plus.is_empty()
    plus.clear()
    assert plus.is_empty()


def test_class_scope():
    from geomesa_amd.stats import Count, Histogram, MinMax
    for binding in ("String", "geometry"):
        with pytest.raises(NotImplementedError):
            Histogram("a", 10, (0, 1), binding)
        with pytest.raises(NotImplementedError):
            MinMax("a", binding)
    with pytest.raises(NotImplementedError):
        Histogram("a", 10, (0, 1), device="cpu").observe(np.array(["x", "y"]))
    with pytest.raises(ValueError):
        Histogram("a", 10, (5, 5), "long", device="cpu")
    d = MinMax("dtg", "date", device="cpu")
    with pytest.raises(NotImplementedError):
        d.cardinality
    assert d.is_empty() and d.to_json_object() == {"min": None, "max": None, "cardinality": 0}
    c = Count()
    assert c.is_empty() and c.to_json_object() == {"count": 0}
    c.observe(41)
    c += Count(1)
    assert (c + Count(8)).count == 50 and c.count == 42 and c.is_equivalent(Count(42))
    c.unobserve(2)
    assert c.to_json_object() == {"count": 40}
    c.clear()
    assert c.is_empty()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from geomesa_amd.stats import Count, MinMax
        same, _ = cpu_hist("long", 10, (0, 199), [F1, F2][rank])            # equal shapes: bin-wise
        same.all_reduce(dist)
        diff, _ = cpu_hist("double", [20, 10][rank], [(-100, 300), (50, 249)][rank], [F1, F2][rank])
        diff.all_reduce(dist)                                                # += in rank order
        mm = MinMax("a", "double", device="cpu")
        mm._slots = torch.tensor(R.minmax_ref("double", [[-0.0, 4.0], [0.0, -7.5]][rank]), dtype=torch.int64)
        mm.registers = torch.tensor(R.hll_registers("double", [F1, F2][rank]), dtype=torch.int32)
        mm.all_reduce(dist)
        c = Count(rank + 5).all_reduce(dist)
        if rank == 1:
            q.put((same.counts.tolist(), diff.bounds, diff.length, diff.counts.tolist(), mm.bounds, mm.cardinality,
                   c.count))
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_gloo(lib):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    same, bounds, length, counts, mm, card, cnt = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert same == observed("long", 10, (0, 199), np.array(F1 + F2)).counts
    want = observed("double", 20, (-100, 300), np.array(F1, np.float64))
    want += observed("double", 10, (50, 249), np.array(F2, np.float64))
    assert bounds == want.bounds and length == want.length and counts == want.counts
    assert mm == (-7.5, 4.0) and card == 194 and cnt == 11
