"""The attribute index table on the device against the restatement of tests/attr_ref.py: gm_attr_index_key,
gm_attr_key_bytes and gm_attr_sort bit for bit, AttributeTable.query against the definitional answer (ids,
n_match) and the byte store (n_scanned), the reference's AttributeIndexTest cases, the ABI contract and a
query's ids as the selection of stats.MinMax.

The four entries are registered in the case table of tests/stream_order.py (attr_streams.py), so
tests/test_gpu_streams.py runs them on a caller's stream and on Context.owned with every other entry.
Shapes: n in {0, 1, 63, 64, 65, 2 * 4096 + 5} -- the wave and block edges of the validity scan (FROWS = 4096) and
an odd tail; values from ~50 distinct ones plus the edge values, so ties exercise the tier order.
"""
import ctypes
import functools

import numpy as np
import pytest

import attr_ref as R
import attr_streams as AS   # registers the four stream cases
from geomesa_amd import _lib
from geomesa_amd import attribute as A
from geomesa_amd.keyspace import Bounds

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 2 * 4096 + 5]
BIG = SIZES[-1]
ATTR = {"int": _lib.GM_ATTR_INT32, "long": _lib.GM_ATTR_INT64, "date": _lib.GM_ATTR_INT64,
        "float": _lib.GM_ATTR_FLOAT32, "double": _lib.GM_ATTR_FLOAT64}
DTYPE = {"int": np.int32, "long": np.int64, "date": np.int64, "float": np.float32, "double": np.float64}
INF, NAN = float("inf"), float("nan")
EDGES = {"int": [-(1 << 31), -1, 0, (1 << 31) - 1], "long": [-(1 << 63), -1, 0, (1 << 63) - 1],
         "date": [-(1 << 63), -1, 0, (1 << 63) - 1],
         "float": [-INF, -1e-45, -0.0, 0.0, 1e-45, INF, NAN], "double": [-INF, -5e-324, -0.0, 0.0, 5e-324, INF, NAN]}
TIER_KIND = {None: _lib.GM_ATTR_TIER_NONE, "date": _lib.GM_ATTR_TIER_DATE, "z3": _lib.GM_ATTR_TIER_Z3}
PERIOD = {"week": 1, "month": 2}
T0 = 1388577600000          # 2014-01-01T12:00:00Z
MIN_LONG = -(1 << 63)
VOFF = 5


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def dataset(n, binding, nulls, seed=0):
    """values (numpy, DTYPE), valid (bool array or None), x, y, t_ms (valid Z3 input), shard."""
    rng = np.random.default_rng(1000 * seed + n + len(binding))
    if binding in ("float", "double"):
        pool = rng.normal(0, 100, 50)
    elif binding == "date":
        pool = T0 + rng.integers(-10**9, 10**9, 50)
    else:
        pool = rng.integers(-1000, 1000, 50)
    pool = np.concatenate([np.asarray(pool, DTYPE[binding]), np.asarray(EDGES[binding], DTYPE[binding])])
    values = pool[rng.integers(0, len(pool), n)]
    valid = {"none": None, "quarter": rng.random(n) >= 0.25, "all": np.zeros(n, bool)}[nulls]
    x, y = rng.uniform(-10, 10, n).round(1), rng.uniform(40, 50, n).round(1)
    t_ms = T0 + rng.integers(0, 40, n) * 43200000 + rng.integers(0, 3, n)      # 20 days: weeks and two months
    return values, valid, x, y, t_ms, rng.integers(0, 4, n).astype(np.uint8)


def bitmap(valid, voff=VOFF):
    bits = np.zeros(voff + len(valid), np.uint8)
    bits[voff:] = valid
    return np.packbits(bits, bitorder="little")


def pylist(values, valid):
    return [None if (valid is not None and not valid[i]) else values[i].item() for i in range(len(values))]


# ---------------------------------------------------------------- gm_attr_index_key
@pytest.mark.parametrize("nulls", ["none", "quarter", "all"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("binding", list(ATTR))
def test_index_key(gpu, binding, n, nulls):
    import torch
    values, valid, *_ = dataset(n, binding, nulls)
    vt = dev(values) if n else None
    bits = None if valid is None else dev(bitmap(valid))
    col = _lib.AttrColumn(ATTR[binding], 0, vt.data_ptr() if n else None, None, None if bits is None else bits.data_ptr(),
                          VOFF if bits is not None else 0)
    v = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    m = ctypes.c_int64(-7)
    rc = gpu.lib.gm_attr_index_key(gpu.handle, ctypes.byref(col), n, p(v), p(rows), ctypes.byref(m))
    assert rc == _lib.GM_OK, _lib.last_error()
    want_rows = [i for i in range(n) if valid is None or valid[i]]
    want_v = R.ordered_column([values[i] for i in want_rows], binding)
    k = len(want_rows)
    assert m.value == k
    assert rows[:k].cpu().tolist() == want_rows
    assert np.array_equal(v[:k].cpu().numpy().view(np.uint64), want_v)
    assert (v[k:] == -7).all() and (rows[k:] == -7).all()           # nothing past the row count


# ---------------------------------------------------------------- gm_attr_key_bytes, gm_attr_sort
def key_columns(n, binding, tier, shards, period="week"):
    """Unsorted table columns of the non-null rows of the quarter-null dataset, and the restatement's rows."""
    import oracle as O
    values, valid, x, y, t_ms, shard = dataset(n, binding, "quarter")
    rows = np.flatnonzero(valid)
    v = R.ordered_column(values[rows], binding)
    if tier == "date":
        t_ms = np.where(np.arange(n) % 7 == 0, MIN_LONG, t_ms)          # null dates: Long.MinValue
    b = z = None
    if tier == "z3":
        b, z = np.zeros(n, np.int16), np.zeros(n, np.int64)
        if n:
            b, z, st = O.z3_index_key_batch(x, y, t_ms, period=PERIOD[period])
            assert not st.any()
        tiers = [R.tier_z3(b[i], z[i]) for i in rows]
        b, z = b[rows], z[rows]
    elif tier == "date":
        tiers = [R.tier_date(t_ms[i]) for i in rows]
    else:
        tiers = [b""] * len(rows)
    keys = [R.row_key(values[i].item(), binding, tiers[k], int(shard[i]) if shards else None) for k, i in enumerate(rows)]
    return v, (shard[rows] if shards else None), b, z, t_ms[rows], keys


@pytest.mark.parametrize("shards", [0, 4])
@pytest.mark.parametrize("tier", [None, "date", "z3"])
@pytest.mark.parametrize("binding,n", [("int", BIG), ("double", BIG), ("float", 65), ("long", 1), ("date", 0)])
def test_key_bytes(gpu, binding, n, tier, shards):
    import torch
    v, sh, b, z, t_ms, keys = key_columns(n, binding, tier, shards)
    m = len(v)
    klen = (1 if shards else 0) + R.HEX[binding] + 1 + {None: 0, "date": 8, "z3": 10}[tier]
    assert 9 <= klen <= 28
    out = torch.full((m * klen + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    t = z if tier == "z3" else (t_ms if tier == "date" else None)
    cols = [None if a is None else dev(a) for a in (sh, v.view(np.int64), b, t)]
    rc = gpu.lib.gm_attr_key_bytes(gpu.handle, ATTR[binding], p(cols[0]), p(cols[1]), TIER_KIND[tier], p(cols[2]), p(cols[3]),
                                   m, p(out))
    assert rc == _lib.GM_OK and gpu.lib.gm_ctx_sync(gpu.handle) == _lib.GM_OK, _lib.last_error()
    got = out.cpu().numpy()
    assert got[:m * klen].tobytes() == b"".join(keys)
    assert (got[m * klen:] == 0xA5).all()


@pytest.mark.parametrize("shards", [0, 4])
@pytest.mark.parametrize("tier", [None, "date", "z3"])
@pytest.mark.parametrize("n", [1, 65, BIG])
def test_sort(gpu, n, tier, shards):
    import torch
    v, sh, b, z, t_ms, keys = key_columns(n, "int", tier, shards)
    m = len(v)
    t = z if tier == "z3" else ((t_ms.view(np.uint64) ^ np.uint64(1 << 63)).view(np.int64) if tier == "date" else None)
    ins = [None if a is None else dev(a) for a in (sh, v.view(np.int64), b, t)]
    outs = [None if a is None else torch.empty_like(a) for a in ins]
    perm = torch.empty(max(m, 1), dtype=torch.int64, device="cuda")
    rc = gpu.lib.gm_attr_sort(gpu.handle, *(p(a) for a in ins), m, *(p(a) for a in outs), p(perm))
    assert rc == _lib.GM_OK, _lib.last_error()
    zero = np.zeros(m, np.int64)
    order = AS.table_order(sh if shards else zero.astype(np.uint8), v, b if b is not None else zero.astype(np.int16),
                           t if t is not None else zero)
    assert perm[:m].cpu().tolist() == order.tolist()
    assert order.tolist() == sorted(range(m), key=lambda i: keys[i])          # the byte store's order, stable
    for got, col in zip(outs, (sh, v.view(np.int64), b, t)):
        if col is not None:
            assert np.array_equal(got.cpu().numpy(), col[order])


# ---------------------------------------------------------------- AttributeTable
CONFIGS = {      # binding, tier, shards, nulls, period, n
    "int-z3-sharded": ("int", "z3", 4, "quarter", "week", BIG),
    "float-z3-month": ("float", "z3", 0, "none", "month", BIG),
    "double-date": ("double", "date", 0, "quarter", "week", BIG),
    "date-date-sharded": ("date", "date", 4, "none", "week", BIG),
    "long-none-sharded": ("long", None, 4, "quarter", "week", BIG),
    "int-z3-65": ("int", "z3", 0, "quarter", "week", 65),
    "int-date-64": ("int", "date", 4, "quarter", "week", 64),
    "double-none-63": ("double", None, 0, "none", "week", 63),
    "int-z3-1": ("int", "z3", 4, "none", "week", 1),
    "int-z3-0": ("int", "z3", 0, "none", "week", 0),
    "int-z3-all-null": ("int", "z3", 4, "all", "week", 65),
}


@functools.lru_cache(maxsize=None)
def built(name):
    """(AttributeTable, the restatement's Store, the columns as Python lists)."""
    import oracle as O
    binding, tier, shards, nulls, period, n = CONFIGS[name]
    values, valid, x, y, t_ms, shard = dataset(n, binding, nulls)
    if tier == "date":
        t_ms = np.where(np.arange(n) % 7 == 0, MIN_LONG, t_ms)
    table = A.AttributeTable(values, binding, validity=None if valid is None else bitmap(valid), x=x, y=y, t_ms=t_ms,
                             tier=tier, shard=shard if shards else None, period=period, validity_offset=VOFF,
                             shards=shards or None)
    vals = pylist(values, valid)
    if tier == "z3" and n:
        b, z, st = O.z3_index_key_batch(x, y, t_ms, period=PERIOD[period])
        tiers = [R.tier_z3(b[i], z[i]) for i in range(n)]
    elif tier == "date":
        tiers = [R.tier_date(t) for t in t_ms.tolist()]
    else:
        tiers = [b""] * n
    store = R.Store([R.row_key(vals[i], binding, tiers[i], int(shard[i]) if shards else None) for i in range(n)])
    return table, store, (vals, x.tolist(), y.tolist(), t_ms.tolist())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_table_order_and_key_bytes(gpu, name):
    table, store, _ = built(name)
    assert table.n == len(store.keys)
    assert table.perm.cpu().tolist() == store.order                     # table row -> input row
    kb = table.key_bytes().cpu().numpy()
    rows = [kb[i].tobytes() for i in range(table.n)]
    assert rows == store.keys
    assert all(a <= b for a, b in zip(rows, rows[1:]))                  # non-decreasing by byte comparison


def pick(vals, k):
    """The k-th distinct non-null, non-NaN value in key-text order (wraps)."""
    d = sorted({v for v in vals if v is not None and v == v})
    return d[k % len(d)] if d else 0


def range_kinds(vals):
    a, b, c = pick(vals, 10), pick(vals, 30), pick(vals, 20)
    lo, hi = min(a, b), max(a, b)
    return {
        "equality": [(a, True, a, True)], "in": [(a, True, a, True), (b, True, b, True), (c, True, c, True)],
        "lt": [(None, False, b, False)], "le": [(None, False, b, True)], "gt": [(a, False, None, False)],
        "ge": [(a, True, None, False)], "between": [(lo, True, hi, True)], "open": [(lo, False, hi, False)],
        "not_null": [(None, False, None, False)], "unbounded": [], "disjoint": "disjoint",
    }


BOX1 = [(-5.0, 42.0, 5.0, 48.0)]
BOX2 = [(-5.0, 42.0, 0.0, 45.0), (2.5, 44.0, 9.0, 49.5)]           # 2.5 and 49.5 fall on points (inclusive)


def secondaries(t_list):
    """(bboxes, intervals) pairs; an interval whose ends fall on a row's exact millisecond (exclusive)."""
    ts = sorted(t for t in t_list if t != MIN_LONG)
    a, b = (ts[len(ts) // 4], ts[3 * len(ts) // 4]) if ts else (T0, T0 + 1)
    during = [(a, False, b, False)]
    return [(None, None), (BOX1, None), (None, during), (BOX1, during), (BOX2, during),
            (None, [(a, True, None, False)]), (BOX1, [(None, False, b, True)])]


def check_query(table, store, cols, binding, tier, shards, period, bounds, bboxes, intervals, map_rows=True):
    vals, x, y, t = cols
    iv = None if intervals is None else [Bounds(lo, hi, li, ui) for lo, li, hi, ui in intervals]
    ids, n_match, n_scanned = table.query(bounds, bboxes, iv, map_rows=map_rows)
    want = R.definition(store, vals, binding, bounds, x, y, t, bboxes, intervals)
    plan = R.plan(bounds, binding, tier, shards, bboxes, intervals, PERIOD[period])
    cand = store.candidates(plan)
    what = (bounds, bboxes, intervals)
    assert n_scanned == len(cand), what
    assert n_match == len(want), what
    if map_rows:
        assert ids.cpu().tolist() == want, what
    else:
        assert [store.order[r] for r in ids.cpu().tolist()] == want, what
    assert set(want) <= {store.order[r] for r in cand}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_query(gpu, name):
    """Every range kind x every secondary filter the tier can take: ids and n_match equal the definitional
    answer, n_scanned the byte store's candidate count."""
    binding, tier, shards, nulls, period, n = CONFIGS[name]
    table, store, cols = built(name)
    for kind, bounds in range_kinds(cols[0]).items():
        for bboxes, intervals in secondaries(cols[3]):
            check_query(table, store, cols, binding, tier, shards, period, bounds, bboxes, intervals)
    check_query(table, store, cols, binding, tier, shards, period, range_kinds(cols[0])["between"], BOX1, None, map_rows=False)
    check_query(table, store, cols, binding, tier, shards, period, [], None, None, map_rows=False)


def test_float_zero_and_nan_keys(gpu):
    """-0.0 and +0.0 are different keys, NaN is a key above +inf."""
    table, store, cols = built("float-z3-month")
    for v in (-0.0, 0.0, NAN, INF):
        check_query(table, store, cols, "float", "z3", 0, "month", [(v, True, v, True)], None, None)
    ids, n0, _ = table.query([(0.0, True, 0.0, True)])
    ids, n1, _ = table.query([(-0.0, True, -0.0, True)])
    ids, n2, _ = table.query([(-0.0, True, 0.0, True)])
    assert n0 > 0 and n1 > 0 and n2 == n0 + n1


def test_attribute_index_test_cases(gpu):
    """AttributeIndexTest.scala:83-109, 202-221, 335-359 through the device."""
    import test_attr_reference as T
    during = [Bounds(T.ST_DURING[0][0], T.ST_DURING[0][2], False, False)]
    names = lambda ids: [T.NAMES[i] for i in ids.cpu().tolist()]
    for shard in (None, T.SHARD):
        height = A.AttributeTable(T.HEIGHT, "float", x=T.X, y=T.Y, t_ms=T.DTG, tier="z3", shard=shard)
        assert names(height.query([(12.0, True, 12.0, True)], T.ST_BOX, during)[0]) == ["bob"]
        assert sorted(names(height.query([(12.0, True, 12.0, True)])[0])) == ["bob", "charles"]
        after = [Bounds(T.ms("2014-01-01T11:45:00.000Z"), None, False, False)]
        plan = height.plan([(12.0, True, 12.0, True)], None, after)
        assert plan and all(len(r.lower) > (1 if shard else 0) + 8 + 1 for r in plan)
        assert sorted(names(height.query([(12.0, True, 12.0, True)], None, after)[0])) == ["bob", "charles"]
        valid = np.packbits(np.array([1, 1, 1, 0], np.uint8), bitorder="little")
        age3 = A.AttributeTable([20, 21, 30, 0], "int", validity=valid, x=T.X, y=T.Y, t_ms=T.DTG, tier="z3", shard=shard)
        assert age3.n == 3 and names(age3.query([(30, True, 30, True)], T.ST_BOX, during)[0]) == ["bob"]
        age = A.AttributeTable([20, 21, 30, 0], "int", validity=valid, t_ms=T.DTG, tier="date", shard=shard)
        t = T.ms("2014-01-01T12:00:00.000Z")
        for iv in (Bounds(t, t, True, True), Bounds(t - 1, t + 1, False, False), Bounds(t, t + 1, True, False)):
            assert names(age.query([(30, True, 30, True)], None, [iv])[0]) == ["bob"]


# ---------------------------------------------------------------- ABI contract
def scan_args(table, arr, flt=None, ids=None, cap=None, nm=None, ns=None, perm=True):
    return (table.ctx.handle, p(table.shard), p(table.v), p(table.bin), p(table.t), table.n, arr.ctypes.data, len(arr),
            None if flt is None else ctypes.byref(flt), p(table.perm) if perm else None, p(ids), cap,
            None if nm is None else ctypes.byref(nm), None if ns is None else ctypes.byref(ns))


def test_abi_contract(gpu):
    import torch
    lib = gpu.lib
    table, store, cols = built("int-z3-sharded")
    arr = A.attr_ranges(table.plan([]), table.layout)
    nm, ns = ctypes.c_int64(-7), ctypes.c_int64(-7)
    # GM_E_CAPACITY with the true count; nothing past ids_cap is written
    ids = torch.full((table.n,), -7, dtype=torch.int64, device="cuda")
    assert lib.gm_attr_table_scan(*scan_args(table, arr, None, ids, 10, nm, ns)) == _lib.GM_E_CAPACITY
    assert nm.value == ns.value == table.n and ids[:10].cpu().tolist() == store.order[:10] and (ids[10:] == -7).all()
    # counting only: ids NULL; no counts: both NULL
    assert lib.gm_attr_table_scan(*scan_args(table, arr, None, None, 0, nm, None)) == _lib.GM_OK and nm.value == table.n
    assert lib.gm_attr_table_scan(*scan_args(table, arr, None, ids, table.n, None, None)) == _lib.GM_OK
    assert ids.cpu().tolist() == store.order
    # ids_cap < 0, a NULL range array, a NULL context
    assert lib.gm_attr_table_scan(*scan_args(table, arr, None, ids, -1, nm, ns)) == _lib.GM_E_INVALID
    bad = list(scan_args(table, arr, None, ids, table.n, nm, ns))
    bad[6] = None
    assert lib.gm_attr_table_scan(*bad) == _lib.GM_E_INVALID
    bad = list(scan_args(table, arr, None, ids, table.n, nm, ns))
    bad[0] = None
    assert lib.gm_attr_table_scan(*bad) == _lib.GM_E_INVALID
    # a misaligned column
    bad = list(scan_args(table, arr, None, ids, table.n, nm, ns))
    bad[2] = ctypes.c_void_p(table.v.data_ptr() + 4)
    assert lib.gm_attr_table_scan(*bad) == _lib.GM_E_INVALID and "alignment" in _lib.last_error()
    # a filter carrying z3filter or polys
    blob = (ctypes.c_uint8 * 8)()
    for field in ("z3filter", "z2filter", "polys"):
        f = _lib.ScanFilter()
        setattr(f, field, ctypes.addressof(blob))
        assert lib.gm_attr_table_scan(*scan_args(table, arr, f, ids, table.n, nm, ns)) == _lib.GM_E_INVALID
        assert "gm_attr_table_scan" in _lib.last_error()
    # boxes without their columns
    f = _lib.ScanFilter()
    f.n_boxes = 1
    assert lib.gm_attr_table_scan(*scan_args(table, arr, f, ids, table.n, nm, ns)) == _lib.GM_E_INVALID
    # GM_ATTR_UTF8 refused with a message, by both entries that take the type
    col = _lib.AttrColumn(_lib.GM_ATTR_UTF8, 0, table.v.data_ptr(), None, None, 0)
    m = ctypes.c_int64()
    assert lib.gm_attr_index_key(gpu.handle, ctypes.byref(col), 4, p(ids), p(ids), ctypes.byref(m)) == _lib.GM_E_INVALID
    assert "GM_ATTR_UTF8" in _lib.last_error()
    out = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert lib.gm_attr_key_bytes(gpu.handle, _lib.GM_ATTR_UTF8, None, p(table.v), 0, None, None, 1, p(out)) == _lib.GM_E_INVALID
    assert "GM_ATTR_UTF8" in _lib.last_error()
    assert lib.gm_attr_key_bytes(gpu.handle, _lib.GM_ATTR_INT32, None, p(table.v), 3, None, None, 1, p(out)) == _lib.GM_E_INVALID
    # the misaligned column of gm_attr_index_key, and the NULL pairs of gm_attr_sort
    col = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, table.v.data_ptr() + 4, None, None, 0)
    assert lib.gm_attr_index_key(gpu.handle, ctypes.byref(col), 4, p(ids), p(ids), ctypes.byref(m)) == _lib.GM_E_INVALID
    s = [p(table.shard), p(table.v), p(table.bin), p(table.t)]
    o = [p(torch.empty_like(table.shard)), p(torch.empty_like(table.v)), p(torch.empty_like(table.bin)), p(torch.empty_like(table.t))]
    for k in (0, 2, 3):
        half = list(o)
        half[k] = None
        assert lib.gm_attr_sort(gpu.handle, *s, table.n, *half, p(ids)) == _lib.GM_E_INVALID
    with pytest.raises(NotImplementedError):
        A.AttributeTable(["a"], "String")
    with pytest.raises(NotImplementedError):
        A.AttributeTable([1], "int", tier="xz3")


def test_z3_tier_reports_a_bad_row(gpu):
    """A point outside the world fails as Z3Table.from_points fails it; lenient clamps."""
    from geomesa_amd.curve import IllegalArgumentException
    x, y, t = [0.0, 181.0], [0.0, 0.0], [T0, T0]
    with pytest.raises(IllegalArgumentException):
        A.AttributeTable([1, 2], "int", x=x, y=y, t_ms=t, tier="z3")
    assert A.AttributeTable([1, 2], "int", x=x, y=y, t_ms=t, tier="z3", lenient=True).n == 2


def test_ids_drive_minmax(gpu):
    """A query's ids as the selection of stats.MinMax over the attribute column."""
    from geomesa_amd.stats import MinMax
    table, store, cols = built("double-date")
    values = dataset(BIG, "double", "quarter")[0]
    ids, n_match, _ = table.query(range_kinds(cols[0])["between"], BOX1)
    assert n_match > 10
    got = MinMax("a", "double").observe(values, ids=ids)
    sel = values[ids.cpu().numpy()]
    assert got.bounds == (float(sel.min()), float(sel.max()))
