"""gm_histogram_attr and gm_minmax_attr on the device against restatement (a) of tests/hist_ref.py (the
reference's loop, one feature at a time): counts, bounds, tally, minmax slots and registers bit for bit.

all_reduce and += of the classes are held to the restatement by tests/test_hist_reference.py (gloo, host-only
stats); here += runs once on device-resident stats.  Both entry points are registered in the case table of
tests/stream_order.py (hist_streams.py), so tests/test_gpu_streams.py runs them on a caller's stream and on
Context.owned with every other entry; test_stream_order_of_both_entries does so here as well.
"""
import ctypes

import numpy as np
import pytest

import hist_ref as R
import hist_streams   # registers the two stream cases  # noqa: F401
from geomesa_amd import _lib

pytestmark = pytest.mark.gpu

ATTR = {"int": _lib.GM_ATTR_INT32, "long": _lib.GM_ATTR_INT64, "date": _lib.GM_ATTR_INT64,
        "float": _lib.GM_ATTR_FLOAT32, "double": _lib.GM_ATTR_FLOAT64}
BLOCK = 4096                      # FROWS: units per block of pass R, per tile of pass C
SEGS = _lib.GM_HIST_MAX_SEGMENTS
LDS_BINS = _lib.GM_HIST_LDS_BINS


# ---------------------------------------------------------------------- plumbing
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def column(binding, values, valid=None, voff=0, misalign=False):
    """(gm_attr_column, the tensors it points into).  misalign: the values start 4 bytes past a 16-B boundary
    (4-byte columns only)."""
    import torch
    v = np.ascontiguousarray(values, R.DTYPE[binding])
    keep = []
    if misalign:
        assert v.itemsize == 4
        t = torch.zeros(v.size + 1, dtype=getattr(torch, v.dtype.name), device="cuda")
        t[1:] = torch.from_numpy(v.copy()).cuda()
        vp = t.data_ptr() + 4
    else:
        t = dev(v)
        vp = t.data_ptr()
    keep.append(t)
    bits = None
    if valid is not None:
        b = np.zeros(voff + len(v), np.uint8)
        b[voff:] = np.asarray(valid, np.uint8)
        bits = dev(np.packbits(b, bitorder="little"))
        keep.append(bits)
    col = _lib.AttrColumn(ATTR[binding], 0, vp if v.size else None, None, bits.data_ptr() if bits is not None else None, voff)
    return col, keep


def selection(n, mask=None, ids=None):
    """(mask words, ids tensor, n_ids, the selected units in order as (row or None for a bad id))."""
    if mask is not None:
        m = np.asarray(mask, bool)
        words = np.packbits(np.concatenate([m, np.zeros(-len(m) % 64, bool)]), bitorder="little").view(np.uint64)
        return dev(words), None, 0, [int(r) for r in np.flatnonzero(m)]
    if ids is not None:
        ids = np.asarray(ids, np.int64)
        t = dev(ids if ids.size else np.zeros(1, np.int64))
        return None, t, len(ids), [int(r) if 0 <= r < n else None for r in ids]
    return None, None, 0, list(range(n))


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def state_of(binding, length, bounds):
    if binding in R.WHOLE:
        return _lib.HistState(ATTR[binding], length, int(bounds[0]), int(bounds[1]), 0.0, 0.0)
    return _lib.HistState(ATTR[binding], length, 0, 0, float(bounds[0]), float(bounds[1]))


def device_hist(gpu, binding, values, length, bounds, valid=None, voff=0, mask=None, ids=None, sign=1, path=0,
                counts0=None, misalign=False):
    """One gm_histogram_attr call -> (bounds, counts, tally)."""
    import torch
    col, keep = column(binding, values, valid, voff, misalign)
    n = len(values)
    m, i, n_ids, _ = selection(n, mask, ids)
    st = state_of(binding, length, bounds)
    counts = dev(np.zeros(length, np.int64) if counts0 is None else np.asarray(counts0, np.int64))
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    rc = gpu.lib.gm_histogram_attr(gpu.handle, ctypes.byref(col), n, p(m), p(i), n_ids, sign, path, ctypes.byref(st),
                                   p(counts), p(tally))
    assert rc == _lib.GM_OK, _lib.last_error()
    got = (st.lo, st.hi) if binding in R.WHOLE else (st.flo, st.fhi)
    return got, counts.cpu().tolist(), tally.cpu().tolist()


def ref_hist(binding, values, length, bounds, valid=None, mask=None, ids=None, sign=1, counts0=None):
    """Restatement (a) over the selected non-null rows in selection order -> (bounds, counts, tally)."""
    _, _, _, units = selection_host(len(values), mask, ids)
    h = R.RefHistogram(binding, length, bounds)
    if counts0 is not None:
        h.counts = [int(c) for c in counts0]
    v = np.asarray(values, R.DTYPE[binding])
    rows = [r for r in units if r is not None and (valid is None or valid[r])]
    seq = v[rows]
    h.observe(seq if binding == "float" else seq.tolist(), sign=sign)
    lo, hi = h.bounds
    b = (lo, hi) if binding in R.WHOLE else (float(lo), float(hi))
    return b, h.counts, [h.observed, h.expansions, sum(r is None for r in units)]


def selection_host(n, mask, ids):
    if mask is not None:
        return None, None, 0, [int(r) for r in np.flatnonzero(np.asarray(mask, bool))]
    if ids is not None:
        return None, None, 0, [int(r) if 0 <= r < n else None for r in ids]
    return None, None, 0, list(range(n))


def same(a, b):
    """Bit for bit: bounds compare with their sign of zero."""
    return a[1] == b[1] and a[2] == b[2] and all(
        x == y and np.signbit(float(x)) == np.signbit(float(y)) for x, y in zip(a[0], b[0]))


def check(gpu, binding, values, length, bounds, **kw):
    refkw = {k: v for k, v in kw.items() if k in ("valid", "mask", "ids", "sign", "counts0")}
    got = device_hist(gpu, binding, values, length, bounds, **kw)
    want = ref_hist(binding, values, length, bounds, **refkw)
    assert same(got, want), (binding, length, kw.get("path"), got[0], want[0], got[2], want[2],
                             [(i, a, b) for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:5])
    return got


def bell(binding, n, seed=0, sigma=1000.0):
    return np.random.default_rng(seed).normal(0, sigma, n).astype(R.DTYPE[binding])


# ---------------------------------------------------------------------- unit counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17])
@pytest.mark.parametrize("binding", R.BINDINGS)
def test_unit_counts(gpu, binding, n):
    got = check(gpu, binding, bell(binding, n, n), 7, (-100, 100))
    assert got[2][0] == n


@pytest.mark.parametrize("binding", ["long", "double"])
def test_several_tiles_per_workgroup(gpu, binding):
    """300,001 rows: 74 tiles over the persistent workgroups, records in a few of them."""
    got = check(gpu, binding, bell(binding, 300_001, 5), 1000, (-100, 100))
    assert 5 < got[2][1] < 60


# ---------------------------------------------------------------------- records at fixed units
N_PLACED = BLOCK + 200
PLACES = {
    "block-edges": [0, 63, 64, BLOCK - 1, BLOCK, BLOCK + 1],
    "one-wave": [10, 11],
    "last-unit": [N_PLACED - 1],
    "none": [],
}


@pytest.mark.parametrize("where", list(PLACES))
@pytest.mark.parametrize("binding", ["int", "long", "float", "double"])
def test_records_at_fixed_units(gpu, binding, where):
    v = np.random.default_rng(3).uniform(-50, 50, N_PLACED).astype(R.DTYPE[binding])
    for k, u in enumerate(PLACES[where]):
        v[u] = (200 + 50 * k) * (1 if k & 1 else -1)      # alternately a new minimum and a new maximum
    got = check(gpu, binding, v, 7, (-100, 100))
    assert got[2][1] == len(PLACES[where])


@pytest.mark.parametrize("binding", ["long", "double"])
def test_repeated_extreme_is_one_record(gpu, binding):
    v = np.random.default_rng(4).uniform(-50, 50, 2 * BLOCK).astype(R.DTYPE[binding])
    v[100] = v[BLOCK + 7] = 900         # the second occurrence lies on the bound: inside
    v[200] = v[201] = -900              # and in the same wave
    got = check(gpu, binding, v, 7, (-100, 100))
    assert got[2][1] == 2 and got[0] == (-900, 900)


# ---------------------------------------------------------------------- more records than one round
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("binding", R.BINDINGS)
def test_sorted_column_takes_rounds(gpu, binding, descending):
    n = 2 * SEGS + 5
    v = (np.arange(n) * 3 + 10).astype(R.DTYPE[binding])
    if descending:
        v = -v
    got = check(gpu, binding, v, 7, (0, 1))
    assert got[2][1] == n == got[2][0]


# ---------------------------------------------------------------------- bindings x selection x validity x path x length x sign
N_X = BLOCK + 77


def _ids(n):
    rng = np.random.default_rng(9)
    ids = rng.integers(0, n, n // 2)
    ids[5], ids[6], ids[70], ids[n // 4] = ids[4], -1, n, n + 12345     # a repeat and three ids out of range
    return ids


COMBOS = [   # (selection, nulls, path, length, sign, misaligned)
    ("none", False, 1, 1, 1, False),
    ("none", True, 2, 2, -1, True),
    ("mask", True, 1, 1000, 1, False),
    ("mask", False, 2, LDS_BINS + 1, 1, True),
    ("mask", False, 0, 2, -1, False),
    ("ids", False, 1, 2, 1, True),
    ("ids", True, 2, 1000, -1, False),
    ("ids", True, 0, LDS_BINS + 1, 1, False),
    ("ids-desc", False, 1, 1000, -1, False),
    ("ids-desc", True, 2, 1, 1, True),
    ("none", True, 0, LDS_BINS, 1, False),
    ("none", False, 2, 1000, 1, False),
]


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "-".join(str(x) for x in c))
@pytest.mark.parametrize("binding", R.BINDINGS)
def test_bindings_crossed(gpu, binding, combo):
    sel, nulls, path, length, sign, misalign = combo
    if misalign and R.DTYPE[binding]().itemsize != 4:
        misalign = False
    v = bell(binding, N_X, 21)
    rng = np.random.default_rng(22)
    kw = {"path": path, "sign": sign, "misalign": misalign}
    if nulls:
        kw["valid"] = rng.random(N_X) < 0.8
        kw["voff"] = 3
    if sel == "mask":
        kw["mask"] = rng.random(N_X) < 0.4
    elif sel == "ids":
        kw["ids"] = _ids(N_X)
    elif sel == "ids-desc":
        kw["ids"] = np.sort(_ids(N_X))[::-1]
    kw["counts0"] = rng.integers(0, 40, length)      # unobserve and the expansions work on what is there
    got = check(gpu, binding, v, length, (-100, 100), **kw)
    if sel.startswith("ids"):
        assert got[2][2] == 3


# ---------------------------------------------------------------------- edge values
@pytest.mark.parametrize("binding", ["float", "double"])
def test_nan_infinity_zero(gpu, binding):
    v = bell(binding, BLOCK + 9, 31)
    v[[3, 700, BLOCK + 2]] = np.nan
    v[[5, 900]] = [-0.0, 0.0]
    got = check(gpu, binding, v, 7, (-100, 100))
    assert got[1][0] >= 3                                   # the NaN rows sit in bin 0
    v[1000], v[BLOCK + 5] = np.inf, -np.inf
    check(gpu, binding, v, 7, (-100, 100))
    check(gpu, binding, np.array([0.0, -0.0, 0.5, -0.0, 1.0, -1e-30, 0.0], R.DTYPE[binding]), 2, (0.0, 1.0))
    check(gpu, binding, np.array([-0.0, 0.25], R.DTYPE[binding]), 2, (0.0, 1.0))   # -0.0 is not below 0.0


def test_long_extremes(gpu):
    lo, hi = R.LONG_MIN, R.LONG_MAX
    check(gpu, "long", np.array([lo + 60, lo, lo + 70, 5, hi - 3, 0, hi, lo + 1, -7], np.int64), 7, (lo + 50, lo + 90))
    check(gpu, "long", np.array([hi - 60, hi, hi - 70, -5, lo + 3, 0, lo, hi - 1, 7], np.int64), 7, (hi - 90, hi - 50))
    check(gpu, "int", np.array([R.INT_MAX, R.INT_MAX - 60, R.INT_MIN, 0, R.INT_MAX], np.int32), 7,
          (R.INT_MAX - 90, R.INT_MAX - 50))


def adversarial_quotients(lo, hi, length):
    """float32 values whose quotient (v - lo) / binSize lands within one ulp of an integer, so that a division
    off by one ulp changes floor(): built from the restatement's own float32 arithmetic."""
    f = np.float32
    bins = R.Binning("float", length, (lo, hi))
    out = []
    for k in range(1, length):
        base = f(lo) + bins.bin_size * f(k)
        for v in (np.nextafter(base, f(-np.inf)), base, np.nextafter(base, f(np.inf))):
            q = (v - bins.lo) / bins.bin_size
            if abs(q - np.rint(q)) <= np.spacing(q) and bins.lo <= v <= bins.hi:
                out.append(v)
    return np.array(out, np.float32)


@pytest.mark.parametrize("bounds,length", [((0.1, 7.3), 1000), ((-3.7, 11.9), 997), ((1e-3, 1.7e-3), 333)])
def test_float32_division_is_correctly_rounded(gpu, bounds, length):
    v = adversarial_quotients(np.float32(bounds[0]), np.float32(bounds[1]), length)
    assert len(v) > length // 2
    b = R.Binning("float", length, bounds)
    on_edge = sum(b.index_of(x) != b.index_of(np.nextafter(x, np.float32(-np.inf))) for x in v[:200])
    assert on_edge > 20                                     # a neighbouring quotient does fall into the bin below
    check(gpu, "float", v, length, (np.float32(bounds[0]), np.float32(bounds[1])))
    check(gpu, "float", v, length, (np.float32(bounds[0]), np.float32(bounds[1])), path=2)


# ---------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("binding", ["int", "double"])
def test_two_calls_equal_one(gpu, binding):
    v = bell(binding, 2 * BLOCK + 300, 41)
    cut = BLOCK + 123
    b1, c1, t1 = device_hist(gpu, binding, v[:cut], 1000, (-100, 100))
    b2, c2, t2 = device_hist(gpu, binding, v[cut:], 1000, b1, counts0=c1)
    whole = ref_hist(binding, v, 1000, (-100, 100))
    assert same((b2, c2, [a + b for a, b in zip(t1, t2)]), whole)


# ---------------------------------------------------------------------- MinMax
def device_minmax(gpu, binding, values, valid=None, mask=None, ids=None, registers=True, start=None, reg0=None):
    import torch
    col, keep = column(binding, values, valid, 3 if valid is not None else 0)
    n = len(values)
    m, i, n_ids, _ = selection(n, mask, ids)
    slots = dev(np.array(start or R.minmax_start(binding), np.int64))
    reg = dev(np.zeros(1024, np.int32) if reg0 is None else np.asarray(reg0, np.int32)) if registers else None
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    rc = gpu.lib.gm_minmax_attr(gpu.handle, ctypes.byref(col), n, p(m), p(i), n_ids, p(slots), p(reg), p(tally))
    assert rc == _lib.GM_OK, _lib.last_error()
    return tuple(slots.cpu().tolist()), None if reg is None else reg.cpu().tolist(), tally.cpu().tolist()


def ref_minmax(binding, values, valid=None, mask=None, ids=None, registers=True):
    units = selection_host(len(values), mask, ids)[3]
    rows = [r for r in units if r is not None and (valid is None or valid[r])]
    seq = np.asarray(values, R.DTYPE[binding])[rows]
    reg = R.hll_registers("long" if binding == "date" else binding, seq) if registers else None
    return R.minmax_ref(binding, seq), reg, [len(rows), 0, sum(r is None for r in units)]


@pytest.mark.parametrize("sel", ["none", "mask", "ids"])
@pytest.mark.parametrize("binding", R.BINDINGS)
def test_minmax_bindings_and_selections(gpu, binding, sel):
    n = 3 * BLOCK + 17
    v = bell(binding, n, 51, 1e6)
    rng = np.random.default_rng(52)
    kw = {"valid": rng.random(n) < 0.7}
    if sel == "mask":
        kw["mask"] = rng.random(n) < 0.3
    elif sel == "ids":
        kw["ids"] = _ids(n)
    registers = binding != "date"
    assert device_minmax(gpu, binding, v, registers=registers, **kw) == ref_minmax(binding, v, registers=registers, **kw)
    assert device_minmax(gpu, binding, v[:0], registers=registers)[0] == R.minmax_start(binding)


@pytest.mark.parametrize("binding", ["float", "double"])
def test_minmax_total_order(gpu, binding):
    dt = R.DTYPE[binding]
    for v in ([0.0, -0.0], [-0.0, 0.0], [1.0, np.nan, -np.inf, np.inf], [np.nan], [-0.0], [5.0, -np.nan]):
        got = device_minmax(gpu, binding, np.array(v, dt))
        assert got == ref_minmax(binding, np.array(v, dt)), v
    mn, mx = device_minmax(gpu, binding, np.array([0.0, -0.0], dt))[0]
    assert np.signbit(R.key_value(mn)) and not np.signbit(R.key_value(mx))


def test_minmax_known_cardinalities(gpu):
    """The eight committed answers (tests/test_hist_reference.py) from the device's registers."""
    want = {"int": (99, 202), "long": (99, 202), "float": (102, 200), "double": (102, 194)}
    for binding, (c100, c200) in want.items():
        s1, r1, _ = device_minmax(gpu, binding, np.arange(100))
        s2, r2, _ = device_minmax(gpu, binding, np.arange(100, 200), start=s1, reg0=r1)
        assert (R.hll_cardinality(r1), R.hll_cardinality(r2)) == (c100, c200)
        lo, hi = s2 if binding in R.WHOLE else (R.key_value(s2[0]), R.key_value(s2[1]))
        assert (lo, hi) == (0, 199)


# ---------------------------------------------------------------------- the classes
def test_classes_on_the_device(gpu):
    from geomesa_amd.stats import Count, Histogram, MinMax
    v = bell("double", 2 * BLOCK + 5, 61)
    mask = np.random.default_rng(62).random(len(v)) < 0.5
    h = Histogram("a", 50, (-100, 100)).observe(v, mask=mask)
    want = ref_hist("double", v, 50, (-100, 100), mask=mask)
    assert h.binding == "double" and (h.bounds, h.counts.tolist(), h.expansions) == (want[0], want[1], want[2][1])
    h.unobserve(v[:100])
    want2 = ref_hist("double", v[:100], 50, want[0], sign=-1, counts0=want[1])
    assert (h.bounds, h.counts.tolist()) == (want2[0], want2[1])
    other = Histogram("a", 20, (500, 9000), "double").observe(v * 3)
    a = R.RefHistogram("double", 50, want2[0]); a.counts = list(want2[1])
    b = R.RefHistogram("double", 20, (500, 9000)).observe((v * 3).tolist())
    a += b
    h += other
    assert (h.length, h.bounds, h.counts.tolist()) == (a.length, a.bounds, a.counts)
    m = MinMax("a").observe(v, mask=mask)
    slots, reg, _ = ref_minmax("double", v, mask=mask)
    assert m.bounds == (R.key_value(slots[0]), R.key_value(slots[1])) and m.cardinality == R.hll_cardinality(reg)
    assert not m.is_empty() and m.tuple == (m.min, m.max, m.cardinality)
    only = MinMax("i", "int").observe(np.full(70, R.INT_MAX, np.int32))
    assert only.is_empty() and only.to_json_object() == {"min": None, "max": None, "cardinality": 0}
    d = MinMax("dtg", "date").observe(np.array([5, -9, 1325376000000]))
    assert d.bounds == (-9, 1325376000000)
    with pytest.raises(NotImplementedError):
        d.cardinality
    m2 = MinMax("a", "double").observe(np.array([-1e9, 4.0]))
    m2 += m
    assert m2.min == -1e9 and m2.max == m.max
    assert Count().observe(int(mask.sum())).count == int(mask.sum())


# ---------------------------------------------------------------------- errors
def test_invalid_arguments_and_their_texts(gpu):
    import torch
    lib, h = gpu.lib, gpu.handle
    v = dev(np.arange(8, dtype=np.int64))
    counts, tally = dev(np.zeros(4, np.int64)), torch.zeros(3, dtype=torch.int64, device="cuda")
    words, ids = dev(np.zeros(1, np.uint64)), dev(np.zeros(2, np.int64))
    slots = dev(np.array(R.minmax_start("long"), np.int64))

    def col(t=_lib.GM_ATTR_INT64, ptr_=None):
        return _lib.AttrColumn(t, 0, v.data_ptr() if ptr_ is None else ptr_, None, None, 0)

    def hist(text, c=None, n=8, mask=None, ids_=None, n_ids=0, sign=1, path=0, st=None, cnt=counts, tl=tally, ctx=h):
        c = col() if c is None else c
        st = state_of("long", 4, (0, 10)) if st is None else st
        rc = lib.gm_histogram_attr(ctx, ctypes.byref(c) if c else None, n, p(mask), p(ids_), n_ids, sign, path,
                                   ctypes.byref(st) if st else None, p(cnt), p(tl))
        assert rc == _lib.GM_E_INVALID and text in _lib.last_error(), (text, rc, _lib.last_error())

    hist("NULL context", ctx=None)
    hist("NULL attribute column", c=False)
    hist("GM_ATTR_UTF8", c=col(_lib.GM_ATTR_UTF8))
    hist("unknown attribute type", c=col(77))
    hist("differs from the state's", c=col(_lib.GM_ATTR_FLOAT64))
    hist("NULL histogram state", st=False)
    hist("length must be at least 1", st=state_of("long", 0, (0, 10)))
    hist("upper bound must be greater", st=state_of("long", 4, (10, 10)))
    hist("upper bound must be greater", st=state_of("long", 4, (11, 10)))
    hist("sign must be +1 or -1", sign=0)
    hist("sign must be +1 or -1", sign=2)
    hist("path must be 0, 1 or 2", path=3)
    hist("path must be 0, 1 or 2", path=-1)
    hist("path 1", path=1, st=state_of("long", LDS_BINS + 1, (0, 10)), cnt=dev(np.zeros(LDS_BINS + 1, np.int64)))
    hist("negative row count", n=-1)
    hist("negative id count", ids_=ids, n_ids=-1)
    hist("mask and ids are exclusive", mask=words, ids_=ids, n_ids=2)
    hist("NULL counts or tally", cnt=None)
    hist("NULL counts or tally", tl=None)
    hist("naturally aligned", c=col(ptr_=v.data_ptr() + 4))
    hist("naturally aligned", c=col(ptr_=0))
    nan_st = _lib.HistState(_lib.GM_ATTR_FLOAT64, 4, 0, 0, float("nan"), 1.0)
    hist("upper bound must be greater", c=col(_lib.GM_ATTR_FLOAT64), st=nan_st)

    def mm(text, c=None, n=8, mask=None, ids_=None, n_ids=0, s=slots, tl=tally, ctx=h):
        c = col() if c is None else c
        rc = lib.gm_minmax_attr(ctx, ctypes.byref(c) if c else None, n, p(mask), p(ids_), n_ids, p(s), None, p(tl))
        assert rc == _lib.GM_E_INVALID and "gm_minmax_attr" in _lib.last_error() and text in _lib.last_error()

    mm("NULL context", ctx=None)
    mm("NULL attribute column", c=False)
    mm("GM_ATTR_UTF8", c=col(_lib.GM_ATTR_UTF8))
    mm("unknown attribute type", c=col(0))
    mm("negative row count", n=-2)
    mm("mask and ids are exclusive", mask=words, ids_=ids, n_ids=2)
    mm("NULL minmax or tally", s=None)
    mm("NULL minmax or tally", tl=None)
    assert counts.cpu().tolist() == [0] * 4 and tally.cpu().tolist() == [0] * 3     # nothing ran


# ---------------------------------------------------------------------- stream order
@pytest.mark.parametrize("kind", ["owned", "caller"])
def test_stream_order_of_both_entries(gpu, kind):
    """The held-stream protocol of tests/stream_order.py on a context's own stream and on a caller's:
    gm_minmax_attr is stream-ordered and returns before the held work, gm_histogram_attr waits for it."""
    import torch
    import stream_order as SO
    if kind == "owned":
        ctx = _lib.Context.owned(0)
        stream = torch.cuda.ExternalStream(ctx.stream)
    else:
        stream = torch.cuda.Stream()
        ctx = _lib.Context(0, stream.cuda_stream)
    try:
        hold = SO.Hold(100.0)
        for name in ("gm_minmax_attr", "gm_histogram_attr"):
            SO.plain_run(ctx, name)
            early = SO.held_run(ctx, stream, name, hold)
            assert early == (not SO.get(name).waits), (name, early)
    finally:
        ctx.close()
