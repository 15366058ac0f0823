"""GPU parity of gm_z3_frequency / gm_frequency_attr / gm_frequency_points / gm_cms_estimate and of the Frequency
and Z3Frequency classes against the numpy restatement (tests/frequency_ref.py): table, size and tally equal
exactly, on every path, launch shape and selection."""
import ctypes
import datetime

import numpy as np
import pytest

import frequency_ref as R
from abi_buffers import Guarded
from test_gpu_parity import T2020, edge_points, random_points

pytestmark = pytest.mark.gpu
DAY, WEEK, MONTH, YEAR = 0, 1, 2, 3
N = 100_003            # odd, and several workgroup blocks
WK = 604800000
W2020 = T2020 // WK    # 2608: the week bin of 2020-01-01; the random points span bins 2608 .. 2661


def ms(s):
    return int(datetime.datetime.fromisoformat(s + "+00:00").timestamp() * 1000)


def dev(a, offset8=False):
    """A device copy of a host array; offset8: 8 B past a 16-B boundary, so the scalar-load kernels run."""
    import torch
    a = np.ascontiguousarray(a)
    if not offset8:
        t = torch.from_numpy(a.copy()).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device="cuda")
    start = (8 - raw.data_ptr()) % 16
    view = raw[start:start + a.nbytes]
    view.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()))
    assert view.data_ptr() % 16 == 8
    return view


def cms(depth=5, width=400, lo=W2020, nb=54, workgroups=0, path=0, hashes=None):
    from geomesa_amd import _lib
    c = _lib.Cms(depth, width, lo, nb, workgroups, path)
    for i, a in enumerate(R.hash_a(min(max(depth, 0), 32)) if hashes is None else hashes):
        c.hash_a[i] = a
    return c


class State:
    """The device block one call adds to (and the next call of a test keeps adding to)."""

    def __init__(self, c):
        import torch
        self.table = torch.zeros((c.n_bins, c.depth, c.width), dtype=torch.int64, device="cuda")
        self.size = torch.zeros(c.n_bins, dtype=torch.int64, device="cuda")
        self.tally = torch.zeros(3, dtype=torch.int64, device="cuda")

    def host(self):
        return self.table.cpu().numpy(), self.size.cpu().numpy(), self.tally.cpu().numpy()


def sel_args(mask_words, ids):
    """(mask pointer, ids pointer, n_ids, keep-alive) of a host selection."""
    from geomesa_amd import _lib
    m = dev(np.asarray(mask_words, np.int64)) if mask_words is not None else None
    i = dev(np.asarray(ids, np.int64)) if ids is not None and len(ids) else None
    if ids is not None and not len(ids):
        i = dev(np.zeros(1, np.int64))
    return _lib.ptr(m), _lib.ptr(i), (len(ids) if ids is not None else 0), (m, i)


def run_z3(x, y, t, period, precision, c, st=None, mask_words=None, ids=None, offset8=False, expect=0):
    from geomesa_amd import _lib
    ctx = _lib.context()
    st = st or State(c)
    X, Y, T = dev(x, offset8), dev(y, offset8), dev(t, offset8)
    mp, ip, ni, keep = sel_args(mask_words, ids)
    rc = ctx.lib.gm_z3_frequency(ctx.handle, _lib.ptr(X), _lib.ptr(Y), _lib.ptr(T), len(x), mp, ip, ni, period,
                                 precision, ctypes.byref(c), _lib.ptr(st.table), _lib.ptr(st.size), _lib.ptr(st.tally))
    assert rc == expect, (rc, _lib.last_error())
    return st


def time_col(t, t_valid, offset8=False):
    from geomesa_amd.arrow import TimeColumnC
    if t is None:
        return None, None
    T = dev(t, offset8)
    V = dev(np.asarray(t_valid, np.uint8)) if t_valid is not None else None
    return TimeColumnC(T.data_ptr(), V.data_ptr() if V is not None else None, 0), (T, V)


ATTR = {"int": (1, np.int32), "long": (2, np.int64), "double": (3, np.float64), "float": (5, np.float32)}


def run_attr(kind, values, precision, c, t=None, period=WEEK, valid=None, t_valid=None, st=None, mask_words=None,
             ids=None, offset8=False, expect=0):
    from geomesa_amd import _lib
    ctx = _lib.context()
    st = st or State(c)
    code, dt = ATTR[kind]
    V = dev(np.asarray(values, dt), offset8)
    VV = dev(np.asarray(valid, np.uint8)) if valid is not None else None
    col = _lib.AttrColumn(code, 0, V.data_ptr(), None, VV.data_ptr() if VV is not None else None, 0)
    tc, keep_t = time_col(t, t_valid, offset8)
    mp, ip, ni, keep = sel_args(mask_words, ids)
    rc = ctx.lib.gm_frequency_attr(ctx.handle, ctypes.byref(col), ctypes.byref(tc) if tc is not None else None,
                                   len(values), mp, ip, ni, period, precision, ctypes.byref(c), _lib.ptr(st.table),
                                   _lib.ptr(st.size), _lib.ptr(st.tally))
    assert rc == expect, (rc, _lib.last_error())
    return st


def run_points(x, y, precision, c, t=None, period=WEEK, t_valid=None, st=None, mask_words=None, ids=None,
               offset8=False, expect=0):
    from geomesa_amd import _lib
    ctx = _lib.context()
    st = st or State(c)
    X, Y = dev(x, offset8), dev(y, offset8)
    tc, keep_t = time_col(t, t_valid, offset8)
    mp, ip, ni, keep = sel_args(mask_words, ids)
    rc = ctx.lib.gm_frequency_points(ctx.handle, _lib.ptr(X), _lib.ptr(Y), ctypes.byref(tc) if tc is not None else None,
                                     len(x), mp, ip, ni, period, precision, ctypes.byref(c), _lib.ptr(st.table),
                                     _lib.ptr(st.size), _lib.ptr(st.tally))
    assert rc == expect, (rc, _lib.last_error())
    return st


def ref_of(c):
    return R.Sketches(c.depth, c.width, c.bin_lo, c.n_bins, [c.hash_a[i] for i in range(c.depth)])


def same(st, ref):
    table, size, tally = st.host()
    assert np.array_equal(tally, ref.tally), (tally, ref.tally)
    assert np.array_equal(size, ref.size)
    assert np.array_equal(table, ref.table)
    return True


_inputs = {}


def inputs():
    """N random points of 2020 plus the edge points (NaN, infinite and out-of-bounds ordinates, dates before
    the epoch and past the last bin): computed once."""
    if not _inputs:
        x, y, t = random_points(N - 4096)
        ex, ey, et = edge_points()
        _inputs["xyt"] = (np.concatenate([x, ex]), np.concatenate([y, ey]), np.concatenate([t, et]))
        assert len(_inputs["xyt"][0]) == N
    return _inputs["xyt"]


def pack(bits, extra_above=True):
    """Mask words of a boolean row selection, the bits at and above n set (they are ignored)."""
    n = len(bits)
    full = np.ones(((n + 63) // 64) * 64, bool) if extra_above else np.zeros(((n + 63) // 64) * 64, bool)
    full[:n] = bits
    return np.packbits(full, bitorder="little").view(np.int64)


# ------------------------------------------------------------------ Z3Frequency

# the window of each period holds part of 2020 only, so tally[1] counts as well
WINDOWS = {DAY: (T2020 // 86400000 + 10, 40), WEEK: (W2020, 54), MONTH: (600, 12), YEAR: (50, 1)}


@pytest.mark.parametrize("period", [DAY, WEEK, MONTH, YEAR])
@pytest.mark.parametrize("precision", [0, 1, 25, 64])
def test_z3_frequency_periods_and_precisions(gpu, oracle, period, precision):
    x, y, t = inputs()
    lo, nb = WINDOWS[period]
    c = cms(lo=lo, nb=nb)
    st = run_z3(x, y, t, period, precision, c)
    ref = ref_of(c).observe_z3(oracle, x, y, t, period, precision)
    assert same(st, ref) and ref.tally[0] > 1000 and ref.size.sum() > 5_000
    if period == DAY:
        assert ref.tally[1] > 50_000
    else:
        assert ref.size.sum() > 90_000


@pytest.mark.parametrize("nb", [1024, 1025])
def test_z3_frequency_at_the_pass_limit(gpu, oracle, nb):
    """1024 day bins of the default shape are 64 LDS passes of 16 bins, the last the automatic path takes;
    1025 bins are 65 and take the device-atomic kernel."""
    x, y, t = inputs()
    c = cms(lo=T2020 // 86400000 + 366 - nb, nb=nb)
    assert same(run_z3(x, y, t, DAY, 25, c), ref_of(c).observe_z3(oracle, x, y, t, DAY, 25))


@pytest.mark.parametrize("nb", [1, 3, 40])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_z3_frequency_windows_and_paths(gpu, oracle, nb, path):
    """Windows of 1, 3 and 40 week bins, all narrower than the data (tally[1]); 40 bins of the default shape
    are 80,040 counters, more than one LDS pass holds (32,768), so paths 0 and 1 take three passes."""
    assert 40 * (5 * 400 + 1) > 2 * 32768
    x, y, t = inputs()
    c = cms(lo=W2020 + 5, nb=nb, path=path)
    st = run_z3(x, y, t, WEEK, 25, c)
    ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25)
    assert same(st, ref) and ref.tally[1] > 10_000 and np.count_nonzero(ref.size) == nb


@pytest.mark.parametrize("depth,width", [(5, 400), (1, 1), (3, 7), (32, 33)])
@pytest.mark.parametrize("path", [0, 2])
def test_sketch_shapes(gpu, oracle, depth, width, path):
    x, y, t = inputs()
    c = cms(depth, width, path=path)
    assert same(run_z3(x, y, t, WEEK, 25, c), ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25))


def test_sketch_too_large_for_lds(gpu, oracle):
    """(20, 20000): one bin's 400,001 counters do not fit a workgroup: automatic takes device atomics, and
    path 1 is GM_E_INVALID."""
    from geomesa_amd import _lib
    x, y, t = inputs()
    c = cms(20, 20000, lo=W2020 + 3, nb=2)
    assert same(run_z3(x, y, t, WEEK, 25, c), ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25))
    c = cms(20, 20000, lo=W2020 + 3, nb=2, path=1)
    st = run_z3(x, y, t, WEEK, 25, c, expect=_lib.GM_E_INVALID)
    assert "do not fit" in _lib.last_error() and not st.table.any() and not st.tally.any()


@pytest.mark.parametrize("workgroups", [1, 3])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("offset8", [False, True])
def test_workgroups_and_accumulation(gpu, oracle, workgroups, path, offset8):
    """One and three workgroups walk all the rows (the flush of hot counters, the workgroup count the
    counter-wrap rule starts from); two calls into one state equal one call over the concatenation."""
    x, y, t = inputs()
    c = cms(lo=W2020, nb=20, workgroups=workgroups, path=path)
    h = 40_001
    st = run_z3(x[:h], y[:h], t[:h], WEEK, 25, c, offset8=offset8)
    st = run_z3(x[h:], y[h:], t[h:], WEEK, 25, c, st=st, offset8=offset8)
    assert same(st, ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25))


def test_hot_counters(gpu, oracle):
    """Every row on three positions: tens of thousands of increments of the same LDS counters."""
    rng = np.random.default_rng(9)
    k = rng.integers(0, 3, 300_001)
    x = np.array([10.0, -75.5, 139.7])[k]
    y = np.array([47.0, 40.1, 35.6])[k]
    t = np.array([T2020 + 5 * 86400000, T2020 + 5 * 86400000 + 1, T2020 + 9 * 86400000])[k]
    for wg in (0, 1):
        c = cms(lo=W2020, nb=3, workgroups=wg)
        st = run_z3(x, y, t, WEEK, 64, c)
        ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 64)
        assert same(st, ref) and ref.table.max() > 90_000


# ------------------------------------------------------------------ Frequency: the attribute rules

def attr_values(kind):
    rng = np.random.default_rng(11)
    if kind == "int":
        v = rng.integers(-(1 << 31), 1 << 31, N, dtype=np.int64).astype(np.int32)
        v[:6] = [-(1 << 31), (1 << 31) - 1, -7, 7, 0, -1]
    elif kind == "long":
        v = rng.integers(-(1 << 63), (1 << 63) - 1, N, dtype=np.int64, endpoint=True)
        v[:7] = [-(1 << 63), (1 << 63) - 1, -7, 7, 0, -1, -1999]
    elif kind == "float":
        v = (rng.normal(0, 1e4, N)).astype(np.float32)
        v[:12] = [0.5, -0.5, 1.5, 2.5, 0.49999997, np.nan, np.inf, -np.inf, 3e9, -3e9, 16777217.0, -0.0]
        v[12:2000] = (rng.integers(-4000, 4000, 1988) + 0.5).astype(np.float32)    # ties
    else:
        v = rng.normal(0, 1e6, N)
        v[:12] = [0.5, -0.5, 1.5, 2.5, 0.49999999999999994, np.nan, np.inf, -np.inf, 1e19, -1e19, 2.0 ** 52 + 1, -0.0]
        v[12:2000] = rng.integers(-4000, 4000, 1988) + 0.5
        v[2000:3000] = rng.normal(0, 1e18, 1000)
    return v


def null_bitmap(n, share, seed):
    rng = np.random.default_rng(seed)
    return np.packbits(rng.random(((n + 7) // 8) * 8) >= share, bitorder="little")


@pytest.mark.parametrize("kind", ["int", "long", "float", "double"])
@pytest.mark.parametrize("precision", [1, 7])
@pytest.mark.parametrize("offset8", [False, True])
def test_frequency_attr_without_dtg(gpu, oracle, kind, precision, offset8):
    """Every key rule over extreme and negative values and null slots, in time bin 0."""
    v = attr_values(kind)
    valid = null_bitmap(N, 0.1, 3)
    c = cms(lo=0, nb=1)
    st = run_attr(kind, v, precision, c, valid=valid, offset8=offset8)
    ref = ref_of(c).observe_attr(oracle, kind, v, precision, valid=valid)
    assert same(st, ref) and 85_000 < ref.size[0] < 95_000 and ref.tally.tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", ["int", "long", "float", "double"])
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("offset8", [False, True])
def test_frequency_attr_with_dtg(gpu, oracle, kind, path, offset8):
    """Dates of 2020 plus the edge dates: a null date slot goes to bin 0 (inside the window here), a date
    BinnedTime rejects counts in tally[0], bins above the window in tally[1]."""
    _, _, t = inputs()
    v = attr_values(kind)
    valid, t_valid = null_bitmap(N, 0.05, 4), null_bitmap(N, 0.2, 5)
    c = cms(3, 50, lo=-2, nb=W2020 + 30, path=path)
    st = run_attr(kind, v, 3, c, t=t, valid=valid, t_valid=t_valid, offset8=offset8)
    ref = ref_of(c).observe_attr(oracle, kind, v, 3, t_ms=t, valid=valid, t_valid=t_valid)
    assert same(st, ref)
    assert ref.size[2] > 15_000 and ref.tally[0] > 500 and ref.tally[1] > 20_000


@pytest.mark.parametrize("period", [DAY, MONTH, YEAR])
def test_frequency_attr_periods(gpu, oracle, period):
    _, _, t = inputs()
    v = attr_values("long")
    lo, nb = WINDOWS[period]
    c = cms(lo=lo, nb=nb)
    st = run_attr("long", v, 1000, c, t=t, period=period)
    assert same(st, ref_of(c).observe_attr(oracle, "long", v, 1000, t_ms=t, period=period))


def test_frequency_date_attribute(gpu, oracle):
    """A Date attribute passes as GM_ATTR_INT64 epoch milliseconds: dateToKey = getTime / precision."""
    _, _, t = inputs()
    c = cms(lo=W2020, nb=54)
    st = run_attr("long", t, 86400000, c, t=t)
    ref = ref_of(c).observe_attr(oracle, "long", t, 86400000, t_ms=t)
    assert same(st, ref) and ref.tally[0] > 500      # the negative dates


@pytest.mark.parametrize("offset8", [False, True])
@pytest.mark.parametrize("with_dtg", [False, True])
def test_frequency_points(gpu, oracle, offset8, with_dtg):
    """The geometry rule: points on and beyond +-180 / +-90 (the edge points), NaN ordinates, dates."""
    x, y, t = inputs()
    t_valid = null_bitmap(N, 0.2, 6)
    c = cms(lo=0, nb=1) if not with_dtg else cms(2, 30, lo=-1, nb=W2020 + 60)     # five LDS passes
    kw = dict(t=t, t_valid=t_valid) if with_dtg else {}
    st = run_points(x, y, 31, c, offset8=offset8, **kw)
    ref = ref_of(c).observe_points(oracle, x, y, 31, **({"t_ms": t, "t_valid": t_valid} if with_dtg else {}))
    assert same(st, ref) and ref.tally[0] > 1000
    if with_dtg:
        assert ref.size[1] > 15_000


@pytest.mark.parametrize("precision", [0, 1, 64])
def test_frequency_points_precisions(gpu, oracle, precision):
    x, y, _ = inputs()
    c = cms(lo=0, nb=1)
    assert same(run_points(x, y, precision, c), ref_of(c).observe_points(oracle, x, y, precision))


# ------------------------------------------------------------------ selection

SELECTIONS = ["mask 1 %", "mask 50 %", "ids", "ids empty"]


def selection(name, n):
    rng = np.random.default_rng(17)
    if name.startswith("mask"):
        return dict(mask_words=pack(rng.random(n) < (0.01 if "1 %" in name else 0.5)))
    if name == "ids empty":
        return dict(ids=np.zeros(0, np.int64))
    ids = rng.integers(0, n, 30_001)                  # shuffled, with repeats
    ids[::100] = rng.integers(n, n + 1000, len(ids[::100]))
    ids[1::100] = -1 - rng.integers(0, 1000, len(ids[1::100]))
    ids[5] = np.iinfo(np.int64).max
    ids[6] = np.iinfo(np.int64).min
    return dict(ids=ids)


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("offset8", [False, True])
def test_selection_z3(gpu, oracle, name, path, offset8):
    x, y, t = inputs()
    sel = selection(name, N)
    c = cms(lo=W2020, nb=20, path=path)     # two LDS passes
    st = run_z3(x, y, t, WEEK, 25, c, offset8=offset8, **sel)
    ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25, **sel)
    assert same(st, ref)
    if name == "ids":
        assert ref.tally[2] > 500
    if name == "ids empty":
        assert not ref.size.any()


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("kind", ["int", "double"])
def test_selection_attr(gpu, oracle, name, kind):
    _, _, t = inputs()
    v = attr_values(kind)
    sel = selection(name, N)
    valid = null_bitmap(N, 0.1, 8)
    c = cms(lo=W2020, nb=54)
    st = run_attr(kind, v, 2, c, t=t, valid=valid, **sel)
    assert same(st, ref_of(c).observe_attr(oracle, kind, v, 2, t_ms=t, valid=valid, **sel))


@pytest.mark.parametrize("name", SELECTIONS)
def test_selection_points(gpu, oracle, name):
    x, y, t = inputs()
    sel = selection(name, N)
    c = cms(lo=W2020, nb=54)
    st = run_points(x, y, 40, c, t=t, **sel)
    assert same(st, ref_of(c).observe_points(oracle, x, y, 40, t_ms=t, **sel))


def test_small_and_odd_batches(gpu, oracle):
    """n = 0, 1, 2, 3 and a 129-row batch whose mask has one whole zero word."""
    x, y, t = random_points(129)
    for n in (0, 1, 2, 3):
        c = cms(lo=W2020, nb=54)
        assert same(run_z3(x[:n], y[:n], t[:n], WEEK, 25, c), ref_of(c).observe_z3(oracle, x[:n], y[:n], t[:n], WEEK, 25))
    bits = np.zeros(129, bool)
    bits[[0, 63, 128]] = True
    for words in (pack(bits), pack(bits, extra_above=False)):
        c = cms(lo=W2020, nb=54)
        st = run_z3(x, y, t, WEEK, 25, c, mask_words=words)
        ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25, mask_words=words)
        assert same(st, ref) and ref.size.sum() == 3


def test_bad_ids_never_leave_the_buffers(gpu, oracle):
    """ids far outside [0, n) are counted and never read through; table, size and tally sit between guards."""
    from geomesa_amd import _lib
    x, y, t = random_points(1001)
    ids = np.array([0, 1000, 1001, -1, 1 << 40, -(1 << 40), 5, 5], np.int64)
    c = cms(3, 7, lo=W2020, nb=54)
    ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25, ids=ids)
    for path in (1, 2):
        c.path = path
        gt, gs, gl = Guarded(54 * 3 * 7 * 8), Guarded(54 * 8), Guarded(24)
        for g in (gt, gs, gl):
            g.write(np.zeros(g.nbytes, np.uint8))
        gx, gy, gtm, gi = Guarded.of(x), Guarded.of(y), Guarded.of(t), Guarded.of(ids)
        ctx = _lib.context()
        rc = ctx.lib.gm_z3_frequency(ctx.handle, gx.ptr, gy.ptr, gtm.ptr, len(x), None, gi.ptr, len(ids), WEEK, 25,
                                     ctypes.byref(c), gt.ptr, gs.ptr, gl.ptr)
        assert rc == 0, _lib.last_error()
        assert np.array_equal(gl.read(np.int64), ref.tally) and ref.tally[2] == 4
        assert np.array_equal(gs.read(np.int64), ref.size)
        assert np.array_equal(gt.read(np.int64).reshape(54, 3, 7), ref.table)
        for g in (gt, gs, gl):
            g.check("path %d" % path)


def test_selections_a_query_returns(gpu, oracle):
    """ids from a Z3Table.query and the mask of filters.query_scan, against the restatement over the same rows."""
    from geomesa_amd import filters as F
    from geomesa_amd.keyspace import Z3IndexKeySpace, during
    from geomesa_amd.stats import Z3Frequency
    from geomesa_amd.table import Z3Table
    x, y, t = random_points(N)
    ks = Z3IndexKeySpace()
    b, z = ks.sfc.index_keys(x, y, t)
    bb, iv = [(-40, 10, 40, 70)], [during(ms("2020-03-01T00:00:00"), ms("2020-06-08T12:00:00"))]
    ids, nm, _ = Z3Table(b, z).query(bb, iv)
    assert nm > 500
    f = Z3Frequency(period="week", precision=25).observe(x, y, t, ids=ids)
    ref = R.Sketches(bin_lo=f.bin_lo, n_bins=f.n_bins).observe_z3(oracle, x, y, t, WEEK, 25, ids=ids.cpu().numpy())
    assert np.array_equal(f.table.cpu().numpy(), ref.table) and np.array_equal(f.sizes.cpu().numpy(), ref.size)
    assert f.size == nm and f.skipped == 0 and f.bad_ids == 0
    mask, _, nk = F.query_scan(x, y, t, bbox=bb[0], during=(ms("2020-03-01T00:00:00"), ms("2020-06-08T12:00:00")))
    keep = mask.cpu().numpy()
    assert nk == keep.sum() > 500
    g = Z3Frequency(period="week", precision=25).observe(x, y, t, mask=mask)
    ref = R.Sketches(bin_lo=g.bin_lo, n_bins=g.n_bins).observe_z3(oracle, x, y, t, WEEK, 25, ids=np.flatnonzero(keep))
    assert np.array_equal(g.table.cpu().numpy(), ref.table) and np.array_equal(g.sizes.cpu().numpy(), ref.size)
    assert g.size == nk


# ------------------------------------------------------------------ gm_cms_estimate

def test_cms_estimate(gpu, oracle):
    """Per bin, summed over the window, and 0 for bins outside it."""
    import torch
    from geomesa_amd import _lib
    x, y, t = inputs()
    c = cms(lo=W2020 + 2, nb=30)
    st = run_z3(x, y, t, WEEK, 25, c)
    ref = ref_of(c).observe_z3(oracle, x, y, t, WEEK, 25)
    b, z, s = oracle.z3_index_key_batch(x[:5000], y[:5000], t[:5000])
    keys = np.concatenate([z & np.int64(R.mask(25)), np.array([0, -1, (1 << 63) - 1, -(1 << 63)], np.int64)])
    bins = np.concatenate([b, np.array([W2020 + 2, W2020 + 31, W2020 + 32, -32768], np.int16)]).astype(np.int16)
    ctx = _lib.context()
    K, B = dev(keys), dev(bins)
    out = torch.full((len(keys),), -7, dtype=torch.int64, device="cuda")
    _lib.check(ctx.lib.gm_cms_estimate(ctx.handle, ctypes.byref(c), _lib.ptr(st.table), _lib.ptr(K), _lib.ptr(B),
                                       len(keys), _lib.ptr(out)), "gm_cms_estimate")
    want = ref.estimate(keys, bins)
    assert np.array_equal(out.cpu().numpy(), want) and want.max() > 1 and (want[:5000][b < W2020 + 2] == 0).all()
    _lib.check(ctx.lib.gm_cms_estimate(ctx.handle, ctypes.byref(c), _lib.ptr(st.table), _lib.ptr(K), None,
                                       len(keys), _lib.ptr(out)), "gm_cms_estimate")
    assert np.array_equal(out.cpu().numpy(), ref.estimate(keys))


# ------------------------------------------------------------------ the classes, end to end

def test_frequency_reference_int_attribute(gpu):
    """FrequencyTest.scala:199-205, 231-250 on the device ("correctly bin values", "combine two Frequencies")."""
    from geomesa_amd.stats import Frequency
    a = Frequency("intAttr", 1)
    assert a.is_empty() and a.size == 0
    a.observe(np.arange(100, dtype=np.int32))
    assert not a.is_empty() and a.size == 100 and a.binding == "int"
    assert set(a.count(np.arange(100)).tolist()) == {1} and a.count(200) == 0
    b = Frequency("intAttr", 1).observe(np.arange(100, 200, dtype=np.int32))
    assert b.size == 100 and set(b.count(np.arange(100, 200)).tolist()) == {1} and b.count(300) == 0
    a += b
    assert a.size == 200 and set(a.count(np.arange(200)).tolist()) == {1, 2} and a.count(300) == 0
    assert b.size == 100 and set(b.count(np.arange(100, 200)).tolist()) == {1}
    assert a.to_json_object() == {"epsilon": 0.005, "confidence": 0.95, "size": 200}
    c = b + b
    assert c.size == 200 and set(c.count(np.arange(100, 200)).tolist()) == {2} and not c.is_equivalent(b)
    a.clear()
    assert a.is_empty() and a.size == 0 and a.count(5) == 0 and a.time_bins() == []


def test_frequency_reference_weekly_binning(gpu):
    """FrequencyTest.scala:69-103 on the device: bins 2340..2343, count(bin, i) == 1, splitByTime."""
    from geomesa_amd.stats import Frequency
    from test_frequency_reference import weekly_features
    v, t = weekly_features()
    f = Frequency("longAttr", 1, dtg="dtg", period="week").observe(v, t)
    assert f.time_bins() == [2340, 2341, 2342, 2343] and f.size == 112 and f.skipped == 0
    splits = dict(f.split_by_time())
    assert sorted(splits) == [2340, 2341, 2342, 2343]
    for w in range(4):
        vals = np.concatenate([np.arange(o + 7 * w, o + 7 * w + 7) for o in (0, 28, 56, 84)])
        assert f.count(2340 + w, vals).tolist() == [1] * 28
        assert splits[2340 + w].count(vals).tolist() == [1] * 28 and splits[2340 + w].size == 28
        assert f.size_of(2340 + w) == 28 and f.count_direct(2340 + w, int(vals[0])) == 1
    assert f.count(2339, 5) == 0 and f.count(5) >= 1
    g = Frequency("longAttr", 1, dtg="dtg", period="week").observe(v[::-1].copy(), t[::-1].copy())
    assert f.is_equivalent(g) and not f.is_equivalent(splits[2340])
    assert int(f.table[2341 - f.bin_lo].sum()) == 5 * 28 and f.size_of(2300) == 0


def test_z3frequency_reference(gpu):
    """Z3FrequencyTest.scala:43-50 on the device: size 100, every count within 1..6 (here 1..5), bin 2191."""
    from geomesa_amd.stats import Z3Frequency
    from test_frequency_reference import z3_features
    x, y, t = z3_features()
    f = Z3Frequency("geom", "dtg", "week", 25)
    assert f.is_empty() and f.size == 0 and f.to_json_object() == {"eps": 0.0, "confidence": 0.0, "size": 0}
    f.observe(x, y, t)
    assert not f.is_empty() and f.size == 100 and f.time_bins() == [2191]
    counts = f.count(x, y, t)
    assert counts.min() == 1 and counts.max() == 5
    assert f.count(float(x[3]), float(y[3]), int(t[3])) == int(counts[3])
    assert f.to_json_object() == {"eps": 0.005, "confidence": 0.95, "size": 100}
    g = f + f
    assert g.size == 200 and np.array_equal(g.count(x, y, t), 2 * counts) and not g.is_equivalent(f)
    f.clear()
    assert f.is_empty() and f.count(x, y, t).tolist() == [0] * 100


def test_frequency_geometry_and_enumerate(gpu, oracle):
    """The geometry binding through observe_points, and Frequency.enumerate (FrequencyTest.scala:61-67) feeding
    count_direct."""
    from geomesa_amd.curve import Z2SFC
    from geomesa_amd.stats import Frequency
    x, y, _ = random_points(20_001)
    f = Frequency("geom", 20).observe_points(x, y)
    ref = R.Sketches().observe_points(oracle, x, y, 20)
    assert np.array_equal(f.table.cpu().numpy(), ref.table) and f.size == 20_001
    assert f.count((float(x[0]), float(y[0]))) == ref.estimate(oracle.z2_index_batch(x[:1], y[:1])[0] & np.int64(R.mask(20)))[0]
    ranges = Z2SFC().ranges([(-10.0, -10.0, 10.0, 10.0)], precision=20)
    keys = list(Frequency.enumerate(ranges, 20))
    assert len(keys) > 4
    got = f.count_direct(np.array(keys, np.int64))
    assert np.array_equal(got, ref.estimate(np.array(keys, np.int64)))
    with pytest.raises(NotImplementedError, match="MurmurHash"):
        Frequency("strAttr", 3).observe(np.array(["a", "b"]))


def test_window_widens_and_merges(gpu, oracle):
    """A second batch below and above the first one's window: the window widens and only the new bins run
    again; += of two stats over different windows is the stat of all rows."""
    from geomesa_amd.stats import Z3Frequency
    x, y, t = random_points(60_000)
    t2 = t[20_000:].copy()
    t2[::3] += 45 * WK       # above
    t2[1::3] -= 60 * WK      # below; the rest inside
    t1 = t[:20_000]
    f = Z3Frequency(period="week", precision=30).observe(x[:20_000], y[:20_000], t1)
    lo0, n0 = f.bin_lo, f.n_bins
    f.observe(x[20_000:], y[20_000:], t2)
    assert f.bin_lo < lo0 and f.n_bins > n0 + 50 and f.skipped == 0
    tt = np.concatenate([t1, t2])
    ref = R.Sketches(bin_lo=f.bin_lo, n_bins=f.n_bins).observe_z3(oracle, x, y, tt, WEEK, 30)
    assert ref.tally.tolist() == [0, 0, 0] and f.size == 60_000
    assert np.array_equal(f.table.cpu().numpy(), ref.table) and np.array_equal(f.sizes.cpu().numpy(), ref.size)
    a = Z3Frequency(period="week", precision=30).observe(x[:20_000], y[:20_000], t1)
    b = Z3Frequency(period="week", precision=30).observe(x[20_000:], y[20_000:], t2)
    a += b
    assert a.is_equivalent(f) and f.is_equivalent(a) and a.size == 60_000
    assert not a.is_equivalent(b) and not a.is_equivalent(Z3Frequency(period="week", precision=29))


def test_frequency_all_reduce_then_observe(gpu, oracle):
    """all_reduce over a gloo group (CPU transport) hands the merged block back on the stat's device, as
    test_z3histogram_all_reduce_then_observe."""
    import os
    import socket
    import torch.distributed as dist
    from geomesa_amd.stats import Frequency, Z3Frequency
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        x, y, t = random_points(40_000)
        f = Z3Frequency(period="week", precision=25).observe(x[:20_000], y[:20_000], t[:20_000])
        f.all_reduce(dist)
        assert f.table.is_cuda and f.sizes.is_cuda
        f.observe(x[20_000:], y[20_000:], t[20_000:])
        ref = R.Sketches(bin_lo=f.bin_lo, n_bins=f.n_bins).observe_z3(oracle, x, y, t, WEEK, 25)
        assert np.array_equal(f.table.cpu().numpy(), ref.table) and np.array_equal(f.sizes.cpu().numpy(), ref.size)
        g = Frequency("longAttr", 10)
        g.all_reduce(dist)                      # empty on every rank: stays empty
        assert g.is_empty()
        g.observe(np.arange(1000, dtype=np.int64)).all_reduce(dist)
        want = R.Sketches().observe_attr(oracle, "long", np.arange(1000, dtype=np.int64), 10).estimate([5])[0]
        assert g.size == 1000 and g.count(50) == want >= 10 and g.table.is_cuda
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ validation

def test_every_invalid_clause(gpu):
    """Each GM_E_INVALID clause of the header once; nothing is written."""
    import torch
    from geomesa_amd import _lib
    from geomesa_amd.arrow import TimeColumnC
    ctx = _lib.context()
    E = _lib.GM_E_INVALID
    x, y, t = (dev(v) for v in random_points(64))
    c0 = cms(lo=W2020, nb=54)
    st = State(c0)
    P = _lib.ptr
    ids = dev(np.arange(4, dtype=np.int64))
    words = dev(np.zeros(1, np.int64))

    def z3(ctxh=ctx.handle, X=P(x), Y=P(y), T=P(t), n=64, mask=None, idp=None, n_ids=0, period=WEEK, precision=25,
           c=c0, table=P(st.table), size=P(st.size), tally=P(st.tally)):
        return ctx.lib.gm_z3_frequency(ctxh, X, Y, T, n, mask, idp, n_ids, period, precision,
                                       ctypes.byref(c) if c is not None else None, table, size, tally)
    assert z3() == 0
    st.table.zero_(); st.size.zero_(); st.tally.zero_()
    off = ctypes.c_void_p(x.data_ptr() + 4)
    bad = [dict(ctxh=None), dict(c=None), dict(table=None), dict(size=None), dict(tally=None), dict(X=None), dict(Y=None),
           dict(T=None), dict(n=-1), dict(period=4), dict(period=-1), dict(c=cms(0, 400)), dict(c=cms(33, 400)),
           dict(c=cms(5, 0)), dict(c=cms(nb=0)), dict(c=cms(lo=-32769, nb=1)), dict(c=cms(lo=32767, nb=2)),
           dict(c=cms(5, 400, lo=0, nb=32768 * 33)), dict(c=cms(32, 1 << 26, lo=0, nb=2)), dict(idp=P(ids), n_ids=-1),
           dict(mask=P(words), idp=P(ids), n_ids=4), dict(c=cms(path=3)), dict(c=cms(path=-1)),
           dict(c=cms(20, 20000, path=1)), dict(c=cms(workgroups=-1)), dict(precision=-1), dict(precision=65),
           dict(X=off), dict(mask=off), dict(idp=off, n_ids=1), dict(table=off), dict(tally=off)]
    for kw in bad:
        assert z3(**kw) == E, kw
        assert _lib.last_error().startswith("gm_z3_frequency: "), kw
    v = dev(np.arange(64, dtype=np.int64))
    tc = TimeColumnC(t.data_ptr(), None, 0)

    def attr(typ=_lib.GM_ATTR_INT64, values=v.data_ptr(), col=True, dtg=tc, precision=1, c=c0, n=64):
        a = _lib.AttrColumn(typ, 0, values, None, None, 0)
        return ctx.lib.gm_frequency_attr(ctx.handle, ctypes.byref(a) if col else None,
                                         ctypes.byref(dtg) if dtg is not None else None, n, None, None, 0, WEEK, precision,
                                         ctypes.byref(c), P(st.table), P(st.size), P(st.tally))
    assert attr() == 0 and attr(precision=-3, typ=_lib.GM_ATTR_FLOAT64) == 0
    st.table.zero_(); st.size.zero_(); st.tally.zero_()
    bad = [dict(col=False), dict(typ=_lib.GM_ATTR_UTF8), dict(typ=0), dict(typ=6), dict(precision=0),
           dict(precision=-1, typ=_lib.GM_ATTR_INT32), dict(values=None), dict(values=v.data_ptr() + 4),
           dict(values=v.data_ptr() + 2, typ=_lib.GM_ATTR_FLOAT32), dict(dtg=TimeColumnC(None, None, 0)),
           dict(dtg=TimeColumnC(t.data_ptr() + 4, None, 0)), dict(c=cms(path=3)), dict(n=-1)]
    for kw in bad:
        assert attr(**kw) == E, kw
        assert _lib.last_error().startswith("gm_frequency_attr: "), kw
    assert "MurmurHash" in (attr(typ=_lib.GM_ATTR_UTF8), _lib.last_error())[1]

    def points(X=P(x), Y=P(y), dtg=None, precision=31, c=c0):
        return ctx.lib.gm_frequency_points(ctx.handle, X, Y, ctypes.byref(dtg) if dtg is not None else None, 64, None,
                                           None, 0, WEEK, precision, ctypes.byref(c), P(st.table), P(st.size), P(st.tally))
    for kw in [dict(X=None), dict(Y=off), dict(precision=65), dict(precision=-1), dict(dtg=TimeColumnC(None, None, 0)),
               dict(c=cms(5, 0))]:
        assert points(**kw) == E, kw
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    b16 = dev(np.zeros(64, np.int16))

    def est(ctxh=ctx.handle, c=c0, table=P(st.table), keys=P(v), bins=P(b16), n=64, o=P(out)):
        return ctx.lib.gm_cms_estimate(ctxh, ctypes.byref(c) if c is not None else None, table, keys, bins, n, o)
    assert est() == 0 and est(bins=None) == 0 and est(n=0, keys=None, o=None) == 0
    for kw in [dict(ctxh=None), dict(c=None), dict(table=None), dict(keys=None), dict(o=None), dict(n=-1),
               dict(c=cms(0, 400)), dict(c=cms(nb=0)), dict(keys=off), dict(bins=ctypes.c_void_p(b16.data_ptr() + 1))]:
        assert est(**kw) == E, kw
    # gm_bin_track / gm_bin_label keep rejecting the type they do not know
    a = _lib.AttrColumn(_lib.GM_ATTR_FLOAT32, 0, v.data_ptr(), None, None, 0)
    tr = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert ctx.lib.gm_bin_track(ctx.handle, ctypes.byref(a), 64, P(tr)) == E
    assert ctx.lib.gm_bin_label(ctx.handle, ctypes.byref(a), 64, P(out)) == E
    torch.cuda.synchronize()
    assert not st.table.any() and not st.size.any() and not st.tally.any()
