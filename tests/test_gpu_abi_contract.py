"""include/geomesa_hip.h clause by clause, through ctypes: return codes, output bounds, alignment dispatch.

Every call here is ctx.lib.gm_* itself, never a wrapper of geomesa_amd/ (a PolygonIndex only builds the
index a join is handed).  Every device buffer is an abi_buffers.Guarded: a payload at a chosen byte
offset from a 256-B boundary inside one 0xA5-filled tensor, so an overrun is a wrong byte of the test's
own tensor, and every run ends with the guards of all its buffers checked.  Results are bit-exact against
the C oracle, or against the definition the existing tests of that entry use.

Rows per block of the index kernels (test_element_failures uses n = 2 x block + 5 and fails row 1, a row
of the second block and the last row, the odd tail):
  gm_z3_index            256   k_z3_index, grid-stride, TPB = 256
  gm_z3_index_key       2048   k_z3_index_key: TPB 256 x UNROLL_KEY 4 pairs
  gm_z2_index            512   k_z2_index: TPB 256 x UNROLL_Z2 1 pair
  gm_binned_time         256   k_binned_time, grid-stride
  gm_xz2_index           512   k_xz2_index_v: XTPB 128 x UNROLL_XZ 2 pairs
  gm_xz3_index           512   k_xz3_index_v: the same
  gm_xz3_index_key       256   k_xz3_index_key, grid-stride
  gm_z3_index_key_arrow 2048   k_z3_key_arrow_v: ATPB 256 x AUNROLL 4 pairs
  gm_z2_index_key_arrow  512   k_z2_key_arrow: ATPB 256 pairs, grid-stride
  gm_xz2/xz3_index_key_arrow 256   k_xz_key_arrow, grid-stride
  gm_legacy_z3/z2_index  256   k_legacy_*_index, grid-stride, LTPB = 256

test_alignment: the fast-path condition of each entry point, and the kernel or branch each case reaches
("all" = every pointer on a 256-B boundary; "p+1" = pointer p moved by one element of its own type, the
others as in "all"):
  gm_z3_index_key   x, y, t_ms, z at 16 B, bin at 4 B, status at 2 B
      all                 k_z3_index_key, store_staged_bins 16-B stores
      bin+2 (4 B in)      k_z3_index_key, store_staged_bins' 4-B stores (bin 4-B but not 16-B aligned)
      bin+1 (2 B in)      k_z3_index_key_s (bin not 4-B aligned)
      status+1 (odd)      k_z3_index_key_s
      x+1, y+1, t_ms+1, z+1   k_z3_index_key_s
  gm_z3_invert      z, x, y, t at 16 B
      all                 k_z3_invert;   z+1, x+1, y+1, t+1   k_z3_invert_s
  gm_z2_index       x, y, z at 16 B, status at 2 B
      all                 k_z2_index;    x+1, y+1, z+1, status+1   k_z2_index_s
  gm_z2_invert      z, x, y at 16 B
      all                 k_z2_invert;   z+1, x+1, y+1   k_z2_invert_s
  gm_xz2_index      xmin, ymin, xmax, ymax, out at 16 B, status at 2 B
      all                 k_xz2_index_v; each of the six +1   k_xz2_index
  gm_xz3_index      the six envelope columns and out at 16 B, status at 2 B
      all                 k_xz3_index_v; each of the eight +1   k_xz3_index
  gm_z3filter_scan  bin, z at 16 B (mask, ids: any 8-B address)
      all                 k_z3filter_mask_v<FAST = true, VEC = true>;   bin+1, z+1   k_z3filter_mask_v<true, false>
      mask+1, ids+1       k_z3filter_mask_v<true, true> and k_mask_to_ids on 8-B aligned outputs
  gm_z2filter_scan  z at 16 B
      all                 k_z2filter_mask_v<true, true>;   z+1   k_z2filter_mask_v<true, false>;   mask+1, ids+1 as above
  gm_strict_scan    x, y, t_ms (with a during) at 16 B
      all                 k_strict_mask_v<DURING = true, VEC = true>;   x+1, y+1, t_ms+1   k_strict_mask_v<true, false>;   mask+1, ids+1
  gm_query_scan     x, y, t_ms (with a during) at 16 B, with a geometry term
      all                 k_query_mask<VEC = true, true, ..>;  x+1, y+1, t_ms+1   k_query_mask<false, true, ..>;  mask+1, ids+1
  gm_z3_histogram   x, y, t_ms at 16 B (LDS-counter path)
      all                 k_z3_hist_lds<.., VEC = true, ..>;   x+1, y+1, t_ms+1   k_z3_hist_lds<.., false, ..>
      present+1, counts+1, tally+1   the same kernel, outputs at odd element offsets
  gm_pip_join_pred  px, py at 16 B
      all                 join_staged<0, true>;      px+1, py+1   join_staged<0, false>
      pt_ids+1, poly_ids+1   join_staged<0, true>, slab stores and k_pair_move on 8-B / 4-B aligned outputs
  gm_pip_relate     px, py at 16 B, poly at 8 B, loc at 2 B
      all                 k_pip_relate<VEC = true, R32>;  px+1, py+1, poly+1, loc+1   k_pip_relate<VEC = false, R32>
"""
import ctypes
import functools

import numpy as np
import pytest

from abi_buffers import FILL, Guarded, untouched
from geomesa_amd import _lib

pytestmark = pytest.mark.gpu

T2020, T2021 = 1577836800000, 1609459200000
WEEK = 1
WEEK_MAX = 604800          # BinnedTime.maxOffset(Week), seconds
OK, E_INVALID, E_CAPACITY, E_ELEMENT = _lib.GM_OK, _lib.GM_E_INVALID, _lib.GM_E_CAPACITY, _lib.GM_E_ELEMENT
I16, I32, I64, U8, U32, U64, F64 = np.int16, np.int32, np.int64, np.uint8, np.uint32, np.uint64, np.float64


def P(g):
    """The pointer argument of a Guarded (None passes through)."""
    return None if g is None else g.ptr


def sync(gpu):
    assert gpu.lib.gm_ctx_sync(gpu.handle) == OK


def check_all(bufs, what=""):
    for k, b in enumerate(bufs):
        if b is not None:
            b.check("%s buffer %d" % (what, k))


def point_struct(coords):
    """gm_geom_column of a Float8 point column over a device buffer of [y, x] tuples."""
    from geomesa_amd.arrow import GeomColumnC
    return GeomColumnC(0, 64, 0, 0, coords.addr if coords is not None else None, None, 0, (ctypes.c_void_p * 3)())


def time_struct(ms):
    from geomesa_amd.arrow import TimeColumnC
    return TimeColumnC(ms.addr if ms is not None else None, None, 0)


def interleave_yx(x, y):
    c = np.empty(2 * len(x), F64)
    c[0::2], c[1::2] = y, x
    return c


# ---------------------------------------------------------------- 1. element failures
# An index case: cols(rng, n) -> clean input columns; spoil(cols, bad) makes rows bad[0..2] fail; call(lib, h,
# ins, n, outs, status, summary, period, lenient) -> rc with pointer lists; outs: output dtypes; expect(O, cols,
# period, lenient) -> (outputs, status) from the oracle, failed rows zero.  period and lenient default to WEEK
# and strict, which every test of this file uses; test_gpu_dispatch.py walks the others.

def xyt_ms(rng, n):
    return [rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.integers(T2020, T2021, n)]


def xyt_off(rng, n):
    return [rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.integers(0, WEEK_MAX + 1, n)]


def spoil_xyt(bad_t):
    def f(c, bad):
        c[0][bad[0]] = 200.0      # out of bounds
        c[2][bad[1]] = bad_t      # before 1970 (epoch millis) / below the period (offsets)
        c[1][bad[2]] = -91.0
    return f


def envelopes(rng, n):
    cx, cy = rng.uniform(-170, 170, n), rng.uniform(-80, 80, n)
    w, h = 10 ** rng.uniform(-5, 0.9, n), 10 ** rng.uniform(-5, 0.9, n)
    return [cx - w, cy - h, cx + w, cy + h]


def spoil_env(c, bad):
    c[2][bad[0]] = 181.0                    # out of bounds
    c[0][bad[1]] = c[2][bad[1]] + 1.0       # unordered
    c[1][bad[2]] = -95.0


def loop_expect(n, row):
    """row(i) -> (status, [outputs]); a failed row's outputs are zero."""
    def f(dtypes):
        outs = [np.zeros(n, d) for d in dtypes]
        st = np.zeros(n, U8)
        for i in range(n):
            s, vals = row(i)
            st[i] = s
            if not s:
                for o, v in zip(outs, vals):
                    o[i] = v
        return outs, st
    return f


class IndexCase:
    def __init__(self, block, cols, spoil, outs, call, expect):
        self.block, self.cols, self.spoil, self.outs, self.call, self.expect = block, cols, spoil, outs, call, expect


def _c_z3_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_z3_index(h, i[0], i[1], i[2], n, period, 21, lenient, o[0], st, sm)

    def expect(O, c, period=WEEK, lenient=False):
        return loop_expect(len(c[0]), lambda i: (lambda s, z: (s, [z]))(
            *O.z3_index(c[0][i], c[1][i], int(c[2][i]), lenient, period, 21)))([I64])
    return IndexCase(256, xyt_off, spoil_xyt(-1), [I64], call, expect)


def _c_z3_index_key():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_z3_index_key(h, i[0], i[1], i[2], n, period, lenient, o[0], o[1], st, sm)

    def expect(O, c, period=WEEK, lenient=False):
        b, z, st = O.z3_index_key_batch(c[0], c[1], c[2], lenient, period)
        return [b, z], st
    return IndexCase(2048, xyt_ms, spoil_xyt(-5), [I16, I64], call, expect)


def _c_z2_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_z2_index(h, i[0], i[1], n, 31, lenient, o[0], st, sm)

    def spoil(c, bad):
        c[0][bad[0]] = 200.0
        c[1][bad[1]] = 90.5
        c[1][bad[2]] = -91.0

    def expect(O, c, period=WEEK, lenient=False):
        z, st = O.z2_index_batch(c[0], c[1], lenient)
        return [z], st
    return IndexCase(512, lambda rng, n: xyt_ms(rng, n)[:2], spoil, [I64], call, expect)


def _c_binned_time():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_binned_time(h, i[0], n, period, o[0], o[1], st, sm)

    def spoil(c, bad):
        c[0][bad[0]] = -1
        c[0][bad[1]] = 32768 * 604800000     # past the last week a short holds
        c[0][bad[2]] = -2**62

    def expect(O, c, period=WEEK, lenient=False):
        n = len(c[0])
        b, o, st = np.zeros(n, I16), np.zeros(n, I64), np.zeros(n, U8)
        for i in range(n):     # as test_binned_time_parity: the oracle's values, failed rows included
            st[i], b[i], o[i] = O.binned_time(period, int(c[0][i]))
        return [b, o], st
    return IndexCase(256, lambda rng, n: [rng.integers(T2020, T2021, n)], spoil, [I16, I64], call, expect)


def _c_xz2_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_xz2_index(h, i[0], i[1], i[2], i[3], n, 12, lenient, o[0], st, sm)

    def expect(O, c, period=WEEK, lenient=False):
        out, st = O.xz2_index_batch(np.stack(c, 1), lenient, 12)
        return [np.where(st != 0, 0, out)], st
    return IndexCase(512, envelopes, spoil_env, [I64], call, expect)


def _xz3_cols(rng, n):
    e = envelopes(rng, n)
    z0 = rng.uniform(0, WEEK_MAX - 2000, n)
    return [e[0], e[1], z0, e[2], e[3], z0 + rng.uniform(0, 1000, n)]


def _c_xz3_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_xz3_index(h, i[0], i[1], i[2], i[3], i[4], i[5], n, 12, period, lenient, o[0], st, sm)

    def spoil(c, bad):
        c[3][bad[0]] = 181.0
        c[2][bad[1]] = c[5][bad[1]] + 1.0     # zmin > zmax: unordered
        c[5][bad[2]] = WEEK_MAX + 1.0

    def expect(O, c, period=WEEK, lenient=False):
        out, st = O.xz3_index_batch(np.stack(c, 1), lenient, 12, period)
        return [np.where(st != 0, 0, out)], st
    return IndexCase(512, _xz3_cols, spoil, [I64], call, expect)


def _xz3_key_row(O, x0, y0, x1, y1, t, period=WEEK, lenient=False):
    s, b, off = O.binned_time(period, int(t))
    if s:
        return s, [0, 0]
    s, xz = O.xz3_index(x0, y0, float(off), x1, y1, float(off), lenient=lenient, g=12, period=period)
    return s, [b, xz]


def _c_xz3_index_key():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_xz3_index_key(h, i[0], i[1], i[2], i[3], i[4], n, 12, period, lenient, o[0], o[1], st, sm)

    def spoil(c, bad):
        c[2][bad[0]] = 181.0
        c[4][bad[1]] = -5                     # bad time
        c[0][bad[2]] = c[2][bad[2]] + 1.0     # unordered

    def expect(O, c, period=WEEK, lenient=False):
        return loop_expect(len(c[0]), lambda i: _xz3_key_row(O, c[0][i], c[1][i], c[2][i], c[3][i], c[4][i], period,
                                                                 lenient))([I16, I64])
    return IndexCase(256, lambda rng, n: envelopes(rng, n) + [rng.integers(T2020, T2021, n)], spoil, [I16, I64],
                     call, expect)


def _arrow_cols(rng, n):
    x, y, t = xyt_ms(rng, n)
    return [interleave_yx(x, y), t]


def _spoil_arrow(c, bad):
    c[0][2 * bad[0] + 1] = 200.0     # x
    c[1][bad[1]] = -5
    c[0][2 * bad[2]] = -91.0         # y


class _Ins:
    """Pointer list of an Arrow case: the structs live as long as the call."""

    def __init__(self, i):
        self.g = point_struct(None)
        self.g.coords = i[0].value if i[0] is not None else None
        self.t = time_struct(None)
        self.t.millis = i[1].value if i[1] is not None else None


def _c_z3_key_arrow():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        a = _Ins(i)
        return lib.gm_z3_index_key_arrow(h, ctypes.byref(a.g), ctypes.byref(a.t), n, period, lenient, o[0], o[1], st,
                                             sm)

    def expect(O, c, period=WEEK, lenient=False):
        b, z, st = O.z3_index_key_batch(c[0][1::2], c[0][0::2], c[1], lenient, period)
        return [b, z], st
    return IndexCase(2048, _arrow_cols, _spoil_arrow, [I16, I64], call, expect)


def _c_z2_key_arrow():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        a = _Ins(i)
        return lib.gm_z2_index_key_arrow(h, ctypes.byref(a.g), n, lenient, o[0], st, sm)

    def spoil(c, bad):
        _spoil_arrow(c, bad)
        c[0][2 * bad[1]] = 90.5

    def expect(O, c, period=WEEK, lenient=False):
        z, st = O.z2_index_batch(c[0][1::2], c[0][0::2], lenient)
        return [z], st
    return IndexCase(512, _arrow_cols, spoil, [I64], call, expect)


def _c_xz2_key_arrow():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        a = _Ins(i)
        return lib.gm_xz2_index_key_arrow(h, ctypes.byref(a.g), n, 12, lenient, o[0], st, sm)

    def spoil(c, bad):
        _spoil_arrow(c, bad)
        c[0][2 * bad[1]] = 90.5

    def expect(O, c, period=WEEK, lenient=False):
        x, y = c[0][1::2], c[0][0::2]
        out, st = O.xz2_index_batch(np.stack([x, y, x, y], 1), lenient, 12)
        return [np.where(st != 0, 0, out)], st
    return IndexCase(256, _arrow_cols, spoil, [I64], call, expect)


def _c_xz3_key_arrow():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        a = _Ins(i)
        return lib.gm_xz3_index_key_arrow(h, ctypes.byref(a.g), ctypes.byref(a.t), n, 12, period, lenient, o[0], o[1], st,
                                              sm)

    def expect(O, c, period=WEEK, lenient=False):
        x, y = c[0][1::2], c[0][0::2]
        return loop_expect(len(x), lambda i: _xz3_key_row(O, x[i], y[i], x[i], y[i], c[1][i], period, lenient))([I16, I64])
    return IndexCase(256, _arrow_cols, _spoil_arrow, [I16, I64], call, expect)


def _c_legacy_z3_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_legacy_z3_index(h, i[0], i[1], i[2], n, 0, period, lenient, o[0], st, sm)

    def expect(O, c, period=WEEK, lenient=False):
        return loop_expect(len(c[0]), lambda i: (lambda s, z: (s, [z]))(
            *O.legacy_z3_index(c[0][i], c[1][i], int(c[2][i]), lenient, period)))([I64])
    return IndexCase(256, xyt_off, spoil_xyt(-1), [I64], call, expect)


def _c_legacy_z2_index():
    def call(lib, h, i, n, o, st, sm, period=WEEK, lenient=0):
        return lib.gm_legacy_z2_index(h, i[0], i[1], n, lenient, o[0], st, sm)

    def spoil(c, bad):
        c[0][bad[0]] = 200.0
        c[1][bad[1]] = 90.5
        c[1][bad[2]] = -91.0

    def expect(O, c, period=WEEK, lenient=False):
        return loop_expect(len(c[0]), lambda i: (lambda s, z: (s, [z]))(
            *O.legacy_z2_index(c[0][i], c[1][i], lenient)))([I64])
    return IndexCase(256, lambda rng, n: xyt_ms(rng, n)[:2], spoil, [I64], call, expect)


INDEX_CASES = {
    "gm_z3_index": _c_z3_index, "gm_z3_index_key": _c_z3_index_key, "gm_z2_index": _c_z2_index,
    "gm_binned_time": _c_binned_time, "gm_xz2_index": _c_xz2_index, "gm_xz3_index": _c_xz3_index,
    "gm_xz3_index_key": _c_xz3_index_key, "gm_z3_index_key_arrow": _c_z3_key_arrow,
    "gm_z2_index_key_arrow": _c_z2_key_arrow, "gm_xz2_index_key_arrow": _c_xz2_key_arrow,
    "gm_xz3_index_key_arrow": _c_xz3_key_arrow, "gm_legacy_z3_index": _c_legacy_z3_index,
    "gm_legacy_z2_index": _c_legacy_z2_index,
}


def run_index(gpu, case, cols, n, with_status, with_summary, offsets=None, names=None):
    """One call on guarded buffers: (rc, outputs, status or None, summary or None); guards checked."""
    offsets = offsets or {}
    names = names or {}
    ins = [Guarded.of(c, offsets.get(names.get(("in", k)), 0)) for k, c in enumerate(cols)]
    outs = [Guarded(n * np.dtype(d).itemsize, offsets.get(names.get(("out", k)), 0))
            for k, d in enumerate(case.outs)]
    st = Guarded(n, offsets.get("status", 0)) if with_status else None
    sm = _lib.BatchStatus(7, 7, 7, 7) if with_summary else None
    rc = case.call(gpu.lib, gpu.handle, [P(g) for g in ins], n, [P(g) for g in outs], P(st),
                   ctypes.byref(sm) if sm is not None else None)
    sync(gpu)
    check_all(ins + outs + [st])
    return (rc, [g.read(d) for g, d in zip(outs, case.outs)], st.read(U8) if st is not None else None,
            (sm.n_errors, sm.first_index, sm.first_code) if sm is not None else None)


@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_element_failures(gpu, oracle, name):
    """The element-failure rule of the header on n = 2 x block + 5 rows with three failed rows (row 1, a row of
    the second block, the odd last row): GM_E_ELEMENT exactly with a summary and without a status; summary,
    status and every output row (failed rows zero) as the oracle's in all four combinations."""
    case = INDEX_CASES[name]()
    n = 2 * case.block + 5
    bad = [1, case.block + 7, n - 1]
    rng = np.random.default_rng(len(name) * 131 + n)
    clean = case.cols(rng, n)
    cols = [c.copy() for c in clean]
    case.spoil(cols, bad)
    exp, est = case.expect(oracle, cols)
    assert np.flatnonzero(est).tolist() == bad, "the oracle fails exactly the chosen rows"
    for with_status in (False, True):
        for with_summary in (False, True):
            what = (name, with_status, with_summary)
            rc, outs, st, sm = run_index(gpu, case, cols, n, with_status, with_summary)
            assert rc == (E_ELEMENT if with_summary and not with_status else OK), what
            if with_summary:
                assert sm == (3, 1, int(est[1])), what
            if with_status:
                assert np.array_equal(st, est), what
            for got, want in zip(outs, exp):
                assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
    # a clean batch: GM_OK and {0, -1, 0}, with and without a status
    cexp, cst = case.expect(oracle, clean)
    assert not cst.any()
    for with_status in (False, True):
        rc, outs, st, sm = run_index(gpu, case, clean, n, with_status, True)
        assert rc == OK and sm == (0, -1, 0), (name, rc, sm)
        assert all(np.array_equal(g, w) for g, w in zip(outs, cexp))
    # n == 0 with NULL columns
    sm = _lib.BatchStatus(7, 7, 7, 7)
    rc = case.call(gpu.lib, gpu.handle, [None] * len(clean), 0, [None] * len(case.outs), None, ctypes.byref(sm))
    assert rc == OK and (sm.n_errors, sm.first_index, sm.first_code) == (0, -1, 0)


# ---------------------------------------------------------------- ranges: shared cases
MR = 200     # maxRanges of every ranges case here


def _z3r(O):
    qs = [([(-10.0, 35.0, 30.0, 60.0)], [(1000, 90000)]), ([(170.0, 0.0, 190.0, 10.0)], [(0, 100)]),
          ([(100.0, -40.0, 120.0, -10.0), (5.0, 5.0, 6.0, 6.0)], [(0, 5000), (300000, 400000)])]
    bo = np.cumsum([0] + [len(q[0]) for q in qs]).astype(I32)
    to = np.cumsum([0] + [len(q[1]) for q in qs]).astype(I32)
    xy = np.array([v for q in qs for b in q[0] for v in b], F64)
    tt = np.array([v for q in qs for t in q[1] for v in t], I64)

    def call(lib, h, sel, out_off, out, cap, needed, qst):
        b, t = _sub_off(bo, sel), _sub_off(to, sel)
        x = np.concatenate([xy[4 * bo[q]:4 * bo[q + 1]] for q in sel])
        tv = np.concatenate([tt[2 * to[q]:2 * to[q + 1]] for q in sel])
        return lib.gm_z3_ranges(h, len(sel), b.ctypes.data, x.ctypes.data, t.ctypes.data, tv.ctypes.data, WEEK, 21, 64,
                                MR, -1, out_off, out, cap, needed, qst)
    return qs, call, lambda q: O.z3_ranges(q[0], q[1], 64, MR, WEEK), 1


def _sub_off(off, sel):
    return np.cumsum([0] + [int(off[q + 1] - off[q]) for q in sel]).astype(I32)


def _z2r(O):
    qs = [[(-10.0, 35.0, 30.0, 60.0)], [(170.0, 0.0, 190.0, 10.0)], [(100.0, -40.0, 120.0, -10.0), (5.0, 5.0, 6.0, 6.0)]]

    def call(lib, h, sel, out_off, out, cap, needed, qst):
        b = np.cumsum([0] + [len(qs[q]) for q in sel]).astype(I32)
        x = np.array([v for q in sel for bx in qs[q] for v in bx], F64)
        return lib.gm_z2_ranges(h, len(sel), b.ctypes.data, x.ctypes.data, 31, 64, MR, -1, out_off, out, cap, needed,
                                qst)
    return qs, call, lambda q: O.z2_ranges(q, 64, MR), 1


def _zr(O):
    Z = lambda x, y, t: O.z3_apply(x, y, t)  # noqa: E731
    qs = [[(Z(2, 2, 0), Z(3, 6, 3))], [(10, 5)], [(Z(100, 7, 50), Z(900, 300, 60)), (Z(5, 5, 5), Z(5, 5, 5) + 1000)]]

    def call(lib, h, sel, out_off, out, cap, needed, qst):
        b = np.cumsum([0] + [len(qs[q]) for q in sel]).astype(I32)
        zb = np.array([v for q in sel for bd in qs[q] for v in bd], I64)
        return lib.gm_zranges(h, 3, len(sel), b.ctypes.data, zb.ctypes.data, 64, MR, -1, out_off, out, cap, needed, qst)
    return qs, call, lambda q: O.zranges(3, q, 64, MR, 7), 3


def _xz2r(O):
    qs = [[(-10.0, 35.0, 30.0, 60.0)], [(170.0, 0.0, 190.0, 10.0)], [(100.0, -40.0, 120.0, -10.0), (5.0, 5.0, 6.0, 6.0)]]

    def call(lib, h, sel, out_off, out, cap, needed, qst):
        b = np.cumsum([0] + [len(qs[q]) for q in sel]).astype(I32)
        w = np.array([v for q in sel for bx in qs[q] for v in bx], F64)
        return lib.gm_xz2_ranges(h, len(sel), b.ctypes.data, w.ctypes.data, 12, MR, out_off, out, cap, needed, qst)
    return qs, call, lambda q: O.xz2_ranges(q, MR, 12), 1


def _xz3r(O):
    qs = [[(-10.0, 35.0, 1000.0, 30.0, 60.0, 90000.0)], [(170.0, 0.0, 0.0, 190.0, 10.0, 100.0)],
          [(100.0, -40.0, 0.0, 120.0, -10.0, 5000.0), (5.0, 5.0, 300000.0, 6.0, 6.0, 400000.0)]]

    def call(lib, h, sel, out_off, out, cap, needed, qst):
        b = np.cumsum([0] + [len(qs[q]) for q in sel]).astype(I32)
        w = np.array([v for q in sel for bx in qs[q] for v in bx], F64)
        return lib.gm_xz3_ranges(h, len(sel), b.ctypes.data, w.ctypes.data, 12, WEEK, MR, out_off, out, cap, needed,
                                 qst)
    return qs, call, lambda q: O.xz3_ranges(q, MR, 12, WEEK), 1


RANGES = {"gm_z3_ranges": _z3r, "gm_z2_ranges": _z2r, "gm_zranges": _zr, "gm_xz2_ranges": _xz2r,
          "gm_xz3_ranges": _xz3r}


def host_ranges(cap, pad=64):
    """A host gm_range buffer of cap entries with `pad` guard entries behind it, all 0xA5."""
    return np.full((cap + pad) * 24, FILL, U8)


def range_rows(raw, a, b):
    r = raw[24 * a:24 * b].view(_RANGE)
    return [(int(x["lower"]), int(x["upper"]), bool(x["contained"])) for x in r]


_RANGE = np.dtype([("lower", "<i8"), ("upper", "<i8"), ("contained", "<i4"), ("reserved", "<i4")])


@pytest.mark.parametrize("name", list(RANGES))
def test_ranges_failed_query(gpu, oracle, name):
    """A three-query batch whose middle query fails (unordered bounds / a box outside the world): with
    query_status the codes come back and rc is GM_OK, without it rc is GM_E_ELEMENT; offsets, *needed and the
    two good queries' lists are delivered, equal to the oracle's, both times."""
    qs, call, orc, code = RANGES[name](oracle)
    exp = [orc(qs[0]), None, orc(qs[2])]
    assert exp[0] and exp[2]
    for with_status in (True, False):
        out_off = np.full(4, -7, I64)
        out = host_ranges(4096)
        needed = ctypes.c_int64(-7)
        qst = np.full(3, -7, I32)
        rc = call(gpu.lib, gpu.handle, [0, 1, 2], out_off.ctypes.data, out.ctypes.data, 4096, ctypes.byref(needed),
                  qst.ctypes.data if with_status else None)
        assert rc == (OK if with_status else E_ELEMENT), (name, with_status, rc)
        if with_status:
            assert qst.tolist() == [0, code, 0]
        assert out_off[0] == 0 and needed.value == out_off[3] and np.all(np.diff(out_off) >= 0)
        for q in (0, 2):
            assert range_rows(out, int(out_off[q]), int(out_off[q + 1])) == exp[q], (name, with_status, q)
        assert untouched(out[24 * int(out_off[3]):])
    # a batch without a failed query stays GM_OK without query_status
    out_off, out, needed = np.full(3, -7, I64), host_ranges(4096), ctypes.c_int64(-7)
    assert call(gpu.lib, gpu.handle, [0, 2], out_off.ctypes.data, out.ctypes.data, 4096, ctypes.byref(needed), None) == OK
    assert needed.value == len(exp[0]) + len(exp[2])


@pytest.mark.parametrize("name", list(RANGES))
def test_ranges_failed_query_pipelined(gpu, oracle, name):
    """The batch of test_ranges_failed_query into page-locked output in pipelined chunks of one query
    (GM_PARAM_RANGES_CHUNK = 1): the failing middle query's status lands in its own slot, the third query's
    offsets are rebased on the first's total and the failure reaches the return code across chunks.  rc, the
    statuses, the offsets, *needed and both good lists equal the one-batch pageable call's and the oracle's."""
    import torch
    qs, call, orc, code = RANGES[name](oracle)
    exp = [orc(qs[0]), None, orc(qs[2])]
    assert exp[0] and exp[2]
    off1, out1, need1, qst1 = np.full(4, -7, I64), host_ranges(4096), ctypes.c_int64(-7), np.full(3, -7, I32)
    assert call(gpu.lib, gpu.handle, [0, 1, 2], off1.ctypes.data, out1.ctypes.data, 4096, ctypes.byref(need1),
                qst1.ctypes.data) == OK
    total = int(off1[3])
    assert qst1.tolist() == [0, code, 0] and need1.value == total == len(exp[0]) + len(exp[2])
    pinned = torch.empty((4096 + 64) * 24, dtype=torch.uint8, pin_memory=True)
    out = pinned.numpy()
    gpu.set_param(_lib.GM_PARAM_RANGES_CHUNK, 1)
    try:
        for with_status in (True, False):
            out[:] = FILL
            out_off, needed, qst = np.full(4, -7, I64), ctypes.c_int64(-7), np.full(3, -7, I32)
            rc = call(gpu.lib, gpu.handle, [0, 1, 2], out_off.ctypes.data, out.ctypes.data, 4096, ctypes.byref(needed),
                      qst.ctypes.data if with_status else None)
            assert rc == (OK if with_status else E_ELEMENT), (name, with_status, rc)
            if with_status:
                assert qst.tolist() == [0, code, 0]
            assert out_off.tolist() == off1.tolist() and needed.value == total, (name, with_status)
            assert np.array_equal(out[:24 * total], out1[:24 * total]), (name, with_status)
            for q in (0, 2):
                assert range_rows(out, int(out_off[q]), int(out_off[q + 1])) == exp[q], (name, with_status, q)
            assert untouched(out[24 * total:])
    finally:
        gpu.set_param(_lib.GM_PARAM_RANGES_CHUNK, 0)


@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("name", list(RANGES))
def test_ranges_capacity(gpu, oracle, name, device_out):
    """cap in {0, total - 1, total}: *needed == total every time, GM_E_CAPACITY below total with nothing
    written past cap (host and device `out`), and the oracle's lists at cap == total."""
    qs, call, orc, _ = RANGES[name](oracle)
    exp = orc(qs[0]) + orc(qs[2])
    total = len(exp)
    assert total > 2
    for cap in (0, total - 1, total):
        out_off, needed = np.full(3, -7, I64), ctypes.c_int64(-7)
        dev = Guarded(cap * 24) if device_out else None
        host = None if device_out else host_ranges(cap)
        rc = call(gpu.lib, gpu.handle, [0, 2], out_off.ctypes.data, dev.ptr if device_out else host.ctypes.data, cap,
                  ctypes.byref(needed), None)
        sync(gpu)
        assert rc == (E_CAPACITY if cap < total else OK), (name, cap, rc)
        assert needed.value == total, (name, cap, needed.value)
        if device_out:
            dev.check("%s cap %d" % (name, cap))
            raw = dev.read()
        else:
            assert untouched(host[24 * cap:]), (name, cap)
            raw = host
        if cap == total:
            assert range_rows(raw, 0, total) == exp and out_off.tolist() == [0, len(orc(qs[0])), total]


# ---------------------------------------------------------------- 2. scans: capacity and bounds
SCAN_N = 2 * 4096 + 77     # two full FROWS blocks and a ragged third
BBOX = np.array([-180.0, -90.0, 0.0, 90.0])


def _pack(mask):
    n = len(mask)
    m = np.zeros(((n + 63) // 64) * 64, bool)
    m[:n] = mask
    return np.packbits(m, bitorder="little").view(U64)


@functools.lru_cache(maxsize=None)
def scan_data():
    import oracle as O
    rng = np.random.default_rng(2024)
    x, y, t = xyt_ms(rng, SCAN_N)
    b, z, st = O.z3_index_key_batch(x, y, t, False, WEEK)
    z2, st2 = O.z2_index_batch(x, y, False)
    assert not st.any() and not st2.any()
    return x, y, t, b, z, z2


def _filters():
    from geomesa_amd import filters as F
    f3 = F.Z3Filter([[0, 0, (1 << 20) - 1, (1 << 21) - 1]], [], 32767, -32768)       # lon < 0: about half
    f2 = F.Z2Filter([[0, 0, (1 << 30) - 1, (1 << 31) - 1]])
    return F.serialize_to_bytes(f3), F.z2_serialize_to_bytes(f2)


def _key_rows(keys):
    from test_gpu_boundary import _rows
    return _rows(keys, np.random.default_rng(5))


def _query_polys():
    from geomesa_amd.join import PolygonIndex, PolygonSet
    from test_gpu_query import SHAPES
    ps = PolygonSet.from_wkt(SHAPES)
    return ps, PolygonIndex(ps)


class Scan:
    """One scan entry point on fixed inputs: the guarded input buffers (offsets by column name), the expected
    mask, and call(mask, ids, cap, n_match) -> rc."""

    def __init__(self, gpu, oracle, kind, offsets=None):
        off = offsets or {}
        lib, h = gpu.lib, gpu.handle
        x, y, t, b, z, z2 = scan_data()
        fb3, fb2 = _filters()
        a3, a2 = np.frombuffer(fb3, U8).copy(), np.frombuffer(fb2, U8).copy()
        self.keep = [a3, a2, BBOX]
        G = lambda name, arr: Guarded.of(arr, off.get(name, 0))  # noqa: E731
        dur = (T2020 + 1000, T2021 - 1000)
        if kind == "gm_z3filter_scan":
            self.ins = [G("bin", b), G("z", z)]
            self.mask = oracle.z3filter_scan(fb3, [], b, z)
            self.call = lambda m, i, c, nm: lib.gm_z3filter_scan(h, a3.ctypes.data, len(a3), None, 0, P(self.ins[0]),
                                                                 P(self.ins[1]), SCAN_N, m, i, c, nm)
        elif kind == "gm_z2filter_scan":
            self.ins = [G("z", z2)]
            self.mask = oracle.z2filter_scan(fb2, z2)
            self.call = lambda m, i, c, nm: lib.gm_z2filter_scan(h, a2.ctypes.data, len(a2), P(self.ins[0]), SCAN_N, m,
                                                                 i, c, nm)
        elif kind == "gm_z3filter_scan_rows":
            keys = np.concatenate([b.astype(">i2").view(U8).reshape(-1, 2), z.astype(">i8").view(U8).reshape(-1, 8)], 1)
            buf, ro = _key_rows(keys)
            self.ins = [G("rows", buf), G("row_off", ro)]
            self.mask = oracle.z3filter_scan(fb3, [], b, z)
            self.call = lambda m, i, c, nm: lib.gm_z3filter_scan_rows(h, a3.ctypes.data, len(a3), P(self.ins[0]),
                                                                      P(self.ins[1]), 0, SCAN_N, m, i, c, nm, None)
        elif kind == "gm_z2filter_scan_rows":
            buf, ro = _key_rows(z2.astype(">i8").view(U8).reshape(-1, 8))
            self.ins = [G("rows", buf), G("row_off", ro)]
            self.mask = oracle.z2filter_scan(fb2, z2)
            self.call = lambda m, i, c, nm: lib.gm_z2filter_scan_rows(h, a2.ctypes.data, len(a2), P(self.ins[0]),
                                                                      P(self.ins[1]), 0, SCAN_N, m, i, c, nm, None)
        elif kind == "gm_strict_scan":
            self.ins = [G("x", x), G("y", y), G("t_ms", t)]
            self.mask = oracle.strict_scan(x, y, t, BBOX, dur)
            self.call = lambda m, i, c, nm: lib.gm_strict_scan(h, P(self.ins[0]), P(self.ins[1]), P(self.ins[2]), SCAN_N,
                                                               BBOX.ctypes.data, 1, dur[0], dur[1], m, i, c, nm)
        elif kind == "gm_query_scan":
            self.ins = [G("x", x), G("y", y), G("t_ms", t)]
            self.mask = oracle.query_scan(x, y, t, bbox=BBOX, during=dur)
            self.call = lambda m, i, c, nm: lib.gm_query_scan(h, P(self.ins[0]), P(self.ins[1]), P(self.ins[2]), SCAN_N,
                                                              BBOX.ctypes.data, 1, dur[0], dur[1], None, 0, m, i, c, nm)
        else:   # gm_query_scan with a geometry term: points over the query shapes, a during that keeps most
            assert kind == "gm_query_scan+geom"
            from test_gpu_query import _points
            ps, self.ix = _query_polys()
            qx, qy, qt = _points(SCAN_N, 5, ps)
            k = np.random.default_rng(6).permutation(len(qx))[:SCAN_N]
            qx, qy, qt = qx[k], qy[k], qt[k]
            self.ins = [G("x", qx), G("y", qy), G("t_ms", qt)]
            ops = oracle.OraclePolySet(*ps.to_arrays())
            self.mask = oracle.query_scan(qx, qy, qt, during=(50, 990), polys=ops, op=1)
            self.call = lambda m, i, c, nm: lib.gm_query_scan(h, P(self.ins[0]), P(self.ins[1]), P(self.ins[2]), SCAN_N,
                                                              None, 1, 50, 990, self.ix._h, 1, m, i, c, nm)
        self.ids = np.flatnonzero(self.mask)
        self.m = len(self.ids)
        self.words = _pack(self.mask)

    def run(self, gpu, cap, want_mask=True, want_ids=True, offsets=None):
        """(rc, n_match) of one call; asserts the mask words, the first min(m, cap) ids, the untouched rest
        of ids and every guard."""
        off = offsets or {}
        mask = Guarded(len(self.words) * 8, off.get("mask", 0)) if want_mask else None
        ids = Guarded(cap * 8, off.get("ids", 0)) if want_ids else None
        nm = ctypes.c_int64(-7)
        rc = self.call(P(mask), P(ids), cap if want_ids else 0, ctypes.byref(nm))
        sync(gpu)
        check_all(self.ins + [mask, ids])
        if want_mask:
            got = mask.read(U64)
            assert np.array_equal(got, self.words), np.flatnonzero(got != self.words)[:8]
        if want_ids:
            got = ids.read(I64)
            k = min(self.m, cap)
            assert np.array_equal(got[:k], self.ids[:k])
            assert untouched(got[k:])
        return rc, nm.value


SCANS = ["gm_z3filter_scan", "gm_z2filter_scan", "gm_z3filter_scan_rows", "gm_z2filter_scan_rows", "gm_strict_scan",
         "gm_query_scan", "gm_query_scan+geom"]


@pytest.mark.parametrize("kind", SCANS)
def test_scan_capacity_and_bounds(gpu, oracle, kind):
    """n = 2 x 4096 + 77 rows, about half of them matching, ids_cap around the match count m: GM_E_CAPACITY
    exactly when m > ids_cap, *n_match == m always, the first min(m, ids_cap) ids ascending as the oracle's,
    nothing written past ids_cap, the mask exactly ceil(n / 64) words with zero tail bits."""
    s = Scan(gpu, oracle, kind)
    m = s.m
    assert SCAN_N // 8 < m < SCAN_N * 7 // 8
    assert int(sum(bin(int(w)).count("1") for w in s.words)) == m
    for cap in (0, 1, m - 1, m, m + 1):
        rc, nm = s.run(gpu, cap)
        assert rc == (E_CAPACITY if m > cap else OK), (kind, cap, rc)
        assert nm == m, (kind, cap, nm)
    assert s.run(gpu, 0, want_ids=False) == (OK, m)                    # mask only
    assert s.run(gpu, m, want_mask=False) == (OK, m)                   # ids only
    assert s.run(gpu, 0, want_mask=False, want_ids=False) == (OK, m)   # count only


@pytest.mark.parametrize("kind", SCANS)
def test_scan_negative_ids_cap(gpu, oracle, kind):
    """ids != NULL with ids_cap < 0 is GM_E_INVALID in every scan (no kernel runs)."""
    s = Scan(gpu, oracle, kind)
    ids = Guarded(64)
    nm = ctypes.c_int64(-7)
    for cap in (-1, -2**40):
        assert s.call(None, ids.ptr, cap, ctypes.byref(nm)) == E_INVALID, (kind, cap)
    sync(gpu)
    ids.check(kind)
    assert untouched(ids.read()) and nm.value == -7


# ---------------------------------------------------------------- 2. join: capacity and bounds
JOIN_GUARD = 65536     # a slab is 4096 pairs: 32 KiB of point ids


@functools.lru_cache(maxsize=None)
def join_data():
    from geomesa_amd.join import PolygonIndex, synthetic_counties, synthetic_points
    from test_gpu_join_faults import _edge_points
    ps = synthetic_counties(6, 3)
    px, py = synthetic_points(17_001, seed=11)
    ex, ey = _edge_points(ps, 1e-4, np.random.default_rng(12))
    px, py = np.concatenate([px, ex]), np.concatenate([py, ey])
    k = np.random.default_rng(13).permutation(len(px))
    return ps, PolygonIndex(ps), px[k], py[k]


def oracle_pairs(oracle, pred):
    ps, _, px, py = join_data()
    pt, pl = oracle.OraclePolySet(*ps.to_arrays()).join(px, py, nthreads=8, predicate=pred)
    return sorted(zip(pt.tolist(), pl.tolist()))


def run_join(gpu, kind, pred, cap, ins, want_count=True, offsets=None):
    """One join on guarded outputs: (rc, n_pairs or None, pt_ids payload, poly_ids payload)."""
    off = offsets or {}
    _, ix, px, _ = join_data()
    n = len(px)
    pt = Guarded(cap * 8, off.get("pt_ids", 0), JOIN_GUARD)
    pl = Guarded(cap * 4, off.get("poly_ids", 0), JOIN_GUARD)
    npairs = ctypes.c_int64(-7)
    cnt = ctypes.byref(npairs) if want_count else None
    code = _lib.GM_SPATIAL_INTERSECTS if pred == "st_intersects" else _lib.GM_SPATIAL_CONTAINS
    if kind == "arrow":
        g = point_struct(ins[0])
        rc = gpu.lib.gm_pip_join_arrow(gpu.handle, ix._h, ctypes.byref(g), n, 0, pt.ptr, pl.ptr, cap, cnt, 0, code)
    else:
        rc = gpu.lib.gm_pip_join_pred(gpu.handle, ix._h, ins[0].ptr, ins[1].ptr, n, 0, pt.ptr, pl.ptr, cap, cnt, 0, code)
    sync(gpu)
    check_all(list(ins) + [pt, pl], "join cap %d" % cap)
    return rc, (npairs.value if want_count else None), pt.read(I64), pl.read(I32)


def join_inputs(kind, offsets=None):
    off = offsets or {}
    _, _, px, py = join_data()
    if kind == "arrow":
        return [Guarded.of(interleave_yx(px, py))]
    return [Guarded.of(px, off.get("px", 0)), Guarded.of(py, off.get("py", 0))]


@pytest.mark.parametrize("kind,pred", [("pred", "st_contains"), ("pred", "st_intersects"), ("arrow", "st_contains")])
def test_join_capacity_and_bounds(gpu, oracle, kind, pred):
    """About 23,000 points (edge points included) on 18 polygons, cap around the pair count p with non-NULL
    arrays: the oracle's pair set and GM_OK for cap >= p, GM_E_CAPACITY and *n_pairs == p below, and 64 KiB of
    guard behind both arrays untouched every time -- also over several chunks and in the stream-ordered form."""
    exp = oracle_pairs(oracle, pred)
    p = len(exp)
    assert p > 4096     # more than one slab of pairs
    ins = join_inputs(kind)
    for cap in (0, 1, p - 1, p, p + 1):
        rc, k, pt, pl = run_join(gpu, kind, pred, cap, ins)
        assert k == p, (cap, k, p)
        assert rc == (OK if cap >= p else E_CAPACITY), (cap, rc)
        if cap >= p:
            assert sorted(zip(pt[:p].tolist(), pl[:p].tolist())) == exp, cap
    gpu.set_param(_lib.GM_PARAM_JOIN_CHUNK, 4096)     # several chunks append to one output
    try:
        rc, k, pt, pl = run_join(gpu, kind, pred, p, ins)
    finally:
        gpu.set_param(_lib.GM_PARAM_JOIN_CHUNK, 0)
    assert (rc, k) == (OK, p) and sorted(zip(pt.tolist(), pl.tolist())) == exp
    rc, _, pt, pl = run_join(gpu, kind, pred, p, ins, want_count=False)     # stream-ordered, then gm_ctx_sync
    assert rc == OK and sorted(zip(pt.tolist(), pl.tolist())) == exp


# ---------------------------------------------------------------- 2. fixed-size outputs
def _key_cols(n, seed):
    rng = np.random.default_rng(seed)
    sh = rng.integers(0, 4, n).astype(U8)
    b = rng.integers(-3, 2700, n).astype(I16)
    z = rng.integers(-2**63, 2**63 - 1, n, dtype=I64)
    z[: n // 2] = z[rng.integers(0, max(n // 8, 1), n // 2)]     # duplicated keys
    return sh, b, z


@pytest.mark.parametrize("n", [2 * 256 + 5, 1])      # k_key_bytes: STPB = 256 rows per block
@pytest.mark.parametrize("sharded", [False, True])
def test_key_bytes_bounds(gpu, n, sharded):
    """gm_z3_key_bytes / gm_z2_key_bytes write exactly n x key_len bytes: [shard?][bin BE16][z BE64]."""
    sh, b, z = _key_cols(n, n + sharded)
    S, B, Z = (Guarded.of(sh) if sharded else None), Guarded.of(b), Guarded.of(z)
    parts = ([sh.reshape(-1, 1)] if sharded else []) + [b.astype(">i2").view(U8).reshape(-1, 2),
                                                       z.astype(">i8").view(U8).reshape(-1, 8)]
    for k3 in (True, False):
        exp = np.concatenate(parts if k3 else parts[:-2] + parts[-1:], 1)
        out = Guarded(exp.size)
        if k3:
            rc = gpu.lib.gm_z3_key_bytes(gpu.handle, P(S), B.ptr, Z.ptr, n, out.ptr)
        else:
            rc = gpu.lib.gm_z2_key_bytes(gpu.handle, P(S), Z.ptr, n, out.ptr)
        sync(gpu)
        assert rc == OK and exp.shape[1] == (10 if k3 else 8) + sharded
        check_all([S, B, Z, out])
        assert np.array_equal(out.read().reshape(n, -1), exp)


@pytest.mark.parametrize("n", [2 * 4096 + 5, 1])
@pytest.mark.parametrize("sharded,binned", [(True, True), (False, True), (False, False)])
def test_sort_keys_bounds(gpu, n, sharded, binned):
    """gm_sort_keys: all four outputs hold the stable table order (table_scan_cases.table_order) and nothing
    is written around them."""
    import table_scan_cases as C
    sh, b, z = _key_cols(n, 3 * n + sharded + 2 * binned)
    sh, b = (sh if sharded else None), (b if binned else None)
    order = C.table_order(sh, b, z)
    ins = [Guarded.of(sh) if sharded else None, Guarded.of(b) if binned else None, Guarded.of(z)]
    outs = [Guarded(n) if sharded else None, Guarded(2 * n) if binned else None, Guarded(8 * n), Guarded(8 * n)]
    rc = gpu.lib.gm_sort_keys(gpu.handle, P(ins[0]), P(ins[1]), P(ins[2]), n, P(outs[0]), P(outs[1]), P(outs[2]),
                              P(outs[3]))
    sync(gpu)
    assert rc == OK
    check_all(ins + outs)
    if sharded:
        assert np.array_equal(outs[0].read(U8), sh[order])
    if binned:
        assert np.array_equal(outs[1].read(I16), b[order])
    assert np.array_equal(outs[2].read(I64), z[order]) and np.array_equal(outs[3].read(I64), order)


@pytest.mark.parametrize("n", [2 * 2048 + 5, 1, 0])      # XTILE = 2048 rows per tile
def test_key_partition_bounds(gpu, oracle, n):
    """gm_key_partition with all five device outputs against oracle.key_partition; n == 0 writes zero counts."""
    sh, b, z = _key_cols(max(n, 1), 17 + n)
    sh, b, z = sh[:n], b[:n], z[:n]
    hi, lo = oracle.table_key_u64(*_key_cols(64, 99))
    k = np.lexsort((lo, hi))[[10, 30, 30, 50]]      # ascending splitters, one repeated
    sp_hi, sp_lo = np.ascontiguousarray(hi[k]), np.ascontiguousarray(lo[k])
    order, counts = oracle.key_partition(sh, b, z, sp_hi, sp_lo)
    ins = [Guarded.of(sh), Guarded.of(b), Guarded.of(z)]
    outs = [Guarded(n), Guarded(2 * n), Guarded(8 * n), Guarded(8 * n), Guarded(4 * n)]
    dc = np.full(5 + 3, -7, I64)
    rc = gpu.lib.gm_key_partition(gpu.handle, *[g.ptr for g in ins], n, sp_hi.ctypes.data, sp_lo.ctypes.data, 4, None,
                                  1000, *[g.ptr for g in outs], dc.ctypes.data)
    sync(gpu)
    assert rc == OK
    check_all(ins + outs)
    assert dc[:5].tolist() == counts.tolist() and np.all(dc[5:] == -7)
    if n:
        assert np.array_equal(outs[0].read(U8), sh[order]) and np.array_equal(outs[1].read(I16), b[order])
        assert np.array_equal(outs[2].read(I64), z[order])
        assert np.array_equal(outs[3].read(I64), order + 1000) and np.array_equal(outs[4].read(U32), order)


def _relate_rows(n, seed):
    from geomesa_amd.join import PolygonIndex, synthetic_counties
    from test_gpu_relate import NX, NY, rows
    ps = synthetic_counties(NX, NY)
    poly, px, py = rows(ps, max(n, 16), seed)
    return ps, PolygonIndex(ps), poly[:n], px[:n], py[:n]


@functools.lru_cache(maxsize=None)
def relate_case(n):
    import oracle as O
    ps, ix, poly, px, py = _relate_rows(n, 31)
    ops = O.OraclePolySet(*ps.to_arrays())
    exp = np.array([255 if p < 0 else ops.locate(int(p), x, y) for p, x, y in zip(poly, px, py)], U8)
    return ix, poly, px, py, exp


def run_relate(gpu, n, offsets=None):
    off = offsets or {}
    ix, poly, px, py, exp = relate_case(n)
    ins = [Guarded.of(poly, off.get("poly", 0)), Guarded.of(px, off.get("px", 0)), Guarded.of(py, off.get("py", 0))]
    loc = Guarded(n, off.get("loc", 0))
    rc = gpu.lib.gm_pip_relate(gpu.handle, ix._h, ins[0].ptr, ins[1].ptr, ins[2].ptr, n, loc.ptr)
    sync(gpu)
    assert rc == OK
    check_all(ins + [loc])
    got = loc.read(U8)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]


@pytest.mark.parametrize("n", [2 * 2048 + 5, 1])      # k_pip_relate: RTPB 1024 x RILP 2 rows per block
def test_relate_bounds(gpu, oracle, n):
    """gm_pip_relate writes exactly n location bytes, each the oracle's PointLocator result."""
    run_relate(gpu, n)


@pytest.mark.parametrize("n", [2 * 256 + 5, 1])
def test_points_to_columns_bounds(gpu, n):
    """gm_arrow_points_to_columns: the [y, x] tuples de-interleaved into exactly n x and n y values."""
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    c = Guarded.of(interleave_yx(x, y))
    X, Y = Guarded(8 * n), Guarded(8 * n)
    g = point_struct(c)
    rc = gpu.lib.gm_arrow_points_to_columns(gpu.handle, ctypes.byref(g), n, X.ptr, Y.ptr)
    sync(gpu)
    assert rc == OK
    check_all([c, X, Y])
    assert np.array_equal(X.read(I64), x.view(I64)) and np.array_equal(Y.read(I64), y.view(I64))


def _invert(name):
    """(block rows, call(lib, h, z, n, outs), output dtypes, expect(O, z))"""
    if name == "gm_z3_invert":      # k_z3_invert: TPB 256 x UNROLL_INV 2 pairs
        return (1024, lambda lib, h, z, n, o: lib.gm_z3_invert(h, z, n, WEEK, 21, o[0], o[1], o[2]), [F64, F64, I64],
                lambda O, z: O.z3_invert_batch(z, WEEK))
    if name == "gm_z2_invert":      # k_z2_invert: TPB 256 x UNROLL_INV2 1 pair
        return (512, lambda lib, h, z, n, o: lib.gm_z2_invert(h, z, n, 31, o[0], o[1]), [F64, F64],
                lambda O, z: O.z2_invert_batch(z))
    if name == "gm_legacy_z3_invert":
        def exp3(O, z):
            r = [O.legacy_z3_invert(int(v), WEEK) for v in z]
            return [np.array([a[k] for a in r], d) for k, d in enumerate([F64, F64, I64])]
        return (256, lambda lib, h, z, n, o: lib.gm_legacy_z3_invert(h, z, n, 0, WEEK, o[0], o[1], o[2]),
                [F64, F64, I64], exp3)

    def exp2(O, z):
        r = [O.legacy_z2_invert(int(v)) for v in z]
        return [np.array([a[k] for a in r], F64) for k in range(2)]
    return (256, lambda lib, h, z, n, o: lib.gm_legacy_z2_invert(h, z, n, o[0], o[1]), [F64, F64], exp2)


def run_invert(gpu, oracle, name, n, offsets=None):
    off = offsets or {}
    _, call, dts, expect = _invert(name)
    rng = np.random.default_rng(n + len(name))
    z = rng.integers(0, 2**63 - 1, n, dtype=I64)
    z[::7] = rng.integers(-2**63, 0, len(z[::7]), dtype=I64)
    Z = Guarded.of(z, off.get("z", 0))
    names = ["x", "y", "t"]
    outs = [Guarded(8 * n, off.get(names[k], 0)) for k in range(len(dts))]
    rc = call(gpu.lib, gpu.handle, Z.ptr, n, [g.ptr for g in outs])
    sync(gpu)
    assert rc == OK
    check_all([Z] + outs)
    for g, want in zip(outs, expect(oracle, z)):
        assert np.array_equal(g.read(I64), np.ascontiguousarray(want).view(I64)), name


@pytest.mark.parametrize("name", ["gm_z3_invert", "gm_z2_invert", "gm_legacy_z3_invert", "gm_legacy_z2_invert"])
def test_invert_bounds(gpu, oracle, name):
    """The invert entry points at n = 2 x block + 5 and n = 1: bit-equal to the oracle, guards untouched."""
    for n in (2 * _invert(name)[0] + 5, 1):
        run_invert(gpu, oracle, name, n)


# ---------------------------------------------------------------- 2. histogram
HIST_N = 10_001
HIST_SHAPES = {"lds": (512, 2600, 53), "global": (10000, 2600, 53)}     # (length, bin_lo, n_bins), test_gpu_stats.py


@functools.lru_cache(maxsize=None)
def hist_points():
    from test_gpu_stats import inputs
    x, y, t = inputs(HIST_N)
    k = np.random.default_rng(3).permutation(len(x))[:HIST_N]     # keeps some of the edge points
    return x[k], y[k], t[k]


def run_hist(gpu, oracle, shape, offsets=None):
    off = offsets or {}
    length, lo, nb = HIST_SHAPES[shape]
    x, y, t = hist_points()
    ins = [Guarded.of(x, off.get("x", 0)), Guarded.of(y, off.get("y", 0)), Guarded.of(t, off.get("t_ms", 0))]
    p0, c0, t0 = np.zeros(nb, U8), np.zeros((nb, length), I64), np.array([5, 9], I64)
    c0[::3, ::5] = 2                                            # accumulated into, never cleared
    outs = [Guarded.of(p0, off.get("present", 0)), Guarded.of(c0, off.get("counts", 0)),
            Guarded.of(t0, off.get("tally", 0))]
    rc = gpu.lib.gm_z3_histogram(gpu.handle, ins[0].ptr, ins[1].ptr, ins[2].ptr, HIST_N, WEEK, length, 0, lo, nb,
                                 outs[0].ptr, outs[1].ptr, outs[2].ptr)
    sync(gpu)
    assert rc == OK
    check_all(ins + outs, "histogram " + shape)
    op, oc, ot = oracle.z3_histogram(x, y, t, length, lo, nb, period=WEEK, present=p0.copy(), counts=c0.copy(),
                                     tally=t0.copy())
    assert np.array_equal(outs[2].read(I64), ot) and np.array_equal(outs[0].read(U8), op)
    assert np.array_equal(outs[1].read(I64).reshape(nb, length), oc)


@pytest.mark.parametrize("shape", list(HIST_SHAPES))
def test_histogram_bounds(gpu, oracle, shape):
    """gm_z3_histogram at n = 10,001 on the LDS-counter and the global-atomic path: present, counts and tally
    accumulate the oracle's values and nothing is written around them."""
    run_hist(gpu, oracle, shape)


# ---------------------------------------------------------------- 3. alignment matrix
def _index_alignment(name, ins, outs):
    """(case, names) of an index entry point: names maps ("in" | "out", k) to the pointer's name."""
    names = {("in", k): v for k, v in enumerate(ins)}
    names.update({("out", k): v for k, v in enumerate(outs)})
    return INDEX_CASES[name](), names


def run_index_aligned(gpu, oracle, name, ins, outs, offsets):
    case, names = _index_alignment(name, ins, outs)
    n = 2 * case.block + 5
    rng = np.random.default_rng(n)
    cols = case.cols(rng, n)
    case.spoil(cols, [1, case.block + 7, n - 1])
    exp, est = case.expect(oracle, cols)
    rc, got, st, sm = run_index(gpu, case, cols, n, True, True, offsets, names)
    assert rc == OK and sm == (3, 1, int(est[1])) and np.array_equal(st, est), (name, offsets)
    for g, w in zip(got, exp):
        assert np.array_equal(g, w), (name, offsets)


ALIGN = {
    # entry point: (pointer names with their element sizes, runner(gpu, oracle, offsets))
    "gm_z3_index_key": ([("x", 8), ("y", 8), ("t_ms", 8), ("bin", 2), ("z", 8), ("status", 1)],
                        lambda g, o, off: run_index_aligned(g, o, "gm_z3_index_key", ["x", "y", "t_ms"], ["bin", "z"], off)),
    "gm_z2_index": ([("x", 8), ("y", 8), ("z", 8), ("status", 1)],
                    lambda g, o, off: run_index_aligned(g, o, "gm_z2_index", ["x", "y"], ["z"], off)),
    "gm_xz2_index": ([("xmin", 8), ("ymin", 8), ("xmax", 8), ("ymax", 8), ("out", 8), ("status", 1)],
                     lambda g, o, off: run_index_aligned(g, o, "gm_xz2_index", ["xmin", "ymin", "xmax", "ymax"], ["out"],
                                                         off)),
    "gm_xz3_index": ([("xmin", 8), ("ymin", 8), ("zmin", 8), ("xmax", 8), ("ymax", 8), ("zmax", 8), ("out", 8),
                      ("status", 1)],
                     lambda g, o, off: run_index_aligned(g, o, "gm_xz3_index",
                                                         ["xmin", "ymin", "zmin", "xmax", "ymax", "zmax"], ["out"], off)),
    "gm_z3_invert": ([("z", 8), ("x", 8), ("y", 8), ("t", 8)],
                     lambda g, o, off: run_invert(g, o, "gm_z3_invert", 2 * 1024 + 5, off)),
    "gm_z2_invert": ([("z", 8), ("x", 8), ("y", 8)], lambda g, o, off: run_invert(g, o, "gm_z2_invert", 2 * 512 + 5, off)),
    "gm_z3filter_scan": ([("bin", 2), ("z", 8), ("mask", 8), ("ids", 8)], None),
    "gm_z2filter_scan": ([("z", 8), ("mask", 8), ("ids", 8)], None),
    "gm_strict_scan": ([("x", 8), ("y", 8), ("t_ms", 8), ("mask", 8), ("ids", 8)], None),
    "gm_query_scan+geom": ([("x", 8), ("y", 8), ("t_ms", 8), ("mask", 8), ("ids", 8)], None),
    "gm_z3_histogram": ([("x", 8), ("y", 8), ("t_ms", 8), ("present", 1), ("counts", 8), ("tally", 8)],
                        lambda g, o, off: run_hist(g, o, "lds", off)),
    "gm_pip_join_pred": ([("px", 8), ("py", 8), ("pt_ids", 8), ("poly_ids", 4)], None),
    "gm_pip_relate": ([("poly", 4), ("px", 8), ("py", 8), ("loc", 1)], lambda g, o, off: run_relate(g, 2 * 2048 + 5, off)),
}


def _align_cases():
    out = []
    for name, (ptrs, _) in ALIGN.items():
        out.append((name, "all", 0))
        out += [(name, p, size) for p, size in ptrs]
        if name == "gm_z3_index_key":
            out.append((name, "bin", 4))      # two elements in: 4-B aligned, not 16-B
    return out


@pytest.mark.parametrize("name,moved,by", _align_cases(), ids=lambda v: str(v))
def test_alignment(gpu, oracle, name, moved, by):
    """Every pointer of an entry point's dispatch condition moved by one element of its own type in turn
    (outputs too; bin also by two elements), against the all-aligned run: the oracle's result bit for bit and
    untouched guards whichever kernel the dispatch picks (the module docstring lists the kernel per case)."""
    off = {moved: by} if by else {}
    runner = ALIGN[name][1]
    if runner is not None:
        runner(gpu, oracle, off)
    elif name == "gm_pip_join_pred":
        exp = oracle_pairs(oracle, "st_contains")
        p = len(exp)
        rc, k, pt, pl = run_join(gpu, "pred", "st_contains", p, join_inputs("pred", off), offsets=off)
        assert (rc, k) == (OK, p) and sorted(zip(pt.tolist(), pl.tolist())) == exp
    else:
        s = Scan(gpu, oracle, name, off)
        assert s.run(gpu, s.m, offsets=off) == (OK, s.m)


# ---------------------------------------------------------------- 4. gm_device_copy
@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, 4096, 256 * 8 * 16 + 24, (1 << 20) + 5])
def test_device_copy(gpu, nbytes):
    """The 16-B vector kernel (both pointers 16-B aligned) plus its hipMemcpyAsync tail, and the plain copy of
    every other alignment: the destination equals the source byte for byte and its guards are untouched."""
    src_bytes = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=U8)
    src_bytes[src_bytes == FILL] = 0
    for so in (0, 8, 1):
        for do in (0, 8, 1):
            src, dst = Guarded.of(src_bytes, so), Guarded(nbytes, do)
            assert gpu.lib.gm_device_copy(gpu.handle, dst.ptr, src.ptr, nbytes) == OK
            sync(gpu)
            check_all([src, dst], "copy %d B, src +%d, dst +%d" % (nbytes, so, do))
            assert np.array_equal(dst.read(), src_bytes), (nbytes, so, do)
    assert gpu.lib.gm_device_copy(gpu.handle, None, None, 0) == OK


# ---------------------------------------------------------------- 4b. gm_gen_points
def test_gen_points_optional_columns(gpu):
    """gm_gen_points writes exactly n values into each column it is given (2 x 256 + 5 rows: k_gen_points has
    256-thread blocks), inside the requested intervals, and a column left NULL changes nothing in the others."""
    n = 2 * 256 + 5
    box = (-125.0, -66.0, 24.0, 50.0)      # lon0, lon1, lat0, lat1

    def gen(wx, wy, wt):
        bufs = [Guarded(8 * n) if w else None for w in (wx, wy, wt)]
        rc = gpu.lib.gm_gen_points(gpu.handle, 77, n, 1000, box[0], box[1], box[2], box[3], T2020, T2021, P(bufs[0]),
                                   P(bufs[1]), P(bufs[2]))
        sync(gpu)
        assert rc == OK
        check_all(bufs)
        return [b.read(I64) if b is not None else None for b in bufs]
    x, y, t = gen(True, True, True)
    xf, yf = x.view(F64), y.view(F64)
    assert np.all((xf >= box[0]) & (xf < box[1])) and np.all((yf >= box[2]) & (yf < box[3]))
    assert np.all((t >= T2020) & (t < T2021)) and len(np.unique(x)) > n // 2
    for w in [(True, True, False), (True, False, False), (False, True, True), (False, False, True)]:
        got = gen(*w)
        for g, full in zip(got, (x, y, t)):
            assert g is None or np.array_equal(g, full), w


# ---------------------------------------------------------------- 5. parameters and arguments (host side)
PARAMS = {   # id: (default, valid values, invalid values)
    _lib.GM_PARAM_JOIN_CHUNK: (0, [4096, 1, 1 << 40, 0], [-1]),
    _lib.GM_PARAM_INDEX_BUILD: (0, [1, 0], [2, -1]),
    _lib.GM_PARAM_RANGES_CHUNK: (0, [5, 1 << 30, 0], [-1]),
    _lib.GM_PARAM_SORT_MODE: (0, [1, 0], [2, -1]),
    _lib.GM_PARAM_INDEX_COARSE: (-1, [0, 1, -1], [-2, 2]),
    _lib.GM_PARAM_HIST_GRID: (0, [1, 1 << 20, 0], [-1, (1 << 20) + 1]),
    _lib.GM_PARAM_RELATE_ROWS64: (0, [1, 0], [2, -1]),
}


def test_params(gpu):
    """Every GM_PARAM_*: the documented default (on a fresh context), set / get, the invalid values (which
    leave the value alone), the read-only and the retired parameter, and unknown ids."""
    ctx = _lib.Context(gpu.device)
    try:
        lib, h = ctx.lib, ctx.handle
        v = ctypes.c_int64(-7)

        def get(p):
            assert lib.gm_ctx_get_param(h, p, ctypes.byref(v)) == OK, p
            return v.value
        for p, (default, valid, invalid) in PARAMS.items():
            assert get(p) == default, p
            for val in valid:
                assert lib.gm_ctx_set_param(h, p, val) == OK and get(p) == val, (p, val)
            for val in invalid:
                assert lib.gm_ctx_set_param(h, p, val) == E_INVALID and get(p) == valid[-1], (p, val)
        assert get(_lib.GM_PARAM_SORT_LAST) == 0
        assert lib.gm_ctx_set_param(h, _lib.GM_PARAM_SORT_LAST, 1) == E_INVALID       # read-only
        assert lib.gm_ctx_set_param(h, _lib.GM_PARAM_INDEX_CORE_RETIRED, 5) == OK     # accepted no-op
        assert get(_lib.GM_PARAM_INDEX_CORE_RETIRED) == 0
        for p in (0, 10, -1, 99):
            assert lib.gm_ctx_set_param(h, p, 0) == E_INVALID
            assert lib.gm_ctx_get_param(h, p, ctypes.byref(v)) == E_INVALID
        assert lib.gm_ctx_get_param(h, _lib.GM_PARAM_JOIN_CHUNK, None) == E_INVALID
        assert lib.gm_ctx_set_param(None, _lib.GM_PARAM_JOIN_CHUNK, 0) == E_INVALID
    finally:
        ctx.close()


def test_domain_limits(gpu):
    """Each documented domain limit is GM_E_INVALID; every call has n == 0 or fails its check before any
    launch, so no kernel runs."""
    lib, h = gpu.lib, gpu.handle
    N = None
    for period in (-1, 4):
        assert lib.gm_z3_index(h, N, N, N, 0, period, 21, 0, N, N, N) == E_INVALID
        assert lib.gm_z3_index_key(h, N, N, N, 0, period, 0, N, N, N, N) == E_INVALID
        assert lib.gm_z3_invert(h, N, 0, period, 21, N, N, N) == E_INVALID
        assert lib.gm_binned_time(h, N, 0, period, N, N, N, N) == E_INVALID
        assert lib.gm_xz3_index(h, N, N, N, N, N, N, 0, 12, period, 0, N, N, N) == E_INVALID
        assert lib.gm_xz3_index_key(h, N, N, N, N, N, 0, 12, period, 0, N, N, N, N) == E_INVALID
        assert lib.gm_z3_histogram(h, N, N, N, 0, period, 16, 0, 0, 1, N, N, N) == E_INVALID
        assert lib.gm_legacy_z3_index(h, N, N, N, 0, 0, period, 0, N, N, N) == E_INVALID
    for prec in (0, 22):
        assert lib.gm_z3_index(h, N, N, N, 0, WEEK, prec, 0, N, N, N) == E_INVALID
        assert lib.gm_z3_invert(h, N, 0, WEEK, prec, N, N, N) == E_INVALID
    for prec in (0, 32):
        assert lib.gm_z2_index(h, N, N, 0, prec, 0, N, N, N) == E_INVALID
        assert lib.gm_z2_invert(h, N, 0, prec, N, N) == E_INVALID
    for g in (0, 31):
        assert lib.gm_xz2_index(h, N, N, N, N, 0, g, 0, N, N, N) == E_INVALID
    for g in (0, 21):
        assert lib.gm_xz3_index(h, N, N, N, N, N, N, 0, g, WEEK, 0, N, N, N) == E_INVALID
        assert lib.gm_xz3_index_key(h, N, N, N, N, N, 0, g, WEEK, 0, N, N, N, N) == E_INVALID
    off = np.zeros(1, I32)
    oo = np.zeros(1, I64)
    for g in (0, 30):
        assert lib.gm_xz2_ranges(h, 0, off.ctypes.data, N, g, 0, oo.ctypes.data, N, 0, N, N) == E_INVALID
    for g in (0, 20):
        assert lib.gm_xz3_ranges(h, 0, off.ctypes.data, N, g, WEEK, 0, oo.ctypes.data, N, 0, N, N) == E_INVALID
    for period in (-1, 4):
        assert lib.gm_z3_ranges(h, 0, off.ctypes.data, N, off.ctypes.data, N, period, 21, 64, 0, -1, oo.ctypes.data, N, 0,
                                N, N) == E_INVALID
        assert lib.gm_xz3_ranges(h, 0, off.ctypes.data, N, 12, period, 0, oo.ctypes.data, N, 0, N, N) == E_INVALID
    for prec in (0, 22):
        assert lib.gm_z3_ranges(h, 0, off.ctypes.data, N, off.ctypes.data, N, WEEK, prec, 64, 0, -1, oo.ctypes.data, N, 0,
                                N, N) == E_INVALID
    for prec in (0, 32):
        assert lib.gm_z2_ranges(h, 0, off.ctypes.data, N, prec, 64, 0, -1, oo.ctypes.data, N, 0, N, N) == E_INVALID
    for dims in (1, 4):
        assert lib.gm_zranges(h, dims, 0, off.ctypes.data, N, 64, 0, -1, oo.ctypes.data, N, 0, N, N) == E_INVALID
    # n < 0
    fb3, fb2 = _filters()
    a3, a2 = np.frombuffer(fb3, U8).copy(), np.frombuffer(fb2, U8).copy()
    assert lib.gm_z3_index(h, N, N, N, -1, WEEK, 21, 0, N, N, N) == E_INVALID
    assert lib.gm_z3_index_key(h, N, N, N, -1, WEEK, 0, N, N, N, N) == E_INVALID
    assert lib.gm_z2_index(h, N, N, -1, 31, 0, N, N, N) == E_INVALID
    assert lib.gm_z3_invert(h, N, -1, WEEK, 21, N, N, N) == E_INVALID
    assert lib.gm_binned_time(h, N, -1, WEEK, N, N, N, N) == E_INVALID
    assert lib.gm_xz2_index(h, N, N, N, N, -1, 12, 0, N, N, N) == E_INVALID
    assert lib.gm_z3filter_scan(h, a3.ctypes.data, len(a3), N, 0, N, N, -1, N, N, 0, N) == E_INVALID
    assert lib.gm_z2filter_scan(h, a2.ctypes.data, len(a2), N, -1, N, N, 0, N) == E_INVALID
    assert lib.gm_strict_scan(h, N, N, N, -1, BBOX.ctypes.data, 0, 0, 0, N, N, 0, N) == E_INVALID
    assert lib.gm_query_scan(h, N, N, N, -1, N, 0, 0, 0, N, 0, N, N, 0, N) == E_INVALID
    assert lib.gm_z3_key_bytes(h, N, N, N, -1, N) == E_INVALID
    assert lib.gm_sort_keys(h, N, N, N, -1, N, N, N, N) == E_INVALID
    assert lib.gm_z3_histogram(h, N, N, N, -1, WEEK, 16, 0, 0, 1, N, N, N) == E_INVALID
    assert lib.gm_gen_points(h, 1, -1, 0, 0.0, 1.0, 0.0, 1.0, 0, 1, N, N, N) == E_INVALID
    assert lib.gm_z3_ranges(h, -1, off.ctypes.data, N, off.ctypes.data, N, WEEK, 21, 64, 0, -1, oo.ctypes.data, N, 0, N,
                            N) == E_INVALID
    # samples, splitters
    assert lib.gm_key_sample(h, N, N, N, 10, 65537, N, N) == E_INVALID
    big = np.zeros(256, U64)
    assert lib.gm_key_partition(h, N, N, N, 0, big.ctypes.data, big.ctypes.data, 256, N, 0, N, N, N, N, N,
                                np.zeros(257, I64).ctypes.data) == E_INVALID
    # the join's arguments and the query's geometry term
    ix = join_data()[1]
    one = Guarded(64)
    cnt = ctypes.c_int64(-7)
    assert lib.gm_pip_join_pred(h, ix._h, N, N, 0, 0, one.ptr, N, 8, ctypes.byref(cnt), 0, 2) == E_INVALID
    assert lib.gm_pip_join_pred(h, ix._h, N, N, 0, 0, N, one.ptr, 8, ctypes.byref(cnt), 0, 2) == E_INVALID
    for pred in (0, 3, -1):
        assert lib.gm_pip_join_pred(h, ix._h, N, N, 0, 0, N, N, 0, ctypes.byref(cnt), 0, pred) == E_INVALID
    assert lib.gm_pip_join_pred(h, ix._h, N, N, 0, 0, N, N, -1, ctypes.byref(cnt), 0, 2) == E_INVALID
    for op in (1, 2):
        assert lib.gm_query_scan(h, N, N, N, 0, N, 0, 0, 0, N, op, N, N, 0, N) == E_INVALID     # no geoms
    for op in (-1, 3):
        assert lib.gm_query_scan(h, N, N, N, 0, N, 0, 0, 0, ix._h, op, N, N, 0, N) == E_INVALID
    assert cnt.value == -7 and untouched(one.read())


def test_malformed_filter_bytes(gpu):
    """Filter bytes truncated anywhere -- so at every field boundary -- are GM_E_INVALID in all four filter
    scans (the parse comes before the n == 0 return); the whole filter is GM_OK."""
    from geomesa_amd import filters as F
    lib, h = gpu.lib, gpu.handle
    N = None
    f3 = F.Z3Filter([[0, 0, 100, 100], [5, 5, 6, 6]], [[[0, 1000], [2000, 3000]], None, [], [[7, 9]]], 3, 6)
    a3 = np.frombuffer(F.serialize_to_bytes(f3), U8).copy()
    a2 = np.frombuffer(F.z2_serialize_to_bytes(F.Z2Filter([[0, 0, 100, 100], [5, 5, 6, 6]])), U8).copy()
    nm = ctypes.c_int64(-7)
    for k in range(len(a3) + 1):
        want = OK if k == len(a3) else E_INVALID
        assert lib.gm_z3filter_scan(h, a3.ctypes.data, k, N, 0, N, N, 0, N, N, 0, ctypes.byref(nm)) == want, k
        assert lib.gm_z3filter_scan_rows(h, a3.ctypes.data, k, N, N, 0, 0, N, N, 0, ctypes.byref(nm), N) == want, k
    for k in range(len(a2) + 1):
        want = OK if k == len(a2) else E_INVALID
        assert lib.gm_z2filter_scan(h, a2.ctypes.data, k, N, 0, N, N, 0, ctypes.byref(nm)) == want, k
        assert lib.gm_z2filter_scan_rows(h, a2.ctypes.data, k, N, N, 0, 0, N, N, 0, ctypes.byref(nm), N) == want, k
    assert lib.gm_z3filter_scan(h, N, 8, N, 0, N, N, 0, N, N, 0, N) == E_INVALID


def _null_calls(gpu):
    """(name, call(args) -> rc, good pointer list): every listed pointer is rejected by a host check of the
    entry point, before any launch, when n > 0 (the `if (!x || ...) return GM_E_INVALID` line after the
    n == 0 return of each; read in geomesa_amd/csrc at this commit)."""
    lib, h = gpu.lib, gpu.handle
    ix = join_data()[1]
    fb3, fb2 = _filters()
    a3, a2 = np.frombuffer(fb3, U8).copy(), np.frombuffer(fb2, U8).copy()
    keep = [a3, a2]
    S = _lib.BatchStatus
    return keep, [
        ("gm_z3_index", lambda a: lib.gm_z3_index(h, a[0], a[1], a[2], 4, WEEK, 21, 0, a[3], None, None), 4),
        ("gm_z3_index_key", lambda a: lib.gm_z3_index_key(h, a[0], a[1], a[2], 4, WEEK, 0, a[3], a[4], None, None), 5),
        ("gm_z3_invert", lambda a: lib.gm_z3_invert(h, a[0], 4, WEEK, 21, a[1], a[2], a[3]), 4),
        ("gm_z2_index", lambda a: lib.gm_z2_index(h, a[0], a[1], 4, 31, 0, a[2], None, None), 3),
        ("gm_z2_invert", lambda a: lib.gm_z2_invert(h, a[0], 4, 31, a[1], a[2]), 3),
        ("gm_binned_time", lambda a: lib.gm_binned_time(h, a[0], 4, WEEK, a[1], a[2], None, None), 3),
        ("gm_xz2_index", lambda a: lib.gm_xz2_index(h, a[0], a[1], a[2], a[3], 4, 12, 0, a[4], None, None), 5),
        ("gm_xz3_index", lambda a: lib.gm_xz3_index(h, a[0], a[1], a[2], a[3], a[4], a[5], 4, 12, WEEK, 0, a[6], None,
                                                   None), 7),
        ("gm_xz3_index_key", lambda a: lib.gm_xz3_index_key(h, a[0], a[1], a[2], a[3], None, 4, 12, WEEK, 0, a[4], a[5],
                                                           None, None), 6),
        ("gm_legacy_z3_index", lambda a: lib.gm_legacy_z3_index(h, a[0], a[1], a[2], 4, 0, WEEK, 0, a[3], None, None), 4),
        ("gm_legacy_z3_invert", lambda a: lib.gm_legacy_z3_invert(h, a[0], 4, 0, WEEK, a[1], a[2], a[3]), 4),
        ("gm_legacy_z2_index", lambda a: lib.gm_legacy_z2_index(h, a[0], a[1], 4, 0, a[2], None, None), 3),
        ("gm_legacy_z2_invert", lambda a: lib.gm_legacy_z2_invert(h, a[0], 4, a[1], a[2]), 3),
        ("gm_z3filter_scan", lambda a: lib.gm_z3filter_scan(h, a3.ctypes.data, len(a3), None, 0, a[0], a[1], 4, None, None,
                                                           0, None), 2),
        ("gm_z2filter_scan", lambda a: lib.gm_z2filter_scan(h, a2.ctypes.data, len(a2), a[0], 4, None, None, 0, None), 1),
        ("gm_z3filter_scan_rows", lambda a: lib.gm_z3filter_scan_rows(h, a3.ctypes.data, len(a3), a[0], a[1], 0, 4, None,
                                                                     None, 0, None, None), 2),
        ("gm_z2filter_scan_rows", lambda a: lib.gm_z2filter_scan_rows(h, a2.ctypes.data, len(a2), a[0], a[1], 0, 4, None,
                                                                     None, 0, None, None), 2),
        ("gm_strict_scan", lambda a: lib.gm_strict_scan(h, a[0], a[1], a[2], 4, BBOX.ctypes.data, 1, 0, 9, None, None, 0,
                                                       None), 3),
        ("gm_query_scan", lambda a: lib.gm_query_scan(h, a[0], a[1], a[2], 4, None, 1, 0, 9, None, 0, None, None, 0,
                                                     None), 3),
        ("gm_pip_join_pred", lambda a: lib.gm_pip_join_pred(h, ix._h, a[0], a[1], 4, 0, None, None, 0, None, 0, 2), 2),
        ("gm_pip_relate", lambda a: lib.gm_pip_relate(h, ix._h, a[0], a[1], a[2], 4, a[3]), 4),
        ("gm_z3_histogram", lambda a: lib.gm_z3_histogram(h, a[0], a[1], a[2], 4, WEEK, 16, 0, 0, 1, a[3], a[4], a[5]), 6),
        ("gm_z3_key_bytes", lambda a: lib.gm_z3_key_bytes(h, None, a[0], a[1], 4, a[2]), 3),
        ("gm_z2_key_bytes", lambda a: lib.gm_z2_key_bytes(h, None, a[0], 4, a[1]), 2),
        ("gm_sort_keys", lambda a: lib.gm_sort_keys(h, None, None, a[0], 4, None, None, a[1], a[2]), 3),
        ("gm_arrow_points_to_columns", lambda a: lib.gm_arrow_points_to_columns(
            h, ctypes.byref(point_struct(None)) if a[0] is None else ctypes.byref(_as_point(a[0])), 4, a[1], a[2]), 3),
        ("gm_device_copy", lambda a: lib.gm_device_copy(h, a[0], a[1], 64), 2),
    ]


def _as_point(p):
    g = point_struct(None)
    g.coords = p.value
    return g


def test_null_pointers(gpu):
    """Each required pointer NULL in turn, the others valid: GM_E_INVALID from the host check, and the valid
    buffers stay untouched (nothing ran)."""
    keep, calls = _null_calls(gpu)
    buf = Guarded(4096)
    for name, call, k in calls:
        good = [ctypes.c_void_p(buf.addr + 256 * j) for j in range(k)]
        for j in range(k):
            args = list(good)
            args[j] = None
            assert call(args) == E_INVALID, (name, j)
    assert gpu.lib.gm_ctx_sync(None) == E_INVALID
    sync(gpu)
    buf.check("null table")
    assert untouched(buf.read())
    # gm_gen_points: each column is optional, none at all is an error
    assert gpu.lib.gm_gen_points(gpu.handle, 1, 4, 0, -1.0, 1.0, -1.0, 1.0, 0, 9, None, None, None) == E_INVALID
    # gm_key_partition: dest_counts is required whatever n is
    assert gpu.lib.gm_key_partition(gpu.handle, None, None, None, 0, None, None, 0, None, 0, None, None, None, None, None,
                                    None) == E_INVALID
