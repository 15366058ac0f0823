"""gm_table_scan against its definition, piece by piece.

The expected result of every scan is composed from pinned parts: the candidates are
oracle.table_scan_rows on the sorted key columns (pinned to the store's byte order by
test_table_scan_reference.py), the row filter is oracle.z3filter_scan / z2filter_scan on the sorted
columns, the full filter is oracle.envelope_scan on the input-order columns, and the table order is
gm_sort_keys' (test_sort_keys_parity).  keep = cand & rowfilter & full[perm]; the ids are
perm[nonzero(keep)] IN THAT ORDER (the scan promises table order), n_match = keep.sum() and n_scanned =
cand.sum() (ranges are merged, so a row is a candidate once).  Everything is bit-exact.

The 12 instantiations of k_range_mask<RF, ENV, DUR> and where each one runs:
  RF_NONE            test_range_shapes, test_range_counts, test_key_ranges_forms, test_every_instantiation[RF_NONE]
  RF_NONE+ENV        test_candidate_totals, test_row_map[xz2-*], test_envelope_edges, test_two_scan_chunks,
                     test_every_instantiation[RF_NONE+ENV]
  RF_NONE+DUR        test_every_instantiation[RF_NONE+DUR]
  RF_NONE+ENV+DUR    test_row_map[xz3-*], test_every_instantiation[RF_NONE+ENV+DUR]
  RF_Z3              test_every_instantiation[RF_Z3]
  RF_Z3+ENV          test_every_instantiation[RF_Z3+ENV]
  RF_Z3+DUR          test_every_instantiation[RF_Z3+DUR]
  RF_Z3+ENV+DUR      test_every_instantiation[RF_Z3+ENV+DUR], test_capacity
  RF_Z2              test_every_instantiation[RF_Z2]
  RF_Z2+ENV          test_every_instantiation[RF_Z2+ENV]
  RF_Z2+DUR          test_every_instantiation[RF_Z2+DUR]
  RF_Z2+ENV+DUR      test_every_instantiation[RF_Z2+ENV+DUR]
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import table_scan_cases as C
from test_gpu_scan_join_ranges import ADVERSARIAL_Z3, adversarial_z2
from test_gpu_xztable import random_envelopes
from geomesa_amd import filters as F

pytestmark = pytest.mark.gpu

T0 = 1577836800000


def as_np(t):
    return t.detach().cpu().numpy()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class HostTable:
    """A _KeyTable (gm_sort_keys order on the device) with its sorted columns and perm read back."""

    def __init__(self, shard, bins, z):
        from geomesa_amd.table import _KeyTable
        self.tb = _KeyTable(bins, z, shard, C.SHARDS if shard is not None else None)
        self.n = len(z)
        self.perm = as_np(self.tb.perm)
        assert np.array_equal(self.perm, C.table_order(shard, bins, z))   # pinned by test_sort_keys_parity
        self.shard = None if shard is None else as_np(self.tb.shard)
        self.bins = None if bins is None else as_np(self.tb.bin)
        self.z = as_np(self.tb.z)
        self.keys = C.keys80(self.shard, self.bins, self.z)

    def cand(self, oracle, arr):
        return oracle.table_scan_rows(self.shard, self.bins, self.z, arr)


@functools.lru_cache(maxsize=None)
def alphabet(n, sharded, binned):
    rng = np.random.default_rng(7 * n + 2 * sharded + binned)
    return HostTable(*C.alphabet_table(rng, n, sharded, binned))


def raw_scan(tb, arr, flt=None, perm=None, cap=None, want_ids=True, guard=8):
    """gm_table_scan itself: (rc, ids buffer of cap + guard slots preset to -7, n_match, n_scanned)."""
    import torch
    from geomesa_amd import _lib
    arr = np.ascontiguousarray(arr, _lib.KEY_RANGE_DTYPE)
    cap = tb.n if cap is None else cap
    ids = torch.full((cap + guard,), -7, dtype=torch.int64, device="cuda") if want_ids else None
    nm, ns = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = tb.ctx.lib.gm_table_scan(tb.ctx.handle, _lib.ptr(tb.shard), _lib.ptr(tb.bin), _lib.ptr(tb.z), tb.n,
                                  arr.ctypes.data if len(arr) else None, len(arr),
                                  ctypes.byref(flt) if flt is not None else None, _lib.ptr(perm), _lib.ptr(ids), cap,
                                  ctypes.byref(nm), ctypes.byref(ns))
    return rc, (as_np(ids) if want_ids else None), nm.value, ns.value


def check_scan(ht, arr, keep, cand, flt=None, what=""):
    """One scan mapped through perm: ids in table order, both counts, nothing written past the matches."""
    rc, ids, nm, ns = raw_scan(ht.tb, arr, flt, ht.tb.perm)
    exp = ht.perm[np.nonzero(keep)[0]]
    assert rc == 0, (what, rc)
    assert ns == int(cand.sum()), (what, ns, int(cand.sum()))
    assert nm == len(exp), (what, nm, len(exp))
    assert np.array_equal(ids[:nm], exp), what
    assert np.all(ids[nm:] == -7), what


# ---------------------------------------------------------------- ranges (k_range_mask<RF_NONE, false, false>)

@pytest.mark.parametrize("sharded,binned", C.TABLE_KINDS)
@pytest.mark.parametrize("n", C.TABLE_SIZES)
def test_range_shapes(gpu, oracle, n, sharded, binned):
    """Every range shape on its own, all of them together, and 40 random ranges with ends on the table's
    keys and their +-1 neighbours."""
    ht = alphabet(n, sharded, binned)
    rng = np.random.default_rng(n)
    groups = C.shape_groups(ht.keys, sharded)
    groups["all_shapes"] = [r for g in groups.values() for r in g if r[1:] != (0, C.K80)]
    groups["random"] = C.random_ranges(rng, ht.keys, 40)
    groups["random_narrow"] = C.random_ranges(rng, ht.keys, 40, narrow=True)
    for name, rs in groups.items():
        arr = C.ranges_array(rs)
        cand = ht.cand(oracle, arr)
        check_scan(ht, arr, cand, cand, what=name)


def disjoint_ranges(rng, keys, count):
    """`count` ranges no two of which overlap or touch, so that merging leaves exactly `count` of them:
    single-key ranges on table keys at least two key steps apart, the rest in a shard the table lacks."""
    out, last = [], None
    for s, k in sorted(set(keys)):
        if len(out) >= min(count, max(1, (count * 3) // 5)):
            break
        if last is None or (s, k) > (last[0], last[1] + 1) and not (s == last[0] + 1 and k == 0):
            out.append((s, k, k))
            last = (s, k)
    out += [(C.ABSENT_SHARD, 10 * i, 10 * i + int(rng.integers(0, 4))) for i in range(count - len(out))]
    return [out[i] for i in rng.permutation(len(out))]


@pytest.mark.parametrize("kind", ["disjoint", "random", "random_narrow"])
@pytest.mark.parametrize("count", [0, 1, 2, 1023, 1024, 1025, 5000])
def test_range_counts(gpu, oracle, count, kind):
    """Range counts around the 1024 threads of the range-offset scan.  disjoint: the merged count is the
    given count (1023 / 1024: one range per thread; 1025: two; 5000: five); random: heavy merging."""
    ht = alphabet(20_011, True, True)
    rng = np.random.default_rng(count)
    if kind == "disjoint":
        rs = disjoint_ranges(rng, ht.keys, count)
    else:
        rs = C.random_ranges(rng, ht.keys, count, narrow=kind == "random_narrow")
    assert len(rs) == count
    arr = C.ranges_array(rs)
    cand = ht.cand(oracle, arr)
    if kind == "disjoint" and count:
        assert cand.any() and not cand.all()
    check_scan(ht, arr, cand, cand, what=kind)


@pytest.mark.parametrize("sharded,binned", C.TABLE_KINDS)
def test_key_ranges_forms(gpu, oracle, sharded, binned):
    """The bounded / lower / upper / unbounded forms as table.key_ranges writes them, one scan each, on
    tables with and without a bin column (where a row's bin reads as 0 and bin_hi = -1 holds it)."""
    from geomesa_amd.table import key_ranges
    ht = alphabet(4097, sharded, binned)
    mid = ht.n // 2
    b = int(ht.bins[mid]) if binned else 0
    zq = np.sort(ht.z[(ht.bins == b) if binned else np.ones(ht.n, bool)].view(np.uint64)).view(np.int64)
    z1, z2 = int(zq[len(zq) // 4]), int(zq[3 * len(zq) // 4])
    forms = [("bounded", (b, z1), (b, z2)), ("lower", (b, z1), None), ("upper", None, (b, z2)),
             ("unbounded", (0, 0), None)]
    for form in forms + [forms]:
        arr, k = key_ranges(form if isinstance(form, list) else [form], C.SHARDS if sharded else None)
        assert k == len(arr) == (len(form) if isinstance(form, list) else 1) * (C.SHARDS if sharded else 1)
        cand = ht.cand(oracle, arr)
        assert cand.any()
        check_scan(ht, arr, cand, cand, what=str(form))
    arr, _ = key_ranges([("unbounded", (0, 0), None)], C.SHARDS if sharded else None)
    assert ht.cand(oracle, arr).all()


# ---------------------------------------------------------------- candidate totals

@functools.lru_cache(maxsize=None)
def arange_table():
    n = 8200
    z = np.random.default_rng(3).permutation(n).astype(np.int64) + 10    # the keys 10 .. n + 9, shuffled
    return HostTable(None, None, z), z


def full_filter(cols, boxes, t=None, interval=None, rows=None):
    """A ScanFilter over device columns (kept alive by the caller); boxes: host (k, 4) float64."""
    from geomesa_amd import _lib
    f = _lib.ScanFilter()
    if boxes is not None and len(boxes):
        f.xmin, f.ymin, f.xmax, f.ymax = (c.data_ptr() for c in cols)
        f.boxes, f.n_boxes = boxes.ctypes.data, len(boxes)
    if interval is not None:
        f.during, f.t_ms, f.t_lo, f.t_hi = 1, t.data_ptr(), int(interval[0]), int(interval[1])
    if rows is not None:
        f.rows = rows.data_ptr()
    return f


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_candidate_totals(gpu, oracle, total):
    """One bounded range of exactly `total` candidates (mask-word, block and two-block boundaries) and an
    envelope filter keeping the first and the last candidate, every third one and a run across row 4096."""
    ht, z_in = arange_table()
    zc = z_in - 10                                                   # the candidate index of a matching row
    want = (zc == 0) | (zc == total - 1) | (zc % 3 == 1) | ((zc >= 4090) & (zc <= 4100))
    col = np.where(want, 0.5, 5.0)
    dcol = dev(col)
    boxes = np.array([[0.0, 0.0, 1.0, 1.0]])
    flt = full_filter((dcol,) * 4, boxes, rows=ht.tb.perm)
    full = oracle.envelope_scan(col, col, col, col, boxes)
    assert np.array_equal(full, want)
    for rs in ([(0, 10, 10 + total - 1)] if total else [(0, 10, 9), (0, 3, 9)]):
        arr = C.ranges_array([rs])
        cand = ht.cand(oracle, arr)
        assert int(cand.sum()) == total
        keep = cand & full[ht.perm]
        assert total == 0 or (keep[np.nonzero(cand)[0][[0, -1]]].all() and keep.sum() < max(total, 2))
        check_scan(ht, arr, keep, cand, flt, what=str(rs))


# ---------------------------------------------------------------- every instantiation

@functools.lru_cache(maxsize=None)
def filter_table():
    """20,011 rows with keys the adversarial filters split (bins -4 .. 9, arbitrary z words, a share with
    small coordinates), envelopes and dtg values in input order."""
    rng = np.random.default_rng(12)
    n = 20_011
    z = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    z[rng.random(n) < 0.3] &= 0x7FFFFFFF
    z[rng.random(n) < 0.2] &= 0x3FFF                     # small enough for the Z2 filters' boxes near 0
    bins = rng.integers(-4, 10, n).astype(np.int16)
    shard = rng.integers(0, C.SHARDS, n).astype(np.uint8)
    ht = HostTable(shard, bins, z)
    xmin, ymin = rng.uniform(0, 10, n), rng.uniform(0, 10, n)
    env = (xmin, ymin, xmin + rng.uniform(0, 1, n), ymin + rng.uniform(0, 1, n))
    t = T0 + rng.integers(0, 1000, n)
    t[:400] = np.array([T_LO, T_LO + 1, T_HI - 1, T_HI])[np.arange(400) % 4]   # the exclusive ends
    return ht, env, t


T_LO, T_HI = T0 + 100, T0 + 700
BOXES = np.array([[2.0, 2.0, 4.0, 7.5], [6.0, 0.5, 9.0, 3.0]])
COMBOS = [(rf, env, dur) for rf in ("RF_NONE", "RF_Z3", "RF_Z2") for env in (False, True) for dur in (False, True)]


def combo_id(c):
    return c[0] + ("+ENV" if c[1] else "") + ("+DUR" if c[2] else "")


def filter_case(oracle, rf, env, dur, k=0):
    """(ScanFilter, things it points to, row-filter mask over table rows, full-filter mask over input rows)."""
    ht, e, t = filter_table()
    hold = []
    if env or dur:
        cols = tuple(dev(c) for c in e) if env else None
        dt = dev(t) if dur else None
        flt = full_filter(cols, BOXES if env else None, dt, (T_LO, T_HI) if dur else None, rows=ht.tb.perm)
        hold += [cols, dt]
        full = oracle.envelope_scan(*e, BOXES if env else [(-math.inf, -math.inf, math.inf, math.inf)],
                                    t if dur else None, (T_LO, T_HI) if dur else None)
    else:
        from geomesa_amd import _lib
        flt, full = _lib.ScanFilter(), np.ones(ht.n, bool)
    rowf = np.ones(ht.n, bool)
    if rf == "RF_Z3":
        fb = F.serialize_to_bytes(ADVERSARIAL_Z3[k])
        rowf = oracle.z3filter_scan(fb, [], ht.bins, ht.z)
    elif rf == "RF_Z2":
        fb = F.z2_serialize_to_bytes(adversarial_z2(k))
        rowf = oracle.z2filter_scan(fb, ht.z)
    if rf != "RF_NONE":
        buf = ctypes.create_string_buffer(fb, len(fb))
        hold.append(buf)
        if rf == "RF_Z3":
            flt.z3filter, flt.z3filter_len = ctypes.addressof(buf), len(fb)
        else:
            flt.z2filter, flt.z2filter_len = ctypes.addressof(buf), len(fb)
    return flt, hold, rowf, full


def filter_ranges(ht):
    rng = np.random.default_rng(77)
    return C.ranges_array(C.random_ranges(rng, ht.keys, 6) + C.random_ranges(rng, ht.keys, 30, narrow=True))


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_every_instantiation(gpu, oracle, combo):
    """k_range_mask<RF, ENV, DUR> for all 12 (RF, ENV, DUR), through gm_table_scan with a ScanFilter; each
    row filter with the three adversarial filters.  DUR without ENV runs with n_boxes = 0 and no envelope
    columns; dtg values sit at t_lo, t_lo + 1, t_hi - 1 and t_hi (the interval is exclusive)."""
    rf, env, dur = combo
    ht, _, t = filter_table()
    arr = filter_ranges(ht)
    cand = ht.cand(oracle, arr)
    assert 1000 < cand.sum() < ht.n
    at_ends = {int(v): (cand & np.isin(t, [v])[ht.perm]).sum() for v in (T_LO, T_LO + 1, T_HI - 1, T_HI)}
    assert all(at_ends.values()), at_ends
    for k in range(len(ADVERSARIAL_Z3) if rf != "RF_NONE" else 1):
        flt, hold, rowf, full = filter_case(oracle, rf, env, dur, k)
        assert flt.n_boxes == (2 if env else 0) and bool(flt.during) == dur and bool(flt.xmin) == env
        keep = cand & rowf & full[ht.perm]
        if k == 0 and combo != ("RF_NONE", False, False):
            assert 0 < keep.sum() < cand.sum(), (keep.sum(), cand.sum())   # the filters do filter
        check_scan(ht, arr, keep, cand, flt, what="%s filter %d" % (combo_id(combo), k))
        del hold


def test_capacity(gpu, oracle):
    """GM_E_CAPACITY exactly when n_match > ids_cap; the ids that fit are the first in table order, nothing
    is written past ids_cap, and n_match stays exact -- also with ids = NULL, which only counts."""
    from geomesa_amd import _lib
    ht, _, _ = filter_table()
    arr = filter_ranges(ht)
    cand = ht.cand(oracle, arr)
    flt, hold, rowf, full = filter_case(oracle, "RF_Z3", True, True)
    keep = cand & rowf & full[ht.perm]
    exp = ht.perm[np.nonzero(keep)[0]]
    m = len(exp)
    assert m > 2
    for cap in (0, 1, m - 1, m, m + 1):
        rc, ids, nm, ns = raw_scan(ht.tb, arr, flt, ht.tb.perm, cap=cap)
        assert rc == (_lib.GM_E_CAPACITY if m > cap else _lib.GM_OK), (cap, rc)
        assert nm == m and ns == int(cand.sum()), cap
        assert np.array_equal(ids[:min(cap, m)], exp[:cap]) and np.all(ids[min(cap, m):] == -7), cap
    rc, _, nm, ns = raw_scan(ht.tb, arr, flt, ht.tb.perm, want_ids=False)
    assert (rc, nm, ns) == (_lib.GM_OK, m, int(cand.sum()))
    rc, _, nm, ns = raw_scan(ht.tb, arr, flt, ht.tb.perm, cap=0, want_ids=False)
    assert (rc, nm, ns) == (_lib.GM_OK, m, int(cand.sum()))
    del hold


# ---------------------------------------------------------------- the full filter's row map

@pytest.mark.parametrize("sharded", [False, True], ids=["unsharded", "sharded"])
@pytest.mark.parametrize("kind", ["xz2", "xz3"])
def test_row_map(gpu, oracle, kind, sharded):
    """map_rows only chooses what the ids are: with table rows asked for, the full filter must still read
    each candidate's own envelope and dtg.  map_rows=False returns rows r with perm[r] equal to the
    map_rows=True ids, in the same order, and both equal the definition; so do columns handed over in
    table order with no map at all, and input-order columns mapped by perm alone (rows = NULL)."""
    import torch
    from geomesa_amd.keyspace import during
    from geomesa_amd.table import XZ2Table, XZ3Table, _full_filter, key_ranges
    n = 20_011
    env = random_envelopes(n, 50 + sharded, span=(0.0, 20.0))
    sh = (np.arange(n) * 2654435761 % 4).astype(np.uint8) if sharded else None
    boxes = [(-60.0, -30.0, 70.0, 50.0), (100.0, -40.0, 120.0, -10.0)]
    if kind == "xz2":
        tb = XZ2Table(*env, shard=sh, shards=4 if sharded else None)
        v = tb.ks.get_index_values(boxes)
        t = iv = dt = None
    else:
        week = 7 * 86_400_000
        t = T0 + np.random.default_rng(9).integers(0, 6 * week, n)
        iv = (T0 + week // 2, T0 + 7 * week // 2)
        t[:200] = np.array([iv[0], iv[0] + 1, iv[1] - 1, iv[1]])[np.arange(200) % 4]
        tb = XZ3Table(*env, t, shard=sh, shards=4 if sharded else None)
        v = tb.ks.get_index_values(boxes, [during(*iv)])
        dt = tb.t
    arr, _ = key_ranges(tb.ks.get_ranges(v, target=2000), tb.shards)
    perm = as_np(tb.perm)
    cand = oracle.table_scan_rows(None if tb.shard is None else as_np(tb.shard),
                                  None if tb.bin is None else as_np(tb.bin), as_np(tb.z), arr)
    full = oracle.envelope_scan(*env, boxes, t, iv)
    keep = cand & full[perm]
    rows_exp = np.nonzero(keep)[0]
    assert 100 < len(rows_exp) < cand.sum()               # the full filter has candidates to reject
    assert not np.array_equal(perm, np.arange(n))

    f, hold = _full_filter(tb.env, v.spatialBounds, iv, dt, perm=tb.perm)
    ids, nm, ns = tb.table_scan(arr, f, map_rows=True)
    rows, nm2, ns2 = tb.table_scan(arr, f, map_rows=False)
    assert ns == ns2 == int(cand.sum()) and nm == nm2 == len(rows_exp)
    assert np.array_equal(as_np(rows), rows_exp)
    assert np.array_equal(as_np(ids), perm[rows_exp])
    assert np.array_equal(perm[as_np(rows)], as_np(ids))
    # input-order columns, rows = NULL: the perm argument maps them (a zero-initialised struct's behaviour)
    f0, hold0 = _full_filter(tb.env, v.spatialBounds, iv, dt)
    assert not f0.rows
    ids0, nm0, _ = tb.table_scan(arr, f0, map_rows=True)
    assert nm0 == nm and np.array_equal(as_np(ids0), perm[rows_exp])
    # columns in table order, no map at all
    tenv = tuple(c[tb.perm].contiguous() for c in tb.env)
    tt = None if dt is None else dt[tb.perm].contiguous()
    f1, hold1 = _full_filter(tenv, v.spatialBounds, iv, tt)
    rows1, nm1, _ = tb.table_scan(arr, f1, map_rows=False)
    assert nm1 == nm and np.array_equal(as_np(rows1), rows_exp)
    # table-order columns and ids mapped to input rows: rows = the identity, perm = the table's
    ident = torch.arange(n, device=tb.z.device)
    f2, hold2 = _full_filter(tenv, v.spatialBounds, iv, tt, perm=ident)
    ids2, nm2, _ = tb.table_scan(arr, f2, map_rows=True)
    assert nm2 == nm and np.array_equal(as_np(ids2), perm[rows_exp])
    del hold, hold0, hold1, hold2


# ---------------------------------------------------------------- envelope edge semantics

def jts_intersects(e, q):
    """JTS Envelope.intersects(Envelope) on (xmin, ymin, xmax, ymax) tuples, written out: isNull is
    maxx < minx and nothing else; then four comparisons, each false when a NaN is in it."""
    if e[2] < e[0] or q[2] < q[0]:
        return False
    return not (q[0] > e[2] or q[2] < e[0] or q[1] > e[3] or q[3] < e[1])


NAN, INF = math.nan, math.inf
UP10, DOWN0 = math.nextafter(10.0, INF), math.nextafter(0.0, -INF)
EDGE_ENVELOPES = [
    (0.0, 0.0, -1.0, -1.0),                                  # JTS's own null envelope
    (6.0, 2.0, 4.0, 8.0), (6.0, 8.0, 4.0, 2.0),              # x-inverted only; x and y inverted
    (2.0, 6.0, 8.0, 4.0), (2.0, 20.0, 8.0, 15.0),            # y-inverted only: inside, outside
    (2.0, 10.0, 8.0, 0.0), (2.0, 4.0, 8.0, -1.0),            # y-inverted only: on the edges, below
    (NAN, 2.0, 8.0, 8.0), (2.0, NAN, 8.0, 8.0), (2.0, 2.0, NAN, 8.0), (2.0, 2.0, 8.0, NAN),
    (NAN, 20.0, 8.0, 30.0), (20.0, NAN, 30.0, 8.0), (NAN, NAN, NAN, NAN),
    (-INF, -INF, INF, INF), (INF, 0.0, INF, 1.0), (-INF, 2.0, -INF, 8.0), (-INF, 2.0, 3.0, 8.0),
    (INF, 2.0, -INF, 8.0), (2.0, -INF, 8.0, INF), (2.0, INF, 8.0, INF), (2.0, INF, 8.0, -INF),
    (10.0, 5.0, 10.0, 5.0), (0.0, 5.0, 0.0, 5.0), (5.0, 10.0, 5.0, 10.0), (5.0, 0.0, 5.0, 0.0),   # on an edge
    (10.0, 10.0, 10.0, 10.0), (0.0, 0.0, 0.0, 0.0), (0.0, 10.0, 0.0, 10.0), (10.0, 0.0, 10.0, 0.0),  # on a corner
    (UP10, 5.0, UP10, 5.0), (DOWN0, 5.0, DOWN0, 5.0), (5.0, UP10, 5.0, UP10), (5.0, DOWN0, 5.0, DOWN0),
    (UP10, UP10, 11.0, 11.0), (-0.0, -0.0, -0.0, -0.0),
    (3.0, 3.0, 4.0, 4.0), (-5.0, -5.0, 15.0, 15.0), (20.0, 20.0, 30.0, 30.0),
]
EDGE_BOXES = [(0.0, 0.0, 10.0, 10.0)] + EDGE_ENVELOPES


def test_envelope_edges(gpu, oracle):
    """Defective envelopes against boxes with the same defects, one box per scan so that every (feature,
    box) pair is decided on its own, then all boxes at once.  The rule is JTS's, written out above;
    oracle.envelope_scan must state the same rule (an envelope inverted in y only is not null)."""
    e = np.array(EDGE_ENVELOPES)
    n = len(e)
    ht = HostTable(None, None, np.random.default_rng(1).permutation(n).astype(np.int64))
    cols = tuple(dev(e[:, k]) for k in range(4))
    arr = C.ranges_array([(0, 0, C.K80)])
    cand = np.ones(n, bool)
    seen = set()
    for q in EDGE_BOXES + [EDGE_BOXES]:
        boxes = np.array(q, np.float64).reshape(-1, 4)
        exp = np.array([any(jts_intersects(tuple(f), tuple(b)) for b in boxes.tolist()) for f in e.tolist()])
        assert np.array_equal(oracle.envelope_scan(e[:, 0], e[:, 1], e[:, 2], e[:, 3], boxes), exp), q
        check_scan(ht, arr, exp[ht.perm], cand, full_filter(cols, boxes, rows=ht.tb.perm), what=str(q))
        seen.add(int(exp.sum()))
    y_inv = (2.0, 6.0, 8.0, 4.0)
    assert jts_intersects(y_inv, EDGE_BOXES[0]) and not jts_intersects((6.0, 2.0, 4.0, 8.0), EDGE_BOXES[0])
    assert all(jts_intersects(f, EDGE_BOXES[0]) for f in EDGE_ENVELOPES[7:11])    # one NaN: no test fails
    assert 0 in seen and len(seen) > 5


# ---------------------------------------------------------------- two chunks of the count scan

def test_two_scan_chunks(gpu, oracle):
    """n = 4096 * 4096 + 4097 rows: 4098 blocks of 4096 candidates, so the count scan's second level sees
    two chunks and the id compaction crosses candidate 16,777,216.  z descends in input order, so the
    table is z = 0 .. n - 1 with perm[r] = n - 1 - r; the envelope filter keeps every 997th input row, the
    rows around the chunk boundary, the first and the last table row.  The same n through gm_strict_scan
    and gm_z3filter_scan, whose compaction is the same code."""
    import torch
    from geomesa_amd.table import _KeyTable
    n = 4096 * 4096 + 4097
    edge = 4096 * 4096
    r = torch.arange(n, device="cuda")
    tb = _KeyTable(None, (n - 1 - r).contiguous())
    assert torch.equal(tb.z, r) and torch.equal(tb.perm, n - 1 - r)
    inp = n - 1 - r                                                   # input row of table row r
    want = (inp % 997 == 0) | ((r >= edge - 2) & (r <= edge + 2)) | (r == 0) | (r == n - 1)
    col_t = torch.where(want, 0.5, 5.0).to(torch.float64)             # table order
    col = col_t.flip(0).contiguous()                                  # input order: row i = table row n - 1 - i
    boxes = np.array([[0.0, 0.0, 1.0, 1.0]])
    exp = inp[want]
    m = int(want.sum().item())
    assert m == exp.numel() and int(want[:edge].sum().item()) > 5 and bool(want[edge:].any()) and bool(want[n - 1])
    arr = C.ranges_array([(0, 0, (0xFFFF << 64) | C.U64)])            # UnboundedRange as key_ranges writes it
    ids, nm, ns = tb.table_scan(arr, full_filter((col,) * 4, boxes, rows=tb.perm), map_rows=True)
    assert (nm, ns) == (m, n) and torch.equal(ids, exp)
    rows, nm, ns = tb.table_scan(arr, full_filter((col_t,) * 4, boxes), map_rows=False)
    assert (nm, ns) == (m, n) and torch.equal(rows, r[want])
    del tb, rows, ids, inp

    # gm_strict_scan over the same column as x and y: point in box, ids ascending
    col_h = as_np(col)
    om = oracle.strict_scan(col_h, col_h, None, boxes[0])
    mk, ids, cnt = F.strict_scan(col, col, None, boxes[0], want_ids=True)
    exp_ids = torch.from_numpy(np.nonzero(om)[0]).cuda()
    assert cnt == m == exp_ids.numel() and torch.equal(ids, exp_ids) and torch.equal(mk, torch.from_numpy(om).cuda())
    del mk, ids, col, col_t, want

    # gm_z3filter_scan: arbitrary z words, a bin per row, the first adversarial filter
    z = r * -7046029254386353131                                      # a 64-bit mix of the row number
    z = (z ^ (z >> 31)) * -4658895280553007687
    z ^= z >> 29
    z[::3] &= 0x7FFFFFFF
    bins = (r % 14 - 4).to(torch.int16)
    fz = ADVERSARIAL_Z3[0]
    om = oracle.z3filter_scan(F.serialize_to_bytes(fz), [(2, 4)], as_np(bins), as_np(z))
    mk, ids, cnt = F.scan(fz, bins, z, [(2, 4)], want_ids=True)
    exp_ids = torch.from_numpy(np.nonzero(om)[0]).cuda()
    assert 0 < int(om[:edge].sum()) and om[edge:].any()
    assert cnt == exp_ids.numel() and torch.equal(ids, exp_ids) and torch.equal(mk, torch.from_numpy(om).cuda())
