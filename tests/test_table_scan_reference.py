"""oracle.table_scan_rows, the definition the table-scan GPU tests check gm_table_scan against, pinned to
the store's own rule: a row is in a scan range when its key BYTES [shard][bin BE16][z BE64]
(Z3IndexKeySpace.scala:81-92) lie between the range's end bytes (getRangeBytes, :196-238), compared as
byte strings."""
import struct

import numpy as np
import pytest

import table_scan_cases as C


def _pack(s, k80):
    return struct.pack(">BHQ", s, k80 >> 64, k80 & C.U64)


def brute_force(keys, rs):
    kb = [_pack(s, k) for s, k in keys]
    mask = np.zeros(len(kb), bool)
    for s, lo, hi in rs:
        lo_b, hi_b = _pack(s, lo), _pack(s, hi)
        mask |= np.array([lo_b <= k <= hi_b for k in kb], bool)
    return mask


def sorted_table(rng, n, sharded, binned):
    shard, bins, z = C.alphabet_table(rng, n, sharded, binned, n_random_z=12)
    o = C.table_order(shard, bins, z)
    return (None if shard is None else shard[o]), (None if bins is None else bins[o]), z[o]


@pytest.mark.parametrize("sharded,binned", C.TABLE_KINDS)
@pytest.mark.parametrize("n", [1, 2, 7, 64, 200])
def test_table_scan_rows_equals_byte_order(oracle, n, sharded, binned):
    """5 sizes x 4 key layouts x 100 random ranges = 2000, each range checked alone (so that no range
    hides another), then the shape groups and the union of everything."""
    rng = np.random.default_rng(1000 * n + 2 * sharded + binned)
    shard, bins, z = sorted_table(rng, n, sharded, binned)
    keys = C.keys80(shard, bins, z)
    hi, lo = oracle.table_key_u64(shard, np.zeros(n, np.int16) if bins is None else bins, z)
    assert sorted(zip(hi.tolist(), lo.tolist())) == list(zip(hi.tolist(), lo.tolist()))   # table order
    rs = C.random_ranges(rng, keys, 50) + C.random_ranges(rng, keys, 50, narrow=True)
    n_empty = 0
    for r in rs:
        got = oracle.table_scan_rows(shard, bins, z, C.ranges_array([r]))
        assert got.dtype == bool and np.array_equal(got, brute_force(keys, [r])), r
        n_empty += r[2] < r[1]
        assert not (r[2] < r[1] and got.any())
    assert n_empty > 0 or n < 7
    for name, g in C.shape_groups(keys, sharded).items():
        got = oracle.table_scan_rows(shard, bins, z, C.ranges_array(g))
        assert np.array_equal(got, brute_force(keys, g)), name
        rs += g
    assert np.array_equal(oracle.table_scan_rows(shard, bins, z, C.ranges_array(rs)), brute_force(keys, rs))


def test_table_scan_rows_shapes_do_what_their_names_say(oracle):
    """The groups meant to hit rows hit some, the ones meant to miss the table miss it."""
    rng = np.random.default_rng(5)
    shard, bins, z = sorted_table(rng, 200, True, True)
    keys = C.keys80(shard, bins, z)
    g = C.shape_groups(keys, True)
    count = {k: int(oracle.table_scan_rows(shard, bins, z, C.ranges_array(v)).sum()) for k, v in g.items()}
    for k in ("empty", "absent_shard", "above_table"):
        assert count[k] == 0, k
    for k in ("single_key", "first_and_last_key", "thrice", "nested", "overlapping", "adjacent_next_bin"):
        assert count[k] > 0, k
    assert count["whole_table"] == 200
    assert count["nested"] == int((shard == sorted(set(keys))[len(set(keys)) // 2][0]).sum())


def test_table_scan_rows_degenerate(oracle):
    z = np.array([3, 5], np.int64)
    none = np.zeros(0, C.KEY_RANGE_DTYPE)
    assert oracle.table_scan_rows(None, None, z, none).tolist() == [False, False]
    assert oracle.table_scan_rows(None, None, z[:0], C.ranges_array([(0, 0, C.K80)])).tolist() == []
    # without a bin column a row's bin reads as 0: the forms key_ranges emits for "lower" (bin_hi = -1) hold it
    assert oracle.table_scan_rows(None, None, z, C.ranges_array([(0, 4, (0xFFFF << 64) | C.U64)])).tolist() == [
        False, True]
    # z compares unsigned: -1 is the largest z
    zz = np.array([0, 2**63 - 1, -2**63, -1], np.int64)
    assert oracle.table_scan_rows(None, None, zz, C.ranges_array([(0, 1 << 63, C.U64)])).tolist() == [
        False, False, True, True]
