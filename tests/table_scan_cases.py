"""Shared inputs of the table-scan tests (test_table_scan_reference.py, test_gpu_table_scan.py): tables
whose keys come from a small alphabet, so that duplicated keys and range ends that land on a key are the
common case, and scan ranges drawn around those keys.

A key is handled as Python ints: `shard` (0..255) and the 80-bit in-shard key `bin as u16 << 64 | z as
u64` (a gm_key_range has one shard for both of its ends).  Nothing here imports the HIP library."""
import numpy as np

from geomesa_amd._lib import KEY_RANGE_DTYPE

BINS = [-32768, -2, -1, 0, 1, 2600, 32767]
Z_EDGES = [0, 1, 2**63 - 1, -2**63, -1]
SHARDS = 4                       # shard column, when present: 0..3
ABSENT_SHARD = 7                 # a shard no table here has
TABLE_SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 20_011]
TABLE_KINDS = [(False, False), (False, True), (True, False), (True, True)]   # (sharded, binned)
K80 = (1 << 80) - 1
U64 = (1 << 64) - 1


def alphabet_table(rng, n, sharded, binned, n_random_z=50):
    """Unsorted (shard u8 | None, bins i16 | None, z i64) columns of n rows."""
    zs = np.concatenate([np.array(Z_EDGES, np.int64),
                         rng.integers(-2**63, 2**63 - 1, n_random_z, dtype=np.int64, endpoint=True)])
    z = zs[rng.integers(0, len(zs), n)]
    bins = np.array(BINS, np.int16)[rng.integers(0, len(BINS), n)] if binned else None
    shard = rng.integers(0, SHARDS, n).astype(np.uint8) if sharded else None
    return shard, bins, z


def table_order(shard, bins, z):
    """The stable sort gm_sort_keys performs (test_sort_keys_parity pins it): input rows in table order."""
    keys = [np.asarray(z).view(np.uint64)]
    if bins is not None:
        keys.append(np.asarray(bins).view(np.uint16))
    if shard is not None:
        keys.append(np.asarray(shard, np.uint8))
    return np.lexsort(keys)


def keys80(shard, bins, z):
    """Per row: (shard, 80-bit in-shard key) as Python ints."""
    n = len(z)
    zu = np.asarray(z).view(np.uint64).tolist()
    bu = np.asarray(bins).view(np.uint16).tolist() if bins is not None else [0] * n
    sh = np.asarray(shard).tolist() if shard is not None else [0] * n
    return [(s, (b << 64) | v) for s, b, v in zip(sh, bu, zu)]


def ranges_array(rs):
    """[(shard, lo80, hi80)] -> gm_key_range rows."""
    arr = np.zeros(len(rs), KEY_RANGE_DTYPE)
    for i, (s, lo, hi) in enumerate(rs):
        assert 0 <= lo <= K80 and 0 <= hi <= K80 and 0 <= s < 256
        arr["shard"][i] = s
        arr["bin_lo"][i] = np.array(lo >> 64, np.uint16).view(np.int16)
        arr["bin_hi"][i] = np.array(hi >> 64, np.uint16).view(np.int16)
        arr["z_lo"][i] = np.array(lo & U64, np.uint64).view(np.int64)
        arr["z_hi"][i] = np.array(hi & U64, np.uint64).view(np.int64)
    return arr


def _near(rng, k):
    return min(max(k + int(rng.integers(-1, 2)), 0), K80)


def random_ranges(rng, keys, count, narrow=False):
    """`count` ranges whose ends are table keys or their +-1 neighbours in key order.  About one in eight
    is left as drawn (so hi < lo, an empty range, occurs); narrow: hi is drawn within two distinct keys of
    lo, so most ranges stay apart and survive merging."""
    if not keys:
        keys = [(0, 0)]
    by_shard = {}
    for s, k in set(keys):
        by_shard.setdefault(s, []).append(k)
    shards = sorted(by_shard)
    for s in shards:
        by_shard[s].sort()
    out = []
    for _ in range(count):
        s = shards[int(rng.integers(0, len(shards)))]
        ks = by_shard[s]
        i = int(rng.integers(0, len(ks)))
        j = min(i + int(rng.integers(0, 3)), len(ks) - 1) if narrow else int(rng.integers(0, len(ks)))
        lo, hi = _near(rng, ks[i]), _near(rng, ks[j])
        if hi < lo and rng.integers(0, 8):
            lo, hi = hi, lo
        out.append((s, lo, hi))
    return out


def shape_groups(keys, sharded):
    """The range shapes every scan must get right, built around the table's own keys: name -> ranges.
    Each group is scanned on its own (a wide range in the same call would hide a narrow one's mistake) and
    all of them together."""
    distinct = sorted(set(keys))
    s0, k0 = distinct[0]
    s1, k1 = distinct[len(distinct) // 2]
    s2, k2 = distinct[-1]
    same = [k for s, k in distinct if s == s1]
    a, b = same[0], same[-1]
    q1, q2, q3 = (same[len(same) * i // 4] for i in (1, 2, 3))
    bin_ = lambda v: (v & 0xFFFF) << 64
    g = {
        "empty": [(s1, k1, k1 - 1) if k1 else (s1, 1, 0), (s1, K80, 0), (s1, bin_(1), bin_(0) | U64)],
        "single_key": [(s1, k1, k1)],
        "first_and_last_key": [(s0, k0, k0), (s2, k2, k2)],
        "thrice": [(s1, q1, q2)] * 3,
        "nested": [(s1, q1, q3), (s1, q2, q2), (s1, a, b)],
        "overlapping": [(s1, q2, b), (s1, a, q2), (s1, q1, q3)],
        "adjacent_key_step": [(s1, min(q2 + 1, K80), max(q3, min(q2 + 1, K80))), (s1, q1, q2)],
        # z = all ones carries into the next bin (bins 0 -> 1 and -2 -> -1 are in the alphabet)
        "adjacent_next_bin": [(s1, bin_(1), bin_(1) | 5), (s1, bin_(0) | 1, bin_(0) | U64),
                              (s1, bin_(-2) | (U64 - 3), bin_(-2) | U64), (s1, bin_(-1), bin_(-1) | 1)],
        # bin 0xFFFF, z = all ones carries into the next shard's bin 0, z = 0
        "adjacent_next_shard": [(s0 + 1, 0, 3), (s0, bin_(-1) | (U64 - 3), bin_(-1) | U64)],
        # one short of adjacent: the key between them (next bin, z = 0) stays out
        "not_adjacent": [(s1, bin_(0) | U64, bin_(0) | U64), (s1, bin_(1) | 1, bin_(1) | 1)],
        "absent_shard": [(ABSENT_SHARD, 0, K80), (ABSENT_SHARD - 1, 5, 5), (ABSENT_SHARD, 0, 0)],
        "above_table": [(s2, k2 + 1, K80) if k2 < K80 else (s2 + 1, 0, K80),
                        (SHARDS if sharded else 1, 0, K80)],
        "whole_table": [(s, 0, K80) for s in range(SHARDS if sharded else 1)],
    }
    if s0 > 0:
        g["below_table"] = [(0, 0, K80)]
    elif k0 > 0:
        g["below_table"] = [(0, 0, k0 - 1)]
    return g
