"""The digit plan of gm_sort_keys restated in plain Python, key generators that hit a chosen plan, and the
cases the plan / run-geometry tests share (test_sort_plan.py on the host, test_gpu_sort_plan.py on the GPU).

The rule (DESIGN.md "Sort"): the key K = shard:bin:z is an 88-bit integer -- z in bits 0..63, bin in
64..79, shard in 80..87.  A bit varies when the OR and the AND of the column differ there.  With a shard
column the key is squeezed first: the shard moves down to sit right above bin's highest varying bit (bit
sq of bs = bin | shard << 16), and bin's constant bits above it (binhi) leave the key.  `lsd` names every
byte of that key on which some bit varies.  A prefix plan takes npre = ceil(pbits / 9) digits (4 at most)
of pw = ceil(pbits / npre) bits, pbits = max(1, ceil(log2 n) - 1): the first digit ends at the highest
varying bit, each later one at the highest varying bit below the digit before it, and a digit that would
start below bit 0 starts at bit 0.  The prefix plan holds in mode 0 when all npre digits were found and
the varying bytes are more than npre; every other call sorts by the `lsd` bytes.

Nothing here reads the C++ planner: test_sort_plan.py compares the two.
"""
import collections
import functools

import numpy as np

Plan = collections.namedtuple("Plan", "prefix npre pw pofs sq binhi lsd")

T = 1792            # k_local_bounds cuts near multiples of LSTEP
RUN_MAX = 256       # k_sort_local ranks runs of at most this many rows
SAMPLE = 65536      # rows of the strided sample the first plan is made from

Z_BITS = frozenset(range(64))
ALL_BITS = frozenset(range(88))


def ceil_log2(n):
    return (int(n) - 1).bit_length()


def plan(or_z, or_bs, and_z, and_bs, sharded, n, mode):
    """The plan of one sort from the OR / AND of z and of bs = bin | shard << 16, n and GM_PARAM_SORT_MODE."""
    var_z = (or_z ^ and_z) & (2**64 - 1)
    var_bin = (or_bs ^ and_bs) & 0xffff
    var_sh = ((or_bs ^ and_bs) >> 16) & 0xff
    if sharded:
        sq = var_bin.bit_length()
        binhi = (and_bs & 0xffff) >> sq << sq
        var_hi = var_bin | (var_sh << sq)
    else:
        sq, binhi = 16, 0
        var_hi = var_bin
    var = var_z | (var_hi << 64)
    lsd = tuple(8 * b for b in range(11) if (var >> (8 * b)) & 0xff)
    if not lsd:
        return Plan(False, 0, 0, (-1, -1, -1, -1), sq, binhi, lsd)
    pbits = max(1, ceil_log2(n) - 1)
    npre = min(4, -(-pbits // 9))
    pw = min(9, -(-pbits // npre))
    pofs, rest = [], var
    while len(pofs) < npre and rest:
        top = rest.bit_length() - 1
        pofs.append(max(0, top - pw + 1))
        rest &= (1 << pofs[-1]) - 1
    found = len(pofs)
    pofs += [-1] * (4 - found)
    return Plan(mode == 0 and len(lsd) > npre and found == npre, npre, pw, tuple(pofs), sq, binhi, lsd)


def first_digits(p):
    """The digits of the first pass set, (offset, width) in pass order: what the sample's plan counts."""
    if p.prefix:
        return tuple((o, p.pw) for o in reversed(p.pofs[:p.npre]))
    return tuple((o, 8) for o in p.lsd)


def or_and(shard, bins, z):
    """(or_z, or_bs, and_z, and_bs) of key columns, as Python ints."""
    zu = np.asarray(z).view(np.uint64)
    bs = np.asarray(bins).view(np.uint16).astype(np.uint32)
    if shard is not None:
        bs = bs | (np.asarray(shard, np.uint8).astype(np.uint32) << 16)
    return (int(np.bitwise_or.reduce(zu)), int(np.bitwise_or.reduce(bs)),
            int(np.bitwise_and.reduce(zu)), int(np.bitwise_and.reduce(bs)))


def plan_of(shard, bins, z, mode, rows=None):
    """plan() of these columns; `rows` restricts the OR / AND to a subset (the sample)."""
    n = len(z)
    if rows is not None:
        shard, bins, z = (None if shard is None else shard[rows]), bins[rows], z[rows]
    return plan(*or_and(shard, bins, z), shard is not None, n, mode)


def sample_rows(n):
    """The rows k_key_or_and_sample reads: every (n // 65536)-th of the first 65,536 such, and the last."""
    step = n // SAMPLE if n > SAMPLE else 1
    r = np.arange(0, min(n, SAMPLE * step), step)
    return np.union1d(r, [n - 1])


def layout_plan(layout, sharded, n, mode=0):
    """plan() for keys whose varying bits are exactly `layout` (constant bits 0: binhi is not told by it)."""
    v = sum(1 << b for b in layout)
    return plan(v & (2**64 - 1), v >> 64, 0, 0, sharded, n, mode)


def _squeezed(p, shard, bins, z):
    zu = np.asarray(z).view(np.uint64)
    bs = np.asarray(bins).view(np.uint16).astype(np.uint64)
    if shard is not None:
        bs = (bs & np.uint64((1 << p.sq) - 1)) | (np.asarray(shard, np.uint8).astype(np.uint64) << np.uint64(p.sq))
    return bs, zu


def prefix_of(p, shard, bins, z):
    """The plan's prefix digits of every row, concatenated (first digit on top), as uint64."""
    bs, zu = _squeezed(p, shard, bins, z)
    out = np.zeros(len(zu), np.uint64)
    mask = np.uint64((1 << p.pw) - 1)
    for off in p.pofs[:p.npre]:
        if off < 0:
            continue
        if off >= 64:
            d = bs >> np.uint64(off - 64)
        else:
            d = zu >> np.uint64(off)
            if off > 0:
                d = d | (bs << np.uint64(64 - off))   # bits past 64 fall off: a digit is 9 bits at most
        out = (out << np.uint64(p.pw)) | (d & mask)
    return out


def longest_run(prefix):
    """Rows of the most frequent prefix: equal prefixes are adjacent once the prefix passes have run."""
    return int(np.unique(prefix, return_counts=True)[1].max())


def expected_last(p, prefix):
    """GM_PARAM_SORT_LAST after the call: 0 when every key is equal; 256 + npre when the prefix passes and
    the local ranks did it; else the byte passes, plus npre when a prefix plan was tried and gave up."""
    if not p.lsd:
        return 0
    if not p.prefix:
        return len(p.lsd)
    return 256 + p.npre if longest_run(prefix) <= RUN_MAX else len(p.lsd) + p.npre


def _masks(layout):
    v = sum(1 << b for b in layout)
    return v & (2**64 - 1), (v >> 64) & 0xffff, v >> 80


def keys(layout, n, sharded, rng, extremes="sampled"):
    """(shard or None, bins i16, z i64): n keys whose varying bits are exactly `layout` (bit positions of
    shard:bin:z).  Varying bits are random, constant bits come from one random constant (bin's top constant
    bit is set, so binhi != 0 whenever bin bit 15 is constant).  One row has every varying bit 0 and one has
    every one 1.  extremes="sampled": rows 0 and n - 1, which the sample reads.  "missed": the all-ones row
    sits where the sample does not look, and it alone sets the layout's highest bit, so the sample's OR /
    AND misses that bit."""
    layout = frozenset(layout)
    assert layout and layout <= ALL_BITS and n >= 2 and (sharded or max(layout) < 80)
    mz, mb, ms = _masks(layout)
    cz = int(rng.integers(0, 2**64, dtype=np.uint64)) & ~mz & (2**64 - 1)
    cb = (int(rng.integers(0, 2**16)) | 0x8000) & ~mb & 0xffff
    cs = int(rng.integers(0, 2**8)) & ~ms & 0xff
    vz = rng.integers(0, 2**64, n, dtype=np.uint64) & np.uint64(mz)
    vb = rng.integers(0, 2**16, n).astype(np.uint16) & np.uint16(mb)
    vs = rng.integers(0, 2**8, n).astype(np.uint8) & np.uint8(ms)
    ones = n - 1
    if extremes == "missed":
        step = n // SAMPLE
        assert step >= 2, "every row of a table of fewer than 2 * 65,536 rows is sampled"
        ones = n // 2
        while ones % step == 0:
            ones += 1
        assert ones < n - 1
        top = max(layout)
        if top < 64:
            vz &= np.uint64(~(1 << top) & (2**64 - 1))
        elif top < 80:
            vb &= np.uint16(~(1 << (top - 64)) & 0xffff)
        else:
            vs &= np.uint8(~(1 << (top - 80)) & 0xff)
    else:
        assert extremes == "sampled"
    vz[0], vb[0], vs[0] = 0, 0, 0
    vz[ones], vb[ones], vs[ones] = mz, mb, ms
    z = (vz | np.uint64(cz)).view(np.int64)
    bins = (vb | np.uint16(cb)).view(np.int16)
    shard = (vs | np.uint8(cs)) if sharded else None
    return shard, bins, z


def deposit(values, bits):
    """Bit i of every value placed at key bit bits[i] (ascending): (shard u8, bin u16, z u64) parts."""
    v = np.asarray(values, np.uint64)
    z = np.zeros(len(v), np.uint64); b = np.zeros(len(v), np.uint64); s = np.zeros(len(v), np.uint64)
    for i, bit in enumerate(sorted(bits)):
        x = (v >> np.uint64(i)) & np.uint64(1)
        if bit < 64:
            z |= x << np.uint64(bit)
        elif bit < 80:
            b |= x << np.uint64(bit - 64)
        else:
            s |= x << np.uint64(bit - 80)
    return s.astype(np.uint8), b.astype(np.uint16), z


def run_keys(runs, field, low, rng, sharded):
    """Keys whose sorted order holds runs of equal `field` values of the given lengths, in that order.
    `field` and `low` are bit positions: the run's value goes into `field` (values ascend with the runs;
    the first is 0 and the last all ones, so every field bit varies), random values into `low` (both
    extremes forced, so every low bit varies; 256 values over a run of 256 rows leave ties, which stability
    decides).  Every other bit is one random constant.  The rows are shuffled."""
    field, low = sorted(field), sorted(low)
    runs = np.asarray(runs, np.int64)
    n, nv = int(runs.sum()), 1 << len(field)
    assert 2 <= len(runs) <= nv and runs.min() >= 1
    vals = np.sort(rng.choice(np.arange(1, nv - 1), len(runs) - 2, replace=False))
    vals = np.concatenate([[0], vals, [nv - 1]]).astype(np.uint64)
    fv = np.repeat(vals, runs)
    lv = rng.integers(0, 1 << len(low), n).astype(np.uint64)
    lv[0], lv[n - 1] = 0, (1 << len(low)) - 1
    fs, fb, fz = deposit(fv, field)
    ls, lb, lz = deposit(lv, low)
    mz, mb, ms = _masks(frozenset(field) | frozenset(low))
    cz = int(rng.integers(0, 2**64, dtype=np.uint64)) & ~mz & (2**64 - 1)
    cb = (int(rng.integers(0, 2**16)) | 0x8000) & ~mb & 0xffff
    cs = int(rng.integers(0, 2**8)) & ~ms & 0xff
    perm = rng.permutation(n)
    z = ((fz | lz | np.uint64(cz))[perm]).view(np.int64)
    bins = ((fb | lb | np.uint16(cb))[perm]).view(np.int16)
    shard = (fs | ls | np.uint8(cs))[perm] if sharded else None
    assert sharded or ms == 0
    return shard, bins, z


# ------------------------------------------------------------------ the plan grid
# One entry per case: (name, n, layout, shardings).  `shardings` lists the values of `sharded` the layout
# allows: a layout with shard bits needs the shard column; the seam cases are about the squeezed key.
def _bits(*ranges):
    out = set()
    for r in ranges:
        out |= set(range(r[0], r[1] + 1)) if isinstance(r, tuple) else {r}
    return frozenset(out)


BOTH, SHARDED, UNSHARDED = (False, True), (True,), (False,)

PLAN_GRID = [
    # n = 2^k: pbits = max(1, k - 1).  One digit up to k = 10, two from k = 11.
    ("k1_two_rows", 2**1, _bits(62, 70, 3), BOTH),
    ("k2_z_top", 2**2, _bits((60, 63), (0, 7), (20, 23)), BOTH),
    ("k3_bin_only_plus_low", 2**3, _bits((64, 66), (8, 15), (30, 33)), BOTH),
    ("k4_shard_to_255", 2**4, _bits((80, 87), (0, 9), (40, 47)), SHARDED),                 # key bit 87 varies
    ("k5_seam_sq0", 2**5, _bits((80, 81), (60, 63), (0, 7), (16, 19)), SHARDED),           # shard right on z
    ("k6_straddle_63_64", 2**6, _bits((64, 65), (61, 63), (0, 7), (24, 27)), BOTH),
    ("k7_seam_sq5", 2**7, _bits((80, 82), (64, 68), (0, 7), (32, 35)), SHARDED),
    ("k8_seam_sq16", 2**8, _bits((80, 83), (76, 79), (0, 7), (50, 52)), SHARDED),
    ("k9_full_z", 2**9, _bits((0, 63)), BOTH),
    ("k10_nine_bit_digit_over_63_64", 2**10, _bits((60, 67), (0, 7), (30, 34)), BOTH),
    ("k11_gap_between_digits", 2**11, _bits((58, 62), (30, 34), (0, 7)), BOTH),            # constants between
    ("k12_long_runs", 2**12, _bits(62, 61, 40, 20, 3), BOTH),                              # 8 prefixes: runs > 256
    ("k13_bin_and_z", 2**13, _bits((64, 70), (56, 63), (0, 7)), BOTH),
    ("k14_shard_bin_z", 2**14, _bits((80, 81), (64, 70), (58, 63), (0, 7)), SHARDED),
    ("k15_full_key", 2**15, _bits((0, 79)), BOTH),
    ("k16_weekly_like", 2**16, _bits((64, 69), (0, 62)), BOTH),
    ("k17_shard_16_up", 2**17, _bits((80, 84), (64, 69), (20, 62)), SHARDED),              # shard values to 31
    ("k18_gap_and_seam", 2**18, _bits((80, 81), (64, 70), (20, 39), (0, 3)), SHARDED),
    ("k19_full_key_sharded", 2**19, _bits((80, 87), (64, 79), (0, 63)), SHARDED),
    ("k19_z_only", 2**19, _bits((10, 62)), BOTH),
    # n = 2^19 + 1: three digits of 7 bits
    ("three_by_7_clamped_overlap", 2**19 + 1, _bits((69, 75), (0, 11)), BOTH),             # pofs = [69, 5, 0]
    ("three_by_7_runs_out", 2**19 + 1, _bits(71, 72, 55, 56), BOTH),                       # nfound 2 < npre 3
    ("three_by_7_plain", 2**19 + 1, _bits((64, 69), (30, 63), (0, 7)), BOTH),
    # n = 2^22 + 1: three digits of 8 bits
    ("three_by_8", 2**22 + 1, _bits((64, 69), (0, 62)), BOTH),
]


def grid_cases():
    """(id, name, n, layout, sharded, extremes) of every run of the plan grid.  "missed" needs a sample step
    of 2 or more, n >= 2 * 65,536: below that the sample reads every row."""
    out = []
    for name, n, layout, shardings in PLAN_GRID:
        for sharded in shardings:
            for extremes in ("sampled", "missed") if n // SAMPLE >= 2 else ("sampled",):
                out.append(("%s-%s-%s" % (name, "sharded" if sharded else "flat", extremes), name, n, layout, sharded,
                            extremes))
    return out


@functools.lru_cache(maxsize=4)
def grid_keys(name, sharded, extremes):
    """The columns of one grid case and their table order (the keys depend on the case, not on the mode)."""
    import table_scan_cases as C
    (n, layout), = [(c[1], c[2]) for c in PLAN_GRID if c[0] == name]
    seed = [k for k, c in enumerate(PLAN_GRID) if c[0] == name][0] * 4 + 2 * sharded + (extremes == "missed")
    shard, bins, z = keys(layout, n, sharded, np.random.default_rng(seed), extremes)
    return shard, bins, z, C.table_order(shard, bins, z)


# ------------------------------------------------------------------ plan properties (from plan() alone)
def digits_of(p):
    return [(o, o + p.pw - 1) for o in p.pofs[:p.npre] if o >= 0]


def prop_npre_pw(npre, pw):
    return lambda p, layout, sharded: p.prefix and (p.npre, p.pw) == (npre, pw)


def prop_straddles_63_64(p, layout, sharded):
    return p.prefix and any(lo <= 63 and hi >= 64 for lo, hi in digits_of(p))


def prop_straddles_seam(sq_ok):
    def f(p, layout, sharded):
        seam = 64 + p.sq          # the shard's lowest bit in the squeezed key
        return sharded and p.prefix and sq_ok(p.sq) and any(lo < seam <= hi for lo, hi in digits_of(p)) \
            and any(b >= 80 for b in layout)
    return f


def prop_constants_between(p, layout, sharded):
    d = digits_of(p)
    return p.prefix and any(d[k][0] - 1 > d[k + 1][1] for k in range(len(d) - 1))


def prop_clamped_overlap(p, layout, sharded):
    d = digits_of(p)
    return p.prefix and len(d) >= 2 and d[-1][0] == 0 and d[-1][1] >= d[-2][0]


def prop_runs_out(p, layout, sharded):
    return not p.prefix and len([o for o in p.pofs if o >= 0]) < p.npre and len(p.lsd) > p.npre


def prop_bit87(p, layout, sharded):
    return sharded and 87 in layout


PLAN_PROPERTIES = [("npre=%d pw=%d" % (a, b), prop_npre_pw(a, b), name) for a, b, name in [
    (1, 1, "k1_two_rows"), (1, 2, "k3_bin_only_plus_low"), (1, 3, "k4_shard_to_255"), (1, 4, "k5_seam_sq0"),
    (1, 5, "k6_straddle_63_64"), (1, 6, "k7_seam_sq5"), (1, 7, "k8_seam_sq16"), (1, 8, "k9_full_z"),
    (1, 9, "k10_nine_bit_digit_over_63_64"), (2, 5, "k11_gap_between_digits"), (2, 6, "k13_bin_and_z"),
    (2, 7, "k14_shard_bin_z"), (2, 8, "k16_weekly_like"), (2, 9, "k18_gap_and_seam"),
    (3, 7, "three_by_7_plain"), (3, 8, "three_by_8")]] + [
    ("digit over key bit 63 | 64", prop_straddles_63_64, "k10_nine_bit_digit_over_63_64"),
    ("digit over the bin | shard seam, sq = 0", prop_straddles_seam(lambda s: s == 0), "k5_seam_sq0"),
    ("digit over the bin | shard seam, sq in 1..15", prop_straddles_seam(lambda s: 1 <= s <= 15), "k7_seam_sq5"),
    ("digit over the bin | shard seam, sq = 16", prop_straddles_seam(lambda s: s == 16), "k8_seam_sq16"),
    ("only constant bits between two digits", prop_constants_between, "k11_gap_between_digits"),
    ("last digit clamped to 0 and overlapping", prop_clamped_overlap, "three_by_7_clamped_overlap"),
    ("nfound < npre, varying bytes > npre", prop_runs_out, "three_by_7_runs_out"),
    ("key bit 87 varies", prop_bit87, "k4_shard_to_255"),
]
# two more properties need the keys, not only the layout: binhi != 0 (k7_seam_sq5) and a prefix plan whose
# longest run exceeds 256 rows (k12_long_runs); test_sort_plan.py checks them on grid_keys().


# ------------------------------------------------------------------ run geometry
def small_runs(total, rng):
    """Run lengths of 1..3 rows that add up to `total`."""
    out, left = [], int(total)
    while left > 0:
        r = min(left, int(rng.integers(1, 4)))
        out.append(r)
        left -= r
    return out


FIELD_Z, LOW = _bits((49, 62)), _bits((0, 7))       # n in (2^14, 2^15]: two digits of 7 bits = z bits 49..62
FIELD_Z12 = _bits((51, 62))                         # n in (2^12, 2^13]: two digits of 6 bits = z bits 51..62
FIELD_SB = _bits((80, 84), (64, 72))                # shard bits 0..4 over bin bits 0..8: squeezed bits 64..77

# name -> (field, sharded, builder(rng) -> run lengths in sorted order, [(start, length)] claimed, n claimed)
def _geo(name, field, sharded, build, claims, n):
    return (name, field, sharded, build, claims, n)


def _around(start, length, n):
    return lambda rng: small_runs(start, rng) + [length] + small_runs(n - start - length, rng)


GEOMETRY = [
    _geo("run256_ends_at_T", FIELD_Z, False, _around(T - 256, 256, 9 * T + 777), [(T - 256, 256)], 9 * T + 777),
    _geo("run256_from_T_minus_1", FIELD_Z, False, _around(T - 1, 256, 9 * T + 777), [(T - 1, 256)], 9 * T + 777),
    _geo("run256_from_T_minus_255", FIELD_Z, False, _around(T - 255, 256, 9 * T + 777), [(T - 255, 256)], 9 * T + 777),
    _geo("run256_from_2T", FIELD_Z, False, _around(2 * T, 256, 9 * T + 777), [(2 * T, 256)], 9 * T + 777),
    _geo("seventy_runs_of_256", FIELD_Z, False, lambda rng: [256] * 70, [(256 * k, 256) for k in range(70)], 10 * T),
    # 2^14 prefix values cannot give more than 2^14 runs, and n must exceed 2^14: one run holds two rows
    _geo("runs_of_one_row", FIELD_Z, False, lambda rng: [1] * 9000 + [2] + [1] * 7383,
         [(0, 1), (8999, 1), (9000, 2), (9002, 1), (16384, 1)], 2**14 + 1),
    _geo("run257_mid_tile", FIELD_Z, False, _around(T + 700, 257, 9 * T + 777), [(T + 700, 257)], 9 * T + 777),
    _geo("run257_from_T_minus_1", FIELD_Z, False, _around(T - 1, 257, 9 * T + 777), [(T - 1, 257)], 9 * T + 777),
    _geo("run600_across_a_bound", FIELD_Z, False, _around(2 * T - 300, 600, 9 * T + 777), [(2 * T - 300, 600)], 9 * T + 777),
    # the last run reaches n across the last bound, so the last tile holds no row.  At n = 3 T + 100 the plan
    # is two digits of 6 bits (n <= 2^13), so that case's field is 12 bits; the same shape at 10 T + 100 has
    # the 14-bit field of the other cases
    _geo("last_run_from_3T_minus_50", FIELD_Z12, False, _around(3 * T - 50, 150, 3 * T + 100), [(3 * T - 50, 150)], 3 * T + 100),
    _geo("last_run_from_10T_minus_50", FIELD_Z, False, _around(10 * T - 50, 150, 10 * T + 100), [(10 * T - 50, 150)],
         10 * T + 100),
    _geo("n_is_10T_plus_1", FIELD_Z, False, lambda rng: small_runs(10 * T + 1, rng), [], 10 * T + 1),
    _geo("sharded_run256_from_T_minus_1", FIELD_SB, True, _around(T - 1, 256, 9 * T + 777), [(T - 1, 256)], 9 * T + 777),
    _geo("sharded_run257_from_T_minus_1", FIELD_SB, True, _around(T - 1, 257, 9 * T + 777), [(T - 1, 257)], 9 * T + 777),
]
GEOMETRY_NAMES = [g[0] for g in GEOMETRY]


@functools.lru_cache(maxsize=None)
def geometry_keys(name):
    """(shard, bins, z, table order, run lengths in sorted order) of one geometry case."""
    import table_scan_cases as C
    k = GEOMETRY_NAMES.index(name)
    _, field, sharded, build, _, n = GEOMETRY[k]
    rng = np.random.default_rng(1000 + k)
    runs = build(rng)
    assert sum(runs) == n
    shard, bins, z = run_keys(runs, field, LOW, rng, sharded)
    return shard, bins, z, C.table_order(shard, bins, z), runs
