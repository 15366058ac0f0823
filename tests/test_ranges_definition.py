"""The range definition (ranges_definition.py) on the CPU: the oracle under the checkers, at the
inputs that test_gpu_ranges_definition.py gives the kernels, and the checkers against broken lists.

The first pins oracle/gm_oracle.c's range walks to what a range list must be, not only to the reference's
unit tests, and proves that every input set and every no-vacuous-pass condition of the GPU file can be
met by the reference alone: a failure there is then a fact about a kernel."""
import numpy as np
import pytest

import ranges_definition as RD
import ranges_definition_cases as C


def _period(oracle, p):
    return oracle.PERIODS[p]


class OracleBackend:
    def __init__(self, oracle):
        self.o = oracle

    def zranges(self, D, qs, mr, rec):
        return [self.o.zranges(D, q, 64, mr, rec) for q in qs]

    def z_user_ranges(self, period, precision, qs, mr):
        if period is None:
            return [self.o.z2_ranges(b, 64, mr, sfc_precision=precision) for b, _ in qs]
        return [self.o.z3_ranges(b, t, 64, mr, period=_period(self.o, period), sfc_precision=precision) for b, t in qs]

    def z_user_index(self, period, precision, x, y, t):
        if period is None:
            out = [self.o.z2_index(float(a), float(b), precision=precision) for a, b in zip(x, y)]
        else:
            p = _period(self.o, period)
            out = [self.o.z3_index(float(a), float(b), int(c), period=p, precision=precision) for a, b, c in zip(x, y, t)]
        assert all(st == 0 for st, _ in out)
        return np.array([z for _, z in out], np.int64)

    def xz_ranges(self, D, g, period, qs, mr):
        if D == 2:
            return [self.o.xz2_ranges(q, mr, g=g) for q in qs]
        return [self.o.xz3_ranges(q, mr, g=g, period=_period(self.o, period)) for q in qs]

    def xz_index(self, D, g, period, env):
        codes, st = self.o.xz2_index_batch(env, g=g) if D == 2 else \
            self.o.xz3_index_batch(env, g=g, period=_period(self.o, period))
        assert not st.any()
        return codes


@pytest.fixture(scope="module")
def be(oracle):
    return OracleBackend(oracle)


# ---------------------------------------------------------------- the definition's own arithmetic
def test_interleave_roundtrip_and_known_values():
    rng = np.random.default_rng(3)
    for D, nbits in ((2, 31), (3, 21)):
        dims = [rng.integers(0, 1 << nbits, 1000) for _ in range(D)]
        z = RD.interleave(dims)
        assert all(np.array_equal(a, b) for a, b in zip(RD.deinterleave(z, D), dims))
    # Z2(2, 3) = 0b1110, Z3(1, 2, 4) = 0b100_010_001: bit i of dimension d is bit D * i + d
    assert int(RD.interleave([np.int64(2), np.int64(3)])) == 0b1110
    assert int(RD.interleave([np.int64(1), np.int64(2), np.int64(4)])) == 0b100010001


def test_interleave_is_the_curves(oracle):
    rng = np.random.default_rng(4)
    for _ in range(200):
        x, y, t = (int(v) for v in rng.integers(0, 1 << 21, 3))
        assert int(RD.interleave([np.int64(x), np.int64(y), np.int64(t)])) == oracle.z3_apply(x, y, t)
        x, y = (int(v) for v in rng.integers(0, 1 << 31, 2))
        assert int(RD.interleave([np.int64(x), np.int64(y)])) == oracle.z2_apply(x, y)


def test_xz_elements_codes_are_the_curves(oracle):
    """An element's code is what XZ2SFC / XZ3SFC.index gives a box that starts at the element's centre
    and is 1.2 of its widths long: too long for the next level, and inside the element's enlarged cell."""
    for D, g in ((2, 4), (3, 3)):
        lev, corners, widths, codes = RD.xz_elements(D, g)
        assert len(set(codes.tolist())) == len(codes) and codes.min() == 1
        lo, hi = C.xz_bounds(D, "week")
        sel = np.arange(len(lev))
        a = corners[sel] + 0.5 * widths[sel, None]
        b = a + 1.2 * widths[sel, None]
        keep = (b <= 1.0).all(1)
        env = np.concatenate([lo + a[keep] * (hi - lo), lo + b[keep] * (hi - lo)], 1)
        got, st = oracle.xz2_index_batch(env, g=g) if D == 2 else oracle.xz3_index_batch(env, g=g)
        assert not st.any() and np.array_equal(got, codes[sel][keep])


# ---------------------------------------------------------------- the oracle under the checkers
@pytest.mark.parametrize("setting", C.Z_SETTINGS)
@pytest.mark.parametrize("with_prefix", [0, 1])
@pytest.mark.parametrize("D,bits", C.Z_RAW)
def test_oracle_zranges_definition(be, D, bits, with_prefix, setting):
    fails, _ = C.run_z_raw(be.zranges, D, bits, with_prefix, setting)
    assert not fails, fails[:3]


@pytest.mark.parametrize("budget", C.Z_BUDGETS)
@pytest.mark.parametrize("period,precision", C.Z3_USER + [(None, p) for p in C.Z2_USER])
def test_oracle_z_user_space_cover(be, period, precision, budget):
    fails, _ = C.run_z_user(be.z_user_ranges, be.z_user_index, period, precision, budget)
    assert not fails, fails[:3]


@pytest.mark.parametrize("budget", C.XZ_ELEMENT_BUDGETS)
@pytest.mark.parametrize("D,g,period", [(2, g, "week") for g in C.XZ2_ELEMENT_G] +
                         [(3, g, p) for g in C.XZ3_ELEMENT_G for p in C.PERIODS])
def test_oracle_xz_elements_definition(be, D, g, period, budget):
    fails, tally = C.run_xz_elements(be.xz_ranges, D, g, period, budget)
    assert not fails, fails[:3]
    assert tally["contained"] == 0   # ranges_definition.py, "contained" after the merge


XZ_END = [(2, g, "week") for g in C.XZ2_END_G] + [(3, g, p) for g in C.XZ3_END_G for p in C.XZ3_END_PERIODS]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("D,g,period", XZ_END)
def test_oracle_xz_end_to_end_cover(be, D, g, period, which):
    fails, tally = C.run_xz_end(be.xz_ranges, be.xz_index, D, g, period, C.xz_end_budgets(g)[which])
    assert not fails, fails[:3]
    assert tally["contained"] == 0   # ranges_definition.py, "contained" after the merge


def test_oracle_long_lists_are_long(oracle):
    """What the GPU parity tests of the long lists rely on.  Z2 with Z2SFC's 7 levels gives 30 ranges for
    this box at any budget, so the long Z2 lists are walked to the last level (maxRecurse past it), on
    the box's corners through Z2.zranges.  The budget of 5,000 fires (the list still grows at 20,000), so
    the walk holds at least 5,000 ranges before the merge (ZN.scala:214): past the 4,096 that are sorted
    in LDS and that the first phase's workspace holds.  Z3: the budget of 70,000 fires as well (the
    list still grows at 100,000), so that walk holds 70,000 ranges and queued cells when it stops, more
    than the 65,536 floor of the workspace caps; an unbounded walk of the same query passes through the
    same state and every queued cell still yields a range, so it is past that floor too."""
    zb = [C.z2_corners(oracle, C.BIG_BOX)]
    assert len(oracle.z2_ranges([C.BIG_BOX], max_ranges=5000)) == len(oracle.z2_ranges([C.BIG_BOX], max_ranges=20000))
    n5 = len(oracle.zranges(2, zb, 64, 5000, C.LARGE))
    n20 = len(oracle.zranges(2, zb, 64, 20000, C.LARGE))
    assert n5 < n20
    n70 = len(oracle.z3_ranges([C.BIG_BOX], [C.BIG_T], max_ranges=70000))
    assert n70 < len(oracle.z3_ranges([C.BIG_BOX], [C.BIG_T], max_ranges=100000))


# ---------------------------------------------------------------- the checkers against broken lists
def _mutations(ranges, drop, cut_upper, cut_lower, swap, split):
    """The six ways to break a list, as (name, list); indices chosen by the caller."""
    r = [tuple(x) for x in ranges]
    out = {}
    out["drop"] = r[:drop] + r[drop + 1:]
    out["upper-1"] = r[:cut_upper] + [(r[cut_upper][0], r[cut_upper][1] - 1, r[cut_upper][2])] + r[cut_upper + 1:]
    out["lower+1"] = r[:cut_lower] + [(r[cut_lower][0] + 1, r[cut_lower][1], r[cut_lower][2])] + r[cut_lower + 1:]
    s = list(r); s[swap], s[swap + 1] = s[swap + 1], s[swap]
    out["swap"] = s
    lo, hi, c = r[split]
    assert hi > lo
    mid = (lo + hi) // 2
    out["split"] = r[:split] + [(lo, mid, c), (mid + 1, hi, c)] + r[split + 1:]
    return out


def test_checker_sees_every_broken_z_list(oracle):
    D, bits = 2, 8
    qs = C.z_raw_queries(D, bits, 0, seed=11)
    wide_of = lambda rs: [k for k, r in enumerate(rs) if r[1] > r[0]]   # noqa: E731
    q = next(q for q in qs if len(wide_of(oracle.zranges(D, q, 64, None, 64))) >= 3)
    good = oracle.zranges(D, q, 64, None, 64)
    assert RD.check_z_list(good, q, D, bits, exact=True) == []
    wide = wide_of(good)
    m = _mutations(good, 1, wide[1], wide[2], 0, wide[0])
    # an exact list holds inside z only, so every z taken away is a z that must be covered
    assert RD.kinds(RD.check_z_list(m["drop"], q, D, bits)) == ["cover"]
    assert RD.kinds(RD.check_z_list(m["upper-1"], q, D, bits)) == ["cover"]
    assert RD.kinds(RD.check_z_list(m["lower+1"], q, D, bits)) == ["cover"]
    assert RD.kinds(RD.check_z_list(m["swap"], q, D, bits)) == ["order"]
    assert RD.kinds(RD.check_z_list(m["split"], q, D, bits)) == ["unmerged"]
    # a truncated walk leaves ranges with z outside the bounds; calling one `contained` is unsound
    loose = oracle.zranges(D, q, 64, 7, C.LARGE)
    assert RD.check_z_list(loose, q, D, bits) == []
    z, dims = RD.z_universe(D, bits)
    inside = RD.z_inside(dims, q, D)
    k = next(k for k, r in enumerate(loose) if not r[2] and not inside[r[0]:r[1] + 1].all())
    lie = loose[:k] + [(loose[k][0], loose[k][1], True)] + loose[k + 1:]
    assert RD.kinds(RD.check_z_list(lie, q, D, bits)) == ["soundness"]
    # and a range that leaves the universe, or an exact list with one z too many
    far = good[:-1] + [(good[-1][0], (1 << 16) + 5, good[-1][2])]
    assert "outside" in RD.kinds(RD.check_z_list(far, q, D, bits))
    assert "exact" in RD.kinds(RD.check_z_list(loose, q, D, bits, exact=True))


def test_checker_sees_every_broken_xz_list(oracle):
    D, g = 2, 5
    el = RD.xz_elements(D, g)
    qs = C.xz_element_queries(D, "week", seed=12)
    q = qs[0]   # holds a big window: contained and open ranges
    wn = C.xz_normalize(q, D)
    good = oracle.xz2_ranges(q, None, g=g)
    assert RD.check_xz_list(good, wn, D, g, elements=el) == []
    needed = set(el[3][RD.xz_meets(el[1], el[2], wn, D)].tolist())
    # ranges whose ends are codes that must be covered (an XZ list also holds codes that need not be)
    up = next(k for k, r in enumerate(good) if r[1] in needed and r[1] > r[0])
    low = next(k for k, r in enumerate(good) if r[0] in needed and r[1] > r[0])
    drop = next(k for k, r in enumerate(good) if r[0] in needed)
    m = _mutations(good, drop, up, low, 0, up)
    assert RD.kinds(RD.check_xz_list(m["drop"], wn, D, g, elements=el)) == ["cover"]
    assert RD.kinds(RD.check_xz_list(m["upper-1"], wn, D, g, elements=el)) == ["cover"]
    assert RD.kinds(RD.check_xz_list(m["lower+1"], wn, D, g, elements=el)) == ["cover"]
    assert RD.kinds(RD.check_xz_list(m["swap"], wn, D, g, elements=el)) == ["order"]
    assert RD.kinds(RD.check_xz_list(m["split"], wn, D, g, elements=el)) == ["unmerged"]
    codes = el[3]
    meets = RD.xz_meets(el[1], el[2], wn, D)
    k = next(k for k, r in enumerate(good) if not r[2] and (~meets[(codes >= r[0]) & (codes <= r[1])]).any())
    lie = good[:k] + [(good[k][0], good[k][1], True)] + good[k + 1:]
    assert RD.kinds(RD.check_xz_list(lie, wn, D, g, elements=el)) == ["soundness"]
    zero = [(0, good[0][1], good[0][2])] + good[1:]
    assert "outside" in RD.kinds(RD.check_xz_list(zero, wn, D, g, elements=el))


def test_check_cover_sees_every_broken_list(be):
    D, g = 2, 12
    env, qs = C.xz_end_case(D, g, "week", seed=13)
    codes = be.xz_index(D, g, "week", env)
    q = qs[0]
    hit = C.xz_end_hit(env, q, D)
    good = be.xz_ranges(D, g, "week", [q], 2000)[0]
    assert RD.check_cover(good, codes, hit) == []
    hs = set(codes[hit].tolist())
    up = next(k for k, r in enumerate(good) if r[1] in hs and r[1] > r[0])
    low = next(k for k, r in enumerate(good) if r[0] in hs and r[1] > r[0])
    m = _mutations(good, up, up, low, 0, up)
    assert RD.kinds(RD.check_cover(m["drop"], codes, hit)) == ["cover"]
    assert RD.kinds(RD.check_cover(m["upper-1"], codes, hit)) == ["cover"]
    assert RD.kinds(RD.check_cover(m["lower+1"], codes, hit)) == ["cover"]
    assert RD.kinds(RD.check_cover(m["swap"], codes, hit)) == ["order"]
    assert RD.kinds(RD.check_cover(m["split"], codes, hit)) == ["unmerged"]
    miss = set(codes[~hit].tolist())
    k = next(k for k, r in enumerate(good) if not r[2] and any(r[0] <= c <= r[1] for c in miss))
    lie = good[:k] + [(good[k][0], good[k][1], True)] + good[k + 1:]
    assert RD.kinds(RD.check_cover(lie, codes, hit)) == ["soundness"]


# ---------------------------------------------------------------- the header
def test_header_names_the_two_statuses():
    """include/geomesa_hip.h names both statuses with the values the kernels write and ranges.py reads."""
    import os
    import re
    from conftest import ROOT
    from geomesa_amd import ranges as R
    text = open(os.path.join(ROOT, "include", "geomesa_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (GM_QS_\w+) (\d+)", text)}
    assert vals == {"GM_QS_CAPACITY": 4, "GM_QS_TOO_MANY_BOUNDS": 5}
    assert set(vals.values()) <= set(R._QS_MSG)
