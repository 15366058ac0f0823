"""gm_sort_keys' digit planner (csrc/gm_sort_plan.hpp, through tools/sort_plan_check.cpp) against its
restatement sort_plan.plan(); proof, from the restatement alone, that the plan grid of
test_gpu_sort_plan.py reaches every plan it claims; and proof that the run-geometry cases put their runs
where they claim.  Host-only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sort_plan as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/sort_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("sort_plan") / "sort_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "sort_plan_check.cpp")])

    def run(cases):
        text = "".join("0x%x 0x%x 0x%x 0x%x %d %d %d\n" % (oz, ob, az, ab, sharded, n, mode)
                       for oz, ob, az, ab, sharded, n, mode in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        plans = []
        for line in out.stdout.splitlines():
            v = [int(x) for x in line.split()]
            plans.append(S.Plan(bool(v[0]), v[1], v[2], tuple(v[3:7]), v[7], v[8], tuple(v[9:])))
        assert len(plans) == len(cases)
        return plans
    return run


def _or_and_of_layout(layout, sharded, rng):
    """An OR / AND pair whose varying bits are `layout`, over a random constant."""
    v = sum(1 << b for b in layout)
    c = int.from_bytes(rng.bytes(11), "little") & ~v
    if not sharded:
        c &= (1 << 80) - 1
    o, a = c | v, c
    return o & (2**64 - 1), o >> 64, a & (2**64 - 1), a >> 64


def _assert_same(cases, got):
    for c, g in zip(cases, got):
        assert g == S.plan(*c), "or_z %#x or_bs %#x and_z %#x and_bs %#x sharded %d n %d mode %d" % c


def test_planner_equals_restatement_on_the_grid(plan_check):
    rng = np.random.default_rng(1)
    cases = []
    for _, _, n, layout, sharded, _ in S.grid_cases():
        for mode in (0, 1):
            cases.append(_or_and_of_layout(layout, sharded, rng) + (int(sharded), n, mode))
    for name in S.GEOMETRY_NAMES:
        shard, bins, z, _, _ = S.geometry_keys(name)
        for mode in (0, 1):
            cases.append(S.or_and(shard, bins, z) + (int(shard is not None), len(z), mode))
    _assert_same(cases, plan_check(cases))


def test_planner_equals_restatement_on_random_draws(plan_check):
    """20,000 draws: n log-uniform in [1, 2^32), from 0 to 88 varying bits (sparse masks reach the plans
    whose varying bits run out), a random constant below them."""
    rng = np.random.default_rng(2)
    cases = []
    for _ in range(20000):
        sharded = bool(rng.integers(0, 2))
        width = 88 if sharded else 80
        nvar = int(rng.integers(0, width + 1)) if rng.integers(0, 3) else int(rng.integers(0, 6))
        layout = rng.choice(width, nvar, replace=False).tolist()
        n = min(2**32 - 1, max(1, int(2.0 ** rng.uniform(0, 32))))
        if rng.integers(0, 4) == 0:     # the sizes where ceil(log2 n) steps
            k = int(rng.integers(0, 32))
            n = max(1, min(2**32 - 1, 2**k + int(rng.integers(-1, 2))))
        cases.append(_or_and_of_layout(layout, sharded, rng) + (int(sharded), n, int(rng.integers(0, 2))))
    got = plan_check(cases)
    _assert_same(cases, got)
    # the draws are no monoculture: all four digit counts, prefix and byte plans, plans that ran out of bits
    assert {p.npre for p in got} == {0, 1, 2, 3, 4}
    assert any(p.prefix for p in got) and any(not p.prefix and p.lsd for p in got)
    assert any(p.lsd and p.pofs[p.npre - 1] < 0 for p in got)


def test_grid_sizes_are_the_smallest_of_each_plan():
    """n = 2^k for k = 1..19, then 2^19 + 1 and 2^22 + 1, the smallest sizes with three digits of 7 and of 8
    bits."""
    sizes = sorted({c[1] for c in S.PLAN_GRID})
    assert sizes == [2**k for k in range(1, 20)] + [2**19 + 1, 2**22 + 1]
    for n in (2**19 + 1, 2**22 + 1):
        a, b = S.layout_plan(S.ALL_BITS, True, n), S.layout_plan(S.ALL_BITS, True, n - 1)
        assert (a.npre, a.pw) != (b.npre, b.pw)


@pytest.mark.parametrize("what,holds,name", S.PLAN_PROPERTIES, ids=[p[0] for p in S.PLAN_PROPERTIES])
def test_grid_has_plan_property(what, holds, name):
    """Each property is shown by plan() on the layout of a named grid case."""
    rows = [c for c in S.PLAN_GRID if c[0] == name]
    assert len(rows) == 1, "the grid has no case %s" % name
    _, n, layout, shardings = rows[0]
    assert any(holds(S.layout_plan(layout, sharded, n), layout, sharded) for sharded in shardings), what


def test_grid_reaches_every_small_plan():
    """Every reachable (npre, pw) with npre <= 3 below 2^25 rows, as a prefix plan."""
    got = set()
    for name, n, layout, shardings in S.PLAN_GRID:
        for sharded in shardings:
            p = S.layout_plan(layout, sharded, n)
            if p.prefix:
                got.add((p.npre, p.pw))
    assert got == {(1, w) for w in range(1, 10)} | {(2, w) for w in range(5, 10)} | {(3, 7), (3, 8)}


def test_grid_has_binhi_and_long_runs():
    """The two properties that depend on the keys: binhi != 0, and a prefix plan with a run past 256 rows."""
    shard, bins, z, _ = S.grid_keys("k7_seam_sq5", True, "sampled")
    p = S.plan_of(shard, bins, z, 0)
    assert p.prefix and p.sq == 5 and p.binhi != 0 and p.binhi & 0x1f == 0
    for sharded in (False, True):
        shard, bins, z, _ = S.grid_keys("k12_long_runs", sharded, "sampled")
        p = S.plan_of(shard, bins, z, 0)
        pre = S.prefix_of(p, shard, bins, z)
        assert p.prefix and S.longest_run(pre) > S.RUN_MAX
        assert S.expected_last(p, pre) == len(p.lsd) + p.npre == 6


@pytest.mark.parametrize("case", S.grid_cases(), ids=[c[0] for c in S.grid_cases()])
def test_grid_keys_have_their_layout(case):
    """keys(): the exact OR ^ AND is the layout, constant z bits are not all 0, and the all-ones row of a
    "missed" case is outside the sample, whose plan then differs from the exact one (mode 0)."""
    _, name, n, layout, sharded, extremes = case
    shard, bins, z = S.keys(layout, n, sharded, np.random.default_rng(7), extremes)
    assert len(z) == n and (shard is None) == (not sharded)
    oz, ob, az, ab = S.or_and(shard, bins, z)
    assert (oz ^ az) | ((ob ^ ab) << 64) == sum(1 << b for b in layout)
    assert az != 0 or len([b for b in layout if b < 64]) > 60
    exact = S.plan_of(shard, bins, z, 0)
    assert exact == S.layout_plan(layout, sharded, n)._replace(binhi=exact.binhi)
    guess = S.plan_of(shard, bins, z, 0, S.sample_rows(n))
    differs = S.first_digits(guess) != S.first_digits(exact) or guess.sq != exact.sq
    assert differs == (extremes == "missed")


@pytest.mark.parametrize("name", S.GEOMETRY_NAMES)
def test_geometry_case_places_its_runs(name):
    """From the table order and prefix_of: the planned prefix is the case's field, and the runs of equal
    prefixes in sorted order are the case's runs, at the rows it claims."""
    _, field, sharded, _, claims, n = S.GEOMETRY[S.GEOMETRY_NAMES.index(name)]
    shard, bins, z, order, runs = S.geometry_keys(name)
    assert len(z) == n and (shard is not None) == sharded
    p = S.plan_of(shard, bins, z, 0)
    oz, ob, az, ab = S.or_and(shard, bins, z)
    assert (oz ^ az) | ((ob ^ ab) << 64) == sum(1 << b for b in field | S.LOW)
    if field == S.FIELD_Z:
        assert 2**14 < n <= 2**15 and (p.npre, p.pw, p.pofs[:2]) == (2, 7, (56, 49))
    elif field == S.FIELD_Z12:
        assert 2**12 < n <= 2**13 and (p.npre, p.pw, p.pofs[:2]) == (2, 6, (57, 51))
    else:
        assert 2**14 < n <= 2**15 and (p.npre, p.pw, p.pofs[:2], p.sq) == (2, 7, (71, 64), 9) and p.binhi != 0
    assert p.prefix and len(p.lsd) == 3
    pre = S.prefix_of(p, shard, bins, z)[order]
    assert np.all(pre[1:] >= pre[:-1])          # the prefix is the top of the key
    starts = np.flatnonzero(np.concatenate([[True], pre[1:] != pre[:-1]]))
    lengths = np.diff(np.concatenate([starts, [n]]))
    assert lengths.tolist() == list(runs)
    where = dict(zip(starts.tolist(), lengths.tolist()))
    for start, length in claims:
        assert where.get(start) == length, (start, length)
    longest = int(lengths.max())
    assert S.expected_last(p, pre) == (256 + 2 if longest <= S.RUN_MAX else len(p.lsd) + 2)
    if longest >= 150:                          # rows of the long run differ in the low bits, with ties
        s = int(starts[np.argmax(lengths)])
        low = z[order][s:s + longest] & 0xff
        assert 1 < len(np.unique(low)) < longest


def test_geometry_cases_cover_the_edges():
    """What the cases claim, in rows: T = 1792 and RUN_MAX = 256."""
    T, claims = S.T, {g[0]: (g[4], g[5]) for g in S.GEOMETRY}
    assert claims["run256_ends_at_T"][0] == [(T - 256, 256)]
    assert claims["run256_from_T_minus_1"][0] == [(T - 1, 256)]
    assert claims["run256_from_T_minus_255"][0] == [(T - 255, 256)]
    assert claims["run256_from_2T"][0] == [(2 * T, 256)]
    assert claims["seventy_runs_of_256"][1] == 10 * T == 17920 and len(claims["seventy_runs_of_256"][0]) == 70
    assert claims["run257_from_T_minus_1"][0] == [(T - 1, 257)]
    (s, length), = claims["run257_mid_tile"][0]
    assert length == 257 and s % T > 256 and (s + length) % T < T - 256 and s // T == (s + length) // T
    (s, length), = claims["run600_across_a_bound"][0]
    assert length == 600 and s < 2 * T < s + length
    for name, k in (("last_run_from_3T_minus_50", 3), ("last_run_from_10T_minus_50", 10)):
        ((s, length),), n = claims[name]
        assert (s, n, s + length) == (k * T - 50, k * T + 100, n)
    assert claims["n_is_10T_plus_1"][1] == 10 * T + 1
    assert claims["sharded_run256_from_T_minus_1"][0] == [(T - 1, 256)]
