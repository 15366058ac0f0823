"""The references of the INTERSECTS-against-polygons full filter (tests/geom_poly_ref.py), the inputs its GPU
tests run on, the ABI of gm_scan_filter.polys and the host bucket builder -- all without a GPU.

  * intersects_exact (Fractions, every vertex both ways) and intersects_restated (the kernel's route) agree
    on the generated features and on a lattice set whose vertices sit on edges, whose edges overlap
    collinearly and cross at vertices;
  * a rectangle given as a polygon is geom_intersects_ref's answer for the same box;
  * the inputs hold, by the reference alone, the cases each step of the procedure decides;
  * tools/poly_query_check.cpp, built with the address and undefined-behaviour sanitizers and run directly,
    builds the buckets of every test query as the Python restatement does.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geom_intersects_ref as R
import geom_poly_ref as P
from test_gpu_geom_scan import KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREAL = ("polygon", "multipolygon")
# the queries whose exact (Fraction) scan over every generated feature is taken; the others share their code
EXACT_QUERIES = ("tri", "concave", "c65", "holed", "multi")


@pytest.mark.parametrize("name", EXACT_QUERIES)
@pytest.mark.parametrize("kind", KINDS)
def test_references_agree_on_the_generated_features(oracle, kind, name):
    rows, env, q = P.features(kind), P.envelopes(kind), P.queries()[name]
    exact = P.scan(rows, kind, q, env, P.intersects_exact)
    assert np.array_equal(exact, P.expected(kind, name)), np.nonzero(exact != P.expected(kind, name))[0][:10]


def lattice_case(kind, seed):
    """Features and queries on the 1/4 lattice of [-2, 2]^2: coincidences are the rule."""
    rng = np.random.default_rng(seed)

    def pt():
        return (float(rng.integers(-8, 9)) / 4, float(rng.integers(-8, 9)) / 4)

    def ring(c, r, m):
        th = np.sort(rng.uniform(0, 2 * np.pi, m))
        pts = [(round((c[0] + r * np.cos(t)) * 4) / 4, round((c[1] + r * np.sin(t)) * 4) / 4) for t in th]
        return pts + [pts[0]]

    def feat():
        if kind == "point":
            return pt()
        if kind in ("multipoint", "linestring"):
            return [pt() for _ in range(int(rng.integers(1, 6)))]
        if kind == "multilinestring":
            return [[pt() for _ in range(int(rng.integers(1, 5)))] for _ in range(int(rng.integers(1, 3)))]
        poly = [ring(pt(), float(rng.choice([0.5, 1.0, 1.75])), int(rng.integers(3, 7)))]
        if rng.random() < 0.4:
            poly.append(ring(poly[0][0], 0.25, 4))
        return poly if kind == "polygon" else [poly, [ring(pt(), 0.5, 4)]]
    rows = [feat() for _ in range(250)]
    sq = [(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0)]
    hole = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5)]
    qs = [P.Query([[sq]]), P.Query([[sq, hole]]),
          P.Query([[[(-2.0, -2.0), (0.0, -2.0), (-2.0, 0.0), (-2.0, -2.0)]], [[(0.25, 0.25), (1.75, 0.25), (1.75, 1.5),
                                                                                (1.0, 0.75), (0.25, 1.5), (0.25, 0.25)]]])]
    return rows, qs


@pytest.mark.parametrize("kind", KINDS)
def test_references_agree_on_the_lattice(oracle, kind):
    rows, qs = lattice_case(kind, 40 + KINDS.index(kind))
    for q in qs:
        exact = [P.intersects_exact(r, kind, q) for r in rows]
        restated = [P.intersects_restated(r, kind, q) for r in rows]
        assert exact == restated, [i for i, (a, b) in enumerate(zip(exact, restated)) if a != b][:10]
        assert 20 <= sum(exact) <= len(rows) - 20, sum(exact)     # both answers are well represented


@pytest.mark.parametrize("kind", KINDS)
def test_rectangle_polygon_is_the_box_filter(oracle, kind):
    rows = P.features(kind)
    for name, box in (("rect", P.RECT), ("world", P.WORLD)):
        assert np.array_equal(P.expected(kind, name), R.scan(rows, kind, [box])), (kind, name)


# ---------------------------------------------------------------- the inputs hold the cases
def counts_of(kind, name):
    rows, q = P.features(kind), P.queries()[name]
    dec = P.decided(kind, name)
    hit = np.array([d is not None for d in dec])
    env_hit = P.envelope_hit(P.envelopes(kind), q)
    miss = np.nonzero(env_hit & ~hit)[0]
    return {
        "envelope_only": len(miss),
        "match": int(hit.sum()),
        "g_in_q": sum(d == "g_in_q" for d in dec),
        "q_in_g": sum(d == "q_in_g" for d in dec),
        "in_query_hole": sum(P.wholly_in_hole_of_query(rows[i], kind, q) for i in miss),
        "part_in_row_hole": sum(P.part_wholly_in_hole_of_row(rows[i], kind, q) for i in miss),
    }


def required(kind, name):
    """The counts that must reach 50 for (kind, query); what is left out is impossible by the definition:
      envelope_only    nothing non-empty misses the world, and a point has no envelope-only miss against a
                       rectangle's own envelope;
      q_in_g, part_in_row_hole  only a polygon holds a part or has a hole, and nothing holds the world;
      in_query_hole    only `holed` has holes."""
    need = {"match", "g_in_q"}
    if name != "world" and not (kind == "point" and name == "rect"):
        need.add("envelope_only")
    if kind in AREAL and name != "world":
        need |= {"q_in_g", "part_in_row_hole"}
    if name == "holed":
        need.add("in_query_hole")
    return need


@pytest.mark.parametrize("name", list(P.queries()))
@pytest.mark.parametrize("kind", KINDS)
def test_inputs_hold_every_case(oracle, kind, name):
    got = counts_of(kind, name)
    for what in sorted(required(kind, name)):
        assert got[what] >= 50, (kind, name, what, got)


@pytest.mark.parametrize("name", list(P.queries()))
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "point"])
def test_inputs_reach_both_kernel_shapes(oracle, kind, name):
    """Each query's envelope survivors hold tuple runs of fewer than 64 segments and, but for the multipoint
    (its tuples are no run), of more than 128."""
    rows, q = P.features(kind), P.queries()[name]
    env_hit = P.envelope_hit(P.envelopes(kind), q)
    runs = [n for r, h in zip(rows, env_hit) if h for n in P.segment_counts(r, kind)]
    if kind == "multipoint":
        assert not runs
        return
    assert sum(n < 64 for n in runs) >= 10 and sum(n > 128 for n in runs) >= 3, (kind, name)


def test_queries_are_what_their_names_say():
    q = P.queries()
    tuples = {k: [len(r) for part in v.parts for r in part] for k, v in q.items()}
    assert tuples["tri"] == [4] and tuples["concave"] == [7] and tuples["rect"] == [5] and tuples["world"] == [5]
    assert [tuples[k] for k in ("c64", "c65", "c66", "c129", "c1000", "c2000")] == [[64], [65], [66], [129], [1000], [2000]]
    assert tuples["holed"] == [129, 5, 65] and len(q["multi"].parts) == 3
    assert all(r[0] == r[-1] for v in q.values() for part in v.parts for r in part)
    assert all(x * 4 == int(x * 4) and y * 4 == int(y * 4) for x, y in q["tri"].parts[0][0])
    # every central part within the disc the planted polygons hold, the small sites inside each of them
    for k, v in q.items():
        if k != "world":
            assert all(np.hypot(x, y) < 9.5 for x, y in v.parts[0][0]), k
    # c2000 is past the entries the kernel stages in LDS, every other query within them
    sizes = {k: sum(len(s) for s in P.buckets(v)[1]) for k, v in q.items()}
    assert sizes["c2000"] > P.LDS_ENTRIES and all(n <= P.LDS_ENTRIES for k, n in sizes.items() if k != "c2000"), sizes


# ---------------------------------------------------------------- the ABI
def test_scan_filter_has_polys_last_and_abi_version_2():
    from geomesa_amd import _lib
    text = open(_lib.HEADER).read()
    body = re.search(r"typedef struct \{([^{}]*)\} gm_scan_filter;", text).group(1)
    members = [re.search(r"(\w+)\s*;", line).group(1) for line in body.split("\n") if ";" in line]
    assert members == [n for n, _ in _lib.ScanFilter._fields_] and members[-1] == "polys"
    # every member is 8 bytes but the two int32, which share a word
    assert ctypes.sizeof(_lib.ScanFilter) == 8 * (len(members) - 1)
    assert _lib.ScanFilter.polys.offset == ctypes.sizeof(_lib.ScanFilter) - 8
    assert int(re.search(r"#define GM_ABI_VERSION (\d+)", text).group(1)) == 2 == _lib.GM_ABI_VERSION
    assert int(re.search(r"#define GM_POLY_QUERY_MAX_VERTICES (\d+)", text).group(1)) == _lib.GM_POLY_QUERY_MAX_VERTICES


# ---------------------------------------------------------------- the bucket builder
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def write_sets(path, sets):
    with open(path, "w") as f:
        f.write("%d\n" % len(sets))
        for parts in sets:
            f.write("%d\n" % len(parts))
            for part in parts:
                f.write("%d\n" % len(part))
                for ring in part:
                    f.write("%d %s\n" % (len(ring), " ".join("%s %s" % (float(x).hex(), float(y).hex()) for x, y in ring)))


def test_host_buckets_sanitized(tmp_path):
    """The program is compiled with -fsanitize=address,undefined and run as it is; nothing loaded into python
    is sanitised."""
    if CXX is None:
        pytest.fail("a host C++ compiler is needed to build tools/poly_query_check.cpp")
    exe = str(tmp_path / "poly_query_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "poly_query_check.cpp")])
    names = list(P.queries())
    tall = [[[(0.0, 0.0)] + [(float(i % 2), 10.0 * (1 - 2 * (i % 2))) for i in range(1, 40)] + [(0.0, 0.0)]]]   # zigzag: every edge in every slab
    flat = [[[(0.0, 1.0), (2.0, 1.0), (1.0, 1.0), (0.0, 1.0)]]]                      # no height: one slab
    bad = [[[[(0.0, 0.0), (1.0, 0.0), (0.0, 0.0)]]], [[[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]],
           [[[(0.0, 0.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, 0.0)]]], []]
    sets = [P.queries()[n].parts for n in names] + [tall, flat] + bad
    write_sets(str(tmp_path / "sets.txt"), sets)
    out = subprocess.run([exe, str(tmp_path / "sets.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr
    lines = out.stdout.split("\n")
    at = 0
    for parts in sets[:len(names) + 2]:
        q = P.Query(parts)
        ns, slabs = P.buckets(q)
        n_edges = sum(len(s) for part in q.segs for s in part)
        assert lines[at] == "set %d %d %d %d" % (len(parts), n_edges, ns, sum(len(s) for s in slabs)), lines[at]
        assert ns == 1 or sum(len(s) for s in slabs) <= 2 * n_edges
        for k in range(ns):
            assert [int(v) for v in lines[at + 1 + k].split()] == slabs[k], (at, k)
        # every edge appears in exactly the slabs its closed y-range overlaps: a run of slabs, once each
        seen = {}
        for k, s in enumerate(slabs):
            for e in s:
                seen.setdefault(e, []).append(k)
        assert sorted(seen) == list(range(n_edges)) and all(v == list(range(v[0], v[-1] + 1)) for v in seen.values())
        at += 1 + ns
        assert lines[at] == "parts"
        for p, part in enumerate(q.parts):
            got = [float.fromhex(v) for v in lines[at + 1 + p].split()]
            assert got == list(q.boxes[p]) + list(part[0][0])
        at += 1 + len(parts)
    texts = ["fewer than 4 tuples", "not closed", "NaN or infinite", "at least one query polygon part"]
    got =[l for l in lines[at:] if l]
    assert len(got) == 4 and all(g.startswith("invalid ") and t in g for g, t in zip(got, texts)), got
    # the zigzag's edges all span the range: the slab count fell to where entries <= 2 x edges
    assert P.buckets(P.Query(tall))[0] <= 2 and P.buckets(P.Query(flat))[0] == 1
