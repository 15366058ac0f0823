"""The two host forms of the density scan's line rendering agree (tests/density_lines_ref.py): the Scala
read line by line, and the vectorised form the GPU tests compare with; and every input class of the GPU
tests occurs, counted from the scalar form's trace alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import density_lines_ref as L
import density_ref as R


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def test_bresenham_lengths_of_gridsnaptest():
    """GridSnapTest.scala:79-97: lengths 9, 9, 9, 1, 9 -- the end pixel is left out."""
    g = L.ScalarLineGrid((0.0, 0.0, 10.0, 10.0), 10, 10)
    ends = [(0, 0, 9, 9), (0, 0, 0, 9), (0, 0, 9, 0), (0, 0, 0, 0), (9, 9, 0, 0)]
    lines = [list(g.bresenham_line(*e)) for e in ends]
    assert [len(b) for b in lines] == [9, 9, 9, 1, 9]
    for e, b in zip(ends, lines):
        assert b[0] == e[:2] and (len(b) == 1 or e[2:] not in b)


def test_fp_error_walk_is_not_the_rational_one():
    """(dX, dY) = (10, 3): the FP64 walk steps at x = 6, the rational one at x = 5; 48 slopes with
    dY <= dX <= 32 differ."""
    g = L.ScalarLineGrid((0.0, 0.0, 1.0, 1.0), 1, 1)
    fp, q = list(g.bresenham_line(0, 0, 10, 3)), L.rational_line(0, 0, 10, 3)
    first = [k for k in range(10) if fp[k] != q[k]][0]
    assert fp[5] == (5, 1) and q[5] == (5, 2) and fp[6] == (6, 2) and first == 5
    assert len(L.fp_differing_slopes(32)) == 48 and (10, 3) in L.fp_differing_slopes(32)


@functools.lru_cache(maxsize=None)
def scalar_case(k):
    name, env, w, h = L.LINE_ENVELOPES[k]
    rows = L.line_set(env, w, h, 5 + k)
    g, tally = L.render_scalar(env, w, h, rows)
    return env, w, h, rows, g, tally


@pytest.mark.parametrize("k", range(len(L.LINE_ENVELOPES)), ids=[e[0] for e in L.LINE_ENVELOPES])
def test_scalar_and_numpy_forms_agree(k):
    env, w, h, rows, g, tally = scalar_case(k)
    grid, t = L.render_lines_numpy(env, w, h, rows)
    assert same(grid, L.scalar_dense(g)) and np.array_equal(t, tally)
    rng = np.random.default_rng(k)
    wt = rng.integers(-1024, 1025, len(rows)) / 8.0
    ids = np.concatenate([rng.permutation(len(rows))[:len(rows) // 2], [3, 3, -1, len(rows)]])
    for sel in ({}, {"mask": rng.random(len(rows)) < 0.5}, {"ids": ids}):
        g2, tally2 = L.render_scalar(env, w, h, rows, wt, **sel)
        grid, t = L.render_lines_numpy(env, w, h, rows, wt, **sel)
        assert same(grid + 0.0, L.scalar_dense(g2) + 0.0) and np.array_equal(t, tally2)
    multi = L.as_multi(rows, k)
    g3, tally3 = L.render_scalar(env, w, h, multi)
    grid, t = L.render_lines_numpy(env, w, h, multi)
    assert same(grid, L.scalar_dense(g3)) and np.array_equal(t, tally3)
    assert same(grid, L.scalar_dense(g))          # parts render as the linestrings they are


CLASS_SETS = [k for k, e in enumerate(L.LINE_ENVELOPES) if min(e[2], e[3]) >= 8]   # 3 columns hold no octant walk


@pytest.mark.parametrize("k", CLASS_SETS, ids=[L.LINE_ENVELOPES[k][0] for k in CLASS_SETS])
def test_every_input_class_occurs(k):
    """At least 20 of each class, from the scalar reference's trace."""
    name, env, w, h = L.LINE_ENVELOPES[k]
    tr = scalar_case(k)[4].trace
    need = ["single_pixel", "first_suppressed", "final_pixel_unwritten", "clip_line", "clip_point", "clip_empty",
            "reenter_on_last_pixel", "below", "above", "skipped_part", "null", "vertices0", "vertices1"]
    need += ["octant%+d%+d%s" % (sx, sy, m) for sx in (1, -1) for sy in (1, -1) for m in "xy"]
    if w > 8:
        need.append("fp_walk_differs")
    if env[2] - env[0] < 360.0:
        need.append("empty")
    if env[2] - env[0] > 360.0:
        need += ["copies2", "copies3"]
    for c in need:
        assert tr[c] >= 20, (name, c, tr[c])
    if "fractional" in name:      # the -1 column: fl(xmin + 360 m) wraps to an ulp below xmin
        assert tr["neg_col"] >= 20, (name, tr["neg_col"])


def test_rational_clip_agrees_where_nothing_rounds():
    env = L.DYADIC_ENV
    rows = L.dyadic_clip_set(3)
    g, _ = L.render_scalar(env, 8, 8, rows)
    exact = [(a, b) for (a, b, ok) in g.clips if ok]
    assert len(exact) >= 20 and len(exact) == len(g.clips)
    kinds = {"empty": 0, "point": 0, "line": 0}
    for a, b in exact:
        fp, q = L.clip_fp(a, b, env), L.clip_exact(a, b, env)
        assert (fp is None) == (q is None)
        if fp is None:
            kinds["empty"] += 1
            continue
        assert tuple(tuple(Fraction(v) for v in p) for p in fp) == q
        kinds["point" if fp[0] == fp[1] else "line"] += 1
    assert kinds["empty"] >= 20 and kinds["line"] >= 20
    grid, t = L.render_lines_numpy(env, 8, 8, rows)
    assert same(grid, L.scalar_dense(g))


def test_density_iterator_linestrings():
    """DensityIteratorTest.scala:120-178 renders LineString and MultiLineString attributes; a line through
    the 15 feature positions adds every pixel of its walk once, its end pixel not at all."""
    lon, lat = R.density_iterator_points(1)
    env = (-1.0, 33.0, 6.0, 40.0)
    rows = [list(zip(lon.tolist(), lat.tolist()))]
    grid, t = L.render_lines_numpy(env, 500, 500, rows)
    g, _ = L.render_scalar(env, 500, 500, rows)
    assert same(grid, L.scalar_dense(g)) and t.tolist() == [0, 0, 0]
    i0, i1 = g.i(lon.min()), g.i(lon.max())
    assert grid.sum() >= i1 - i0 - 1 and set(np.nonzero(grid)[0].tolist()) == {285}
