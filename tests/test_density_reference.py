"""The density scan's host side (no GPU): the two references of tests/density_ref.py held equal on every
input class the GPU tests use, and the reference project's known answers -- GridSnapTest and
DensityIteratorTest -- for the references and for geomesa_amd.density.GridSnap."""
import numpy as np
import pytest

import density_ref as R
from geomesa_amd.density import GridSnap


def both(env, w, h, x, y, weight=None):
    g = R.render_scalar(env, w, h, x, y, weight)
    dense, dropped = R.scalar_dense(g)
    grid, tally = R.render_numpy(env, w, h, x, y, weight)
    assert np.array_equal(grid, dense)
    assert tally[0] == g.trace["skipped"] and tally[1] == dropped and tally[2] == 0
    return g, grid, tally


# ------------------------------------------------------------------ the two references agree

@pytest.mark.parametrize("name,env,w,h", R.EDGE_ENVELOPES, ids=[e[0] for e in R.EDGE_ENVELOPES])
def test_references_agree_on_the_edge_set(name, env, w, h):
    x, y = R.edge_set(env, w, h)
    g, grid, tally = both(env, w, h, x, y)
    t = g.trace
    # each class occurs, counted from the scalar reference alone
    assert t["skipped"] >= 20                      # NaN, +-inf, |x| > 2^31 rows (x and y)
    assert t["row_out"] >= 20                      # one ulp below ymin, one above ymax
    assert t["below"] >= 20 and t["above"] >= 20   # whole turns outside, either side
    if env[2] - env[0] < 360.0:
        assert t["empty"] >= 20                    # translated past the other edge (never with a full turn)
    assert t["added"] >= 20 and t["clamped"] >= 20  # the xmax edge is clamped to the last column
    if env[2] - env[0] > 360.0:
        assert t["copies2"] >= 20 and t["copies3"] + t["copies1"] >= 20


def test_minus_one_column_class_occurs_in_wide_and_narrow_envelopes():
    """x = fl(xmin + 360 k) with a non-integer xmin: xt / xup lands below xmin in a share of the cases, and
    the reference adds to the map key (-1, j).  Counted from the scalar reference, in the edge set of both
    envelopes and, for the narrow one, over k = -400 .. 400."""
    for name, env, w, h in R.EDGE_ENVELOPES:
        if "fractional" not in name:
            continue
        x, y = R.edge_set(env, w, h)
        g, grid, tally = both(env, w, h, x, y)
        assert g.trace["neg_col"] >= 20, (name, g.trace)
        assert any(i == -1 for (i, _) in g.pixels)
        assert tally[1] == g.trace["neg_col"]
    name, env, w, h = R.EDGE_ENVELOPES[-1]
    k = np.arange(-400, 401)
    x = np.float64(env[0]) + 360.0 * k[k != 0]
    g, _, tally = both(env, w, h, x, np.full(len(x), (env[1] + env[3]) / 2))
    assert 0.10 * len(x) <= g.trace["neg_col"] == tally[1]


@pytest.mark.parametrize("name,env,w,h", R.EDGE_ENVELOPES, ids=[e[0] for e in R.EDGE_ENVELOPES])
def test_references_agree_on_random_points_and_weights(name, env, w, h):
    rng = np.random.default_rng(5)
    n = 4000
    span = env[2] - env[0]
    x = rng.uniform(env[0] - 2.5 * max(span, 360.0), env[2] + 2.5 * max(span, 360.0), n)
    y = rng.uniform(env[1] - 0.1 * (env[3] - env[1]), env[3] + 0.1 * (env[3] - env[1]), n)
    g, _, _ = both(env, w, h, x, y)
    assert g.trace["added"] >= 20 and g.trace["row_out"] >= 20
    wt = rng.integers(-1024, 1025, n) / 8.0     # dyadic: every partial sum is exact
    both(env, w, h, x, y, wt)


def test_cell_edges_take_the_division_not_a_reciprocal():
    """On the cell edges of a grid whose dx is not a power of two, floor(t / dx) and floor(t * (1 / dx))
    differ for some edges: the references (and the kernel) divide."""
    env, w = (-1.0, 33.0, 6.0, 40.0), 500
    dx = (np.float64(env[2]) - np.float64(env[0])) / w
    k = np.arange(w + 1)
    x = np.float64(env[0]) + k * dx
    t = x - np.float64(env[0])
    assert np.count_nonzero(np.floor(t / dx) != np.floor(t * (1.0 / dx))) >= 20
    g = R.render_scalar(env, w, 1, x, np.full(len(x), 35.0))
    cols = np.minimum(np.floor(t / dx).astype(np.int64), w - 1)
    want = np.bincount(cols, minlength=w).astype(np.float64)
    assert np.array_equal(R.scalar_dense(g)[0][0], want)


def test_selection_and_multipoint_rows():
    env, w, h = (-1.0, 33.0, 6.0, 40.0), 50, 50
    rng = np.random.default_rng(3)
    x = rng.uniform(-2, 7, 500)
    y = rng.uniform(32, 41, 500)
    ids = np.array([3, 3, 499, -1, 500, 1 << 40, 0])
    grid, tally = R.render_numpy(env, w, h, x, y, ids=ids)
    want, _ = R.render_numpy(env, w, h, x[[3, 3, 499, 0]], y[[3, 3, 499, 0]])
    assert np.array_equal(grid, want) and tally[2] == 3
    mask = rng.random(500) < 0.3
    grid, _ = R.render_numpy(env, w, h, x, y, mask=mask)
    assert np.array_equal(grid, R.render_numpy(env, w, h, x[mask], y[mask])[0])
    rows = [None, (1.0, 35.0), [], [(1.0, 35.0), (2.0, 36.0), (float("nan"), 1.0)]]
    grid, tally = R.render_rows(env, w, h, rows, weight=np.array([9.0, 2.0, 5.0, 0.5]))
    assert grid.sum() == 2.0 + 0.5 + 0.5 and list(tally) == [2, 0, 0]


# ------------------------------------------------------------------ GridSnapTest

def test_gridsnap_centres_and_snaps():
    """GridSnapTest.scala:29-55."""
    g = GridSnap((0.0, -4.0, 4.0, 0.0), 4, 4)
    assert [g.x(i) for i in range(4)] == [0.5, 1.5, 2.5, 3.5]
    assert [g.y(j) for j in range(4)] == [-3.5, -2.5, -1.5, -0.5]
    for (x, y), want in [((0, -4.0), (0.5, -3.5)), ((0.1, -3.9), (0.5, -3.5)), ((0.9, -3.1), (0.5, -3.5)),
                         ((1.0, -3.0), (1.5, -2.5)), ((1.1, -2.9), (1.5, -2.5)), ((1.9, -2.1), (1.5, -2.5)),
                         ((3.0, -1.0), (3.5, -0.5)), ((3.1, -0.9), (3.5, -0.5)), ((3.9, -0.1), (3.5, -0.5)),
                         ((4.0, 0.0), (3.5, -0.5))]:
        assert g.snap(x, y) == want
        s = R.ScalarGrid((0.0, -4.0, 4.0, 0.0), 4, 4)
        assert (g.x(s.i(x)), g.y(s.j(y))) == want


def test_gridsnap_min_max_and_out_of_bounds():
    """GridSnapTest.scala:57-77."""
    g = GridSnap((0.0, 0.0, 10.0, 10.0), 100, 10)
    s = R.ScalarGrid((0.0, 0.0, 10.0, 10.0), 100, 10)
    for snap in (g, s):
        assert snap.i(0.0) == 0 and snap.j(0.0) == 0
        assert snap.i(10.0) == 99 and snap.j(10.0) == 9
        assert snap.i(-1.0) == -1 and snap.j(-1.0) == -1
        assert snap.i(11.0) == -1 and snap.j(11.0) == -1
    # arrays in, arrays out
    assert g.i(np.array([0.0, 10.0, -1.0, 11.0, np.nan])).tolist() == [0, 99, -1, -1, 0]


def test_gridsnap_has_no_floating_point_errors():
    """GridSnapTest.scala:99-117: x(i(x(k))) == x(k) for a 100 x 100 grid over (0, 10)."""
    g = GridSnap((0.0, 0.0, 10.0, 10.0), 100, 100)
    s = R.ScalarGrid((0.0, 0.0, 10.0, 10.0), 100, 100)
    for k in range(100):
        assert g.x(g.i(g.x(k))) == g.x(k) and g.y(g.j(g.y(k))) == g.y(k)
        assert s.i(g.x(k)) == k and s.j(g.y(k)) == k
    k = np.arange(100)
    assert np.array_equal(g.i(g.x(k)), k) and np.array_equal(g.j(g.y(k)), k)


def test_gridsnap_to_int_saturates():
    g = GridSnap((0.0, 0.0, 5e-324, 1.0), 3, 1)    # dx underflows to 0: 0/0 -> NaN -> 0, t/0 -> inf -> clamp
    assert g.i(0.0) == 0 and g.i(5e-324) == 2
    s = R.ScalarGrid((0.0, 0.0, 5e-324, 1.0), 3, 1)
    assert s.i(0.0) == 0 and s.i(5e-324) == 2


# ------------------------------------------------------------------ DensityIteratorTest

@pytest.mark.parametrize("seed", range(200))
def test_density_iterator_points(seed):
    """DensityIteratorTest.scala:93-108: 15 points around 5 longitudes, envelope (-1, 33, 6, 40), 500 x 500
    -> 5 pixels of weight 3, sum 15: columns 142, 214, 285, 357, 428 of row 285."""
    lon, lat = R.density_iterator_points(seed)
    env = (-1.0, 33.0, 6.0, 40.0)
    g, grid, tally = both(env, 500, 500, lon, lat)
    assert grid.sum() == 15 and list(tally) == [0, 0, 0]
    jj, ii = np.nonzero(grid)
    assert jj.tolist() == [285] * 5 and ii.tolist() == [142, 214, 285, 357, 428]
    assert grid[jj, ii].tolist() == [3.0] * 5
    snap = GridSnap(env, 500, 500)
    assert snap.i(lon).tolist() == [142] * 3 + [214] * 3 + [285] * 3 + [357] * 3 + [428] * 3
    assert snap.j(37.0) == 285


def test_density_iterator_filter_smaller_than_the_envelope():
    """DensityIteratorTest.scala:182-191: world envelope, only the 3 points in lon [0.5, 1.5] -> sum 3."""
    lon, lat = R.density_iterator_points(0)
    keep = (lon >= 0.5) & (lon <= 1.5)
    assert keep.sum() == 3
    grid, tally = R.render_numpy((-180.0, -90.0, 180.0, 90.0), 500, 500, lon, lat, mask=keep)
    assert grid.sum() == 3 and list(tally) == [0, 0, 0]
    g = R.render_scalar((-180.0, -90.0, 180.0, 90.0), 500, 500, lon[keep], lat[keep])
    assert np.array_equal(R.scalar_dense(g)[0], grid)
