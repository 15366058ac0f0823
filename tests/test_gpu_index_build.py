"""The join index built on the device (GM_PARAM_INDEX_BUILD = 0, the default) against the host build
(= 1): the eight exported arrays must be byte-identical and the statistics equal, over the synthetic
counties (holes, MultiPolygons), the US-state shapefile fixture, polygons with more edges than the
build kernel's LDS band (its global-band path), several grid densities, and a row wider than one
256-cell segment.  The joins themselves are checked against the oracle by the other join tests,
which now run on device-built indexes.

The second half pins the paths where gm_pip_index_create_ex chooses between the builds, against the
oracle's join: a polygon with more rings than the device build takes (it declines, the host build
runs), sets whose envelope has no width or height (host build, every cell a slab-walk blob), sets
with nothing to match, and an imported index (the same finish as a built one)."""
import numpy as np
import pytest

from shapefile import us_states

pytestmark = pytest.mark.gpu


def _build(ps, cells, host):
    from geomesa_amd import _lib
    from geomesa_amd.join import PolygonIndex
    ctx = _lib.context()
    try:
        ctx.set_param(_lib.GM_PARAM_INDEX_BUILD, 1 if host else 0)
        ix = PolygonIndex(ps, ctx, cells)
    finally:
        ctx.set_param(_lib.GM_PARAM_INDEX_BUILD, 0)
    return ix


def _compare(ps, cells):
    d, h = _build(ps, cells, False), _build(ps, cells, True)
    assert d.stats() == h.stats()
    ld, ad = d.export_arrays()
    lh, ah = h.export_arrays()
    assert bytes(ld) == bytes(lh)
    names = ["rings", "slab_off", "slab_edges", "cell_word", "coarse_word", "compact", "list_ent", "blob"]
    for k, (x, y) in enumerate(zip(ad, ah)):
        assert x.numel() == y.numel(), names[k]
        assert bool((x == y).all()), names[k]
    return d


def _star_polys(nv, n, rng, holes=False):
    polys = []
    for j in range(n):
        cx, cy = -100 + 6 * j, 38.0
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        rad = 2.5 * (0.5 + 0.5 * rng.uniform(0, 1, nv))
        rings = [np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)]
        if holes:
            ha = np.sort(rng.uniform(0, 2 * np.pi, 40))
            rings.append(np.stack([cx + 0.3 * np.cos(ha), cy + 0.3 * np.sin(ha)], 1))
        polys.append([rings])
    return polys


@pytest.mark.parametrize("grid,cells", [((20, 10), 0), ((20, 10), 512), ((40, 20), 8192), ((80, 40), 0)])
def test_device_build_matches_host_counties(gpu, grid, cells):
    from geomesa_amd.join import synthetic_counties
    _compare(synthetic_counties(*grid), cells)


@pytest.mark.parametrize("cells", [0, 2048])
def test_device_build_matches_host_states(gpu, cells):
    _compare(us_states()[0], cells)


def test_device_build_matches_host_large_rings(gpu):
    """3,000-vertex rings (band beyond the LDS capacity) with holes, and a 4-polygon set whose grid
    rows are several 256-cell segments wide."""
    from geomesa_amd.join import PolygonSet
    rng = np.random.default_rng(4)
    _compare(PolygonSet.from_polygons(_star_polys(3000, 3, rng, holes=True)), 0)
    _compare(PolygonSet.from_polygons(_star_polys(200, 4, rng)), 200_000)


def test_device_build_join_equals_oracle(gpu, oracle):
    from geomesa_amd.join import PolygonSet, synthetic_points
    rng = np.random.default_rng(8)
    ps = PolygonSet.from_polygons(_star_polys(3000, 3, rng, holes=True))
    ix = _compare(ps, 0)
    px, py = synthetic_points(400_000, seed=3, box=(-104, 34, -82, 42))
    from test_gpu_scan_join_ranges import _sorted_pairs
    opt, opl = oracle.OraclePolySet(*ps.to_arrays()).join(px, py, nthreads=16)
    exp = np.stack([opt, opl.astype(np.int64)], 1)
    exp = exp[np.lexsort((exp[:, 1], exp[:, 0]))]
    assert np.array_equal(_sorted_pairs(*ix.join(px, py)), exp)


# ------------------------------------------------------------------ the paths that choose a build
def _oracle_pairs(oracle, ps, px, py, predicate):
    opt, opl = oracle.OraclePolySet(*ps.to_arrays()).join(px, py, predicate=predicate)
    exp = np.stack([opt, opl.astype(np.int64)], 1).reshape(-1, 2)
    return exp[np.lexsort((exp[:, 1], exp[:, 0]))]


def _join_pairs(ix, px, py, predicate):
    from test_gpu_scan_join_ranges import _sorted_pairs
    return _sorted_pairs(*ix.join(px, py, predicate=predicate)).reshape(-1, 2)


def _check_joins(oracle, ix, ps, px, py, expect=None):
    """ix.join equals the oracle's for both predicates; expect = (st_contains, st_intersects) pair counts."""
    for k, predicate in enumerate(("st_contains", "st_intersects")):
        exp = _oracle_pairs(oracle, ps, px, py, predicate)
        if expect is not None:
            assert len(exp) == expect[k], predicate
        assert np.array_equal(_join_pairs(ix, px, py, predicate), exp), predicate


def _lattice_polygon(n_holes):
    """Shell (0,0)-(34,18) with n_holes square holes of side 0.5 centred in the unit cells of a 32 x 16 lattice."""
    rings = [[(0, 0), (34, 0), (34, 18), (0, 18)]]
    for k in range(n_holes):
        x, y = 1.25 + k % 32, 1.25 + k // 32
        rings.append([(x, y), (x + 0.5, y), (x + 0.5, y + 0.5), (x, y + 0.5)])
    return [rings]


@pytest.mark.parametrize("cells", [0, 512])
@pytest.mark.parametrize("n_holes,pairs", [(512, 13534), (511, 13542)])
def test_ring_count_at_the_device_build_limit(gpu, oracle, n_holes, pairs, cells):
    """513 rings (2,565 vertices): the device build declines and the host build runs; 512 rings: still
    built on the device.  Either way the arrays equal the host build's and the join the oracle's."""
    from geomesa_amd.join import PolygonSet
    ps = PolygonSet.from_polygons([_lattice_polygon(n_holes)])
    assert ps.n_vertices == 5 * (n_holes + 1)
    rng = np.random.default_rng(1)
    px, py = rng.uniform(-1, 35, 20_000), rng.uniform(-1, 19, 20_000)
    _check_joins(oracle, _compare(ps, cells), ps, px, py, expect=(pairs, pairs))


@pytest.mark.parametrize("n_holes,line", [(511, "[gm_pip] device build:"), (512, "[gm_pip] build: classify")])
def test_ring_limit_picks_the_build(gpu, monkeypatch, capfd, n_holes, line):
    """With the device build asked for, 512 rings are built on the device and 513 by the host build:
    the GM_PIP_DEBUG line of the build that ran says which."""
    from geomesa_amd.join import PolygonSet
    ps = PolygonSet.from_polygons([_lattice_polygon(n_holes)])
    monkeypatch.setenv("GM_PIP_DEBUG", "1")
    capfd.readouterr()
    _build(ps, 512, False)
    lines = [l for l in capfd.readouterr().err.splitlines() if "build:" in l]
    assert len(lines) == 1 and lines[0].startswith(line), lines


def _on_and_around(rng, on_x, on_y, box):
    px = np.concatenate([rng.uniform(box[0], box[2], 1000), on_x])
    py = np.concatenate([rng.uniform(box[1], box[3], 1000), on_y])
    return px, py


@pytest.mark.parametrize("vertical", [False, True])
def test_degenerate_envelope_line(gpu, oracle, vertical):
    """A ring (0,0),(1,0),(2,0): zero height (or, turned, zero width).  Nothing is contained; the 50
    points on it intersect."""
    from geomesa_amd.join import PolygonSet
    rng = np.random.default_rng(2)
    t, z = rng.uniform(0, 2, 50), np.zeros(50)
    ring, box = [(0, 0), (1, 0), (2, 0)], (-1, -1, 3, 1)
    px, py = _on_and_around(rng, t, z, box)
    if vertical:
        ring, px, py = [(y, x) for x, y in ring], py, px
    ps = PolygonSet.from_polygons([[[ring]]])
    _check_joins(oracle, _compare(ps, 0), ps, px, py, expect=(0, 50))


def test_degenerate_envelope_point(gpu, oracle):
    """A ring of three equal points (1,1): only the point (1,1) intersects it."""
    from geomesa_amd.join import PolygonSet
    ps = PolygonSet.from_polygons([[[[(1, 1), (1, 1), (1, 1)]]]])
    ix = _compare(ps, 0)
    _check_joins(oracle, ix, ps, np.array([1.0, 2.0]), np.array([1.0, 1.0]), expect=(0, 1))
    rng = np.random.default_rng(3)
    px, py = _on_and_around(rng, np.ones(50), np.ones(50), (0, 0, 2, 2))
    _check_joins(oracle, ix, ps, px, py, expect=(0, 50))


@pytest.mark.parametrize("polys", [[], [[], [[]]]], ids=["no-polygons", "no-rings"])
def test_nothing_to_match(gpu, oracle, polys):
    """A set without polygons, and polygons without rings: no pairs, and the index still reports,
    exports and imports.  Both build settings give the same statistics, layout and array bytes (the
    first layout.bytes[k] of each exported tensor: a 0-byte array exports as one unwritten byte, which
    _compare would read)."""
    from geomesa_amd.join import PolygonIndex, PolygonSet
    ps = PolygonSet.from_polygons(polys)
    rng = np.random.default_rng(5)
    px, py = rng.uniform(-2, 2, 1000), rng.uniform(-2, 2, 1000)
    ix, host = _build(ps, 0, False), _build(ps, 0, True)
    assert ix.stats() == host.stats() and ix.stats()["entries"] == 0
    lay, arrs = ix.export_arrays()
    lay_h, arrs_h = host.export_arrays()
    assert bytes(lay) == bytes(lay_h)
    for k, (x, y) in enumerate(zip(arrs, arrs_h)):
        assert bool((x[:lay.bytes[k]] == y[:lay.bytes[k]]).all()), k
    im = PolygonIndex.from_arrays(lay, arrs, ix.ctx, ps)
    for index in (ix, host, im):
        _check_joins(oracle, index, ps, px, py, expect=(0, 0))


def test_empty_polygon_beside_a_real_one(gpu, oracle):
    from geomesa_amd.join import PolygonSet
    shell = [(0, 0), (4, 0), (4, 3), (0, 3)]
    ps = PolygonSet.from_polygons([[], [[shell]]])
    rng = np.random.default_rng(6)
    px = np.concatenate([rng.uniform(-1, 5, 1000), rng.uniform(0, 4, 50)])
    py = np.concatenate([rng.uniform(-1, 4, 1000), np.zeros(50)])
    for cells in (0, 512):
        _check_joins(oracle, _compare(ps, cells), ps, px, py)


def test_imported_index_joins_like_the_built_one(gpu):
    """Import runs the same finish (shortcut tables, list polygons) as the builds."""
    from geomesa_amd.join import PolygonIndex, synthetic_counties, synthetic_points
    ps = synthetic_counties(20, 10)
    ix = _build(ps, 512, False)
    lay, arrs = ix.export_arrays()
    im = PolygonIndex.from_arrays(lay, arrs, ix.ctx, ps)
    assert im.stats() == ix.stats()
    px, py = synthetic_points(100_000, seed=11)
    for predicate in ("st_contains", "st_intersects"):
        got = _join_pairs(im, px, py, predicate)
        assert len(got) > 0
        assert np.array_equal(got, _join_pairs(ix, px, py, predicate)), predicate
