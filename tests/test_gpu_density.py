"""GPU parity of the density scan (gm_density_points / gm_density_arrow / gm_density_sparse and
geomesa_amd.density.RenderingGrid) with tests/density_ref.render_numpy, which test_density_reference.py
holds equal to the Scala read line by line.

Unweighted grids and the tallies are compared bit for bit on every accumulation path (0 automatic,
1 workgroup-private LDS counters, 2 device atomics) and drain; weighted ones bit for bit where every partial
sum is exact (dyadic weights) and otherwise inside the bound that holds for any order of summation.
The kernel's vector-load block iteration covers 4096 rows (1024 threads x 2 pairs x 2 rows), so
n = 2 * 4096 + 5 crosses a block edge and ends on the odd last row."""
import ctypes
import functools
import math

import numpy as np
import pytest

import density_ref as R
from abi_buffers import Guarded, untouched

pytestmark = pytest.mark.gpu

N_BLOCKS = 2 * 4096 + 5
LDS_CELLS = 40704            # uint32 pixels of one LDS pass (gm_density.hip: DENS_LDS_BYTES / 4), FP64: half
MAX_PASSES = 8
GRIDS = [(1, 1), (3, 1000), (64, 64), (256, 256), (500, 500), (1024, 1024)]


def fits(w, h, weighted=False):
    rows = min(h, (LDS_CELLS // (2 if weighted else 1)) // w)
    return rows >= 1 and -(-h // rows) <= MAX_PASSES


def paths(w, h, weighted=False):
    return [0, 1, 2] if fits(w, h, weighted) else [0, 2]


def as_np(t):
    return t.detach().cpu().numpy()


def gpu_render(env, w, h, x, y, weight=None, mask=None, ids=None, path=0, workgroups=0, into=None):
    from geomesa_amd.density import RenderingGrid
    g = into if into is not None else RenderingGrid(env, w, h, path=path, workgroups=workgroups)
    g.render(x, y, weight, mask=mask, ids=ids)
    return as_np(g.grid), np.array(g.tally, np.int64), g


def same(got, want):
    """Bit for bit, -0.0 and 0.0 apart included."""
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def random_points(env, n, seed):
    """Points over the envelope and a margin of turns around it, a share outside in y."""
    rng = np.random.default_rng(seed)
    span = max(env[2] - env[0], 360.0)
    x = rng.uniform(env[0] - 2.2 * span, env[2] + 2.2 * span, n)
    inside = rng.random(n) < 0.6
    x[inside] = rng.uniform(env[0], env[2], int(inside.sum()))
    y = rng.uniform(env[1] - 0.05 * (env[3] - env[1]), env[3] + 0.05 * (env[3] - env[1]), n)
    return x, y


ENV_OF_GRID = {(1, 1): (-1.0, 33.0, 6.0, 40.0), (3, 1000): (-200.3, -90.0, 600.1, 90.0),
               (64, 64): (170.0, -10.0, 190.0, 10.0), (256, 256): (-180.0, -90.0, 180.0, 90.0),
               (500, 500): (-1.0, 33.0, 6.0, 40.0), (1024, 1024): (-180.0, -90.0, 180.0, 90.0)}


@functools.lru_cache(maxsize=None)
def block_case(w, h):
    env = ENV_OF_GRID[(w, h)]
    x, y = random_points(env, N_BLOCKS, 7 * w + h)
    grid, tally = R.render_numpy(env, w, h, x, y)
    assert grid.sum() >= 1000
    return env, x, y, grid, tally


@pytest.mark.parametrize("w,h,path", [(w, h, p) for (w, h) in GRIDS for p in paths(w, h)])
def test_grids_and_paths(gpu, w, h, path):
    """Every grid size on every path it can take: grid and tally equal the reference bit for bit."""
    env, x, y, want, tally = block_case(w, h)
    got, t, _ = gpu_render(env, w, h, x, y, path=path)
    assert same(got, want) and np.array_equal(t, tally)


@pytest.mark.parametrize("w,h,path", [(64, 64, 1), (256, 256, 0), (500, 500, 2)])
@pytest.mark.parametrize("moved", ["x", "y"])
def test_column_moved_by_8_bytes_takes_the_scalar_load_kernel(gpu, w, h, path, moved):
    import torch
    env, x, y, want, tally = block_case(w, h)
    cols = {}
    for name, a in (("x", x), ("y", y)):
        buf = torch.zeros(len(a) + 2, dtype=torch.float64, device="cuda")
        k = 0 if buf.data_ptr() % 16 == 0 else 1          # k: a 16-B aligned start
        if name == moved:
            k += 1
        buf[k:k + len(a)] = torch.from_numpy(a)
        cols[name] = buf[k:k + len(a)]
        assert (cols[name].data_ptr() % 16 == 8) == (name == moved)
    got, t, _ = gpu_render(env, w, h, cols["x"], cols["y"], path=path)
    assert same(got, want) and np.array_equal(t, tally)


@pytest.mark.parametrize("moved", [False, True], ids=["vector-loads", "scalar-loads"])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sel", ["none", "mask", "ids"])
def test_every_column_kernel(gpu, sel, weighted, path, moved):
    """Each instantiation gm_density_points can reach: selection x weights x accumulation x load width."""
    import torch
    env, x, y, _, _ = block_case(64, 64)
    n = len(x)
    rng = np.random.default_rng(17)
    wt = rng.integers(-1024, 1025, n) / 8.0 if weighted else None
    kw = {"none": {}, "mask": {"mask": rng.random(n) < 0.5}, "ids": {"ids": rng.permutation(n)[:n // 2]}}[sel]
    want, tally = R.render_numpy(env, 64, 64, x, y, wt, **kw)
    buf = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    k = (0 if buf.data_ptr() % 16 == 0 else 1) + int(moved)
    buf[k:k + n] = torch.from_numpy(x)
    got, t, _ = gpu_render(env, 64, 64, buf[k:k + n], y, wt, path=path, **kw)
    assert same(got, want) and np.array_equal(t, tally)


@functools.lru_cache(maxsize=None)
def edge_case(k):
    name, env, w, h = R.EDGE_ENVELOPES[k]
    ex, ey = R.edge_set(env, w, h)
    rx, ry = random_points(env, 300_001, 100 + k)
    x, y = np.concatenate([rx, ex]), np.concatenate([ry, ey])
    grid, tally = R.render_numpy(env, w, h, x, y)
    edge_only = R.render_numpy(env, w, h, ex, ey)
    return env, w, h, x, y, grid, tally, (ex, ey) + edge_only


@pytest.mark.parametrize("k,path", [(k, p) for k, e in enumerate(R.EDGE_ENVELOPES) for p in paths(e[2], e[3])],
                         ids=["%s-path%d" % (e[0], p) for e in R.EDGE_ENVELOPES for p in paths(e[2], e[3])])
def test_random_points_plus_the_edge_set(gpu, k, path):
    """300,001 random points plus the edge set (envelope and cell edges +-1 ulp, whole turns outside, the
    antimeridian and wide envelopes, the -1-column class, NaN / inf / |x| > 2^31 rows), and the edge set
    alone.  test_density_reference.py counts every class from the scalar reference."""
    env, w, h, x, y, want, tally, (ex, ey, ewant, etally) = edge_case(k)
    got, t, _ = gpu_render(env, w, h, x, y, path=path)
    assert same(got, want) and np.array_equal(t, tally)
    assert tally[0] >= 20 and ("fractional" not in R.EDGE_ENVELOPES[k][0] or tally[1] >= 20)
    got, t, _ = gpu_render(env, w, h, ex, ey, path=path)
    assert same(got, ewant) and np.array_equal(t, etally)


def test_cell_edges_follow_the_division(gpu):
    """Every cell edge of a 500-column grid whose dx is not dyadic: a reciprocal multiply would move >= 20 of them."""
    env, w = (-1.0, 33.0, 6.0, 40.0), 500
    dx = (np.float64(env[2]) - np.float64(env[0])) / w
    x = np.float64(env[0]) + np.arange(w + 1) * dx
    x = np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)])
    y = np.full(len(x), 35.0)
    want, tally = R.render_numpy(env, w, 1, x, y)
    for path in (1, 2):
        got, t, _ = gpu_render(env, w, 1, x, y, path=path)
        assert same(got, want) and np.array_equal(t, tally)


# ------------------------------------------------------------------ selection

@functools.lru_cache(maxsize=None)
def select_case():
    env, w, h = (-1.0, 33.0, 6.0, 40.0), 500, 500
    n = N_BLOCKS + 64
    x, y = random_points(env, n, 11)
    x[::7] = np.nan
    return env, w, h, n, x, y


def test_mask_from_strict_scan(gpu, oracle):
    """The mask words gm_strict_scan writes select the rows the oracle's scan keeps; garbage in the bits at
    and above n of the last word changes nothing."""
    import torch
    from geomesa_amd import _lib
    from geomesa_amd.curve import _dev_col
    env, w, h, n, x, y = select_case()
    n -= 27                                        # the last word is partly used
    x, y = x[:n], y[:n]
    bbox = (0.5, 34.0, 4.25, 39.0)
    dx, dy = _dev_col(x, torch.float64), _dev_col(y, torch.float64)
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    bb = (ctypes.c_double * 4)(*bbox)
    _lib.check(gpu.lib.gm_strict_scan(gpu.handle, _lib.ptr(dx), _lib.ptr(dy), None, n, bb, 0, 0, 0, _lib.ptr(words),
                                      None, 0, None), "gm_strict_scan")
    keep = oracle.strict_scan(x, y, None, bbox)
    assert 100 < keep.sum() < n - 100
    want, tally = R.render_numpy(env, w, h, x, y, mask=keep)
    for path in (0, 2):
        got, t, _ = gpu_render(env, w, h, dx, dy, mask=words, path=path)
        assert same(got, want) and np.array_equal(t, tally)
    assert n % 64 != 0
    words[-1] |= torch.tensor(-1 << (n % 64), dtype=torch.int64, device="cuda")
    got, t, _ = gpu_render(env, w, h, dx, dy, mask=words)
    assert same(got, want) and np.array_equal(t, tally)
    # a boolean mask (what filters.strict_scan / query_scan return) packs to the same words
    got, t, _ = gpu_render(env, w, h, dx, dy, mask=torch.from_numpy(keep))
    assert same(got, want) and np.array_equal(t, tally)
    # a mask over rows with unrenderable ones: the NaN rows it selects are counted
    rng = np.random.default_rng(2)
    m = rng.random(n) < 0.5
    want, tally = R.render_numpy(env, w, h, x, y, mask=m)
    got, t, _ = gpu_render(env, w, h, dx, dy, mask=m)
    assert same(got, want) and np.array_equal(t, tally) and tally[0] > 100


@pytest.mark.parametrize("order", ["ascending", "permuted", "duplicated", "out-of-range"])
@pytest.mark.parametrize("path", [0, 2])
def test_ids(gpu, order, path):
    env, w, h, n, x, y = select_case()
    rng = np.random.default_rng(4)
    ids = np.flatnonzero(rng.random(n) < 0.4).astype(np.int64)
    if order != "ascending":
        ids = rng.permutation(ids)
    if order == "duplicated":
        ids = np.concatenate([ids, ids[:1000], ids[:10], ids[:10]])
    if order == "out-of-range":
        ids = np.concatenate([ids[:500], [-1, n, 1 << 40, -(1 << 62), n + 1], ids[500:], [-1]])
    want, tally = R.render_numpy(env, w, h, x, y, ids=ids)
    got, t, _ = gpu_render(env, w, h, x, y, ids=ids, path=path)
    assert same(got, want) and np.array_equal(t, tally)
    assert tally[2] == (6 if order == "out-of-range" else 0)
    wt = rng.integers(-1024, 1025, n) / 8.0
    want, tally = R.render_numpy(env, w, h, x, y, wt, ids=ids)
    got, t, _ = gpu_render(env, w, h, x, y, wt, ids=ids, path=path)
    assert same(got, want) and np.array_equal(t, tally)


def test_empty_selections_and_no_rows(gpu):
    env, w, h, n, x, y = select_case()
    zero = np.zeros((h, w))
    for kw in ({"ids": np.zeros(0, np.int64)}, {"mask": np.zeros(n, bool)}):
        got, t, _ = gpu_render(env, w, h, x, y, **kw)
        assert same(got, zero) and t.tolist() == [0, 0, 0]
    got, t, _ = gpu_render(env, w, h, x[:0], y[:0])
    assert same(got, zero) and t.tolist() == [0, 0, 0]
    got, t, _ = gpu_render(env, w, h, x[:0], y[:0], ids=np.array([0, 5, -3]))   # no rows: every id is outside
    assert same(got, zero) and t.tolist() == [0, 0, 3]
    got, t, _ = gpu_render(env, w, h, x[1:2], y[1:2])
    assert same(got, R.render_numpy(env, w, h, x[1:2], y[1:2])[0])


# ------------------------------------------------------------------ weights

@pytest.mark.parametrize("w,h", [(64, 64), (256, 256), (500, 500)])
def test_dyadic_weights_are_bit_equal_on_both_paths(gpu, w, h):
    """Weights k / 8, |k| <= 1024: every partial sum is exact, so the order of the FP64 additions (LDS cells,
    flushes, device atomics) cannot show."""
    env, x, y, _, _ = block_case(w, h)
    rng = np.random.default_rng(9)
    wt = rng.integers(-1024, 1025, len(x)) / 8.0
    want, tally = R.render_numpy(env, w, h, x, y, wt)
    for path in paths(w, h, weighted=True):
        got, t, _ = gpu_render(env, w, h, x, y, wt, path=path)
        assert same(got, want) and np.array_equal(t, tally)
    m = rng.random(len(x)) < 0.5
    want, tally = R.render_numpy(env, w, h, x, y, wt, mask=m)
    got, t, _ = gpu_render(env, w, h, x, y, wt, mask=m)
    assert same(got, want) and np.array_equal(t, tally)


@pytest.mark.parametrize("w,h,path", [(8, 8, 1), (8, 8, 2), (64, 64, 1), (500, 500, 2)])
def test_random_weights_within_the_any_order_bound(gpu, w, h, path):
    """A pixel that receives m addends satisfies |got - fsum| <= (m - 1) 2^-53 sum|w| whatever the order
    of the additions (each of the m - 1 roundings is at most half an ulp of a partial sum, and no partial
    sum exceeds sum|w|): derived, not tuned.  One lost update moves a pixel by hundreds.  fsum's own
    rounding (half an ulp of the sum) is not in the bound; for m = 2 the two are the same double, and for
    same-sign addends got and fsum lie on one grid of ulps, (m - 1) / 2 of which the bound covers.  The
    largest error / bound seen is printed: 0.93 at 500 x 500 (a pixel of three addends, one ulp apart),
    below 0.25 elsewhere."""
    env = (-1.0, 33.0, 6.0, 40.0)
    rng = np.random.default_rng(13)
    n = 100_000
    x = rng.uniform(env[0], env[2], n)
    y = rng.uniform(env[1], env[3], n)
    wt = rng.uniform(-1000.0, 1000.0, n)
    pix, wts, _, _ = R.additions(env, w, h, x, y, wt)
    order = np.argsort(pix, kind="stable")
    pix, wts = pix[order], wts[order]
    starts = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
    ends = np.r_[starts[1:], len(pix)]
    got, t, _ = gpu_render(env, w, h, x, y, wt, path=path)
    got = got.reshape(-1)
    seen = np.zeros(w * h, bool)
    worst = 0.0
    for a, b in zip(starts, ends):
        m = b - a
        exact = math.fsum(wts[a:b].tolist())
        bound = (m - 1) * 2.0 ** -53 * float(np.abs(wts[a:b]).sum())
        err = abs(float(got[pix[a]]) - exact)
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else math.inf))
        assert err <= bound, (int(pix[a]), m, err, bound)
        seen[pix[a]] = True
    assert not got[~seen].any() and t.tolist() == [0, 0, 0]
    print("largest error / bound over %d pixels: %.3g" % (len(starts), worst))


def test_zero_weight_adds_nothing(gpu):
    env, w, h = (0.0, 0.0, 8.0, 8.0), 8, 8
    x = np.array([0.5, 1.5, 1.5, 2.5, 3.5])
    y = np.array([0.5, 0.5, 0.5, 0.5, 0.5])
    wt = np.array([0.0, 2.0, -2.0, -0.0, 4.0])
    for path in (1, 2):
        got, _, g = gpu_render(env, w, h, x, y, wt, path=path)
        assert got[0, :5].tolist() == [0.0, 0.0, 0.0, 4.0, 0.0]
        i, j, v = g.sparse()
        # the pixel of the zero weight and the pixel whose weights sum to zero are not reported
        assert as_np(i).tolist() == [3] and as_np(j).tolist() == [0] and as_np(v).tolist() == [4.0]


# ------------------------------------------------------------------ contention and drains

@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_contention(gpu, spread, weighted):
    """2^22 + 3 points in one pixel, or over it and its eight neighbours, with one workgroup and with the
    default launch, on both paths: counts are exact.  The LDS counters are 32 bits wide and flushed once,
    at the end; that they cannot wrap rests on the launch-size rule (launch_density gives a workgroup fewer
    than 2^31 additions), which a test of a few seconds cannot reach."""
    import torch
    n = (1 << 22) + 3
    env, w, h = (0.0, 0.0, 256.0, 256.0), 256, 256
    k = torch.arange(n, device="cuda")
    if spread:
        ci, cj = 99 + k % 3, 199 + (k // 3) % 3
    else:
        ci, cj = torch.full_like(k, 100), torch.full_like(k, 200)
    x = ci.to(torch.float64) + 0.5
    y = cj.to(torch.float64) + 0.25
    unit = 0.125 if weighted else 1.0
    wt = torch.full((n,), unit, dtype=torch.float64, device="cuda") if weighted else None
    want = np.zeros((h, w))
    np.add.at(want, (as_np(cj), as_np(ci)), unit)
    assert want.sum() == n * unit and np.count_nonzero(want) == (9 if spread else 1)
    for path, workgroups in ((1, 1), (1, 0), (1, 7), (2, 0)):
        got, t, _ = gpu_render(env, w, h, x, y, wt, path=path, workgroups=workgroups)
        assert same(got, want) and t.tolist() == [0, 0, 0], (path, workgroups)


def test_two_calls_equal_one_call_over_the_concatenation(gpu):
    env, x, y, want, tally = block_case(256, 256)
    cut = 4097
    _, _, g = gpu_render(env, 256, 256, x[:cut], y[:cut])
    got, t, _ = gpu_render(env, 256, 256, x[cut:], y[cut:], into=g)
    assert same(got, want) and np.array_equal(t, tally)
    g.clear()
    assert g.is_empty() and g.tally == [0, 0, 0]


# ------------------------------------------------------------------ Arrow

def arrow_points(x, y, f32, flip, nulls=None):
    import pyarrow as pa
    a, b = (x, y) if flip else (y, x)
    flat = np.stack([a, b], 1).reshape(-1).astype(np.float32 if f32 else np.float64)
    return pa.FixedSizeListArray.from_arrays(pa.array(flat), 2, mask=None if nulls is None else pa.array(nulls))


def arrow_multipoints(x, y, counts, f32, flip, nulls):
    import pyarrow as pa
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return pa.ListArray.from_arrays(pa.array(off), arrow_points(x[:off[-1]], y[:off[-1]], f32, flip), mask=pa.array(nulls))


@pytest.mark.parametrize("kind", ["point", "multipoint"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("flip", [False, True])
def test_arrow_columns(gpu, oracle, kind, f32, flip):
    """POINT and MULTIPOINT columns, Float8 and Float4, both axis orders, null slots and empty multipoints,
    unselected, with a mask and with ids, weighted and not, against the reference over oracle.arrow_rows."""
    from geomesa_amd.density import RenderingGrid
    env, w, h = (-1.0, 33.0, 6.0, 40.0), 100, 100
    rng = np.random.default_rng(21)
    n = 3001
    x, y = random_points(env, 6 * n, 22)
    x[::41] = np.nan
    nulls = rng.random(n) < 0.1
    if kind == "point":
        arr = arrow_points(x[:n], y[:n], f32, flip, nulls)
    else:
        counts = rng.integers(0, 6, n)
        counts[5] = 0
        arr = arrow_multipoints(x, y, counts, f32, flip, nulls)
    rows = oracle.arrow_rows(arr, kind, flip)
    assert sum(r is None for r in rows) > 100 and (kind == "point" or any(r == [] for r in rows))
    wt = rng.integers(-1024, 1025, n) / 8.0
    mask = rng.random(n) < 0.5
    ids = np.concatenate([rng.permutation(n)[:1500], [3, 3, -1, n]]).astype(np.int64)
    for weight in (None, wt):
        for sel in ({}, {"mask": mask}, {"ids": ids}):
            want, tally = R.render_rows(env, w, h, rows, weight, **sel)
            for path in (0, 2):
                g = RenderingGrid(env, w, h, path=path)
                g.render_arrow(arr, weight, kind=kind, flip_axis=flip, **sel)
                assert same(as_np(g.grid), want) and g.tally == tally.tolist(), (weight is None, list(sel), path)
    assert tally[0] > 50 and tally[2] == 2


def test_multipoint_slot_longer_than_a_thread_drain(gpu):
    """One slot of 2^19 + 7 points in one pixel (a thread drains the workgroup's counters after 2^19 additions of
    its own) beside ordinary slots: exact counts."""
    from geomesa_amd.density import RenderingGrid
    env, w, h = (0.0, 0.0, 8.0, 8.0), 8, 8
    big = (1 << 19) + 7
    x = np.concatenate([np.full(big, 2.5), [0.5, 1.5, 2.5]])
    y = np.concatenate([np.full(big, 3.5), [0.5, 0.5, 3.5]])
    arr = arrow_multipoints(x, y, np.array([big, 2, 1]), False, True, np.zeros(3, bool))
    g = RenderingGrid(env, w, h, path=1)
    g.render_arrow(arr, kind="multipoint", flip_axis=True)
    want = np.zeros((h, w))
    want[3, 2], want[0, 0], want[0, 1] = big + 1, 1, 1
    assert same(as_np(g.grid), want) and g.tally == [0, 0, 0]


# ------------------------------------------------------------------ sparse / decode

def test_sparse_and_decode(gpu):
    from geomesa_amd import _lib
    from geomesa_amd.density import GridSnap
    import torch
    env, x, y, want, _ = block_case(500, 500)
    rng = np.random.default_rng(31)
    wt = rng.integers(1, 64, len(x)) / 8.0
    want, _ = R.render_numpy(env, 500, 500, x, y, wt)
    _, _, g = gpu_render(env, 500, 500, x, y, wt)
    ii, jj = np.nonzero(want.T)                     # column i, then row j
    i, j, v = g.sparse()
    assert len(ii) > 1000
    assert as_np(i).tolist() == ii.tolist() and as_np(j).tolist() == jj.tolist()
    assert same(as_np(v), want[jj, ii])
    dx, dy, dv = g.decode()
    snap = GridSnap(env, 500, 500)
    ref = R.ScalarGrid(env, 500, 500)
    assert same(dx, snap.x(ii)) and same(dy, snap.y(jj)) and same(dv, want[jj, ii])
    assert dx[0] == ref.x_min + ref.dx / 2 + ref.dx * ii[0] and dy[0] == ref.y_min + ref.dy / 2 + ref.dy * jj[0]
    # capacity: nothing past cap is written, *n_cells reports the need; cap = 0 only counts
    n = ctypes.c_int64()
    cap = 100
    gi, gj, gv = Guarded(cap * 4), Guarded(cap * 4), Guarded(cap * 8)
    rc = gpu.lib.gm_density_sparse(gpu.handle, _lib.ptr(g.grid), 500, 500, cap, gi.ptr, gj.ptr, gv.ptr, ctypes.byref(n))
    assert rc == _lib.GM_E_CAPACITY and n.value == len(ii)
    assert gi.read(np.int32).tolist() == ii[:cap].tolist() and gj.read(np.int32).tolist() == jj[:cap].tolist()
    assert same(gv.read(np.float64), want[jj, ii][:cap])
    for b in (gi, gj, gv):
        b.check("gm_density_sparse")
    n = ctypes.c_int64(-1)
    rc = gpu.lib.gm_density_sparse(gpu.handle, _lib.ptr(g.grid), 500, 500, 0, None, None, None, ctypes.byref(n))
    assert rc == _lib.GM_E_CAPACITY and n.value == len(ii)
    empty = torch.zeros((3, 5), dtype=torch.float64, device="cuda")
    rc = gpu.lib.gm_density_sparse(gpu.handle, _lib.ptr(empty), 5, 3, 0, None, None, None, ctypes.byref(n))
    assert rc == _lib.GM_OK and n.value == 0
    rc = gpu.lib.gm_density_sparse(gpu.handle, _lib.ptr(empty), 5, 0, 0, None, None, None, ctypes.byref(n))
    assert rc == _lib.GM_E_INVALID


# ------------------------------------------------------------------ end to end

def test_density_iterator_features_through_a_table_query(gpu):
    """DensityIteratorTest.scala:93-108 and :182-191 through Z3Table.query(...) -> render(ids=...)."""
    from geomesa_amd.density import RenderingGrid
    from geomesa_amd.keyspace import during
    from geomesa_amd.table import Z3Table
    from test_host_planning import ms
    lon, lat = R.density_iterator_points(1)
    t = ms("2012-01-01T19:00:00.000Z") + 60000 * np.arange(15)
    tb = Z3Table.from_points(lon, lat, t)
    iv = [during(ms("2012-01-01T18:00:00.000Z"), ms("2012-01-01T23:00:00.000Z"))]
    ids, n, _ = tb.query([(-1, 33, 6, 40)], iv)
    assert n == 15
    g = RenderingGrid((-1.0, 33.0, 6.0, 40.0), 500, 500).render(lon, lat, ids=ids)
    dx, dy, dv = g.decode()
    assert len(dv) == 5 and dv.tolist() == [3.0] * 5 and dv.sum() == 15
    i, j, _ = g.sparse()
    assert as_np(i).tolist() == [142, 214, 285, 357, 428] and as_np(j).tolist() == [285] * 5
    ids, n, _ = tb.query([(0.5, 33, 1.5, 40)], iv)
    g = RenderingGrid((-180.0, -90.0, 180.0, 90.0), 500, 500).render(lon, lat, ids=ids)
    assert n == 3 and float(g.grid.sum()) == 3.0 and g.tally == [0, 0, 0]


def test_random_points_through_a_table_query(gpu, oracle):
    from geomesa_amd import filters as F
    from geomesa_amd.density import RenderingGrid
    from geomesa_amd.keyspace import Z3IndexKeySpace, during
    from geomesa_amd.table import Z3Table
    from test_host_planning import ms
    rng = np.random.default_rng(41)
    n = 100_003
    x, y = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    t = rng.integers(1577836800000, 1609459200000, n)
    ks = Z3IndexKeySpace()
    b, z = ks.sfc.index_keys(x, y, t)
    tb = Z3Table(b, z)
    bb, iv = [(-40, 10, 40, 70)], [during(ms("2020-03-01T00:00:00.000Z"), ms("2020-06-08T12:00:00.000Z"))]
    ids, nm, _ = tb.query(bb, iv)
    v = ks.get_index_values(bb, iv)
    keep = oracle.z3filter_scan(F.serialize_to_bytes(F.Z3Filter.from_values(v)), ks.bin_ranges(v), as_np(b), as_np(z))
    assert nm == keep.sum() > 500
    env = (-40.0, 10.0, 40.0, 70.0)
    want, tally = R.render_numpy(env, 256, 256, x, y, mask=keep)
    g = RenderingGrid(env, 256, 256).render(x, y, ids=ids)
    assert same(as_np(g.grid), want) and g.tally == tally.tolist()


# ------------------------------------------------------------------ invalid arguments

def grid_c(env=(-1.0, 33.0, 6.0, 40.0), w=16, h=16, workgroups=0, path=0):
    from geomesa_amd import _lib
    return _lib.DensityGrid(env[0], env[1], env[2], env[3], w, h, workgroups, path)


INVALID = {
    "null-ctx": dict(ctx=None),
    "null-grid-description": dict(g=None),
    "null-grid": dict(grid=None),
    "null-tally": dict(tally=None),
    "width-0": dict(g=dict(w=0)),
    "height-negative": dict(g=dict(h=-1)),
    "too-many-pixels": dict(g=dict(w=65536, h=32768)),
    "xmax-equals-xmin": dict(g=dict(env=(1.0, 33.0, 1.0, 40.0))),
    "ymax-below-ymin": dict(g=dict(env=(-1.0, 40.0, 6.0, 33.0))),
    "nan-bound": dict(g=dict(env=(float("nan"), 33.0, 6.0, 40.0))),
    "infinite-bound": dict(g=dict(env=(-1.0, 33.0, float("inf"), 40.0))),
    "bound-beyond-2^31": dict(g=dict(env=(-1.0, 33.0, 6.0, 3e9))),
    "wider-than-64-turns": dict(g=dict(env=(-12000.0, 33.0, 11040.5, 40.0))),
    "mask-and-ids": dict(both=True),
    "path-3": dict(g=dict(path=3)),
    "path-negative": dict(g=dict(path=-1)),
    "path-1-does-not-fit": dict(g=dict(w=1024, h=1024, path=1)),
    "workgroups-negative": dict(g=dict(workgroups=-1)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
@pytest.mark.parametrize("entry", ["points", "arrow"])
def test_invalid_arguments(gpu, case, entry):
    """Every GM_E_INVALID of the contract, on guarded buffers: the code, a gm_last_error text, and no write
    to grid, tally or anything else."""
    from geomesa_amd import _lib
    from geomesa_amd.arrow import GeomColumnC
    spec = INVALID[case]
    n = 100
    rng = np.random.default_rng(0)
    X, Y = Guarded.of(rng.uniform(-1, 6, n)), Guarded.of(rng.uniform(33, 40, n))
    YX = Guarded.of(rng.uniform(33, 40, 2 * n))
    M, I = Guarded.of(np.full(2, -1, np.int64)), Guarded.of(np.arange(n, dtype=np.int64))
    gkw = spec.get("g", {})
    G, T = Guarded(16 * 16 * 8), Guarded(24)
    g = None if gkw is None else grid_c(**gkw)
    ctx = spec.get("ctx", gpu.handle)
    grid = spec.get("grid", G.ptr)
    tally = spec.get("tally", T.ptr)
    both = bool(spec.get("both"))
    mask = M.ptr if both else None
    ids = I.ptr if both else None
    gp = ctypes.byref(g) if g is not None else None
    if entry == "points":
        rc = gpu.lib.gm_density_points(ctx, X.ptr, Y.ptr, None, n, mask, ids, n if both else 0, gp, grid, tally)
    else:
        col = GeomColumnC(0, 64, 0, 0, YX.addr, None, 0, (ctypes.c_void_p * 3)(None, None, None))
        rc = gpu.lib.gm_density_arrow(ctx, ctypes.byref(col), None, n, mask, ids, n if both else 0, gp, grid, tally)
    assert rc == _lib.GM_E_INVALID
    assert "gm_density_" + entry in _lib.last_error()
    gpu.sync()
    assert untouched(G.read()) and untouched(T.read())
    for b in (X, Y, YX, M, I, G, T):
        b.check(case)


def test_invalid_sources_and_alignment(gpu):
    from geomesa_amd import _lib
    from geomesa_amd.arrow import GeomColumnC
    n = 64
    X, Y = Guarded.of(np.zeros(n)), Guarded.of(np.zeros(n), offset=4)
    G, T = Guarded(16 * 16 * 8), Guarded(24)
    g = grid_c()
    lib, h = gpu.lib, gpu.handle
    assert lib.gm_density_points(h, X.ptr, Y.ptr, None, n, None, None, 0, ctypes.byref(g), G.ptr, T.ptr) == _lib.GM_E_INVALID
    assert lib.gm_density_points(h, None, X.ptr, None, n, None, None, 0, ctypes.byref(g), G.ptr, T.ptr) == _lib.GM_E_INVALID
    assert lib.gm_density_points(h, X.ptr, X.ptr, None, -1, None, None, 0, ctypes.byref(g), G.ptr, T.ptr) == _lib.GM_E_INVALID
    line = GeomColumnC(1, 64, 0, 0, X.addr, None, 0, (ctypes.c_void_p * 3)(X.addr, None, None))
    assert lib.gm_density_arrow(h, ctypes.byref(line), None, 4, None, None, 0, ctypes.byref(g), G.ptr, T.ptr) == _lib.GM_E_INVALID
    assert "GM_GEOM_POINT" in _lib.last_error()
    gpu.sync()
    assert untouched(G.read()) and untouched(T.read())
    # valid: 8-B aligned columns (the scalar-load kernel) on guarded buffers write grid and tally only
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 6, n + 1), rng.uniform(33, 40, n + 1)
    X, Y = Guarded.of(x, offset=8), Guarded.of(y, offset=16)
    G.write(np.zeros(16 * 16)); T.write(np.zeros(3, np.int64))
    assert lib.gm_density_points(h, X.ptr, Y.ptr, None, n + 1, None, None, 0, ctypes.byref(g), G.ptr, T.ptr) == _lib.GM_OK
    gpu.sync()
    want, tally = R.render_numpy((-1.0, 33.0, 6.0, 40.0), 16, 16, x, y)
    assert same(G.read(np.float64).reshape(16, 16), want) and T.read(np.int64).tolist() == tally.tolist()
    for b in (X, Y, G, T):
        b.check("valid call")


def test_two_abi_calls_of_gm_density_arrow_into_one_grid_add_up(gpu):
    """gm_density_arrow twice into one grid and tally, two different POINT batches of two blocks and an odd tail,
    nothing waited for in between: each batch alone equals its reference, and the shared grid equals the sum of
    both references."""
    from geomesa_amd import _lib
    from geomesa_amd.arrow import GeomColumnC
    env, px, n = ENV_OF_GRID[(256, 256)], 256, N_BLOCKS
    g = grid_c(env, px, px)
    pts = [random_points(env, n, 1500 + seed) for seed in (0, 1)]
    for seed, (x, y) in enumerate(pts):
        x[seed::41 + seed] = np.nan         # the tallies add up too
    refs = [R.render_numpy(env, px, px, x, y) for x, y in pts]
    assert all(r[0].sum() > 1000 and r[1].any() for r in refs) and not same(refs[0][0], refs[1][0])
    YX = [Guarded.of(np.stack([y, x], 1).reshape(-1)) for x, y in pts]
    cols = [GeomColumnC(0, 64, 0, 0, b.addr, None, 0, (ctypes.c_void_p * 3)(None, None, None)) for b in YX]

    def fresh():
        G, T = Guarded(px * px * 8), Guarded(24)
        G.write(np.zeros(px * px)); T.write(np.zeros(3, np.int64))
        return G, T

    def render(col, G, T):
        assert gpu.lib.gm_density_arrow(gpu.handle, ctypes.byref(col), None, n, None, None, 0, ctypes.byref(g), G.ptr,
                                        T.ptr) == _lib.GM_OK, _lib.last_error()

    for k, (col, (want, tally)) in enumerate(zip(cols, refs)):
        G, T = fresh()
        render(col, G, T)
        gpu.sync()
        assert same(G.read(np.float64).reshape(px, px), want) and T.read(np.int64).tolist() == tally.tolist(), k
    G, T = fresh()
    render(cols[0], G, T)
    render(cols[1], G, T)
    gpu.sync()
    assert same(G.read(np.float64).reshape(px, px), refs[0][0] + refs[1][0])
    assert T.read(np.int64).tolist() == (refs[0][1] + refs[1][1]).tolist()
    for buf in YX + [G, T]:
        buf.check("two calls")
