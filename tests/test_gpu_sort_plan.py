"""gm_sort_keys over its plan space and its run geometry (sort_plan.py names the cases; test_sort_plan.py
proves on the host that they reach the plans and place the runs they claim).

Every call runs on guarded buffers, its four outputs must equal the stable table order
(table_scan_cases.table_order = np.lexsort) bit for bit, and GM_PARAM_SORT_LAST must name the path that
sort_plan.expected_last() derives from the keys: 256 + npre for prefix passes + local ranks, the number of
varying bytes for the byte passes (plus npre after a prefix attempt that met a run past 256 rows)."""
import numpy as np
import pytest

import sort_plan as S
import table_scan_cases as C
from abi_buffers import Guarded
from geomesa_amd import _lib

pytestmark = pytest.mark.gpu

T2020, T2021 = 1577836800000, 1609459200000


@pytest.fixture
def sort_mode(gpu):
    """Sets GM_PARAM_SORT_MODE on the shared context; mode 0 is back whatever the test does."""
    try:
        yield lambda mode: gpu.set_param(_lib.GM_PARAM_SORT_MODE, mode)
    finally:
        gpu.set_param(_lib.GM_PARAM_SORT_MODE, 0)


def P(g):
    return None if g is None else g.ptr


def sort_and_check(gpu, shard, bins, z, order, in_off=(0, 0, 0), out_off=(0, 0, 0)):
    """One gm_sort_keys call on guarded buffers (byte offsets from a 256-B boundary for shard, bin, z) whose
    outputs must be the table order; returns GM_PARAM_SORT_LAST."""
    n = len(z)
    ins = [None if shard is None else Guarded.of(shard, in_off[0]), Guarded.of(bins, in_off[1]), Guarded.of(z, in_off[2])]
    outs = [None if shard is None else Guarded(n, out_off[0]), Guarded(2 * n, out_off[1]), Guarded(8 * n, out_off[2]),
            Guarded(8 * n)]
    rc = gpu.lib.gm_sort_keys(gpu.handle, P(ins[0]), P(ins[1]), P(ins[2]), n, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]))
    assert gpu.lib.gm_ctx_sync(gpu.handle) == _lib.GM_OK
    assert rc == _lib.GM_OK, _lib.last_error()
    for k, g in enumerate(ins + outs):
        if g is not None:
            g.check("buffer %d" % k)
    assert np.array_equal(outs[3].read(np.int64), order)
    assert np.array_equal(outs[2].read(np.int64), z[order])
    assert np.array_equal(outs[1].read(np.int16), bins[order])
    if shard is not None:
        assert np.array_equal(outs[0].read(np.uint8), shard[order])
    return gpu.get_param(_lib.GM_PARAM_SORT_LAST)


def expected_last(shard, bins, z, mode):
    p = S.plan_of(shard, bins, z, mode)
    return S.expected_last(p, S.prefix_of(p, shard, bins, z)) if p.prefix else len(p.lsd)


GRID = S.grid_cases()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_plan_grid(gpu, sort_mode, case, mode):
    """One case per plan property (sort_plan.PLAN_PROPERTIES), each with the two extreme rows where the
    sample reads them and, from 2 * 65,536 rows, where it does not: then the sample's plan differs from the
    exact one and the digits are counted again."""
    _, name, n, layout, sharded, extremes = case
    shard, bins, z, order = S.grid_keys(name, sharded, extremes)
    exact = S.plan_of(shard, bins, z, mode)
    if extremes == "missed" and mode == 0:
        guess = S.plan_of(shard, bins, z, mode, S.sample_rows(n))
        assert S.first_digits(guess) != S.first_digits(exact) or guess.sq != exact.sq
    sort_mode(mode)
    last = sort_and_check(gpu, shard, bins, z, order)
    print("SORT_LAST %s mode %d: %d  (npre %d pw %d pofs %s sq %d binhi %d lsd %d)" % (
        case[0], mode, last, exact.npre, exact.pw, list(exact.pofs), exact.sq, exact.binhi, len(exact.lsd)))
    assert last == expected_last(shard, bins, z, mode)
    if mode == 1:
        assert last == len(exact.lsd)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", S.GEOMETRY_NAMES)
def test_run_geometry(gpu, sort_mode, name, mode):
    """Runs of equal prefixes at the edges of k_local_bounds' cuts (multiples of 1792 rows) and of
    k_sort_local's run limit (256 rows): runs of at most 256 rows are ranked locally (256 + 2), a longer one
    sends the call to the byte passes (3 + 2)."""
    shard, bins, z, order, runs = S.geometry_keys(name)
    sort_mode(mode)
    last = sort_and_check(gpu, shard, bins, z, order)
    print("SORT_LAST %s mode %d: %d  (longest run %d)" % (name, mode, last, max(runs)))
    if mode == 1:
        assert last == 3
    else:
        assert last == (256 + 2 if max(runs) <= S.RUN_MAX else 3 + 2)
        assert last == expected_last(shard, bins, z, 0)


_REAL = {}


def real_keys(n, sharded):
    """Z3 keys of uniform points over 2020, in table order (ascending), with 4 shards when sharded."""
    if (n, sharded) not in _REAL:
        from geomesa_amd.keyspace import Z3IndexKeySpace
        rng = np.random.default_rng(n)
        x = rng.uniform(-180, 180, n); y = rng.uniform(-90, 90, n); t = rng.integers(T2020, T2021, n)
        b, zz = Z3IndexKeySpace().sfc.index_keys(x, y, t)
        bins, z = b.cpu().numpy(), zz.cpu().numpy()
        shard = rng.integers(0, 4, n).astype(np.uint8) if sharded else None
        o = C.table_order(shard, bins, z)
        _REAL[(n, sharded)] = (None if shard is None else shard[o], bins[o], z[o])
    return _REAL[(n, sharded)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("kind", ["ascending", "descending_x3", "organ_pipe"])
def test_input_order(gpu, sort_mode, kind, sharded, mode):
    """Presorted input: in the high digit's pass every tile holds one or two digits, so the look-back walks
    over zero-count granules.  Descending with each key three times: stability reverses nothing inside a
    key.  Organ pipe: the evens ascending, then the odds descending."""
    n = 3 * 8192 + 5
    shard, bins, z = real_keys(n, sharded)
    if kind == "ascending":
        idx = np.arange(n)
    elif kind == "descending_x3":
        idx = np.repeat(np.arange(n)[::3], 3)[:n][::-1]
    else:
        idx = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)[::-1]])
    shard, bins, z = (None if shard is None else shard[idx].copy()), bins[idx].copy(), z[idx].copy()
    order = C.table_order(shard, bins, z)
    if kind == "ascending":
        assert np.array_equal(order, np.arange(n))
    sort_mode(mode)
    last = sort_and_check(gpu, shard, bins, z, order)
    print("SORT_LAST %s sharded %d mode %d: %d" % (kind, sharded, mode, last))
    assert last == expected_last(shard, bins, z, mode)
    if mode == 0:
        assert last == 256 + 2      # 14 prefix bits over 24,581 (8,194) uniform keys: no run near 256 rows


def random_keys(n, sharded, seed):
    rng = np.random.default_rng(seed)
    bins = rng.integers(-2**15, 2**15, n).astype(np.int16)
    z = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    shard = rng.integers(0, 256, n).astype(np.uint8) if sharded else None
    return shard, bins, z


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("n", [511, 512, 513, 8191, 8192, 8193, 16384, 65536, 65537, 131071, 131072])
def test_sizes_at_tile_edges(gpu, sort_mode, n, sharded, mode):
    """Full-range random keys at the edges of the count's 512-row chunks, the passes' 8192-row tiles and the
    sample's step (1 up to 131,071 rows, 2 from 131,072)."""
    shard, bins, z = random_keys(n, sharded, n + sharded)
    order = C.table_order(shard, bins, z)
    sort_mode(mode)
    last = sort_and_check(gpu, shard, bins, z, order)
    print("SORT_LAST n %d sharded %d mode %d: %d" % (n, sharded, mode, last))
    assert last == expected_last(shard, bins, z, mode)
    assert last == ((11 if sharded else 10) if mode == 1 else 256 + (1 if n <= 1024 else 2))


@pytest.mark.parametrize("n", [1, 5000])
def test_equal_keys_report_zero(gpu, sort_mode, n):
    shard, bins, z = np.full(n, 200, np.uint8), np.full(n, -3, np.int16), np.full(n, -(2**62) + 5, np.int64)
    sort_mode(0)
    assert sort_and_check(gpu, shard, bins, z, np.arange(n)) == 0


ALIGNMENTS = {
    # byte offsets of (shard, bin, z) from a 256-B boundary, inputs then outputs
    "in_z16_bin4_shard2": ((2, 4, 0), (0, 0, 0)),     # full-tile loads of the first pass, no 16-B count loads
    "in_bin2": ((0, 2, 0), (0, 0, 0)),                # neither
    "out_z8": ((0, 0, 0), (0, 0, 8)),
    "out_bin2": ((0, 0, 0), (0, 2, 0)),
    "out_shard1": ((0, 0, 0), (1, 0, 0)),
}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", sorted(ALIGNMENTS))
def test_column_alignment(gpu, sort_mode, which, mode):
    """Columns moved off the 16-B grid one at a time: the load paths are chosen per call from the input
    pointers (z 16 B, bin 4 B, shard 2 B for the passes' full-tile loads; all three 16 B for the count's
    wide loads), and the outputs may sit at any element boundary.  sort_and_check reads every guard."""
    n = 2 * 8192 + 5
    shard, bins, z = random_keys(n, True, 77)
    in_off, out_off = ALIGNMENTS[which]
    sort_mode(mode)
    last = sort_and_check(gpu, shard, bins, z, C.table_order(shard, bins, z), in_off, out_off)
    assert last == (11 if mode == 1 else 256 + 2)
