"""The sizes at which the shared loops of the key kernels (pair_stream / row_stream, csrc/gm_stream.hpp) can
go wrong and n = 2 x block + 5 of the other tests does not reach.

With `block` the rows per workgroup of the kernel the aligned call reaches (the IndexCase blocks of
test_gpu_abi_contract.py):
  1              the odd-row tail alone (pair kernels: no pair at all)
  2, 3           one pair; one pair and the tail
  block - 1      the last pair of the block missing, and a tail
  block          exactly one full block: in k_z3_key_arrow_v the unguarded load branch with nothing behind it
  block + 1      a full block and the tail
  block + 2      a full block, then a block of one pair
  2 x block      full blocks only
Each size runs all-aligned (the pair kernel where the entry point has one) and with the first input column 8 B
in (the row kernel; the Arrow keys' pair-strided kernel), on guarded buffers, with the last row failing:
outputs, status and summary bit for bit the C oracle's.  The inverts have no status; their outputs and guards
are checked the same way.
"""
import numpy as np
import pytest

import test_gpu_abi_contract as A
import test_gpu_dispatch as D
from test_gpu_abi_contract import OK

pytestmark = pytest.mark.gpu

INVERTS = ("gm_z3_invert", "gm_z2_invert")


def sizes(block):
    return (1, 2, 3, block - 1, block, block + 1, block + 2, 2 * block)


@pytest.mark.parametrize("name", list(D.CASES) + list(INVERTS))
def test_stream_sizes(gpu, oracle, name):
    if name in INVERTS:
        for n in sizes(A._invert(name)[0]):
            for off in (None, {"z": D.MOVE}):
                A.run_invert(gpu, oracle, name, n, off)
        return
    case = D.CASES[name]()
    for n in sizes(case.block):
        cols = case.cols(np.random.default_rng(131 * len(name) + n), n)
        case.spoil(cols, [n - 1] * 3)
        exp, est = case.expect(oracle, cols)
        assert np.flatnonzero(est).tolist() == [n - 1], "the oracle fails exactly the last row"
        for moved in (None, ("in", 0)):
            what = (name, n, moved)
            rc, outs, st, sm = A.run_index(gpu, case, cols, n, True, True, {"moved": D.MOVE} if moved else None,
                                           {moved: "moved"} if moved else None)
            assert rc == OK and sm == (1, n - 1, int(est[n - 1])), (what, rc, sm)
            assert np.array_equal(st, est), (what, np.flatnonzero(st != est)[:8])
            for got, want in zip(outs, exp):
                assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
