"""The row selection of the aggregating scans (density, BIN) as the Python layer prepares it:
curve._selection on host tensors, against numpy.packbits."""
import numpy as np
import pytest
import torch

from geomesa_amd.curve import _selection

CPU = torch.device("cpu")


def test_mask_and_ids_are_exclusive():
    with pytest.raises(ValueError):
        _selection(4, np.ones(4, bool), np.arange(4), CPU)


def test_no_selection():
    assert _selection(4, None, None, CPU) == (None, None, 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_bool_mask_packs_little_endian(n):
    m = np.random.default_rng(n).random(n) < 0.5
    m[-1] = True                                        # the last row's bit is in the last word
    want = np.packbits(np.pad(m, (0, -n % 64)), bitorder="little").view(np.int64)
    for given in (m, torch.from_numpy(m)):
        words, ids, n_ids = _selection(n, given, None, CPU)
        assert ids is None and n_ids == 0
        assert words.dtype == torch.int64 and words.is_contiguous()
        assert np.array_equal(words.numpy(), want)


def test_bool_mask_of_the_wrong_length():
    for k in (63, 65):
        with pytest.raises(ValueError):
            _selection(64, np.ones(k, bool), None, CPU)


def test_int64_words():
    w = torch.arange(3, dtype=torch.int64)
    words, _, _ = _selection(130, w, None, CPU)         # ceil(130 / 64) = 3
    assert words.data_ptr() == w.data_ptr()              # words pass through
    with pytest.raises(ValueError):
        _selection(130, w[:2], None, CPU)
    with pytest.raises(ValueError):
        _selection(130, w.to(torch.int32), None, CPU)    # neither bool nor int64


def test_ids():
    _, ids, n_ids = _selection(10, None, [3, 1, 3], CPU)
    assert n_ids == 3 and ids.dtype == torch.int64 and ids.tolist() == [3, 1, 3]
    _, ids, n_ids = _selection(10, None, np.empty(0, np.int32), CPU)
    assert n_ids == 0 and ids.dtype == torch.int64 and ids.numel() >= 1 and ids.data_ptr() != 0
