"""The built library exports the BIN scan's entry points and the binding's structs have the header's layout
(no GPU calls)."""
import ctypes

from geomesa_amd import _lib

BIN_SYMBOLS = ["gm_bin_track", "gm_bin_label", "gm_bin_points", "gm_bin_arrow", "gm_bin_sort"]


def test_library_exports_the_bin_entry_points():
    from geomesa_amd import build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in BIN_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_declares_them():
    for s in BIN_SYMBOLS:
        assert s in _lib.SIGNATURES
    header = open(_lib.HEADER).read()
    for s in BIN_SYMBOLS:
        assert "int %s(gm_ctx* ctx" % s in header


def test_struct_layouts():
    assert ctypes.sizeof(_lib.AttrColumn) == 40 and _lib.AttrColumn.values.offset == 8
    assert _lib.AttrColumn.validity_offset.offset == 32
    assert ctypes.sizeof(_lib.BinOpts) == 16 and _lib.BinOpts.lat_lon.offset == 4
    assert (_lib.GM_ATTR_INT32, _lib.GM_ATTR_INT64, _lib.GM_ATTR_FLOAT64, _lib.GM_ATTR_UTF8) == (1, 2, 3, 4)


def test_encoder_is_exported_and_decodes_on_the_host():
    """decode needs no GPU: BinaryOutputEncoder.decode over bytes."""
    import numpy as np
    import bin_ref as R
    import geomesa_amd
    from geomesa_amd.bin import BinEncoder, RECORD16, RECORD24
    assert geomesa_amd.BinEncoder is BinEncoder
    assert RECORD16.itemsize == 16 and RECORD24.itemsize == 24
    data = R.put(7, 1.5, -2.5, -1999, 99) + R.put(-8, 0.0, 3.0, 5000, -1)
    enc = BinEncoder.__new__(BinEncoder)
    enc.label = True
    got = enc.decode(np.frombuffer(data, np.uint8))
    assert got["track"].tolist() == [7, -8] and got["dtg"].tolist() == [-1000, 5000]
    assert got["lat"].tolist() == [1.5, 0.0] and got["lon"].tolist() == [-2.5, 3.0] and got["label"].tolist() == [99, -1]
