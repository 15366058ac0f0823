"""The Histogram / MinMax entry points in header, binding and library (no GPU calls)."""
import ctypes
import re

from geomesa_amd import _lib

SYMBOLS = ["gm_minmax_attr", "gm_histogram_attr", "gm_hist_index_of", "gm_hist_bin_bounds", "gm_hist_median",
           "gm_hist_copy_into", "gm_hist_merge"]


def header():
    return open(_lib.HEADER).read()


def test_signatures_present():
    from geomesa_amd import build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    # one ctypes argument per declared parameter
    for s in SYMBOLS:
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, code, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s


def test_hist_state_matches_header():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*gm_hist_state;", code).group(1)
    fields = [f for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert fields == [f[0] for f in _lib.HistState._fields_] == ["type", "length", "lo", "hi", "flo", "fhi"]
    assert ctypes.sizeof(_lib.HistState) == 40
    assert _lib.HistState.lo.offset == 8 and _lib.HistState.flo.offset == 24


def test_limits_match_header():
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(GM_HIST_[A-Z_]+)\s+(\d+)", header()))
    assert defs == {"GM_HIST_MAX_SEGMENTS": _lib.GM_HIST_MAX_SEGMENTS, "GM_HIST_LDS_BINS": _lib.GM_HIST_LDS_BINS}
    assert _lib.GM_HIST_MAX_SEGMENTS == 256 and _lib.GM_HIST_LDS_BINS == 16384


def test_host_entries_need_no_context():
    """The host half answers without a GPU or a context."""
    from geomesa_amd import build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    st = _lib.HistState(_lib.GM_ATTR_INT64, 10, 0, 99, 0.0, 0.0)
    v = (ctypes.c_int64 * 4)(0, 55, 99, 100)
    out = (ctypes.c_int32 * 4)()
    assert lib.gm_hist_index_of(ctypes.byref(st), v, ctypes.c_int64(4), out) == _lib.GM_OK
    assert list(out) == [0, 5, 9, -1]
