"""The Frequency / Z3Frequency entry points in header, binding and library (no GPU calls)."""
import ctypes
import re

from geomesa_amd import _lib

SYMBOLS = ["gm_z3_frequency", "gm_frequency_attr", "gm_frequency_points", "gm_cms_estimate"]


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


def test_attr_type_values_match_header():
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(GM_ATTR_[A-Z0-9]+)\s+(\d+)", header()))
    assert defs["GM_ATTR_FLOAT32"] == 5 == _lib.GM_ATTR_FLOAT32
    assert len(set(defs.values())) == len(defs) == 5
    for k, v in defs.items():
        assert getattr(_lib, k) == v, k


def test_cms_struct_matches_header():
    m = re.search(r"#define\s+GM_CMS_MAX_DEPTH\s+(\d+)", header())
    assert int(m.group(1)) == _lib.GM_CMS_MAX_DEPTH == 32
    assert ctypes.sizeof(_lib.Cms) == 6 * 4 + 8 * 32
    assert _lib.Cms.hash_a.offset == 24 and _lib.Cms.path.offset == 20
