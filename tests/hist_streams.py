"""The stream-order cases of gm_minmax_attr and gm_histogram_attr, added to the case table of
tests/stream_order.py through its own add(): tests/test_gpu_streams.py then runs them with every other entry
(held stream on a caller's stream and on Context.owned, the shuffled table), and tests/test_abi.py finds every
new symbol covered.  Imported by tests/test_gpu_hist.py, which pytest collects before either of them.

The histogram case also calls the five host entries (gm_hist_index_of, gm_hist_bin_bounds, gm_hist_median,
gm_hist_copy_into, gm_hist_merge) while the stream is held: they take no context and must not touch it.
"""
import ctypes

import numpy as np

import hist_ref as R
import stream_order as SO
from geomesa_amd import _lib

N = 2 * 4096 + 5     # two blocks of pass R and an odd tail
LENGTH = 1000
HOST_ENTRIES = ("gm_hist_index_of", "gm_hist_bin_bounds", "gm_hist_median", "gm_hist_copy_into", "gm_hist_merge")


def _values(seed):
    return np.random.default_rng(2100 + seed).normal(0, 1000, N)


def _minmax_case(scale):
    def ins(seed):
        return {"v": _values(seed)}
    init = {"minmax": np.array(R.minmax_start("double"), np.int64), "registers": np.zeros(1024, np.int32),
            "tally": np.zeros(3, np.int64)}

    def call(lib, h, p, host):
        host["col"] = _lib.AttrColumn(_lib.GM_ATTR_FLOAT64, 0, p["v"].value, None, None, 0)
        return lib.gm_minmax_attr(h, ctypes.byref(host["col"]), N, None, None, 0, p["minmax"], p["registers"], p["tally"])

    def expect(O, d):
        slots = np.array(R.minmax_ref("double", d["v"].tolist()), np.int64)
        reg = np.array(R.hll_registers("double", d["v"].tolist()), np.int32)
        return {"dev": {"minmax": slots, "registers": reg, "tally": np.array([N, 0, 0], np.int64)}, "elems": slots}
    return SO.Case(ins, init, call, expect)


def _other():
    """A second histogram of another shape, for the host entries."""
    return R.RefHistogram("double", 17, (40.0, 900.0)).observe(_values(7)[:300].tolist())


def _hist_case(scale):
    def ins(seed):
        return {"v": _values(seed)}
    init = {"counts": np.zeros(LENGTH, np.int64), "tally": np.zeros(3, np.int64)}

    def call(lib, h, p, host):
        host["col"] = _lib.AttrColumn(_lib.GM_ATTR_FLOAT64, 0, p["v"].value, None, None, 0)
        st = host["state"] = _lib.HistState(_lib.GM_ATTR_FLOAT64, LENGTH, 0, 0, -100.0, 100.0)
        # the host half first, with the stream still held
        o = _other()
        so = _lib.HistState(_lib.GM_ATTR_FLOAT64, o.length, 0, 0, *o.bounds)
        oc = np.array(o.counts, np.int64)
        probe = np.array([-100.0, 0.0, 99.99, 100.0, 100.5], np.float64)
        idx = np.zeros(len(probe), np.int32)
        out, iv, fv = _lib.HistState(), ctypes.c_int64(), ctypes.c_double()
        to = np.zeros(LENGTH, np.int64)
        sa = _lib.HistState(_lib.GM_ATTR_FLOAT64, LENGTH, 0, 0, -100.0, 100.0)
        acc = np.zeros(LENGTH, np.int64)
        acc[3] = 9
        rcs = [lib.gm_hist_index_of(ctypes.byref(st), probe.ctypes.data, len(probe), idx.ctypes.data),
               lib.gm_hist_bin_bounds(ctypes.byref(st), 7, ctypes.byref(out)),
               lib.gm_hist_median(ctypes.byref(st), 7, ctypes.byref(iv), ctypes.byref(fv)),
               lib.gm_hist_copy_into(ctypes.byref(st), to.ctypes.data, ctypes.byref(so), oc.ctypes.data),
               lib.gm_hist_merge(ctypes.byref(sa), acc.ctypes.data, ctypes.byref(so), oc.ctypes.data)]
        host["host_rcs"] = np.array(rcs)
        host["index"], host["bin"], host["median"] = idx, np.array([out.flo, out.fhi]), fv
        host["copied"], host["merged"] = to, np.concatenate([[sa.length, sa.flo, sa.fhi], acc[:sa.length]])
        rc = lib.gm_histogram_attr(h, ctypes.byref(host["col"]), N, None, None, 0, 1, 0, ctypes.byref(st), p["counts"],
                                   p["tally"])
        host["lo"], host["hi"] = ctypes.c_double(st.flo), ctypes.c_double(st.fhi)
        return rc

    def expect(O, d):
        a = R.RefHistogram("double", LENGTH, (-100.0, 100.0)).observe(d["v"].tolist())
        assert a.expansions > 5
        counts = np.array(a.counts, np.int64)
        fresh = R.RefHistogram("double", LENGTH, (-100.0, 100.0))
        o = _other()
        to = [0] * LENGTH
        R.copy_into(fresh.bins, to, o.bins, o.counts)
        m = R.RefHistogram("double", LENGTH, (-100.0, 100.0))
        m.counts[3] = 9
        m += o
        host = {"host_rcs": np.zeros(5, np.int64),
                "index": np.array([fresh.bins.index_of(x) for x in (-100.0, 0.0, 99.99, 100.0, 100.5)], np.int32),
                "bin": np.array(fresh.bins.bin_bounds(7)), "median": fresh.bins.median_value(7),
                "copied": np.array(to, np.int64), "merged": np.concatenate([[m.length, *m.bounds], m.counts]),
                "lo": a.bounds[0], "hi": a.bounds[1]}
        return {"dev": {"counts": counts, "tally": np.array([N, a.expansions, 0], np.int64)}, "host": host,
                "elems": counts, "counters": True}
    return SO.Case(ins, init, call, expect)


if "gm_minmax_attr" not in SO.TABLE:
    # include/geomesa_hip.h: gm_minmax_attr "Stream-ordered, no readback"; gm_histogram_attr "Synchronises the
    # context stream: it reads the record count back"
    SO.add("gm_minmax_attr", "gm_minmax_attr", False, _minmax_case)
    SO.add("gm_histogram_attr", ("gm_histogram_attr",) + HOST_ENTRIES, True, _hist_case)
