"""Times gm_histogram_attr and gm_minmax_attr over resident columns and writes profiles/attr_stats_probe.json.

In one process: the streaming copy (gm_device_copy) every rate is a share of, gm_z3_histogram at 1024 x 54 and
gm_frequency_attr over the same int64 column as yardsticks, torch's histc / aminmax over the float64 column;
gm_histogram_attr at length 1,000 over an int64 and a float64 column of Gaussian values (sigma 1,000) with
bounds that hold everything (no record: pass R and pass C, no host replay), with bounds of +-100 (a few dozen
records: the replay on the host), under a 1 % mask and with path = 2 (device atomics); gm_minmax_attr with and
without the HyperLogLog registers.  Device events around enough calls to pass half a second, after a warm-up
call.  No pass or fail threshold: the file records what was found.

    python tools/attr_stats_probe.py [--n 1000000000] [--out profiles/attr_stats_probe.json]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geomesa_amd import _lib  # noqa: E402
from geomesa_amd.stats import cms_hash_a  # noqa: E402
from bench import SEED, T2020, T2021  # noqa: E402

P = _lib.ptr
LENGTH = 1000


def timed(f, floor_s=0.5):
    """ms per call of f: one warm-up, then enough calls to pass floor_s in total."""
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(math.ceil(floor_s * 1000.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_stats_probe.json"))
    a = ap.parse_args()
    n = a.n
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    torch.manual_seed(SEED)
    f64 = torch.empty(n, dtype=torch.float64, device="cuda")
    step = 1 << 26
    for lo in range(0, n, step):
        k = min(step, n - lo)
        f64[lo:lo + k] = torch.randn(k, dtype=torch.float64, device="cuda") * 1000.0
    i64 = f64.to(torch.int64)
    words = (n + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device="cuda")
    bits = torch.arange(64, device="cuda", dtype=torch.int64)
    for lo in range(0, words, 1 << 20):
        k = min(1 << 20, words - lo)
        m = (torch.rand((k, 64), device="cuda") < 0.01).to(torch.int64)
        mask[lo:lo + k] = (m << bits).sum(1)
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = {"n": n, "device": torch.cuda.get_device_name(0), "length": LENGTH,
           "max_segments": _lib.GM_HIST_MAX_SEGMENTS, "lds_bins": _lib.GM_HIST_LDS_BINS, "rows": []}
    copy_gbs = [0.0]

    def note(name, ms, reps, bytes_per_row, **kw):
        gbs = bytes_per_row * n / ms / 1e6
        row = dict(name=name, ms=round(ms, 4), reps=reps, rows_per_s=round(n / ms * 1e3), gb_per_s=round(gbs, 1),
                   bytes_per_row=bytes_per_row, **kw)
        if copy_gbs[0]:
            row["share_of_copy"] = round(gbs / copy_gbs[0], 3)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        return ms

    scratch = torch.empty(n, dtype=torch.float64, device="cuda")
    ms, reps = timed(lambda: _lib.check(lib.gm_device_copy(h, P(scratch), P(f64), n * 8), "gm_device_copy"))
    copy_gbs[0] = 16 * n / ms / 1e6
    note("gm_device_copy", ms, reps, 16)
    del scratch

    # yardsticks: Z3Histogram over generated points, Frequency over the int64 column, torch
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    _lib.check(lib.gm_gen_points(h, SEED, n, 0, -180.0, 180.0, -90.0, 90.0, T2020, T2021, P(x), P(y), P(t)),
               "gm_gen_points")
    present = torch.zeros(54, dtype=torch.uint8, device="cuda")
    zc = torch.zeros((54, 1024), dtype=torch.int64, device="cuda")
    ms, reps = timed(lambda: _lib.check(lib.gm_z3_histogram(h, P(x), P(y), P(t), n, 1, 1024, 0, 2608, 54, P(present),
                                                            P(zc), P(tally)), "gm_z3_histogram"))
    note("gm_z3_histogram 1024 x 54", ms, reps, 24)
    del x, y, t
    cms = _lib.Cms(5, 400, 0, 1, 0, 0)
    for k, v in enumerate(cms_hash_a(5)):
        cms.hash_a[k] = v
    table = torch.zeros((1, 5, 400), dtype=torch.int64, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    icol = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, i64.data_ptr(), None, None, 0)
    fcol = _lib.AttrColumn(_lib.GM_ATTR_FLOAT64, 0, f64.data_ptr(), None, None, 0)
    ms, reps = timed(lambda: _lib.check(lib.gm_frequency_attr(h, ctypes.byref(icol), None, n, None, None, 0, 1, 1,
                                                              ctypes.byref(cms), P(table), P(size), P(tally)),
                                        "gm_frequency_attr"))
    note("gm_frequency_attr int64, precision 1", ms, reps, 8)
    ms, reps = timed(lambda: torch.histc(f64, bins=LENGTH, min=-6000.0, max=6000.0))
    note("torch.histc float64, 1000 bins", ms, reps, 8)
    ms, reps = timed(lambda: torch.aminmax(f64))
    note("torch.aminmax float64", ms, reps, 8)
    ms, reps = timed(lambda: torch.aminmax(i64))
    note("torch.aminmax int64", ms, reps, 8)
    tally.zero_()

    counts = torch.zeros(LENGTH, dtype=torch.int64, device="cuda")

    def hist(col, whole, bound, path=0, m=None):
        expansions = [0]

        def call():
            st = _lib.HistState(col.type, LENGTH, -bound, bound, float(-bound), float(bound))   # the bounds anew
            tally.zero_()
            _lib.check(lib.gm_histogram_attr(h, ctypes.byref(col), n, P(m), None, 0, 1, path, ctypes.byref(st), P(counts),
                                             P(tally)), "gm_histogram_attr")
            expansions[0] = int(tally[1])
        ms, reps = timed(call)
        return ms, reps, expansions[0]

    for name, col, whole in (("int64", icol, True), ("float64", fcol, False)):
        for label, bound, kw in (("bounds hold everything", 10_000_000, {}),
                                 ("bounds +-100", 100, {}),
                                 ("bounds hold everything, 1 % mask", 10_000_000, {"m": mask}),
                                 ("bounds hold everything, path 2", 10_000_000, {"path": 2}),
                                 ("bounds +-100, path 2", 100, {"path": 2})):
            ms, reps, exp = hist(col, whole, bound, **kw)
            bpr = 0.125 * 2 + 0.01 * 8 * 3 if "m" in kw else 3 * 8     # pass R reads the column twice, pass C once
            note("gm_histogram_attr %s, %s" % (name, label), ms, reps, bpr, expansions=exp)

    slots = torch.zeros(2, dtype=torch.int64, device="cuda")
    reg = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for name, col in (("int64", icol), ("float64", fcol)):
        for label, r in (("with registers", reg), ("without registers", None)):
            ms, reps = timed(lambda: _lib.check(lib.gm_minmax_attr(h, ctypes.byref(col), n, None, None, 0, P(slots), P(r),
                                                                   P(tally)), "gm_minmax_attr"))
            note("gm_minmax_attr %s, %s" % (name, label), ms, reps, 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
