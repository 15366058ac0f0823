"""Times the Frequency / Z3Frequency scans over resident generated points and writes profiles/frequency_probe.json.

In one process: the streaming copy (gm_device_copy) every rate is a share of, and gm_z3_histogram at 1024 x 54
(one LDS increment per row) as yardsticks; gm_z3_frequency at the default sketch shape (depth 5, width 400)
over points of one week into a one-bin window (one LDS pass) and over points of a year into 54 week bins (four
passes); gm_frequency_attr over an int64 column without a dtg, with precision 1 and 1000 (a 64-bit division per
row), and under a 1 % mask; the same scans with path = 2 (device atomics); and a sweep of the window that gives
1, 2, 4 and 8 LDS passes, from which the file derives the time per pass and the number of passes at which the
device-atomic kernel catches up -- what FREQ_MAX_PASSES (gm_freq.hip) is set from.  Device events around enough
calls to pass half a second, after a warm-up call.

    python tools/frequency_probe.py [--n 1000000000] [--out profiles/frequency_probe.json]
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

ENV = (-180.0, -90.0, 180.0, 90.0)
WK = 604800000
P = _lib.ptr


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frequency_probe.json"))
    a = ap.parse_args()
    n = a.n
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")     # a year of dates: week bins 2608 .. 2661
    t1 = torch.empty(n, dtype=torch.int64, device="cuda")    # one week of dates: bin 2610
    _lib.check(lib.gm_gen_points(h, SEED, n, 0, ENV[0], ENV[2], ENV[1], ENV[3], T2020, T2021, P(x), P(y), P(t)),
               "gm_gen_points")
    _lib.check(lib.gm_gen_points(h, SEED + 1, n, 0, ENV[0], ENV[2], ENV[1], ENV[3], 2610 * WK, 2611 * WK, None, None,
                                 P(t1)), "gm_gen_points")
    words = (n + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device="cuda")
    bits = torch.arange(64, device="cuda", dtype=torch.int64)
    step = 1 << 20
    for lo in range(0, words, step):
        k = min(step, words - lo)
        m = (torch.rand((k, 64), device="cuda") < 0.01).to(torch.int64)
        mask[lo:lo + k] = (m << bits).sum(1)
    scratch = torch.empty(n, dtype=torch.float64, device="cuda")
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = {"n": n, "device": torch.cuda.get_device_name(0), "depth": 5, "width": 400, "rows": []}
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

    ms, reps = timed(lambda: _lib.check(lib.gm_device_copy(h, P(scratch), P(x), n * 8), "gm_device_copy"))
    copy_gbs[0] = 16 * n / ms / 1e6
    note("gm_device_copy", ms, reps, 16)
    del scratch

    present = torch.zeros(54, dtype=torch.uint8, device="cuda")
    counts = torch.zeros((54, 1024), dtype=torch.int64, device="cuda")
    ms, reps = timed(lambda: _lib.check(lib.gm_z3_histogram(h, P(x), P(y), P(t), n, 1, 1024, 0, 2608, 54, P(present),
                                                            P(counts), P(tally)), "gm_z3_histogram"))
    hist_ms = note("gm_z3_histogram 1024 x 54 (one increment per row)", ms, reps, 24)
    tally.zero_()

    def sketch(lo, nb, path=0):
        c = _lib.Cms(5, 400, lo, nb, 0, path)
        for i, v in enumerate(cms_hash_a(5)):
            c.hash_a[i] = v
        table = torch.zeros((nb, 5, 400), dtype=torch.int64, device="cuda")
        size = torch.zeros(nb, dtype=torch.int64, device="cuda")
        return c, table, size

    def z3(tt, lo, nb, path=0, m=None):
        c, table, size = sketch(lo, nb, path)
        return timed(lambda: _lib.check(lib.gm_z3_frequency(h, P(x), P(y), P(tt), n, P(m), None, 0, 1, 25,
                                                            ctypes.byref(c), P(table), P(size), P(tally)),
                                        "gm_z3_frequency"))

    def attr(precision, path=0, m=None):
        c, table, size = sketch(0, 1, path)
        col = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, t.data_ptr(), None, None, 0)
        return timed(lambda: _lib.check(lib.gm_frequency_attr(h, ctypes.byref(col), None, n, P(m), None, 0, 1, precision,
                                                              ctypes.byref(c), P(table), P(size), P(tally)),
                                        "gm_frequency_attr"))

    ms, reps = z3(t1, 2610, 1)
    one_ms = note("gm_z3_frequency, 1 week bin (one LDS pass)", ms, reps, 24, passes=1, path="LDS")
    ms, reps = z3(t, 2608, 54)
    note("gm_z3_frequency, 54 week bins (four LDS passes)", ms, reps, 4 * 24, passes=4, path="LDS")
    ms, reps = z3(t1, 2610, 1, m=mask)
    note("gm_z3_frequency, 1 week bin, 1 % mask", ms, reps, 0.125 + 0.01 * 24, passes=1, path="LDS")
    for prec in (1, 1000):
        ms, reps = attr(prec)
        note("gm_frequency_attr int64, no dtg, precision %d" % prec, ms, reps, 8, passes=1, path="LDS")
    ms, reps = attr(1000, m=mask)
    note("gm_frequency_attr int64, no dtg, precision 1000, 1 % mask", ms, reps, 0.125 + 0.01 * 8, passes=1, path="LDS")
    ms, reps = z3(t1, 2610, 1, path=2)
    note("gm_z3_frequency, 1 week bin, path 2 (device atomics)", ms, reps, 24, path="atomics")
    ms, reps = z3(t, 2608, 54, path=2)
    atomic_ms = note("gm_z3_frequency, 54 week bins, path 2 (device atomics)", ms, reps, 24, path="atomics")
    ms, reps = attr(1000, path=2)
    note("gm_frequency_attr int64, no dtg, precision 1000, path 2", ms, reps, 8, path="atomics")

    # the pass sweep: windows of 16 k bins around the data take k passes of 16 bins each (path 1)
    sweep = []
    for passes in (1, 2, 4, 8):
        nb = 16 * passes
        ms, reps = z3(t, 2608, nb, path=1)
        note("gm_z3_frequency, %d week bins, path 1 (%d LDS passes)" % (nb, passes), ms, reps, 24 * passes,
             passes=passes, path="LDS")
        sweep.append((passes, ms))
    per_pass = (sweep[-1][1] - sweep[0][1]) / (sweep[-1][0] - sweep[0][0])
    res["derived"] = {
        "hist_ms_per_1e9_rows": round(hist_ms * 1e9 / n, 3),
        "one_bin_ms_per_1e9_rows": round(one_ms * 1e9 / n, 3),
        "one_bin_over_depth_x_hist": round(one_ms / (5 * hist_ms), 3),
        "lds_ms_per_further_pass": round(per_pass, 4),
        "atomics_54_bins_ms": round(atomic_ms, 4),
        "passes_at_which_atomics_catch_up": round(1 + (atomic_ms - sweep[0][1]) / per_pass, 1),
    }
    print(json.dumps(res["derived"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
