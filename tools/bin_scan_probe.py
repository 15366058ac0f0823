"""Times the BIN track-record scan over resident generated points and writes profiles/bin_scan_probe.json.

In one process: the streaming copy (gm_device_copy) every rate is a share of; gm_bin_points over n points as
16-B and 24-B records, with no selection and under a 1 % mask, and the 24-B form into an output that is only
8-B aligned (8-B stores in place of the LDS-staged 16-B ones), the 16-B form with one column moved by 8 B
(scalar loads) and with one NaN row (the direct write, then the three passes); the encode followed by the sort at n_sort
records; gm_bin_track over n_sort 16-byte strings; and, as yardsticks from the same run, the density scan's
one LDS pass (128 x 128, unweighted), the Z3 key encode, and a torch composition that produces the same
bytes (truncating division, casts, stack, view).  Every leg reports its share of the copy rate over its own
bytes per row (44 B for the 16-B point form: 28 read, 16 written).  Device events around enough calls to pass
half a second, after a warm-up call.

    python tools/bin_scan_probe.py [--n 1000000000] [--n-sort 100000000] [--out profiles/bin_scan_probe.json]
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
from bench import gen_points  # noqa: E402

ENV = (-180.0, -90.0, 180.0, 90.0)
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
    ap.add_argument("--n-sort", type=int, default=100_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_scan_probe.json"))
    a = ap.parse_args()
    n, ns = a.n, min(a.n_sort, a.n)
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    gen_points(ctx, n, 0, ENV, x, y, t)
    label = torch.empty(n, dtype=torch.int64, device="cuda")
    _lib.check(lib.gm_gen_points(h, 78, n, 0, 0.0, 1.0, 0.0, 1.0, 0, 1 << 40, None, None, P(label)), "gm_gen_points")
    track = label.view(torch.int32)[::2].contiguous()       # the low words: any int32 column will do
    words = (n + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device="cuda")
    bits = torch.arange(64, device="cuda", dtype=torch.int64)
    step = 1 << 20
    for lo in range(0, words, step):
        k = min(step, words - lo)
        m = (torch.rand((k, 64), device="cuda") < 0.01).to(torch.int64)
        mask[lo:lo + k] = (m << bits).sum(1)
    out = torch.empty(n * 24 + 16, dtype=torch.uint8, device="cuda")
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    nrec = ctypes.c_int64()
    torch.cuda.synchronize()
    res = {"n": n, "n_sort": ns, "device": torch.cuda.get_device_name(0), "rows": []}
    copy_gbs = [0.0]

    def note(name, ms, reps, bytes_per_row, rows=n, **kw):
        gbs = bytes_per_row * rows / ms / 1e6
        row = dict(name=name, ms=round(ms, 4), reps=reps, rows=rows, rows_per_s=round(rows / ms * 1e3),
                   gb_per_s=round(gbs, 1), bytes_per_row=bytes_per_row, **kw)
        if copy_gbs[0]:
            row["share_of_copy"] = round(gbs / copy_gbs[0], 3)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

    ms, reps = timed(lambda: _lib.check(lib.gm_device_copy(h, P(out), P(x), n * 8), "gm_device_copy"))
    copy_gbs[0] = 16 * n / ms / 1e6
    note("gm_device_copy", ms, reps, 16)

    def encode(rows, with_label, sel, sort=0, dst=out, cols=(x, y, t, track, label)):
        o = _lib.BinOpts(sort, 0)
        cx, cy, ct, ck, cl = cols
        rc = lib.gm_bin_points(h, P(cx), P(cy), P(ct), P(ck), P(cl) if with_label else None, rows,
                               P(mask) if sel else None, None, 0, ctypes.byref(o), P(dst), rows, ctypes.byref(nrec),
                               P(tally))
        _lib.check(rc, "gm_bin_points")

    for with_label in (False, True):
        rb, read = (24, 36) if with_label else (16, 28)
        ms, reps = timed(lambda: encode(n, with_label, False))
        note("gm_bin_points %d-B" % rb, ms, reps, read + rb, selection="none")
        ms, reps = timed(lambda: encode(n, with_label, True))
        note("gm_bin_points %d-B" % rb, ms, reps, 0.125 + 0.01 * (read + rb), selection="mask 1 %", records=nrec.value)
    ms, reps = timed(lambda: encode(n, True, False, dst=out[8:]))
    note("gm_bin_points 24-B, 8-B aligned output (8-B stores)", ms, reps, 60, selection="none")
    xs = torch.empty(n + 1, dtype=torch.float64, device="cuda")[1:]
    xs.copy_(x)
    ms, reps = timed(lambda: encode(n, False, False, cols=(xs, y, t, track, label)))
    note("gm_bin_points 16-B, x moved by 8 B (scalar loads)", ms, reps, 44, selection="none")
    del xs
    # one NaN row: the direct write finds it, and the count -> scan -> write passes run after it
    xn = x.clone()
    xn[12345] = float("nan")
    ms, reps = timed(lambda: encode(n, False, False, cols=(xn, y, t, track, label)))
    note("gm_bin_points 16-B, one NaN row (direct attempt, then count + scan + write)", ms, reps, 44 + 60,
         selection="none", records=nrec.value)
    del xn

    # yardsticks of the same run
    grid = torch.zeros((128, 128), dtype=torch.float64, device="cuda")
    g = _lib.DensityGrid(ENV[0], ENV[1], ENV[2], ENV[3], 128, 128, 0, 0)
    ms, reps = timed(lambda: _lib.check(lib.gm_density_points(h, P(x), P(y), None, n, None, None, 0, ctypes.byref(g),
                                                              P(grid), P(tally)), "gm_density_points"))
    note("gm_density_points 128x128 (one LDS pass)", ms, reps, 16)
    b = out[:2 * n].view(torch.int16)
    z = out[2 * n + (-2 * n) % 16:][:8 * n].view(torch.int64)
    ms, reps = timed(lambda: _lib.check(lib.gm_z3_index_key(h, P(x), P(y), P(t), n, 1, 0, P(b), P(z), None, None),
                                        "gm_z3_index_key"))
    note("gm_z3_index_key (week)", ms, reps, 34)
    tally.zero_()

    # encode + sort
    for with_label in (False, True):
        rb, read = (24, 36) if with_label else (16, 28)
        ms, reps = timed(lambda: encode(ns, with_label, False, sort=1))
        note("gm_bin_points %d-B + sort" % rb, ms, reps, read + rb, rows=ns)
    encode(ns, False, False)                                # ns unsorted records in out
    src = out[:ns * 16].clone()
    ms, reps = timed(lambda: _lib.check(lib.gm_bin_sort(h, P(src), ns, 16, P(out)), "gm_bin_sort"))
    note("gm_bin_sort 16-B", ms, reps, 32, rows=ns)
    del src

    # gm_bin_track over 16-byte strings
    data = torch.randint(97, 123, (ns * 16,), dtype=torch.uint8, device="cuda")
    off = (torch.arange(ns + 1, device="cuda", dtype=torch.int64) * 16).to(torch.int32)
    col = _lib.AttrColumn(_lib.GM_ATTR_UTF8, 0, data.data_ptr(), off.data_ptr(), None, 0)
    hashes = torch.empty(ns, dtype=torch.int32, device="cuda")
    ms, reps = timed(lambda: _lib.check(lib.gm_bin_track(h, ctypes.byref(col), ns, P(hashes)), "gm_bin_track"))
    note("gm_bin_track 16-byte strings", ms, reps, 24, rows=ns)
    del data, off, hashes

    # the torch composition of the same bytes, in pieces of 2^27 rows so its temporaries stay small
    piece = 1 << 27
    tout = out[:16 * min(n, piece)].view(torch.int32).view(-1, 4)

    def torch_route(rows):
        for lo in range(0, rows, piece):
            hi = min(rows, lo + piece)
            secs = torch.div(t[lo:hi], 1000, rounding_mode="trunc").to(torch.int32)
            torch.stack([track[lo:hi], secs, y[lo:hi].to(torch.float32).view(torch.int32),
                         x[lo:hi].to(torch.float32).view(torch.int32)], 1, out=tout[:hi - lo])
    ms, reps = timed(lambda: torch_route(n), floor_s=0.3)
    note("torch div + cast + stack, 16-B", ms, reps, 44)
    k = min(n, piece)
    torch_route(k)
    theirs = tout[:k].clone()
    mine = torch.empty(k * 16, dtype=torch.uint8, device="cuda")
    encode(k, False, False, dst=mine)
    res["torch_route_equal"] = bool(torch.equal(mine.view(torch.int32).view(-1, 4), theirs))
    print("torch route equal:", res["torch_route_equal"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
