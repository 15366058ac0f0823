"""Times the density scan over resident generated points and writes profiles/density_scan_probe.json.

gm_density_points unweighted and weighted, with no selection and with a 1 % mask, at 128 x 128 (one LDS
pass), 256 x 256, 512 x 512 and 1024 x 1024, on the automatic path and on the device-atomic path, beside two
yardsticks in the same process: gm_z3_histogram at length 512 (the kernel of this shape the project already
has: 24 B/point against the density scan's 16) and a torch route over the same columns (indices by tensor
arithmetic, then torch.bincount: what a user without the kernel does), and the streaming copy
(gm_device_copy) the rates are shares of.  Device events around enough calls to pass half a second, after
a warm-up call of every shape.

    python tools/density_scan_probe.py [--n 1000000000] [--out profiles/density_scan_probe.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_scan_probe.json"))
    a = ap.parse_args()
    n = a.n
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    gen_points(ctx, n, 0, ENV, x, y, t)
    w = torch.empty_like(x)
    _lib.check(lib.gm_gen_points(h, 77, n, 0, 0.0, 4.0, 0.0, 1.0, 0, 1, P(w), None, None), "gm_gen_points")
    # a 1 % mask: random words with about 1 % of their bits set (the AND of independent draws, in pieces)
    words = (n + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device="cuda")
    bits = torch.arange(64, device="cuda", dtype=torch.int64)
    step = 1 << 20
    for lo in range(0, words, step):
        k = min(step, words - lo)
        m = (torch.rand((k, 64), device="cuda") < 0.01).to(torch.int64)
        mask[lo:lo + k] = (m << bits).sum(1)
    torch.cuda.synchronize()
    res = {"n": n, "envelope": ENV, "device": torch.cuda.get_device_name(0), "rows": []}

    def note(name, ms, reps, bytes_per_row, **kw):
        row = dict(name=name, ms=round(ms, 4), reps=reps, rows_per_s=round(n / ms * 1e3),
                   gb_per_s=round(bytes_per_row * n / ms / 1e6, 1), bytes_per_row=bytes_per_row, **kw)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

    # the streaming copy the rates are shares of: n * 8 B read + n * 8 B written
    ms, reps = timed(lambda: _lib.check(lib.gm_device_copy(h, P(w), P(x), n * 8), "gm_device_copy"))
    note("gm_device_copy", ms, reps, 16)
    _lib.check(lib.gm_gen_points(h, 77, n, 0, 0.0, 4.0, 0.0, 1.0, 0, 1, P(w), None, None), "gm_gen_points")

    c = torch.zeros((54, 512), dtype=torch.int64, device="cuda")
    pr = torch.zeros(54, dtype=torch.uint8, device="cuda")
    tl = torch.zeros(2, dtype=torch.int64, device="cuda")
    ms, reps = timed(lambda: _lib.check(lib.gm_z3_histogram(h, P(x), P(y), P(t), n, 1, 512, 0, 2608, 54, P(pr), P(c),
                                                            P(tl)), "gm_z3_histogram"))
    note("gm_z3_histogram length 512", ms, reps, 24)

    tally = torch.zeros(3, dtype=torch.int64, device="cuda")
    for size in (128, 256, 512, 1024):
        grid = torch.zeros((size, size), dtype=torch.float64, device="cuda")
        for weighted in (False, True):
            for sel in ("none", "mask 1 %"):
                for path in (0, 2):
                    g = _lib.DensityGrid(ENV[0], ENV[1], ENV[2], ENV[3], size, size, 0, path)
                    f = lambda: _lib.check(lib.gm_density_points(  # noqa: E731
                        h, P(x), P(y), P(w) if weighted else None, n, P(mask) if sel != "none" else None, None, 0,
                        ctypes.byref(g), P(grid), P(tally)), "gm_density_points")
                    ms, reps = timed(f)
                    bpr = 16 + (8 if weighted else 0) + (0.125 if sel != "none" else 0)
                    note("gm_density_points %dx%d" % (size, size), ms, reps, bpr, weighted=weighted, selection=sel,
                         path=path)

    # the torch route, in pieces of 2^27 rows so its temporaries stay small
    def torch_route(size, weighted):
        out = torch.zeros(size * size, dtype=torch.float64, device="cuda")
        dx, dy = (ENV[2] - ENV[0]) / size, (ENV[3] - ENV[1]) / size
        piece = 1 << 27
        for lo in range(0, n, piece):
            xs, ys = x[lo:lo + piece], y[lo:lo + piece]
            i = torch.floor((xs - ENV[0]) / dx).to(torch.int64).clamp_(max=size - 1)
            j = torch.floor((ys - ENV[1]) / dy).to(torch.int64).clamp_(max=size - 1)
            ok = (xs >= ENV[0]) & (xs <= ENV[2]) & (ys >= ENV[1]) & (ys <= ENV[3])
            flat = (j * size + i)[ok]
            out += torch.bincount(flat, weights=w[lo:lo + piece][ok] if weighted else None, minlength=size * size)
        return out

    for size in (256, 1024):
        for weighted in (False, True):
            ms, reps = timed(lambda: torch_route(size, weighted), floor_s=0.3)
            note("torch floor + bincount %dx%d" % (size, size), ms, reps, 16 + (8 if weighted else 0), weighted=weighted,
                 selection="none")
    # the two routes agree (unweighted, points inside the envelope)
    grid = torch.zeros((256, 256), dtype=torch.float64, device="cuda")
    g = _lib.DensityGrid(ENV[0], ENV[1], ENV[2], ENV[3], 256, 256, 0, 0)
    _lib.check(lib.gm_density_points(h, P(x), P(y), None, n, None, None, 0, ctypes.byref(g), P(grid), P(tally)),
               "gm_density_points")
    res["torch_route_equal_256"] = bool(torch.equal(grid.view(-1), torch_route(256, False)))
    print("torch route equal:", res["torch_route_equal_256"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
