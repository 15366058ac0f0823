"""Times the density scan over resident generated line features and writes profiles/density_lines_probe.json.

gm_density_lines over LineString columns of 20 vertices per track built on the device: short tracks (a
random walk, every step 1 to 3 pixels of a 512 x 512 grid) and long segments (vertices uniform in a box of
80 x 80 such pixels: tens of pixels per segment), at 128 x 128, 512 x 512 and 1024 x 1024 over the world,
unweighted and weighted, on the automatic path and on the device-atomic path, and with a 1 % mask; beside, in
the same run, the streaming copy (gm_device_copy) and gm_density_points on its device-atomic path over as
many points as there are vertices.  Every row states vertices/s, its 16 B/vertex as a share of the copy
rate, and additions/s (the additions are the sum of the unweighted grid of one call).  Device events
around one call, or around enough calls to pass half a second, after a warm-up call.

    python tools/density_lines_probe.py [--n 1000000000] [--out profiles/density_lines_probe.json]
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
from geomesa_amd.arrow import GeomColumnC  # noqa: E402
from bench import gen_points  # noqa: E402

ENV = (-180.0, -90.0, 180.0, 90.0)
PER = 20                                  # vertices per track
PX, PY = 360.0 / 512, 180.0 / 512         # the pixel the track shapes are stated in
P = _lib.ptr


def timed(f, floor_s=0.5):
    """ms per call of f, after a warm-up call by the caller: one call, and when that is short enough
    calls to pass floor_s in total."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    first = e0.elapsed_time(e1)
    if first >= floor_s * 500.0:
        return first, 1
    reps = max(3, int(math.ceil(floor_s * 1000.0 / max(first, 1e-3))))
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def make_tracks(tracks, shape, seed):
    """[y, x] tuples (tracks * PER, 2) of `shape` tracks: "short" (steps of 1 to 3 pixels) or "long"
    (vertices uniform in a box of 80 x 80 pixels)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    out = torch.empty((tracks * PER, 2), dtype=torch.float64, device="cuda")
    piece = 1 << 21
    for lo in range(0, tracks, piece):
        k = min(piece, tracks - lo)

        def rand(*s):
            return torch.rand(s, generator=gen, dtype=torch.float64, device="cuda")
        cx, cy = rand(k, 1) * 300.0 - 150.0, rand(k, 1) * 120.0 - 60.0
        if shape == "short":
            ang, r = rand(k, PER) * (2 * math.pi), 1.0 + 2.0 * rand(k, PER)
            r[:, 0] = 0.0
            x = cx + torch.cumsum(r * torch.cos(ang), 1) * PX
            y = cy + torch.cumsum(r * torch.sin(ang), 1) * PY
        else:
            x = cx + (rand(k, PER) - 0.5) * 80.0 * PX
            y = cy + (rand(k, PER) - 0.5) * 80.0 * PY
        v = out[lo * PER:(lo + k) * PER]
        v[:, 0] = y.reshape(-1)
        v[:, 1] = x.reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_lines_probe.json"))
    a = ap.parse_args()
    tracks = a.n // PER
    n = tracks * PER
    ctx = _lib.context()
    lib, h = ctx.lib, ctx.handle
    res = {"vertices": n, "tracks": tracks, "vertices_per_track": PER, "envelope": ENV,
           "device": torch.cuda.get_device_name(0), "rows": []}
    tally = torch.zeros(3, dtype=torch.int64, device="cuda")

    def note(name, ms, reps, units, **kw):
        row = dict(name=name, ms=round(ms, 4), reps=reps, units_per_s=round(units / ms * 1e3), **kw)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        return row

    # yardsticks of the same run: the streaming copy, and the point scan's device atomics over n points
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    gen_points(ctx, n, 0, ENV, x, y, t)
    copy = lambda: _lib.check(lib.gm_device_copy(h, P(y), P(x), n * 8), "gm_device_copy")  # noqa: E731
    copy()
    ms, reps = timed(copy)
    copy_gbs = 16.0 * n / ms / 1e6
    note("gm_device_copy", ms, reps, n, gb_per_s=round(copy_gbs, 1), bytes_per_unit=16)
    gen_points(ctx, n, 0, ENV, x, y, t)
    del t
    res["point_atomics"] = {}
    for size in (128, 512, 1024):
        grid = torch.zeros((size, size), dtype=torch.float64, device="cuda")
        g = _lib.DensityGrid(ENV[0], ENV[1], ENV[2], ENV[3], size, size, 0, 2)
        pts = lambda: _lib.check(lib.gm_density_points(h, P(x), P(y), None, n, None, None, 0, ctypes.byref(g),  # noqa: E731
                                                       P(grid), P(tally)), "gm_density_points")
        pts()
        ms, reps = timed(pts)
        row = note("gm_density_points %dx%d" % (size, size), ms, reps, n, path=2, additions_per_s=round(n / ms * 1e3))
        res["point_atomics"][size] = row["additions_per_s"]
    del x, y
    torch.cuda.empty_cache()

    off = (torch.arange(tracks + 1, device="cuda", dtype=torch.int64) * PER).to(torch.int32)
    w = torch.rand(tracks, dtype=torch.float64, device="cuda") * 4.0
    words = (tracks + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device="cuda")
    bits = torch.arange(64, device="cuda", dtype=torch.int64)
    step = 1 << 20
    for lo in range(0, words, step):
        k = min(step, words - lo)
        mask[lo:lo + k] = ((torch.rand((k, 64), device="cuda") < 0.01).to(torch.int64) << bits).sum(1)
    for shape in ("short", "long"):
        coords = make_tracks(tracks, shape, 7)
        col = GeomColumnC(1, 64, 0, 0, coords.data_ptr(), None, 0, (ctypes.c_void_p * 3)(off.data_ptr(), None, None))
        for size in (128, 512, 1024):
            grid = torch.zeros((size, size), dtype=torch.float64, device="cuda")

            def call(path, weighted, masked):
                g = _lib.DensityGrid(ENV[0], ENV[1], ENV[2], ENV[3], size, size, 0, path)
                _lib.check(lib.gm_density_lines(h, ctypes.byref(col), P(w) if weighted else None, tracks,
                                                P(mask) if masked else None, None, 0, ctypes.byref(g), P(grid),
                                                P(tally)), "gm_density_lines")
            additions = {}
            for masked in (False, True):
                grid.zero_()
                call(2, False, masked)
                additions[masked] = int(grid.sum().item())
            for weighted in (False, True):
                for masked in (False, True):
                    for path in (0, 2):
                        if path == 0:
                            call(path, weighted, masked)          # warm-up; path 2 had the additions call
                        ms, reps = timed(lambda: call(path, weighted, masked))
                        adds = additions[masked]
                        note("gm_density_lines %s %dx%d" % (shape, size, size), ms, reps, n, tracks=shape, size=size,
                             weighted=weighted, selection="mask 1 %" if masked else "none", path=path,
                             additions=adds, additions_per_s=round(adds / ms * 1e3),
                             share_of_copy_at_16B_per_vertex=round(16.0 * n / ms / 1e6 / copy_gbs, 4),
                             point_atomics_additions_per_s=res["point_atomics"][size])
        del coords
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
