"""Times the XZ2 table scan with the envelope filter (gm_table_scan) and with the exact geometry filter
(gm_table_scan_geom) over a table of linestrings (tuning probe; no bench.py leg).

  python tools/geom_scan_probe.py [n_lines] [--parent-lib=PATH] [--rounds=K]

Seeded inputs generated on the device: n_lines (default 20M) linestrings, tuple counts log-uniform in 2..256,
each an arc about a uniform centre; one query box that about 1% of the envelopes meet.  Timed with HIP events
(gm_timer_start / gm_timer_stop) after warm-up:
  (a) gm_table_scan, envelope filter -- on this tree's library and, with --parent-lib, on a build of the
      parent commit, alternating, K rounds of `reps` calls each;
  (b) gm_table_scan_geom.
The geometry result is checked on a strided sample of the envelope pass's survivors and of all features
against tests/geom_intersects_ref.intersects_restated.  The box filter's (k_refine, BoxPred) bytes model is the survivors' tuples
x 16 B; its share of 8 TB/s is taken over (b) - (a), the time the geometry filter adds."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from geomesa_amd import _lib  # noqa: E402
from geomesa_amd.arrow import GeomColumnC  # noqa: E402
from geomesa_amd.table import XZ2Table, _full_filter, key_ranges  # noqa: E402

BOX = (-10.0, 30.0, 26.0, 48.0)      # 1% of the world's area
REPS = 10


def make_lines(n, seed=5):
    """(coords [x, y] float64, int32 offsets, counts) on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(n, device="cuda", dtype=torch.float64, generator=g)
    cnt = torch.floor(torch.exp(np.log(2.0) + u * (np.log(257.0) - np.log(2.0)))).to(torch.int64).clamp_(2, 256)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(cnt, 0, out=off[1:])
    total = int(off[-1].item())
    assert total < 2 ** 31
    cx = torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 340 - 170
    cy = torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 160 - 80
    rad = torch.pow(10.0, torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 2 - 1.3)   # 0.05 .. 5 degrees
    th0 = torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 6.283185307179586
    span = (torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 0.85 + 0.05) * 3.141592653589793
    line = torch.repeat_interleave(torch.arange(n, device="cuda"), cnt, output_size=total)
    k = torch.arange(total, device="cuda") - off[line]
    th = th0[line] + span[line] * k.to(torch.float64) / (cnt[line] - 1).to(torch.float64)
    del k
    coords = torch.empty((total, 2), dtype=torch.float64, device="cuda")
    coords[:, 0] = cx[line] + rad[line] * torch.cos(th)
    coords[:, 1] = cy[line] + rad[line] * torch.sin(th)
    return coords, off.to(torch.int32), cnt


def bind(lib):
    for name in ("gm_ctx_create", "gm_table_scan", "gm_timer_start", "gm_timer_stop"):
        f = getattr(lib, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--"))
    n = int(args[0]) if args else 20_000_000
    rounds = int(opts.get("rounds", 3))
    ctx = _lib.context()
    lib, h, P = ctx.lib, ctx.handle, _lib.ptr
    coords, off, cnt = make_lines(n)
    gc = GeomColumnC(1, 64, 1, 0, coords.data_ptr(), None, 0, (ctypes.c_void_p * 3)(off.data_ptr(), None, None))
    env = torch.empty((4, n), dtype=torch.float64, device="cuda")
    _lib.check(lib.gm_arrow_envelopes(h, ctypes.byref(gc), n, *[P(env[k]) for k in range(4)]), "gm_arrow_envelopes")
    tb = XZ2Table(*[env[k] for k in range(4)])
    v = tb.ks.get_index_values([BOX])
    kr, _ = key_ranges(tb.ks.get_ranges(v), tb.shards)
    f, keep = _full_filter(tb.env, v.spatialBounds, perm=tb.perm)
    ids = torch.empty(n, dtype=torch.int64, device="cuda")
    nm, ns, ne = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    head = (P(tb.shard), P(tb.bin), P(tb.z), n, kr.ctypes.data, len(kr), ctypes.byref(f))
    tail = (P(tb.perm), P(ids), n, ctypes.byref(nm), ctypes.byref(ns))

    def timed(lb, hh, call):
        ms = ctypes.c_float()
        for _ in range(2):
            assert call() == 0
        assert lb.gm_timer_start(hh) == 0
        for _ in range(REPS):
            assert call() == 0
        assert lb.gm_timer_stop(hh, ctypes.byref(ms)) == 0
        return ms.value / REPS

    libs = [("tree", lib, h)]
    if "parent-lib" in opts:
        pl = bind(ctypes.CDLL(opts["parent-lib"]))
        ph = ctypes.c_void_p()
        assert pl.gm_ctx_create(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ph)) == 0
        libs.insert(0, ("parent", pl, ph))
    times = {name: [] for name, _, _ in libs}
    for _ in range(rounds):
        for name, lb, hh in libs:
            times[name].append(timed(lb, hh, lambda: lb.gm_table_scan(hh, *head, *tail)))
    env_ids = ids[:nm.value].clone()
    n_env, scanned = nm.value, ns.value
    t_geom = [timed(lib, h, lambda: lib.gm_table_scan_geom(h, *head, ctypes.byref(gc), *tail, ctypes.byref(ne)))
              for _ in range(rounds)]
    geom_ids = ids[:nm.value].clone()
    assert ne.value == n_env
    surv_tuples = int(cnt[env_ids].sum().item())
    # survivors the envelope shortcut does not decide (a LineString's x- or y-range within the box's): the walkers
    e = [env[k][env_ids] for k in range(4)]
    walk = ~(((e[0] >= BOX[0]) & (e[2] <= BOX[2])) | ((e[1] >= BOX[1]) & (e[3] <= BOX[3])))
    n_walk, walk_tuples = int(walk.sum().item()), int(cnt[env_ids][walk].sum().item())

    # strided samples against the host restatement
    import geom_intersects_ref as R
    hit = torch.zeros(n, dtype=torch.bool, device="cuda")
    hit[geom_ids] = True
    sample = torch.cat([env_ids[::max(1, n_env // 1500)], torch.arange(0, n, max(1, n // 500), device="cuda")])
    o64, hits = off.to(torch.int64), hit[sample].cpu().numpy()
    bad = 0
    for i, got in zip(sample.cpu().tolist(), hits):
        row = [tuple(t) for t in coords[int(o64[i]):int(o64[i + 1])].cpu().tolist()]
        bad += R.intersects_restated(row, "linestring", BOX) != bool(got)
    a = float(np.median(times["tree"]))
    b = float(np.median(t_geom))
    print("lines %d  tuples %d  scanned %d  envelope hits %d (%.2f%%)  geometry hits %d" %
          (n, int(off[-1].item()), scanned, n_env, 100.0 * n_env / n, len(geom_ids)))
    for name in times:
        print("(a) gm_table_scan      %-6s ms per call, rounds: %s" % (name, " ".join("%.4f" % t for t in times[name])))
    if "parent" in times:
        p = times["parent"]
        print("    parent spread %.4f ms, tree median - parent median %+.4f ms" %
              (max(p) - min(p), a - float(np.median(p))))
    else:
        print("    parent: not measured")
    print("(b) gm_table_scan_geom        ms per call, rounds: %s" % " ".join("%.4f" % t for t in t_geom))
    byts = surv_tuples * 16
    print("    survivors' tuples %d x 16 B = %.1f MB; over (b) - (a) = %.4f ms: %.1f GB/s, %.4f of 8 TB/s" %
          (surv_tuples, byts / 1e6, b - a, byts / max(b - a, 1e-9) / 1e6, byts / max(b - a, 1e-9) / 1e6 / 8000.0))
    print("    of them walked (not decided by the envelope shortcuts): %d survivors, %d tuples = %.1f MB" %
          (n_walk, walk_tuples, walk_tuples * 16 / 1e6))
    print("sample of %d features against intersects_restated: %d disagreements" % (len(hits), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
