"""Curve probe: times gm_xz2_index / gm_xz3_index over 100M envelopes shaped as the bench's configs[4] leg, and
the row kernels bench.py does not time: gm_z3_index_key, gm_z2_index, gm_z3_invert and gm_xz2_index with every
column viewed one row in (8-B aligned, not 16-B: the scalar fallbacks) and gm_legacy_z3_index.  Device events
around ten calls (tuning and A/B probe; GEOMESA_HIP_LIB selects a variant)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from geomesa_amd import _lib  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    m = n + 1     # one spare row: [:n] is the allocation's own alignment, [1:] is 8 B in
    ctx = _lib.context()
    lib, h, P = ctx.lib, ctx.handle, _lib.ptr
    x = torch.empty(m, dtype=torch.float64, device="cuda"); y = torch.empty_like(x)
    t = torch.empty(m, dtype=torch.int64, device="cuda")
    bench.gen_points(ctx, m, 0, (-180.0, -90.0, 180.0, 90.0), x, y, t)
    g = torch.Generator(device="cuda").manual_seed(11)
    w = torch.pow(10.0, torch.rand(m, device="cuda", dtype=torch.float64, generator=g) * 7 - 6)
    hg = torch.pow(10.0, torch.rand(m, device="cuda", dtype=torch.float64, generator=g) * 7 - 6)
    xmax = torch.clamp(x + w, max=180.0); ymax = torch.clamp(y + hg, max=90.0)
    zmin = torch.remainder(t, 604_800_000).to(torch.float64) / 1000.0
    zmax = torch.clamp(zmin + torch.pow(10.0, torch.rand(m, device="cuda", dtype=torch.float64, generator=g) * 4.94),
                       max=604800.0)
    toff = torch.remainder(t, 604_800_000) // 1000     # offsets within the week, seconds
    del w, hg
    xo = torch.empty(m, dtype=torch.int64, device="cuda")
    bo = torch.empty(m, dtype=torch.int16, device="cuda")
    a = lambda v: P(v[:n])      # noqa: E731  aligned view
    u = lambda v: P(v[1:])      # noqa: E731  one row in
    legs = (
        ("xz2_index", lambda: lib.gm_xz2_index(h, a(x), a(y), a(xmax), a(ymax), n, 12, 0, a(xo), None, None), 40),
        ("xz3_index", lambda: lib.gm_xz3_index(h, a(x), a(y), a(zmin), a(xmax), a(ymax), a(zmax), n, 12, 1, 0, a(xo), None,
                                               None), 56),
        ("z3_index_key_unaligned", lambda: lib.gm_z3_index_key(h, u(x), u(y), u(t), n, 1, 0, u(bo), u(xo), None, None), 34),
        ("z2_index_unaligned", lambda: lib.gm_z2_index(h, u(x), u(y), n, 31, 0, u(xo), None, None), 24),
        ("z3_invert_unaligned", lambda: lib.gm_z3_invert(h, u(t), n, 1, 21, u(zmin), u(zmax), u(xo)), 32),
        ("xz2_index_unaligned", lambda: lib.gm_xz2_index(h, u(x), u(y), u(xmax), u(ymax), n, 12, 0, u(xo), None, None), 40),
        ("legacy_z3_index", lambda: lib.gm_legacy_z3_index(h, a(x), a(y), a(toff), n, 0, 1, 0, a(xo), None, None), 32),
    )     # the invert leg runs after the XZ3 one: it overwrites zmin / zmax (any int64 is a valid z)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn, bpu in legs:
        fn(); torch.cuda.synchronize()
        ev0.record()
        for _ in range(10):
            assert fn() == 0
        ev1.record(); torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1) / 10
        print("%-24s %8.4f ms  %6.3f of 8 TB/s" % (name, ms, bpu * n / ms / 1e9 / 8.0), flush=True)


if __name__ == "__main__":
    main()
