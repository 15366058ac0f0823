"""The case table and the held-stream protocol of tests/test_gpu_streams.py.

A case is one C-ABI entry point in one form (with or without the host count or summary that makes it wait):
its device inputs for a seed (0 = the true dataset A, 1 = the decoy B; everything structural -- offsets,
validity, row_off, ids, polygon indexes, sorted table keys -- is the same in both, so a read stays inside its
buffer whichever dataset it sees), its outputs with their initial content (a size: 0xA5 fill; an array: what an
accumulating entry adds to), the call, and the reference result from the oracle or the definition module the
entry's own tests use.  A key of the input dictionary that starts with "_" is host data the reference needs and
is not uploaded.

held_run is the protocol: buffers with B on the default stream, device-wide synchronise, then on the context's
stream a hold, the copies of A, the refill of the outputs and an event; the entry is called while the event is
still pending, and after gm_ctx_sync every output must equal the reference of A.  A kernel, copy or memset that
the library put on another stream ran during the hold: it read B, or the late refill wiped what it wrote.
plain_run is the same call with A in place and no hold (warm-up, shuffles, threads).
"""
import ctypes
import functools

import numpy as np

import test_gpu_abi_contract as C
from abi_buffers import FILL, Guarded, untouched
from geomesa_amd import _lib

OK, E_INVALID = _lib.GM_OK, _lib.GM_E_INVALID
I16, I32, I64, U8, U32, U64, F64 = C.I16, C.I32, C.I64, C.U8, C.U32, C.U64, C.F64
WEEK, T2020, T2021 = C.WEEK, C.T2020, C.T2021
WK_MS = 604800000
W2020 = T2020 // WK_MS

# rows per block of the kernels whose own tests name them (two blocks and an odd tail each)
DENSITY_BLOCK = 4096      # gm_density.hip: DTPB 1024 threads x 2 pairs x 2 rows (test_gpu_density.N_BLOCKS)
BIN_BLOCK = 2048          # gm_bin.hip: BROWS = BTPB 256 x BPAIRS 4 x 2 rows
FREQ_BLOCK = 4096         # gm_freq.hip: QTPB 1024 threads x 2 pairs x 2 rows, as the density kernel
COPY_BLOCK = 256 * 4 * 16     # gm_ctx.hip: k_stream_copy, 256 lanes x CPY_U 4 vectors x 16 B


class Case:
    name = entries = waits = None

    def __init__(self, ins, outs, call, expect, prepare=None, finish=None):
        self.ins, self.outs, self.call, self.expect, self.prepare, self.finish = ins, outs, call, expect, prepare, finish


# case name -> (the entry points it covers, waits, factory(scale) -> Case).  `waits` is transcribed from
# include/geomesa_hip.h: True = the call (in this form) synchronises the context stream before it returns,
# False = the header calls it asynchronous or stream-ordered.  The header line is cited where a case is added.
TABLE = {}

# Entry points of _lib.SIGNATURES without a case, one reason each: they enqueue no device work of their own
# on the context stream, or (the timers) are out of scope.
EXCLUDED = {
    "gm_abi_version": "a constant",
    "gm_ctx_create": "context lifecycle: the fixture of every case",
    "gm_ctx_create_owned": "context lifecycle: the fixture of every case",
    "gm_ctx_destroy": "context lifecycle: the teardown of every fixture",
    "gm_ctx_sync": "context lifecycle: step 6 of every case",
    "gm_ctx_stream": "context lifecycle: how every owned case reaches its stream",
    "gm_last_error": "thread-local text: host state, no device work",
    "gm_ctx_set_param": "parameters: host state of the context",
    "gm_ctx_get_param": "parameters: host state of the context",
    "gm_device_alloc": "alloc / free: hipMalloc, no stream",
    "gm_device_free": "alloc / free: hipFree, no stream",
    "gm_timer_start": "the timers are out of scope",
    "gm_timer_stop": "the timers are out of scope",
    "gm_pip_index_destroy": "index destroy: frees, enqueues nothing",
    "gm_pip_index_stats": "index stats: host fields of the index",
    "gm_pip_join_census": "the census: a diagnostic without a reference counterpart",
}


def add(name, entries, waits, factory):
    assert name not in TABLE
    TABLE[name] = ((entries,) if isinstance(entries, str) else tuple(entries), waits, factory)


@functools.lru_cache(maxsize=None)
def get(name, scale=1):
    entries, waits, factory = TABLE[name]
    c = factory(scale)
    c.name, c.entries, c.waits = name, entries, waits
    return c


@functools.lru_cache(maxsize=None)
def inputs(name, seed, scale=1):
    return get(name, scale).ins(seed)


@functools.lru_cache(maxsize=None)
def reference(name, seed, scale=1):
    import oracle as O
    O.lib()
    return get(name, scale).expect(O, inputs(name, seed, scale))


def decoy_share(name, scale=1):
    """The share of elements in which the references of A and B differ (counters: of those non-zero in
    either); None for a case without device inputs, which has no decoy."""
    if not any(not k.startswith("_") for k in inputs(name, 0, scale)):
        return None
    a, b = reference(name, 0, scale), reference(name, 1, scale)
    ea, eb = np.asarray(a["elems"]), np.asarray(b["elems"])
    assert ea.shape == eb.shape, name
    ne = ea != eb
    if ne.ndim > 1:
        ne = ne.reshape(len(ne), -1).any(axis=1)
        live = np.ones(len(ne), bool)
    else:
        live = ((ea != 0) | (eb != 0)) if a.get("counters") else np.ones(len(ne), bool)
    return float(ne[live].sum()) / max(int(live.sum()), 1)


# ---------------------------------------------------------------- running a case
_GPU = {}     # device-side objects cases share (polygon indexes), built once by their prepare()


def gpu_object(key, build):
    if key not in _GPU:
        _GPU[key] = build()
    return _GPU[key]


def payload(g):
    return g.buf[g.lo:g.hi]


def _bytes(a):
    return np.ascontiguousarray(a).view(U8).reshape(-1)


def _device_ins(d):
    return {k: v for k, v in d.items() if not k.startswith("_")}


def _out_bytes(v):
    return int(v) if isinstance(v, (int, np.integer)) else np.ascontiguousarray(v).nbytes


def hostval(v):
    if isinstance(v, _lib.BatchStatus):
        return (v.n_errors, v.first_index, v.first_code)
    if isinstance(v, np.ndarray):
        return v.tolist()
    return v.value if hasattr(v, "value") else v


def verify(case, rc, bufs, outs, host, exp, what):
    assert rc == exp.get("rc", OK), (what, rc, _lib.last_error())
    for k, g in list(bufs.items()) + list(outs.items()):
        g.check("%s %s" % (what, k))
    for k, want in exp["dev"].items():
        got = outs[k].read()
        if callable(want):
            want(got)
            continue
        w = _bytes(want)
        bad = np.flatnonzero(got[:w.size] != w)
        assert not bad.size, (what, k, "first wrong byte %d of %d" % (bad[0], w.size), int(bad.size))
        assert untouched(got[w.size:]), (what, k, "written past the result")
    if "check" in exp:
        exp["check"]({k: g.read() for k, g in outs.items()})
    for k, want in exp.get("host", {}).items():
        assert hostval(host[k]) == hostval(want), (what, k, hostval(host[k]), hostval(want))


def _pointers(bufs, outs):
    p = {k: g.ptr for k, g in bufs.items()}
    p.update({k: g.ptr for k, g in outs.items()})
    return p


def plain_run(ctx, name, scale=1):
    """The case with A in place from the start, no hold: call, gm_ctx_sync, compare with the reference."""
    import torch
    case, A, exp = get(name, scale), inputs(name, 0, scale), reference(name, 0, scale)
    if case.prepare:
        case.prepare()
    bufs = {k: Guarded.of(v) for k, v in _device_ins(A).items()}
    outs = {k: (Guarded(v) if isinstance(v, (int, np.integer)) else Guarded.of(v)) for k, v in case.outs.items()}
    torch.cuda.synchronize()
    host = {}
    try:
        rc = case.call(ctx.lib, ctx.handle, _pointers(bufs, outs), host)
        assert ctx.lib.gm_ctx_sync(ctx.handle) == OK, _lib.last_error()
        verify(case, rc, bufs, outs, host, exp, name)
    finally:
        if case.finish:
            case.finish(ctx.lib, host)


class Held:
    """Steps 1 to 4 of the protocol done; finish() is steps 5 (observed, returned) and 6."""

    def __init__(self, ctx, stream, name, hold, scale=1):
        import torch
        self.ctx, self.name = ctx, name
        self.case, A, B = get(name, scale), _device_ins(inputs(name, 0, scale)), _device_ins(inputs(name, 1, scale))
        self.exp = reference(name, 0, scale)
        share = decoy_share(name, scale)
        assert share is None or share > 0.5, (name, "the decoy's reference is too close to the true one", share)
        if self.case.prepare:
            self.case.prepare()
        self.bufs = {k: Guarded.of(B[k]) for k in A}
        self.outs = {k: Guarded(_out_bytes(v)) for k, v in self.case.outs.items()}
        late = {k: torch.from_numpy(_bytes(A[k]).copy()).pin_memory() for k in A if A[k].size}
        init = {k: torch.from_numpy(_bytes(v).copy()).pin_memory() for k, v in self.case.outs.items()
                if not isinstance(v, (int, np.integer)) and _out_bytes(v)}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hold()
            for k, t in late.items():
                payload(self.bufs[k]).copy_(t, non_blocking=True)
            for k, g in self.outs.items():
                if k in init:
                    payload(g).copy_(init[k], non_blocking=True)
                elif g.nbytes:
                    payload(g).fill_(FILL)
            self.ready = torch.cuda.Event()
            self.ready.record(stream)
        self.keep = (late, init)
        self.host = {}
        try:
            assert not self.ready.query(), (name, "step 3: the hold ended before the call; lengthen it")
            self.rc = self.case.call(ctx.lib, ctx.handle, _pointers(self.bufs, self.outs), self.host)
            self.early = not self.ready.query()     # step 5: the call returned with the stream's earlier work pending
        except BaseException:
            stream.synchronize()      # the late copies still read the staging blocks
            late.clear()              # emptied, not just dropped: the traceback keeps this frame and its locals
            init.clear()
            self.release()
            if self.case.finish:
                self.case.finish(ctx.lib, self.host)
            raise

    def finish(self):
        try:
            assert self.ctx.lib.gm_ctx_sync(self.ctx.handle) == OK, _lib.last_error()
            assert self.ready.query()
            verify(self.case, self.rc, self.bufs, self.outs, self.host, self.exp, self.name + " (held)")
        finally:
            self.release()
            if self.case.finish:
                self.case.finish(self.ctx.lib, self.host)
        return self.early

    def release(self):
        """Drops the pinned staging blocks.  torch's pinned-memory allocator records an event on every stream a
        block was used on when the block is freed, so they must go while the context's stream still exists: an
        owned stream dies with its context."""
        self.keep = None


def held_run(ctx, stream, name, hold, scale=1):
    return Held(ctx, stream, name, hold, scale).finish()


class Hold:
    """torch.cuda._sleep for `ms` milliseconds on the current stream, calibrated once with events."""

    def __init__(self, ms=100.0):
        import torch
        s = torch.cuda.Stream()
        probe = 20_000_000
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            torch.cuda._sleep(probe)
            e1.record(s)
        e1.synchronize()
        self.cycles_per_ms = probe / max(e0.elapsed_time(e1), 1e-3)
        self.ms = ms
        self.cycles = int(ms * self.cycles_per_ms)

    def __call__(self):
        import torch
        torch.cuda._sleep(self.cycles)


# ---------------------------------------------------------------- memory helpers
def _copy_case(which):
    def factory(scale):
        nbytes = 2 * COPY_BLOCK + 24     # two blocks of the vector kernel, one 16-B vector, an 8-B tail
        data = [np.random.default_rng(40 + s).integers(0, 256, nbytes, dtype=U8) for s in (0, 1)]
        for d in data:
            d[d == FILL] = 0
        if which == "gm_device_copy":
            return Case(lambda seed: {"src": data[seed]}, {"dst": nbytes},
                        lambda lib, h, p, host: lib.gm_device_copy(h, p["dst"], p["src"], nbytes),
                        lambda O, d: {"dev": {"dst": d["src"]}, "elems": d["src"]})
        if which == "gm_copy_to_device":
            return Case(lambda seed: {}, {"dst": nbytes},
                        lambda lib, h, p, host: lib.gm_copy_to_device(h, p["dst"], data[0].ctypes.data, nbytes),
                        lambda O, d: {"dev": {"dst": data[0]}, "elems": data[0]})

        def call(lib, h, p, host):
            host["dst"] = np.full(nbytes + 64, FILL, U8)
            return lib.gm_copy_to_host(h, host["dst"].ctypes.data, p["src"], nbytes)
        return Case(lambda seed: {"src": data[seed]}, {}, call,
                    lambda O, d: {"dev": {}, "host": {"dst": np.concatenate([d["src"], np.full(64, FILL, U8)])},
                                  "elems": d["src"]})
    return factory


add("gm_device_copy", "gm_device_copy", False, _copy_case("gm_device_copy"))          # :159 "(asynchronous)"
add("gm_copy_to_device", "gm_copy_to_device", True, _copy_case("gm_copy_to_device"))  # gm_internal.hpp:63 "Both synchronise"
add("gm_copy_to_host", "gm_copy_to_host", True, _copy_case("gm_copy_to_host"))


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9e3779b97f4a7c15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def _gen_points(scale):
    """gm_gen_points (:986-988): SplitMix64 keyed by (seed, index), restated in numpy from the header and
    k_gen_points' keying (three draws per index, key (3 index + j) x 0xd1b54a32d192ed03 xor seed)."""
    n, seed, base = 2 * 256 + 5, 77, 1000
    box, t0, t1 = (-125.0, -66.0, 24.0, 50.0), T2020, T2021

    def expect(O, d):
        with np.errstate(over="ignore"):
            k = (base + np.arange(n)).astype(U64)
            r = [_splitmix64(np.uint64(seed) ^ ((k * np.uint64(3) + np.uint64(j)) * np.uint64(0xd1b54a32d192ed03)))
                 for j in range(3)]
        unit = [(v >> np.uint64(11)).astype(F64) * 2.0 ** -53 for v in r[:2]]
        x = box[0] + unit[0] * (box[1] - box[0])
        y = box[2] + unit[1] * (box[3] - box[2])
        t = t0 + (r[2] % np.uint64(t1 - t0)).astype(I64)
        return {"dev": {"x": x, "y": y, "t": t}, "elems": x}
    return Case(lambda seed_: {}, {"x": 8 * n, "y": 8 * n, "t": 8 * n},
                lambda lib, h, p, host: lib.gm_gen_points(h, seed, n, base, box[0], box[1], box[2], box[3], t0, t1, p["x"],
                                                          p["y"], p["t"]), expect)


add("gm_gen_points", "gm_gen_points", False, _gen_points)     # :29-31 "only enqueue work ... and return"


# ---------------------------------------------------------------- index entries (:20-25: asynchronous without a summary)
def _index_case(entry, summary, status=None):
    status = summary if status is None else status

    def factory(scale):
        ic = C.INDEX_CASES[entry]()
        n = 2 * ic.block + 5
        bad = [1, ic.block + 7, n - 1]
        ncols = len(ic.cols(np.random.default_rng(0), 8))

        def ins(seed):
            cols = [np.array(c) for c in ic.cols(np.random.default_rng(7919 * seed + len(entry)), n)]
            ic.spoil(cols, bad)
            return {"c%d" % k: c for k, c in enumerate(cols)}
        outs = {"o%d" % k: n * np.dtype(d).itemsize for k, d in enumerate(ic.outs)}
        if status:
            outs["status"] = n

        def call(lib, h, p, host):
            host["summary"] = _lib.BatchStatus(7, 7, 7, 7)
            return ic.call(lib, h, [p["c%d" % k] for k in range(ncols)], n, [p["o%d" % k] for k in range(len(ic.outs))],
                           p.get("status"), ctypes.byref(host["summary"]) if summary else None)

        def expect(O, d):
            exp, est = ic.expect(O, [d["c%d" % k] for k in range(ncols)])
            assert np.flatnonzero(est).tolist() == bad
            dev = {"o%d" % k: np.asarray(e, dt) for k, (e, dt) in enumerate(zip(exp, ic.outs))}
            out = {"dev": dev, "elems": np.stack([np.asarray(e, I64) for e in exp], 1)}
            if status:
                dev["status"] = np.asarray(est, U8)
            if summary:
                out["host"] = {"summary": (3, 1, int(est[1]))}
            return out
        return Case(ins, outs, call, expect)
    return factory


for _e in C.INDEX_CASES:
    add(_e, _e, False, _index_case(_e, False))                    # :23-25 summary == NULL: stays asynchronous
    add(_e + "[status]", _e, False, _index_case(_e, False, True))     # :22-25 status != NULL, summary == NULL: the same
    add(_e + "[summary]", _e, True, _index_case(_e, True))        # the summary is read back: waits


def _invert_case(entry):
    def factory(scale):
        block, call_, dts, expect_ = C._invert(entry)
        n = 2 * block + 5

        def ins(seed):
            rng = np.random.default_rng(n + len(entry) + 101 * seed)
            z = rng.integers(0, 2**63 - 1, n, dtype=I64)
            z[::7] = rng.integers(-2**63, 0, len(z[::7]), dtype=I64)
            return {"z": z}

        def expect(O, d):
            want = [np.ascontiguousarray(w) for w in expect_(O, d["z"])]
            return {"dev": {"o%d" % k: w for k, w in enumerate(want)}, "elems": np.stack([w.view(I64) for w in want], 1)}
        return Case(ins, {"o%d" % k: 8 * n for k in range(len(dts))},
                    lambda lib, h, p, host: call_(lib, h, p["z"], n, [p["o%d" % k] for k in range(len(dts))]), expect)
    return factory


for _e in ("gm_z3_invert", "gm_z2_invert", "gm_legacy_z3_invert", "gm_legacy_z2_invert"):
    add(_e, _e, False, _invert_case(_e))       # :29-31 "only enqueue work ... and return"


# ---------------------------------------------------------------- ranges (host inputs: no decoy, a late refill of `out`)
def _ranges_case(entry):
    def factory(scale):
        import oracle as O
        O.lib()
        qs, call_, orc, _ = C.RANGES[entry](O)
        sel = [0, 2] * scale
        cap = 4096 * scale

        def call(lib, h, p, host):
            host["out_off"], host["needed"] = np.full(len(sel) + 1, -7, I64), ctypes.c_int64(-7)
            return call_(lib, h, sel, host["out_off"].ctypes.data, p["out"], cap, ctypes.byref(host["needed"]), None)

        def expect(O_, d):
            lists = [orc(qs[q]) for q in sel]
            flat = np.zeros(sum(len(x) for x in lists), C._RANGE)
            for k, (lo, hi, c) in enumerate(r for x in lists for r in x):
                flat[k] = (lo, hi, int(c), 0)
            off = np.cumsum([0] + [len(x) for x in lists]).astype(I64)
            assert 2 < len(flat) <= cap
            return {"dev": {"out": flat}, "host": {"out_off": off, "needed": len(flat)}, "elems": flat["lower"]}
        return Case(lambda seed: {}, {"out": cap * 24}, call, expect)
    return factory


for _e in C.RANGES:
    add(_e, _e, True, _ranges_case(_e))        # :215 out_off and *needed are host outputs: the call waits


# ---------------------------------------------------------------- scans (:256 "synchronises when n_match != NULL")
def _polys_of_query():
    from geomesa_amd.join import PolygonSet
    from test_gpu_query import SHAPES
    return PolygonSet.from_wkt(SHAPES)


def _scan_case(kind, count, own_mask=True):
    """own_mask False: mask == NULL, so the scan keeps its mask words in the context's workspace (alloc_scan) and
    only the ids and the count come back."""
    def factory(scale):
        from test_gpu_boundary import _rows
        n = C.SCAN_N * scale
        fb3, fb2 = C._filters()
        a3, a2 = np.frombuffer(fb3, U8).copy(), np.frombuffer(fb2, U8).copy()
        dur = (T2020 + 1000, T2021 - 1000)
        bbox = C.BBOX.copy()

        def ins(seed):
            import oracle as O
            rng = np.random.default_rng(2024 + 31 * seed + scale)
            if kind == "gm_query_scan+geom":
                from test_gpu_query import _points
                qx, qy, qt = _points(n, 5 + 2 * seed, _polys_of_query())
                k = rng.permutation(len(qx))[:n]
                return {"x": qx[k], "y": qy[k], "t": qt[k]}
            x, y, t = C.xyt_ms(rng, n)
            if kind in ("gm_strict_scan", "gm_query_scan"):
                return {"x": x, "y": y, "t": t}
            if kind.startswith("gm_z3"):
                b, z, st = O.z3_index_key_batch(x, y, t, False, WEEK)
                assert not st.any()
                if kind == "gm_z3filter_scan":
                    return {"bin": b, "z": z}
                keys = np.concatenate([b.astype(">i2").view(U8).reshape(-1, 2), z.astype(">i8").view(U8).reshape(-1, 8)], 1)
                buf, ro = _rows(keys, np.random.default_rng(5))
                return {"rows": buf, "row_off": ro, "_b": b, "_z": z}
            z2, st = O.z2_index_batch(x, y, False)
            assert not st.any()
            if kind == "gm_z2filter_scan":
                return {"z": z2}
            buf, ro = _rows(z2.astype(">i8").view(U8).reshape(-1, 8), np.random.default_rng(5))
            return {"rows": buf, "row_off": ro, "_z": z2}

        def call(lib, h, p, host):
            host["n_match"] = ctypes.c_int64(-7)
            nm = ctypes.byref(host["n_match"]) if count else None
            m, i = p.get("mask"), p["ids"]
            if kind == "gm_z3filter_scan":
                return lib.gm_z3filter_scan(h, a3.ctypes.data, len(a3), None, 0, p["bin"], p["z"], n, m, i, n, nm)
            if kind == "gm_z2filter_scan":
                return lib.gm_z2filter_scan(h, a2.ctypes.data, len(a2), p["z"], n, m, i, n, nm)
            if kind == "gm_z3filter_scan_rows":
                return lib.gm_z3filter_scan_rows(h, a3.ctypes.data, len(a3), p["rows"], p["row_off"], 0, n, m, i, n, nm, None)
            if kind == "gm_z2filter_scan_rows":
                return lib.gm_z2filter_scan_rows(h, a2.ctypes.data, len(a2), p["rows"], p["row_off"], 0, n, m, i, n, nm, None)
            if kind == "gm_strict_scan":
                return lib.gm_strict_scan(h, p["x"], p["y"], p["t"], n, bbox.ctypes.data, 1, dur[0], dur[1], m, i, n, nm)
            if kind == "gm_query_scan":
                return lib.gm_query_scan(h, p["x"], p["y"], p["t"], n, bbox.ctypes.data, 1, dur[0], dur[1], None, 0, m, i, n,
                                         nm)
            return lib.gm_query_scan(h, p["x"], p["y"], p["t"], n, None, 1, 50, 990, _GPU["query_ix"]._h, 1, m, i, n, nm)

        def expect(O, d):
            if kind == "gm_z3filter_scan":
                mask = O.z3filter_scan(fb3, [], d["bin"], d["z"])
            elif kind == "gm_z3filter_scan_rows":
                mask = O.z3filter_scan(fb3, [], d["_b"], d["_z"])
            elif kind == "gm_z2filter_scan":
                mask = O.z2filter_scan(fb2, d["z"])
            elif kind == "gm_z2filter_scan_rows":
                mask = O.z2filter_scan(fb2, d["_z"])
            elif kind == "gm_strict_scan":
                mask = O.strict_scan(d["x"], d["y"], d["t"], bbox, dur)
            elif kind == "gm_query_scan":
                mask = O.query_scan(d["x"], d["y"], d["t"], bbox=bbox, during=dur)
            else:
                ops = O.OraclePolySet(*_polys_of_query().to_arrays())
                mask = O.query_scan(d["x"], d["y"], d["t"], during=(50, 990), polys=ops, op=1)
            mask = np.asarray(mask, bool)
            ids = np.flatnonzero(mask).astype(I64)
            assert n // 8 < len(ids) < n * 7 // 8
            out = {"dev": {"mask": C._pack(mask), "ids": ids}, "elems": C._pack(mask)}
            if not own_mask:
                del out["dev"]["mask"]
            if count:
                out["host"] = {"n_match": len(ids)}
            return out

        def prepare():
            if kind == "gm_query_scan+geom":
                from geomesa_amd.join import PolygonIndex
                gpu_object("query_ix", lambda: PolygonIndex(_polys_of_query()))
        outs = {"mask": ((n + 63) // 64) * 8, "ids": 8 * n}
        if not own_mask:
            del outs["mask"]
        return Case(ins, outs, call, expect, prepare)
    return factory


for _k in C.SCANS:
    # :256 "synchronises when n_match != NULL"; :259-264 the filter_bytes scans wait once for their descriptor
    # upload whatever n_match is, and gm_query_scan with a geometry term always synchronises
    add(_k, _k.split("+")[0], "filter" in _k or "+geom" in _k, _scan_case(_k, False))
    add(_k + "[count]", _k.split("+")[0], True, _scan_case(_k, True))
    add(_k + "[ids]", _k.split("+")[0], True, _scan_case(_k, True, own_mask=False))


# ---------------------------------------------------------------- join, relate, index transfer
@functools.lru_cache(maxsize=None)
def _join_host():
    """The points and polygons of test_gpu_abi_contract.join_data, without its device index."""
    from geomesa_amd.join import synthetic_counties, synthetic_points
    from test_gpu_join_faults import _edge_points
    ps = synthetic_counties(6, 3)
    px, py = synthetic_points(17_001, seed=11)
    ex, ey = _edge_points(ps, 1e-4, np.random.default_rng(12))
    px, py = np.concatenate([px, ex]), np.concatenate([py, ey])
    k = np.random.default_rng(13).permutation(len(px))
    return ps, px[k], py[k]


def _join_points(seed, scale):
    _, px, py = _join_host()
    if seed:
        px, py = px[::-1], py[::-1]
    return np.tile(px, scale).copy(), np.tile(py, scale).copy()


def _join_index():
    from geomesa_amd.join import PolygonIndex
    return gpu_object("join_ix", lambda: PolygonIndex(_join_host()[0]))


def _pairs_check(exp_pairs, id_base=0):
    """The pair set in any order (the header leaves the order open).  cap is above the pair count here, and
    the header promises nothing about the entries between the two (the join stages whole slabs there); the
    guards behind cap are checked with every buffer."""
    p = len(exp_pairs)

    def check(got):
        pt, pl = got["pt"].view(I64), got["pl"].view(I32)
        assert sorted(zip((pt[:p] - id_base).tolist(), pl[:p].tolist())) == exp_pairs
    return check


def _join_expect(O, px, py, pred, count, id_base=0):
    ps = _join_host()[0]
    a, b = O.OraclePolySet(*ps.to_arrays()).join(px, py, nthreads=8, predicate=pred)
    pairs = sorted(zip(a.tolist(), b.tolist()))
    assert len(pairs) > 4096 and len(pairs) <= 2 * len(px)
    own = np.full(len(px), -1, I64)
    own[a] = b
    out = {"dev": {}, "check": _pairs_check(pairs, id_base), "elems": own}
    if count:
        out["host"] = {"n_pairs": len(pairs)}
    return out


def _join_case(entry, count):
    pred = "st_intersects" if entry == "gm_pip_join_pred" else "st_contains"

    def factory(scale):
        n = len(_join_host()[1]) * scale
        cap = 2 * n

        def ins(seed):
            px, py = _join_points(seed, scale)
            return {"yx": C.interleave_yx(px, py)} if entry == "gm_pip_join_arrow" else {"px": px, "py": py}

        def call(lib, h, p, host):
            host["n_pairs"] = ctypes.c_int64(-7)
            cnt = ctypes.byref(host["n_pairs"]) if count else None
            ix = _GPU["join_ix"]._h
            if entry == "gm_pip_join":
                return lib.gm_pip_join(h, ix, p["px"], p["py"], n, 1000, p["pt"], p["pl"], cap, cnt)
            if entry == "gm_pip_join_ex":
                return lib.gm_pip_join_ex(h, ix, p["px"], p["py"], n, 0, p["pt"], p["pl"], cap, cnt, _lib.GM_JOIN_DIRECT)
            if entry == "gm_pip_join_pred":
                return lib.gm_pip_join_pred(h, ix, p["px"], p["py"], n, 0, p["pt"], p["pl"], cap, cnt, 0,
                                            _lib.GM_SPATIAL_INTERSECTS)
            host["g"] = C.point_struct(None)
            host["g"].coords = p["yx"].value
            return lib.gm_pip_join_arrow(h, ix, ctypes.byref(host["g"]), n, 0, p["pt"], p["pl"], cap, cnt, 0,
                                         _lib.GM_SPATIAL_CONTAINS)

        def expect(O, d):
            px, py = (d["yx"][1::2], d["yx"][0::2]) if entry == "gm_pip_join_arrow" else (d["px"], d["py"])
            return _join_expect(O, px, py, pred, count, 1000 if entry == "gm_pip_join" else 0)
        return Case(ins, {"pt": 8 * cap, "pl": 4 * cap}, call, expect, _join_index)
    return factory


for _e in ("gm_pip_join", "gm_pip_join_ex", "gm_pip_join_pred", "gm_pip_join_arrow"):
    add(_e, _e, False, _join_case(_e, False))                 # :359 "With n_pairs = NULL the call is stream-ordered"
    add(_e + "[count]", _e, True, _join_case(_e, True))       # :360 "with n_pairs it synchronises the context stream"


def _index_build_case(how):
    """An index built (or imported) on the context while its stream is held, then joined stream-ordered on the
    same context with late points: the build's uploads and kernels must be ordered before the join."""
    def factory(scale):
        n = len(_join_host()[1])
        cap = 2 * n

        def call(lib, h, p, host):
            ps = _join_host()[0]
            ix = ctypes.c_void_p()
            host["index"] = ix
            if how == "gm_pip_index_create":
                host["cs"] = ps.c_struct()
                rc = lib.gm_pip_index_create(h, ctypes.byref(host["cs"]), ctypes.byref(ix))
            elif how == "gm_pip_index_create_ex":
                host["cs"] = ps.c_struct()
                rc = lib.gm_pip_index_create_ex(h, ctypes.byref(host["cs"]), 4096, ctypes.byref(ix))
            elif how == "gm_pip_index_create_arrow":
                from geomesa_amd.arrow import GeomColumnC
                host["yx"] = C.interleave_yx(ps.vx, ps.vy)
                offs = (ctypes.c_void_p * 3)(ps.poly_part_off.ctypes.data, ps.part_ring_off.ctypes.data,
                                             ps.ring_vert_off.ctypes.data)
                host["g"] = GeomColumnC(5, 64, 0, 0, host["yx"].ctypes.data, None, 0, offs)
                rc = lib.gm_pip_index_create_arrow(h, ctypes.byref(host["g"]), ps.n_polys, 0, ctypes.byref(ix))
            else:
                import torch
                src = _GPU["join_ix"]._h
                lay = _lib.PipIndexLayout()
                rc = lib.gm_pip_index_export(src, ctypes.byref(lay))
                host["arrays"] = [torch.empty(max(int(lay.bytes[k]), 16), dtype=torch.uint8, device="cuda")
                                  for k in range(_lib.GM_PIP_INDEX_ARRAYS)]
                for k, t in enumerate(host["arrays"]):
                    rc = rc or lib.gm_pip_index_copy_array(h, src, k, _lib.ptr(t))
                ptrs = (ctypes.c_void_p * _lib.GM_PIP_INDEX_ARRAYS)(*[t.data_ptr() for t in host["arrays"]])
                rc = rc or lib.gm_pip_index_import(h, ctypes.byref(lay), ptrs, ctypes.byref(ix))
            if rc != OK:
                return rc
            return lib.gm_pip_join(h, ix, p["px"], p["py"], n, 0, p["pt"], p["pl"], cap, None)

        def finish(lib, host):
            if host.get("index"):
                lib.gm_pip_index_destroy(host["index"])

        def ins(seed):
            px, py = _join_points(seed, 1)
            return {"px": px, "py": py}
        return Case(ins, {"pt": 8 * cap, "pl": 4 * cap}, call,
                    lambda O, d: _join_expect(O, d["px"], d["py"], "st_contains", False), _join_index, finish)
    return factory


# :309-316 and :331-350 promise no asynchrony for a build or an import (they return a finished handle), so
# these cases assert no early return; gm_pip_index_copy_array alone is "(stream-ordered)" (:335)
add("gm_pip_index_create", "gm_pip_index_create", True, _index_build_case("gm_pip_index_create"))
add("gm_pip_index_create_ex", "gm_pip_index_create_ex", True, _index_build_case("gm_pip_index_create_ex"))
add("gm_pip_index_create_arrow", "gm_pip_index_create_arrow", True, _index_build_case("gm_pip_index_create_arrow"))
add("gm_pip_index_transfer", ("gm_pip_index_export", "gm_pip_index_copy_array", "gm_pip_index_import"), True,
    _index_build_case("transfer"))


@functools.lru_cache(maxsize=None)
def _relate_polys():
    from geomesa_amd.join import synthetic_counties
    from test_gpu_relate import NX, NY
    return synthetic_counties(NX, NY)


def _relate_case(scale):
    from test_gpu_relate import rows
    n = 2 * 2048 + 5      # k_pip_relate: RTPB 1024 x RILP 2 rows per block

    def ins(seed):
        poly, px, py = rows(_relate_polys(), n, 31 + seed)
        return {"poly": np.asarray(poly[:n], I32), "px": px[:n], "py": py[:n]}

    def expect(O, d):
        ops = O.OraclePolySet(*_relate_polys().to_arrays())
        loc = np.array([255 if p < 0 else ops.locate(int(p), x, y) for p, x, y in zip(d["poly"], d["px"], d["py"])], U8)
        return {"dev": {"loc": loc}, "elems": np.stack([loc.astype(I64), d["poly"].astype(I64)], 1)}

    def prepare():
        from geomesa_amd.join import PolygonIndex
        gpu_object("relate_ix", lambda: PolygonIndex(_relate_polys()))
    return Case(ins, {"loc": n},
                lambda lib, h, p, host: lib.gm_pip_relate(h, _GPU["relate_ix"]._h, p["poly"], p["px"], p["py"], n, p["loc"]),
                expect, prepare)


add("gm_pip_relate", "gm_pip_relate", False, _relate_case)      # :415 "Stream-ordered"


# ---------------------------------------------------------------- key table
def _key_bytes_case(k3):
    def factory(scale):
        n = 2 * 256 + 5      # k_key_bytes: STPB = 256 rows per block

        def ins(seed):
            sh, b, z = C._key_cols(n, 600 + seed)
            return {"shard": sh, "bin": b, "z": z}

        def expect(O, d):
            parts = [d["shard"].reshape(-1, 1)] + ([d["bin"].astype(">i2").view(U8).reshape(-1, 2)] if k3 else []) + \
                [d["z"].astype(">i8").view(U8).reshape(-1, 8)]
            rows = np.ascontiguousarray(np.concatenate(parts, 1))
            return {"dev": {"out": rows}, "elems": rows}

        def call(lib, h, p, host):
            if k3:
                return lib.gm_z3_key_bytes(h, p["shard"], p["bin"], p["z"], n, p["out"])
            return lib.gm_z2_key_bytes(h, p["shard"], p["z"], n, p["out"])
        return Case(ins, {"out": n * (11 if k3 else 9)}, call, expect)
    return factory


add("gm_z3_key_bytes", "gm_z3_key_bytes", False, _key_bytes_case(True))     # :29-31 "only enqueue work ... and return"
add("gm_z2_key_bytes", "gm_z2_key_bytes", False, _key_bytes_case(False))


def _sort_case(scale):
    import table_scan_cases as TS
    n = (2 * 4096 + 5) * scale

    def ins(seed):
        sh, b, z = C._key_cols(n, 700 + seed)
        return {"shard": sh, "bin": b, "z": z}

    def expect(O, d):
        order = TS.table_order(d["shard"], d["bin"], d["z"])
        return {"dev": {"shard_out": d["shard"][order], "bin_out": d["bin"][order], "z_out": d["z"][order],
                        "perm": np.asarray(order, I64)}, "elems": np.asarray(order, I64)}
    return Case(ins, {"shard_out": n, "bin_out": 2 * n, "z_out": 8 * n, "perm": 8 * n},
                lambda lib, h, p, host: lib.gm_sort_keys(h, p["shard"], p["bin"], p["z"], n, p["shard_out"], p["bin_out"],
                                                         p["z_out"], p["perm"]), expect)


add("gm_sort_keys", "gm_sort_keys", True, _sort_case)     # :509 "Synchronises the context stream"


def _sample_case(scale):
    n, ns = 2 * 4096 + 5, 101

    def ins(seed):
        sh, b, z = C._key_cols(n, 800 + seed)
        return {"shard": sh, "bin": b, "z": z}

    def call(lib, h, p, host):
        host["hi"], host["lo"] = np.full(ns, 7, U64), np.full(ns, 7, U64)
        return lib.gm_key_sample(h, p["shard"], p["bin"], p["z"], n, ns, host["hi"].ctypes.data, host["lo"].ctypes.data)

    def expect(O, d):
        rows = [(2 * i + 1) * n // (2 * ns) for i in range(ns)]
        hi, lo = O.table_key_u64(d["shard"], d["bin"], d["z"])
        return {"dev": {}, "host": {"hi": hi[rows], "lo": lo[rows]}, "elems": lo[rows]}
    return Case(ins, {}, call, expect)


add("gm_key_sample", "gm_key_sample", True, _sample_case)      # :521 "Synchronises the context stream"


def _partition_case(scale):
    n = (2 * 2048 + 5) * scale      # XTILE = 2048 rows per tile

    def splitters(O):
        hi, lo = O.table_key_u64(*C._key_cols(64, 99))
        k = np.lexsort((lo, hi))[[10, 30, 30, 50]]
        return np.ascontiguousarray(hi[k]), np.ascontiguousarray(lo[k])

    def ins(seed):
        sh, b, z = C._key_cols(n, 900 + seed)
        return {"shard": sh, "bin": b, "z": z}

    def call(lib, h, p, host):
        import oracle as O
        host["sp"] = splitters(O)
        host["counts"] = np.full(5, -7, I64)
        return lib.gm_key_partition(h, p["shard"], p["bin"], p["z"], n, host["sp"][0].ctypes.data, host["sp"][1].ctypes.data,
                                    4, None, 1000, p["shard_out"], p["bin_out"], p["z_out"], p["ids_out"], p["rows_out"],
                                    host["counts"].ctypes.data)

    def expect(O, d):
        order, counts = O.key_partition(d["shard"], d["bin"], d["z"], *splitters(O))
        return {"dev": {"shard_out": d["shard"][order], "bin_out": d["bin"][order], "z_out": d["z"][order],
                        "ids_out": np.asarray(order + 1000, I64), "rows_out": np.asarray(order, U32)},
                "host": {"counts": np.asarray(counts, I64)}, "elems": np.asarray(order, I64)}
    return Case(ins, {"shard_out": n, "bin_out": 2 * n, "z_out": 8 * n, "ids_out": 8 * n, "rows_out": 4 * n}, call, expect)


add("gm_key_partition", "gm_key_partition", True, _partition_case)     # :530 "Synchronises the context stream"


def _table_scan_case(entry):
    """A sorted table is structural (the same keys in A and B); the decoy differs in perm and in the full
    filter's columns, so ids and, with the filter, the matches themselves differ."""
    def factory(scale):
        import table_scan_cases as TS
        n = (2 * 4096 + 5) * scale
        box = np.array([-180.0, -90.0, 0.0, 90.0])

        @functools.lru_cache(maxsize=None)
        def table():
            sh, b, z = C._key_cols(n, 1000)
            order = TS.table_order(sh, b, z)
            sh, b, z = sh[order], b[order], z[order]
            keys = TS.keys80(sh, b, z)
            rs = TS.random_ranges(np.random.default_rng(3), keys, 12 * scale)
            return sh, b, z, np.ascontiguousarray(TS.ranges_array(rs), _lib.KEY_RANGE_DTYPE)

        def ins(seed):
            sh, b, z, _ = table()
            rng = np.random.default_rng(1100 + seed)
            d = {"shard": sh, "bin": b, "z": z, "perm": rng.permutation(n).astype(I64)}
            if entry != "gm_key_range_scan":
                d["x"], d["y"] = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
            if entry == "gm_table_scan_geom":
                d["yx"] = C.interleave_yx(d["x"], d["y"])
            return d

        def call(lib, h, p, host):
            arr = table()[3]
            host["n_match"], host["n_scanned"], host["n_env"] = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
            nm, ns = ctypes.byref(host["n_match"]), ctypes.byref(host["n_scanned"])
            if entry == "gm_key_range_scan":
                return lib.gm_key_range_scan(h, p["shard"], p["bin"], p["z"], n, arr.ctypes.data, len(arr), None, 0, p["perm"],
                                             p["ids"], n, nm, ns)
            f = _lib.ScanFilter()
            f.xmin, f.ymin, f.xmax, f.ymax = p["x"].value, p["y"].value, p["x"].value, p["y"].value
            f.boxes, f.n_boxes = box.ctypes.data, 1
            host["f"] = f
            if entry == "gm_table_scan":
                return lib.gm_table_scan(h, p["shard"], p["bin"], p["z"], n, arr.ctypes.data, len(arr), ctypes.byref(f),
                                         p["perm"], p["ids"], n, nm, ns)
            host["g"] = C.point_struct(None)
            host["g"].coords = p["yx"].value
            return lib.gm_table_scan_geom(h, p["shard"], p["bin"], p["z"], n, arr.ctypes.data, len(arr), ctypes.byref(f),
                                          ctypes.byref(host["g"]), p["perm"], p["ids"], n, nm, ns, ctypes.byref(host["n_env"]))

        def expect(O, d):
            sh, b, z, arr = table()
            cand = np.asarray(O.table_scan_rows(sh, b, z, arr), bool)
            keep = cand
            if entry != "gm_key_range_scan":
                full = np.asarray(O.envelope_scan(d["x"], d["y"], d["x"], d["y"], box.reshape(1, 4)), bool)
                keep = cand & full[d["perm"]]
            ids = d["perm"][np.flatnonzero(keep)]
            assert n // 16 < len(ids) < n
            host = {"n_match": len(ids), "n_scanned": int(cand.sum())}
            if entry == "gm_table_scan_geom":
                host["n_env"] = len(ids)      # a point's envelope test is its geometry test
            return {"dev": {"ids": ids}, "host": host, "elems": np.where(keep, d["perm"], -1)[cand]}
        return Case(ins, {"ids": 8 * n}, call, expect)
    return factory


for _e in ("gm_key_range_scan", "gm_table_scan", "gm_table_scan_geom"):
    add(_e, _e, True, _table_scan_case(_e))      # :556, :602, :620 "Synchronises"


# ---------------------------------------------------------------- Arrow adapters
def _points_to_columns_case(scale):
    n = 2 * 256 + 5

    def ins(seed):
        rng = np.random.default_rng(1200 + seed)
        return {"yx": C.interleave_yx(rng.uniform(-180, 180, n), rng.uniform(-90, 90, n))}

    def call(lib, h, p, host):
        host["g"] = C.point_struct(None)
        host["g"].coords = p["yx"].value
        return lib.gm_arrow_points_to_columns(h, ctypes.byref(host["g"]), n, p["x"], p["y"])
    return Case(ins, {"x": 8 * n, "y": 8 * n}, call,
                lambda O, d: {"dev": {"x": d["yx"][1::2].copy(), "y": d["yx"][0::2].copy()}, "elems": d["yx"][1::2].view(I64)})


add("gm_arrow_points_to_columns", "gm_arrow_points_to_columns", False, _points_to_columns_case)   # :29-31


def _line_column(p, host, n_slots, multi):
    """gm_geom_column of a LineString column (4 vertices per line) or a MultiLineString one (2 lines per slot)."""
    from geomesa_amd.arrow import GeomColumnC
    offs = [p["slot_off"].value, p["line_off"].value, None] if multi else [p["line_off"].value, None, None]
    host["g"] = GeomColumnC(4 if multi else 1, 64, 0, 0, p["yx"].value, None, 0, (ctypes.c_void_p * 3)(*offs))
    return ctypes.byref(host["g"])


def _lines(seed, n_lines, env, multi):
    """n_lines lines of 4 vertices over env and a margin: (device inputs, rows as the line references take them)."""
    rng = np.random.default_rng(1300 + seed)
    w, h = env[2] - env[0], env[3] - env[1]
    x = rng.uniform(env[0] - 0.1 * w, env[2] + 0.1 * w, 4 * n_lines)
    y = rng.uniform(env[1] - 0.1 * h, env[3] + 0.1 * h, 4 * n_lines)
    d = {"yx": C.interleave_yx(x, y), "line_off": (4 * np.arange(n_lines + 1)).astype(I32)}
    rows = [[(float(x[4 * r + v]), float(y[4 * r + v])) for v in range(4)] for r in range(n_lines)]
    if multi:
        d["slot_off"] = (2 * np.arange(n_lines // 2 + 1)).astype(I32)
        rows = [rows[2 * r:2 * r + 2] for r in range(n_lines // 2)]
    d["_rows"] = rows
    return d


def _envelopes_case(scale):
    n = 2 * 256 + 5
    env = (-170.0, -80.0, 170.0, 80.0)

    def expect(O, d):
        x, y = d["yx"][1::2].reshape(n, 4), d["yx"][0::2].reshape(n, 4)
        dev = {"xmin": x.min(1), "ymin": y.min(1), "xmax": x.max(1), "ymax": y.max(1)}
        return {"dev": dev, "elems": np.stack([v.view(I64) for v in dev.values()], 1)}
    return Case(lambda seed: _lines(seed, n, env, False), {k: 8 * n for k in ("xmin", "ymin", "xmax", "ymax")},
                lambda lib, h, p, host: lib.gm_arrow_envelopes(h, _line_column(p, host, n, False), n, p["xmin"], p["ymin"],
                                                               p["xmax"], p["ymax"]), expect)


add("gm_arrow_envelopes", "gm_arrow_envelopes", False, _envelopes_case)      # :475 "Asynchronous"


# ---------------------------------------------------------------- accumulating stats: the outputs are refilled with zero
def _hist_case(scale):
    n = C.HIST_N
    length, lo, nb = C.HIST_SHAPES["lds"]

    def ins(seed):
        x, y, t = C.xyt_ms(np.random.default_rng(1400 + seed), n)
        return {"x": x, "y": y, "t": t}
    init = {"present": np.zeros(nb, U8), "counts": np.zeros((nb, length), I64), "tally": np.zeros(2, I64)}

    def expect(O, d):
        p, c, t = O.z3_histogram(d["x"], d["y"], d["t"], length, lo, nb, period=WEEK, present=init["present"].copy(),
                                 counts=init["counts"].copy(), tally=init["tally"].copy())
        return {"dev": {"present": np.asarray(p, U8), "counts": np.asarray(c, I64), "tally": np.asarray(t, I64)},
                "elems": np.asarray(c, I64).reshape(-1), "counters": True}
    return Case(ins, init, lambda lib, h, p, host: lib.gm_z3_histogram(h, p["x"], p["y"], p["t"], n, WEEK, length, 0, lo, nb,
                                                                      p["present"], p["counts"], p["tally"]), expect)


add("gm_z3_histogram", "gm_z3_histogram", False, _hist_case)      # :655 "asynchronous on the context stream"

DENS_ENV, DENS_W, DENS_H = (-180.0, -90.0, 180.0, 90.0), 256, 256


def _grid_c(env, w, h):
    return _lib.DensityGrid(env[0], env[1], env[2], env[3], w, h, 0, 0)


def _density_case(entry):
    def factory(scale):
        import density_ref as R
        n = 2 * DENSITY_BLOCK + 5

        def ins(seed):
            from test_gpu_density import random_points
            x, y = random_points(DENS_ENV, n, 1500 + seed)
            return {"yx": C.interleave_yx(x, y)} if entry == "gm_density_arrow" else {"x": x, "y": y}
        init = {"grid": np.zeros((DENS_H, DENS_W), F64), "tally": np.zeros(3, I64)}

        def call(lib, h, p, host):
            host["gd"] = _grid_c(DENS_ENV, DENS_W, DENS_H)
            if entry == "gm_density_points":
                return lib.gm_density_points(h, p["x"], p["y"], None, n, None, None, 0, ctypes.byref(host["gd"]), p["grid"],
                                             p["tally"])
            host["g"] = C.point_struct(None)
            host["g"].coords = p["yx"].value
            return lib.gm_density_arrow(h, ctypes.byref(host["g"]), None, n, None, None, 0, ctypes.byref(host["gd"]), p["grid"],
                                        p["tally"])

        def expect(O, d):
            x, y = (d["yx"][1::2], d["yx"][0::2]) if entry == "gm_density_arrow" else (d["x"], d["y"])
            grid, tally = R.render_numpy(DENS_ENV, DENS_W, DENS_H, x, y)
            return {"dev": {"grid": np.asarray(grid, F64), "tally": np.asarray(tally, I64)},
                    "elems": np.asarray(grid, F64).reshape(-1), "counters": True}
        return Case(ins, init, call, expect)
    return factory


add("gm_density_points", "gm_density_points", False, _density_case("gm_density_points"))    # :708 "the call is stream-ordered"
add("gm_density_arrow", "gm_density_arrow", False, _density_case("gm_density_arrow"))       # :721 as gm_density_points

LINE_ENV, LINE_W, LINE_H = (-1.0, 33.0, 6.0, 40.0), 64, 64


def _density_lines_case(multi):
    def factory(scale):
        import density_lines_ref as L
        n_lines = 2 * 1024 + 6      # one lane per segment: 3 x 2054 = 6 blocks of DTPB 1024 lanes + 18; even: slots pair up
        n = n_lines // 2 if multi else n_lines
        init = {"grid": np.zeros((LINE_H, LINE_W), F64), "tally": np.zeros(3, I64)}

        def call(lib, h, p, host):
            host["gd"] = _grid_c(LINE_ENV, LINE_W, LINE_H)
            return lib.gm_density_lines(h, _line_column(p, host, n, multi), None, n, None, None, 0, ctypes.byref(host["gd"]),
                                        p["grid"], p["tally"])

        def expect(O, d):
            grid, tally = L.render_lines_numpy(LINE_ENV, LINE_W, LINE_H, d["_rows"])
            return {"dev": {"grid": np.asarray(grid, F64), "tally": np.asarray(tally, I64)},
                    "elems": np.asarray(grid, F64).reshape(-1), "counters": True}
        return Case(lambda seed: _lines(seed, n_lines, LINE_ENV, multi), init, call, expect)
    return factory


add("gm_density_lines", "gm_density_lines", False, _density_lines_case(False))           # :729 "Stream-ordered"
# :729-730 "a GM_GEOM_MULTILINESTRING call waits for the stream once" (DESIGN documents the same wait)
add("gm_density_lines[multi]", "gm_density_lines", True, _density_lines_case(True))


def _sparse_case(scale):
    w, h = 97, 85      # 8245 cells = 2 x SP_CELLS (gm_density.hip: SCAN_TPB 256 x SP_PER 16 = 4096) + 53

    def ins(seed):
        rng = np.random.default_rng(1600 + seed)
        g = np.where(rng.random((h, w)) < 0.3, rng.integers(1, 50, (h, w)), 0).astype(F64)
        return {"grid": g}
    cap = w * h

    def call(lib, h_, p, host):
        host["n_cells"] = ctypes.c_int64(-7)
        return lib.gm_density_sparse(h_, p["grid"], w, h, cap, p["i"], p["j"], p["w"], ctypes.byref(host["n_cells"]))

    def expect(O, d):
        i, j = np.nonzero(d["grid"].T)      # ordered by column i, then row j
        return {"dev": {"i": i.astype(I32), "j": j.astype(I32), "w": d["grid"].T[i, j].copy()},
                "host": {"n_cells": len(i)}, "elems": d["grid"].reshape(-1), "counters": True}
    return Case(ins, {"i": 4 * cap, "j": 4 * cap, "w": 8 * cap}, call, expect)


add("gm_density_sparse", "gm_density_sparse", True, _sparse_case)      # :786 "Synchronises the context stream"


# ---------------------------------------------------------------- BIN
def _bin_attr_case(label):
    def factory(scale):
        n = 2 * 256 + 5      # one lane per slot (:817), 256-thread blocks

        def ins(seed):
            return {"v": np.random.default_rng(1700 + seed).integers(-2**63, 2**63 - 1, n, dtype=I64)}

        def call(lib, h, p, host):
            host["col"] = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, p["v"].value, None, None, 0)
            f = lib.gm_bin_label if label else lib.gm_bin_track
            return f(h, ctypes.byref(host["col"]), n, p["out"])

        def expect(O, d):
            v = d["v"]
            want = v if label else (v ^ (v.view(U64) >> np.uint64(32)).view(I64)).astype(I32)     # Long.hashCode
            return {"dev": {"out": want}, "elems": np.asarray(want, I64)}
        return Case(ins, {"out": n * (8 if label else 4)}, call, expect)
    return factory


add("gm_bin_track", "gm_bin_track", False, _bin_attr_case(False))      # :817 "stream-ordered"
add("gm_bin_label", "gm_bin_label", False, _bin_attr_case(True))


def _bin_cols(seed):
    from test_gpu_bin import columns
    return columns(2 * BIN_BLOCK + 5, 5 + seed)


def _bin_encode_case(entry):
    def factory(scale):
        import bin_ref as R
        n = 2 * BIN_BLOCK + 5

        def ins(seed):
            x, y, t, track, label = _bin_cols(seed)
            d = {"t": t, "track": track, "label": label}
            d.update({"yx": C.interleave_yx(x, y)} if entry == "gm_bin_arrow" else {"x": x, "y": y})
            return d

        def call(lib, h, p, host):
            host["o"], host["n_records"] = _lib.BinOpts(0, 0), ctypes.c_int64(-7)
            if entry == "gm_bin_points":
                return lib.gm_bin_points(h, p["x"], p["y"], p["t"], p["track"], p["label"], n, None, None, 0,
                                         ctypes.byref(host["o"]), p["out"], n, ctypes.byref(host["n_records"]), p["tally"])
            host["g"] = C.point_struct(None)
            host["g"].coords = p["yx"].value
            host["dtg"] = C.time_struct(None)
            host["dtg"].millis = p["t"].value
            return lib.gm_bin_arrow(h, ctypes.byref(host["g"]), ctypes.byref(host["dtg"]), None, None, p["track"], p["label"], n,
                                    None, None, 0, ctypes.byref(host["o"]), p["out"], n, ctypes.byref(host["n_records"]),
                                    p["tally"])

        def expect(O, d):
            from test_gpu_bin import features
            x, y = (d["yx"][1::2], d["yx"][0::2]) if entry == "gm_bin_arrow" else (d["x"], d["y"])
            data, tally = R.scan(features(x, y, d["t"], d["track"], d["label"]), label=True)
            rec = np.frombuffer(data, U8).reshape(n, 24)
            return {"dev": {"out": rec, "tally": np.asarray(tally, I64)}, "host": {"n_records": n}, "elems": rec}
        return Case(ins, {"out": 24 * n, "tally": np.zeros(3, I64)}, call, expect)
    return factory


add("gm_bin_points", "gm_bin_points", True, _bin_encode_case("gm_bin_points"))    # :861 "synchronises the context stream"
add("gm_bin_arrow", "gm_bin_arrow", True, _bin_encode_case("gm_bin_arrow"))       # :874 as gm_bin_points


def _bin_sort_case(scale):
    import bin_ref as R
    n = 2 * BIN_BLOCK + 5

    def ins(seed):
        rng = np.random.default_rng(1800 + seed)
        rec = rng.integers(0, 256, (n, 16), dtype=U8)
        rec[:, 4:8] = rng.integers(-500, 500, n).astype("<i4").view(U8).reshape(n, 4)     # many equal seconds: ties
        return {"in": rec}

    def expect(O, d):
        want = np.frombuffer(R.stable_sort_np(d["in"].tobytes(), 16), U8).reshape(n, 16)
        return {"dev": {"out": want}, "elems": want}
    return Case(ins, {"out": 16 * n}, lambda lib, h, p, host: lib.gm_bin_sort(h, p["in"], n, 16, p["out"]), expect)


add("gm_bin_sort", "gm_bin_sort", True, _bin_sort_case)      # :889-890 "Synchronises the context stream, as gm_sort_keys"


# ---------------------------------------------------------------- Frequency / Z3Frequency
def _cms():
    import frequency_ref as R
    c = _lib.Cms(5, 400, W2020, 54, 0, 0)
    for i, a in enumerate(R.hash_a(5)):
        c.hash_a[i] = a
    return c


def _sketches():
    import frequency_ref as R
    return R.Sketches(5, 400, W2020, 54)


def _freq_case(entry):
    def factory(scale):
        n = 2 * FREQ_BLOCK + 5

        def ins(seed):
            rng = np.random.default_rng(1900 + seed)
            x, y, t = C.xyt_ms(rng, n)
            if entry == "gm_frequency_attr":
                return {"v": rng.integers(-10**6, 10**6, n), "t": t}
            return {"x": x, "y": y, "t": t}
        init = {"table": np.zeros((54, 5, 400), I64), "size": np.zeros(54, I64), "tally": np.zeros(3, I64)}

        def call(lib, h, p, host):
            host["cms"] = _cms()
            host["dtg"] = C.time_struct(None)
            host["dtg"].millis = p["t"].value
            tail = (ctypes.byref(host["cms"]), p["table"], p["size"], p["tally"])
            if entry == "gm_z3_frequency":
                return lib.gm_z3_frequency(h, p["x"], p["y"], p["t"], n, None, None, 0, WEEK, 25, *tail)
            if entry == "gm_frequency_points":
                return lib.gm_frequency_points(h, p["x"], p["y"], ctypes.byref(host["dtg"]), n, None, None, 0, WEEK, 25, *tail)
            host["col"] = _lib.AttrColumn(_lib.GM_ATTR_INT64, 0, p["v"].value, None, None, 0)
            return lib.gm_frequency_attr(h, ctypes.byref(host["col"]), ctypes.byref(host["dtg"]), n, None, None, 0, WEEK, 7, *tail)

        def expect(O, d):
            s = _sketches()
            if entry == "gm_z3_frequency":
                s.observe_z3(O, d["x"], d["y"], d["t"], WEEK, 25)
            elif entry == "gm_frequency_points":
                s.observe_points(O, d["x"], d["y"], 25, d["t"], WEEK)
            else:
                s.observe_attr(O, "long", d["v"], 7, d["t"], WEEK)
            assert s.size.sum() > n // 2
            return {"dev": {"table": s.table, "size": s.size, "tally": s.tally}, "elems": s.table.reshape(-1),
                    "counters": True}
        return Case(ins, init, call, expect)
    return factory


for _e in ("gm_z3_frequency", "gm_frequency_attr", "gm_frequency_points"):
    add(_e, _e, False, _freq_case(_e))      # :932-933 "the call is stream-ordered" (:961, :973 "as gm_z3_frequency")


def _estimate_case(scale):
    n = 2 * 256 + 5

    def ins(seed):
        rng = np.random.default_rng(2000 + seed)
        table = rng.integers(0, 1000, (54, 5, 400))
        return {"table": table, "keys": rng.integers(-2**62, 2**62, n)}

    def call(lib, h, p, host):
        host["cms"] = _cms()
        return lib.gm_cms_estimate(h, ctypes.byref(host["cms"]), p["table"], p["keys"], None, n, p["out"])

    def expect(O, d):
        s = _sketches()
        s.table = d["table"]
        want = np.asarray(s.estimate(d["keys"]), I64)
        return {"dev": {"out": want}, "elems": want}
    return Case(ins, {"out": 8 * n}, call, expect)


add("gm_cms_estimate", "gm_cms_estimate", False, _estimate_case)      # :980 "Stream-ordered"

# the cases whose temporaries come from a context workspace (gm_internal.hpp:67-72) or the stream's pool: run at
# 8n, n, 8n on one context by test_workspace_reuse
WORKSPACE_USERS = [k for k in TABLE if k.split("[")[0].split("+")[0] in (
    "gm_z3filter_scan", "gm_z2filter_scan", "gm_z3filter_scan_rows", "gm_z2filter_scan_rows", "gm_strict_scan",
    "gm_query_scan", "gm_sort_keys", "gm_pip_join", "gm_pip_join_pred", "gm_key_partition", "gm_key_range_scan",
    "gm_table_scan", "gm_z3_ranges", "gm_z2_ranges", "gm_zranges", "gm_xz2_ranges", "gm_xz3_ranges")]


def covered_entries():
    return {e for entries, _, _ in TABLE.values() for e in entries}
