"""Guarded device buffers for the C-ABI tests (test_gpu_abi_contract.py).

One device byte tensor filled with 0xA5 holds a payload with a guard on both sides.  The payload starts at
a chosen byte offset from a 256-B boundary, so a test decides the alignment of every pointer it passes.
Guard and payload share one allocation: a kernel that writes past its output changes a byte of this
tensor (check() sees it) and never touches memory the test does not own.
"""
import ctypes

import numpy as np

FILL = 0xA5
GUARD = 4096      # bytes on each side, at least
BOUNDARY = 256


class Guarded:
    """nbytes of device memory at `offset` bytes past a 256-B boundary, `guard` bytes of 0xA5 on both sides."""

    def __init__(self, nbytes, offset=0, guard=GUARD):
        import torch
        assert 0 <= offset < BOUNDARY and guard >= GUARD
        self.nbytes = int(nbytes)
        self.buf = torch.full((guard + 2 * BOUNDARY + self.nbytes + guard,), FILL, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        start = -(-(base + guard) // BOUNDARY) * BOUNDARY + offset
        self.lo = start - base
        self.hi = self.lo + self.nbytes
        assert self.lo >= guard and self.buf.numel() - self.hi >= guard
        self.addr = start

    @classmethod
    def of(cls, arr, offset=0, guard=GUARD):
        """A guarded copy of a numpy array."""
        arr = np.ascontiguousarray(arr)
        g = cls(arr.nbytes, offset, guard)
        g.write(arr)
        return g

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def write(self, arr):
        import torch
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        if b.size:
            self.buf[self.lo:self.hi].copy_(torch.from_numpy(b.copy()))

    def read(self, dtype=np.uint8):
        """The payload as a host array of `dtype` (synchronises)."""
        return self.buf[self.lo:self.hi].cpu().numpy().view(dtype)

    def check(self, what=""):
        """Both guards still hold 0xA5."""
        h = self.buf.cpu().numpy()
        bad = np.flatnonzero(np.concatenate([h[:self.lo], h[self.hi:]]) != FILL)
        if bad.size:
            pos = int(bad[0])
            where = "%d B before the payload" % (self.lo - pos) if pos < self.lo else \
                "%d B past the payload's end" % (pos - self.lo)
            raise AssertionError("%s: guard overwritten (%d bytes, first %s)" % (what, bad.size, where))


def untouched(a):
    """True where every byte of the (host) array still holds the 0xA5 fill."""
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))
