"""Device buffers for GPU tests, through the C ABI's own allocator (no torch),
and Guarded: an output buffer between two guard bands."""
import ctypes as C

import numpy as np

from immustore_amd import _native as N

GUARD = 4096
FILL = 0xA5


class DevBuf:
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        N.check(N.load().mh_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_host(cls, ctx, arr):
        a = np.ascontiguousarray(arr)
        b = cls(ctx, a.nbytes)
        if a.nbytes:
            N.check(N.load().mh_memcpy_h2d(ctx.handle, b.ptr, a.ctypes.data, a.nbytes))
            ctx.synchronize()
        return b

    def to_host(self, dtype=np.uint8, count=None):
        count = self.nbytes // np.dtype(dtype).itemsize if count is None else count
        out = np.zeros(max(count, 1), dtype)
        nb = count * np.dtype(dtype).itemsize
        if nb:
            N.check(N.load().mh_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, nb))
            self.ctx.synchronize()
        return out[:count]

    def free(self):
        if self.ptr:
            N.load().mh_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Guarded:
    """nbytes of memory filled with 0xA5 between two 4096-byte guards, all in
    one allocation: the payload never touches either end of it, so a write past
    the payload lands in a guard and is seen, not faulted on.

    offset (bytes, below 4096) moves the payload that far into the allocation,
    for the alignment cases; the bytes skipped belong to the front guard.
    pinned=False: device memory (a torch tensor, filled on torch's stream:
    synchronise before a call on another stream).  pinned=True: page-locked
    host memory from mh_host_alloc_pinned, which kernels write directly."""

    def __init__(self, nbytes, offset=0, pinned=False):
        self.n = int(nbytes)
        self.offset = int(offset)
        assert 0 <= self.offset < GUARD
        self.lo = GUARD + self.offset          # the payload is [lo, lo + n) of the allocation
        self.size = self.lo + self.n + GUARD
        self.pinned = pinned
        self._hp = None
        if pinned:
            p = C.c_void_p()
            N.check(N.load().mh_host_alloc_pinned(self.size, C.byref(p)))
            self._hp = p.value
            self.t = np.ctypeslib.as_array((C.c_uint8 * self.size).from_address(p.value))
            self.t[:] = FILL
            base = p.value
        else:
            import torch
            self.t = torch.full((self.size,), FILL, dtype=torch.uint8, device="cuda")
            base = self.t.data_ptr()
        assert base % 16 == 0
        self.ptr = base + self.lo
        assert self.ptr % 16 == self.offset % 16

    def _all_fill(self, a, b):
        v = self.t[a:b] == FILL
        return bool(v.all()) if self.pinned else bool(v.all().item())

    def _host(self, a, b):
        return np.array(self.t[a:b]) if self.pinned else self.t[a:b].cpu().numpy()

    def payload(self):
        """The payload's bytes, copied to host memory."""
        return self._host(self.lo, self.lo + self.n)

    def rows(self):
        return self.payload().reshape(-1, 32)

    def view(self, dtype):
        return self.payload().view(dtype)

    def put(self, arr):
        """Host bytes into the start of the payload (for inputs placed at an offset)."""
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert a.size <= self.n
        if self.pinned:
            self.t[self.lo:self.lo + a.size] = a
        else:
            import torch
            self.t[self.lo:self.lo + a.size] = torch.from_numpy(a.copy()).cuda()

    def front_intact(self):
        return self._all_fill(0, self.lo)

    def back_intact(self):
        return self._all_fill(self.lo + self.n, self.size)

    def guards_intact(self):
        return self.front_intact() and self.back_intact()

    def untouched(self):
        return self._all_fill(0, self.size)

    def free(self):
        if self._hp:
            self.t = None
            N.load().mh_host_free_pinned(self._hp)
            self._hp = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
