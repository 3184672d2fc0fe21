"""Python mirror of the leader's side of replication (C ABI
mh_export_tx_batch): what ImmuStore.ExportTx (immustore.go:2621-2770) returns
for a run of consecutive txs of a store whose tx log, commit log and value
logs are resident on the device, in one device pass.  The blobs are the bytes
replicate.replicate_tx_batch takes.

Everything runs in libimmustore_merkle.so on the context's device; there is no
CPU path.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .merkle import Context, _addr, default_context


class _Vlog(C.Structure):  # mh_export_vlog
    _fields_ = [("data", C.c_void_p), ("first_off", C.c_uint64), ("end_off", C.c_uint64)]


class _Store(C.Structure):  # mh_export_store
    _fields_ = [("txlog", C.c_void_p), ("txlog_len", C.c_uint64), ("clog", C.c_void_p),
                ("ntx", C.c_uint64), ("clog_entry_size", C.c_uint32), ("max_entries", C.c_uint32),
                ("max_key_len", C.c_uint32), ("vlogs", C.c_void_p), ("nvlogs", C.c_uint32)]


class ExportStore:
    """The tx log (data after its appendable header), its commit log (ntx
    entries of 12 or 44 bytes) and the value logs on the context's device.
    vlogs[k] is value log k + 1: its bytes, or (first_off, bytes) for a window
    whose first byte is the log's byte first_off.  Everything is copied into
    allocations of the context, the tx log's and every value log's with the 256
    bytes of slack the kernels' block reads need."""

    def __init__(self, txlog: bytes, clog: bytes, vlogs=(), clog_entry_size: int = 12, *,
                 ctx: Context = None, max_entries: int = 1024, max_key_len: int = 1024):
        self._lib, self._ctx = N.load(), ctx or default_context()
        self.txlog_len, self.es = len(txlog), clog_entry_size
        self.ntx = len(clog) // clog_entry_size
        self.max_entries, self.max_key_len = max_entries, max_key_len
        self._bufs = []
        self._txlog = self._put(txlog, 256)
        self._clog = self._put(clog, 0)
        self._vl = (_Vlog * max(len(vlogs), 1))()
        self.nvlogs = len(vlogs)
        for k, v in enumerate(vlogs):
            first, raw = v if isinstance(v, tuple) else (0, v)
            self._vl[k].data = self._put(raw, 256) if len(raw) else None
            self._vl[k].first_off, self._vl[k].end_off = first, first + len(raw)
        self._ctx.synchronize()

    def _put(self, raw, slack):
        p = C.c_void_p()
        N.check(self._lib.mh_dev_alloc(self._ctx.handle, max(len(raw) + slack, 1), C.byref(p)))
        self._bufs.append(p)
        if len(raw):
            a = np.frombuffer(raw, np.uint8)
            N.check(self._lib.mh_memcpy_h2d(self._ctx.handle, p.value, _addr(a), len(raw)))
            self._ctx.synchronize()  # (a is the only owner of a bytearray's view)
        return p.value

    @property
    def ctx(self) -> Context:
        return self._ctx

    def close(self):
        for p in self._bufs:
            if p.value and self._ctx.handle:  # (a closed context has nothing left to free through)
                self._lib.mh_dev_free(self._ctx.handle, p.value)
            p.value = None
        self._bufs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def descriptor(self) -> _Store:
        s = _Store()
        s.txlog, s.txlog_len, s.clog, s.ntx = self._txlog, self.txlog_len, self._clog, self.ntx
        s.clog_entry_size, s.max_entries, s.max_key_len = self.es, self.max_entries, self.max_key_len
        s.vlogs, s.nvlogs = C.addressof(self._vl), self.nvlogs
        return s


def export_tx_batch_raw(store: ExportStore, first_tx: int, count: int, out: int, out_cap: int):
    """The C call as it is: out an address (host or the context's device) ->
    (off[count + 1] uint64, status[count] int32, truncated[count] uint8)."""
    s = store.descriptor()
    off = np.zeros(count + 1, np.uint64)
    st = np.zeros(max(count, 1), np.int32)
    tr = np.zeros(max(count, 1), np.uint8)
    N.check(store._lib.mh_export_tx_batch(store.ctx.handle, C.addressof(s), first_tx, count, out, out_cap,
                                          _addr(off), _addr(st), _addr(tr)))
    return off, st[:count].copy(), tr[:count].copy()


def export_tx_batch(store: ExportStore, first_tx: int, count: int, *, out_cap=None, size_hint=None):
    """ExportTx of txs first_tx .. first_tx + count - 1 -> (blobs, status[count]
    int32, truncated[count] uint8, off[count + 1] uint64).  blobs[k] is b"" for
    a tx whose status is not MH_OK.  out_cap: the output capacity in bytes, as
    the C call takes it (blobs past it: MH_ERR_BUFFER_TOO_SMALL).  With out_cap
    None the output is sized by the call itself: a first call into size_hint
    bytes (0: only to learn off[count]; the values are hashed in it all the
    same), a second one when a blob did not fit."""
    def call(cap):
        out = np.zeros(max(cap, 1), np.uint8)
        return (out,) + export_tx_batch_raw(store, first_tx, count, _addr(out), cap)

    if out_cap is None:
        out, off, st, tr = call(int(size_hint or 0))
        if (st == N.MH_ERR_BUFFER_TOO_SMALL).any():
            out, off, st, tr = call(int(off[count]))
    else:
        out, off, st, tr = call(out_cap)
    blobs = [bytes(out[int(off[k]):int(off[k + 1])]) if st[k] == N.MH_OK else b"" for k in range(count)]
    return blobs, st, tr, off
