"""Python mirror of the server's side of the verified reads (C ABI
mh_verifiable_answer_pb_batch): whole schema.VerifiableTx and
schema.VerifiableEntry answers of a store resident on the device, in one
device pass.

  db.VerifiableTxByID (nil EntriesSpec)   pkg/database/database.go:1462-1528
  db.VerifiableSet, once committed        pkg/database/database.go:767-814
  db.VerifiableGet                        pkg/database/database.go:817-896
  ImmuStore.DualProof and its tx readers  immustore.go:2394-2562, tx_reader.go:69-101
  TxToProto / TxEntryToProto              pkg/api/schema/database_protoconv.go:27-67

tx_answers (mh_tx_answer_pb_batch) serves the same reads, and db.TxByID /
db.TxScan, under an EntriesSpec: db.serializeTx (database.go:1080-1231) with
ImmuStore.ReadValue (immustore.go:3149-3240) over an export.ExportStore.

Everything runs in libimmustore_merkle.so on the tree's device; there is no
CPU path.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .merkle import AHtree, _addr

MH_ANS_TX, MH_ANS_ENTRY = N.MH_ANS_TX, N.MH_ANS_ENTRY


class _Store(C.Structure):  # mh_answer_store
    _fields_ = [("txlog", C.c_void_p), ("txlog_len", C.c_uint64), ("clog", C.c_void_p),
                ("ntx", C.c_uint64), ("clog_entry_size", C.c_uint32), ("max_entries", C.c_uint32),
                ("max_key_len", C.c_uint32)]


class _Batch(C.Structure):  # mh_answer_batch
    _fields_ = [("n", C.c_uint64), ("kind", C.c_void_p), ("tx", C.c_void_p),
                ("prove_since", C.c_void_p), ("keys", C.c_void_p), ("key_off", C.c_void_p),
                ("entries", C.c_void_p), ("entry_off", C.c_void_p)]


class ResidentStore:
    """The tx log (data after its appendable header), its commit log (ntx
    entries of 12 or 44 bytes) and the ahtree over the Alh values, all on the
    tree's device.  The logs are copied into allocations of the context (the
    tx log's with the 256 bytes of slack the kernels' block reads need)."""

    def __init__(self, tree: AHtree, txlog: bytes, clog: bytes, clog_entry_size: int = 12, *,
                 max_entries: int = 1024, max_key_len: int = 1024):
        self.tree, self._lib, self._ctx = tree, N.load(), tree.ctx
        self.txlog_len, self.es = len(txlog), clog_entry_size
        self.ntx = len(clog) // clog_entry_size
        self.max_entries, self.max_key_len = max_entries, max_key_len
        self._txlog, self._clog = C.c_void_p(), C.c_void_p()
        N.check(self._lib.mh_dev_alloc(self._ctx.handle, len(txlog) + 256, C.byref(self._txlog)))
        N.check(self._lib.mh_dev_alloc(self._ctx.handle, max(len(clog), 1), C.byref(self._clog)))
        for dst, raw in ((self._txlog, txlog), (self._clog, clog)):
            if raw:
                a = np.frombuffer(raw, np.uint8)
                N.check(self._lib.mh_memcpy_h2d(self._ctx.handle, dst.value, _addr(a), len(raw)))
        self._ctx.synchronize()

    def close(self):
        for p in (self._txlog, self._clog):
            if p.value and self._ctx.handle:  # (a closed context has nothing left to free through)
                self._lib.mh_dev_free(self._ctx.handle, p.value)
            p.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def descriptor(self) -> _Store:
        s = _Store()
        s.txlog, s.txlog_len, s.clog, s.ntx = self._txlog.value, self.txlog_len, self._clog.value, self.ntx
        s.clog_entry_size, s.max_entries, s.max_key_len = self.es, self.max_entries, self.max_key_len
        return s


def _csr(blobs, n):
    off = np.zeros(n + 1, np.uint64)
    if n:
        off[1:] = np.cumsum([len(x) for x in blobs], dtype=np.uint64)
    flat = b"".join(bytes(x) for x in blobs)
    return (np.frombuffer(flat, np.uint8).copy() if flat else np.zeros(1, np.uint8)), off


def verifiable_answers(store: ResidentStore, kind, tx, prove_since, keys=None, entries=None, *,
                       out_cap=None, size_hint=None, arrays=None):
    """n requests -> (messages, status[n] int32, off[n + 1] uint64).  kind[p]:
    MH_ANS_TX (VerifiableTx{tx, dualProof}) or MH_ANS_ENTRY (VerifiableEntry{entry,
    verifiableTx, inclusionProof}); tx[p] the tx to read, prove_since[p] the
    client's state tx; keys[p] (ENTRY) the key as the tx stores it, entries[p]
    the marshalled schema.Entry to embed.  messages[p] is b"" for a request
    whose status is not MH_OK.  out_cap: the output capacity in bytes, as the
    C call takes it (messages past it: MH_ERR_BUFFER_TOO_SMALL).  With out_cap
    None the output is sized by the call itself, and that costs a whole device
    pass, the re-hash of every distinct tx included: a first call with capacity
    0 only to learn off[n], a second to write.  size_hint: an upper bound of
    the answers' bytes the caller knows (e.g. the last batch's off[n]): the
    first call then writes into that much, and a second one runs only if a
    message did not fit.  arrays: a function that places each request array
    (e.g. into pinned memory) before the call."""
    n = len(kind)
    kd = np.ascontiguousarray(kind, np.uint8)
    tx = np.ascontiguousarray(tx, np.uint64)
    ps = np.ascontiguousarray(prove_since, np.uint64)
    kb, ko = _csr(keys if keys is not None else [b""] * n, n)
    eb, eo = _csr(entries if entries is not None else [b""] * n, n)
    if arrays is not None:
        kd, tx, ps, kb, ko, eb, eo = (arrays(x) for x in (kd, tx, ps, kb, ko, eb, eo))
    b = _Batch()
    b.n, b.kind, b.tx, b.prove_since = n, _addr(kd), _addr(tx), _addr(ps)
    b.keys, b.key_off, b.entries, b.entry_off = _addr(kb), _addr(ko), _addr(eb), _addr(eo)
    s = store.descriptor()
    off = np.zeros(n + 1, np.uint64)
    st = np.zeros(max(n, 1), np.int32)
    L = N.load()

    def call(cap):
        out = np.zeros(max(cap, 1), np.uint8)
        N.check(L.mh_verifiable_answer_pb_batch(store.tree.handle, C.addressof(s), C.addressof(b),
                                                _addr(out), cap, _addr(off), _addr(st)))
        return out

    if out_cap is None:
        out = call(int(size_hint or 0))
        if (st[:n] == N.MH_ERR_BUFFER_TOO_SMALL).any():
            out = call(int(off[n]))
    else:
        out = call(out_cap)
    msgs = [bytes(out[int(off[p]):int(off[p + 1])]) if st[p] == N.MH_OK else b"" for p in range(n)]
    return msgs, st[:n].copy(), off


def VerifiableTxByID(store: ResidentStore, tx: int, prove_since_tx: int) -> bytes:
    """db.VerifiableTxByID with a nil EntriesSpec: the marshalled VerifiableTx."""
    msgs, st, _ = verifiable_answers(store, [MH_ANS_TX], [tx], [prove_since_tx])
    N.check(int(st[0]))
    return msgs[0]


def VerifiableGet(store: ResidentStore, tx: int, prove_since_tx: int, key: bytes,
                  entry: bytes = b"") -> bytes:
    """db.VerifiableGet once the index has named the tx: the marshalled
    VerifiableEntry around the caller's schema.Entry."""
    msgs, st, _ = verifiable_answers(store, [MH_ANS_ENTRY], [tx], [prove_since_tx], [key], [entry])
    N.check(int(st[0]))
    return msgs[0]


# ---------------------------------------------------------------- under an EntriesSpec
MH_TXA_TX, MH_TXA_VERIFIABLE, MH_TXA_NO_SPEC = N.MH_TXA_TX, N.MH_TXA_VERIFIABLE, N.MH_TXA_NO_SPEC
EXCLUDE, ONLY_DIGEST, RAW_VALUE, RESOLVE = 0, 1, 2, 3  # schema.EntryTypeAction


class _TxBatch(C.Structure):  # mh_tx_answer_batch
    _fields_ = [("n", C.c_uint64), ("kind", C.c_void_p), ("tx", C.c_void_p),
                ("prove_since", C.c_void_p), ("has_spec", C.c_void_p), ("kv_action", C.c_void_p),
                ("z_action", C.c_void_p), ("sql_action", C.c_void_p), ("now_unix", C.c_int64)]


def tx_answers_raw(store, tree, kind, tx, prove_since, specs, now_unix, out: int, out_cap: int):
    """The C call mh_tx_answer_pb_batch as it is: out an address (host or the
    context's device) -> (off[n + 1] uint64, status[n] int32).  store: an
    export.ExportStore; tree: the AHtree over its Alh values on the store's
    context, or None when no request is MH_TXA_VERIFIABLE; specs[p]: None
    (req.EntriesSpec is nil) or (kv, z, sql), each an EntryTypeAction value or
    None for a nil EntryTypeSpec."""
    n = len(kind)
    kd = np.ascontiguousarray(kind, np.uint8)
    txa = np.ascontiguousarray(tx, np.uint64)
    ps = np.ascontiguousarray(prove_since, np.uint64)
    hs = np.array([sp is not None for sp in specs], np.uint8)
    acts = np.full((3, max(n, 1)), MH_TXA_NO_SPEC, np.uint8)
    for p, sp in enumerate(specs):
        for k in range(3):
            if sp is not None and sp[k] is not None:
                acts[k, p] = sp[k]
    b = _TxBatch()
    b.n, b.kind, b.tx, b.prove_since, b.has_spec = n, _addr(kd), _addr(txa), _addr(ps), _addr(hs)
    b.kv_action, b.z_action, b.sql_action = (_addr(acts[k]) for k in range(3))
    b.now_unix = int(now_unix)
    s = store.descriptor()
    off = np.zeros(n + 1, np.uint64)
    st = np.zeros(max(n, 1), np.int32)
    N.check(N.load().mh_tx_answer_pb_batch(store.ctx.handle, tree.handle if tree is not None else None,
                                           C.addressof(s), C.addressof(b), out, out_cap, _addr(off),
                                           _addr(st)))
    return off, st[:n].copy()


def tx_answers(store, tree, kind, tx, prove_since, specs, now_unix, *, out_cap=None, size_hint=None):
    """db.TxByID / an item of db.TxScan (kind MH_TXA_TX: the marshalled
    schema.Tx) and db.VerifiableTxByID (MH_TXA_VERIFIABLE: the marshalled
    schema.VerifiableTx) under an EntriesSpec (db.serializeTx,
    pkg/database/database.go:1080-1231; ImmuStore.ReadValue, immustore.go:
    3149-3240) -> (messages, status[n] int32, off[n + 1] uint64); the arguments
    as tx_answers_raw's.  messages[p] is b"" for a request whose status is not
    MH_OK.  out_cap / size_hint as verifiable_answers: with out_cap None the
    call sizes its output itself, and a sizing pass hashes the values too."""
    n = len(kind)

    def call(cap):
        out = np.zeros(max(cap, 1), np.uint8)
        return (out,) + tx_answers_raw(store, tree, kind, tx, prove_since, specs, now_unix, _addr(out), cap)

    if out_cap is None:
        out, off, st = call(int(size_hint or 0))
        if (st == N.MH_ERR_BUFFER_TOO_SMALL).any():
            out, off, st = call(int(off[n]))
    else:
        out, off, st = call(out_cap)
    msgs = [bytes(out[int(off[p]):int(off[p + 1])]) if st[p] == N.MH_OK else b"" for p in range(n)]
    return msgs, st, off


def tx_list(msgs) -> bytes:
    """db.TxScan's schema.TxList of consecutive MH_TXA_TX answers: every Tx as
    field 1 (0x0a, varint length, body)."""
    out = bytearray()
    for m in msgs:
        out.append(0x0a)
        v = len(m)
        while v >= 0x80:
            out.append(v & 0x7f | 0x80)
            v >>= 7
        out.append(v)
        out += m
    return bytes(out)
