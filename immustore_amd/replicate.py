"""Python mirror of the follower's side of replication (C ABI
mh_replicate_tx_batch): ImmuStore.ReplicateTx (immustore.go:2772-2932) for a
run of exported txs in one device pass.

  ExportTx's bytes parsed          immustore.go:2773-2881, tx.go:166-247
  OngoingTx.set and validations    ongoing_tx.go:242-267, :798, immustore.go:3243
  hVal, entry digests, the htree   immustore.go:1620-1632, tx.go:332-355
  Eh / id / BlRoot / PrevAlh       immustore.go:1649-1722
  aht.Append of the accepted Alh   immustore.go:1921-1946

Everything runs in libimmustore_merkle.so on the tree's device; there is no
CPU path.
"""
import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from .merkle import AHtree, _addr
from .txlayer import TX_HEADER

# mh_replicated_entry: where an entry lies in the exported bytes
REPLICATED_ENTRY = np.dtype([("key_off", "<u8"), ("md_off", "<u8"), ("val_off", "<u8"),
                             ("key_len", "<u4"), ("md_len", "<u4"), ("val_len", "<u4"),
                             ("flags", "<u4")])
assert REPLICATED_ENTRY.itemsize == 40

EMPTY_ALH = bytes.fromhex("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")


class _Batch(C.Structure):  # mh_replicate_batch
    _fields_ = [("n", C.c_uint64), ("txs", C.c_void_p), ("tx_off", C.c_void_p),
                ("max_entries", C.c_uint32), ("max_key_len", C.c_uint32),
                ("max_value_len", C.c_uint32), ("flags", C.c_uint32),
                ("prev_alh", C.c_uint8 * 32)]


def replicate_tx_batch(tree: AHtree, exported, prev_alh: bytes = EMPTY_ALH, *,
                       max_entries: int = 1024, max_key_len: int = 1024,
                       max_value_len: int = 1 << 25, flags: int = 0, tx_off=None,
                       ents_cap: Optional[int] = None, want_entries: bool = True):
    """exported: a sequence of ExportTx byte strings, or (with tx_off, n + 1
    offsets) one uint8 array holding them back to back (possibly a view of
    pinned memory).  Returns a dict of numpy arrays: status [n] int32, accepted
    (int), hdrs [n] TX_HEADER, md_blob, alh [n, 32], ent_off [n + 1], ents
    [E] REPLICATED_ENTRY and hvals [E, 32] (offsets index the concatenated
    bytes).  ents_cap too small raises ErrBufferTooSmall; the needed count is
    the exception's `needed`."""
    if tx_off is None:
        blobs = [bytes(x) for x in exported]
        off = np.zeros(len(blobs) + 1, np.uint64)
        if blobs:
            off[1:] = np.cumsum([len(x) for x in blobs], dtype=np.uint64)
        flat = b"".join(blobs)
        buf = np.frombuffer(flat, np.uint8).copy() if flat else np.zeros(1, np.uint8)
    else:
        buf = exported
        off = np.ascontiguousarray(tx_off, np.uint64)
    n = len(off) - 1
    if ents_cap is None:  # an entry is at least 8 bytes of its blob
        ents_cap = int(off[-1] - off[0]) // 8 if n > 0 else 0
    m = max(n, 1)
    st = np.zeros(m, np.int32)
    hd = np.zeros(m, TX_HEADER)
    md = np.zeros(m * 268, np.uint8)
    alh = np.zeros((m, 32), np.uint8)
    eo = np.zeros(n + 1, np.uint64)
    en = np.zeros(max(ents_cap, 1), REPLICATED_ENTRY) if want_entries else None
    hv = np.zeros((max(ents_cap, 1), 32), np.uint8) if want_entries else None
    b = _Batch()
    b.n, b.txs, b.tx_off = n, _addr(buf), _addr(off)
    b.max_entries, b.max_key_len, b.max_value_len, b.flags = (max_entries, max_key_len,
                                                              max_value_len, flags)
    b.prev_alh[:] = list(bytes(prev_alh))
    acc = C.c_uint64(0)
    rc = N.load().mh_replicate_tx_batch(tree.handle, C.addressof(b), _addr(st), C.byref(acc),
                                        _addr(hd), _addr(md), _addr(alh), _addr(eo), _addr(en),
                                        ents_cap, _addr(hv))
    if rc == N.MH_ERR_BUFFER_TOO_SMALL:
        e = N.ErrBufferTooSmall(rc)
        e.needed = int(eo[n])
        raise e
    N.check(rc)
    ne = int(eo[n])
    return {"status": st[:n], "accepted": acc.value, "hdrs": hd[:n], "md_blob": md[:n * 268],
            "alh": alh[:n], "ent_off": eo,
            "ents": en[:ne] if want_entries else None,
            "hvals": hv[:ne] if want_entries else None}
