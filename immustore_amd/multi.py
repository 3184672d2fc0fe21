"""Multi-GPU htree builds behind the C ABI (mh_multi_*).

One process drives K devices (the shape of a cgo caller: one Go process, the
commit path of immustore.go:1620-1632): one context (HIP stream) per device,
an RCCL clique over them inside libimmustore_merkle.so, power-of-two leaf
shards, one all-gather of the 32-byte subtree roots, the top levels reduced
on the devices.  bench.py's --gpus N path is the same decomposition with one
process per GPU over torch.distributed (immustore_amd/sharding.py).
"""
import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import _native as N
from . import commit, merkle, txlayer
from .merkle import _addr, levels_len


def shard_plan(n: int, ndev: int) -> Tuple[int, int]:
    """(S, G): shard size (power of two >= ceil(n / ndev)) and shard count."""
    s, g = C.c_uint64(), C.c_uint64()
    N.check(N.load().mh_multi_shard_plan(n, ndev, C.byref(s), C.byref(g)))
    return s.value, g.value


def ahtree_range_plan(n0: int, total: int, ndev: int) -> Tuple[int, list]:
    """(k, bounds): the ranges (bounds[d], bounds[d+1]] of a multi-device
    ahtree append of `total` appends onto a tree of n0 (interior bounds are
    multiples of 2^k), as mh_multi_(dev_)ahtree_append_batch cut them."""
    k, g = C.c_int(), C.c_int()
    b = (C.c_uint64 * (ndev + 1))()
    N.check(N.load().mh_ahtree_range_plan(n0, total, ndev, C.byref(k), b, C.byref(g)))
    return k.value, [b[i] for i in range(g.value + 1)]


def peaks_of(dlog: np.ndarray, n: int) -> bytes:
    """The popcount(n) peaks of a tree of size n (lowest level first) from a
    host dLog indexed from 0: node(n with the bits below l cleared, l)."""
    L = N.load()
    out = []
    for l in range(64):
        if (n >> l) & 1:
            out.append(bytes(dlog[L.mh_ahtree_node_index((n >> l) << l, l)]))
    return b"".join(out)


class MultiDevice:
    """mh_multi over the given device ordinals (a device may repeat: more
    shards than devices, roots gathered by device copies instead of RCCL)."""

    _abi = "mh_multi_"  # merkle._call

    def __init__(self, devices: Sequence[int]):
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        N.check(N.load().mh_multi_create(len(devices), arr, C.byref(h)))
        self.handle = h.value
        self.devices = list(devices)

    def close(self):
        if self.handle:
            N.load().mh_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uses_rccl(self) -> bool:
        """RCCL clique (distinct devices) vs device copies (a device repeats)."""
        return len(set(self.devices)) == len(self.devices)

    def ctx_handle(self, d: int):
        return N.load().mh_multi_ctx(self.handle, d)

    def synchronize(self):
        N.check(N.load().mh_multi_synchronize(self.handle))

    def build_entries_fixed(self, version: int, keys: np.ndarray, vals: np.ndarray,
                            want_levels: bool = True):
        """Host arrays keys (n, klen), vals (n, vlen) -> (hvals, levels, root)."""
        keys = np.ascontiguousarray(keys, np.uint8)
        vals = np.ascontiguousarray(vals, np.uint8)
        n = keys.shape[0]
        hv = np.zeros((max(n, 1), 32), np.uint8)
        lv = np.zeros((max(levels_len(n), 1), 32), np.uint8) if want_levels else None
        root = np.zeros(32, np.uint8)
        N.check(N.load().mh_multi_htree_build_entries_fixed(
            self.handle, version, n, _addr(keys), keys.shape[1], _addr(vals), vals.shape[1],
            _addr(hv), _addr(lv), _addr(root)))
        return hv[:n], (lv[:levels_len(n)] if want_levels else None), root.tobytes()

    def dev_build_entries_fixed(self, version, n_per_dev, keys, key_len, vals, val_len, levels,
                                top_levels, roots, hvals=None):
        """Device pointers per device (sequences of ints) -- asynchronous."""
        K = len(self.devices)
        P = C.c_void_p * K
        N.check(N.load().mh_multi_dev_htree_build_entries_fixed(
            self.handle, version, n_per_dev, P(*keys), key_len, P(*vals), val_len,
            P(*hvals) if hvals is not None else None, P(*levels), P(*top_levels), P(*roots)))

    def ahtree_append_batch(self, payloads, want_dlog: bool = True, n0: int = 0,
                            peaks: bytes = None):
        """AppendBatch of the rows of `payloads` (m, plen) onto an ahtree of
        size n0 with the given peaks (see peaks_of) across the devices ->
        (the NEW dLog digests (nodesUpto(n0+m) - nodesUpto(n0), 32) or None,
        RootAt(n0 + m))."""
        p = np.ascontiguousarray(payloads, np.uint8)
        m, plen = p.shape
        L = N.load()
        nd = L.mh_ahtree_nodes_upto(n0 + m) - L.mh_ahtree_nodes_upto(n0)
        dl = np.zeros((max(nd, 1), 32), np.uint8) if want_dlog else None
        root = np.zeros(32, np.uint8)
        pk = np.frombuffer(peaks, np.uint8) if peaks else None
        N.check(L.mh_multi_ahtree_append_batch(self.handle, n0, _addr(pk), _addr(p), m, plen,
                                                _addr(dl), _addr(root)))
        return (dl[:nd] if want_dlog else None), root.tobytes()

    def dev_ahtree_append_batch(self, total, payloads, plen, dlogs, roots_out=None, n0: int = 0,
                                peaks: bytes = None):
        """Device pointers per range (sequences of ints; None entries for
        unused ranges; range d as ahtree_range_plan cuts it) -- asynchronous."""
        K = len(self.devices)
        P = C.c_void_p * K
        pk = np.frombuffer(peaks, np.uint8) if peaks else None
        N.check(N.load().mh_multi_dev_ahtree_append_batch(
            self.handle, n0, _addr(pk), total, P(*payloads), plen, P(*dlogs),
            P(*roots_out) if roots_out is not None else None))

    def build_entries(self, version, kb, ko, mb, mo, vb, vo, ov=None, use=None,
                      want_levels: bool = True):
        """CSR host arrays (as mh_htree_build_entries; mb/mo and ov/use may be
        None) -> (hvals, levels, root)."""
        n = len(ko) - 1
        ko = np.ascontiguousarray(ko, np.uint64)
        vo = np.ascontiguousarray(vo, np.uint64)
        mo = None if mo is None else np.ascontiguousarray(mo, np.uint64)
        kb, vb = np.ascontiguousarray(kb, np.uint8), np.ascontiguousarray(vb, np.uint8)
        mb = None if mb is None else np.ascontiguousarray(mb, np.uint8)
        ov = None if ov is None else np.ascontiguousarray(ov, np.uint8)
        use = None if use is None else np.ascontiguousarray(use, np.uint8)
        hv = np.zeros((max(n, 1), 32), np.uint8)
        lv = np.zeros((max(levels_len(n), 1), 32), np.uint8) if want_levels else None
        root = np.zeros(32, np.uint8)
        N.check(N.load().mh_multi_htree_build_entries(
            self.handle, version, n, _addr(kb), _addr(ko), _addr(mb), _addr(mo), _addr(vb),
            _addr(vo), _addr(ov), _addr(use), _addr(hv), _addr(lv), _addr(root)))
        return hv[:n], (lv[:levels_len(n)] if want_levels else None), root.tobytes()

    # ---- the PCIe-bound batch paths split over the devices (mh_multi_*): the
    # single-context wrappers, which marshal the arguments, given this clique
    # in place of a context (merkle._call)
    def htree_verify_inclusion_batch(self, leaf, width, term_off, terms, digests, roots):
        """merkle.verify_inclusion_arrays, proofs split by index -> ok[n]."""
        return merkle.verify_inclusion_arrays(leaf, width, term_off, terms, digests, roots, self)

    def verify_dual_proof_v2_batch(self, src_hdrs, tgt_hdrs, md_blob, incl, cons, src, tgt,
                                   src_alh, tgt_alh):
        """txlayer.verify_dual_proof_v2_batch, split by index -> status[n]."""
        return txlayer.verify_dual_proof_v2_batch(src_hdrs, tgt_hdrs, md_blob, incl, cons, src,
                                                  tgt, src_alh, tgt_alh, self)

    def verify_values(self, vals, off, hvals, vlen=None):
        """merkle.verify_values, parts of nearly equal value bytes ->
        (corrupted count, status[n])."""
        return merkle.verify_values(vals, off, hvals, vlen, self)

    def verify_dual_proof_v2_pb_batch(self, msgs, src, tgt, src_alh, tgt_alh):
        """txlayer.verify_dual_proof_v2_pb_batch, parts of nearly equal message
        bytes -> status[n]."""
        return txlayer.verify_dual_proof_v2_pb_batch(msgs, src, tgt, src_alh, tgt_alh, self)

    def verify_dual_proof_pb_batch(self, msgs, src, tgt, src_alh, tgt_alh):
        """txlayer.verify_dual_proof_pb_batch (DualProof v1), parts of nearly
        equal message bytes -> (status[n], ok[n])."""
        return txlayer.verify_dual_proof_pb_batch(msgs, src, tgt, src_alh, tgt_alh, self)

    def verify_verifiable_entry_pb_batch(self, msgs, keys, at_tx, state_tx, state_alh):
        """txlayer.verify_verifiable_entry_pb_batch (whole VerifiableGet answers),
        parts of nearly equal message bytes ->
        (status[n], ok[n], new_tx[n], new_alh[n, 32])."""
        return txlayer.verify_verifiable_entry_pb_batch(msgs, keys, at_tx, state_tx, state_alh,
                                                        self)

    def verify_verifiable_tx_pb_batch(self, msgs, kinds, specs, at_tx, state_tx, state_alh):
        """txlayer.verify_verifiable_tx_pb_batch (whole VerifiableTx answers),
        parts of nearly equal message bytes ->
        (status[n], ok[n], new_tx[n], new_alh[n, 32], eh[n, 32])."""
        return txlayer.verify_verifiable_tx_pb_batch(msgs, kinds, specs, at_tx, state_tx,
                                                     state_alh, self)

    def verify_document_batch(self, docs):
        """txlayer.verify_document_batch, parts of nearly equal entries +
        document bytes -> (status[n], target_alh[n, 32])."""
        return txlayer.verify_document_batch(docs, self)

    def precommit_csr(self, version: int, tx_off, keys, key_off, vals, val_off, md=None,
                      md_off=None, hval_override=None, use_override=None, expect_eh=None,
                      max_width: int = 0):
        """commit.precommit_csr: whole transactions, parts of nearly equal value
        bytes, a commit pipe per device -> (hvals, eh, status)."""
        return commit.precommit_csr(self, version, tx_off, keys, key_off, vals, val_off, md, md_off,
                                    hval_override, use_override, expect_eh, max_width)

    def txlog_validate(self, buf, max_entries: int = 1024, max_key_len: int = 1024,
                       max_txs=None, out=None):
        """txlayer.txlog_validate: the log cut at record boundaries, every part
        over its own link -> (status, ntx, consumed, hdrs, alh, per_tx)."""
        return txlayer.txlog_validate(buf, max_entries, max_key_len, max_txs, self, out)

