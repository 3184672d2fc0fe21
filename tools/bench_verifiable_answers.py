#!/usr/bin/env python3
"""Throughput of mh_verifiable_answer_pb_batch (whole VerifiableTx /
VerifiableEntry answers generated in one device pass from a resident store)
beside the two existing calls that bound its parts.

Store: 2^--txs-log2 txs of --entries entries with 8-byte keys (version-1
headers, BlTxID lagging 1 to 4), its tx log, 12-byte commit log and ahtree
resident on the device.  Load: --requests requests, half TX and half ENTRY, the
tx drawn uniformly, prove_since drawn from --states distinct client states.
A sample of the answers is compared with the Go-shaped messages of
tests/answer_util.py.  One JSON line:

  answers          answers/s and output GiB/s of the call (median of --reps,
                   host clock around the synchronous call, after --warmup calls)
  distinct_records the distinct txs the batch reads (each re-hashed once)
  rehash_only      mh_txlog_validate_clog over exactly those records (their
                   gathered commit log on the device), same inputs, same process
  dual_only        mh_dev_dual_proof_pb_batch for the same (source, target)
                   pairs over a dense digest window of the whole store
  kernels_ms       per-kernel times of one call from mh_ctx_timing (a separate
                   call: timing serialises the launches)

    python3 tools/bench_verifiable_answers.py
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import struct
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "oracle"), os.path.join(HERE, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

KERNELS = ("ans_heads", "ans_popc", "ans_compact", "txlog_struct", "txlog_lanes", "txlog_wave",
           "tx_alh", "ans_verdict", "ans_link", "ans_counts", "txe_index", "txe_leaf", "ans_trees",
           "ans_esize", "ans_find", "ans_txsize", "pb_dual1_size", "ans_size", "ans_tx_header",
           "ans_tx_entries", "ans_assemble", "pb_dual1_write")
REHASH = ("txlog_struct", "txlog_lanes", "txlog_wave", "tx_alh")


def bl_of(k):
    return max(0, k - 1 - (k % 4))


def build_store(N, w):
    """-> (raw tx log, 12-byte cLog, the Alh of every tx)"""
    import oracle as orc
    sha = lambda b: hashlib.sha256(b).digest()  # noqa: E731
    raw, clog, alhs = bytearray(), bytearray(), []
    aht = orc.AHtree(N)
    prev = sha(b"")
    for k in range(1, N + 1):
        ents, lv = bytearray(), []
        for j in range(w):
            key = struct.pack(">Q", (k << 16) | j)
            hv = sha(b"value %d.%d" % (k, j))
            lv.append(sha(b"\x00" + sha(b"\x00\x00\x00\x08" + key + hv)))
            ents += b"\x00\x00\x00\x08" + key + struct.pack(">IQ", 12, 16 * k + j) + hv
        while len(lv) > 1:
            lv = [sha(b"\x01" + lv[i] + lv[i + 1]) if i + 1 < len(lv) else lv[i]
                  for i in range(0, len(lv), 2)]
        bl, blroot = bl_of(k), bytes(32)
        if bl:
            st, blroot = aht.root_at(bl)
            assert st == 0
            blroot = bytes(blroot)
        ts = 1700000000 + k
        st, inner = orc.tx_inner_hash(ts, 1, b"", w, lv[0], bl, blroot)
        assert st == 0
        alh = bytes(orc.tx_alh(k, prev, inner))
        rec = struct.pack(">QqQ", k, ts, bl) + blroot + prev + struct.pack(">HHI", 1, 0, w) + ents + alh
        clog += struct.pack(">QI", len(raw), len(rec))
        raw += rec
        aht.append(alh)
        alhs.append(alh)
        prev = alh
    return bytes(raw), bytes(clog), alhs


def read_set(T, S):
    """the txs ImmuStore.DualProof reads for one request, and its (src, tgt)"""
    root = T if S == 0 else S
    src, tgt = (root, T) if S <= T else (T, root)
    bl, sbl = bl_of(tgt), bl_of(src)
    r = {T, root}
    if bl:
        r.add(bl)
    r.update(range(max(src, bl), tgt + 1))
    r.update(range(sbl + 1, min(src, bl) + 1))
    return r, src, tgt


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs-log2", type=int, default=16)
    ap.add_argument("--entries", type=int, default=16)
    ap.add_argument("--requests", type=int, default=65536)
    ap.add_argument("--states", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=24, help="answers checked against the CPU expectation")
    ap.add_argument("--host-only", action="store_true", help="build the store and the load, then stop")
    a = ap.parse_args()
    N, w, n = 1 << a.txs_log2, a.entries, a.requests
    t0 = time.perf_counter()
    raw, clog, alhs = build_store(N, w)
    build_s = time.perf_counter() - t0
    rng = np.random.default_rng(20240)
    states = np.sort(rng.choice(N, a.states, replace=False).astype(np.uint64) + 1)
    tx = rng.integers(1, N + 1, n).astype(np.uint64)
    since = states[rng.integers(0, a.states, n)]
    kind = (np.arange(n) % 2).astype(np.uint8)
    keys = [struct.pack(">Q", (int(tx[p]) << 16) | (p % w)) if kind[p] else b"" for p in range(n)]
    ents = [b"\x08" + bytes([1 + p % 100]) if kind[p] else b"" for p in range(n)]
    distinct, pairs = set(), []
    for p in range(n):
        r, src, tgt = read_set(int(tx[p]), int(since[p]))
        distinct |= r
        pairs.append((src, tgt))
    ids = np.array(sorted(distinct), np.uint64)
    res = {"txs": N, "entries_per_tx": w, "requests": n, "states": a.states,
           "distinct_records": int(ids.size), "txlog_bytes": len(raw),
           "store_build_s": round(build_s, 2)}
    if a.host_only:
        print(json.dumps(res))
        return

    import torch  # noqa: F401  (the HIP runtime the library links)
    import immustore_amd as m
    from immustore_amd import _native as Nn
    from immustore_amd import answers as ans
    from immustore_amd.txlayer import TX_HEADER, tx_alh_batch, txlog_validate_clog
    L = Nn.load()
    ctx = m.Context(0)
    tree = m.AHtree(ctx)
    tree.append_batch(np.frombuffer(b"".join(alhs), np.uint8).reshape(-1, 32))
    store = m.ResidentStore(tree, raw, clog, 12)

    # ---- the call
    kb, ko = ans._csr(keys, n)
    eb, eo = ans._csr(ents, n)
    b = ans._Batch()
    b.n, b.kind, b.tx, b.prove_since = n, kind.ctypes.data, tx.ctypes.data, since.ctypes.data
    b.keys, b.key_off, b.entries, b.entry_off = kb.ctypes.data, ko.ctypes.data, eb.ctypes.data, \
        eo.ctypes.data
    sd = store.descriptor()
    off = np.zeros(n + 1, np.uint64)
    st = np.zeros(n, np.int32)
    Nn.check(L.mh_verifiable_answer_pb_batch(tree.handle, C.addressof(sd), C.addressof(b), None, 0,
                                             off.ctypes.data, st.ctypes.data))
    total = int(off[n])
    out = np.zeros(total + 64, np.uint8)

    def call():
        Nn.check(L.mh_verifiable_answer_pb_batch(tree.handle, C.addressof(sd), C.addressof(b),
                                                 out.ctypes.data, total, off.ctypes.data,
                                                 st.ctypes.data))

    med, lo, hi = median_ms(call, a.warmup, a.reps)
    assert not st.any(), "an answer failed"
    res["answers"] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                      "per_s": round(n / med * 1e3), "out_bytes": total,
                      "out_gib_s": round(total / med * 1e3 / 2 ** 30, 2)}
    if a.sample:  # against the Go-shaped messages
        import answer_util as A
        from tx_util import clog_for, record_spans
        cut = min(N, 64)
        spans = record_spans(raw, cut)
        sraw = raw[:spans[-1][1]]
        small = A.AnsStore(sraw, clog_for(sraw, spans, 12), 12)
        stree = m.AHtree(ctx)
        stree.append_batch(np.frombuffer(b"".join(alhs[:cut]), np.uint8).reshape(-1, 32))
        sstore = m.ResidentStore(stree, sraw, small.clog, 12)
        reqs = [(p % 2, 1 + (p * 7) % cut, (p * 5) % (cut + 1),
                 struct.pack(">Q", ((1 + (p * 7) % cut) << 16) | (p % w)) if p % 2 else b"",
                 b"\x08\x01" if p % 2 else b"") for p in range(a.sample)]
        msgs, sst, _ = m.verifiable_answers(sstore, *A.columns(reqs))
        assert [(int(x), y) for x, y in zip(sst, msgs)] == [small.expect(*r) for r in reqs]
        res["sample_checked"] = len(reqs)
        sstore.close()
        stree.close()

    # ---- per-kernel split (a call of its own)
    ctx.set_timing(True)
    ctx.timing_reset()
    call()
    ctx.synchronize()
    km = {}
    for name in KERNELS:
        ms, cnt = ctx.timing(name)
        if cnt:
            km[name] = round(ms, 4)
    ctx.set_timing(False)
    ctx.timing_reset()
    res["kernels_ms"] = km
    res["kernels_ms_rehash"] = round(sum(v for k, v in km.items() if k in REHASH), 4)
    res["kernels_ms_new"] = round(sum(v for k, v in km.items() if k not in REHASH), 4)

    # ---- the re-hash of exactly those records, by the existing call
    cb = np.frombuffer(clog, np.uint8).reshape(N, 12)
    gathered = np.ascontiguousarray(cb[ids.astype(np.int64) - 1]).reshape(-1)
    gp = C.c_void_p()
    Nn.check(L.mh_dev_alloc(ctx.handle, gathered.size, C.byref(gp)))
    Nn.check(L.mh_memcpy_h2d(ctx.handle, gp.value, gathered.ctypes.data, gathered.size))
    ctx.synchronize()
    D = int(ids.size)
    hp, ap_, sp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    Nn.check(L.mh_dev_alloc(ctx.handle, D * TX_HEADER.itemsize, C.byref(hp)))
    Nn.check(L.mh_dev_alloc(ctx.handle, D * 32, C.byref(ap_)))
    Nn.check(L.mh_dev_alloc(ctx.handle, D * 4, C.byref(sp)))

    def rehash():
        rc = txlog_validate_clog(store._txlog.value, len(raw), None, ntx=D, ctx=ctx,
                                 out=(hp.value, ap_.value, sp.value), clog_dev=gp.value)
        assert rc[0] == 0 and rc[1] == 0, rc[:3]

    med, lo, hi = median_ms(rehash, a.warmup, a.reps)
    res["rehash_only"] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                          "records_per_s": round(D / med * 1e3)}

    # ---- the DualProofs of the same pairs, by the existing device call
    _, _, _, hdrs, alh_all, per_tx = txlog_validate_clog(store._txlog.value, len(raw), clog, ctx=ctx)
    assert not per_tx.any()
    inner_all, alh2 = tx_alh_batch(hdrs, ctx=ctx)
    assert np.array_equal(alh2, alh_all)
    sh = np.ascontiguousarray(hdrs[np.array([s_ for s_, _ in pairs]) - 1])
    th = np.ascontiguousarray(hdrs[np.array([t_ for _, t_ in pairs]) - 1])

    def dev(arr):
        p = C.c_void_p()
        Nn.check(L.mh_dev_alloc(ctx.handle, max(arr.nbytes, 16), C.byref(p)))
        Nn.check(L.mh_memcpy_h2d(ctx.handle, p.value, arr.ctypes.data, arr.nbytes))
        return p

    dsh, dth = dev(sh), dev(th)
    dalh, dinn = dev(np.ascontiguousarray(alh_all)), dev(np.ascontiguousarray(inner_all))
    ctx.synchronize()
    L.mh_pb_dual_scratch_size.restype = C.c_uint64
    scratch, doff, dst = C.c_void_p(), C.c_void_p(), C.c_void_p()
    Nn.check(L.mh_dev_alloc(ctx.handle, L.mh_pb_dual_scratch_size(n), C.byref(scratch)))
    Nn.check(L.mh_dev_alloc(ctx.handle, (n + 1) * 8, C.byref(doff)))
    Nn.check(L.mh_dev_alloc(ctx.handle, n * 4, C.byref(dst)))
    dlog = C.c_void_p()
    Nn.check(L.mh_ahtree_dlog_device(tree.handle, C.byref(dlog)))

    def dual(phase, outp, cap):
        Nn.check(L.mh_dev_dual_proof_pb_batch(ctx.handle, phase, dlog.value, N, n, dsh.value,
                                              dth.value, store._txlog.value, 1, N, dalh.value,
                                              dinn.value, outp, cap, doff.value, dst.value,
                                              scratch.value))
        ctx.synchronize()

    dual(1, None, 0)
    hoff = np.zeros(n + 1, np.uint64)
    Nn.check(L.mh_memcpy_d2h(ctx.handle, hoff.ctypes.data, doff.value, (n + 1) * 8))
    ctx.synchronize()
    dtotal = int(hoff[n])
    dout = C.c_void_p()
    Nn.check(L.mh_dev_alloc(ctx.handle, dtotal + 64, C.byref(dout)))
    med, lo, hi = median_ms(lambda: dual(3, dout.value, dtotal), a.warmup, a.reps)
    hst = np.zeros(n, np.int32)
    Nn.check(L.mh_memcpy_d2h(ctx.handle, hst.ctypes.data, dst.value, n * 4))
    ctx.synchronize()
    assert not hst.any()
    res["dual_only"] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                        "proofs_per_s": round(n / med * 1e3), "bytes": dtotal}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
