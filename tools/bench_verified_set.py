#!/usr/bin/env python3
"""Throughput of mh_verify_verifiable_tx_pb_batch (whole VerifiableTx answers
of verified writes verified in one device pass) against what bounds it.

About 1 GiB of pinned host memory goes up per call: the VerifiableTx answers
of a synthetic store (tests/verifiable_tx_util.py, version-1 txs of --entries
entries with plain values of --value-len bytes) as a server would answer a
client one to three txs behind, plus what the client sent (keys and values:
the call hashes them too); the distinct answers are repeated to the target
size.  Every answer must verify, a sample is checked against the CPU
reference.  --entries 1 asks as SET, more as SET_ALL.  One JSON line:

  fused            answers/s, entries/s and GiB/s of the fused call (median of --reps)
  h2d              a plain pinned host-to-device copy of the same bytes, same run
  dual_only        mh_verify_dual_proof_pb_batch over just those answers'
                   DualProof bytes (pinned), same process
  kernels_ms       per-kernel times of one fused call from mh_ctx_timing (a
                   separate call: timing serialises the launches)

    python3 tools/bench_verified_set.py --entries 1 --value-len 256
    python3 tools/bench_verified_set.py --entries 1 --value-len 4096
    python3 tools/bench_verified_set.py --entries 64
    python3 tools/bench_verified_set.py --entries 1024
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "oracle"), os.path.join(HERE, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the HIP runtime the library links)

import immustore_amd as m  # noqa: E402
from immustore_amd import _native as N  # noqa: E402
from immustore_amd.txlayer import _Pinned, _VerifiedTxBatch, _addr  # noqa: E402

KERNELS = ("pbd_vtx_size", "pbd_vtx_write", "vtx_leaf", "vtx_spec", "leaf_for", "small_roots",
           "seg_level", "pbd_dual1_size", "pbd_dual1_write", "vtx_answer", "ventry_verdict")


def distinct_answers(entries, value_len):
    """-> (answers, kind, specs per answer, S, state_alh, new tx, the answers'
    DualProof bytes and their (src, tgt, src_alh, tgt_alh))"""
    import verifiable_tx_util as V
    ntx = 40 if entries == 1 else (24 if entries <= 64 else 10)
    s = V.store(value_len, (entries,) * ntx)
    kind = V.SET if entries == 1 else V.SET_ALL
    asks = [(k, k - d) for k in range(5, ntx + 1) for d in (1, 2, 3)]
    answers = [V.answer(k, S, s=s).SerializeToString() for k, S in asks]
    specs = [V.request(k, kind, s)[1] for k, _ in asks]
    for i in range(0, len(asks), 7):  # the CPU reference on a sample
        k, S = asks[i]
        assert V.reference(answers[i], kind, specs[i], 0, S, s.alhs[S - 1])[:4] == \
            (0, True, k, s.alhs[k - 1]), i
    duals = [V.dual_msg(S, k, s) for k, S in asks]
    dual_args = ([S for _, S in asks], [k for k, _ in asks], [s.alhs[S - 1] for _, S in asks],
                 [s.alhs[k - 1] for k, _ in asks])
    return (answers, kind, specs, [S for _, S in asks], [s.alhs[S - 1] for _, S in asks],
            [k for k, _ in asks], duals, dual_args)


def tiled(items, reps):
    """items repeated reps times, back to back -> (pinned bytes, pinned offsets)"""
    block = np.frombuffer(b"".join(items), np.uint8)
    lens = np.tile(np.array([len(x) for x in items], np.uint64), reps)
    off = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    return _Pinned(np.concatenate([np.tile(block, reps), np.zeros(1, np.uint8)])), _Pinned(off)


def median_ms(fn, reps):
    fn()  # warm-up: buffers grown, clocks up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1)
    ap.add_argument("--value-len", type=int, default=256)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert m.device_count() > 0, "no GPU"
    ctx = m.Context(0)
    L = N.load()
    answers, kind, specs, S, salh, want_tx, duals, (ds, dt, dsa, dta) = \
        distinct_answers(a.entries, a.value_len)
    k = len(answers)
    keys = [key for sp in specs for key, _ in sp]
    vals = [val for sp in specs for _, val in sp]
    block = sum(len(x) for x in answers) + sum(len(x) for x in keys) + sum(len(x) for x in vals)
    reps = max(1, int(a.gib * (1 << 30)) // block)
    n = k * reps
    msgs, off = tiled(answers, reps)
    kbuf, koff = tiled(keys, reps)
    vbuf, voff = tiled(vals, reps)
    rep32 = lambda xs: _Pinned(np.tile(np.frombuffer(b"".join(xs), np.uint8).reshape(-1, 32),  # noqa: E731
                                       (reps, 1)))
    rep64 = lambda xs: _Pinned(np.tile(np.asarray(xs, np.uint64), reps))  # noqa: E731
    soff = np.zeros(n + 1, np.uint64)
    np.cumsum(np.tile(np.array([len(sp) for sp in specs], np.uint64), reps), out=soff[1:])
    kd, soff = _Pinned(np.full(n, kind, np.uint8)), _Pinned(soff)
    at, stx, sa = _Pinned(np.zeros(n, np.uint64)), rep64(S), rep32(salh)
    b = _VerifiedTxBatch(n, *[_addr(x.a) for x in (msgs, off, kd, soff, kbuf, koff, vbuf, voff, at,
                                                   stx, sa)])
    st, ok = _Pinned(np.zeros(n, np.int32)), _Pinned(np.zeros(n, np.uint8))
    ntx, nalh = _Pinned(np.zeros(n, np.uint64)), _Pinned(np.zeros((n, 32), np.uint8))
    eh = _Pinned(np.zeros((n, 32), np.uint8))

    def fused():
        N.check(L.mh_verify_verifiable_tx_pb_batch(ctx.handle, ctypes.byref(b), _addr(st.a),
                                                   _addr(ok.a), _addr(ntx.a), _addr(nalh.a),
                                                   _addr(eh.a)))

    fused_ms, fused_all = median_ms(fused, a.reps)
    assert (st.a == 0).all() and (ok.a == 1).all(), "an answer did not verify"
    assert np.array_equal(ntx.a[:k], np.asarray(want_tx, np.uint64))
    # the same bytes, copied and nothing else
    mb, kb, vb = msgs.a.nbytes - 1, kbuf.a.nbytes - 1, vbuf.a.nbytes - 1
    up = mb + kb + vb
    dst = ctypes.c_void_p()
    N.check(L.mh_dev_alloc(ctx.handle, up, ctypes.byref(dst)))

    def h2d():
        o = 0
        for x, nb in ((msgs, mb), (kbuf, kb), (vbuf, vb)):
            N.check(L.mh_memcpy_h2d(ctx.handle, ctypes.c_void_p(dst.value + o), _addr(x.a), nb))
            o += nb
        ctx.synchronize()

    h2d_ms, _ = median_ms(h2d, a.reps)
    N.check(L.mh_dev_free(ctx.handle, dst))
    # the dual-only call over just the DualProof bytes of the same answers
    dmsgs, doff = tiled(duals, reps)
    d_s, d_t, d_sa, d_ta = rep64(ds), rep64(dt), rep32(dsa), rep32(dta)
    dst_, dok = _Pinned(np.zeros(n, np.int32)), _Pinned(np.zeros(n, np.uint8))

    def dual_only():
        N.check(L.mh_verify_dual_proof_pb_batch(ctx.handle, n, _addr(dmsgs.a), _addr(doff.a),
                                                _addr(d_s.a), _addr(d_t.a), _addr(d_sa.a),
                                                _addr(d_ta.a), _addr(dst_.a), _addr(dok.a)))

    dual_ms, _ = median_ms(dual_only, a.reps)
    assert (dst_.a == 0).all() and (dok.a == 1).all()
    db = dmsgs.a.nbytes - 1
    # per-kernel times of one fused call
    ctx.set_timing(True)
    ctx.timing_reset()
    fused()
    kern = {name: round(ctx.timing(name)[0], 3) for name in KERNELS}
    kern["all"] = round(ctx.timing("")[0], 3)
    kern["dual_proof_v1_core"] = round(kern["all"] - sum(kern[x] for x in KERNELS), 3)
    ctx.set_timing(False)
    extra_h2d = h2d_ms * (up - db) / up  # the bytes the dual-only call does not carry
    print(json.dumps({
        "tool": "bench_verified_set", "entries": a.entries, "value_len": a.value_len,
        "kind": "SET" if a.entries == 1 else "SET_ALL", "answers": n, "distinct": k,
        "uploaded_bytes": int(up), "message_bytes": int(mb), "key_bytes": int(kb),
        "value_bytes": int(vb), "dual_proof_bytes": int(db), "mean_answer_bytes": round(mb / n, 1),
        "fused": {"ms": round(fused_ms, 3), "ms_all": [round(x, 3) for x in fused_all],
                  "answers_per_s": round(n / fused_ms * 1e3),
                  "entries_per_s": round(n * a.entries / fused_ms * 1e3),
                  "gib_per_s": round(up / fused_ms / 1073741.824, 2)},
        "h2d": {"ms": round(h2d_ms, 3), "gib_per_s": round(up / h2d_ms / 1073741.824, 2)},
        "dual_only": {"ms": round(dual_ms, 3), "gib_per_s": round(db / dual_ms / 1073741.824, 2)},
        "fused_over_h2d": round(fused_ms / h2d_ms, 3),
        "fused_over_dual_only": round(fused_ms / dual_ms, 3),
        "dual_only_plus_extra_h2d_ms": round(dual_ms + extra_h2d, 3),
        "excess_ms": round(fused_ms - dual_ms - extra_h2d, 3),
        "kernels_ms": kern,
        "checked": "every answer ok; new_tx of the first block; a sample vs the CPU reference"}))
    ctx.close()


if __name__ == "__main__":
    main()
