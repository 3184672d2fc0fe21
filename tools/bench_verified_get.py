#!/usr/bin/env python3
"""Throughput of mh_verify_verifiable_entry_pb_batch (whole VerifiableGet
answers verified in one device pass) against what bounds it.

About 1 GiB of answers in pinned host memory: the asked entries of the tests'
synthetic store (tests/verifiable_entry_util.py, every plain value of
--value-len bytes, txs of up to 17 entries) as a server would answer them for
a client one to three txs behind, the DualProof of every answer generated on
the device (mh_ahtree_dual_proof_pb_batch); the distinct answers are repeated
to the target size.  Every answer must verify, a sample is checked against the
CPU reference.  One JSON line:

  fused            answers/s and message GiB/s of the fused call (median of --reps)
  h2d              a plain pinned host-to-device copy of the same bytes, same run
  dual_only        mh_verify_dual_proof_pb_batch over just those answers'
                   DualProof bytes (pinned), same process: the call this one extends
  kernels_ms       per-kernel times of one fused call from mh_ctx_timing (a
                   separate call: timing serialises the launches)

    python3 tools/bench_verified_get.py --value-len 256
    python3 tools/bench_verified_get.py --value-len 4096
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
from immustore_amd.txlayer import _Pinned, _VerifiedGetBatch, _addr  # noqa: E402

KERNELS = ("pbd_ventry_size", "pbd_ventry_write", "pbd_dual1_size", "pbd_dual1_write",
           "ventry_verify", "ventry_verdict")


def distinct_answers(ctx, value_len):
    """-> (answers, keys, S, state_alh, the answers' DualProof bytes, their
    (src, tgt, src_alh, tgt_alh))"""
    import verifiable_entry_util as V
    s = V.store(value_len)
    slots = [sl for sl in s.slots if s.width[sl.tx] <= 17 and not sl.is_ref and sl.tx > 4]
    asks = [(sl, sl.tx - d) for sl in slots for d in (1, 2, 3)]
    pairs = [V.proof_pair(sl, S) for sl, S in asks]
    t = m.AHtree(ctx)
    try:
        t.append_batch(np.stack([np.frombuffer(a, np.uint8) for a in s.alhs]))
        duals, st = t.dual_proof_pb_batch(s.recs[[a - 1 for a, _ in pairs]],
                                          s.recs[[b - 1 for _, b in pairs]], s.blob, 1, s.alhs,
                                          s.inners)
    finally:
        t.close()
    assert (np.asarray(st) == 0).all()
    duals = [bytes(d) for d in duals]
    answers = [V.answer(sl, S, s=s, dual=d).SerializeToString() for (sl, S), d in zip(asks, duals)]
    for k in range(0, len(asks), 7):  # the CPU reference on a sample
        sl, S = asks[k]
        assert V.reference(answers[k], sl.key, 0, S, s.alhs[S - 1]) == \
            (0, True, sl.tx, s.alhs[sl.tx - 1]), k
    dual_args = ([a for a, _ in pairs], [b for _, b in pairs], [s.alhs[a - 1] for a, _ in pairs],
                 [s.alhs[b - 1] for _, b in pairs])
    return (answers, [sl.key for sl, _ in asks], [S for _, S in asks],
            [s.alhs[S - 1] for _, S in asks], duals, dual_args)


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
    ap.add_argument("--value-len", type=int, default=256)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert m.device_count() > 0, "no GPU"
    ctx = m.Context(0)
    L = N.load()
    answers, keys, S, salh, duals, (ds, dt, dsa, dta) = distinct_answers(ctx, a.value_len)
    k = len(answers)
    reps = max(1, int(a.gib * (1 << 30)) // sum(len(x) for x in answers))
    n = k * reps
    msgs, off = tiled(answers, reps)
    kbuf, koff = tiled(keys, reps)
    rep32 = lambda xs: _Pinned(np.tile(np.frombuffer(b"".join(xs), np.uint8).reshape(-1, 32),  # noqa: E731
                                       (reps, 1)))
    rep64 = lambda xs: _Pinned(np.tile(np.asarray(xs, np.uint64), reps))  # noqa: E731
    at, stx, sa = _Pinned(np.zeros(n, np.uint64)), rep64(S), rep32(salh)
    b = _VerifiedGetBatch(n, *[_addr(x.a) for x in (msgs, off, kbuf, koff, at, stx, sa)])
    st, ok = _Pinned(np.zeros(n, np.int32)), _Pinned(np.zeros(n, np.uint8))
    ntx, nalh = _Pinned(np.zeros(n, np.uint64)), _Pinned(np.zeros((n, 32), np.uint8))

    def fused():
        N.check(L.mh_verify_verifiable_entry_pb_batch(ctx.handle, ctypes.byref(b), _addr(st.a),
                                                      _addr(ok.a), _addr(ntx.a), _addr(nalh.a)))

    fused_ms, fused_all = median_ms(fused, a.reps)
    assert (st.a == 0).all() and (ok.a == 1).all(), "an answer did not verify"
    assert np.array_equal(ntx.a[:k], np.asarray([s_ + d for s_, d in zip(S, [1, 2, 3] * (k // 3))],
                                                np.uint64))
    # the same bytes, copied and nothing else
    mb = msgs.a.nbytes - 1
    dst = ctypes.c_void_p()
    N.check(L.mh_dev_alloc(ctx.handle, mb, ctypes.byref(dst)))

    def h2d():
        N.check(L.mh_memcpy_h2d(ctx.handle, dst, _addr(msgs.a), mb))
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
    extra_h2d = h2d_ms * (mb - db) / mb  # the bytes the dual-only call does not carry
    # compressions k_ventry_verify runs per answer: value, digest (2), leaf,
    # 2 per inclusion term (1.65 full-compression equivalents with the
    # tabulated second block), the header's Alh (3 + 2)
    import verifiable_entry_util as V
    nterms = np.mean([len(V.parse(x)[1].inclusionProof.terms) for x in answers])
    comp = (a.value_len + 1 + 9 + 63) // 64 + 2 + 1 + 2 * nterms + 5
    rate = n * comp / (kern["ventry_verify"] * 1e-3) if kern["ventry_verify"] else 0.0
    print(json.dumps({
        "tool": "bench_verified_get", "value_len": a.value_len, "answers": n, "distinct": k,
        "message_bytes": int(mb), "dual_proof_bytes": int(db), "mean_answer_bytes": round(mb / n, 1),
        "fused": {"ms": round(fused_ms, 3), "ms_all": [round(x, 3) for x in fused_all],
                  "answers_per_s": round(n / fused_ms * 1e3),
                  "gib_per_s": round(mb / fused_ms / 1073741.824, 2)},
        "h2d": {"ms": round(h2d_ms, 3), "gib_per_s": round(mb / h2d_ms / 1073741.824, 2)},
        "dual_only": {"ms": round(dual_ms, 3), "gib_per_s": round(db / dual_ms / 1073741.824, 2)},
        "fused_over_h2d": round(fused_ms / h2d_ms, 3),
        "fused_over_dual_only": round(fused_ms / dual_ms, 3),
        "dual_only_plus_extra_h2d_ms": round(dual_ms + extra_h2d, 3),
        "excess_ms": round(fused_ms - dual_ms - extra_h2d, 3),
        "kernels_ms": kern,
        "ventry_verify": {"compressions_per_answer": round(float(comp), 2),
                          "g_compressions_per_s": round(rate / 1e9, 3),
                          "of_sha_ceiling_30.9": round(rate / 30.9e9, 3)},
        "checked": "every answer ok; new_tx of the first block; a sample vs the CPU reference"}))
    ctx.close()


if __name__ == "__main__":
    main()
