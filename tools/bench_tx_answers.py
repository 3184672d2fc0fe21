#!/usr/bin/env python3
"""Throughput of mh_tx_answer_pb_batch (db.TxByID / db.TxScan under an
EntriesSpec in one device pass) beside mh_export_tx_batch over the same txs of
the same store, which hashes and copies the same values with the same loop:
--txs txs of --entries kv entries with --value-len byte values (the default is
export_util.big_store's shape with 4 KiB values), resident, kv RAW_VALUE, out
on the device.

One JSON line:

  tx_answers / export   ms per call (median, min, max of --reps after --warmup;
                        host clock around the synchronous call) and GiB/s of
                        value bytes, the two calls timed alternately in the
                        same run; `spread` is (max - min) / median
  rounds                the medians of --rounds repetitions of that comparison
                        in the same session (the run-to-run spread)
  kernels_ms            per-kernel times of one call of each from mh_ctx_timing
                        (a separate call: timing serialises the launches)
  value_kernels         txs_values against exp_values_store, and each against
                        the measured SHA ceiling (30.9 G compressions/s,
                        DESIGN.md section 4) from (vLen + 72) / 64 per value
  verifiable            the same requests as VERIFIABLE with prove_since = tx

    python3 tools/bench_tx_answers.py
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "oracle"), os.path.join(HERE, "tests"), os.path.join(HERE, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from bench_export import SHA_CEILING, build_store, summary, timed  # noqa: E402

KERNELS = ("ans_heads", "ans_compact", "txlog_struct", "txlog_lanes", "txlog_wave", "tx_alh", "ans_verdict",
           "txe_index", "txs_variants", "txs_plan", "txs_vsize", "pb_dual1_size", "txs_size", "txs_place",
           "txs_header", "txs_entries", "varlen_sort", "txs_values", "txs_copy", "txs_assemble",
           "pb_dual1_write", "txs_status",
           "exp_counts", "exp_entry", "exp_tx", "exp_offsets", "exp_head", "exp_keys", "exp_values_store",
           "exp_status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=17)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--value-len", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=3, help="answers checked against the CPU restatement")
    a = ap.parse_args()
    import torch
    import immustore_amd as m
    from immustore_amd import _native as N
    from immustore_amd import answers
    import export_util as X
    import tx_spec_util as U
    N_, w, vl = a.txs, a.entries, a.value_len
    raw, clog, vals = build_store(N_, w, vl)
    ctx = m.Context(0)
    L = N.load()
    os.environ["MH_EXPORT_ARM"] = "A"
    dev = m.ExportStore(raw, clog, [vals], ctx=ctx)
    ref = U.SpecStore(X.ExpStore(raw, clog, [(0, vals)]))
    tree = m.AHtree(ctx)
    tree.append_batch(np.frombuffer(b"".join(ref.ans.alhs), np.uint8).reshape(-1, 32))
    s = dev.descriptor()
    n_val, vbytes = N_ * w, N_ * w * vl
    spec = (U.RAW_VALUE, None, None)
    txs = list(range(1, N_ + 1))

    def answer(kind, out, cap):
        return answers.tx_answers_raw(dev, tree if kind else None, [kind] * N_, txs, txs, [spec] * N_, U.NOW,
                                      out, cap)

    off, st = answer(U.TXA_TX, None, 0)
    total = int(off[N_])
    voff, _ = answer(U.TXA_VERIFIABLE, None, 0)
    vtotal = int(voff[N_])
    eoff, est, etr = np.zeros(N_ + 1, np.uint64), np.zeros(N_, np.int32), np.zeros(N_, np.uint8)

    def export(out, cap):
        N.check(L.mh_export_tx_batch(ctx.handle, C.addressof(s), 1, N_, out, cap, eoff.ctypes.data,
                                     est.ctypes.data, etr.ctypes.data))

    export(None, 0)
    etotal = int(eoff[N_])
    dout = torch.empty(max(total, vtotal, etotal) + 64, dtype=torch.uint8, device="cuda:0")
    # ---- correctness: a sample of the answers against the restatement
    off, st = answer(U.TXA_TX, dout.data_ptr(), total)
    assert not st.any(), "the store is not served cleanly"
    got = dout[:total].cpu().numpy()
    for t in np.linspace(1, N_, a.sample).astype(int):
        e = U.expect_one(ref, U.TXA_TX, int(t), 0, spec)
        assert e[0] == 0 and bytes(got[int(off[t - 1]):int(off[t])]) == e[1], t
    voff, st = answer(U.TXA_VERIFIABLE, dout.data_ptr(), vtotal)
    assert not st.any()
    got = dout[:vtotal].cpu().numpy()
    e = U.expect_one(ref, U.TXA_VERIFIABLE, N_, N_, spec)
    assert bytes(got[int(voff[N_ - 1]):int(voff[N_])]) == e[1]
    # ---- the two calls, alternately; the comparison repeated
    calls = {"tx_answers": lambda: answer(U.TXA_TX, dout.data_ptr(), total),
             "export": lambda: export(dout.data_ptr(), etotal)}
    res = {"shape": {"txs": N_, "entries": w, "value_len": vl, "value_bytes": vbytes, "answer_bytes": total,
                     "blob_bytes": etotal},
           "rounds": {k: [] for k in calls}}
    for fn in calls.values():
        timed(fn, a.warmup, 0)
    for rnd in range(a.rounds):
        rows = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                rows[k] += timed(fn, 0, 1)
        for k in calls:
            r = summary(rows[k])
            r["spread"] = round((r["max_ms"] - r["min_ms"]) / r["median_ms"], 3)
            r["value_GiBps"] = round(vbytes / 2 ** 30 / (r["median_ms"] * 1e-3), 1)
            res["rounds"][k].append(r["median_ms"])
            if rnd == 0:
                res[k] = r
    for k in calls:
        med = res["rounds"][k]
        res[k]["run_to_run_spread"] = round((max(med) - min(med)) / statistics.median(med), 3)
    res["ratio_to_export"] = round(statistics.median(res["rounds"]["tx_answers"]) /
                                   statistics.median(res["rounds"]["export"]), 3)
    r = summary(timed(lambda: answer(U.TXA_VERIFIABLE, dout.data_ptr(), vtotal), a.warmup, a.reps))
    r["value_GiBps"] = round(vbytes / 2 ** 30 / (r["median_ms"] * 1e-3), 1)
    res["verifiable"] = r
    # ---- per-kernel times, the value kernels against each other and the SHA ceiling
    comps = n_val * ((vl + 72) >> 6)
    res["kernels_ms"] = {}
    for k, fn in calls.items():
        ctx.set_timing(True)
        ctx.timing_reset()
        fn()
        ks = {}
        for name in KERNELS:
            ms, cnt = ctx.timing(name)
            if cnt:
                ks[name] = round(ms, 4)
        ctx.set_timing(False)
        ctx.timing_reset()
        res["kernels_ms"][k] = ks
    tv, ev = res["kernels_ms"]["tx_answers"]["txs_values"], res["kernels_ms"]["export"]["exp_values_store"]
    res["value_kernels"] = {"txs_values_ms": tv, "exp_values_store_ms": ev, "ratio": round(tv / ev, 3),
                            "compressions": comps,
                            "txs_values_of_sha_ceiling_30.9": round(comps / (tv * 1e-3) / SHA_CEILING, 3),
                            "exp_values_store_of_sha_ceiling_30.9": round(comps / (ev * 1e-3) / SHA_CEILING, 3)}
    dev.close()
    tree.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
