#!/usr/bin/env python3
"""Throughput of mh_export_tx_batch (ImmuStore.ExportTx for a run of txs of a
resident store in one device pass) beside the calls that could already do its
parts, in the shape of the replicate benchmark: --txs txs of --entries entries
with --value-len byte values, resident, out on the device.

One JSON line:

  arm_A / arm_B   ms per call (median, min, max of --reps after --warmup; host
                  clock around the synchronous call) and GiB/s of value bytes,
                  the two arms timed alternately in the same run: A the hashing
                  lane stores its own blocks, B hash-only lanes and a wave-per-
                  value copy kernel (MH_EXPORT_ARM)
  pinned_out      the same call (the default arm) with out in pinned host
                  memory: bound by the PCIe copy of the blobs
  composition     what the calls before this one do for the same bytes:
                  mh_txlog_validate_clog over the range + mh_dev_verify_values_batch
                  over the same values with host-built offsets + one device-to-
                  device copy of off[count] bytes, each timed alone and summed;
                  `spread` is (max - min) / median of the sum over the reps
  target          the kept arm against 1.15 x that sum (or 1 + spread when the
                  spread is above 15 %)
  kernels_ms      per-kernel times of one call of each arm from mh_ctx_timing (a
                  separate call: timing serialises the launches)
  value_kernel    the value kernel's share of the measured SHA ceiling (30.9 G
                  compressions/s) from the compressions the
                  shapes imply, (vLen + 72) / 64 per value

    python3 tools/bench_export.py
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

SHA_CEILING = 30.9e9
KERNELS = ("txlog_struct", "txlog_lanes", "txlog_wave", "exp_counts", "txe_index", "exp_entry", "exp_tx",
           "exp_offsets", "exp_head", "exp_keys", "varlen_sort", "exp_values_store", "exp_values_hash", "exp_copy",
           "exp_status")


def build_store(N, w, vlen, seed=3):
    """-> (raw tx log, 12-byte cLog, vLog 1): a chain of N v1 txs of w entries
    with 8-byte keys, BlTxID = id - 1, the values back to back in vLog 1"""
    import oracle as orc
    sha = lambda b: hashlib.sha256(b).digest()  # noqa: E731
    vals = np.random.default_rng(seed).integers(0, 256, N * w * vlen, dtype=np.uint8).tobytes()
    raw, clog = bytearray(), bytearray()
    aht = orc.AHtree(N)
    prev = sha(b"")
    for k in range(1, N + 1):
        ents, lv = bytearray(), []
        for j in range(w):
            at = ((k - 1) * w + j) * vlen
            key = struct.pack(">Q", (k << 16) | j)
            hv = sha(vals[at:at + vlen])
            lv.append(sha(b"\x00" + sha(b"\x00\x00\x00\x08" + key + hv)))
            ents += b"\x00\x00\x00\x08" + key + struct.pack(">IQ", vlen, (1 << 56) | at) + hv
        while len(lv) > 1:
            lv = [sha(b"\x01" + lv[i] + lv[i + 1]) if i + 1 < len(lv) else lv[i]
                  for i in range(0, len(lv), 2)]
        bl, blroot = k - 1, bytes(32)
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
        prev = alh
    return bytes(raw), bytes(clog), vals


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=4096)
    ap.add_argument("--entries", type=int, default=16)
    ap.add_argument("--value-len", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sample", type=int, default=5, help="blobs checked against the CPU restatement")
    ap.add_argument("--kept", default=None, help="the arm the target is judged on (default: the faster)")
    a = ap.parse_args()
    import torch
    import immustore_amd as m
    from immustore_amd import _native as N
    import export_util as X
    N_, w, vl = a.txs, a.entries, a.value_len
    raw, clog, vals = build_store(N_, w, vl)
    ctx = m.Context(0)
    L = N.load()
    dev = m.ExportStore(raw, clog, [vals], ctx=ctx)
    s = dev.descriptor()
    n_val = N_ * w
    vbytes = n_val * vl
    off = np.zeros(N_ + 1, np.uint64)
    st = np.zeros(N_, np.int32)
    tr = np.zeros(N_, np.uint8)

    def call(out, cap):
        N.check(L.mh_export_tx_batch(ctx.handle, C.addressof(s), 1, N_, out, cap, off.ctypes.data,
                                     st.ctypes.data, tr.ctypes.data))

    call(None, 0)
    total = int(off[N_])
    dout = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
    dsrc = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
    # ---- correctness of both arms: a sample against the restatement, A == B everywhere
    ref = X.ExpStore(raw, clog, [(0, vals)])
    outs = {}
    for arm in "AB":
        os.environ["MH_EXPORT_ARM"] = arm
        dout.zero_()
        call(dout.data_ptr(), total)
        assert not st.any() and not tr.any(), "the store does not export cleanly"
        outs[arm] = dout[:total].cpu().numpy().copy()
    assert np.array_equal(outs["A"], outs["B"])
    for t in np.linspace(1, N_, a.sample).astype(int):
        stt, blob, _, _ = ref.export_one(int(t))
        assert stt == 0 and bytes(outs["A"][int(off[t - 1]):int(off[t])]) == blob, t
    # ---- the two arms, alternately
    arms = {"A": [], "B": []}
    for arm in "AB":
        os.environ["MH_EXPORT_ARM"] = arm
        timed(lambda: call(dout.data_ptr(), total), a.warmup, 0)
    for _ in range(a.reps):
        for arm in "AB":
            os.environ["MH_EXPORT_ARM"] = arm
            arms[arm] += timed(lambda: call(dout.data_ptr(), total), 0, 1)
    res = {"shape": {"txs": N_, "entries": w, "value_len": vl, "value_bytes": vbytes, "blob_bytes": total}}
    for arm in "AB":
        r = summary(arms[arm])
        r["value_GiBps"] = round(vbytes / 2 ** 30 / (r["median_ms"] * 1e-3), 1)
        res["arm_" + arm] = r
    kept = a.kept or min("AB", key=lambda x: res["arm_" + x]["median_ms"])
    os.environ["MH_EXPORT_ARM"] = kept
    # ---- per-kernel times, the value kernel against the SHA ceiling
    comps = n_val * ((vl + 72) >> 6)
    res["kernels_ms"] = {}
    for arm in "AB":
        os.environ["MH_EXPORT_ARM"] = arm
        ctx.set_timing(True)
        ctx.timing_reset()
        call(dout.data_ptr(), total)
        ks = {}
        for name in KERNELS:
            ms, cnt = ctx.timing(name)
            if cnt:
                ks[name] = round(ms, 4)
        ctx.set_timing(False)
        ctx.timing_reset()
        res["kernels_ms"][arm] = ks
    os.environ["MH_EXPORT_ARM"] = kept
    vk = res["kernels_ms"][kept]["exp_values_store" if kept == "A" else "exp_values_hash"]
    res["value_kernel"] = {"arm": kept, "ms": vk, "compressions": comps,
                           "of_sha_ceiling_30.9": round(comps / (vk * 1e-3) / SHA_CEILING, 3)}
    # ---- out in pinned host memory (PCIe-bound)
    pin = C.c_void_p()
    N.check(L.mh_host_alloc_pinned(total + 64, C.byref(pin)))
    r = summary(timed(lambda: call(pin.value, total), a.warmup, a.reps))
    r["blob_GiBps"] = round(total / 2 ** 30 / (r["median_ms"] * 1e-3), 1)
    r["note"] = "PCIe-bound: the blobs are copied down once"
    res["pinned_out"] = r
    assert bytes(C.string_at(pin.value, 4096)) == bytes(outs["A"][:4096])
    N.check(L.mh_host_free_pinned(pin.value))
    # ---- the composition the calls before this one offer for the same bytes
    voff = np.arange(n_val + 1, dtype=np.uint64) * vl
    hv = np.frombuffer(b"".join(hashlib.sha256(vals[i * vl:(i + 1) * vl]).digest() for i in range(n_val)),
                       np.uint8)
    d_off, d_hv, d_st = (torch.from_numpy(x.copy()).to("cuda:0") for x in
                         (voff.view(np.uint8), hv, np.zeros(n_val * 4, np.uint8)))
    vst = np.zeros(N_, np.int32)
    nbad, first = C.c_uint64(), C.c_uint64()

    def rehash():
        N.check(L.mh_txlog_validate_clog(ctx.handle, s.txlog, s.txlog_len, s.clog, N_, 12, 1024, 1024,
                                         None, None, vst.ctypes.data, C.byref(nbad), C.byref(first)))

    def values():
        N.check(L.mh_dev_verify_values_batch(ctx.handle, n_val, dev._vl[0].data, d_off.data_ptr(), None,
                                             d_hv.data_ptr(), d_st.data_ptr()))
        ctx.synchronize()

    def d2d():
        dout[:total].copy_(dsrc[:total])
        torch.cuda.synchronize()

    parts = {"txlog_validate_clog": rehash, "dev_verify_values_batch": values, "device_copy": d2d}
    for fn in parts.values():
        timed(fn, a.warmup, 0)
    rows = {k: [] for k in parts}
    for _ in range(a.reps):
        for k, fn in parts.items():
            rows[k] += timed(fn, 0, 1)
    assert nbad.value == 0 and not d_st.cpu().numpy().any()
    sums = [sum(rows[k][i] for k in parts) for i in range(a.reps)]
    comp = {k: summary(v) for k, v in rows.items()}
    comp["sum"] = summary(sums)
    spread = (max(sums) - min(sums)) / statistics.median(sums)
    comp["spread"] = round(spread, 3)
    res["composition"] = comp
    margin = 1.15 if spread <= 0.15 else 1 + spread
    ratio = res["arm_" + kept]["median_ms"] / comp["sum"]["median_ms"]
    res["target"] = {"kept_arm": kept, "ratio_to_composition": round(ratio, 3), "margin": round(margin, 3),
                     "met": bool(ratio <= margin)}
    dev.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
