#!/usr/bin/env python3
"""Secondary benchmarks for BASELINE.json configs other than the headline one.

  --workload c3     configs[2]: embedded/ahtree batch append of 10^7 x 32 B
                    tx-hash payloads to an empty tree, device resident
                    (leaves + perfect nodes + spine chains = the full dLog).
  --workload c5     configs[4]: htree.VerifyInclusion re-hash of 10^6 proofs of
                    depth 24 over a 2^24-leaf tree, 10 % tampered, bit-exact
                    result bitmap checked against the expected count; plus the
                    ahtree set: 10^6 inclusion + 10^6 consistency proofs over a
                    2^24-append tree (j = 2^24, random i), 10 % tampered.
  --workload c2e2e  configs[1] end to end: entries copied host->device from
                    pinned memory, build, levels + root copied back (PCIe
                    inclusive rate, for DESIGN.md; never the headline value).
  --workload txlog  SURVEY.md 8(a) a14: tx-log read-path validation
                    (tx.go:388-630) of 2^16 records x 16 entries (16 B keys,
                    v1, no metadata) through mh_txlog_validate: host parse,
                    H2D, entry digests + one htree per tx + Alh on the GPU.
  --workload wire   SURVEY.md 8(f) row 4: proofs as protobuf messages built on
                    the device -- 10^6 DualProofV2 (ImmuStore.DualProofV2 over
                    a 2^24-append ahtree + TxHeader encoding) and 10^6 htree
                    InclusionProof messages over a 2^24-leaf tree; sizes pass,
                    scan, write pass; a sample checked against oracle/wire.py;
                    then the same 10^6 DualProofV2 messages decoded back
                    (mh_dual_proof_v2_pb_decode_batch, host buffers).
  --workload ragged SURVEY.md 8(a) a1-a4 over ragged EntrySpecs (the general
                    CSR entry path, mh_dev_htree_build_entries): 2^20 entries,
                    value length uniform in [0, 4096] (MaxValueLen), keys of
                    8-64 B, KV metadata of 0-11 B, v1, device resident;
                    value hashes + entry digests + leaves + all levels; SHA
                    ceiling fraction of the ragged-message kernel; root and
                    hVals checked against the oracle.
  --workload document  pkg/verification.VerifyDocument (verification.go:37-196, the
                    package configs[4] names) over a batch: 8192 documents, each in its
                    own v1 transaction of 64 entries (KV metadata on some), a trivial
                    DualProofV2 (source = target = the tx) and the tx as known state,
                    inputs in pinned host memory as a cgo caller hands them over;
                    mh_verify_document_batch end to end; every status / Alh checked
                    against the oracle on a sample.
  --workload commit SURVEY.md 8(f) row 1: ImmuStore.precommit hashing over a
                    batch of 2^16 txs x 16 entries x 1 KiB values (8 B keys,
                    v1) in pinned host memory through mh_precommit_batch: value
                    hashes, entry digests, one htree per tx, hVals + Eh copied
                    back; chunked two-stream pipeline vs one chunk, next to the
                    plain pinned H2D rate of the same bytes (the PCIe bound) and
                    the oracle on 16 host threads.
  --workload dualv1 the proof immudb serves: 10^5 ImmuStore.DualProof (v1, with
                    LinearProof and LinearAdvanceProof) over a 2^20-append ahtree
                    whose BlTxID lags each tx by 1-4 txs, generated and marshalled
                    as schema.DualProof on the device from the resident dLog and a
                    resident Alh / innerHash window (mh_dev_dual_proof_pb_batch:
                    sizes pass, scan, write pass); proofs/s and output GiB/s; a
                    sample checked against the CPU restatement of the tests.
  --workload dualv1verify  the client's side of that wire: about 1 GiB of DualProof
                    (v1) messages (device-generated over the tests' synthetic store of
                    3000 txs, so every proof really verifies) in pinned host memory,
                    verified (a) by mh_dual_proof_pb_decode_batch then
                    mh_verify_dual_proof_batch with pinned host arrays and (b) by the
                    fused mh_verify_dual_proof_pb_batch, timed in the same run, next to
                    the pinned H2D time of the message bytes; a sample of verdicts
                    checked against the oracle.

Each prints one JSON line.  bench.py stays the driver's headline benchmark.

Under torch.distributed.run (WORLD_SIZE > 1, one process per GPU) c3 and c5 run
their SURVEY.md 8(e) multi-GPU forms, weak scaling:
  c3  every rank appends 2^23 payloads of one global batch (shard = 2^23):
      local leaves + perfect levels, RCCL all-gather of the 32-byte shard roots,
      cross-shard nodes, spine (immustore_amd/sharding.py).
  c5  every rank re-hashes its own 10^6 proofs (split by index, no collective
      in the timed region).
MH_DIST_BACKEND=gloo rehearses several ranks on one GPU.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def timed(step, steps, warmup, sync):
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return (time.perf_counter() - t0) / steps


def timed_k(ctx, fn, steps, warmup, sync):
    """timed() with the context's per-kernel timing events off, then the same
    steps again with them on for the kernel times (ctx.timing: steps + warmup
    launches): the events add a few microseconds per launch, which a timed
    region of many small launches would otherwise carry."""
    t = timed(fn, steps, warmup, sync)
    ctx.timing_reset()
    ctx.set_timing(True)
    timed(fn, steps, warmup, sync)
    ctx.set_timing(False)
    return t


def prewarm(step, sync, seconds):
    """Run `step` untimed for `seconds` so the GPU clock reaches its sustained
    value before the timed region (the headline bench's 2000 steps do the same;
    a few-step run right after setup otherwise measures the clock ramp)."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        step()
        sync()


SPLITMIX_G = 0x9E3779B97F4A7C15


def _oracle():
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as orc
    orc.use_shani(True)
    return orc


def host_threads(share=1):
    """Host threads this process may use, split over `share` processes."""
    try:
        avail = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        avail = os.cpu_count() or 1
    return max(1, avail // max(share, 1))


def corrupt_hook(buf, who, at=100):
    """Test-only (MH_BENCH_CORRUPT=<rank>): flip byte `at` of this rank's
    inputs after they were generated, so its result check must fail."""
    if os.environ.get("MH_BENCH_CORRUPT", "") == str(who):
        buf[at:at + 1].bitwise_xor_(1)
        return True
    return False


def aht_samples(lo, hi, rng, edge=64, rand=256):
    """Appends of the range (lo, hi] the check looks at: the first and last
    `edge` and `rand` random ones (the last is always included: RootAt(hi))."""
    import numpy as np
    cnt = hi - lo
    s = set(range(lo + 1, lo + 1 + min(edge, cnt))) | set(range(max(lo + 1, hi - edge + 1), hi + 1))
    s |= set(int(x) for x in rng.integers(lo + 1, hi + 1, rand))
    return np.array(sorted(s), np.uint64)


def c3_rank_check(orc, seed, plen, lo, hi, dlog_rows, root_rows, samples, threads):
    """One rank's ahtree range (lo, hi] against the oracle without rebuilding
    the tree: the peaks of lo from the payload stream in blocks
    (orc.ahtree_peaks_streamed), then the range streamed from them
    (orc.ahtree_stream, ahtree.go:287-322), every digest each sampled append
    wrote and its RootAt compared.  dlog_rows(idx) / root_rows(idx) return the
    device's rows at range-relative indices as (len, 32) host arrays.
    -> (ok, RootAt(hi) of the oracle)."""
    import numpy as np
    up = orc.nodes_upto
    pk = orc.ahtree_peaks_streamed(seed, plen, lo, threads=threads) if lo else None
    ref, _ = orc.ahtree_stream(seed, plen, lo, hi, samples, peaks_in=pk)
    base = up(lo)
    idx, want = [], []
    for n in (int(x) for x in samples):
        first = up(n - 1) - base  # nodesUntil(n), range-relative
        idx.extend(range(first, first + len(ref[n])))
        want.extend(ref[n])
    got = dlog_rows(np.array(idx, np.int64))
    ok = bool(np.array_equal(got, np.frombuffer(b"".join(want), np.uint8).reshape(-1, 32)))
    r = root_rows(samples.astype(np.int64) - lo - 1)
    ok &= bool(np.array_equal(r, np.frombuffer(b"".join(ref[int(n)][-1] for n in samples),
                                               np.uint8).reshape(-1, 32)))
    return ok, ref[int(hi)][-1]


def c5_rank_check(orc, leaf, W, terms, digests, root, ok_dev, tamper, sample):
    """One rank's VerifyInclusion bitmap: every verdict equals the expected
    one (~tamper), and on `sample` the oracle's htree.VerifyInclusion
    (htree.go:166-195) over the very same terms / digests / root gives the
    device's verdicts.  terms (s, D, 32), digests (s, 32) host arrays of the
    sampled proofs.  -> (ok, sampled verdicts agreeing)."""
    import numpy as np
    exact = bool((ok_dev.astype(bool) == ~tamper).all())
    _, ok_o = orc.htree_verify_batch(leaf[sample].astype(np.uint64), W, terms, digests, root)
    agree = bool((ok_o.astype(bool) == ok_dev[sample].astype(bool)).all())
    return exact and agree, int(len(sample))


def share_verdict(dist, backend, dev, ok, corrupted, payload=b""):
    """All-gather a 64-byte record per rank (verdict, corrupted flag, 32 B
    payload) -> (every rank ok, corrupted ranks, payloads in rank order)."""
    import numpy as np
    import torch
    rec = np.zeros(64, np.uint8)
    rec[0], rec[1] = int(ok), int(corrupted)
    rec[32:32 + len(payload)] = np.frombuffer(payload, np.uint8)
    on = torch.device("cpu") if backend == "gloo" else dev
    world = dist.get_world_size()
    g = torch.empty(world * 64, dtype=torch.uint8, device=on)
    dist.all_gather_into_tensor(g, torch.from_numpy(rec).to(on))
    recs = g.cpu().numpy().reshape(world, 64)
    return (bool(all(recs[:, 0] == 1)), [r for r in range(world) if recs[r, 1]],
            [recs[r, 32:64].tobytes() for r in range(world)])


def distributed_main(a):
    """One process per GPU (torch.distributed.run; MH_DIST_FORCE_PG=1 runs the
    same code as one rank over a real process group).  c3 / c5 in their
    SURVEY.md 8(e) multi-GPU forms, weak scaling; every line checks its result
    against the oracle after the timed region and exits 1 on a mismatch."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import immustore_amd as m
    from immustore_amd import _native as N
    from immustore_amd import sharding

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    backend = os.environ.get("MH_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    if backend == "gloo":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    stream = torch.cuda.current_stream(dev)
    ctx = m.Context(dev.index, stream.cuda_stream)
    L = N.load()
    on = torch.device("cpu") if backend == "gloo" else dev
    threads = host_threads(int(os.environ.get("LOCAL_WORLD_SIZE", world)))

    def sync_all():
        torch.cuda.synchronize(dev)
        dist.barrier()
        torch.cuda.synchronize(dev)

    def timed_max(step):
        # clock pre-warm as the single-GPU lines: chunks of 4 steps until
        # a.prewarm seconds have passed, every rank deciding after the same
        # chunk (a step may hold a collective)
        if a.prewarm > 0:
            tp = time.perf_counter()
            while True:
                for _ in range(4):
                    step()
                sync_all()
                more = torch.tensor([int(time.perf_counter() - tp < a.prewarm)], dtype=torch.int64,
                                    device=on)
                dist.all_reduce(more, op=dist.ReduceOp.MAX)
                if not int(more.item()):
                    break
        for _ in range(a.warmup):
            step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        sync_all()
        t = torch.tensor([(time.perf_counter() - t0) / a.steps], dtype=torch.float64, device=on)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    if a.workload == "c3":
        # every rank appends 2^23 payloads of one global batch onto an empty
        # tree, keeping ONLY its own dLog range (the ranged
        # form of mh_multi_dev_ahtree_append_batch): leaves + perfect levels,
        # one all-gather of its pieces' level-k roots, the piece tree, spines
        from immustore_amd.multi import ahtree_range_plan
        up = L.mh_ahtree_nodes_upto
        seed, plen, n0 = 3, 32, 0
        total = world * a.per_rank
        k, b = ahtree_range_plan(n0, total, world)
        G = len(b) - 1
        send_b, work_b = sharding.ahtree_range_sizes(n0, total, world)
        lo, hi = (b[rank], b[rank + 1]) if rank < G else (b[G], b[G])
        cnt = hi - lo
        pay = torch.empty(max(cnt, 1) * plen, dtype=torch.uint8, device=dev)
        sd = (seed + lo * (plen // 8) * SPLITMIX_G) & 0xFFFFFFFFFFFFFFFF  # payload lo of the stream
        N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), sd))
        torch.cuda.synchronize(dev)
        corrupted = corrupt_hook(pay, rank)
        dlog = torch.empty(max(up(hi) - up(lo), 1) * 32, dtype=torch.uint8, device=dev)
        ro = torch.empty(max(cnt, 1) * 32, dtype=torch.uint8, device=dev)
        work = torch.empty(work_b, dtype=torch.uint8, device=dev)
        send = torch.zeros(send_b, dtype=torch.uint8, device=dev)
        recv = torch.empty(world * send_b, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def exchange():
            if backend == "gloo":
                r = torch.empty(world * send_b, dtype=torch.uint8)
                dist.all_gather_into_tensor(r, send.cpu())
                recv.copy_(r)
            else:
                dist.all_gather_into_tensor(recv, send)

        def step():
            sharding.ahtree_range_append(ctx, n0, None, total, world, rank, pay.data_ptr(), plen,
                                         dlog.data_ptr(), work.data_ptr(), send.data_ptr(),
                                         recv.data_ptr(), exchange if G > 1 else None,
                                         ro.data_ptr())

        t = timed_max(step)
        # ---- check vs the oracle, after the timed region
        tc = time.perf_counter()
        orc = _oracle()
        ok, root_o = True, b"\0" * 32
        samples = np.zeros(0, np.uint64)
        if cnt:
            samples = aht_samples(lo, hi, np.random.default_rng(7 + rank))
            dl, rr = dlog.view(-1, 32), ro.view(-1, 32)
            rows = lambda t_, i: t_[torch.from_numpy(i).to(dev)].cpu().numpy()  # noqa: E731
            ok, root_o = c3_rank_check(orc, seed, plen, lo, hi, lambda i: rows(dl, i),
                                       lambda i: rows(rr, i), samples, threads)
        ok_all, bad, roots = share_verdict(dist, backend, dev, ok, corrupted, root_o)
        rcheck = {"vs": "oracle", "ok": ok_all, "n": total, "ranges": G, "shard_bits": k,
                  "root": roots[G - 1].hex(), "samples_per_rank": int(len(samples)),
                  "corrupted_ranks": bad, "host_threads_per_rank": threads,
                  "seconds": round(time.perf_counter() - tc, 2),
                  "what": "per rank: the oracle's peaks of its range start (payload stream "
                          "hashed block by block) and its range streamed from them "
                          "(oracle/orc_ahtree_stream, ahtree.go:287-322); every dLog digest "
                          "and RootAt of 64 first, 64 last and 256 random appends compared "
                          "(RootAt(n) of the last rank = the batch's root)"}
        new_digests = up(n0 + total) - up(n0)
        out = {"metric": "ahtree batch append, sharded, %d payloads per GPU (configs[2] at scale)"
                         % a.per_rank,
               "value": round(total / t / 1e6, 3), "unit": "M appends/s", "n_gpus": world,
               "ms_per_step": round(t * 1e3, 3), "scaling": "weak", "appends_total": total,
               "dlog_bytes_this_rank": int(dlog.numel()),
               "dlog_bytes_whole_tree": int(new_digests * 32),
               "exchange": "all-gather of %d B per rank (%s)" % (send_b, backend),
               "root_check": rcheck}
    elif a.workload == "c5":
        # proofs are independent: every rank re-hashes its own share (split by
        # index, its own seed) against the replicated 2^D-leaf tree, with no
        # collective in the timed region
        D, P = a.depth, a.proofs
        W = 1 << D
        dig = torch.empty(W * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, dig.data_ptr(), dig.numel(), 5))
        levels = torch.empty(m.levels_len(W) * 32, dtype=torch.uint8, device=dev)
        root = torch.empty(32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_htree_build_digests(ctx.handle, dig.data_ptr(), W, levels.data_ptr(),
                                             root.data_ptr()))
        rng = np.random.default_rng(5 + rank)  # this rank's share of the proofs
        leaf = rng.integers(0, W, P, dtype=np.int64)
        leaf_t = torch.from_numpy(leaf).to(dev)
        terms = torch.empty(P * D * 32, dtype=torch.uint8, device=dev)
        nterms = torch.empty(P, dtype=torch.int32, device=dev)
        pst = torch.empty(P, dtype=torch.int32, device=dev)
        N.check(L.mh_dev_htree_inclusion_proof_batch(ctx.handle, levels.data_ptr(), W, P,
                                                     leaf_t.data_ptr(), terms.data_ptr(), D,
                                                     nterms.data_ptr(), pst.data_ptr()))
        torch.cuda.synchronize(dev)
        assert int(pst.abs().sum().item()) == 0 and int((nterms != D).sum().item()) == 0
        tamper = rng.random(P) < 0.10
        src = np.where(tamper, (leaf + 1) % W, leaf)  # a wrong digest for 10 %
        digests = dig.view(-1, 32)[torch.from_numpy(src).to(dev)].contiguous()
        roots = root.view(1, 32).expand(P, 32).contiguous()
        width_t = torch.full((P,), W, dtype=torch.int64, device=dev)
        toff = torch.arange(0, (P + 1) * D, D, dtype=torch.int64, device=dev)
        ok = torch.zeros(P, dtype=torch.uint8, device=dev)
        # test hook: one term of the first untampered proof flipped
        first_good = int(np.nonzero(~tamper)[0][0])
        corrupted = corrupt_hook(terms, rank, at=first_good * D * 32 + 5)
        torch.cuda.synchronize(dev)

        def step():
            N.check(L.mh_dev_htree_verify_inclusion_batch(
                ctx.handle, P, leaf_t.data_ptr(), width_t.data_ptr(), toff.data_ptr(),
                terms.data_ptr(), digests.data_ptr(), roots.data_ptr(), ok.data_ptr()))

        t = timed_max(step)
        tc = time.perf_counter()
        orc = _oracle()
        okh = ok.cpu().numpy()
        srng = np.random.default_rng(11 + rank)
        sample = np.unique(np.concatenate([np.arange(min(P, 1 << 13)),
                                           srng.integers(0, P, 1 << 13)]))
        if corrupted:
            sample = np.unique(np.concatenate([sample, [first_good]]))
        st = torch.from_numpy(sample).to(dev)
        th = terms.view(P, D, 32)[st].cpu().numpy()
        dh = digests[st].cpu().numpy()
        rk_ok, ns = c5_rank_check(orc, leaf, W, th, dh, root.cpu().numpy().tobytes(), okh, tamper,
                                  sample)
        nver = int(okh.astype(bool).sum())
        ok_all, bad, _ = share_verdict(dist, backend, dev, rk_ok, corrupted)
        tot = torch.tensor([nver], dtype=torch.int64, device=on)
        dist.all_reduce(tot)
        rcheck = {"vs": "oracle", "ok": ok_all, "proofs": world * P, "verified": int(tot.item()),
                  "sampled_per_rank": ns, "corrupted_ranks": bad,
                  "seconds": round(time.perf_counter() - tc, 2),
                  "what": "per rank: every verdict equals the expected bitmap (10 % tampered "
                          "digests false, the rest true), and the oracle's VerifyInclusion "
                          "(htree.go:166-195) over the same terms / digests / root of >= 2^13 "
                          "proofs gives the device's verdicts"}
        out = {"metric": "htree inclusion-proof re-hash, %d proofs x depth %d per GPU" % (P, D),
               "value": round(world * P / t / 1e6, 3), "unit": "M proofs/s", "n_gpus": world,
               "ms_per_step": round(t * 1e3, 3), "scaling": "weak", "root_check": rcheck}
    else:
        raise SystemExit("multi-GPU mode covers --workload c3 / c5")
    out["workload"] = a.workload
    out["process_group"] = {"backend": backend, "world_size": dist.get_world_size()}
    if rank == 0:
        print(json.dumps(out), flush=True)
    ctx.close()
    dist.destroy_process_group()
    if not out["root_check"]["ok"]:
        print("root_check FAILED: %s" % json.dumps(out["root_check"]), file=sys.stderr, flush=True)
        raise SystemExit(1)


def make_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", choices=["c3", "c5", "c2e2e", "txlog", "commit", "wire", "ragged", "document",
                                          "values", "c3range", "dualv1", "dualv1verify", "replicate"],
                   required=True)
    p.add_argument("--logs", action="store_true",
                   help="c3: also write the pLog / cLog appendable records (8(f) row 4)")
    p.add_argument("--txs", type=int, default=1 << 16, help="txlog records")
    p.add_argument("--tx-entries", type=int, default=16, help="txlog entries per record")
    p.add_argument("--vlen", type=int, default=1024, help="commit value bytes")
    p.add_argument("--chunk-mib", type=int, default=64, help="commit pipeline chunk")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--prewarm", type=float, default=0.5,
                   help="seconds of untimed steps before each device-resident timed region")
    p.add_argument("--m", type=int, default=10 ** 7, help="c3 appends")
    p.add_argument("--per-rank", type=int, default=1 << 23,
                   help="c3 under torch.distributed: appends per rank (weak scaling)")
    p.add_argument("--proofs", type=int, default=10 ** 6, help="c5 proofs")
    p.add_argument("--depth", type=int, default=24, help="c5 tree depth")
    p.add_argument("--no-ahtree", action="store_true", help="c5: htree proofs only")
    p.add_argument("--entries", type=int, default=1 << 20, help="ragged entries")
    p.add_argument("--max-vlen", type=int, default=4096, help="ragged: max value length")
    p.add_argument("--no-check", action="store_true", help="ragged: skip the oracle check")
    p.add_argument("--docs", type=int, default=8192, help="document: documents")
    p.add_argument("--doc-entries", type=int, default=64, help="document: entries per tx")
    p.add_argument("--v1-proofs", type=int, default=None,
                   help="dualv1: header pairs (default 10^5); dualv1verify: random pairs "
                        "(default: as many as make about 1 GiB of messages)")
    p.add_argument("--v1-depth", type=int, default=20, help="dualv1: log2 of the appends")
    p.add_argument("--repl-txs", type=int, default=4096, help="replicate: exported txs")
    p.add_argument("--repl-leaves", type=int, default=10 ** 5,
                   help="replicate: leaves of the follower's tree before the batch")
    return p


def np_nodes_until(n):
    """nodesUntil(n) = nodesUpto(n-1) (ahtree.go:485-511) for a uint64 array:
    n - 1 + sum_{x < n-1} popcount(x), summed bit by bit."""
    import numpy as np
    x = np.asarray(n, np.uint64) - np.uint64(1)
    s = x.copy()
    for k in range(63):
        hi = (x >> np.uint64(k + 1)) << np.uint64(k)
        lo = x & np.uint64((1 << (k + 1)) - 1)
        s += hi + np.where(lo > np.uint64(1 << k), lo - np.uint64(1 << k), np.uint64(0))
    return s


def c5_ahtree(a, m, N, L, ctx, dev, sync):
    """configs[4]'s ahtree half: 10^6 inclusion and 10^6 consistency proofs
    against a 2^24-append tree (j = 2^24, random i), generated on the device
    from the resident dLog, 10 % tampered (one bit of the first term), then
    re-hashed by ahtree.VerifyInclusion / VerifyConsistency
    (ahtree/verification.go:21-109); the bitmaps must be exact."""
    import numpy as np
    import torch
    P, W = a.proofs, 1 << a.depth
    rng = np.random.default_rng(55)
    pay = torch.empty(W * 32, dtype=torch.uint8, device=dev)
    N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), 55))
    dlog = torch.empty(m.nodes_upto(W) * 32, dtype=torch.uint8, device=dev)
    N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(), W, 32,
                                         None))
    dl = dlog.view(-1, 32)
    res = {}
    for kind, name, S in ((0, "inclusion", 64), (1, "consistency", 128)):
        iv = rng.integers(1, W + 1, P).astype(np.uint64)
        jv = np.full(P, W, np.uint64)
        it = torch.from_numpy(iv.view(np.int64)).to(dev)
        jt = torch.from_numpy(jv.view(np.int64)).to(dev)
        terms = torch.empty(P * S * 32, dtype=torch.uint8, device=dev)
        nt = torch.empty(P, dtype=torch.int32, device=dev)
        st = torch.empty(P, dtype=torch.int32, device=dev)
        N.check(L.mh_dev_ahtree_proof_batch(ctx.handle, kind, dlog.data_ptr(), W, P, it.data_ptr(),
                                            jt.data_ptr(), terms.data_ptr(), S, nt.data_ptr(),
                                            st.data_ptr()))
        sync()
        assert int(st.abs().sum().item()) == 0
        # compact the fixed-stride proofs into the CSR layout of the verifier
        cnt = nt.to(torch.int64)
        off = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(cnt, 0)
        rows = torch.repeat_interleave(torch.arange(P, device=dev), cnt)
        pos = torch.arange(int(off[P].item()), device=dev) - off[:-1][rows]
        flat = terms.view(P, S, 32)[rows, pos].contiguous()
        tamper = (rng.random(P) < 0.10) & (cnt.cpu().numpy() > 0)
        tp = torch.from_numpy(np.nonzero(tamper)[0]).to(dev)
        flat[off[:-1][tp], 0] ^= 1
        # a / b: VerifyInclusion(leaf(i), root(j)), VerifyConsistency(root(i), root(j))
        pc = lambda v: np.array([bin(int(x - 1)).count("1") for x in v], np.uint64)  # noqa: E731
        root_idx = lambda v: np.asarray(np_nodes_until(v)) + pc(v)  # noqa: E731
        ai = np_nodes_until(iv) if kind == 0 else root_idx(iv)
        bi = root_idx(jv[:1]).repeat(P)
        av = dl[torch.from_numpy(ai.view(np.int64)).to(dev)].contiguous()
        bv = dl[torch.from_numpy(bi.view(np.int64)).to(dev)].contiguous()
        ok = torch.zeros(P, dtype=torch.uint8, device=dev)

        def step():
            N.check(L.mh_dev_ahtree_verify_batch(ctx.handle, kind, P, it.data_ptr(), jt.data_ptr(),
                                                 off.data_ptr(), flat.data_ptr(), av.data_ptr(),
                                                 bv.data_ptr(), ok.data_ptr(), None))

        prewarm(step, sync, a.prewarm)
        t = timed_k(ctx, step, a.steps, a.warmup, sync)
        kms = ctx.timing("ahtree_verify")[0] / (a.steps + a.warmup)
        okh = ok.cpu().numpy().astype(bool)
        res[name] = {"M_proofs_per_s": round(P / t / 1e6, 1), "ms_per_step": round(t * 1e3, 3),
                     "kernel_ms": round(kms, 3), "mean_terms": round(float(cnt.float().mean()), 2),
                     "bitmap_exact": bool((okh == ~tamper).all()),
                     "tampered": int(tamper.sum())}
    return res


def txlog_records(ntx, ne, kl, seed=14):
    """The synthetic tx log of the a14 lines (immustore.go:1812-1924 record
    layout): ntx v1 records without metadata, ne entries each (kl-byte random
    keys, vLen 100, random hVal), random blRoot / prevAlh; the stored Alh
    (last 32 bytes of each record) left zero for the caller to seal.  ->
    (ntx, record bytes) uint8 array."""
    import struct
    import numpy as np
    rng = np.random.default_rng(seed)
    ent = 2 + 2 + kl + 4 + 8 + 32
    hdr = 8 + 8 + 8 + 32 + 32 + 2 + 2 + 4
    rec = hdr + ne * ent + 32
    buf = np.zeros((ntx, rec), np.uint8)
    buf[:, 0:8] = np.arange(1, ntx + 1, dtype=">u8").view(np.uint8).reshape(ntx, 8)
    buf[:, 8:16] = np.frombuffer(struct.pack(">Q", 1666885208), np.uint8)
    buf[:, 24:88] = rng.integers(0, 256, (ntx, 64), dtype=np.uint8)  # blRoot, prevAlh
    buf[:, 89] = 1  # version 1, mdLen 0
    buf[:, 92:96] = np.frombuffer(struct.pack(">I", ne), np.uint8)
    e = buf[:, hdr:hdr + ne * ent].reshape(ntx, ne, ent)
    e[:, :, 3] = kl
    e[:, :, 4:4 + kl] = rng.integers(0, 256, (ntx, ne, kl), dtype=np.uint8)
    e[:, :, 4 + kl + 3] = 100  # vLen
    e[:, :, 4 + kl + 12:] = rng.integers(0, 256, (ntx, ne, 32), dtype=np.uint8)  # hVal
    return buf


def ragged_inputs(n, max_vlen, seed=6):
    """Host CSR arrays of the ragged workload (seeded): value length uniform
    in [0, max_vlen], key 8-64 B, KV metadata 0-11 B (embedded/store/
    options.go:37-39, kv_metadata.go:41-43)."""
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as orc
    rng = np.random.default_rng(seed)
    out = {}
    for name, lo, hi, sd in (("v", 0, max_vlen, seed), ("k", 8, 64, seed + 1), ("m", 0, 11, seed + 2)):
        ln = rng.integers(lo, hi + 1, n).astype(np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(ln, out=off[1:])
        out[name] = (orc.fill_random(int(off[-1]) + 16, sd), off)
    return out


def ragged(a, m, N, L, ctx, dev, sync):
    import numpy as np
    import torch
    n = a.entries
    R = ragged_inputs(n, a.max_vlen)
    d = {}
    for name, (buf, off) in R.items():
        d[name] = (torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int64)).to(dev))
    nl = m.levels_len(n)
    lv = torch.empty(nl * 32, dtype=torch.uint8, device=dev)
    hv = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    root = torch.empty(32, dtype=torch.uint8, device=dev)
    sync()

    def step():
        N.check(L.mh_dev_htree_build_entries(ctx.handle, 1, n, d["k"][0].data_ptr(),
                                             d["k"][1].data_ptr(), d["m"][0].data_ptr(),
                                             d["m"][1].data_ptr(), d["v"][0].data_ptr(),
                                             d["v"][1].data_ptr(), None, None, hv.data_ptr(),
                                             lv.data_ptr(), root.data_ptr()))

    prewarm(step, sync, a.prewarm)
    t = timed_k(ctx, step, a.steps, a.warmup, sync)
    runs = a.steps + a.warmup
    tm = {k: round(ctx.timing(k)[0] / runs, 4) for k in ("varlen_sort", "entries_varlen", "reduce")}
    sha_ms = tm["entries_varlen"]
    vl = np.diff(R["v"][1]).astype(np.int64)
    ml = 36 + np.diff(R["k"][1]).astype(np.int64) + np.diff(R["m"][1]).astype(np.int64)
    comp_val = int(((vl + 72) // 64).sum())
    comp_dig = int(((ml + 72) // 64).sum())
    comp_tree = n + 2 * (n - 1)
    sha_rate = (comp_val + comp_dig + n) / (sha_ms * 1e-3) / 1e9
    SHA_PEAK = 30.9  # profiles/microbench_r01.txt
    res = {"metric": "ragged htree build (value hashes + entry digests + all levels), device "
                     "resident", "entries": n,
           "value": round(float(vl.sum()) / t / 2 ** 30, 2), "unit": "GiB/s of values",
           "M_entries_per_s": round(n / t / 1e6, 2), "ms_per_step": round(t * 1e3, 3),
           "kernel_ms": tm,
           "compressions": {"values": comp_val, "digests": comp_dig, "tree": comp_tree},
           "sha": {"kernel": "k_entries_varlen (value blocks + digest blocks + leaf)",
                   "gcomp_per_s": round(sha_rate, 2), "peak_gcomp_per_s": SHA_PEAK,
                   "frac": round(sha_rate / SHA_PEAK, 4)},
           "step_gcomp_per_s": round((comp_val + comp_dig + comp_tree) / t / 1e9, 2),
           "sorted": True}
    if not a.no_check:
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        import oracle as orc
        st, ohv, _, oroot = orc.build_entries_csr(1, R["k"][0], R["k"][1], R["m"][0], R["m"][1],
                                                  R["v"][0], R["v"][1], want_levels=False)
        res["oracle_match"] = bool(st == 0 and root.cpu().numpy().tobytes() == oroot and
                                   np.array_equal(hv.cpu().numpy().reshape(-1, 32), ohv))
    return res


def document_batch(ndocs, width, seed=31):
    """Synthetic VerifyDocument inputs: document k is the value of entry 0 of
    its own v1 tx of `width` entries (keys doc/<k>/<e>, KV metadata on three
    entries of four), the tx's Eh / Alh sealed by the oracle (EntrySpec
    digests with the stored HValues, htree, innerHash, Alh), a trivial
    DualProofV2 (source = target = the tx) and the tx as known state."""
    import hashlib
    import struct
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as orc
    from immustore_amd.txlayer import TX_HEADER
    rng = np.random.default_rng(seed)
    mds = [b"", b"\x00", b"\x02", b"\x01" + struct.pack(">Q", 1_800_000_000)]
    ml = np.array([len(mds[e % 4]) for e in range(width)], np.uint64)
    mo = np.zeros(width + 1, np.uint64)
    np.cumsum(ml, out=mo[1:])
    mb = np.frombuffer(b"".join(mds[e % 4] for e in range(width)) + bytes(8), np.uint8)
    docs = []
    for k in range(ndocs):
        keys = [b"doc/%08d/%04d" % (k, e) for e in range(width)]
        kb = np.frombuffer(b"".join(keys) + bytes(8), np.uint8)
        ko = np.arange(width + 1, dtype=np.uint64) * len(keys[0])
        doc = rng.integers(0, 256, int(rng.integers(64, 1024)), dtype=np.uint8).tobytes()
        hv = rng.integers(0, 256, (width, 32), dtype=np.uint8)
        hv[0] = np.frombuffer(hashlib.sha256(doc).digest(), np.uint8)
        st, _, _, eh = orc.build_entries_csr(1, kb, ko, mb, mo, np.zeros(8, np.uint8),
                                             np.zeros(width + 1, np.uint64), want_levels=False,
                                             ov=hv, use=np.ones(width, np.uint8))
        assert st == 0
        h = np.zeros(1, TX_HEADER)
        h["id"], h["bl_tx_id"], h["version"], h["nentries"] = 100 + k, 99 + k, 1, width
        h["eh"] = np.frombuffer(eh, np.uint8)
        h["ts"] = 1_700_000_000 + k
        alh = orc.tx_header_alh(h[0])[2]
        ents = [(keys[e], mds[e % 4], hv[e].tobytes()) for e in range(width)]
        docs.append({"encoded_document": doc, "doc_key": keys[0], "tx_hdr": h[0], "entries": ents,
                     "src_hdr": h[0], "tgt_hdr": h[0], "incl": [], "cons": [],
                     "known_tx_id": 100 + k, "known_alh": alh})
    return docs


def document(a, ctx):
    import concurrent.futures as cf
    import numpy as np
    from immustore_amd import txlayer
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as orc
    docs = document_batch(a.docs, a.doc_entries)
    # the batch packed as the cgo shim packs it: every array in ONE pinned
    # arena (one upload of the span); beside it, one pinned allocation per array
    b, keep = txlayer.pack_document_batch(docs, pinned="arena")
    b1, keep1 = txlayer.pack_document_batch(docs, pinned=True)
    n = len(docs)
    res = {}

    def step():
        res["out"] = txlayer.call_document_batch(b, n, ctx)

    def step_per_array():
        res["out1"] = txlayer.call_document_batch(b1, n, ctx)

    t1 = timed(step_per_array, a.steps, a.warmup, lambda: None)
    t = timed(step, a.steps, a.warmup, lambda: None)
    st, alh = res["out"]
    assert np.array_equal(st, res["out1"][0]) and np.array_equal(alh, res["out1"][1])
    sample = range(0, n, max(1, n // 256))
    ok = all(int(st[k]) == 0 and alh[k].tobytes() == orc.verify_document(docs[k])[1]
             for k in sample)
    # CPU baseline: the oracle's hashing of the same documents on 16 host
    # threads -- EntrySpec digests + one htree per tx (orc_precommit_batch with
    # every HValue as the hVal override: the same digests and trees) plus
    # SHA256(document); innerHash / Alh (4 compressions per doc) left out.
    # Packed outside the timed region, as the device batch is.
    W = a.doc_entries
    kb = np.frombuffer(b"".join(e[0] for d in docs for e in d["entries"]) + bytes(8), np.uint8)
    ko = np.zeros(n * W + 1, np.uint64)
    np.cumsum([len(e[0]) for d in docs for e in d["entries"]], out=ko[1:])
    mbb = np.frombuffer(b"".join(e[1] for d in docs for e in d["entries"]) + bytes(8), np.uint8)
    mo_ = np.zeros(n * W + 1, np.uint64)
    np.cumsum([len(e[1]) for d in docs for e in d["entries"]], out=mo_[1:])
    hv = np.frombuffer(b"".join(e[2] for d in docs for e in d["entries"]), np.uint8)
    txo = np.arange(n + 1, dtype=np.uint64) * W
    dbs = np.frombuffer(b"".join(d["encoded_document"] for d in docs), np.uint8)
    dof = np.zeros(n + 1, np.uint64)
    np.cumsum([len(d["encoded_document"]) for d in docs], out=dof[1:])
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(2) as ex:
        f = ex.submit(orc.precommit_batch, 1, txo, kb, ko, np.zeros(8, np.uint8),
                      np.zeros(n * W + 1, np.uint64), mbb, mo_, hv, np.ones(n * W, np.uint8),
                      None, 0, 16)
        # SHA256(document) beside it: the documents' bytes once, one core
        orc.precommit_batch(0, np.arange(n + 1, dtype=np.uint64), np.zeros(8, np.uint8),
                            np.zeros(n + 1, np.uint64), dbs, dof, nthreads=1)
        _, ehs, sts = f.result()
    tc = time.perf_counter() - t0
    roots = [ehs[k].tobytes() for k in range(n)]
    assert all(r == bytes(docs[k]["tx_hdr"]["eh"]) for k, r in enumerate(roots))
    return {"metric": "VerifyDocument batch (hashing part), documents in host memory", "docs": n,
            "entries_per_doc": a.doc_entries, "value": round(n / t / 1e3, 1),
            "unit": "K documents/s", "ms_per_step": round(t * 1e3, 3),
            "layout": "one pinned arena (the shim's packing)",
            "per_array_pinned": {"ms_per_step": round(t1 * 1e3, 3),
                                 "value": round(n / t1 / 1e3, 1)},
            "all_valid": bool((st == 0).all()), "sample_matches_oracle": bool(ok),
            "cpu_baseline": {"kind": "port", "cores": 16, "value": round(n / tc / 1e3, 1),
                             "unit": "K documents/s",
                             "sample": "the whole batch once: oracle orc_precommit_batch over "
                                       "the docs' txs with the HValues as overrides (EntrySpec "
                                       "digests + htree, 16 threads) beside SHA256 of every "
                                       "document (1 thread)"}}


def values(a, m, N, L, ctx, dev, sync):
    """readValueAt's integrity check (immustore.go:3235) over a batch of
    a.entries ragged values (0..a.max_vlen B, seeded), 1 % corrupted: device
    resident (mh_dev_verify_values_batch), and from pinned host memory through
    the chunked copy / check pipeline (mh_verify_values_batch)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as orc
    n = a.entries
    rng = np.random.default_rng(8)
    lens = rng.integers(0, a.max_vlen + 1, n).astype(np.uint64)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    vb = torch.empty(total + 16, dtype=torch.uint8).pin_memory()
    vb.numpy()[:] = orc.fill_random(total + 16, 18)
    dv = vb.to(dev)
    do = torch.from_numpy(off.view(np.int64)).to(dev)
    dh = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    sync()
    N.check(L.mh_dev_sha256_batch(ctx.handle, dv.data_ptr(), do.data_ptr(), n, dh.data_ptr()))
    sync()
    hv = dh.cpu().numpy().reshape(n, 32).copy()
    bad = rng.choice(n, n // 100, replace=False)
    hv[bad, 0] ^= 1
    dh.copy_(torch.from_numpy(hv.reshape(-1)))
    dl = torch.from_numpy(lens.view(np.int64)).to(dev)
    ds = torch.empty(n, dtype=torch.int32, device=dev)
    sync()

    def step():
        N.check(L.mh_dev_verify_values_batch(ctx.handle, n, dv.data_ptr(), do.data_ptr(),
                                             dl.data_ptr(), dh.data_ptr(), ds.data_ptr()))

    prewarm(step, sync, a.prewarm)
    t = timed_k(ctx, step, a.steps, a.warmup, sync)
    runs = a.steps + a.warmup
    kms = ctx.timing("verify_values")[0] / runs
    sort_ms = ctx.timing("varlen_sort")[0] / runs
    st = ds.cpu().numpy()
    comp = int(((lens.astype(np.int64) + 72) // 64).sum())
    # host memory in and out (pinned values), the pipelined call
    hp = torch.from_numpy(hv.reshape(-1)).pin_memory()
    stp = torch.empty(n, dtype=torch.int32).pin_memory()
    import ctypes as C
    badc = C.c_uint64()
    offc = np.ascontiguousarray(off)
    lenc = np.ascontiguousarray(lens)

    def host_step():
        N.check(L.mh_verify_values_batch(ctx.handle, n, vb.data_ptr(), offc.ctypes.data,
                                         lenc.ctypes.data, hp.data_ptr(), stp.data_ptr(),
                                         C.byref(badc)))

    th = timed(host_step, max(1, a.steps // 2), 1, sync)
    # plain pinned H2D of the same value bytes: the PCIe bound of the host call
    tmp = torch.empty(total, dtype=torch.uint8, device=dev)
    th2d = timed(lambda: tmp.copy_(vb[:total], non_blocking=True), 3, 1, sync)
    del tmp
    ok_dev = bool(np.array_equal(np.sort(np.nonzero(st)[0]), np.sort(bad)))
    ok_host = bool(np.array_equal(stp.numpy(), st)) and badc.value == len(bad)
    # CPU baseline: the oracle on 16 threads over the first 2^18 values
    ns = min(n, 1 << 18)
    t0 = time.perf_counter()
    oc, ost = orc.verify_values(vb.numpy(), off[:ns + 1], hv[:ns], lens[:ns], nthreads=16)
    tc = time.perf_counter() - t0
    ok_orc = bool(np.array_equal(ost, st[:ns]))
    SHA_PEAK = 30.9
    return {"metric": "readValueAt integrity check (immustore.go:3235) over a batch of ragged "
                      "values, device resident", "entries": n, "value_bytes": total,
            "value": round(total / t / 2 ** 30, 2), "unit": "GiB/s of values",
            "M_values_per_s": round(n / t / 1e6, 2), "ms_per_step": round(t * 1e3, 3),
            "kernel_ms": {"verify_values": round(kms, 4), "varlen_sort": round(sort_ms, 4)},
            "sha": {"kernel": "k_sha_varlen (compare fused)",
                    "gcomp_per_s": round(comp / (kms * 1e-3) / 1e9, 2),
                    "frac": round(comp / (kms * 1e-3) / 1e9 / SHA_PEAK, 4)},
            "roofline": {"bound": "hbm", "achieved": round((total + 52 * n) / (kms * 1e-3) / 1e9, 1),
                         "peak": 8000.0, "unit": "GB/s",
                         "frac": round((total + 52 * n) / (kms * 1e-3) / 1e9 / 8000.0, 4)},
            "host_pinned": {"ms": round(th * 1e3, 3), "gib_per_s": round(total / th / 2 ** 30, 2),
                            "h2d_only_ms": round(th2d * 1e3, 3),
                            "note": "mh_verify_values_batch from pinned host memory (64 MiB "
                                    "chunks, copy stream + compute stream) vs a plain pinned "
                                    "H2D of the same bytes"},
            "corrupted": len(bad), "statuses_match": ok_dev and ok_host and ok_orc,
            "cpu_baseline": {"kind": "port", "cores": 16, "unit": "GiB/s of values",
                             "value": round(int(off[ns]) / tc / 2 ** 30, 2),
                             "sample": "oracle orc_verify_values over the first %d values, 16 "
                                       "threads, SHA-NI=%s" % (ns, orc.has_shani())}}


def c3range(a, m, N, L, ctx, dev, sync):
    """syncBinaryLinking's replay (immustore.go:1198-1232) on one device:
    a.m appends onto a tree of n0 = 10^6 + 3, (1) with the whole old dLog
    resident (mh_dev_ahtree_append_batch) and (2) with only the old tree's
    peaks on the device and the new digests in a buffer of their own
    (mh_dev_ahtree_append_range, the form each device of the multi-GPU append
    runs).  Both new dLog slices and last roots are compared."""
    import numpy as np
    import torch
    from immustore_amd.multi import peaks_of
    M, n0 = a.m, 10 ** 6 + 3
    up = L.mh_ahtree_nodes_upto
    pay = torch.empty((n0 + M) * 32, dtype=torch.uint8, device=dev)
    N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), 3))
    full = torch.empty(up(n0 + M) * 32, dtype=torch.uint8, device=dev)
    # the old tree (n0 appends), its peaks read back from the device dLog
    N.check(L.mh_dev_ahtree_append_batch(ctx.handle, full.data_ptr(), 0, pay.data_ptr(), n0, 32, None))
    sync()
    pk = np.zeros(32 * bin(n0).count("1"), np.uint8)
    N.check(L.mh_dev_ahtree_peaks(ctx.handle, full.data_ptr(), n0, pk.ctypes.data))
    rng_buf = torch.empty((up(n0 + M) - up(n0)) * 32, dtype=torch.uint8, device=dev)
    ro_a = torch.empty(M * 32, dtype=torch.uint8, device=dev)
    ro_b = torch.empty(M * 32, dtype=torch.uint8, device=dev)
    newp = pay[n0 * 32:]

    def step_full():
        N.check(L.mh_dev_ahtree_append_batch(ctx.handle, full.data_ptr(), n0, newp.data_ptr(), M,
                                             32, ro_a.data_ptr()))

    def step_range():
        N.check(L.mh_dev_ahtree_append_range(ctx.handle, rng_buf.data_ptr(), n0, pk.ctypes.data,
                                             newp.data_ptr(), M, 32, ro_b.data_ptr()))

    prewarm(step_full, sync, a.prewarm)
    res = {}
    for name, st in (("full_dlog", step_full), ("range", step_range), ("full_dlog_2", step_full),
                     ("range_2", step_range)):
        t = timed(st, a.steps, a.warmup, sync)
        res[name] = round(t * 1e3, 3)
    same = bool(torch.equal(full[up(n0) * 32:], rng_buf) and torch.equal(ro_a, ro_b))
    t = min(res["range"], res["range_2"]) * 1e-3
    return {"metric": "ahtree replay append onto a tree of 10^6+3: 10^7 x 32 B payloads, one "
                      "device, only the old peaks resident (mh_dev_ahtree_append_range)",
            "value": round(M / t / 1e6, 1), "unit": "M appends/s", "ms": res,
            "device_bytes": {"range": int(rng_buf.numel()), "full_dlog": int(full.numel())},
            "identical_to_full_dlog_append": same}


def replicate(a, m, N, L, ctx, sync):
    """The follower's catch-up: --repl-txs consecutive exported txs (v1,
    --tx-entries entries of 8-byte keys and --vlen-byte values, pinned) onto a
    tree of --repl-leaves leaves through mh_replicate_tx_batch, next to today's
    path over the same txs already repacked into CSR arrays (no host parse):
    mh_precommit_batch + mh_tx_alh_batch + mh_ahtree_append_batch."""
    import ctypes as C
    import struct
    import numpy as np
    import torch
    from immustore_amd.replicate import _Batch, REPLICATED_ENTRY
    from immustore_amd.txlayer import TX_HEADER
    orc = _oracle()
    orc.use_shani(True)
    ntx, per, vlen, P = a.repl_txs, a.tx_entries, a.vlen, a.repl_leaves
    n = ntx * per
    pin = lambda nbytes: torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory().numpy()  # noqa: E731
    rng = np.random.default_rng(24)
    # the follower's tree: P random Alh values, on the device and in the oracle
    old = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    ot = orc.AHtree(P + ntx)
    if P:
        ot.append_batch(old)
    prev = old[-1].tobytes() if P else orc.sha256(b"")
    # the primary's txs: hVal, Eh (oracle, 16 threads), then the chain
    vals = pin(n * vlen)
    vals[:] = rng.integers(0, 256, n * vlen, dtype=np.uint8)
    keys = pin(n * 8)
    keys[:] = np.frombuffer(np.arange(n, dtype=">u8").tobytes(), np.uint8)
    pin_u64 = lambda x: pin(x.nbytes).view(np.uint64)  # noqa: E731
    csr = dict(tx_off=np.arange(0, n + 1, per, dtype=np.uint64), keys=keys,
               key_off=np.arange(0, 8 * n + 1, 8, dtype=np.uint64), vals=vals,
               val_off=np.arange(0, vlen * n + 1, vlen, dtype=np.uint64))
    for k in ("tx_off", "key_off", "val_off"):
        q = pin_u64(csr[k])
        q[:] = csr[k]
        csr[k] = q
    _, eh, st = orc.precommit_batch(1, nthreads=16, **csr)
    assert not st.any()
    hdrs = pin(ntx * TX_HEADER.itemsize).view(TX_HEADER)
    hdrs[:] = np.zeros(ntx, TX_HEADER)
    alhs = np.zeros((ntx, 32), np.uint8)
    blobs, cur = [], prev
    for k in range(ntx):
        txid = P + k + 1
        bl = txid - 1
        bl_root = ot.root_at(bl)[1] if bl else bytes(32)
        ts = 1700000000 + k
        s_, inner = orc.tx_inner_hash(ts, 1, b"", per, eh[k].tobytes(), bl, bl_root)
        alh = orc.tx_alh(txid, cur, inner)
        h = hdrs[k]
        h["id"], h["ts"], h["bl_tx_id"], h["version"], h["nentries"] = txid, ts, bl, 1, per
        h["bl_root"] = np.frombuffer(bl_root, np.uint8)
        h["prev_alh"] = np.frombuffer(cur, np.uint8)
        h["eh"] = eh[k]
        hb = struct.pack(">Q", txid) + cur + struct.pack(">qHHI", ts, 1, 0, per) + eh[k].tobytes() + \
            struct.pack(">Q", bl) + bl_root
        ents = b"".join(struct.pack(">H", 8) + keys[8 * e:8 * e + 8].tobytes() + struct.pack(">HI", 0, vlen)
                        + vals[vlen * e:vlen * (e + 1)].tobytes() for e in range(k * per, (k + 1) * per))
        blobs.append(struct.pack(">I", len(hb)) + hb + ents + b"\x00\x01\x00")
        ot.append(alh)
        alhs[k] = np.frombuffer(alh, np.uint8)
        cur = alh
    flat = b"".join(blobs)
    txs = pin(len(flat))
    txs[:] = np.frombuffer(flat, np.uint8)
    off = pin_u64(np.zeros(ntx + 1, np.uint64))
    off[0] = 0
    off[1:] = np.cumsum([len(x) for x in blobs], dtype=np.uint64)
    root_want = ot.root_at(P + ntx)[1]

    t = m.AHtree(ctx)
    if P:
        t.append_batch(old)
    # ---- the new call, every output pinned
    b = _Batch()
    b.n, b.txs, b.tx_off = ntx, txs.ctypes.data, off.ctypes.data
    b.max_entries, b.max_key_len, b.max_value_len, b.flags = 1024, 1024, 1 << 25, 0
    b.prev_alh[:] = list(prev)
    o_st = pin(ntx * 4).view(np.int32)
    o_hd = pin(ntx * TX_HEADER.itemsize)
    o_md = pin(ntx * 268)
    o_alh = pin(ntx * 32)
    o_eo = pin_u64(np.zeros(ntx + 1, np.uint64))
    o_en = pin(n * REPLICATED_ENTRY.itemsize)
    o_hv = pin(n * 32)
    acc = C.c_uint64(0)

    def step_new():
        N.check(L.mh_ahtree_reset_size(t.handle, P))
        N.check(L.mh_replicate_tx_batch(t.handle, C.addressof(b), o_st.ctypes.data, C.byref(acc),
                                        o_hd.ctypes.data, o_md.ctypes.data, o_alh.ctypes.data,
                                        o_eo.ctypes.data, o_en.ctypes.data, n, o_hv.ctypes.data))
        assert acc.value == ntx

    # ---- today's path: three calls with a host round trip between each
    pipe = m.CommitPipe(ctx)
    hv = pin(n * 32).reshape(n, 32)
    eh_o = pin(ntx * 32).reshape(ntx, 32)
    inner_o = pin(ntx * 32)
    alh_o = pin(ntx * 32)
    md1 = np.zeros(1, np.uint8)

    def step_old():
        N.check(L.mh_ahtree_reset_size(t.handle, P))
        _, _, st_ = pipe.precommit_csr(1, expect_eh=eh, hvals_out=hv, eh_out=eh_o, **csr)
        assert not st_.any()
        N.check(L.mh_tx_alh_batch(ctx.handle, ntx, hdrs.ctypes.data, md1.ctypes.data, 0,
                                  inner_o.ctypes.data, alh_o.ctypes.data))
        N.check(L.mh_ahtree_append_batch(t.handle, alh_o.ctypes.data, ntx, 32, None))

    prewarm(step_new, sync, a.prewarm)
    t_old1 = timed(step_old, a.steps, a.warmup, sync)
    t_new = timed_k(ctx, step_new, a.steps, a.warmup, sync)
    names = ("repl_struct_size", "repl_struct_write", "repl_set", "repl_leaf", "leaf_for", "repl_alh",
             "repl_verdict", "aht")
    kd = {k: round(ctx.timing(k)[0] / (a.steps + a.warmup), 3) for k in names}
    n_new, root_new = t.root()
    ok_new = bool(n_new == P + ntx and root_new == root_want and not o_st.any()
                  and o_alh.tobytes() == alhs.tobytes())
    t_old2 = timed(step_old, a.steps, a.warmup, sync)
    n_old, root_old = t.root()
    ok_old = bool(n_old == P + ntx and root_old == root_want)
    t_old = min(t_old1, t_old2)
    pipe.close()
    t.close()
    gib = len(flat) / 2 ** 30
    return {"metric": "ReplicateTx of a run of exported txs in one call: parse, hash, verdicts, append",
            "value": round(ntx / t_new), "unit": "txs/s", "ms_per_step": round(t_new * 1e3, 3),
            "gib_per_s": round(gib / t_new, 3),
            "three_calls": {"ms": round(t_old * 1e3, 3), "ms_before": round(t_old1 * 1e3, 3),
                            "ms_after": round(t_old2 * 1e3, 3),
                            "note": "mh_precommit_batch + mh_tx_alh_batch + mh_ahtree_append_batch over "
                                    "the same txs already repacked (pinned CSR arrays): no host parse, "
                                    "no BlRoot / PrevAlh / id checks"},
            "three_calls_over_new": round(t_old / t_new, 3),
            "kernel_ms": kd,
            "config": {"txs": ntx, "entries_per_tx": per, "key_len": 8, "value_len": vlen,
                       "version": 1, "tree_leaves": P, "blob_bytes": len(flat), "pinned": True},
            "root_check": {"ok": ok_new and ok_old, "new_call": ok_new, "three_calls": ok_old,
                           "root": root_want.hex(),
                           "against": "oracle AHtree over the same Alh values; the call's statuses "
                                      "and Alh values"}}


def run_single(a):
    """One GPU: run workload a.workload, return its result dict."""
    import numpy as np
    import torch
    import immustore_amd as m
    from immustore_amd import _native as N

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    ctx = m.Context(0, stream.cuda_stream)
    L = N.load()
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    out = {}

    if a.workload == "c3":
        M = a.m
        pay = torch.empty(M * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), 3))
        nd = m.nodes_upto(M)
        dlog = torch.empty(nd * 32, dtype=torch.uint8, device=dev)
        if a.logs:
            plog = torch.empty(M * 36, dtype=torch.uint8, device=dev)
            clog = torch.empty(M * 12, dtype=torch.uint8, device=dev)

        def step():
            if a.logs:
                N.check(L.mh_dev_ahtree_append_batch_logs(
                    ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(), M, 32, 0, plog.data_ptr(),
                    clog.data_ptr(), None))
            else:
                N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0,
                                                     pay.data_ptr(), M, 32, None))

        prewarm(step, sync, a.prewarm)
        t = timed_k(ctx, step, a.steps, a.warmup, sync)
        kt = {k: ctx.timing(k)[0] / (a.steps + a.warmup) for k in ("aht_leaves", "aht_perfect",
                                                                   "aht_spine")}
        comps = M + 2 * (nd - M)
        # ---- check vs the oracle, after the timed region (as the multi-rank
        # line): the batch once more with its RootAt values kept, then every
        # dLog digest and RootAt of 64 first, 64 last and 256 random appends
        # against the oracle's streamed append of the same payload stream
        # (orc.ahtree_stream, ahtree.go:287-322)
        tc = time.perf_counter()
        rts = torch.empty(M * 32, dtype=torch.uint8, device=dev)
        if a.logs:
            N.check(L.mh_dev_ahtree_append_batch_logs(ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(),
                                                      M, 32, 0, plog.data_ptr(), clog.data_ptr(),
                                                      rts.data_ptr()))
        else:
            N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(), M,
                                                 32, rts.data_ptr()))
        sync()
        orc = _oracle()
        samples = aht_samples(0, M, np.random.default_rng(7))
        dl, rr = dlog.view(-1, 32), rts.view(-1, 32)
        rows = lambda t_, i: t_[torch.from_numpy(i).to(dev)].cpu().numpy()  # noqa: E731
        ok, root_o = c3_rank_check(orc, 3, 32, 0, M, lambda i: rows(dl, i), lambda i: rows(rr, i),
                                   samples, host_threads())
        pay_h = pay.view(-1, 32)
        out = {"metric": "ahtree batch append, 10^7 x 32 B payloads (configs[2])",
               "value": round(M / t / 1e6, 3), "unit": "M appends/s",
               "ms_per_step": round(t * 1e3, 3), "dlog_digests": nd,
               "dlog_GBps": round(nd * 32 / t / 1e9, 2),
               "gcomp_per_s": round(comps / t / 1e9, 2),
               "kernel_ms": {k: round(v, 3) for k, v in kt.items()},
               "root_check": {"vs": "oracle", "ok": bool(ok), "root": root_o.hex(),
                              "samples": int(len(samples)),
                              "seconds": round(time.perf_counter() - tc, 2),
                              "what": "every dLog digest and RootAt of 64 first, 64 last and "
                                      "256 random appends vs the oracle's streamed append of "
                                      "the same payload stream (orc.ahtree_stream)"}}
        if a.logs:
            # records of the first / last appends vs the format (ahtree.go:266-282, 341-351)
            import struct
            pl = plog.view(-1, 36)
            cl = clog.view(-1, 12)
            for n in (0, 1, M - 1):
                ok &= bytes(pl[n].cpu().numpy()) == struct.pack(">I", 32) + bytes(
                    pay_h[n].cpu().numpy())
                ok &= bytes(cl[n].cpu().numpy()) == struct.pack(">QI", 36 * n, 32)
            out["metric"] += " + pLog/cLog appendable records"
            out["records_bytes"] = M * 48
            out["root_check"]["ok"] = bool(ok)
            out["root_check"]["what"] += "; pLog / cLog records of appends 1, 2, M vs the format"

    elif a.workload == "c5":
        D = a.depth
        W = 1 << D
        P = a.proofs
        dig = torch.empty(W * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, dig.data_ptr(), dig.numel(), 5))
        nl = m.levels_len(W)
        levels = torch.empty(nl * 32, dtype=torch.uint8, device=dev)
        root = torch.empty(32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_htree_build_digests(ctx.handle, dig.data_ptr(), W, levels.data_ptr(),
                                             root.data_ptr()))
        sync()
        rng = np.random.default_rng(5)
        leaf = rng.integers(0, W, P, dtype=np.int64)
        leaf_t = torch.from_numpy(leaf.astype(np.uint64).view(np.int64)).to(dev)
        # the proofs themselves, generated on the device from the resident
        # levels (htree.go:121-164 as a gather); width
        # 2^D: exactly D terms each, so the fixed stride is the CSR layout
        terms = torch.empty(P * D * 32, dtype=torch.uint8, device=dev)
        nterms = torch.empty(P, dtype=torch.int32, device=dev)
        pst = torch.empty(P, dtype=torch.int32, device=dev)

        def gen():
            N.check(L.mh_dev_htree_inclusion_proof_batch(
                ctx.handle, levels.data_ptr(), W, P, leaf_t.data_ptr(), terms.data_ptr(), D,
                nterms.data_ptr(), pst.data_ptr()))

        prewarm(gen, sync, a.prewarm)
        tgen = timed_k(ctx, gen, a.steps, a.warmup, sync)
        assert int(pst.abs().sum().item()) == 0 and int((nterms != D).sum().item()) == 0
        gen_ms = ctx.timing("htree_proof")[0] / (a.steps + a.warmup)
        # 10 % tampered as SURVEY 8(d) states it: one bit of one term flipped
        tamper = rng.random(P) < 0.10
        tp = np.nonzero(tamper)[0]
        tbyte = tp * (D * 32) + rng.integers(0, D * 32, len(tp))
        tbit = (1 << rng.integers(0, 8, len(tp))).astype(np.uint8)
        tv = terms.view(-1)
        ti = torch.from_numpy(tbyte).to(dev)
        tv[ti] ^= torch.from_numpy(tbit).to(dev)
        digests = dig.view(-1, 32)[leaf_t].contiguous()
        roots = root.view(1, 32).expand(P, 32).contiguous()
        width_t = torch.full((P,), W, dtype=torch.int64, device=dev)
        toff = torch.arange(0, (P + 1) * D, D, dtype=torch.int64, device=dev)
        ok = torch.zeros(P, dtype=torch.uint8, device=dev)

        def step():
            N.check(L.mh_dev_htree_verify_inclusion_batch(
                ctx.handle, P, leaf_t.data_ptr(), width_t.data_ptr(), toff.data_ptr(),
                terms.data_ptr(), digests.data_ptr(), roots.data_ptr(), ok.data_ptr()))

        prewarm(step, sync, a.prewarm)
        t = timed_k(ctx, step, a.steps, a.warmup, sync)
        kms = ctx.timing("htree_verify")[0] / (a.steps + a.warmup)
        nok = int(ok.sum().item())
        exp = int((~tamper).sum())
        comps = P * (1 + 2 * D)
        # ---- check vs the oracle, after the timed region (as the multi-rank line)
        tc = time.perf_counter()
        orc = _oracle()
        okh = ok.cpu().numpy()
        srng = np.random.default_rng(11)
        sample = np.unique(np.concatenate([np.arange(min(P, 1 << 13)), srng.integers(0, P, 1 << 13),
                                           tp[:256]]))
        st_ = torch.from_numpy(sample).to(dev)
        rk_ok, ns = c5_rank_check(orc, leaf, W, terms.view(P, D, 32)[st_].cpu().numpy(),
                                  digests[st_].cpu().numpy(), root.cpu().numpy().tobytes(), okh,
                                  tamper, sample)
        out = {"metric": "htree inclusion-proof re-hash, 10^6 proofs x depth 24 (configs[4])",
               "value": round(P / t / 1e6, 3), "unit": "M proofs/s",
               "ms_per_step": round(t * 1e3, 3), "kernel_ms": round(kms, 3),
               "gcomp_per_s": round(comps / (kms * 1e-3) / 1e9, 2),
               # a node's second block has a precomputed schedule (K+W table in
               # LDS: 901 VALU instructions vs 1388 for a full compression,
               # profiles/isa_counts_r01.txt), so this rate may exceed the
               # full-compression ceiling; the full-compression equivalent:
               "full_comp_equiv_gcomp_per_s": round(
                   P * (1355 + D * (1388 + 901)) / 1388 / (kms * 1e-3) / 1e9, 2),
               "proof_bytes_GBps": round(P * (D * 32 + 32 + 32 + 24) / (kms * 1e-3) / 1e9, 1),
               "proof_generation": {"M_proofs_per_s": round(P / tgen / 1e6, 1),
                                    "kernel_ms": round(gen_ms, 3),
                                    "terms_GBps": round(P * D * 32 / (gen_ms * 1e-3) / 1e9, 1)},
               "verified": nok, "expected_verified": exp, "bitmap_exact": nok == exp and bool(
                   (okh.astype(bool) == ~tamper).all()),
               "root_check": {"vs": "oracle", "ok": bool(rk_ok), "sampled": ns,
                              "seconds": round(time.perf_counter() - tc, 2),
                              "what": "every verdict equals the expected bitmap (10 % of the "
                                      "proofs with one bit of one term flipped: false, the rest "
                                      "true), and the oracle's VerifyInclusion (htree.go:166-195) "
                                      "over the same terms / digests / root of >= 2^13 proofs "
                                      "gives the device's verdicts"}}
        if not a.no_ahtree:
            out["ahtree"] = c5_ahtree(a, m, N, L, ctx, dev, sync)

    elif a.workload == "txlog":
        ntx, ne, kl = a.txs, a.tx_entries, 16
        buf = txlog_records(ntx, ne, kl)
        rec = buf.shape[1]
        hdr = rec - ne * (2 + 2 + kl + 4 + 8 + 32) - 32
        raw = buf.reshape(-1)
        # seal: the stored Alh of every record is the one the read path recomputes
        rc, n, used, _, alh, _ = m.txlog_validate(raw, ctx=ctx)
        assert rc == 0 and n == ntx
        buf[:, rec - 32:] = alh
        raw_pageable = buf.reshape(-1).copy()
        # the log as the cgo shim would hold it: read into a pinned arena
        # (mh_host_alloc_pinned), so the record bytes go over PCIe as DMA
        pin = torch.empty(raw_pageable.size, dtype=torch.uint8).pin_memory()
        raw = pin.numpy()
        raw[:] = raw_pageable

        def step_pageable():
            r = m.txlog_validate(raw_pageable, ctx=ctx)
            assert r[0] == 0 and r[1] == ntx

        # outputs kept across calls in pinned memory, as the cgo shim keeps
        # its arena (fresh pageable outputs cost page faults on every call)
        from immustore_amd.txlayer import TX_HEADER
        outs = (torch.empty(ntx * TX_HEADER.itemsize, dtype=torch.uint8).pin_memory().numpy()
                .view(TX_HEADER),
                torch.empty(ntx * 32, dtype=torch.uint8).pin_memory().numpy().reshape(ntx, 32),
                torch.empty(ntx, dtype=torch.int32).pin_memory().numpy())

        def step():
            r = m.txlog_validate(raw, ctx=ctx, out=outs)
            assert r[0] == 0 and r[1] == ntx

        t_pageable = timed(step_pageable, a.steps, a.warmup, sync)

        def step_pageable_po():  # the pageable log, results into the pinned arena
            r = m.txlog_validate(raw_pageable, ctx=ctx, out=outs)
            assert r[0] == 0 and r[1] == ntx

        t_pageable_po = timed(step_pageable_po, a.steps, a.warmup, sync)
        prewarm(step, sync, a.prewarm)
        # (the call's ~25 launches would carry ~0.15 ms of timing events)
        t = timed_k(ctx, step, a.steps, a.warmup, sync)
        names = ("txlog_lanes", "txlog_wave", "tx_hdr_from_raw", "txe_index", "txe_leaf",
                 "small_roots", "seg_level", "tx_alh")
        kt = {k: ctx.timing(k)[0] / (a.steps + a.warmup) for k in names}
        # breakdown: the host hop alone (mh_txlog_scan, no headers out) and a
        # plain pinned H2D of the log
        import ctypes
        from immustore_amd import _native as Nn
        lib = Nn.load()
        cnt, used = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def hop_only():
            rc = lib.mh_txlog_scan(ctypes.c_void_p(raw.ctypes.data), raw.size, 1024, 1024, ntx,
                                   ctypes.byref(cnt), ctypes.byref(used), None, None)
            assert rc == 0 and cnt.value == ntx

        t_hop = timed(hop_only, a.steps, a.warmup, lambda: None)
        dlog = torch.empty(raw.size, dtype=torch.uint8, device=dev)

        def h2d():
            dlog.copy_(pin, non_blocking=True)

        t_h2d = timed(h2d, a.steps, a.warmup, sync)
        del dlog
        # device-resident log (the scrub / re-validate caller: the log is in
        # HBM already, mh_txlog_validate_resident): one group, so each call is
        # the host hop + ONE launch over the whole log -- the kernel's own
        # time, per a14 kernel
        dres = torch.zeros(raw.size + 256, dtype=torch.uint8, device=dev)
        dres[:raw.size].copy_(pin)
        sync()
        resident = {}
        kvar = os.environ.get("MH_TXLOG_KERNEL")
        # per kernel: results into device arrays (copied back after the launch:
        # kernel_ms is the kernel's own time) and into the caller's pinned
        # arrays (the kernel stores 172 B per record over PCIe itself)
        for kern, tname, o in (("lanes", "txlog_lanes", None), ("wave", "txlog_wave", None),
                               ("lanes", "txlog_lanes", outs), ("wave", "txlog_wave", outs)):
            os.environ["MH_TXLOG_KERNEL"] = kern

            def step_res():
                r = m.txlog_validate(raw, ctx=ctx, out=o, dev=dres.data_ptr())
                assert r[0] == 0 and r[1] == ntx and not r[5].any()

            prewarm(step_res, sync, a.prewarm)
            tr = timed_k(ctx, step_res, a.steps, a.warmup, sync)
            kms = ctx.timing(tname)[0] / (a.steps + a.warmup)
            resident[kern + ("" if o is None else "_pinned_outputs")] = {
                "ms_per_call": round(tr * 1e3, 3), "kernel_ms": round(kms, 4),
                "gcomp_per_s": round(ntx * (ne * 2 + 2 * (ne - 1) + 4) / (kms * 1e-3) / 1e9, 2),
                "sha_frac": round(ntx * (ne * 2 + 2 * (ne - 1) + 4) / (kms * 1e-3) / 1e9 / 30.9, 4)}
        if kvar is None:
            os.environ.pop("MH_TXLOG_KERNEL", None)
        else:
            os.environ["MH_TXLOG_KERNEL"] = kvar
        # the same resident log indexed by its commit log (mh_txlog_validate_clog:
        # no host copy, no host hop -- the structure pass, the lane kernel and
        # a status summary on the device; results into device arrays)
        from immustore_amd.txlayer import txlog_validate_clog
        import struct as _st
        clog = b"".join(_st.pack(">QI", k * rec, rec) for k in range(ntx))
        dcl = torch.frombuffer(bytearray(clog), dtype=torch.uint8).to(dev)
        d_alh = torch.empty(ntx * 32, dtype=torch.uint8, device=dev)
        d_sts = torch.empty(ntx, dtype=torch.int32, device=dev)
        d_out = (None, d_alh.data_ptr(), d_sts.data_ptr())

        def step_clog():
            r = txlog_validate_clog(dres.data_ptr(), raw.size, None, ntx=ntx, clog_dev=dcl.data_ptr(),
                                    ctx=ctx, out=d_out)
            assert r[0] == 0 and r[1] == 0 and r[2] == ntx

        prewarm(step_clog, sync, a.prewarm)
        tcl = timed_k(ctx, step_clog, a.steps, a.warmup, sync)
        k_struct = ctx.timing("txlog_struct")[0] / (a.steps + a.warmup)
        k_lanes = ctx.timing("txlog_lanes")[0] / (a.steps + a.warmup)
        got_alh = d_alh.view(ntx, 32).cpu().numpy()
        samp = np.unique(np.random.default_rng(3).integers(0, ntx, 256))
        orc = _oracle()  # (after the timed region: the checker, not the measured path)
        o_alh, o_sts = orc.txlog_validate_clog(raw_pageable, b"".join(clog[12 * k:12 * k + 12] for k in samp))
        clog_ok = bool(np.array_equal(got_alh, alh) and np.array_equal(got_alh[samp], o_alh)
                       and not o_sts.any() and not d_sts.cpu().numpy().any())
        dbad = dres.clone()
        dbad[(ntx // 2) * rec + hdr + 4 + kl + 12] ^= 1  # one hVal of the middle record
        rb = txlog_validate_clog(dbad.data_ptr(), raw.size, clog, ctx=ctx)
        clog_bad_ok = bool(rb[1] == 1 and rb[2] == ntx // 2 and rb[5][ntx // 2] == 14)
        del dbad
        resident["clog"] = {"ms_per_call": round(tcl * 1e3, 3),
                            "kernel_ms": {"txlog_struct": round(k_struct, 4),
                                          "txlog_lanes": round(k_lanes, 4)},
                            "root_check": {"vs": "oracle (256 sampled records) + the sealed Alh",
                                           "ok": bool(clog_ok and clog_bad_ok)}}
        if not (clog_ok and clog_bad_ok):
            print(json.dumps({"clog_check_failed": True}), file=sys.stderr)
            sys.exit(1)
        # the log in host memory (the pinned arena of the headline call, and a
        # pageable copy) indexed by its cLog: copied up in chunks, each chunk's
        # records checked as it lands -- the headline's PCIe-inclusive work
        # without the host hop; results into the pinned arena
        for key, src in (("clog_host_pinned", raw), ("clog_host_pageable", raw_pageable)):
            def step_hcl(src=src):
                r = txlog_validate_clog(src, src.size, None, ntx=ntx, clog_dev=dcl.data_ptr(), ctx=ctx,
                                        out=outs)
                assert r[0] == 0 and r[1] == 0 and r[2] == ntx

            prewarm(step_hcl, sync, a.prewarm)
            th = timed_k(ctx, step_hcl, a.steps, a.warmup, sync)
            ok = bool(np.array_equal(outs[1], alh) and not outs[2].any()
                      and np.array_equal(outs[1][samp], o_alh))
            resident[key] = {"ms_per_call": round(th * 1e3, 3),
                             "M_tx_per_s": round(ntx / th / 1e6, 3),
                             "root_check": {"vs": "oracle (256 sampled records) + the sealed Alh",
                                            "ok": ok}}
            if not ok:
                print(json.dumps({key + "_check_failed": True}), file=sys.stderr)
                sys.exit(1)
        del dres
        _, _, _, _, _, sts = m.txlog_validate(raw, ctx=ctx)
        bad = raw_pageable.copy()
        bad[(ntx // 2) * rec + hdr + 4 + kl + 12] ^= 1  # one hVal of the middle record
        sts_bad = m.txlog_validate(bad, ctx=ctx)[5]
        comps = ntx * (ne * 2 + 2 * (ne - 1) + 2 + 2)
        out = {"metric": "tx-log read-path validation (a14), %d records x %d entries" % (ntx, ne),
               "value": round(ntx / t / 1e6, 3), "unit": "M tx/s",
               "entries_per_s_M": round(ntx * ne / t / 1e6, 2),
               "ms_per_step": round(t * 1e3, 3), "log_bytes": int(raw.size),
               "log_GBps_incl_parse_and_h2d": round(raw.size / t / 1e9, 2),
               "pageable_input": {"ms_per_step": round(t_pageable * 1e3, 3),
                                  "M_tx_per_s": round(ntx / t_pageable / 1e6, 3),
                                  "outputs": "fresh pageable arrays per call",
                                  "pinned_outputs_ms_per_step": round(t_pageable_po * 1e3, 3)},
               "kernel_ms": {k: round(v, 3) for k, v in kt.items()},
               "host_hop_only_ms": round(t_hop * 1e3, 3), "h2d_only_ms": round(t_h2d * 1e3, 3),
               "gcomp_per_s_kernels": round(comps / max(sum(kt.values()) * 1e-3, 1e-12) / 1e9, 2),
               "resident_log": dict(resident, note="mh_txlog_validate_resident: the log already "
                                    "in HBM, one launch over all records after the host hop; "
                                    "kernel_ms = that launch (HIP events; *_pinned_outputs: the "
                                    "kernel also stores the results into pinned host arrays "
                                    "over PCIe), sha_frac vs the "
                                    "30.9 G comp/s ceiling at %d compressions per record"
                                    % (ne * 2 + 2 * (ne - 1) + 4)),
               "all_valid": bool((sts == 0).all()),
               "tamper_detected_exactly": bool(list(np.nonzero(sts_bad)[0]) == [ntx // 2])}

    elif a.workload == "commit":
        ntx, per, vlen = a.txs, a.tx_entries, a.vlen
        n = ntx * per
        vals = torch.empty(n * vlen, dtype=torch.uint8).pin_memory()
        g = torch.Generator().manual_seed(2)
        for k in range(0, n * vlen, 1 << 28):  # chunked: bounded host temporaries
            e = min(n * vlen, k + (1 << 28))
            vals[k:e].copy_(torch.randint(0, 256, (e - k,), dtype=torch.uint8, generator=g))
        keys = torch.from_numpy(np.frombuffer(np.arange(n, dtype=">u8").tobytes(), np.uint8)
                                .copy()).pin_memory()
        pin_u64 = lambda x: torch.from_numpy(x.view(np.int64)).pin_memory().numpy().view(np.uint64)  # noqa: E731
        b = dict(tx_off=pin_u64(np.arange(0, n + 1, per, dtype=np.uint64)), keys=keys.numpy(),
                 key_off=pin_u64(np.arange(0, 8 * n + 1, 8, dtype=np.uint64)), vals=vals.numpy(),
                 val_off=pin_u64(np.arange(0, vlen * n + 1, vlen, dtype=np.uint64)))
        hv = torch.empty(n * 32, dtype=torch.uint8).pin_memory().numpy().reshape(n, 32)
        eh = torch.empty(ntx * 32, dtype=torch.uint8).pin_memory().numpy().reshape(ntx, 32)
        res = {}
        for name, chunk in (("pipelined", a.chunk_mib << 20), ("one_chunk", n * (vlen + 8) + 1)):
            p = m.CommitPipe(ctx, chunk_bytes=chunk)

            def step():
                _, _, st = p.precommit_csr(1, hvals_out=hv, eh_out=eh, **b)
                assert (st == 0).all()

            res[name] = timed(step, a.steps, a.warmup, sync)
            p.close()
        # the PCIe bound: plain pinned H2D of the same value + key bytes
        dv = torch.empty(n * vlen, dtype=torch.uint8, device=dev)
        dk = torch.empty(n * 8, dtype=torch.uint8, device=dev)

        def h2d():
            dv.copy_(vals, non_blocking=True)
            dk.copy_(keys, non_blocking=True)

        t_h2d = timed(h2d, a.steps, a.warmup, sync)
        # parity spot check: the oracle on the first 512 txs
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        import oracle as orc
        orc.use_shani(True)
        k = 512
        sub = dict(tx_off=b["tx_off"][:k + 1].copy(), keys=b["keys"], key_off=b["key_off"],
                   vals=b["vals"], val_off=b["val_off"])
        _, eh_o, _ = orc.precommit_batch(1, nthreads=16, **sub)
        parity = bool(np.array_equal(eh_o, eh[:k]))
        # CPU baseline: the oracle over all txs on 16 host threads (1 warm-up, median of 3)
        cpu = []
        for r in range(4):
            t0 = time.perf_counter()
            orc.precommit_batch(1, nthreads=16, **b)
            if r:
                cpu.append(time.perf_counter() - t0)
        t_cpu = float(np.median(cpu))
        gib = n * vlen / 2 ** 30
        t = res["pipelined"]
        out = {"metric": "precommit hashing of a tx batch incl. pinned H2D and D2H of hVals + Eh",
               "value": round(gib / t, 3), "unit": "GiB/s", "ms_per_step": round(t * 1e3, 3),
               "txs_per_s": round(ntx / t), "entries_per_s": round(n / t),
               "one_chunk_ms": round(res["one_chunk"] * 1e3, 3),
               "one_chunk_gibs": round(gib / res["one_chunk"], 3),
               "h2d_only_ms": round(t_h2d * 1e3, 3),
               "h2d_only_gbs": round(n * (vlen + 8) / t_h2d / 1e9, 2),
               "frac_of_h2d_bound": round(t_h2d / t, 4),
               "config": {"txs": ntx, "entries_per_tx": per, "value_len": vlen, "key_len": 8,
                          "chunk_mib": a.chunk_mib},
               "parity_first_512_txs": parity,
               "cpu_baseline": {"value": round(gib / t_cpu, 3), "unit": "GiB/s", "cores": 16,
                                "kind": "port",
                                "sample": "oracle orc_precommit_batch over the same batch, 16 "
                                          "threads, SHA-NI=%s, median of 3 = %.3f s"
                                          % (orc.has_shani(), t_cpu)}}

    elif a.workload == "ragged":
        out = ragged(a, m, N, L, ctx, dev, sync)
    elif a.workload == "document":
        out = document(a, ctx)
    elif a.workload == "values":
        out = values(a, m, N, L, ctx, dev, sync)
    elif a.workload == "c3range":
        out = c3range(a, m, N, L, ctx, dev, sync)
    elif a.workload == "replicate":
        out = replicate(a, m, N, L, ctx, sync)
    elif a.workload == "c2e2e":
        n, vlen, klen = 1 << 20, 1024, 8
        hv = torch.empty(n * vlen, dtype=torch.uint8).pin_memory()
        hk = torch.empty(n * klen, dtype=torch.uint8).pin_memory()
        hv.copy_(torch.randint(0, 256, (n * vlen,), dtype=torch.uint8))
        hk.copy_(torch.from_numpy(np.frombuffer(np.arange(n, dtype=">u8").tobytes(), np.uint8)))
        nl = m.levels_len(n)
        dv = torch.empty(n * vlen, dtype=torch.uint8, device=dev)
        dk = torch.empty(n * klen, dtype=torch.uint8, device=dev)
        dl = torch.empty(nl * 32, dtype=torch.uint8, device=dev)
        dr = torch.empty(32, dtype=torch.uint8, device=dev)
        hl = torch.empty(nl * 32, dtype=torch.uint8).pin_memory()
        hr = torch.empty(32, dtype=torch.uint8).pin_memory()

        def step():
            dv.copy_(hv, non_blocking=True)
            dk.copy_(hk, non_blocking=True)
            N.check(L.mh_dev_htree_build_entries_fixed(ctx.handle, 1, n, dk.data_ptr(), klen,
                                                       dv.data_ptr(), vlen, None, dl.data_ptr(),
                                                       dr.data_ptr()))
            hl.copy_(dl, non_blocking=True)
            hr.copy_(dr, non_blocking=True)

        t = timed(step, a.steps, a.warmup, sync)

        def dev_only():
            N.check(L.mh_dev_htree_build_entries_fixed(ctx.handle, 1, n, dk.data_ptr(), klen,
                                                       dv.data_ptr(), vlen, None, dl.data_ptr(),
                                                       dr.data_ptr()))

        td = timed(dev_only, a.steps, a.warmup, sync)
        out = {"metric": "htree build incl. pinned H2D of entries and D2H of all levels + root",
               "value": round(n * vlen / t / 2 ** 30, 3), "unit": "GiB/s",
               "ms_per_step": round(t * 1e3, 3), "device_resident_ms": round(td * 1e3, 3),
               "h2d_bytes": n * (vlen + klen), "d2h_bytes": nl * 32 + 32}
    elif a.workload == "wire":
        from immustore_amd.txlayer import TX_HEADER
        P = a.proofs
        D = a.depth
        W = 1 << D
        rng = np.random.default_rng(12)
        # ahtree of W appends and a W-leaf htree, both resident
        pay = torch.empty(W * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), 12))
        dlog = torch.empty(m.nodes_upto(W) * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(), W, 32,
                                             None))
        levels = torch.empty(m.levels_len(W) * 32, dtype=torch.uint8, device=dev)
        root = torch.empty(32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_htree_build_digests(ctx.handle, pay.data_ptr(), W, levels.data_ptr(),
                                             root.data_ptr()))
        # header pairs: tgt.ID in [2, W+1] (BlTxID = ID-1 <= W), src.ID in [1, tgt.ID)
        tid = rng.integers(2, W + 2, P).astype(np.uint64)
        sid = (rng.random(P) * (tid - 1)).astype(np.uint64) + 1

        def hdrs(ids):
            h = np.zeros(P, TX_HEADER)
            h["id"] = ids
            h["bl_tx_id"] = ids - 1
            h["ts"] = 1666885208 + ids.astype(np.int64)
            h["version"] = 1
            h["nentries"] = 16
            for f in ("bl_root", "prev_alh", "eh"):
                h[f] = rng.integers(0, 256, (P, 32), dtype=np.uint8)
            return torch.from_numpy(h.view(np.uint8).reshape(-1)).to(dev)

        hs, ht = hdrs(sid), hdrs(tid)
        off = torch.empty(P + 1, dtype=torch.int64, device=dev)
        st = torch.empty(P, dtype=torch.int32, device=dev)
        scratch = torch.empty(L.mh_pb_scratch_size(P), dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_dual_proof_v2_pb_batch(ctx.handle, 1, dlog.data_ptr(), W, P,
                                                hs.data_ptr(), ht.data_ptr(), None, None, 0,
                                                off.data_ptr(), st.data_ptr(),
                                                scratch.data_ptr()))
        sync()
        total = int(off[P].item())
        outb = torch.empty(total, dtype=torch.uint8, device=dev)

        def step_dual():
            N.check(L.mh_dev_dual_proof_v2_pb_batch(ctx.handle, 3, dlog.data_ptr(), W, P,
                                                    hs.data_ptr(), ht.data_ptr(), None,
                                                    outb.data_ptr(), total, off.data_ptr(),
                                                    st.data_ptr(), scratch.data_ptr()))

        prewarm(step_dual, sync, a.prewarm)
        td = timed_k(ctx, step_dual, a.steps, a.warmup, sync)
        kd = {k: ctx.timing(k)[0] / (a.steps + a.warmup) for k in ("pb_dual_size",
                                                                   "pb_dual_write")}
        assert int(st.abs().sum().item()) == 0
        # sample check against the oracle (C-oracle proofs + protobuf runtime)
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        import oracle as O
        import wire as WR
        # the oracle walks the device dLog (its values are pinned by the parity
        # tests; this checks the proof assembly and the encoding)
        o = O.AHtree(1)
        o.dlog = dlog.view(-1, 32).cpu().numpy()
        o.size = W
        hs_h = hs.cpu().numpy().view(TX_HEADER)
        ht_h = ht.cpu().numpy().view(TX_HEADER)
        offs = off.cpu().numpy()
        ob = outb.cpu().numpy()

        def rec(r):
            return {"id": int(r["id"]), "ts": int(r["ts"]), "bltxid": int(r["bl_tx_id"]),
                    "blroot": r["bl_root"].tobytes(), "prevalh": r["prev_alh"].tobytes(),
                    "eh": r["eh"].tobytes(), "version": int(r["version"]),
                    "nentries": int(r["nentries"]), "md": b""}

        ok = True
        for k in [int(x) for x in rng.integers(0, P, 300)]:
            ok &= WR.dual_proof_v2_pb(rec(hs_h[k]), rec(ht_h[k]), o) == (
                0, ob[offs[k]:offs[k + 1]].tobytes())
        # htree InclusionProof messages over the W-leaf tree
        leaf = torch.from_numpy(rng.integers(0, W, P).astype(np.int64)).to(dev)
        off2 = torch.empty(P + 1, dtype=torch.int64, device=dev)
        N.check(L.mh_dev_htree_inclusion_proof_pb_batch(ctx.handle, 1, levels.data_ptr(), W, P,
                                                        leaf.data_ptr(), None, 0, off2.data_ptr(),
                                                        st.data_ptr(), scratch.data_ptr()))
        sync()
        total2 = int(off2[P].item())
        outi = torch.empty(total2, dtype=torch.uint8, device=dev)

        def step_incl():
            N.check(L.mh_dev_htree_inclusion_proof_pb_batch(
                ctx.handle, 3, levels.data_ptr(), W, P, leaf.data_ptr(), outi.data_ptr(), total2,
                off2.data_ptr(), st.data_ptr(), scratch.data_ptr()))

        prewarm(step_incl, sync, a.prewarm)
        ti = timed_k(ctx, step_incl, a.steps, a.warmup, sync)
        ki = {k: ctx.timing(k)[0] / (a.steps + a.warmup) for k in ("pb_incl_size",
                                                                   "pb_incl_write")}
        assert int(st.abs().sum().item()) == 0
        lv_h = levels.view(-1, 32).cpu().numpy()
        leaf_h = leaf.cpu().numpy()
        offs2 = off2.cpu().numpy()
        oi = outi.cpu().numpy()
        for k in [int(x) for x in rng.integers(0, P, 300)]:
            ok &= WR.htree_inclusion_proof_pb(lv_h, W, int(leaf_h[k])) == (
                0, oi[offs2[k]:offs2[k + 1]].tobytes())
        # the client side: the same messages decoded (mh_dual_proof_v2_pb_decode_batch,
        # host buffers in and out: H2D of the messages, D2H of headers + terms)
        msgs_h = ob
        n_dec = P
        dsh, dth = np.zeros(n_dec, TX_HEADER), np.zeros(n_dec, TX_HEADER)
        dmd = np.zeros(2 * n_dec * 268, np.uint8)
        dio, dco = np.zeros(n_dec + 1, np.uint64), np.zeros(n_dec + 1, np.uint64)
        dst = np.zeros(n_dec, np.int32)
        moff = offs.astype(np.uint64)
        A = lambda x: x.ctypes.data  # noqa: E731
        rc = L.mh_dual_proof_v2_pb_decode_batch(ctx.handle, n_dec, A(msgs_h), A(moff), A(dsh), A(dth),
                                                A(dmd), A(dio), None, 0, A(dco), None, 0, A(dst))
        assert rc == 19, rc
        dit = np.zeros((int(dio[n_dec]), 32), np.uint8)
        dct = np.zeros((int(dco[n_dec]), 32), np.uint8)

        def step_decode():
            N.check(L.mh_dual_proof_v2_pb_decode_batch(
                ctx.handle, n_dec, A(msgs_h), A(moff), A(dsh), A(dth), A(dmd), A(dio), A(dit),
                dit.shape[0], A(dco), A(dct), dct.shape[0], A(dst)))

        tdec = timed(step_decode, max(1, a.steps // 2), 1, sync)
        ok &= bool((dst == 0).all())
        # ... then VerifyDualProofV2 over the decoded arrays (host in, statuses
        # out), against the fused call (messages in, statuses out)
        from immustore_amd import txlayer as TL
        _, s_alh = TL.tx_alh_batch(hs_h, b"", ctx)
        _, t_alh = TL.tx_alh_batch(ht_h, b"", ctx)
        vsrc, vtgt = hs_h["id"].copy(), ht_h["id"].copy()
        vst = np.zeros(n_dec, np.int32)

        def step_verify():
            N.check(L.mh_verify_dual_proof_v2_batch(
                ctx.handle, n_dec, A(dsh), A(dth), A(dmd), dmd.size, A(dio), A(dit), A(dco), A(dct),
                A(vsrc), A(vtgt), A(s_alh), A(t_alh), A(vst)))

        fst = np.zeros(n_dec, np.int32)

        def step_fused():
            N.check(L.mh_verify_dual_proof_v2_pb_batch(ctx.handle, n_dec, A(msgs_h), A(moff),
                                                       A(vsrc), A(vtgt), A(s_alh), A(t_alh), A(fst)))

        tver = timed(step_verify, max(1, a.steps // 2), 1, sync)
        tfus = timed(step_fused, max(1, a.steps // 2), 1, sync)
        ok &= bool((vst == fst).all())
        # the same with the messages in a pinned arena (a cgo shim's receive buffer)
        msgs_pin = torch.empty(msgs_h.size, dtype=torch.uint8).pin_memory().numpy()
        msgs_pin[:] = msgs_h

        def step_fused_pinned():
            N.check(L.mh_verify_dual_proof_v2_pb_batch(ctx.handle, n_dec, A(msgs_pin), A(moff),
                                                       A(vsrc), A(vtgt), A(s_alh), A(t_alh), A(fst)))

        tfp = timed(step_fused_pinned, max(1, a.steps // 2), 1, sync)
        ok &= bool((vst == fst).all())
        for k in [int(x) for x in rng.integers(0, P, 300)]:
            ok &= dsh[k].tobytes()[:128] == hs_h[k].tobytes()[:128]
            ok &= dth[k].tobytes()[:128] == ht_h[k].tobytes()[:128]
        out = {"metric": "DualProofV2 protobuf messages built on the device, 10^6 x (2^24 tree)",
               "value": round(P / td / 1e6, 3), "unit": "M messages/s",
               "ms_per_step": round(td * 1e3, 3), "bytes_out": total,
               "out_GBps": round(total / td / 1e9, 1),
               "kernel_ms": {k: round(v, 3) for k, v in kd.items()},
               "inclusion_proof_pb": {"M_messages_per_s": round(P / ti / 1e6, 3),
                                      "ms_per_step": round(ti * 1e3, 3), "bytes_out": total2,
                                      "out_GBps": round(total2 / ti / 1e9, 1),
                                      "kernel_ms": {k: round(v, 3) for k, v in ki.items()}},
               "decode_dual_proof_v2_pb": {
                   "M_messages_per_s": round(n_dec / tdec / 1e6, 3), "ms_per_step": round(tdec * 1e3, 3),
                   "bytes_in": int(moff[-1]), "in_GBps": round(int(moff[-1]) / tdec / 1e9, 2),
                   "note": "host buffers (pageable): H2D of the messages, D2H of the headers, "
                           "the packed metadata and the terms"},
               "verify_decoded_dual_proof_v2": {"M_proofs_per_s": round(n_dec / tver / 1e6, 3),
                                                "ms_per_step": round(tver * 1e3, 3)},
               "verify_dual_proof_v2_from_wire_fused": {
                   "M_messages_per_s": round(n_dec / tfus / 1e6, 3),
                   "ms_per_step": round(tfus * 1e3, 3),
                   "vs_decode_then_verify": round((tdec + tver) / tfus, 2),
                   "pinned_messages": {"M_messages_per_s": round(n_dec / tfp / 1e6, 3),
                                       "ms_per_step": round(tfp * 1e3, 3)},
                   "statuses_equal": bool((vst == fst).all()),
                   "note": "mh_verify_dual_proof_v2_pb_batch: messages + ids + Alh values up, "
                           "statuses down; the bench tree's payloads are not these headers' Alh, "
                           "so the verdicts are 'inclusion not valid' (every kernel still runs)"},
               "sample_vs_oracle": bool(ok)}

    elif a.workload == "dualv1":
        from immustore_amd.txlayer import TX_HEADER
        P, W = a.v1_proofs or 10 ** 5, 1 << a.v1_depth
        rng = np.random.default_rng(21)
        # the resident state of a server: the dLog of W appends and the Alh /
        # innerHash of every tx (random digests: the generator hashes nothing)
        pay = torch.empty(W * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, pay.data_ptr(), pay.numel(), 21))
        dlog = torch.empty(m.nodes_upto(W) * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0, pay.data_ptr(), W, 32,
                                             None))
        inner = torch.empty(W * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_fill_random(ctx.handle, inner.data_ptr(), inner.numel(), 22))
        alh = pay  # tx k's Alh is leaf k's payload
        tid = rng.integers(2, W + 1, P).astype(np.uint64)
        sid = (rng.random(P) * tid).astype(np.uint64) + 1
        sid = np.minimum(sid, tid)

        def hdrs(ids):
            h = np.zeros(P, TX_HEADER)
            h["id"] = ids
            lag = ids.astype(np.int64) - 1 - (ids.astype(np.int64) % 4)  # BlTxID 1-4 txs behind
            h["bl_tx_id"] = np.maximum(lag, 0).astype(np.uint64)
            h["ts"] = 1666885208 + ids.astype(np.int64)
            h["version"] = 1
            h["nentries"] = 16
            for f in ("bl_root", "prev_alh", "eh"):
                h[f] = rng.integers(0, 256, (P, 32), dtype=np.uint8)
            return torch.from_numpy(h.view(np.uint8).reshape(-1)).to(dev)

        hs, ht = hdrs(sid), hdrs(tid)
        off = torch.empty(P + 1, dtype=torch.int64, device=dev)
        st = torch.empty(P, dtype=torch.int32, device=dev)
        scratch = torch.empty(L.mh_pb_dual_scratch_size(P), dtype=torch.uint8, device=dev)

        def call(phase, out_ptr, cap):
            N.check(L.mh_dev_dual_proof_pb_batch(ctx.handle, phase, dlog.data_ptr(), W, P,
                                                 hs.data_ptr(), ht.data_ptr(), None, 1, W,
                                                 alh.data_ptr(), inner.data_ptr(), out_ptr, cap,
                                                 off.data_ptr(), st.data_ptr(), scratch.data_ptr()))

        call(1, None, 0)
        sync()
        total = int(off[P].item())
        outb = torch.empty(total, dtype=torch.uint8, device=dev)

        def step_v1():
            call(3, outb.data_ptr(), total)

        prewarm(step_v1, sync, a.prewarm)
        td = timed_k(ctx, step_v1, a.steps, a.warmup, sync)
        kd = {k: ctx.timing(k)[0] / (a.steps + a.warmup) for k in ("pb_dual1_size",
                                                                   "pb_dual1_write")}
        assert int(st.abs().sum().item()) == 0
        # sample check against the CPU restatement (tests/dual_v1_gen_util.py: the
        # oracle's ahtree walks over the device dLog + the protobuf runtime)
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        sys.path.insert(0, os.path.join(HERE, "tests"))
        import oracle as O
        import dual_v1_gen_util as U
        o = O.AHtree(1)
        o.dlog = dlog.view(-1, 32).cpu().numpy()
        o.size = W
        alh_h, inner_h = alh.view(-1, 32).cpu().numpy(), inner.view(-1, 32).cpu().numpy()
        hs_h = hs.cpu().numpy().view(TX_HEADER)
        ht_h = ht.cpu().numpy().view(TX_HEADER)
        offs = off.cpu().numpy()
        ob = outb.cpu().numpy()
        ok = True
        for k in [int(x) for x in rng.integers(0, P, 200)]:
            est, parts = U.go_dual_proof_parts(hs_h[k], ht_h[k], b"", o, 1, alh_h, inner_h)
            ok &= est == 0 and U.dual_v1_marshal(parts) == ob[offs[k]:offs[k + 1]].tobytes()
        sizes = np.diff(offs)
        out = {"metric": "DualProof (v1) protobuf messages built on the device, %d x (2^%d tree, "
                         "BlTxID 1-4 txs behind)" % (P, a.v1_depth),
               "value": round(P / td / 1e6, 3), "unit": "M proofs/s",
               "ms_per_step": round(td * 1e3, 3), "bytes_out": total,
               "out_GiBps": round(total / td / 2 ** 30, 2),
               "message_bytes": {"min": int(sizes.min()), "mean": round(float(sizes.mean()), 1),
                                 "max": int(sizes.max())},
               "kernel_ms": {k: round(v, 3) for k, v in kd.items()},
               "sample_vs_restatement": bool(ok)}

    elif a.workload == "dualv1verify":
        import ctypes as C
        from immustore_amd import txlayer as TL
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        sys.path.insert(0, os.path.join(HERE, "tests"))
        import oracle as O
        import wire as WIRE
        import dual_v1_gen_util as U
        from dual_v1_verify_util import reference
        s = U.synthetic_store()
        W = U.N_TX
        rng = np.random.default_rng(23)
        A = lambda x: x.ctypes.data  # noqa: E731
        todev = lambda x: torch.from_numpy(np.array(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        alh_h = np.stack([np.frombuffer(x, np.uint8) for x in s.alhs])
        alh = todev(alh_h)
        inner = todev(np.stack([np.frombuffer(x, np.uint8) for x in s.inners]))
        blob = todev(np.frombuffer(s.blob + bytes(16), np.uint8))
        dlog = torch.empty(m.nodes_upto(W) * 32, dtype=torch.uint8, device=dev)
        N.check(L.mh_dev_ahtree_append_batch(ctx.handle, dlog.data_ptr(), 0, alh.data_ptr(), W, 32,
                                             None))

        def generate(P):
            """P random pairs -> (messages, offsets, source ids, target ids), on the host"""
            tid = rng.integers(1, W + 1, P)
            sid = np.minimum((rng.random(P) * tid).astype(np.int64) + 1, tid)
            hs, ht = todev(s.recs[sid - 1]), todev(s.recs[tid - 1])
            off = torch.empty(P + 1, dtype=torch.int64, device=dev)
            st = torch.empty(P, dtype=torch.int32, device=dev)
            scratch = torch.empty(L.mh_pb_dual_scratch_size(P), dtype=torch.uint8, device=dev)
            outb = None
            for phase in (1, 3):
                N.check(L.mh_dev_dual_proof_pb_batch(
                    ctx.handle, phase, dlog.data_ptr(), W, P, hs.data_ptr(), ht.data_ptr(),
                    blob.data_ptr(), 1, W, alh.data_ptr(), inner.data_ptr(),
                    outb.data_ptr() if outb is not None else None,
                    outb.numel() if outb is not None else 0, off.data_ptr(), st.data_ptr(),
                    scratch.data_ptr()))
                sync()
                if phase == 1:
                    outb = torch.empty(int(off[P].item()), dtype=torch.uint8, device=dev)
            assert int(st.abs().sum().item()) == 0
            return outb.cpu().numpy(), off.cpu().numpy().astype(np.uint64), sid, tid

        P = a.v1_proofs
        if P is None:  # about 1 GiB of messages, from the mean of a sample
            _, o_, _, _ = generate(2048)
            P = int((1 << 30) / (int(o_[-1]) / 2048))
        msgs_h, moff, sid, tid = generate(P)
        total = int(moff[-1])
        sizes = np.diff(moff)

        def pin(shape, dtype):
            n_ = int(np.prod(shape)) * np.dtype(dtype).itemsize
            t_ = torch.empty(max(n_, 1), dtype=torch.uint8).pin_memory()
            keep.append(t_)
            return t_.numpy()[:n_].view(dtype).reshape(shape)

        keep = []
        msgs = pin(total + 16, np.uint8)
        msgs[:total] = msgs_h
        vsrc, vtgt = pin(P, np.uint64), pin(P, np.uint64)
        vsrc[:], vtgt[:] = sid, tid
        sa, ta = pin((P, 32), np.uint8), pin((P, 32), np.uint8)
        sa[:], ta[:] = alh_h[sid - 1], alh_h[tid - 1]
        # (a) the two existing calls, every array pinned: sizes from a first call
        d = {"src_hdr": pin(P, TL.TX_HEADER), "tgt_hdr": pin(P, TL.TX_HEADER),
             "md_blob": pin(2 * P * 268, np.uint8), "target_bl_tx_alh": pin((P, 32), np.uint8),
             "has_linear": pin(P, np.uint8), "linear_src": pin(P, np.uint64),
             "linear_tgt": pin(P, np.uint64), "has_advance": pin(P, np.uint8),
             "advance_incl_first": pin(P + 1, np.uint64), "advance_incl_off": pin(1, np.uint64)}
        lists = ("incl", "cons", "last", "linear", "advance")
        for t_ in lists:
            d[t_ + "_off"] = pin(P + 1, np.uint64)
        dst = pin(P, np.int32)
        caps = {}

        def decoded():
            for t_ in lists + ("advance_incl",):
                d[t_ + "_terms"] = pin((max(caps.get(t_, 0), 1), 32), np.uint8)
            d["advance_incl_off"] = pin(caps.get("nested", 0) + 1, np.uint64)
            return TL._DualProofDecoded(*[A(d[f]) for f, _ in TL._DualProofDecoded._fields_[:21]],
                                        *[caps.get(t_, 0) for t_ in lists], caps.get("nested", 0),
                                        caps.get("advance_incl", 0), 0, 0)

        dd = decoded()
        rc = L.mh_dual_proof_pb_decode_batch(ctx.handle, P, A(msgs), A(moff), C.byref(dd), A(dst))
        assert rc == N.MH_ERR_BUFFER_TOO_SMALL, rc
        caps = {t_: int(d[t_ + "_off"][P]) for t_ in lists}
        caps["nested"], caps["advance_incl"] = int(dd.nested_proofs), int(dd.nested_terms)
        dd = decoded()
        oka, okb, stb = pin(P, np.uint8), pin(P, np.uint8), pin(P, np.int32)
        B = TL._DualProofBatch(
            P, A(d["src_hdr"]), A(d["tgt_hdr"]), A(d["md_blob"]), d["md_blob"].size,
            A(d["incl_off"]), A(d["incl_terms"]), A(d["cons_off"]), A(d["cons_terms"]),
            A(d["target_bl_tx_alh"]), A(d["last_off"]), A(d["last_terms"]), A(d["has_linear"]),
            A(d["linear_src"]), A(d["linear_tgt"]), A(d["linear_off"]), A(d["linear_terms"]),
            A(d["has_advance"]), A(d["advance_off"]), A(d["advance_terms"]),
            A(d["advance_incl_first"]), A(d["advance_incl_off"]), A(d["advance_incl_terms"]),
            A(vsrc), A(vtgt), A(sa), A(ta))

        def step_decode():
            N.check(L.mh_dual_proof_pb_decode_batch(ctx.handle, P, A(msgs), A(moff), C.byref(dd),
                                                    A(dst)))

        def step_verify():
            N.check(L.mh_verify_dual_proof_batch(ctx.handle, C.byref(B), A(oka)))

        def step_two_calls():
            step_decode()
            step_verify()

        def step_fused():
            N.check(L.mh_verify_dual_proof_pb_batch(ctx.handle, P, A(msgs), A(moff), A(vsrc),
                                                    A(vtgt), A(sa), A(ta), A(stb), A(okb)))

        # the floor of either path: the message bytes over the link, pinned
        landing = torch.empty(total, dtype=torch.uint8, device=dev)
        src_pin = torch.from_numpy(msgs[:total])

        def step_h2d():
            landing.copy_(src_pin, non_blocking=True)

        prewarm(step_fused, sync, a.prewarm)
        th2d = timed(step_h2d, a.steps, a.warmup, sync)
        ta1 = timed(step_two_calls, a.steps, a.warmup, sync)
        tdec = timed(step_decode, a.steps, 0, sync)
        tfus = timed_k(ctx, step_fused, a.steps, a.warmup, sync)
        kd = {k: round(ctx.timing(k)[0] / (a.steps + a.warmup), 3)
              for k in ("pbd_dual1_size", "pbd_dual1_write", "dp1_prep", "tx_alh", "leaf_for",
                        "ahtree_verify", "linear_verify", "advance_chain", "dp1_nested",
                        "dp1_verdict")}
        ta2 = timed(step_two_calls, a.steps, a.warmup, sync)
        # the fused call with every 128 MiB chunk decoded alone (no groups of chunks)
        os.environ["MH_PB_GROUP_RATIO"] = "0"
        tfus0 = timed(step_fused, max(1, a.steps // 2), 1, sync)
        del os.environ["MH_PB_GROUP_RATIO"]
        ok = bool((dst == 0).all() and (stb == 0).all() and oka.all() and okb.all())
        for k in [int(x) for x in rng.integers(0, P, 100)]:
            raw = msgs_h[int(moff[k]):int(moff[k + 1])].tobytes()
            ok &= reference(WIRE, O, raw, int(sid[k]), int(tid[k]), bytes(sa[k]), bytes(ta[k])) == \
                (int(stb[k]), bool(okb[k])) == (0, True)
        # ... and a sample that must fail: the target id one too high
        vtgt[:] = tid + 1
        step_fused()
        sync()
        ok &= bool((stb == 0).all()) and not okb[sid != tid].any()
        vtgt[:] = tid
        ta_ = min(ta1, ta2)
        out = {"metric": "DualProof (v1) messages verified from the wire, %d x (synthetic store of "
                         "%d txs, not a 2^20 tree; every proof verifies)" % (P, W),
               "value": round(P / tfus / 1e3, 1), "unit": "k proofs/s (fused call)",
               "ms_per_step": round(tfus * 1e3, 3), "message_bytes": total,
               "message_bytes_each": {"min": int(sizes.min()), "mean": round(float(sizes.mean()), 1),
                                      "max": int(sizes.max())},
               "in_GBps": round(total / tfus / 1e9, 2),
               "two_calls_pinned": {"k_proofs_per_s": round(P / ta_ / 1e3, 1),
                                    "ms_per_step": [round(ta1 * 1e3, 3), round(ta2 * 1e3, 3)],
                                    "spread_ms": round(abs(ta1 - ta2) * 1e3, 3),
                                    "decode_ms": round(tdec * 1e3, 3),
                                    "note": "mh_dual_proof_pb_decode_batch + "
                                            "mh_verify_dual_proof_batch, every array pinned; run "
                                            "before and after the fused call"},
               "fused_vs_two_calls": round(ta_ / tfus, 2),
               "fused_chunk_by_chunk_ms": round(tfus0 * 1e3, 3),
               "h2d_floor": {"ms": round(th2d * 1e3, 3), "pinned_GBps": round(total / th2d / 1e9, 2),
                             "fused_over_floor": round(tfus / th2d, 2)},
               "kernel_ms": kd,
               "sample_vs_oracle": bool(ok)}

    out["workload"] = a.workload
    ctx.close()
    return out


def relaunch_one_rank():
    """MH_DIST_FORCE_PG=1 without a launcher: start this command as ONE rank
    under torch.distributed.run (a CHILD process, before anything here touches
    the GPU) and exit with its status."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    a = make_parser().parse_args()
    force = os.environ.get("MH_DIST_FORCE_PG", "") == "1"
    if force and "WORLD_SIZE" not in os.environ:
        raise SystemExit(relaunch_one_rank())
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or force:
        return distributed_main(a)
    out = run_single(a)
    print(json.dumps(out), flush=True)
    # a line whose own result check failed exits non-zero (as the multi-rank lines)
    bad = [k for k, v in list(out.items()) + list(out.get("resident_log", {}).items())
           if isinstance(v, dict) and v.get("root_check", v if k == "root_check" else {}).get("ok") is False]
    if bad:
        print("result check FAILED: %s" % bad, file=sys.stderr, flush=True)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
