// capi_answer.hip -- C ABI of the server's side of the verified reads: whole
// schema.VerifiableTx / schema.VerifiableEntry answers of a resident store in
// one device pass (db.VerifiableTxByID database.go:1462-1528, db.VerifiableSet
// :767-814, db.VerifiableGet :817-896).
//
//   the store: its arguments, where it lies               store_args_ok, store_resident (capi_txlog.hip)
//   AnsRead, the read-set stage (answer_read.hip; also capi_txspec.hip's):
//   the reads of a request: T, S, ImmuStore.DualProof's   k_ans_heads (answer_kernels.hip)
//   every distinct tx once: bitmap, scan, gathered cLog   k_ans_popc, k_ans_compact
//   ReadTx / ReadTxHeader / the tx readers: re-hash       mh_txlog_validate_clog over that cLog
//   innerHash                                             k_tx_alh
//   record verdicts, src / tgt, Alh links                 k_ans_verdict, k_ans_link
//   the call's own:
//   entry index, digests, trees of the ENTRY txs          k_txe_index, k_txe_leaf, k_ans_trees
//   Tx.IndexOf                                            k_ans_find
//   DualProof sizes and statuses                          k_pb_dual1_size over the RankWindow
//   sizes, one scan                                       k_ans_esize, k_ans_txsize, k_ans_size
//   schema.Tx once per tx, the answers, the DualProofs    k_ans_tx_*, k_ans_assemble, k_pb_dual1_write
//
// The host waits for the number of distinct txs (scratch), inside the read
// path, for the entry and node totals of the asked txs, and for the offsets
// (the output's size); only off, status and the messages come back.
#include "capi_internal.hpp"

extern "C" int mh_verifiable_answer_pb_batch(mh_ahtree *t, const mh_answer_store *s,
                                             const mh_answer_batch *b, uint8_t *out, uint64_t out_cap,
                                             uint64_t *off, int32_t *status) {
    return mh_guard([&]() -> int {
        if (!t || !s || !b) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        if (n == 0) {
            if (off) off[0] = 0;
            return MH_OK;
        }
        // ---- the arguments alone
        if (!off || !status || (!out && out_cap) || !b->kind || !b->tx || !b->prove_since ||
            !b->key_off || !b->entry_off)
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (!store_args_ok(*s, nullptr, 0)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!monotonic(b->key_off, n) || !monotonic(b->entry_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t k0 = b->key_off[0], kb = b->key_off[n] - k0, e0 = b->entry_off[0],
                       eb = b->entry_off[n] - e0;
        if ((kb && !b->keys) || (eb && !b->entries)) return MH_ERR_ILLEGAL_ARGUMENTS;
        for (uint64_t p = 0; p < n; p++) {
            if (b->kind[p] != MH_ANS_TX && b->kind[p] != MH_ANS_ENTRY) return MH_ERR_ILLEGAL_ARGUMENTS;
            if (b->kind[p] == MH_ANS_TX && b->key_off[p + 1] != b->key_off[p])
                return MH_ERR_ILLEGAL_ARGUMENTS;
        }
        const uint64_t N = s->ntx;
        if (N >= (1ull << 36)) return MH_ERR_ILLEGAL_ARGUMENTS;  // the bitmap's words are scanned as ints
        // the tree's lock, then its context's (the order of mh_replicate_tx_batch): the whole
        // working set -- s_ans*, p_small, the stream -- is the context's
        std::lock_guard<std::recursive_mutex> lk_(t->mu);  // AHtree.mutex (ahtree.go:60-84)
        mh_ctx *c = t->ctx;
        std::lock_guard<std::mutex> lkc_(c->mu);
        MH_HIP(hipSetDevice(c->device));
        // ---- where the store lies
        if (!store_resident(*s, nullptr, 0, c->device)) return MH_ERR_ILLEGAL_ARGUMENTS;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        StreamGuard guard{{st}};  // no copy from or into the caller's arrays is pending on any way out

        // ---- requests up, the read set
        AnsArrays a{};
        AnsRead r{c, *s, a};
        Layout L;
        const uint64_t b_ko = L.add((n + 1) * 8), b_eo = L.add((n + 1) * 8), b_keys = L.add(kb),
                       b_ent = L.add(eb);
        if (int e = r.requests(n, L)) return e;
        uint8_t *base = r.base;
        auto U = [&](uint64_t o) { return (uint64_t *)(base + o); };
        auto h2d = [&](uint64_t at, const void *p, uint64_t bytes) -> hipError_t {
            return bytes ? hipMemcpyAsync(base + at, p, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
        };
        MH_HIP(h2d(r.b_kind, b->kind, n));
        MH_HIP(h2d(r.b_tx, b->tx, n * 8));
        MH_HIP(h2d(r.b_since, b->prove_since, n * 8));
        MH_HIP(h2d(b_ko, b->key_off, (n + 1) * 8));
        MH_HIP(h2d(b_eo, b->entry_off, (n + 1) * 8));
        MH_HIP(h2d(b_keys, kb ? b->keys + k0 : nullptr, kb));
        MH_HIP(h2d(b_ent, eb ? b->entries + e0 : nullptr, eb));
        a.key_off = U(b_ko), a.entry_off = U(b_eo);
        a.keys = base + b_keys - k0, a.entries = base + b_ent - e0;  // biased: the offsets keep their base
        if (int e = r.heads()) return e;  // wait 1: the distinct txs read
        const uint64_t D = a.D, D1 = r.D1;

        // ---- every distinct tx read and re-hashed once
        Layout S;
        const uint64_t d_tb = S.add(D1 * 8), d_vo = S.add((D1 + 1) * 8), d_tp = S.add((D1 + 1) * 8),
                       d_hsz = S.add(D1 * 4);
        if (int e = r.reads(S)) return e;
        uint8_t *sb = r.sb;
        auto V = [&](uint64_t o) { return (uint64_t *)(sb + o); };
        volatile uint64_t *hw = r.hw;
        a.txbody = V(d_tb), a.lvl_off = V(d_vo), a.txpos = V(d_tp), a.hsz = (uint32_t *)(sb + d_hsz);
        MH_HIP(scan_offsets_u64(st, D1, a.ncnt, V(d_vo), r.dscan, r.dscan_bytes));
        MH_HIP(hipMemcpyAsync((void *)hw, a.leaf_off + D, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync((void *)(hw + 1), a.lvl_off + D, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 2: the entries and tree nodes of the asked txs
        const uint64_t E = a.E = D ? hw[0] : 0, NN = D ? hw[1] : 0, E1 = std::max<uint64_t>(E, 1);
        if (E > 0x7fffffffull) return MH_ERR_ILLEGAL_STATE;  // hipcub's int item count

        // ---- the entries of the asked txs: index, digests, trees, the asked keys
        const size_t escan_bytes = pb_scan_temp_bytes(E1);
        Layout X;
        const uint64_t e_ro = X.add(E1 * 8), e_ver = X.add(E1),
                       e_dig = X.add(E1 * 32), e_sz = X.add(E1 * 8), e_pos = X.add((E1 + 1) * 8),
                       e_nodes = X.add(std::max<uint64_t>(NN, 1) * 32), e_scan = X.add(escan_bytes);
        MH_HIP(c->s_ans_ent.ensure(X.total));
        uint8_t *xb = c->s_ans_ent.as<uint8_t>();
        a.rec_off = (uint64_t *)(xb + e_ro), a.ver = xb + e_ver;
        a.dig = xb + e_dig, a.esz = (uint64_t *)(xb + e_sz), a.epos = (uint64_t *)(xb + e_pos);
        a.nodes = xb + e_nodes;
        if (E) {
            MH_HIP(launch_txe_index(st, tm, D, s->txlog, a.hd, a.ent_start, a.leaf_off, a.rec_off, a.ver));
            MH_HIP(launch_txe_leaf(st, tm, E, s->txlog, a.rec_off, a.ver, false, a.dig));
        }
        if (NN) MH_HIP(launch_ans_trees(st, tm, a));
        MH_HIP(launch_ans_find(st, tm, a));
        MH_HIP(scan_offsets_u64(st, E, a.esz, (uint64_t *)(xb + e_pos), xb + e_scan, escan_bytes));
        MH_HIP(launch_ans_txsize(st, tm, a));
        MH_HIP(scan_offsets_u64(st, D1, a.txbody, V(d_tp), r.dscan, r.dscan_bytes));

        // ---- DualProof(src, tgt): statuses and lengths; then every answer's
        RankWindow win{a.bits, a.rank, a.rst, a.lnk, N, a.dpos};
        MH_HIP(launch_pb_dual_v1_ranked(st, tm, 1, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                        s->txlog, win, a.alh, a.inner, nullptr, U(r.b_dpo),
                                        (int32_t *)(base + r.b_dst), base + r.b_dps));
        MH_HIP(launch_ans_size(st, tm, a));
        MH_HIP(scan_offsets_u64(st, n, a.sizes, U(r.b_off), r.scan, r.scan_bytes));
        MH_HIP(hipMemcpyAsync(off, a.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync((void *)hw, a.txpos + D1, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 3: the sizes
        const uint64_t tx_bytes = hw[0], fit = fit_prefix(off, n, out_cap);

        // ---- write: schema.Tx once per tx, the answers around it, the proofs
        Layout O;
        const uint64_t o_tx = O.add(tx_bytes + 16), o_out = O.add(fit + 64);
        MH_HIP(c->s_ans_out.ensure(O.total));
        uint8_t *ob = c->s_ans_out.as<uint8_t>();
        a.txbuf = ob + o_tx, a.out = ob + o_out, a.out_cap = fit;
        MH_HIP(launch_ans_tx_write(st, tm, a));
        MH_HIP(launch_ans_assemble(st, tm, a));
        MH_HIP(launch_pb_dual_v1_ranked(st, tm, 2, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                        s->txlog, win, a.alh, a.inner, a.out, U(r.b_dpo), a.status,
                                        base + r.b_dps));
        if (fit) MH_HIP(hipMemcpyAsync(out, a.out, fit, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, a.status, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        guard.streams.clear();
        return MH_OK;
    });
}
