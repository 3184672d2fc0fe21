// capi_answer.hip -- C ABI of the server's side of the verified reads: whole
// schema.VerifiableTx / schema.VerifiableEntry answers of a resident store in
// one device pass (db.VerifiableTxByID database.go:1462-1528, db.VerifiableSet
// :767-814, db.VerifiableGet :817-896).
//
//   the reads of a request: T, S, ImmuStore.DualProof's   k_ans_heads (answer_kernels.hip)
//   every distinct tx once: bitmap, scan, gathered cLog   k_ans_popc, k_ans_compact
//   ReadTx / ReadTxHeader / the tx readers: re-hash       mh_txlog_validate_clog over that cLog
//   innerHash                                             k_tx_alh
//   record verdicts, src / tgt, Alh links                 k_ans_verdict, k_ans_link
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

namespace {

bool is_device_ptr(const void *q, int device) {
    hipPointerAttribute_t a;
    const bool d = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeDevice &&
                   a.device == device;
    (void)hipGetLastError();
    return d;
}

}  // namespace

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
        if (!off || !status || (!out && out_cap) || !b->kind || !b->tx || !b->prove_since ||
            !b->key_off || !b->entry_off)
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (s->clog_entry_size != 12 && s->clog_entry_size != 44) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!monotonic(b->key_off, n) || !monotonic(b->entry_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t k0 = b->key_off[0], kb = b->key_off[n] - k0, e0 = b->entry_off[0],
                       eb = b->entry_off[n] - e0;
        if ((kb && !b->keys) || (eb && !b->entries)) return MH_ERR_ILLEGAL_ARGUMENTS;
        for (uint64_t p = 0; p < n; p++) {
            if (b->kind[p] != MH_ANS_TX && b->kind[p] != MH_ANS_ENTRY) return MH_ERR_ILLEGAL_ARGUMENTS;
            if (b->kind[p] == MH_ANS_TX && b->key_off[p + 1] != b->key_off[p])
                return MH_ERR_ILLEGAL_ARGUMENTS;
        }
        const uint64_t N = s->ntx, es = s->clog_entry_size;
        if (N >= (1ull << 36)) return MH_ERR_ILLEGAL_ARGUMENTS;  // the bitmap's words are scanned as ints
        if (N && (!s->txlog || !s->clog)) return MH_ERR_ILLEGAL_ARGUMENTS;
        // the tree's lock, then its context's (the order of mh_replicate_tx_batch): the whole
        // working set -- s_ans*, p_small, the stream -- is the context's
        std::lock_guard<std::recursive_mutex> lk_(t->mu);  // AHtree.mutex (ahtree.go:60-84)
        mh_ctx *c = t->ctx;
        std::lock_guard<std::mutex> lkc_(c->mu);
        MH_HIP(hipSetDevice(c->device));
        if (N) {
            if (!is_device_ptr(s->txlog, c->device) || !is_device_ptr(s->clog, c->device))
                return MH_ERR_ILLEGAL_ARGUMENTS;
            if (!dev_range(s->txlog, s->txlog_len + 256) || !dev_range(s->clog, N * es))
                return MH_ERR_ILLEGAL_ARGUMENTS;
        }
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        StreamGuard guard{{st}};  // no copy from or into the caller's arrays is pending on any way out

        // ---- requests up, the read set
        AnsArrays a{};
        a.txlog = s->txlog, a.clog = s->clog, a.txlog_len = s->txlog_len, a.ntx = N, a.es = (uint32_t)es;
        a.n = n;
        a.words = (N + 63) / 64;
        const uint64_t W = std::max<uint64_t>(a.words, 1);
        const size_t scan_bytes = pb_scan_temp_bytes(std::max(n, W));
        Layout L;
        const uint64_t b_kind = L.add(n), b_tx = L.add(n * 8), b_since = L.add(n * 8),
                       b_ko = L.add((n + 1) * 8), b_eo = L.add((n + 1) * 8), b_keys = L.add(kb),
                       b_ent = L.add(eb), b_pre = L.add(n * 4), b_hs = L.add(n * sizeof(mh_tx_header)),
                       b_ht = L.add(n * sizeof(mh_tx_header)), b_leaf = L.add(n * 8),
                       b_dst = L.add(n * 4), b_dpo = L.add((n + 1) * 8), b_sz = L.add(n * 8),
                       b_dpos = L.add(n * 8), b_off = L.add((n + 1) * 8), b_st = L.add(n * 4),
                       b_bits = L.add(W * 8), b_wcnt = L.add(W * 8), b_rank = L.add((W + 1) * 8),
                       b_scan = L.add(scan_bytes), b_dps = L.add(pb_dual_v1_scratch_bytes(n));
        MH_HIP(c->s_ans.ensure(L.total));
        uint8_t *base = c->s_ans.as<uint8_t>();
        auto U = [&](uint64_t o) { return (uint64_t *)(base + o); };
        auto h2d = [&](uint64_t at, const void *p, uint64_t bytes) -> hipError_t {
            return bytes ? hipMemcpyAsync(base + at, p, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
        };
        MH_HIP(h2d(b_kind, b->kind, n));
        MH_HIP(h2d(b_tx, b->tx, n * 8));
        MH_HIP(h2d(b_since, b->prove_since, n * 8));
        MH_HIP(h2d(b_ko, b->key_off, (n + 1) * 8));
        MH_HIP(h2d(b_eo, b->entry_off, (n + 1) * 8));
        MH_HIP(h2d(b_keys, kb ? b->keys + k0 : nullptr, kb));
        MH_HIP(h2d(b_ent, eb ? b->entries + e0 : nullptr, eb));
        a.kind = base + b_kind, a.tx = U(b_tx), a.since = U(b_since);
        a.key_off = U(b_ko), a.entry_off = U(b_eo);
        a.keys = base + b_keys - k0, a.entries = base + b_ent - e0;  // biased: the offsets keep their base
        a.pre = (int32_t *)(base + b_pre), a.hs = (MhTxHeader *)(base + b_hs);
        a.ht = (MhTxHeader *)(base + b_ht), a.leaf = U(b_leaf);
        a.dst = (int32_t *)(base + b_dst), a.dp_off = U(b_dpo), a.sizes = U(b_sz), a.dpos = U(b_dpos);
        a.off = U(b_off), a.status = (int32_t *)(base + b_st);
        a.bits = U(b_bits), a.wcnt = U(b_wcnt), a.rank = U(b_rank);
        uint8_t *scan = base + b_scan;
        MH_HIP(hipMemsetAsync(a.bits, 0, W * 8, st));
        MH_HIP(hipMemsetAsync(a.wcnt, 0, W * 8, st));
        MH_HIP(launch_ans_heads(st, tm, a));
        if (a.words) MH_HIP(launch_ans_popc(st, tm, a));
        MH_HIP(scan_offsets_u64(st, W, a.wcnt, a.rank, scan, scan_bytes));
        MH_HIP(c->p_small.ensure(64));
        volatile uint64_t *hw = c->p_small.as<volatile uint64_t>();
        MH_HIP(hipMemcpyAsync((void *)hw, a.rank + W, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 1: the distinct txs read
        const uint64_t D = a.D = hw[0], D1 = std::max<uint64_t>(D, 1);
        if (D > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count; grids of D blocks

        // ---- every distinct tx read and re-hashed once
        const size_t dscan_bytes = pb_scan_temp_bytes(D1);
        Layout S;
        const uint64_t d_ids = S.add(D1 * 8), d_cl = S.add(D1 * es),
                       d_hd = S.add(D1 * sizeof(mh_tx_header)), d_alh = S.add(D1 * 32),
                       d_in = S.add(D1 * 32), d_rst = S.add(D1 * 4), d_lnk = S.add(D1),
                       d_fl = S.add(D1 * 4), d_ec = S.add(D1 * 8), d_nc = S.add(D1 * 8),
                       d_tb = S.add(D1 * 8), d_lo = S.add((D1 + 1) * 8), d_vo = S.add((D1 + 1) * 8),
                       d_tp = S.add((D1 + 1) * 8), d_hsz = S.add(D1 * 4), d_es = S.add(D1 * 8),
                       d_am = S.add(D1 * kTxInnerStride), d_scan = S.add(dscan_bytes);
        MH_HIP(c->s_ans_tx.ensure(S.total));
        uint8_t *sb = c->s_ans_tx.as<uint8_t>();
        auto V = [&](uint64_t o) { return (uint64_t *)(sb + o); };
        a.ids = V(d_ids), a.gclog = sb + d_cl, a.hd = (MhTxHeader *)(sb + d_hd);
        a.alh = sb + d_alh, a.inner = sb + d_in, a.rst = (int32_t *)(sb + d_rst), a.lnk = sb + d_lnk;
        a.flags = (uint32_t *)(sb + d_fl), a.ecnt = V(d_ec), a.ncnt = V(d_nc), a.txbody = V(d_tb);
        a.leaf_off = V(d_lo), a.lvl_off = V(d_vo), a.txpos = V(d_tp), a.hsz = (uint32_t *)(sb + d_hsz);
        a.ent_start = V(d_es);
        MH_HIP(hipMemsetAsync(sb, 0, d_am, st));  // (no slot: the scans below still read one item)
        if (D) {
            MH_HIP(launch_ans_compact(st, tm, a));
            // ReadTx with the integrity check, per distinct tx (its own waits; c->mu is held)
            if (int e = txlog_validate_clog_core(c, s->txlog, s->txlog_len, a.gclog, D, (uint32_t)es,
                                                 s->max_entries, s->max_key_len, a.hd, a.alh, a.rst,
                                                 nullptr, nullptr))
                return e;
            hw = c->p_small.as<volatile uint64_t>();  // (the read path may have grown it)
            MH_HIP(launch_tx_alh(st, tm, D, a.hd, s->txlog, nullptr, sb + d_am, nullptr, nullptr,
                                 a.inner, a.alh, nullptr));
        }
        MH_HIP(launch_ans_verdict(st, tm, a));
        MH_HIP(scan_offsets_u64(st, D1, a.ecnt, V(d_lo), sb + d_scan, dscan_bytes));
        MH_HIP(scan_offsets_u64(st, D1, a.ncnt, V(d_vo), sb + d_scan, dscan_bytes));
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
        MH_HIP(scan_offsets_u64(st, D1, a.txbody, V(d_tp), sb + d_scan, dscan_bytes));

        // ---- DualProof(src, tgt): statuses and lengths; then every answer's
        RankWindow win{a.bits, a.rank, a.rst, a.lnk, N, a.dpos};
        MH_HIP(launch_pb_dual_v1_ranked(st, tm, 1, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                        s->txlog, win, a.alh, a.inner, nullptr, U(b_dpo),
                                        (int32_t *)(base + b_dst), base + b_dps));
        MH_HIP(launch_ans_size(st, tm, a));
        MH_HIP(scan_offsets_u64(st, n, a.sizes, U(b_off), scan, scan_bytes));
        MH_HIP(hipMemcpyAsync(off, a.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync((void *)hw, a.txpos + D1, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 3: the sizes
        const uint64_t total = off[n], tx_bytes = hw[0];
        // the answers that fit are a prefix of the batch's bytes
        uint64_t fit = 0;
        for (uint64_t p = 0; p < n; p++)
            if (off[p + 1] <= out_cap) fit = off[p + 1];
        (void)total;

        // ---- write: schema.Tx once per tx, the answers around it, the proofs
        Layout O;
        const uint64_t o_tx = O.add(tx_bytes + 16), o_out = O.add(fit + 64);
        MH_HIP(c->s_ans_out.ensure(O.total));
        uint8_t *ob = c->s_ans_out.as<uint8_t>();
        a.txbuf = ob + o_tx, a.out = ob + o_out, a.out_cap = fit;
        MH_HIP(launch_ans_tx_write(st, tm, a));
        MH_HIP(launch_ans_assemble(st, tm, a));
        MH_HIP(launch_pb_dual_v1_ranked(st, tm, 2, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                        s->txlog, win, a.alh, a.inner, a.out, U(b_dpo), a.status,
                                        base + b_dps));
        if (fit) MH_HIP(hipMemcpyAsync(out, a.out, fit, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, a.status, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        guard.streams.clear();
        return MH_OK;
    });
}
