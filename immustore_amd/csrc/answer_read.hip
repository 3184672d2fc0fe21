// answer_read.hip -- AnsRead (capi_internal.hpp), the read-set stage behind
// mh_verifiable_answer_pb_batch (capi_answer.hip, whose header lists its
// kernels) and mh_tx_answer_pb_batch (capi_txspec.hip).
#include "capi_internal.hpp"

int AnsRead::requests(uint64_t n, Layout &L) {
    const uint64_t N = s.ntx;
    a.txlog = s.txlog, a.clog = s.clog, a.txlog_len = s.txlog_len, a.ntx = N, a.es = s.clog_entry_size;
    a.n = n;
    a.words = (N + 63) / 64;
    W = std::max<uint64_t>(a.words, 1);
    scan_bytes = pb_scan_temp_bytes(std::max(n, W));
    b_kind = L.add(n), b_tx = L.add(n * 8), b_since = L.add(n * 8);
    const uint64_t b_pre = L.add(n * 4), b_hs = L.add(n * sizeof(mh_tx_header)),
                   b_ht = L.add(n * sizeof(mh_tx_header)), b_leaf = L.add(n * 8);
    b_dst = L.add(n * 4), b_dpo = L.add((n + 1) * 8);
    const uint64_t b_sz = L.add(n * 8), b_dpos = L.add(n * 8);
    b_off = L.add((n + 1) * 8);
    const uint64_t b_st = L.add(n * 4), b_bits = L.add(W * 8), b_wcnt = L.add(W * 8),
                   b_rank = L.add((W + 1) * 8), b_scan = L.add(scan_bytes);
    b_dps = L.add(pb_dual_v1_scratch_bytes(n));
    MH_HIP(c->s_ans.ensure(L.total));
    base = c->s_ans.as<uint8_t>();
    auto U = [&](uint64_t o) { return (uint64_t *)(base + o); };
    a.kind = base + b_kind, a.tx = U(b_tx), a.since = U(b_since);
    a.pre = (int32_t *)(base + b_pre), a.hs = (MhTxHeader *)(base + b_hs);
    a.ht = (MhTxHeader *)(base + b_ht), a.leaf = U(b_leaf);
    a.dst = (int32_t *)(base + b_dst), a.dp_off = U(b_dpo), a.sizes = U(b_sz), a.dpos = U(b_dpos);
    a.off = U(b_off), a.status = (int32_t *)(base + b_st);
    a.bits = U(b_bits), a.wcnt = U(b_wcnt), a.rank = U(b_rank);
    scan = base + b_scan;
    return MH_OK;
}

int AnsRead::heads() {
    hipStream_t st = c->stream;
    Timer *tm = c->tm();
    MH_HIP(hipMemsetAsync(a.bits, 0, W * 8, st));
    MH_HIP(hipMemsetAsync(a.wcnt, 0, W * 8, st));
    MH_HIP(launch_ans_heads(st, tm, a));
    if (a.words) MH_HIP(launch_ans_popc(st, tm, a));
    MH_HIP(scan_offsets_u64(st, W, a.wcnt, a.rank, scan, scan_bytes));
    MH_HIP(c->p_small.ensure(64));
    hw = c->p_small.as<volatile uint64_t>();
    MH_HIP(hipMemcpyAsync((void *)hw, a.rank + W, 8, hipMemcpyDeviceToHost, st));
    MH_HIP(hipStreamSynchronize(st));  // wait 1: the distinct txs read
    a.D = hw[0], D1 = std::max<uint64_t>(a.D, 1);
    if (a.D > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count; grids of D blocks
    dscan_bytes = pb_scan_temp_bytes(D1);
    return MH_OK;
}

int AnsRead::reads(Layout &S) {
    hipStream_t st = c->stream;
    Timer *tm = c->tm();
    const uint64_t D = a.D, es = a.es;
    const uint64_t d_ids = S.add(D1 * 8), d_cl = S.add(D1 * es), d_hd = S.add(D1 * sizeof(mh_tx_header)),
                   d_alh = S.add(D1 * 32), d_in = S.add(D1 * 32), d_rst = S.add(D1 * 4),
                   d_lnk = S.add(D1), d_fl = S.add(D1 * 4), d_ec = S.add(D1 * 8), d_nc = S.add(D1 * 8),
                   d_lo = S.add((D1 + 1) * 8), d_es = S.add(D1 * 8), d_am = S.add(D1 * kTxInnerStride),
                   d_scan = S.add(dscan_bytes);
    MH_HIP(c->s_ans_tx.ensure(S.total));
    sb = c->s_ans_tx.as<uint8_t>();
    auto V = [&](uint64_t o) { return (uint64_t *)(sb + o); };
    a.ids = V(d_ids), a.gclog = sb + d_cl, a.hd = (MhTxHeader *)(sb + d_hd);
    a.alh = sb + d_alh, a.inner = sb + d_in, a.rst = (int32_t *)(sb + d_rst), a.lnk = sb + d_lnk;
    a.flags = (uint32_t *)(sb + d_fl), a.ecnt = V(d_ec), a.ncnt = V(d_nc);
    a.leaf_off = V(d_lo), a.ent_start = V(d_es);
    dscan = sb + d_scan;
    MH_HIP(hipMemsetAsync(sb, 0, d_am, st));  // (no slot: the caller's scans still read one item)
    if (D) {
        MH_HIP(launch_ans_compact(st, tm, a));
        // ReadTx with the integrity check, per distinct tx (its own waits; c->mu is held)
        if (int e = txlog_validate_clog_core(c, s.txlog, s.txlog_len, a.gclog, D, (uint32_t)es, s.max_entries,
                                             s.max_key_len, a.hd, a.alh, a.rst, nullptr, nullptr))
            return e;
        hw = c->p_small.as<volatile uint64_t>();  // (the read path may have grown it)
        MH_HIP(launch_tx_alh(st, tm, D, a.hd, s.txlog, nullptr, sb + d_am, nullptr, nullptr, a.inner,
                             a.alh, nullptr));
    }
    MH_HIP(launch_ans_verdict(st, tm, a));
    MH_HIP(scan_offsets_u64(st, D1, a.ecnt, V(d_lo), dscan, dscan_bytes));
    return MH_OK;
}
