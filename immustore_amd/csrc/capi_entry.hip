// capi_entry.hip -- C ABI of the client side of VerifiableGet: what
// pkg/client's verifiedGet (pkg/client/client.go:1119-1234) does with every
// answer before the state signature check, for a batch of answers in one
// device pass.
//
//   proto.Unmarshal into schema.VerifiableEntry      k_pbd_ventry (pb_decode.hip)
//   DualProofFromProto  database_protoconv.go:213-287  dual1_decode_size / _write
//                                                      (k_pbd_dual1, pb_decode.hip)
//   EncodeEntrySpec / EncodeReference, EntrySpecDigest, htree.VerifyInclusion,
//   the source / target choice, TxHeader.Alh          k_ventry_verify (ventry_kernels.hip)
//   store.VerifyDualProof  verification.go:127-235     dual_proof_v1_core (capi_tx.hip)
//
// The frame is the one of mh_verify_dual_proof_pb_batch: the messages go up
// in chunks (PbChunkFrame, ChunkCopier), chunk 0 carrying the per-answer
// arrays and the request keys; groups of chunks (PbChunkFrame::group /
// wait_group) are decoded and verified as they land.
#include "capi_internal.hpp"

namespace {

// One group's envelope pass: sizes, the two scans, the totals (inclusion
// terms, concatenated DualProof bytes) read back through pinned memory, the
// inclusion term area (c->s_ventry), the write pass.  so: 2 x (nk + 1) words.
int ventry_decode_group(mh_ctx *c, hipStream_t st, Timer *tm, uint64_t nk, const uint8_t *dmsg,
                        const uint64_t *doff, VentryArrays &v, uint64_t *so, uint8_t *scan,
                        size_t scan_bytes, uint64_t cat_cap, int32_t *dst, uint64_t tot[2]) {
    {
        TimerScope ts(tm, "pbd_ventry_size", st);
        MH_HIP(launch_pbd_ventry(st, false, nk, dmsg, doff, v, dst));
    }
    for (int j = 0; j < 2; j++)
        MH_HIP(scan_offsets_u64(st, nk, v.cnt + j * nk, so + (uint64_t)j * (nk + 1), scan, scan_bytes));
    volatile uint64_t *pt = c->p_small.as<volatile uint64_t>();
    MH_HIP(launch_put2_host(st, so + nk, so + (nk + 1) + nk, (uint64_t *)c->p_small.p));
    MH_HIP(hipStreamSynchronize(st));
    tot[0] = pt[0], tot[1] = pt[1];
    // every concatenated byte is a byte of its message
    if (tot[1] > cat_cap) return MH_ERR_ILLEGAL_STATE;
    MH_HIP(c->s_ventry.ensure(std::max<uint64_t>(tot[0], 1) * 32));
    v.term_off = so;
    v.cat_off = so + (nk + 1);
    v.terms = c->s_ventry.as<uint8_t>();
    {
        TimerScope ts(tm, "pbd_ventry_write", st);
        MH_HIP(launch_pbd_ventry(st, true, nk, dmsg, doff, v, dst));
    }
    return MH_OK;
}

}  // namespace

// the frame's rules first: its limit on n, before n sizes the read of key_off
bool verified_get_args_ok(const mh_verified_get_batch &b, const int32_t *status, const uint8_t *ok,
                          const uint64_t *new_tx, const uint8_t *new_alh) {
    if (!b.key_off || !b.at_tx || !b.state_tx || !b.state_alh) return false;
    if (!PbChunkFrame::args_ok(b.n, b.msgs, b.msg_off, status && ok && new_tx && new_alh))
        return false;
    if (!monotonic(b.key_off, b.n)) return false;
    return b.key_off[b.n] == b.key_off[0] || b.keys;
}

extern "C" int mh_verify_verifiable_entry_pb_batch(mh_ctx *c, const mh_verified_get_batch *b,
                                                   int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                                   uint8_t *new_alh) {
    return mh_guard([&]() -> int {
        if (!c || !b) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        if (n == 0) return MH_OK;
        if (!verified_get_args_ok(*b, status, ok, new_tx, new_alh)) return MH_ERR_ILLEGAL_ARGUMENTS;
        PbChunkFrame F;
        if (int e = F.open_checked(c, n, b->msgs, b->msg_off)) return e;
        const uint64_t *key_off = b->key_off;
        const uint64_t k0 = key_off[0], kb = key_off[n] - k0;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        F.group();
        const uint64_t M = F.group_n, GB = F.group_bytes;  // the largest group
        Layout L;
        // the messages and, in the same allocation (DualProof ranges are
        // relative to the messages), one group's concatenation area; the
        // caller's arrays and the results, whole; then one group's decode
        const uint64_t b_msg = L.add(F.mb + 16), b_cat = L.add(GB + 16), b_off = L.add((n + 1) * 8),
                       b_at = L.add(n * 8), b_stx = L.add(n * 8), b_salh = L.add(n * 32),
                       b_koff = L.add((n + 1) * 8), b_keys = L.add(kb + 16), b_st = L.add(n * 4),
                       b_ok = L.add(n), b_ntx = L.add(n * 8), b_nalh = L.add(n * 32);
        const uint64_t b_info = L.add(M * sizeof(mh_verifiable_entry_info)),
                       b_vcnt = L.add(2 * M * 8), b_vso = L.add(2 * (M + 1) * 8),
                       b_dbeg = L.add(M * 8), b_dend = L.add(M * 8), b_dst2 = L.add(M * 4),
                       b_vsrc = L.add(M * 8), b_vtgt = L.add(M * 8), b_valh = L.add(2 * M * 32),
                       b_iok = L.add(M), b_dok = L.add(M);
        const Dual1Scratch ds = dual1_decode_scratch(L, M);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        auto U = [&](uint64_t off) { return (uint64_t *)(base + off); };
        ChunkCopier cc(c);
        F.fill(cc, base + b_msg,
               {{base + b_off, b->msg_off, (n + 1) * 8},
                {base + b_at, b->at_tx, n * 8},
                {base + b_stx, b->state_tx, n * 8},
                {base + b_salh, b->state_alh, n * 32},
                {base + b_koff, key_off, (n + 1) * 8},
                {base + b_keys, b->keys ? b->keys + k0 : nullptr, kb}});
        MH_HIP(cc.start());
        const uint8_t *dmsg = base + b_msg - F.m0, *dkeys = base + b_keys - k0;
        int32_t *dst_all = (int32_t *)(base + b_st), *dst2 = (int32_t *)(base + b_dst2);
        DevBuf &tb = c->s_tree;
        for (int g = 0; g < F.ng; g++) {
            uint64_t lo, nk;
            if (int e = F.wait_group(c, cc, g, lo, nk)) return e;
            const uint64_t *doff = (const uint64_t *)(base + b_off) + lo;
            int32_t *dst = dst_all + lo;
            // 1. the envelopes: validate, locate, inclusion terms, DualProof ranges
            VentryArrays v{};
            v.info = (mh_verifiable_entry_info *)(base + b_info);
            v.cnt = U(b_vcnt);
            v.cat = base + b_cat;
            v.dual_beg = U(b_dbeg);
            v.dual_end = U(b_dend);
            v.cat_all = 0;
            uint64_t vt[2];
            if (int e = ventry_decode_group(c, st, tm, nk, dmsg, doff, v, U(b_vso), base + ds.scan,
                                            ds.scan_bytes, GB, dst, vt))
                return e;
            // 2. DualProofFromProto over the located ranges; its term area, the
            // Alh messages and the verifier's scratch in one allocation
            uint64_t totals[kCounts];
            if (int e = dual1_decode_size(c, nk, dmsg, v.dual_beg, v.dual_end, base, ds, dst2, totals))
                return e;
            const uint64_t Q = totals[kQ];
            Layout T;
            const Dual1Terms dterms = dual1_decode_terms(T, totals);
            const uint64_t t_alh = T.add(nk * kTxInnerStride),
                           t_core = T.add(dual_proof_v1_scratch_bytes(nk, Q));
            MH_HIP(tb.ensure(T.total + 8));
            uint8_t *dt = tb.as<uint8_t>();
            Dual1Arrays o;
            if (int e = dual1_decode_write(c, nk, dmsg, v.dual_beg, v.dual_end, base, ds, dt, dterms,
                                           dst2, o))
                return e;
            // 3. value hash, digest, inclusion, the header's Alh; source and target
            VentryVerify w{};
            w.msgs = dmsg;
            w.keys = dkeys;
            w.key_off = (const uint64_t *)(base + b_koff) + lo;
            w.at_tx = (const uint64_t *)(base + b_at) + lo;
            w.state_tx = (const uint64_t *)(base + b_stx) + lo;
            w.state_alh = base + b_salh + 32 * lo;
            w.status = dst;
            w.info = v.info;
            w.term_off = v.term_off;
            w.terms = v.terms;
            w.src_hdr = o.src_hdr;
            w.tgt_hdr = o.tgt_hdr;
            w.md_blob = o.md_blob;
            w.alh_msg = dt + t_alh;
            w.src = U(b_vsrc);
            w.tgt = U(b_vtgt);
            w.src_alh = base + b_valh;
            w.tgt_alh = base + b_valh + 32 * nk;
            w.incl_ok = base + b_iok;
            MH_HIP(launch_ventry_verify(st, tm, nk, w));
            // 4. VerifyDualProof (verification.go:127-235), then the verdict
            if (int e = dual_proof_v1_core(st, tm, nk, o, w.src, w.tgt, w.src_alh, w.tgt_alh, dst2,
                                           2 * nk * (uint64_t)kMdSlot, kDp1V0MetadataDropped, Q,
                                           dt + t_core, base + b_dok))
                return e;
            MH_HIP(launch_ventry_verdict(st, tm, nk, dst, w.state_tx, w.incl_ok, base + b_dok, w.tgt,
                                         w.tgt_alh, base + b_ok + lo, U(b_ntx) + lo,
                                         base + b_nalh + 32 * lo));
        }
        MH_HIP(cc.join());
        MH_HIP(hipMemcpyAsync(status, dst_all, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(ok, base + b_ok, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(new_tx, base + b_ntx, n * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(new_alh, base + b_nalh, n * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

// The envelope pass alone, every DualProof copied out (cat_all): one upload,
// the two passes, the arrays back.
extern "C" int mh_verifiable_entry_pb_decode_batch(mh_ctx *c, uint64_t n, const uint8_t *msgs,
                                                   const uint64_t *msg_off,
                                                   mh_verifiable_entry_decoded *out,
                                                   int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c || !out || !out->incl_off || !out->dual_off) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n && (!msg_off || !status || !out->info)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) {
            out->incl_off[0] = out->dual_off[0] = 0;
            return MH_OK;
        }
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (!monotonic(msg_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t m0 = msg_off[0], mb = msg_off[n] - m0;
        if (mb && !msgs) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        MH_HIP(c->p_small.ensure(64));
        hipStream_t st = c->stream;
        const size_t scan_bytes = pb_scan_temp_bytes(n);
        Layout L;
        const uint64_t b_msg = L.add(mb + 16), b_cat = L.add(mb + 16), b_off = L.add((n + 1) * 8),
                       b_info = L.add(n * sizeof(mh_verifiable_entry_info)),
                       b_vcnt = L.add(2 * n * 8), b_vso = L.add(2 * (n + 1) * 8),
                       b_dbeg = L.add(n * 8), b_dend = L.add(n * 8), b_st = L.add(n * 4),
                       b_scan = L.add(scan_bytes);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        if (mb) MH_HIP(hipMemcpyAsync(base + b_msg, msgs + m0, mb, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        VentryArrays v{};
        v.info = (mh_verifiable_entry_info *)(base + b_info);
        v.cnt = (uint64_t *)(base + b_vcnt);
        v.cat = base + b_cat;
        v.dual_beg = (uint64_t *)(base + b_dbeg);
        v.dual_end = (uint64_t *)(base + b_dend);
        v.cat_all = 1;
        uint64_t tot[2];
        uint64_t *so = (uint64_t *)(base + b_vso);
        if (int e = ventry_decode_group(c, st, c->tm(), n, base + b_msg - m0,
                                        (const uint64_t *)(base + b_off), v, so, base + b_scan,
                                        scan_bytes, mb, (int32_t *)(base + b_st), tot))
            return e;
        MH_HIP(hipMemcpyAsync(out->incl_off, so, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->dual_off, so + (n + 1), (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, base + b_st, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->info, v.info, n * sizeof(mh_verifiable_entry_info),
                              hipMemcpyDeviceToHost, st));
        const bool fits = tot[0] <= out->incl_cap && tot[1] <= out->dual_cap;
        const bool have = (!tot[0] || out->incl_terms) && (!tot[1] || out->dual_bytes);
        if (fits && have) {
            if (tot[0])
                MH_HIP(hipMemcpyAsync(out->incl_terms, v.terms, tot[0] * 32, hipMemcpyDeviceToHost, st));
            if (tot[1])
                MH_HIP(hipMemcpyAsync(out->dual_bytes, v.cat, tot[1], hipMemcpyDeviceToHost, st));
        }
        MH_HIP(hipStreamSynchronize(st));
        return !fits ? MH_ERR_BUFFER_TOO_SMALL : !have ? MH_ERR_ILLEGAL_ARGUMENTS : MH_OK;
    });
}
