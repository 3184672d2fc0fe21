// capi_vtx.hip -- C ABI of the client side of the verified writes and of
// VerifiedTxByID: what pkg/client does with every schema.VerifiableTx answer
// before the state signature check (VerifiedSet client.go:1337-1391,
// streamVerifiedSet streams.go:205-260, VerifiedSetReferenceAt :1716-1770,
// VerifiedZAddAt :1882-1940, VerifiedTxByID :1554-1583), for a batch of
// answers in one device pass.
//
//   proto.Unmarshal into schema.VerifiableTx, TxFromProto's reads
//     database_protoconv.go:69-95                      k_pbd_vtx (pb_decode.hip)
//   TxEntryDigest of every wire entry  tx.go:690-731    k_vtx_leaf (ventry_kernels.hip)
//   EncodeEntrySpec / EncodeReference, EntrySpecDigest,
//   Tx.IndexOf, the inclusion decision                  k_vtx_spec
//   BuildHashTree  tx.go:332-355                        build_many_dev (capi_tx.hip)
//   DualProofFromProto  database_protoconv.go:213-287   k_pbd_dual1 (pb_decode.hip)
//   deleted / Eh rules, TxHeader.Alh, source and target k_vtx_answer
//   store.VerifyDualProof  verification.go:127-235      dual_proof_v1_core (capi_tx.hip)
//
// The frame is the one of mh_verify_verifiable_entry_pb_batch: the messages
// go up in chunks (PbChunkFrame, ChunkCopier), chunk 0 carrying the
// per-answer arrays and the request's keys and values; groups of chunks are
// decoded and verified as they land.  The host knows every tree's shape from
// the request (spec_off), so the entry records need no scan.
#include <hipcub/hipcub.hpp>

#include "capi_internal.hpp"

namespace {

constexpr uint32_t kMdSlot = MH_MAX_TX_METADATA_LEN;  // metadata bytes per header

}  // namespace

extern "C" int mh_verify_verifiable_tx_pb_batch(mh_ctx *c, const mh_verified_tx_batch *b,
                                                int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                                uint8_t *new_alh, uint8_t *eh_out) {
    return mh_guard([&]() -> int {
        if (!c || !b) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        if (n == 0) return MH_OK;
        if (!b->kind || !b->spec_off || !b->key_off || !b->val_off || !b->at_tx || !b->state_tx ||
            !b->state_alh)
            return MH_ERR_ILLEGAL_ARGUMENTS;
        // the frame's limit (a header's md_off is 32 bits), before n sizes any read
        if (2 * n * (uint64_t)kMdSlot > 0xffffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!monotonic(b->spec_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t *spec_off = b->spec_off, *key_off = b->key_off, *val_off = b->val_off;
        const uint64_t s0 = spec_off[0], T = spec_off[n] - s0;
        for (uint64_t p = 0; p < n; p++) {
            const uint64_t K = spec_off[p + 1] - spec_off[p];
            switch (b->kind[p]) {
            case MH_VTX_SET:
            case MH_VTX_REFERENCE:
            case MH_VTX_ZADD:
                if (K != 1) return MH_ERR_ILLEGAL_ARGUMENTS;
                break;
            case MH_VTX_SET_ALL:
                if (K < 1) return MH_ERR_ILLEGAL_ARGUMENTS;
                break;
            case MH_VTX_TX_BY_ID:
                if (K != 0) return MH_ERR_ILLEGAL_ARGUMENTS;
                break;
            default: return MH_ERR_ILLEGAL_ARGUMENTS;
            }
        }
        if (!monotonic(key_off + s0, T) || !monotonic(val_off + s0, T))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t k0 = key_off[s0], kb = key_off[s0 + T] - k0;
        const uint64_t v0 = val_off[s0], vb = val_off[s0 + T] - v0;
        if ((kb && !b->keys) || (vb && !b->vals)) return MH_ERR_ILLEGAL_ARGUMENTS;
        PbChunkFrame F;
        // at_tx / state_tx / state_alh stand where the dual-proof calls pass
        // src / tgt / the Alh values: the frame only checks and keeps them
        if (int e = F.open(c, n, b->msgs, b->msg_off, b->at_tx, b->state_tx, b->state_alh,
                           b->state_alh, status && ok && new_tx && new_alh))
            return e;
        const uint64_t *msg_off = b->msg_off;
        const std::vector<uint64_t> &cut = F.cut;
        const uint64_t m0 = F.m0, mb = F.mb;
        const int nch = F.nch;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        const std::vector<int> gcut = F.groups();
        const int ng = (int)gcut.size() - 1;
        uint64_t M = 0, GB = 0, TG = 0;  // answers / message bytes / slots of the largest group
        for (int g = 0; g < ng; g++) {
            const uint64_t lo = cut[gcut[g]], hi = cut[gcut[g + 1]];
            M = std::max(M, hi - lo);
            GB = std::max(GB, msg_off[hi] - msg_off[lo]);
            TG = std::max(TG, spec_off[hi] - spec_off[lo]);
        }
        size_t scan_bytes = 0;
        MH_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (const uint64_t *)nullptr,
                                                (uint64_t *)nullptr, (int)M, st));
        Layout L;
        // the messages and, in the same allocation (DualProof ranges are
        // relative to the messages), one group's concatenation area; the
        // caller's arrays and the results, whole; then one group's work
        const uint64_t b_msg = L.add(mb + 16), b_cat = L.add(GB + 16), b_off = L.add((n + 1) * 8),
                       b_kind = L.add(n), b_soff = L.add((n + 1) * 8), b_at = L.add(n * 8),
                       b_stx = L.add(n * 8), b_salh = L.add(n * 32), b_koff = L.add((T + 1) * 8),
                       b_keys = L.add(kb + 16), b_voff = L.add((T + 1) * 8), b_vals = L.add(vb + 16),
                       b_st = L.add(n * 4), b_ok = L.add(n), b_ntx = L.add(n * 8),
                       b_nalh = L.add(n * 32), b_eh = L.add(n * 32);
        const uint64_t b_thdr = L.add(M * sizeof(mh_tx_header)), b_tmd = L.add(M * (uint64_t)kMdSlot),
                       b_live = L.add(M), b_vcnt = L.add(M * 8), b_vso = L.add((M + 1) * 8),
                       b_recs = L.add(std::max<uint64_t>(TG, 1) * sizeof(VtxRec)),
                       b_dig = L.add(std::max<uint64_t>(TG, 1) * 32), b_dok = L.add(TG + 1),
                       b_xok = L.add(TG + 1), b_roots = L.add(M * 32), b_dbeg = L.add(M * 8),
                       b_dend = L.add(M * 8), b_dst2 = L.add(M * 4), b_vsrc = L.add(M * 8),
                       b_vtgt = L.add(M * 8), b_valh = L.add(2 * M * 32), b_pok = L.add(M),
                       b_dok2 = L.add(M);
        const uint64_t b_cnt = L.add(kCounts * M * 8), b_so = L.add(kCounts * (M + 1) * 8),
                       b_scan = L.add(scan_bytes), b_h = L.add(2 * M * sizeof(mh_tx_header)),
                       b_md = L.add(2 * M * (uint64_t)kMdSlot), b_tba = L.add(M * 32),
                       b_flags = L.add(2 * M), b_lsrc = L.add(2 * M * 8);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        auto U = [&](uint64_t off) { return (uint64_t *)(base + off); };
        ChunkCopier cc(c);
        cc.chunks.resize(nch);
        cc.chunks[0] = {{base + b_off, msg_off, (n + 1) * 8},
                        {base + b_kind, b->kind, n},
                        {base + b_soff, spec_off, (n + 1) * 8},
                        {base + b_at, b->at_tx, n * 8},
                        {base + b_stx, b->state_tx, n * 8},
                        {base + b_salh, b->state_alh, n * 32},
                        {base + b_koff, key_off + s0, (T + 1) * 8},
                        {base + b_keys, b->keys ? b->keys + k0 : nullptr, kb},
                        {base + b_voff, val_off + s0, (T + 1) * 8},
                        {base + b_vals, b->vals ? b->vals + v0 : nullptr, vb}};
        for (int k = 0; k < nch; k++) {
            const uint64_t lo = cut[k], hi = cut[k + 1];
            cc.chunks[k].push_back({base + b_msg + (msg_off[lo] - m0), b->msgs + msg_off[lo],
                                    msg_off[hi] - msg_off[lo]});
        }
        MH_HIP(cc.start());
        const uint8_t *dmsg = base + b_msg - m0;
        int32_t *dst_all = (int32_t *)(base + b_st), *dst2 = (int32_t *)(base + b_dst2);
        uint64_t *cnt = U(b_cnt), *so = U(b_so);
        DevBuf &tb = c->s_tree;
        std::vector<uint64_t> leaf_off;
        for (int g = 0; g < ng; g++) {
            for (int k = gcut[g]; k < gcut[g + 1]; k++) {
                MH_HIP(cc.wait(k));
                MH_HIP(hipStreamWaitEvent(st, c->ev_chunks[k], 0));
            }
            const uint64_t lo = cut[gcut[g]], nk = cut[gcut[g + 1]] - lo;
            const uint64_t Tg = spec_off[lo + nk] - spec_off[lo];
            const uint64_t *doff = (const uint64_t *)(base + b_off) + lo;
            int32_t *dst = dst_all + lo;
            // 1. the envelopes: validate, status, the tx header, the entry
            // records, the DualProof ranges
            VtxArrays v{};
            v.kind = base + b_kind + lo;
            v.spec_off = (const uint64_t *)(base + b_soff) + lo;
            v.state_tx = (const uint64_t *)(base + b_stx) + lo;
            v.spec_base = spec_off[lo];
            v.cnt = U(b_vcnt);
            v.cat = base + b_cat;
            v.dual_beg = U(b_dbeg);
            v.dual_end = U(b_dend);
            v.hdr = (mh_tx_header *)(base + b_thdr);
            v.md_blob = base + b_tmd;
            v.live = base + b_live;
            v.recs = (VtxRec *)(base + b_recs);
            {
                TimerScope ts(tm, "pbd_vtx_size", st);
                MH_HIP(launch_pbd_vtx(st, false, nk, dmsg, doff, v, dst));
            }
            uint64_t *vso = U(b_vso);
            MH_HIP(hipMemsetAsync(vso, 0, 8, st));
            {
                size_t sb = scan_bytes;
                MH_HIP(hipcub::DeviceScan::InclusiveSum(base + b_scan, sb, (const uint64_t *)v.cnt,
                                                        vso + 1, (int)nk, st));
            }
            volatile uint64_t *tot = c->p_small.as<volatile uint64_t>();
            MH_HIP(launch_put2_host(st, vso + nk, vso + nk, (uint64_t *)c->p_small.p));
            MH_HIP(hipStreamSynchronize(st));
            // every concatenated byte is a byte of its message
            if (tot[0] > GB) return MH_ERR_ILLEGAL_STATE;
            v.cat_off = vso;
            {
                TimerScope ts(tm, "pbd_vtx_write", st);
                MH_HIP(launch_pbd_vtx(st, true, nk, dmsg, doff, v, dst));
            }
            // 2. the wire entries' digests, the request's spec digests against
            // them, every answer's tree
            VtxVerify w{};
            w.nk = nk;
            w.msgs = dmsg;
            w.keys = base + b_keys - k0;
            w.vals = base + b_vals - v0;
            w.spec_off = v.spec_off;
            w.key_off = (const uint64_t *)(base + b_koff) - s0;
            w.val_off = (const uint64_t *)(base + b_voff) - s0;
            w.kind = v.kind;
            w.at_tx = (const uint64_t *)(base + b_at) + lo;
            w.state_tx = v.state_tx;
            w.state_alh = base + b_salh + 32 * lo;
            w.status = dst;
            w.live = v.live;
            w.hdr = v.hdr;
            w.md_blob = v.md_blob;
            w.recs = v.recs;
            w.dig = base + b_dig;
            w.dok = base + b_dok;
            w.xok = base + b_xok;
            w.roots = base + b_roots;
            if (Tg) {
                // a slot of an answer that is not live is touched by no kernel
                MH_HIP(hipMemsetAsync(w.dig, 0, Tg * 32, st));
                MH_HIP(hipMemsetAsync(w.dok, 0, Tg, st));
                MH_HIP(hipMemsetAsync(w.xok, 0, Tg, st));
                MH_HIP(launch_vtx_leaf(st, tm, Tg, w));
                MH_HIP(launch_vtx_spec(st, tm, Tg, w));
            }
            leaf_off.resize(nk + 1);
            for (uint64_t p = 0; p <= nk; p++) leaf_off[p] = spec_off[lo + p] - spec_off[lo];
            if (int e = build_many_dev(c, st, nk, leaf_off.data(), w.dig, base + b_roots,
                                       c->s_digests, c->s_offs))
                return e;
            // 3. DualProofFromProto over the located ranges: sizes, the eight
            // scans, the seven totals, the write pass
            {
                TimerScope ts(tm, "pbd_dual1_size", st);
                MH_HIP(launch_pbd_dual1_range(st, false, nk, dmsg, v.dual_beg, v.dual_end, cnt,
                                              Dual1Arrays{}, dst2));
            }
            for (int j = 0; j < kCounts; j++) {
                uint64_t *sj = so + (uint64_t)j * (nk + 1);
                MH_HIP(hipMemsetAsync(sj, 0, 8, st));
                size_t sb = scan_bytes;
                MH_HIP(hipcub::DeviceScan::InclusiveSum(base + b_scan, sb,
                                                        (const uint64_t *)(cnt + j * nk), sj + 1,
                                                        (int)nk, st));
            }
            MH_HIP(launch_put7_host(st, so, nk, (uint64_t *)c->p_small.p));
            MH_HIP(hipStreamSynchronize(st));
            uint64_t totals[kMd];
            for (int j = 0; j < kMd; j++) totals[j] = tot[j];
            const uint64_t Q = totals[kQ];
            Layout TL;
            uint64_t t_terms[5];
            for (int j = 0; j < 5; j++) t_terms[j] = TL.add(totals[j] * 32);
            const uint64_t t_qt = TL.add(totals[kQT] * 32), t_qo = TL.add((Q + 1) * 8),
                           t_alh = TL.add(nk * kTxInnerStride),
                           t_core = TL.add(dual_proof_v1_scratch_bytes(nk, Q));
            MH_HIP(tb.ensure(TL.total + 8));
            uint8_t *dt = tb.as<uint8_t>();
            Dual1Arrays o;
            for (int j = 0; j < kCounts; j++) o.off[j] = so + (uint64_t)j * (nk + 1);
            for (int j = 0; j < 5; j++) o.terms[j] = dt + t_terms[j];
            o.qterms = dt + t_qt;
            o.qoff = (uint64_t *)(dt + t_qo);
            o.src_hdr = (mh_tx_header *)(base + b_h);
            o.tgt_hdr = o.src_hdr + nk;
            o.md_blob = base + b_md;
            o.tbl_alh = base + b_tba;
            o.has_lin = base + b_flags;
            o.has_adv = base + b_flags + nk;
            o.lin_src = U(b_lsrc);
            o.lin_tgt = o.lin_src + nk;
            {
                TimerScope ts(tm, "pbd_dual1_write", st);
                MH_HIP(launch_pbd_dual1_range(st, true, nk, dmsg, v.dual_beg, v.dual_end, nullptr, o,
                                              dst2));
            }
            // 4. the answer: its slots, the Eh rules, the Alh; source and
            // target; VerifyDualProof (verification.go:127-235); the verdict
            w.src_hdr = o.src_hdr;
            w.tgt_hdr = o.tgt_hdr;
            w.dual_md = o.md_blob;
            w.alh_msg = dt + t_alh;
            w.src = U(b_vsrc);
            w.tgt = U(b_vtgt);
            w.src_alh = base + b_valh;
            w.tgt_alh = base + b_valh + 32 * nk;
            w.pre_ok = base + b_pok;
            w.eh_out = base + b_eh + 32 * lo;
            MH_HIP(launch_vtx_answer(st, tm, w));
            if (int e = dual_proof_v1_core(st, tm, nk, o, w.src, w.tgt, w.src_alh, w.tgt_alh, dst2,
                                           2 * nk * (uint64_t)kMdSlot, kDp1V0MetadataDropped, Q,
                                           dt + t_core, base + b_dok2))
                return e;
            MH_HIP(launch_ventry_verdict(st, tm, nk, dst, w.state_tx, w.pre_ok, base + b_dok2, w.tgt,
                                         w.tgt_alh, base + b_ok + lo, U(b_ntx) + lo,
                                         base + b_nalh + 32 * lo));
        }
        MH_HIP(cc.join());
        MH_HIP(hipMemcpyAsync(status, dst_all, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(ok, base + b_ok, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(new_tx, base + b_ntx, n * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(new_alh, base + b_nalh, n * 32, hipMemcpyDeviceToHost, st));
        if (eh_out) MH_HIP(hipMemcpyAsync(eh_out, base + b_eh, n * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}
