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
//   DualProofFromProto  database_protoconv.go:213-287   dual1_decode_size / _write
//                                                       (k_pbd_dual1, pb_decode.hip)
//   deleted / Eh rules, TxHeader.Alh, source and target k_vtx_answer
//   store.VerifyDualProof  verification.go:127-235      dual_proof_v1_core (capi_tx.hip)
//
// The frame is the one of mh_verify_verifiable_entry_pb_batch: the messages
// go up in chunks (PbChunkFrame, ChunkCopier), chunk 0 carrying the
// per-answer arrays and the request's keys and values; groups of chunks
// (PbChunkFrame::group / wait_group) are decoded and verified as they land.
// The host knows every tree's shape from the request (spec_off), so the entry
// records need no scan.
#include "capi_internal.hpp"

// the frame's rules first: its limits on n, before n sizes any other read
bool verified_tx_args_ok(const mh_verified_tx_batch &b, const int32_t *status, const uint8_t *ok,
                         const uint64_t *new_tx, const uint8_t *new_alh) {
    const uint64_t n = b.n;
    if (!b.kind || !b.spec_off || !b.key_off || !b.val_off || !b.at_tx || !b.state_tx || !b.state_alh)
        return false;
    if (!PbChunkFrame::args_ok(n, b.msgs, b.msg_off, status && ok && new_tx && new_alh)) return false;
    if (!monotonic(b.spec_off, n)) return false;
    const uint64_t s0 = b.spec_off[0], T = b.spec_off[n] - s0;
    for (uint64_t p = 0; p < n; p++) {
        const uint64_t K = b.spec_off[p + 1] - b.spec_off[p];
        switch (b.kind[p]) {
        case MH_VTX_SET:
        case MH_VTX_REFERENCE:
        case MH_VTX_ZADD:
            if (K != 1) return false;
            break;
        case MH_VTX_SET_ALL:
            if (K < 1) return false;
            break;
        case MH_VTX_TX_BY_ID:
            if (K != 0) return false;
            break;
        default: return false;
        }
    }
    if (!monotonic(b.key_off + s0, T) || !monotonic(b.val_off + s0, T)) return false;
    return (b.key_off[s0 + T] == b.key_off[s0] || b.keys) &&
           (b.val_off[s0 + T] == b.val_off[s0] || b.vals);
}

extern "C" int mh_verify_verifiable_tx_pb_batch(mh_ctx *c, const mh_verified_tx_batch *b,
                                                int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                                uint8_t *new_alh, uint8_t *eh_out) {
    return mh_guard([&]() -> int {
        if (!c || !b) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        if (n == 0) return MH_OK;
        if (!verified_tx_args_ok(*b, status, ok, new_tx, new_alh)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t *spec_off = b->spec_off, *key_off = b->key_off, *val_off = b->val_off;
        const uint64_t s0 = spec_off[0], T = spec_off[n] - s0;
        const uint64_t k0 = key_off[s0], kb = key_off[s0 + T] - k0;
        const uint64_t v0 = val_off[s0], vb = val_off[s0 + T] - v0;
        PbChunkFrame F;
        if (int e = F.open_checked(c, n, b->msgs, b->msg_off)) return e;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        F.group();
        const uint64_t M = F.group_n, GB = F.group_bytes;  // the largest group
        uint64_t TG = 0;                                   // the most slots of a group
        for (int g = 0; g < F.ng; g++)
            TG = std::max(TG, spec_off[F.cut[F.gcut[g + 1]]] - spec_off[F.cut[F.gcut[g]]]);
        Layout L;
        // the messages and, in the same allocation (DualProof ranges are
        // relative to the messages), one group's concatenation area; the
        // caller's arrays and the results, whole; then one group's work
        const uint64_t b_msg = L.add(F.mb + 16), b_cat = L.add(GB + 16), b_off = L.add((n + 1) * 8),
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
        const Dual1Scratch ds = dual1_decode_scratch(L, M);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        auto U = [&](uint64_t off) { return (uint64_t *)(base + off); };
        ChunkCopier cc(c);
        F.fill(cc, base + b_msg,
               {{base + b_off, b->msg_off, (n + 1) * 8},
                {base + b_kind, b->kind, n},
                {base + b_soff, spec_off, (n + 1) * 8},
                {base + b_at, b->at_tx, n * 8},
                {base + b_stx, b->state_tx, n * 8},
                {base + b_salh, b->state_alh, n * 32},
                {base + b_koff, key_off + s0, (T + 1) * 8},
                {base + b_keys, b->keys ? b->keys + k0 : nullptr, kb},
                {base + b_voff, val_off + s0, (T + 1) * 8},
                {base + b_vals, b->vals ? b->vals + v0 : nullptr, vb}});
        MH_HIP(cc.start());
        const uint8_t *dmsg = base + b_msg - F.m0;
        int32_t *dst_all = (int32_t *)(base + b_st), *dst2 = (int32_t *)(base + b_dst2);
        DevBuf &tb = c->s_tree;
        std::vector<uint64_t> leaf_off;
        for (int g = 0; g < F.ng; g++) {
            uint64_t lo, nk;
            if (int e = F.wait_group(c, cc, g, lo, nk)) return e;
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
            MH_HIP(scan_offsets_u64(st, nk, v.cnt, vso, base + ds.scan, ds.scan_bytes));
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
            // 3. DualProofFromProto over the located ranges; its term area, the
            // Alh messages and the verifier's scratch in one allocation
            uint64_t totals[kCounts];
            if (int e = dual1_decode_size(c, nk, dmsg, v.dual_beg, v.dual_end, base, ds, dst2, totals))
                return e;
            const uint64_t Q = totals[kQ];
            Layout TL;
            const Dual1Terms dterms = dual1_decode_terms(TL, totals);
            const uint64_t t_alh = TL.add(nk * kTxInnerStride),
                           t_core = TL.add(dual_proof_v1_scratch_bytes(nk, Q));
            MH_HIP(tb.ensure(TL.total + 8));
            uint8_t *dt = tb.as<uint8_t>();
            Dual1Arrays o;
            if (int e = dual1_decode_write(c, nk, dmsg, v.dual_beg, v.dual_end, base, ds, dt, dterms,
                                           dst2, o))
                return e;
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
