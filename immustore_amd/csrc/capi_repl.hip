// capi_repl.hip -- C ABI of the follower's side of replication: what
// ImmuStore.ReplicateTx (immustore.go:2772-2932) does with the bytes ExportTx
// wrote, up to and including the ahtree append of the tx's Alh, for a run of
// exported txs in one device pass.
//
//   the envelope, TxHeader.ReadFrom, the entry and trailer walk
//     immustore.go:2773-2881, tx.go:166-247          k_repl_struct (repl_kernels.hip)
//   OngoingTx.set, validateAgainst, validateEntries
//     ongoing_tx.go:242-267, :798, immustore.go:3243  k_repl_dup, k_repl_set
//   hVal and the entry digests  immustore.go:1620-1632  k_repl_leaf
//   BuildHashTree  tx.go:332-355                       build_many_dev (capi_tx.hip)
//   Eh against the header, TxHeader.Alh  :1649-1654    k_repl_alh
//   performPrecommit's aht.Append  :1921-1946          launch_ahtree_append
//   id order, BlRoot == RootAt(BlTxID), PrevAlh  :1656-1722   k_repl_verdict
//
// The frame is the one of mh_verify_verifiable_tx_pb_batch: the blobs go up
// in chunks (PbChunkFrame, ChunkCopier), groups of chunks are parsed and hashed
// as they land.  A tx's Alh depends on its own bytes only (the exported
// PrevAlh is hashed, the chain is a comparison), so every group's Alh values
// are final when the group is done; once the last group is, all n candidates
// are appended behind the P resident leaves, the verdict kernel reads
// RootAt(BlTxID) out of that dLog -- a node of the dLog covers leaves before
// it only, so a tx of the accepted prefix never reads a node that a refused tx
// contributed to -- and the tree's size is set to P + a.  Per group the host
// waits once for the scanned entry offsets (the trees' shapes) and once in
// build_many_dev, as mh_verify_verifiable_tx_pb_batch does.
#include "capi_internal.hpp"

extern "C" int mh_replicate_tx_batch(mh_ahtree *t, const mh_replicate_batch *b, int32_t *status,
                                     uint64_t *accepted, mh_tx_header *hdrs, uint8_t *md_blob,
                                     uint8_t *alh, uint64_t *ent_off, mh_replicated_entry *ents,
                                     uint64_t ents_cap, uint8_t *hvals) {
    return mh_guard([&]() -> int {
        if (!t || !b || !status || !accepted) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        *accepted = 0;
        if (n == 0) {
            if (ent_off) ent_off[0] = 0;
            return MH_OK;
        }
        std::lock_guard<std::recursive_mutex> lk_(t->mu);  // AHtree.mutex (ahtree.go:60-84)
        mh_ctx *c = t->ctx;
        PbChunkFrame F;
        if (int e = F.open(c, n, b->txs, b->tx_off, true)) return e;
        const uint64_t P = t->size;
        if (int e = aht_reserve(t, P + n)) return e;
        MH_HIP(t->ctr.ensure(256));
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        F.group();
        const uint64_t M = F.group_n;
        const ReplLimits lim{b->max_entries, b->max_key_len, b->max_value_len, b->flags};
        Layout L;
        // the blobs, the offsets and the per-tx results, whole; then one group's work
        const uint64_t b_msg = L.add(F.mb + 16), b_off = L.add((n + 1) * 8), b_stl = L.add(n * 4),
                       b_stf = L.add(n * 4), b_hdr = L.add(n * sizeof(mh_tx_header)),
                       b_md = L.add(n * (uint64_t)kMdSlot), b_alh = L.add(n * 32), b_bad = L.add(8);
        const size_t scan_bytes = pb_scan_temp_bytes(M);
        const uint64_t b_cnt = L.add(M * 8), b_eo = L.add((M + 1) * 8), b_trunc = L.add(M),
                       b_roots = L.add(M * 32), b_amsg = L.add(M * kTxInnerStride),
                       b_scan = L.add(scan_bytes);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        StreamGuard sg;  // no copy into the caller's arrays is pending on any way out
        sg.streams.push_back(st);
        ChunkCopier cc(c);
        F.fill(cc, base + b_msg, {{base + b_off, b->tx_off, (n + 1) * 8}});
        MH_HIP(cc.start());
        // a tx that does not parse leaves zeros
        MH_HIP(hipMemsetAsync(base + b_hdr, 0, n * sizeof(mh_tx_header), st));
        MH_HIP(hipMemsetAsync(base + b_md, 0, n * (uint64_t)kMdSlot, st));
        MH_HIP(hipMemsetAsync(base + b_bad, 0xff, 8, st));
        const uint8_t *dmsg = base + b_msg - F.m0;
        int32_t *d_stl = (int32_t *)(base + b_stl), *d_stf = (int32_t *)(base + b_stf);
        mh_tx_header *d_hdr = (mh_tx_header *)(base + b_hdr);
        std::vector<uint64_t> h_eo;
        uint64_t tot = 0;  // entries of the groups so far
        bool overflow = false;
        for (int g = 0; g < F.ng; g++) {
            uint64_t lo, nk;
            if (int e = F.wait_group(c, cc, g, lo, nk)) return e;
            ReplGroup G{};
            G.nk = nk;
            G.first = lo;
            G.msgs = dmsg;
            G.tx_off = (const uint64_t *)(base + b_off) + lo;
            G.status = d_stl + lo;
            G.cnt = (uint64_t *)(base + b_cnt);
            G.ent_off = (const uint64_t *)(base + b_eo);
            G.hdr = d_hdr + lo;
            G.md_blob = base + b_md;
            G.trunc = base + b_trunc;
            G.roots = base + b_roots;
            G.alh = base + b_alh + 32 * lo;
            G.alh_msg = base + b_amsg;
            // 1. the wire grammar: status, the entry counts, their offsets
            MH_HIP(launch_repl_struct(st, tm, false, G));
            MH_HIP(scan_offsets_u64(st, nk, G.cnt, (uint64_t *)(base + b_eo), base + b_scan, scan_bytes));
            h_eo.resize(nk + 1);
            MH_HIP(hipMemcpyAsync(h_eo.data(), base + b_eo, (nk + 1) * 8, hipMemcpyDeviceToHost, st));
            MH_HIP(hipStreamSynchronize(st));
            const uint64_t Tg = h_eo[nk];
            // every entry record is at least 8 bytes of its blob
            if (Tg > F.group_bytes / 8) return MH_ERR_ILLEGAL_STATE;
            if (ent_off)
                for (uint64_t k = 0; k < nk; k++) ent_off[lo + k] = tot + h_eo[k];
            if (ents && tot + Tg > ents_cap) overflow = true;
            tot += Tg;
            if (overflow) continue;  // only the count is still wanted
            Layout E;
            const uint64_t e_ent = E.add(Tg * sizeof(mh_replicated_entry)), e_dup = E.add(Tg),
                           e_dig = E.add(std::max<uint64_t>(Tg, 1) * 32), e_hv = E.add(Tg * 32);
            // (not s_tree: build_many_dev's tree plan lays its nodes out there)
            MH_HIP(c->s_ventry.ensure(E.total + 8));
            uint8_t *eb = c->s_ventry.as<uint8_t>();
            G.ents = (mh_replicated_entry *)(eb + e_ent);
            G.dup = eb + e_dup;
            G.dig = eb + e_dig;
            G.hv = eb + e_hv;
            MH_HIP(launch_repl_struct(st, tm, true, G));
            // 2. OngoingTx.set and the validations, then the hashing of what is left
            MH_HIP(launch_repl_set(st, tm, Tg, G, lim));
            // (an entry of a refused tx is hashed by no lane: its tree is built
            // over zeros and never looked at)
            if (Tg) MH_HIP(hipMemsetAsync(G.dig, 0, Tg * 32, st));
            if (Tg && hvals) MH_HIP(hipMemsetAsync(G.hv, 0, Tg * 32, st));
            MH_HIP(launch_repl_leaf(st, tm, Tg, G));
            if (ents && Tg) {
                MH_HIP(hipMemcpyAsync(ents + (tot - Tg), G.ents, Tg * sizeof(mh_replicated_entry),
                                      hipMemcpyDeviceToHost, st));
                if (hvals)
                    MH_HIP(hipMemcpyAsync(hvals + 32 * (tot - Tg), G.hv, Tg * 32, hipMemcpyDeviceToHost,
                                          st));
            }
            if (int e = build_many_dev(c, st, nk, h_eo.data(), G.dig, base + b_roots, c->s_digests,
                                       c->s_offs))
                return e;
            // 3. Eh against the exported header, the Alh
            MH_HIP(launch_repl_alh(st, tm, G, lim));
        }
        MH_HIP(cc.sync());
        if (ent_off) ent_off[n] = tot;
        if (overflow) {
            MH_HIP(hipStreamSynchronize(st));
            return MH_ERR_BUFFER_TOO_SMALL;
        }
        // 4. every candidate behind the resident leaves, the chain and linking
        // verdicts, the accepted prefix
        MH_HIP(launch_ahtree_append(st, tm, t->dlog.as<uint8_t>(), P, base + b_alh, n, 32, nullptr,
                                    t->ctr.as<uint32_t>()));
        ReplPrev prev;
        memcpy(prev.alh, b->prev_alh, 32);
        unsigned long long *d_bad = (unsigned long long *)(base + b_bad);
        MH_HIP(launch_repl_verdict(st, tm, n, d_stl, d_hdr, base + b_alh, t->dlog.as<uint8_t>(), P, prev,
                                   d_stf, d_bad));
        unsigned long long bad = 0;
        MH_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, d_stf, n * 4, hipMemcpyDeviceToHost, st));
        if (hdrs) MH_HIP(hipMemcpyAsync(hdrs, d_hdr, n * sizeof(mh_tx_header), hipMemcpyDeviceToHost, st));
        if (md_blob)
            MH_HIP(hipMemcpyAsync(md_blob, base + b_md, n * (uint64_t)kMdSlot, hipMemcpyDeviceToHost, st));
        if (alh) MH_HIP(hipMemcpyAsync(alh, base + b_alh, n * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        const uint64_t a = std::min<uint64_t>(bad, n);
        *accepted = a;
        if (!(b->flags & MH_REPL_DRY_RUN)) t->size = P + a;
        return MH_OK;
    });
}
