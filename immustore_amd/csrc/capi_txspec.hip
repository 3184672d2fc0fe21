// capi_txspec.hip -- C ABI of the server's tx reads under an EntriesSpec: the
// schema.Tx of db.TxByID (database.go:1034-1063) and of every item of
// db.TxScan's TxList (:1531-1583), and the schema.VerifiableTx of
// db.VerifiableTxByID (:1462-1528), with db.serializeTx (:1080-1231) and
// ImmuStore.ReadValue (immustore.go:3149-3240) run on the device.
//
//   the store: its arguments, where it lies              store_args_ok, store_resident (capi_txlog.hip)
//   the reads of a request, every distinct tx once,      AnsRead, the answer path's read-set
//     ReadTx's re-hash, verdicts, links                  stage (capi_answer.hip's list)
//   entry index                                          k_txe_index
//   variants and groups of the batch                     the host, from the requests alone
//   serializeTx's switch, ReadValue up to the read       k_txs_plan (txspec_kernels.hip)
//   DualProof sizes and statuses                         k_pb_dual1_size over the RankWindow
//   sizes, one scan                                      k_txs_vsize, k_txs_size
//   schema.Tx once per variant                           k_txs_header, k_txs_entries
//   SHA-256(value) against hVal, the value bytes         k_txs_values (/ k_txs_copy): value_lane (value_store.hpp)
//   the answers, the DualProofs, the statuses            k_txs_assemble, k_pb_dual1_write, k_txs_status
//
// The host waits for the number of distinct txs, inside the read path, for the
// entries of the asked txs, for the items of the variants (scratch) and for the
// offsets (what fits); only off, status and -- when out is host memory -- the
// answers come back.
#include <algorithm>
#include <numeric>
#include <vector>

#include "capi_internal.hpp"

namespace {

// req.EntriesSpec's three actions as a variant's mode; false: outside the enum
bool txs_mode(const mh_tx_answer_batch *b, uint64_t p, uint8_t *mode, bool *resolve) {
    if (!b->has_spec[p]) {
        *mode = kTxsNoSpec;
        return true;
    }
    uint32_t m = 0;
    const uint8_t act[3] = {b->kv_action[p], b->z_action[p], b->sql_action[p]};
    for (int k = 0; k < 3; k++) {
        const uint32_t x = act[k] == MH_TXA_NO_SPEC ? 0u : act[k];  // a nil spec excludes
        if (x > 3) return false;
        if (x == 3 && k < 2) *resolve = true;
        m |= x << (2 * k);
    }
    *mode = (uint8_t)m;
    return true;
}

// the classes a mode reads (RAW_VALUE): bit 0 kv, 1 z, 2 sql
uint32_t txs_reads(uint8_t mode) {
    if (mode == kTxsNoSpec) return 0;
    return ((mode & 3) == 2) | (((mode >> 2) & 3) == 2) << 1 | (((mode >> 4) & 3) == 2) << 2;
}

}  // namespace

extern "C" int mh_tx_answer_pb_batch(mh_ctx *c, mh_ahtree *t, const mh_export_store *s,
                                     const mh_tx_answer_batch *b, uint8_t *out, uint64_t out_cap,
                                     uint64_t *off, int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c || !s || !b) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = b->n;
        if (n == 0) {
            if (off) off[0] = 0;
            return MH_OK;
        }
        // ---- the arguments alone
        if (!off || !status || (!out && out_cap) || !b->kind || !b->tx || !b->prove_since ||
            !b->has_spec || !b->kv_action || !b->z_action || !b->sql_action)
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        const mh_answer_store cs = store_prefix(*s);
        const uint64_t N = s->ntx;
        if (!store_args_ok(cs, s->vlogs, s->nvlogs)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (N >= (1ull << 36)) return MH_ERR_ILLEGAL_ARGUMENTS;  // the bitmap's words are scanned as ints
        if (t && t->ctx != c) return MH_ERR_ILLEGAL_ARGUMENTS;
        // ---- the requests: variants (tx, actions) and groups (tx, classes read)
        std::vector<uint8_t> mode(n);
        std::vector<uint64_t> since(n);
        bool resolve = false;
        for (uint64_t p = 0; p < n; p++) {
            if (b->kind[p] != MH_TXA_TX && b->kind[p] != MH_TXA_VERIFIABLE) return MH_ERR_ILLEGAL_ARGUMENTS;
            if (b->kind[p] == MH_TXA_VERIFIABLE && !t) return MH_ERR_ILLEGAL_ARGUMENTS;
            if (!txs_mode(b, p, &mode[p], &resolve)) return MH_ERR_ILLEGAL_ARGUMENTS;
            since[p] = b->kind[p] == MH_TXA_VERIFIABLE ? b->prove_since[p] : 0;
        }
        if (resolve) return MH_ERR_ILLEGAL_ARGUMENTS;  // kv / z RESOLVE needs the index: not covered
        std::vector<uint32_t> order(n), rv(n);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            if (b->tx[x] != b->tx[y]) return b->tx[x] < b->tx[y];
            if (mode[x] != mode[y]) return mode[x] < mode[y];
            return x < y;
        });
        std::vector<uint64_t> vtx;
        std::vector<uint8_t> vmode, vprim;
        std::vector<uint32_t> vgroup, vfirst, vcnt;
        uint32_t G = 0;
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t p = order[k];
            if (!k || b->tx[p] != vtx.back() || mode[p] != vmode.back()) {
                // (the variants of a tx are neighbours: its groups are looked up among them)
                uint32_t g = G;
                for (uint64_t u = vtx.size(); u-- > 0 && vtx[u] == b->tx[p];)
                    if (txs_reads(vmode[u]) == txs_reads(mode[p])) g = vgroup[u];
                vprim.push_back(g == G);
                if (g == G) G++;
                vtx.push_back(b->tx[p]);
                vmode.push_back(mode[p]);
                vgroup.push_back(g);
                vfirst.push_back(p);
                vcnt.push_back(0);
            }
            vcnt.back()++;
            rv[p] = (uint32_t)(vtx.size() - 1);
        }
        const uint64_t V = vtx.size();
        // ---- where the store lies
        std::unique_lock<std::recursive_mutex> lkt_;
        if (t) lkt_ = std::unique_lock<std::recursive_mutex>(t->mu);  // the tree's lock, then its context's
        std::lock_guard<std::mutex> lkc_(c->mu);
        const int dev = c->device;
        MH_HIP(hipSetDevice(dev));
        if (!store_resident(cs, s->vlogs, s->nvlogs, dev)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const bool out_dev = out_cap && on_device(out, dev);
        if (out_dev && !dev_range(out, out_cap)) return MH_ERR_ILLEGAL_ARGUMENTS;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        StreamGuard guard{{st}};  // no copy from or into the caller's arrays is pending on any way out

        // ---- requests up, the read set (the answer path's, every kind its MH_ANS_TX)
        AnsArrays a{};
        TxsArrays x{};
        AnsRead r{c, cs, a};
        x.V = V, x.nvlogs = s->nvlogs, x.now = b->now_unix;
        const uint64_t nv = std::max<uint32_t>(s->nvlogs, 1);
        Layout L;
        const uint64_t b_zoff = L.add((n + 1) * 8), b_xk = L.add(n), b_rv = L.add(n * 4),
                       b_wst = L.add(n * 4), b_vl = L.add(nv * sizeof(ExpVlog));
        if (int e = r.requests(n, L)) return e;
        uint8_t *base = r.base;
        auto U = [&](uint64_t o) { return (uint64_t *)(base + o); };
        auto h2d = [&](uint8_t *dst, const void *p, uint64_t bytes) -> hipError_t {
            return bytes ? hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
        };
        MH_HIP(hipMemsetAsync(base + r.b_kind, 0, n, st));  // MH_ANS_TX
        MH_HIP(hipMemsetAsync(base + b_zoff, 0, (n + 1) * 8, st));
        MH_HIP(hipMemsetAsync(base + r.b_dpo, 0, (n + 1) * 8, st));
        MH_HIP(hipMemsetAsync(base + r.b_dst, 0, n * 4, st));
        MH_HIP(h2d(base + r.b_tx, b->tx, n * 8));
        MH_HIP(h2d(base + r.b_since, since.data(), n * 8));
        MH_HIP(h2d(base + b_xk, b->kind, n));
        MH_HIP(h2d(base + b_rv, rv.data(), n * 4));
        static_assert(sizeof(ExpVlog) == sizeof(mh_export_vlog), "the vLog table goes up as it is");
        MH_HIP(h2d(base + b_vl, s->vlogs, s->nvlogs * sizeof(ExpVlog)));
        a.key_off = a.entry_off = U(b_zoff);
        a.keys = a.entries = base;
        x.kind = base + b_xk, x.rv = (const uint32_t *)(base + b_rv), x.wst = (int32_t *)(base + b_wst);
        x.vlogs = (const ExpVlog *)(base + b_vl);
        if (int e = r.heads()) return e;  // wait 1: the distinct txs read
        const uint64_t D = a.D;

        // ---- every distinct tx read and re-hashed once
        Layout S;
        if (int e = r.reads(S)) return e;
        volatile uint64_t *hw = r.hw;

        // ---- the variants: their slots, their items
        const size_t vscan_bytes = pb_scan_temp_bytes(V);
        Layout Y;
        const uint64_t v_tx = Y.add(V * 8), v_mode = Y.add(V), v_prim = Y.add(V), v_grp = Y.add(V * 4),
                       v_first = Y.add(V * 4), v_cnt = Y.add(V * 4), v_slot = Y.add(V * 8),
                       v_w = Y.add(V * 8), v_io = Y.add((V + 1) * 8), v_ei = Y.add(V * 4),
                       v_est = Y.add(V * 4), v_body = Y.add(V * 8), v_hsz = Y.add(V * 4),
                       v_share = Y.add(V * 8), v_pos = Y.add((V + 1) * 8), v_dst = Y.add(V * 8),
                       v_gbad = Y.add((uint64_t)G * 4), v_scan = Y.add(vscan_bytes);
        MH_HIP(c->s_txs.ensure(Y.total));
        uint8_t *yb = c->s_txs.as<uint8_t>();
        MH_HIP(h2d(yb + v_tx, vtx.data(), V * 8));
        MH_HIP(h2d(yb + v_mode, vmode.data(), V));
        MH_HIP(h2d(yb + v_prim, vprim.data(), V));
        MH_HIP(h2d(yb + v_grp, vgroup.data(), V * 4));
        MH_HIP(h2d(yb + v_first, vfirst.data(), V * 4));
        MH_HIP(h2d(yb + v_cnt, vcnt.data(), V * 4));
        MH_HIP(hipMemsetAsync(yb + v_gbad, 0xff, (uint64_t)G * 4, st));  // kExpNone
        x.vtx = (const uint64_t *)(yb + v_tx), x.vmode = yb + v_mode, x.vprim = yb + v_prim;
        x.vgroup = (const uint32_t *)(yb + v_grp), x.vfirst = (const uint32_t *)(yb + v_first);
        x.vcnt = (const uint32_t *)(yb + v_cnt);
        x.vslot = (uint64_t *)(yb + v_slot), x.vw = (uint64_t *)(yb + v_w);
        x.item_off = (uint64_t *)(yb + v_io), x.early_idx = (uint32_t *)(yb + v_ei);
        x.early_st = (int32_t *)(yb + v_est), x.vbody = (uint64_t *)(yb + v_body);
        x.vhsz = (uint32_t *)(yb + v_hsz), x.vshare = (uint64_t *)(yb + v_share);
        x.vpos = (uint64_t *)(yb + v_pos), x.vdst = (uint8_t **)(yb + v_dst);
        x.gbad = (uint32_t *)(yb + v_gbad);
        MH_HIP(launch_txs_variants(st, tm, a, x));
        MH_HIP(scan_offsets_u64(st, V, x.vw, x.item_off, yb + v_scan, vscan_bytes));
        MH_HIP(hipMemcpyAsync((void *)hw, a.leaf_off + D, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync((void *)(hw + 1), x.item_off + V, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 2: the entries of the asked txs, the items
        const uint64_t E = a.E = D ? hw[0] : 0, E1 = std::max<uint64_t>(E, 1);
        const uint64_t I = x.I = E ? hw[1] : 0, I1 = std::max<uint64_t>(I, 1);
        if (E > 0x7fffffffull || I > 0x7fffffffull) return MH_ERR_ILLEGAL_STATE;  // hipcub's int item count

        // ---- the entries of the asked txs, the items under their actions
        Layout X;
        const uint64_t e_ro = X.add(E1 * 8), e_ver = X.add(E1), i_kind = X.add(I1), i_fail = X.add(I1),
                       i_sz = X.add(I1 * 8), i_pos = X.add(I1 * 8), i_src = X.add(I1 * 8),
                       i_vl = X.add(I1 * 8), i_skip = X.add(I1), i_sort = X.add(sha_varlen_scratch_bytes(I1));
        MH_HIP(c->s_ans_ent.ensure(X.total));
        uint8_t *xb = c->s_ans_ent.as<uint8_t>();
        a.rec_off = (uint64_t *)(xb + e_ro), a.ver = xb + e_ver;
        x.ikind = xb + i_kind, x.ifail = xb + i_fail;
        x.isz = (uint64_t *)(xb + i_sz), x.ipos = (uint64_t *)(xb + i_pos);
        x.vsrc = (const uint8_t **)(xb + i_src), x.vlen = (uint64_t *)(xb + i_vl), x.skip = xb + i_skip;
        if (E) MH_HIP(launch_txe_index(st, tm, D, s->txlog, a.hd, a.ent_start, a.leaf_off, a.rec_off, a.ver));
        MH_HIP(launch_txs_plan(st, tm, a, x));
        MH_HIP(scan_offsets_u64(st, V, x.vshare, x.vpos, yb + v_scan, vscan_bytes));

        // ---- DualProof(src, tgt) of the VERIFIABLE requests: statuses and lengths; the sizes
        RankWindow win{a.bits, a.rank, a.rst, a.lnk, N, a.dpos};
        if (t)
            MH_HIP(launch_pb_dual_v1_ranked(st, tm, 1, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                            s->txlog, win, a.alh, a.inner, nullptr, U(r.b_dpo),
                                            (int32_t *)(base + r.b_dst), base + r.b_dps));
        MH_HIP(launch_txs_size(st, tm, a, x));
        MH_HIP(scan_offsets_u64(st, n, a.sizes, U(r.b_off), r.scan, r.scan_bytes));
        MH_HIP(hipMemcpyAsync(off, a.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync((void *)hw, x.vpos + V, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 3: the sizes
        const uint64_t shared_bytes = hw[0], fit = fit_prefix(off, n, out_cap);

        // ---- write: schema.Tx once per variant, the values hashed and stored, the answers
        Layout O;
        const uint64_t o_tx = O.add(shared_bytes + 16), o_out = O.add((out_dev ? 0 : fit) + 64);
        MH_HIP(c->s_ans_out.ensure(O.total));
        uint8_t *ob = c->s_ans_out.as<uint8_t>();
        x.txbuf = ob + o_tx;
        a.out = out_dev ? out : ob + o_out, a.out_cap = fit;
        MH_HIP(launch_txs_write(st, tm, a, x));
        if (I) {
            hipError_t se;
            const uint32_t *perm = sha_varlen_order(st, tm, x.vlen, x.skip, I, xb + i_sort, &se);
            MH_HIP(se);
            MH_HIP(launch_txs_values(st, tm, a, x, perm));
        }
        MH_HIP(launch_txs_assemble(st, tm, a, x));
        if (t)
            MH_HIP(launch_pb_dual_v1_ranked(st, tm, 2, t->dlog.as<uint8_t>(), t->size, n, a.hs, a.ht,
                                            s->txlog, win, a.alh, a.inner, a.out, U(r.b_dpo), x.wst,
                                            base + r.b_dps));
        MH_HIP(launch_txs_status(st, tm, a, x));
        if (!out_dev && fit) MH_HIP(hipMemcpyAsync(out, a.out, fit, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, a.status, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        guard.streams.clear();
        return MH_OK;
    });
}
