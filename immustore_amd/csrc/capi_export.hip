// capi_export.hip -- C ABI of the leader's side of replication: what
// ImmuStore.ExportTx (immustore.go:2621-2770) returns for a run of consecutive
// txs of a store whose tx log, commit log and value logs are resident, in one
// device pass (the follower's side is capi_repl.hip).
//
//   the store: its arguments, where it lies                 store_args_ok, store_resident (capi_txlog.hip)
//   readTx with the integrity check  :2622, tx.go:388-630   mh_txlog_validate_clog's core
//   the entries of the valid txs                            k_exp_scan, k_txe_index
//   decodeOffset, readValueAt's io.EOF  :1429, :3183-3218   k_exp_entry (export_kernels.hip)
//   "partially truncated"  :2703, :2726; the sizes          k_exp_tx, k_exp_scan
//   hdr, keys, metadata, hVal of truncated txs, trailer     k_exp_head, k_exp_ent
//   SHA-256(value) against hVal  :3235, the value bytes     k_exp_values (/ k_exp_copy): value_lane (value_store.hpp)
//   the statuses in Go's order                              k_exp_status
//
// The host waits inside the read path, for the number of entries (scratch) and,
// when out is host memory, for the offsets (the staging's size); only off,
// status, truncated and -- when out is host memory -- the blobs that fit come
// back.
#include <cstdlib>

#include "capi_internal.hpp"

namespace {

// MH_EXPORT_ARM=A|B picks the value kernels of a call (tools/bench_export.py
// times both); the default is the faster one of profiles/export_bench.md
char export_arm() {
    const char *e = getenv("MH_EXPORT_ARM");
    return e && (e[0] == 'A' || e[0] == 'B') ? e[0] : 'A';
}

}  // namespace

extern "C" int mh_export_tx_batch(mh_ctx *c, const mh_export_store *s, uint64_t first_tx,
                                  uint64_t count, uint8_t *out, uint64_t out_cap, uint64_t *off,
                                  int32_t *status, uint8_t *truncated) {
    return mh_guard([&]() -> int {
        if (count == 0) {
            if (off) off[0] = 0;
            return MH_OK;
        }
        // ---- the arguments alone
        if (!c || !s || !off || !status || (!out && out_cap)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (first_tx == 0 || count > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // (count / 4 workgroups a launch)
        const mh_answer_store cs = store_prefix(*s);
        const uint64_t N = s->ntx, es = s->clog_entry_size;
        if (!store_args_ok(cs, s->vlogs, s->nvlogs)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (count > N || first_tx > N - count + 1) return MH_ERR_TX_NOT_FOUND;  // immustore.go:3000
        // ---- where the store lies (N > 0 here)
        const int dev = c->device;
        if (!store_resident(cs, s->vlogs, s->nvlogs, dev)) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk_(c->mu);  // txlog_validate_clog_core requires it
        MH_HIP(hipSetDevice(dev));
        const bool out_dev = out_cap && on_device(out, dev);
        if (out_dev && !dev_range(out, out_cap)) return MH_ERR_ILLEGAL_ARGUMENTS;
        hipStream_t st = c->stream;
        Timer *tm = c->tm();
        StreamGuard guard{{st}};  // no copy from or into the caller's arrays is pending on any way out

        // ---- the txs of the run re-hashed: headers with the rebuilt Eh, verdicts
        const uint64_t n = count, nv = std::max<uint32_t>(s->nvlogs, 1);
        Layout L;
        const uint64_t b_hd = L.add(n * sizeof(mh_tx_header)), b_alh = L.add(n * 32), b_rst = L.add(n * 4),
                       b_ec = L.add(n * 8), b_es = L.add(n * 8), b_lo = L.add((n + 1) * 8),
                       b_md = L.add(n * (uint64_t)kMdSlot), b_mdl = L.add(n * 4), b_ei = L.add(n * 4),
                       b_est = L.add(n * 4), b_vb = L.add(n * 4), b_tr = L.add(n), b_sz = L.add(n * 8),
                       b_off = L.add((n + 1) * 8), b_st = L.add(n * 4), b_to = L.add(n),
                       b_vl = L.add(nv * sizeof(ExpVlog));
        MH_HIP(c->s_exp.ensure(L.total));
        uint8_t *base = c->s_exp.as<uint8_t>();
        auto U = [&](uint64_t o) { return (uint64_t *)(base + o); };
        ExpArrays a{};
        a.n = n;
        a.txlog = s->txlog, a.clog = s->clog + (first_tx - 1) * es;
        a.es = (uint32_t)es, a.nvlogs = s->nvlogs;
        a.vlogs = (const ExpVlog *)(base + b_vl);
        a.hd = (const MhTxHeader *)(base + b_hd), a.rst = (const int32_t *)(base + b_rst);
        a.ecnt = U(b_ec), a.ent_start = U(b_es), a.leaf_off = U(b_lo);
        a.md = base + b_md, a.mdl = (uint32_t *)(base + b_mdl);
        a.early_idx = (uint32_t *)(base + b_ei), a.early_st = (int32_t *)(base + b_est);
        a.vbad = (uint32_t *)(base + b_vb), a.trunc = base + b_tr;
        a.size = U(b_sz), a.off = U(b_off), a.status = (int32_t *)(base + b_st), a.trunc_out = base + b_to;
        static_assert(sizeof(ExpVlog) == sizeof(mh_export_vlog), "the vLog table goes up as it is");
        if (int e = txlog_validate_clog_core(c, s->txlog, s->txlog_len, a.clog, n, (uint32_t)es,
                                             s->max_entries, s->max_key_len, (mh_tx_header *)(base + b_hd),
                                             base + b_alh, (int32_t *)(base + b_rst), nullptr, nullptr))
            return e;

        // (the read path is done with the pinned staging: the vLog table goes up
        // through it, off / status / truncated come down through it)
        const uint64_t p_vl = 0, p_off = p_vl + nv * sizeof(ExpVlog), p_st = p_off + (n + 1) * 8,
                       p_tr = p_st + n * 4;
        MH_HIP(c->p_stage.ensure(p_tr + n));
        uint8_t *pin = c->p_stage.as<uint8_t>();
        if (s->nvlogs) {
            memcpy(pin + p_vl, s->vlogs, s->nvlogs * sizeof(ExpVlog));
            MH_HIP(hipMemcpyAsync(base + b_vl, pin + p_vl, s->nvlogs * sizeof(ExpVlog), hipMemcpyHostToDevice, st));
        }

        // ---- the entries of the valid txs
        MH_HIP(launch_exp_counts(st, tm, a));
        MH_HIP(c->p_small.ensure(64));
        volatile uint64_t *hw = c->p_small.as<volatile uint64_t>();
        MH_HIP(hipMemcpyAsync((void *)hw, a.leaf_off + n, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));  // wait 1: the entries
        const uint64_t E = a.E = hw[0], E1 = std::max<uint64_t>(E, 1);
        if (E > 0x7fffffffull) return MH_ERR_ILLEGAL_STATE;  // (E / 4 workgroups a launch; the order is 32-bit)
        Layout X;
        const uint64_t e_ro = X.add(E1 * 8), e_ver = X.add(E1), e_cls = X.add(E1), e_sz = X.add(E1 * 8),
                       e_pos = X.add(E1 * 8), e_src = X.add(E1 * 8), e_vl = X.add(E1 * 8),
                       e_skip = X.add(E1), e_sort = X.add(sha_varlen_scratch_bytes(E1));
        MH_HIP(c->s_exp_ent.ensure(X.total));
        uint8_t *xb = c->s_exp_ent.as<uint8_t>();
        a.rec_off = (uint64_t *)(xb + e_ro), a.ver = xb + e_ver, a.cls = xb + e_cls;
        a.esz = (uint64_t *)(xb + e_sz), a.epos = (uint64_t *)(xb + e_pos);
        a.vsrc = (const uint8_t **)(xb + e_src), a.vlen = (uint64_t *)(xb + e_vl);
        a.skip = xb + e_skip;
        if (E) {
            MH_HIP(launch_txe_index(st, tm, n, s->txlog, a.hd, a.ent_start, a.leaf_off, a.rec_off, a.ver));
            MH_HIP(launch_exp_entries(st, tm, a));
        }
        // ---- the class rule, the sizes: off is complete whatever out_cap is
        MH_HIP(launch_exp_sizes(st, tm, a));
        MH_HIP(hipMemcpyAsync(pin + p_off, a.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        uint64_t fit = 0;  // the blobs that fit are a prefix of the run's bytes
        if (!out_dev) {
            // out in host memory: the blobs are staged on the device, and the
            // staging is sized by what fits (out in device memory needs neither:
            // the kernels compare off with out_cap themselves, nothing waits)
            MH_HIP(hipStreamSynchronize(st));  // wait 2: the sizes
            fit = fit_prefix((const uint64_t *)(pin + p_off), n, out_cap);
            MH_HIP(c->s_exp_out.ensure(fit + 64));
        }

        // ---- write: the frames, then the values hashed (and copied)
        a.out = out_dev ? out : c->s_exp_out.as<uint8_t>();
        a.out_cap = out_cap;
        MH_HIP(launch_exp_frame(st, tm, a));
        if (E) {
            hipError_t se;
            const uint32_t *perm = sha_varlen_order(st, tm, a.vlen, a.skip, E, xb + e_sort, &se);
            MH_HIP(se);
            MH_HIP(launch_exp_values(st, tm, a, perm, export_arm()));
        }
        MH_HIP(launch_exp_status(st, tm, a));
        if (!out_dev && fit) MH_HIP(hipMemcpyAsync(out, a.out, fit, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(pin + p_st, a.status, n * 4, hipMemcpyDeviceToHost, st));
        if (truncated) MH_HIP(hipMemcpyAsync(pin + p_tr, a.trunc_out, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        guard.streams.clear();
        memcpy(off, pin + p_off, (n + 1) * 8);
        memcpy(status, pin + p_st, n * 4);
        if (truncated) memcpy(truncated, pin + p_tr, n);
        return MH_OK;
    });
}
