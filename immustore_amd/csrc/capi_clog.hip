// capi_clog.hip -- a14 over a tx log indexed by its commit log
// (txOffsetAndSize, immustore.go:2569-2597): no host hop.  The structure pass
// (txlog_struct.hip) parses every record where its cLog entry points, with
// every check of the host hop; the lane kernel hashes the accepted ones (entry
// digests, htree, innerHash, Alh vs the stored Alh); a record whose metadata
// is valid but not canonical (Go hashes the re-serialised form), that is wider
// than the lane kernel takes, or whose read runs past the bytes landed when
// its group ran is re-validated by mh_txlog_validate's body on a host copy of
// that record alone (host_fallback).
//  * log in device memory: one group, no copy;
//  * log in host memory (pinned: the cgo shim's arena): copied up in chunks
//    (5 : 2 : 1 from 16 MiB, as mh_txlog_validate), each chunk's records --
//    those whose cLog entry ends inside it, when the entries are in log order
//    -- checked as soon as it lands, under the copy of the rest; the lane
//    kernel takes its entries per lane from the structure pass's widest
//    record on the device (launch shape from the cLog sizes), so nothing
//    waits on the host between the chunks.
#include "capi_internal.hpp"

namespace {

// What the helpers of one cLog call share; mh_txlog_validate_clog fills it.
// stats (device): [0] a lane launch whose shape was too narrow for its records
// (the resident form launches on the previous call's widest record without
// waiting for this one's: a wider log goes again), [2] failed records, [3] the
// first of them; from stats[4] two words per group: its widest accepted record
// and its records for the host.  hs: their pinned copies (stats at hs[0, 4),
// the groups' from hs[8]).
struct ClogState {
    mh_ctx *c;
    hipStream_t st;
    const uint8_t *dlog, *clog;
    uint64_t len, ntx;
    uint32_t es;  // bytes per cLog entry: 12, or 44 with the Alh
    HopLimits lim;
    TxlogOutputs out;
    TxlogOutputs::Dst dst;  // where the kernels store the outputs themselves
    bool log_dev = false, clog_dev = false;
    uint64_t *ro = nullptr, *stats = nullptr;
    int32_t *pre = nullptr, *sts = nullptr;
    uint8_t *alh = nullptr;
    MhTxHeader *hd = nullptr;  // staged headers (null: stored by the kernel, or not asked for)
    volatile uint64_t *hs = nullptr;
    // the host's view of the cLog entries (for the groups and the launch
    // shapes of a host log, and for the host fallback)
    std::vector<uint8_t> hcl_copy;
    const uint8_t *hcl = nullptr;
    hipError_t fetch_clog() {  // a device cLog, down on st (not waited for)
        hcl_copy.resize(ntx * es);
        hcl = hcl_copy.data();
        return hipMemcpyAsync(hcl_copy.data(), clog, ntx * es, hipMemcpyDeviceToHost, st);
    }

    // The status summary goes in two halves around the launches it counts:
    // reset_stats clears stats[w0, w0 + nwords) and the "first failed" word,
    // results_down summarises the statuses, fetches stats[w0, 4) (and the stats of
    // ngstats groups) and copies down the outputs the kernels could not store.
    int reset_stats(uint64_t w0, uint64_t nwords) const {
        MH_HIP(hipMemsetAsync(stats + w0, 0, nwords * 8, st));
        MH_HIP(hipMemsetAsync(stats + 3, 0xff, 8, st));
        return MH_OK;
    }
    int results_down(uint64_t w0, size_t ngstats) const {
        MH_HIP(launch_txlog_status_summary(st, ntx, sts, stats));
        MH_HIP(hipMemcpyAsync((void *)(hs + w0), stats + w0, (4 - w0) * 8, hipMemcpyDeviceToHost, st));
        if (ngstats) MH_HIP(hipMemcpyAsync((void *)(hs + 8), stats + 4, 2 * ngstats * 8, hipMemcpyDeviceToHost, st));
        return out.copy_down(st, 0, ntx, dst, sts, alh, hd);
    }

    // records for the host hop (rare: a log not written by immudb, or a record
    // that disagrees with its cLog entry): the kTxlNeedsHost records gathered,
    // each re-validated by mh_txlog_validate's body, the results written back
    int host_fallback() {
        struct Fix {
            uint64_t t;
            int32_t st;
            mh_tx_header h;
            uint8_t alh[32];
        };
        std::vector<Fix> fix;
        std::vector<int32_t> hpre(ntx);
        std::vector<uint64_t> hro(ntx);
        if (clog_dev && hcl_copy.empty()) MH_HIP(fetch_clog());
        MH_HIP(hipMemcpyAsync(hpre.data(), pre, ntx * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(hro.data(), ro, ntx * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        std::vector<uint8_t> rb;
        for (uint64_t t = 0; t < ntx; t++) {
            if (hpre[t] != kTxlNeedsHost) continue;
            const uint64_t off = hro[t], size = be_at(hcl + t * es + 8, 4);
            Fix f{};
            f.t = t;
            int32_t one = 0;
            // the record within its cLog size first (valid records end
            // there); a read past it needs the rest of the log (readTx reads
            // on), for the reader's own verdict
            uint64_t n = 0, used = 0, span = off < len ? std::min(size, len - off) : 0;
            int rc = off >= len || len - off < 8 ? MH_ERR_TRUNCATED : MH_OK;  // the reader's EOF
            for (int pass = 0; pass < 2 && rc == MH_OK; pass++) {
                const uint8_t *src = dlog + off;
                if (log_dev) {
                    rb.resize(span);
                    MH_HIP(hipMemcpy(rb.data(), dlog + off, span, hipMemcpyDeviceToHost));
                    src = rb.data();
                }
                n = used = 0;
                memset(&f.h, 0, sizeof f.h);
                rc = txlog_validate_core(c, src, nullptr, span, lim, 1, &n, &used,
                                         TxlogOutputs{&one, f.alh, &f.h}, nullptr);
                if (rc < 0) return rc;
                if ((rc != MH_ERR_TRUNCATED && (rc != MH_OK || n == 1)) || span == len - off) break;
                span = len - off;
                rc = MH_OK;
            }
            int s1 = rc != MH_OK ? rc : n != 1 ? MH_ERR_TRUNCATED : used != size ? MH_ERR_CORRUPTED_DATA : MH_OK;
            if (s1 == MH_OK && es == 44) {
                uint8_t a[32];
                if (log_dev)
                    MH_HIP(hipMemcpy(a, dlog + off + size - 32, 32, hipMemcpyDeviceToHost));
                else
                    memcpy(a, dlog + off + size - 32, 32);
                if (memcmp(hcl + t * es + 12, a, 32)) s1 = MH_ERR_CORRUPTED_DATA;
            }
            if (s1 != MH_OK) {
                memset(&f.h, 0, sizeof f.h);
                memset(f.alh, 0, 32);
            }
            f.st = s1 != MH_OK ? s1 : one;
            if (f.h.version) f.h.md_off += (uint32_t)off;  // relative to the log, as the kernel's
            fix.push_back(f);
        }
        MH_HIP(c->p_stage.ensure(fix.size() * sizeof(Fix)));
        Fix *pf = c->p_stage.as<Fix>();
        for (size_t k = 0; k < fix.size(); k++) pf[k] = fix[k];
        for (size_t k = 0; k < fix.size(); k++) {  // into the device arrays the summary reads
            const uint64_t t = pf[k].t;
            MH_HIP(hipMemcpyAsync(sts + t, &pf[k].st, 4, hipMemcpyHostToDevice, st));
            MH_HIP(hipMemcpyAsync(alh + t * 32, pf[k].alh, 32, hipMemcpyHostToDevice, st));
            if (hd) MH_HIP(hipMemcpyAsync(hd + t, &pf[k].h, sizeof(mh_tx_header), hipMemcpyHostToDevice, st));
            // device outputs get theirs here, host outputs after the sync
            if (int e = out.put_device(st, dst, t, &pf[k].st, pf[k].alh, &pf[k].h)) return e;
        }
        if (int e = reset_stats(2, 1)) return e;
        if (int e = results_down(2, 0)) return e;
        MH_HIP(hipStreamSynchronize(st));
        for (size_t k = 0; k < fix.size(); k++)  // host outputs (pinned: the kernel wrote zeros)
            out.put_host(dst, pf[k].t, pf[k].st, pf[k].alh, pf[k].h);
        return MH_OK;
    }
};

// The groups of a host log, one per copy chunk when the cLog entries are in
// log order, else one.  Group g: records [tg[g], tg[g + 1]), read within the
// first lim[g] bytes, no record wider than bound[g].
void clog_groups(const ClogState &s, const std::vector<uint64_t> &cut, std::vector<uint64_t> &tg,
                 std::vector<uint64_t> &lim, std::vector<uint64_t> &bound) {
    const uint64_t nck = cut.size() - 1;
    // the widest record a cLog size allows: header + Alh >= 124 bytes,
    // an entry >= 48 (2 + 2 + 4 + 8 + 32)
    auto wbound = [&](uint64_t t) -> uint64_t {
        const uint64_t sz = be_at(s.hcl + t * s.es + 8, 4);
        return std::min<uint64_t>(kTxlLanesMaxEntries, sz >= 124 ? (sz - 124) / 48 : 0);
    };
    bool ordered = true;
    uint64_t prev_end = 0;
    std::vector<uint64_t> end(s.ntx);
    for (uint64_t t = 0; t < s.ntx; t++) {
        const uint64_t off = be_at(s.hcl + t * s.es, 8), sz = be_at(s.hcl + t * s.es + 8, 4);
        end[t] = off + sz < off ? ~0ull : off + sz;
        ordered &= end[t] >= prev_end;
        prev_end = end[t];
    }
    if (ordered && nck > 1) {
        tg.assign(nck + 1, 0);
        lim.assign(nck, s.len);
        for (uint64_t k = 1; k < nck; k++) {
            tg[k] = (uint64_t)(std::upper_bound(end.begin(), end.end(), cut[k]) - end.begin());
            lim[k - 1] = cut[k];
        }
        tg[nck] = s.ntx;
    }
    bound.assign(tg.size() - 1, 1);
    for (size_t g = 0; g + 1 < tg.size(); g++)
        for (uint64_t t = tg[g]; t < tg[g + 1]; t++) bound[g] = std::max(bound[g], wbound(t));
}

}  // namespace

// mh_txlog_validate_clog's body; c->mu MUST be held by the caller (the public
// call takes it; mh_verifiable_answer_pb_batch holds it for its whole pass).
int txlog_validate_clog_core(mh_ctx *c, const uint8_t *dlog, uint64_t len, const uint8_t *clog,
                             uint64_t ntx, uint32_t clog_entry_size, uint32_t max_entries,
                             uint32_t max_key_len, mh_tx_header *hdrs_out, uint8_t *alh_out,
                             int32_t *status_out, uint64_t *nbad_out, uint64_t *first_bad_out) {
    {
        const uint32_t es = clog_entry_size;
        if (!c || (es != 12 && es != 44) || (ntx && (!dlog || !clog))) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (nbad_out) *nbad_out = 0;
        if (first_bad_out) *first_bad_out = ntx;
        if (!ntx) return MH_OK;
        if (ntx > (1ull << 40)) return MH_ERR_ILLEGAL_ARGUMENTS;
        hipSetDevice(c->device);
        MH_HIP(c->copy_lane());
        hipStream_t st = c->stream;
        ClogState s{c, st, dlog, clog, len, ntx, es, HopLimits{max_entries, max_key_len},
                    TxlogOutputs{status_out, alh_out, hdrs_out}};
        auto is_dev = [](const void *q) {
            hipPointerAttribute_t a;
            const bool d = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeDevice;
            (void)hipGetLastError();
            return d;
        };
        const bool log_dev = s.log_dev = is_dev(dlog), clog_dev = s.clog_dev = is_dev(clog);
        // a resident log: the kernels' unguarded block reads run up to 256
        // bytes past a record, inside the allocation
        if (log_dev && !dev_range(dlog, len + 256)) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (clog_dev && !dev_range(clog, ntx * es)) return MH_ERR_ILLEGAL_ARGUMENTS;
        s.dst = s.out.dst(0, ntx, true);
        if (s.dst.bad || !s.dst.aligned()) return MH_ERR_ILLEGAL_ARGUMENTS;
        // ---- copy chunks of a host log; record groups: one for a resident
        // log, at most one per copy chunk
        bool pinned = false;
        const std::vector<uint64_t> cut = txlog_chunk_cuts(dlog, len, log_dev, &pinned);
        const uint64_t nck = cut.size() - 1;
        const size_t ngmax = log_dev ? 1 : nck;
        const bool stage_hd = hdrs_out && !s.dst.hd;
        Layout L;
        const uint64_t b_ro = L.add(ntx * 8), b_ao = L.add(ntx * 8), b_pre = L.add(ntx * 4),
                       b_st = L.add(ntx * 4), b_eh = L.add(ntx * 32), b_a = L.add(ntx * 32),
                       b_hd = L.add(stage_hd ? ntx * sizeof(mh_tx_header) : 0),
                       b_cl = L.add(clog_dev ? 0 : ntx * es), b_stats = L.add((4 + 2 * ngmax) * 8);
        MH_HIP(c->s_clog.ensure(L.total));
        uint8_t *base = c->s_clog.as<uint8_t>(), *eh = base + b_eh;
        uint64_t *ro = s.ro = (uint64_t *)(base + b_ro), *ao = (uint64_t *)(base + b_ao),
                 *stats = s.stats = (uint64_t *)(base + b_stats), *gstats = stats + 4;
        int32_t *pre = s.pre = (int32_t *)(base + b_pre), *sts = s.sts = (int32_t *)(base + b_st);
        s.alh = base + b_a;
        MhTxHeader *hd = s.hd = stage_hd ? (MhTxHeader *)(base + b_hd) : nullptr;
        const uint8_t *dcl = clog_dev ? clog : base + b_cl;
        if (!log_dev) MH_HIP(c->s_txlog.ensure(len + 256));
        const uint8_t *db = log_dev ? dlog : c->s_txlog.as<uint8_t>();
        if (int e = s.reset_stats(0, 4 + 2 * ngmax)) return e;
        MH_HIP(c->p_small.ensure(64 + 16 * ngmax));
        volatile uint64_t *hs = s.hs = c->p_small.as<volatile uint64_t>();
        // every exit waits for the stream (kernels may store into the caller's
        // pinned / device arrays; copies read the caller's log)
        StreamGuard guard{{st}};
        ChunkCopier cc(c);
        if (!log_dev) {
            MH_HIP(ensure_chunk_events(c, nck));
            cc.chunks.resize(nck);
            for (uint64_t k = 0; k < nck; k++)
                cc.chunks[k] = {{const_cast<uint8_t *>(db) + cut[k], dlog + cut[k], cut[k + 1] - cut[k]}};
            cc.inline_issue = pinned;
            MH_HIP(cc.start());
        }
        // (after the chunk copies are issued: they wait for this stream's
        // earlier work, the previous call's readers of the staging buffer)
        if (!clog_dev) MH_HIP(hipMemcpyAsync(base + b_cl, clog, ntx * es, hipMemcpyHostToDevice, st));
        // (the host's pass over the cLog runs under the copies: ~2-3 ns per
        // entry, 0.15-0.2 ms for 65 536 entries, was ahead of them)
        s.hcl = clog_dev ? nullptr : clog;
        if (clog_dev && !log_dev) {
            // (on this stream, not hipMemcpy's: that one would wait for the
            // copy streams, i.e. for the whole log to land)
            MH_HIP(s.fetch_clog());
            MH_HIP(hipStreamSynchronize(st));
        }
        std::vector<uint64_t> tg{0, ntx}, lim{len}, bound{kTxlLanesMaxEntries};
        if (!log_dev) clog_groups(s, cut, tg, lim, bound);
        const size_t ng = tg.size() - 1;
        // group g's arrays start at its first record
        auto run_group = [&](size_t g, uint64_t wmax, const uint64_t *wmax_dev) -> int {
            const uint64_t t0 = tg[g], n = tg[g + 1] - t0;
            if (!n) return MH_OK;
            TxlogHostOut ho = s.dst.host_out();
            if (ho.status) ho.status += t0;
            if (ho.alh) ho.alh += t0 * 8;
            if (ho.hdrs) ho.hdrs += t0 * 17;
            MH_HIP(launch_txlog_lanes(st, c->tm(), n, db, ro + t0, ao + t0, nullptr, pre + t0,
                                      hd ? hd + t0 : nullptr, eh + t0 * 32, s.alh + t0 * 32, sts + t0, ho,
                                      std::max<uint64_t>(wmax, 1), len, wmax_dev, wmax_dev ? stats : nullptr));
            return MH_OK;
        };
        if (log_dev) {
            // 1. every record's structure where its cLog entry points
            MH_HIP(launch_txlog_struct(st, c->tm(), ntx, db, len, len, dcl, es, ro, ao, nullptr,
                                       max_entries, max_key_len, pre, gstats));
            // 2. the accepted records hashed and checked, the launch shaped by
            // the previous call's widest record (no wait: 0.264 -> ~0.245 ms
            // on 65 536 records), by this one's on a first call
            if (c->clog_wmax) {
                if (int e = run_group(0, c->clog_wmax, gstats)) return e;
            } else {
                MH_HIP(hipMemcpyAsync((void *)hs, gstats, 2 * 8, hipMemcpyDeviceToHost, st));
                MH_HIP(hipStreamSynchronize(st));
                if (int e = run_group(0, hs[0], nullptr)) return e;
            }
        } else {
            for (size_t g = 0; g < ng; g++) {
                const uint64_t t0 = tg[g], n = tg[g + 1] - t0;
                // the group's bytes have landed: chunk g (or every chunk for the
                // one group of a cLog out of log order)
                const size_t ck = ng == nck ? g : nck - 1;
                if (ng == nck || g == 0) {
                    for (size_t k = ng == nck ? ck : 0; k <= ck; k++) {
                        if (hipError_t e = cc.wait(k)) return -(int)e;
                        MH_HIP(cc.stream_wait(st, k));
                    }
                }
                if (!n) continue;
                MH_HIP(launch_txlog_struct(st, c->tm(), n, db, len, lim[g], dcl + t0 * es, es, ro + t0,
                                           ao + t0, nullptr, max_entries, max_key_len, pre + t0,
                                           gstats + 2 * g));
                if (int e = run_group(g, bound[g], gstats + 2 * g)) return e;
            }
        }
        // 3. how many records failed, and the first (and, for a host log, how
        // many records the host must re-validate); results down
        if (int e = s.results_down(0, ng)) return e;
        MH_HIP(hipStreamSynchronize(st));
        if (!log_dev)
            if (hipError_t e = cc.sync()) return -(int)e;  // the caller's log is no longer read
        if (hs[0]) {  // a launch too narrow for its records: again, shaped by them
            if (int e = s.reset_stats(0, 4)) return e;
            for (size_t g = 0; g < ng; g++)
                if (int e = run_group(g, hs[8 + 2 * g], nullptr)) return e;
            if (int e = s.results_down(0, 0)) return e;
            MH_HIP(hipStreamSynchronize(st));
        }
        uint64_t nhost = 0;
        for (size_t g = 0; g < ng; g++) nhost += hs[8 + 2 * g + 1];
        if (log_dev) c->clog_wmax = std::max<uint64_t>((uint64_t)hs[8], 1);
        // 4. the records the device left to the host
        if (nhost)
            if (int e = s.host_fallback()) return e;
        guard.streams.clear();
        if (nbad_out) *nbad_out = hs[2];
        if (first_bad_out) *first_bad_out = hs[2] ? hs[3] : ntx;
        return MH_OK;
    }
}

extern "C" int mh_txlog_validate_clog(mh_ctx *c, const uint8_t *dlog, uint64_t len,
                                      const uint8_t *clog, uint64_t ntx, uint32_t clog_entry_size,
                                      uint32_t max_entries, uint32_t max_key_len,
                                      mh_tx_header *hdrs_out, uint8_t *alh_out,
                                      int32_t *status_out, uint64_t *nbad_out,
                                      uint64_t *first_bad_out) {
    return mh_guard([&]() -> int {
        if (!c) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        return txlog_validate_clog_core(c, dlog, len, clog, ntx, clog_entry_size, max_entries,
                                        max_key_len, hdrs_out, alh_out, status_out, nbad_out,
                                        first_bad_out);
    });
}
