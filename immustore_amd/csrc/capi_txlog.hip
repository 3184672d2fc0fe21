// capi_txlog.hip -- the device read path of a tx log (a14): mh_txlog_validate,
// mh_txlog_validate_resident and txlog_validate_parsed (the multi-device
// call's entry), all three over one driver, TxlogCall, plus the pieces the
// cLog call (capi_clog.hip) shares with it: copy-chunk cuts, the caller's
// output arrays (TxlogOutputs), the device range check -- and with it the
// resident-store check of the answer, export and tx-answer calls.
//
// The host hop is in txlog_hop.hip; every SHA-256 runs in tx_kernels.hip,
// txlog_wave.hip, txlog_lanes.hip and htree_kernels.hip.
#include "capi_internal.hpp"

// ------------------------------------------------------------ shared pieces
// The device address of [p, p + bytes) when the whole range is pinned host
// memory the kernels can store to (one registration or allocation, word
// aligned), else null.
static uint32_t *host_words(void *p, uint64_t bytes) {
    if (!p || !bytes || ((uintptr_t)p & 3) || (bytes & 3)) return nullptr;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess ||
        hipPointerGetAttributes(&b, (uint8_t *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || b.type != hipMemoryTypeHost || !a.devicePointer ||
        (uint8_t *)b.devicePointer - (uint8_t *)a.devicePointer != (ptrdiff_t)(bytes - 1))
        return nullptr;
    return (uint32_t *)a.devicePointer;
}

bool dev_range(const void *p, uint64_t bytes) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t b = (uintptr_t)base, d = (uintptr_t)p;
    return d >= b && d - b <= size && bytes <= size - (d - b);
}

bool on_device(const void *q, int device) {
    hipPointerAttribute_t a;
    const bool d = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeDevice &&
                   a.device == device;
    (void)hipGetLastError();
    return d;
}

bool store_args_ok(const mh_answer_store &s, const mh_export_vlog *vlogs, uint32_t nvlogs) {
    if (s.clog_entry_size != 12 && s.clog_entry_size != 44) return false;
    if (nvlogs > 127 || (nvlogs && !vlogs)) return false;  // MaxParallelIO
    if (s.ntx && (!s.txlog || !s.clog)) return false;
    for (uint32_t k = 0; k < nvlogs; k++) {
        const mh_export_vlog &v = vlogs[k];
        if (v.end_off < v.first_off) return false;
        if (v.end_off > v.first_off && (!v.data || ((uintptr_t)v.data & 3))) return false;
    }
    return true;
}

bool store_resident(const mh_answer_store &s, const mh_export_vlog *vlogs, uint32_t nvlogs, int device) {
    if (s.ntx && (!on_device(s.txlog, device) || !on_device(s.clog, device))) return false;
    for (uint32_t k = 0; k < nvlogs; k++)
        if (vlogs[k].end_off > vlogs[k].first_off && !on_device(vlogs[k].data, device)) return false;
    // (memory of another place is refused before the device is touched at all)
    if (hipSetDevice(device) != hipSuccess) return false;
    if (s.ntx && (!dev_range(s.txlog, s.txlog_len + 256) || !dev_range(s.clog, s.ntx * s.clog_entry_size)))
        return false;
    for (uint32_t k = 0; k < nvlogs; k++) {
        const mh_export_vlog &v = vlogs[k];
        if (v.end_off > v.first_off && !dev_range(v.data, v.end_off - v.first_off + 256)) return false;
    }
    return true;
}

// Where a kernel can store the caller's output array p of `bytes`: p itself
// when it is device memory (its whole range in one allocation; *bad when it
// is not), the device alias of pinned host memory, else null (staged on the
// device and copied down).
static uint32_t *kernel_dst(void *p, uint64_t bytes, bool *bad, bool *is_dev) {
    if (!p || !bytes) return nullptr;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;  // pageable host memory
    }
    if (a.type == hipMemoryTypeDevice) {
        if (!dev_range(p, bytes)) *bad = true;
        *is_dev = true;
        return (uint32_t *)p;
    }
    return a.type == hipMemoryTypeHost ? host_words(p, bytes) : nullptr;
}

TxlogOutputs::Dst TxlogOutputs::dst(uint64_t t0, uint64_t nt, bool device_ok) const {
    Dst d;
    auto where = [&](void *p, uint64_t bytes, bool *is_dev) {
        return device_ok ? kernel_dst(p, bytes, &d.bad, is_dev) : host_words(p, bytes);
    };
    if (status) d.st = where(status + t0, nt * 4, &d.st_dev);
    if (alh) d.alh = where(alh + t0 * 32, nt * 32, &d.alh_dev);
    if (hdrs) d.hd = where(hdrs + t0, nt * sizeof(mh_tx_header), &d.hd_dev);
    d.all = (!status || d.st) && (!alh || d.alh) && (!hdrs || d.hd);
    return d;
}

int TxlogOutputs::copy_down(hipStream_t st, uint64_t t0, uint64_t nt, const Dst &d,
                            const void *st_src, const void *alh_src, const void *hd_src) const {
    if (status && !d.st) MH_HIP(hipMemcpyAsync(status + t0, st_src, nt * 4, hipMemcpyDeviceToHost, st));
    if (alh && !d.alh) MH_HIP(hipMemcpyAsync(alh + t0 * 32, alh_src, nt * 32, hipMemcpyDeviceToHost, st));
    if (hdrs && !d.hd)
        MH_HIP(hipMemcpyAsync(hdrs + t0, hd_src, nt * sizeof(mh_tx_header), hipMemcpyDeviceToHost, st));
    return MH_OK;
}

int TxlogOutputs::put_device(hipStream_t st, const Dst &d, uint64_t t, const int32_t *s,
                             const uint8_t *a, const mh_tx_header *h) const {
    if (d.st_dev) MH_HIP(hipMemcpyAsync(status + t, s, 4, hipMemcpyHostToDevice, st));
    if (d.alh_dev) MH_HIP(hipMemcpyAsync(alh + t * 32, a, 32, hipMemcpyHostToDevice, st));
    if (d.hd_dev) MH_HIP(hipMemcpyAsync(hdrs + t, h, sizeof(mh_tx_header), hipMemcpyHostToDevice, st));
    return MH_OK;
}

void TxlogOutputs::put_host(const Dst &d, uint64_t t, int32_t s, const uint8_t *a, const mh_tx_header &h) const {
    if (status && !d.st_dev) status[t] = s;
    if (alh && !d.alh_dev) memcpy(alh + t * 32, a, 32);
    if (hdrs && !d.hd_dev) hdrs[t] = h;
}

// relative sizes of a pinned log's copy chunks, first to last: 5 : 2 : 1.
// The first two groups take the lane-per-record kernel (k_txlog_lanes, >=
// 16384 records of 2^16), whose launch over 5/8 of the log finishes under the
// next chunk's copy; the last group (1/8) takes the wave kernel, the shorter
// chain per record after the last byte lands.  One chunk boundary fewer than
// round 4's 4 : 2 : 1 : 1: 1.529-1.535 vs 1.555-1.568 ms per call, 3
// interleaved rounds (profiles/txlog_lanes_r05.txt; 6 : 1 : 1 ties, 7 : 1
// and 13 : 2 : 1 overrun the last copy, 11 : 4 : 1 and 9 : 4 : 2 : 1 lose).
// MH_TXLOG_WEIGHTS="w0:w1:..." gives any sizes (read per call, tests: up to
// 16 positive numbers separated by ':' or ',')
static std::vector<double> txlog_weights() {
    std::vector<double> w;
    if (const char *e = getenv("MH_TXLOG_WEIGHTS")) {
        for (const char *p = e; *p && w.size() < 16;) {
            char *q = nullptr;
            const double v = strtod(p, &q);
            if (q == p || !(v > 0)) break;
            w.push_back(v);
            if (*q != ',' && *q != ':') break;
            p = q + 1;
        }
    }
    if (w.empty()) w = {5, 2, 1};
    return w;
}

// A pinned log: 3 chunks from 16 MiB up (the last chunk's device work is the
// tail after the copy), all queued from the calling thread at once.  A
// pageable one is staged by the runtime inside each copy call, so a helper
// thread (ChunkCopier) issues those under the hop, in two chunks (3/4 + 1/4:
// every staged call has its own setup).
std::vector<uint64_t> txlog_chunk_cuts(const uint8_t *log, uint64_t len, bool resident, bool *pinned) {
    // the whole range in one pinned allocation (first and last byte)
    *pinned = len && !resident && pinned_same_alloc(log, log + len - 1);
    // (a resident log: one chunk without a copy)
    if (resident || len < (16ull << 20)) return {0, len};
    const std::vector<double> wts = *pinned ? txlog_weights() : std::vector<double>{3, 1};
    const uint64_t K = wts.size();
    std::vector<uint64_t> cut(K + 1, 0);
    double wsum = 0, pre = 0;
    for (double w : wts) wsum += w;
    for (uint64_t k = 1; k < K; k++) {
        pre += wts[k - 1];  // the first k weights
        cut[k] = std::max<uint64_t>(cut[k - 1], (uint64_t)((double)len * pre / wsum) & ~4095ull);
    }
    cut[K] = len;
    return cut;
}

namespace {

// The mh_tx_header words of the record at buf + rec other than Eh (words
// 11-14), exactly as k_txlog_wave stores them: id, ts, blTxID (BE64), blRoot
// and prevAlh (raw), version | nentries << 32, v1: mdLen | (rec + 92) << 32.
// The hop has bounds-checked the record.
void fill_header_host(const uint8_t *buf, uint64_t rec, uint64_t *h) {
    const uint8_t *p = buf + rec;
    h[0] = be_at(p, 8);
    h[1] = be_at(p + 8, 8);
    h[2] = be_at(p + 16, 8);
    memcpy(h + 3, p + 24, 64);
    const uint32_t ver = (uint32_t)be_at(p + 88, 2);
    const uint32_t ml = ver ? (uint32_t)be_at(p + 90, 2) : 0;  // (v0: the entry count is there)
    const uint32_t nent = (uint32_t)(ver ? be_at(p + 92 + ml, 4) : be_at(p + 90, 2));
    h[15] = (uint64_t)ver | ((uint64_t)nent << 32);
    h[16] = ver ? (uint64_t)ml | ((uint64_t)(uint32_t)(rec + 92) << 32) : 0;
}

// Appends records [r0, r1) of src to dst, their byte offsets moved by shift
// (modulo 2^64: a negative move is its two's complement), and their patches
// -- src.P from *p on, which is in record order -- renumbered to dst's records
// (moved out of a source that is not const).
template <class Hop>
void hop_append(HopOut &dst, Hop &src, size_t r0, size_t r1, size_t *p, uint64_t shift) {
    const uint64_t renum = dst.R.size() - r0;
    for (size_t r = r0; r < r1; r++)
        dst.R.push_back(HopRec{src.R[r].rec + shift, src.R[r].alh + shift, src.R[r].nent, 0});
    for (; *p < src.P.size() && src.P[*p].rec < r1; ++*p) {
        dst.P.push_back(std::move(src.P[*p]));
        dst.P.back().rec += renum;
    }
}

// ---- one group of records: its own device arrays (per entry record offset,
// version, leaf digest; per tx header, entry-count word, record offset, Alh
// offset, leaf offset, Eh, inner-hash scratch, Alh, status) and pinned index
// staging, all indexed from the group's first record
struct Grp {
    uint64_t t0 = 0, t1 = 0, E = 0, wmax = 0, k = 0;
    bool small = true, fetched = false, host_done = false, early = false, host_hdrs = false;
    uint64_t *pro = nullptr, *pap = nullptr, *plo = nullptr;  // pinned: record, Alh, leaf offsets
    uint64_t idx_bytes = 0;                                   // of those; the tree plan's follow
    uint64_t *rec = nullptr, *es = nullptr, *ro = nullptr, *ap = nullptr, *lo = nullptr, *stats = nullptr;
    uint8_t *ver = nullptr, *lv = nullptr, *eh = nullptr, *inner = nullptr, *alh = nullptr;
    MhTxHeader *hd = nullptr;
    int32_t *status = nullptr, *pre = nullptr;
    TreePlan P;

    uint64_t nt() const { return t1 - t0; }
    // the device arrays, laid out from address b; returns their total size
    // (b = 0: only the size is wanted)
    uint64_t place(uintptr_t b) {
        Layout L;
        const uint64_t n = nt();
        rec = (uint64_t *)(b + L.add(E * 8)), ver = (uint8_t *)(b + L.add(E));
        lv = (uint8_t *)(b + L.add(std::max<uint64_t>(E, 1) * 32));
        hd = (MhTxHeader *)(b + L.add(n * sizeof(mh_tx_header))), es = (uint64_t *)(b + L.add(n * 8));
        ro = (uint64_t *)(b + L.add(n * 8)), ap = (uint64_t *)(b + L.add(n * 8));
        lo = (uint64_t *)(b + L.add((n + 1) * 8)), eh = (uint8_t *)(b + L.add(n * 32));
        inner = (uint8_t *)(b + L.add(n * kTxInnerStride)), alh = (uint8_t *)(b + L.add(n * 32));
        status = (int32_t *)(b + L.add(n * 4)), pre = (int32_t *)(b + L.add(n * 4));
        stats = (uint64_t *)(b + L.add(4 * 8));
        return L.total;
    }
    // index arrays up (a kernel reads them from the pinned staging: a DMA copy
    // would wait behind the log chunks still in flight)
    hipError_t fetch(hipStream_t st) {
        fetched = true;
        return launch_fetch_host(st, HostRuns{{pro, pap, plo}, {ro, ap, lo}, {nt(), nt(), nt() + 1}});
    }
};

// One validation call.  The raw records go to the device first, in chunks
// with an event after each: the copy (DMA when buf is pinned) runs under the
// host hop, and the device work on the records of a chunk starts as soon as
// it has landed, under the copy of the rest.  Events ev_chunks[0, K) mark the
// chunks' arrival (no system-scope fence: their waiters are device streams),
// ev_results[0, K) the end of each group's kernels (with the fence:
// c->d2h_stream's copies of a group's results may run on a DMA engine,
// ADVICE r04).  validate() is the driver and reads top to bottom.
struct TxlogCall {
    // ---- the call: context (c->mu held), log, limits, caller outputs
    mh_ctx *c;
    const uint8_t *buf, *dlog;
    uint64_t len, max_txs;
    HopLimits lim;
    TxlogOutputs out;
    const HopView *view;  // the records, parsed already (null: hopped here)
    // ---- copies
    hipStream_t st = nullptr;
    const uint8_t *dbuf = nullptr;  // the log on the device as the kernels read it
    // the rest group's metadata patch lists (upload_patches): npe entry patches, nph header
    // patches, at pl on the device ([ne idx][ne off][nh idx][nh off | len << 32])
    const uint64_t *pl = nullptr;
    uint64_t npe = 0, nph = 0;
    std::vector<uint64_t> cut;  // copy chunk k: bytes [cut[k], cut[k + 1])
    uint64_t nck = 0;
    StreamGuard guard;  // (before cc: the copies are waited for first)
    ChunkCopier cc{c};
    // ---- records and groups
    HopOut hop;                // every record of the call, offsets from buf
    size_t view_r = view ? view->r0 : 0, view_p = view ? view->p0 : 0;  // its next record / patch
    std::vector<Grp> gs;
    size_t queued = 0;         // gs[0, queued) are queued
    // D2H copies into pageable memory return only when done: those of the
    // early groups are issued once every group is queued
    std::vector<std::pair<const Grp *, hipEvent_t>> late;
    bool d2h_used = false;     // anything queued on c->d2h_stream this call

    // ---- cut the log, make the events, start the copies
    int start_copies() {
        hipSetDevice(c->device);
        MH_HIP(c->copy_lane());
        st = c->stream;
        // + 256: k_txlog_wave's staging of a wave's records reads up to 128
        // bytes past the last record's stored Alh (16-byte pieces + its
        // unguarded block over-read pad), inside the allocation
        if (len && !dlog) MH_HIP(c->s_txlog.ensure(len + 256));
        dbuf = dlog ? dlog : c->s_txlog.as<uint8_t>();
        bool pinned = false;
        cut = txlog_chunk_cuts(buf, len, dlog != nullptr, &pinned);
        nck = len ? cut.size() - 1 : 0;
        MH_HIP(ensure_chunk_events(c, nck));
        MH_HIP(ensure_result_events(c, nck));
        // once a group's kernels are queued they may store into the caller's
        // pinned status / alh / header arrays: every exit (errors included)
        // waits for both streams, so nothing writes caller memory after return
        // (every group on the context's stream: a second compute stream for
        // alternate groups slowed the last one, profiles/ab_txlog_streams_r04.txt)
        guard.streams = {st, c->d2h_stream};
        cc.chunks.resize(nck);
        for (uint64_t k = 0; k < nck; k++)
            cc.chunks[k] = {{const_cast<uint8_t *>(dbuf) + cut[k], buf + cut[k], dlog ? 0 : cut[k + 1] - cut[k]}};
        cc.inline_issue = pinned;
        MH_HIP(cc.start());
        gs.reserve(nck + 1);  // (late keeps pointers into gs)
        return MH_OK;
    }

    // ---- appends to hop the records that end inside [pos, end) of the log, at
    // most room of them, and sets hop.rc / hop.end: hopped here, or read from
    // the view, where the stretch reads as truncated while more records follow,
    // as the hop of a cut log does
    void records(uint64_t pos, uint64_t end, uint64_t room) {
        const size_t r0 = hop.R.size();
        if (!view) {
            HopOut h;
            size_t p = 0;
            txlog_hop(buf + pos, end - pos, room, lim, h);
            hop_append(hop, h, 0, h.R.size(), &p, pos);
            hop.rc = h.rc;
            hop.end = pos + h.end;
            return;
        }
        const HopOut &all = *view->all;
        size_t r1 = view_r;
        while (r1 < view->r1 && r1 - view_r < room && all.R[r1].alh - view->base + 32 <= end) r1++;
        hop_append(hop, all, view_r, r1, &view_p, 0 - view->base);
        view_r = r1;
        hop.rc = view_r < view->r1 ? MH_ERR_TRUNCATED : MH_OK;
        // (the view ends at len)
        hop.end = hop.rc == MH_OK ? end : hop.R.size() > r0 ? hop.R.back().alh + 32 : pos;
    }

    // records [t0, t1) of hop.R as group number gi
    int prepare(Grp &g, size_t gi, uint64_t t0, uint64_t t1) {
        g.t0 = t0;
        g.t1 = t1;
        const uint64_t nt = g.nt();
        for (uint64_t t = t0; t < t1; t++) {
            g.E += hop.R[t].nent;
            g.wmax = std::max<uint64_t>(g.wmax, hop.R[t].nent);
        }
        g.small = small_roots_fit(nt, g.wmax);
        while (c->s_txg.size() <= gi) c->s_txg.emplace_back();
        while (c->p_txg.size() <= gi) c->p_txg.emplace_back();
        MH_HIP(c->s_txg[gi].ensure(g.place(0)));
        g.place((uintptr_t)c->s_txg[gi].p);
        g.idx_bytes = 3 * (nt + 1) * 8;
        uint64_t pin = g.idx_bytes;
        if (!g.small) {
            std::vector<uint64_t> lof(nt + 1);
            lof[0] = 0;
            for (uint64_t t = 0; t < nt; t++) lof[t + 1] = lof[t] + hop.R[t0 + t].nent;
            g.P.build(nt, lof.data());
            pin += plan_index_bytes(g.P, nt);
        }
        // the previous call's kernels read this staging: done (synced)
        MH_HIP(c->p_txg[gi].ensure(pin));
        g.pro = c->p_txg[gi].as<uint64_t>();
        g.pap = g.pro + (nt + 1);
        g.plo = g.pap + (nt + 1);
        uint64_t acc = 0;
        for (uint64_t t = 0; t < nt; t++) {
            g.pro[t] = hop.R[t0 + t].rec;
            g.pap[t] = hop.R[t0 + t].alh;
            g.plo[t] = acc;
            acc += hop.R[t0 + t].nent;
        }
        g.plo[nt] = acc;
        return MH_OK;
    }

    // ---- a group's device work, reading the log at dbuf: index arrays up,
    // headers, per-entry index (tx.go:578-585), entry digests hashed in place
    // from the raw entry records (tx.go:690-731), one htree per tx
    // (tx.go:617-621; small trees one lane / wave per tree, a group with a wide
    // tx through the host tree plan), Alh with the rebuilt Eh vs the stored one
    // (tx.go:623-627), with the metadata patch lists if any (upload_patches).
    // pre (resident logs): the per-record statuses of the device bytes'
    // structure (txlog_struct.hip) -- filled here for the fused kernels,
    // by the caller for the chain -- so no kernel walks a length of the
    // resident log that differs from the host copy's.
    int run(Grp &g, int32_t *pre) {
        const uint64_t nt = g.nt();
        if (!g.fetched) MH_HIP(g.fetch(st));
        if (g.small && npe + nph == 0) {  // the whole chain in one launch
            if (pre)  // the resident bytes' structure against the host's
                MH_HIP(launch_txlog_struct(st, c->tm(), nt, dbuf, len, len, nullptr, 0, g.ro, g.ap, g.lo,
                                           lim.max_entries, lim.max_key_len, pre, g.stats));
            // pinned outputs: the kernel writes the results there itself
            TxlogHostOut ho;
            const TxlogOutputs::Dst d = out.dst(g.t0, nt, false);
            if (d.all && d.aligned()) {
                ho = d.host_out();
                g.host_done = true;
            }
            // a group of >= 16384 records takes the lane-per-record kernel
            // (throughput), a smaller one the wave kernel (its chain per
            // record is shorter: the latency-shaped tail after the last
            // chunk lands).  MH_TXLOG_KERNEL=wave | lanes (read per call)
            // forces one of them: the tests run both on the same logs.
            const char *kn = getenv("MH_TXLOG_KERNEL");
            const bool lanes = kn ? strcmp(kn, "lanes") == 0 : nt >= 16384;
            // The last chunk's group -- its kernel is the tail of the call
            // -- writes only the Eh words of the caller's pinned headers;
            // the host fills the other fields from the log while that
            // kernel runs (32 instead of 136 B per record over PCIe at the
            // end: -4..-10 us per call in 9 of 10 interleaved rounds with
            // the 5 : 2 : 1 chunks, profiles/txlog_lanes_r05.txt).
            if (!lanes && ho.hdrs && g.early && g.k + 1 == nck) {
                ho.eh_only = 1;
                g.host_hdrs = true;
            }
            if (lanes)
                MH_HIP(launch_txlog_lanes(st, c->tm(), nt, dbuf, g.ro, g.ap, g.lo, pre, g.hd, g.eh,
                                          g.alh, g.status, ho, g.wmax, len));
            else
                MH_HIP(launch_txlog_wave(st, c->tm(), nt, dbuf, g.ro, g.ap, g.lo, pre, g.hd, g.eh,
                                         g.alh, g.status, ho, g.wmax, g.pro, g.pap));
            return MH_OK;
        }
        MH_HIP(launch_tx_hdr_from_raw(st, c->tm(), nt, dbuf, g.ro, g.hd, g.es));
        MH_HIP(launch_txe_index(st, c->tm(), nt, dbuf, g.hd, g.es, g.lo, g.rec, g.ver));
        if (npe + nph)
            MH_HIP(launch_txlog_patch(st, npe, pl, pl + npe, g.rec, nph, pl + 2 * npe,
                                      pl + 2 * npe + nph, g.hd));
        MH_HIP(launch_txe_leaf(st, c->tm(), g.E, dbuf, g.rec, g.ver, g.small, g.lv));
        if (g.small) {
            MH_HIP(launch_small_roots(st, c->tm(), nt, g.lo, g.lv, g.eh, g.wmax));
        } else if (int e = run_tree_plan_on(c->s_tree, st, c->tm(), g.P, nt, g.E, g.lv, g.eh,
                                            reinterpret_cast<uint8_t *>(g.pro) + g.idx_bytes)) {
            return e;
        }
        MH_HIP(launch_tx_alh(st, c->tm(), nt, g.hd, dbuf, g.eh, g.inner, dbuf, g.ap, nullptr, g.alh,
                             g.status));
        if (pre)  // records whose resident bytes differ from the host copy
            MH_HIP(launch_txlog_apply_pre(st, nt, pre, g.status, g.alh));
        if (out.hdrs)  // the device headers with the rebuilt Eh
            MH_HIP(launch_put_eh(st, nt, g.eh, g.hd));
        return MH_OK;
    }

    // ---- a group's results down to the caller's arrays at record t0: by kernel
    // stores when they are pinned host memory (on the results stream, beside the
    // next group's kernels; a D2H copy would wait behind the log chunks on the
    // DMA engine), else by D2H copies (results_dma, late).  After event ev.
    int results(const Grp &g, hipEvent_t ev) {
        if (g.host_done) return MH_OK;  // stored by the group's kernel
        const uint64_t nt = g.nt();
        const TxlogOutputs::Dst d = out.dst(g.t0, nt, false);
        if (!d.all) {
            late.emplace_back(&g, ev);
            return MH_OK;
        }
        d2h_used = true;
        MH_HIP(hipStreamWaitEvent(c->d2h_stream, ev, 0));
        MH_HIP(launch_store_host(
            c->d2h_stream,
            HostWordRuns{{(const uint32_t *)g.status, (const uint32_t *)g.alh, (const uint32_t *)g.hd},
                         {d.st, d.alh, d.hd},
                         {d.st ? nt : 0, d.alh ? nt * 8 : 0, d.hd ? nt * sizeof(mh_tx_header) / 4 : 0}}));
        return MH_OK;
    }

    int results_dma(const Grp &g, hipEvent_t ev) {
        d2h_used = true;
        MH_HIP(hipStreamWaitEvent(c->d2h_stream, ev, 0));
        return out.copy_down(c->d2h_stream, g.t0, g.nt(), {}, g.status, g.alh, g.hd);
    }

    // an early group behind the event of its chunk, results on their stream
    int launch(Grp &g) {
        // the index arrays do not need the chunk: fetched before its event
        MH_HIP(g.fetch(st));
        g.early = true;
        if (hipError_t e = cc.wait(g.k)) return -(int)e;
        MH_HIP(cc.stream_wait(st, g.k));
        if (int e = run(g, nullptr)) return e;
        MH_HIP(hipEventRecord(c->ev_results[g.k], st));
        return results(g, c->ev_results[g.k]);
    }

    // ---- host hop (tx.go:419-603): record structure and limits only.  Per
    // entry the host reads the two lengths it needs to find the next entry
    // (parked helper threads over a long stretch, txlog_hop); the per-entry
    // index (record offsets, versions, message lengths) is rebuilt on the
    // device from each tx's first entry (k_txe_index).
    //
    // It runs in one phase per copy chunk: phase k parses the records
    // that end inside chunk k, from where phase k-1 stopped (a record
    // crossing the chunk's end reads as truncated there and is parsed
    // again by the next phase), and their device work is queued at once
    // behind the chunk's event.  The records and the return code are the
    // one-pass parse's either way: every check of hop_record reads only
    // bytes it has bounds-checked, so a shorter buffer can only end a
    // parse early with TRUNCATED or a short-id EOF.  A phase with
    // non-canonical metadata or a wide tx stops the early groups: the
    // rest goes as one group once the whole log is in.
    int phases() {
        uint64_t pos = 0;
        // (a log past 4 GiB is parsed in one phase: hop_record's 32-bit
        // metadata-offset check depends on where the parse starts)
        const uint64_t nphase = len <= 0xffffffffull ? nck : 1;
        bool early = nphase > 1;
        for (uint64_t k = 0; k < nphase; k++) {
            const uint64_t end = k + 1 < nphase ? cut[k + 1] : len;
            const uint64_t r0 = hop.R.size(), p0 = hop.P.size();
            records(pos, end, max_txs - r0);
            const bool patched = hop.P.size() > p0;
            const bool more = k + 1 < nphase && hop.R.size() < max_txs &&
                              (hop.rc == MH_ERR_TRUNCATED || (hop.rc == MH_OK && hop.end + 8 > end));
            if (patched) {
                early = false;
            } else if (early && hop.R.size() > r0) {
                gs.emplace_back();
                Grp &g = gs.back();
                if (int e = prepare(g, gs.size() - 1, r0, hop.R.size())) return e;
                if (!g.small) {
                    gs.pop_back();
                    early = false;
                } else {
                    g.k = k;
                    // queued now if its chunk's copy is (a pageable log's copy
                    // calls block their thread: the remaining phases of the
                    // hop go first, and these groups after them)
                    if (queued == gs.size() - 1 && cc.issued(k)) {
                        if (int e = launch(g)) return e;
                        queued++;
                    }
                }
            }
            if (!more) break;
            pos = hop.end;
        }
        if (!nck && !view) txlog_hop(buf, len, max_txs, lim, hop);  // empty log
        return MH_OK;
    }

    // a resident log whose group the fused kernels do not take (re-encoded
    // metadata, a wide tx): the chain runs over the host copy uploaded beside
    // it, and a record whose resident bytes differ from that copy is corrupted
    // (one byte compare).  dbuf becomes the uploaded copy.
    int upload_host_copy(Grp &g, int32_t *pre) {
        MH_HIP(c->s_txlog.ensure(len + 256));
        MH_HIP(hipMemcpyAsync(c->s_txlog.as<uint8_t>(), buf, len, hipMemcpyHostToDevice, st));
        MH_HIP(g.fetch(st));
        MH_HIP(launch_txlog_bytes_cmp(st, g.nt(), dlog, c->s_txlog.as<uint8_t>(), g.ro, g.ap, pre));
        dbuf = c->s_txlog.as<uint8_t>();
        return MH_OK;
    }

    // metadata that parses but is not in canonical form (a log not written by
    // immudb): Go hashes KVMetadata.Bytes() / TxMetadata.Bytes(), so the
    // canonical entry records / tx metadata go after the log bytes in a copy of
    // the log on the device (dbuf from here on), and the group's entry index /
    // headers point at them (pl, npe, nph)
    int upload_patches(const Grp &g) {
        uint64_t side = 0;
        for (const HopPatch &hp : hop.P) {
            side += hp.bytes.size();
            (hp.kind == 0 ? npe : nph)++;
        }
        if (len + side > 0xffffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::vector<uint8_t> sbuf;
        sbuf.reserve(side);
        std::vector<uint64_t> patch(2 * (npe + nph));  // [ne idx][ne off][nh idx][nh off | len << 32]
        uint64_t ie = 0, ih = 0;
        for (const HopPatch &hp : hop.P) {
            if (hp.rec < g.t0) return MH_ERR_ILLEGAL_STATE;  // early groups have none
            const uint64_t off = len + sbuf.size();
            if (hp.kind == 0) {
                patch[ie] = g.plo[hp.rec - g.t0] + hp.entry;  // (its first leaf, group-local)
                patch[npe + ie++] = off;
            } else {
                patch[2 * npe + ih] = hp.rec - g.t0;
                patch[2 * npe + nph + ih++] = off | ((uint64_t)hp.bytes.size() << 32);
            }
            sbuf.insert(sbuf.end(), hp.bytes.begin(), hp.bytes.end());
        }
        const uint64_t po = (len + side + 7) & ~7ull;
        MH_HIP(c->s_txpatch.ensure(po + patch.size() * 8));
        uint8_t *nb = c->s_txpatch.as<uint8_t>();
        MH_HIP(hipMemcpyAsync(nb, dbuf, len, hipMemcpyDeviceToDevice, st));
        MH_HIP(hipMemcpyAsync(nb + len, sbuf.data(), side, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(nb + po, patch.data(), patch.size() * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipStreamSynchronize(st));  // the host vectors go out of scope
        dbuf = nb;
        pl = reinterpret_cast<const uint64_t *>(nb + po);
        return MH_OK;
    }

    // ---- the records no early group took, as one group once the whole log is in
    int rest_group() {
        const uint64_t t_rest = gs.empty() ? 0 : gs.back().t1, ntx = hop.R.size();
        if (t_rest == ntx) return MH_OK;
        if (nck) MH_HIP(cc.stream_wait(st, nck - 1));
        gs.emplace_back();
        Grp &g = gs.back();
        if (int e = prepare(g, gs.size() - 1, t_rest, ntx)) return e;
        int32_t *pre = dlog ? g.pre : nullptr;
        if (dlog && !(g.small && hop.P.empty()))
            if (int e = upload_host_copy(g, pre)) return e;
        if (!hop.P.empty())
            if (int e = upload_patches(g)) return e;
        if (int e = run(g, pre)) return e;
        MH_HIP(hipEventRecord(c->ev_done[1], st));
        return results(g, c->ev_done[1]);
    }

    int validate(uint64_t *ntx_out, uint64_t *consumed_out) {
        if (int e = start_copies()) return e;
        if (int e = phases()) return e;
        for (; queued < gs.size(); queued++)
            if (int e = launch(gs[queued])) return e;
        // header fields other than Eh of a host_hdrs group (readHeader,
        // tx.go:419-518, as k_txlog_wave lays them out: 17 words per record)
        for (const Grp &g : gs)
            if (g.host_hdrs)
                for (uint64_t t = g.t0; t < g.t1; t++)
                    fill_header_host(buf, hop.R[t].rec, reinterpret_cast<uint64_t *>(out.hdrs + t));
        if (!gs.empty() && mh_fault(MH_FAULT_TXLOG_AFTER_GROUP)) return -(int)hipErrorOutOfMemory;
        // on an error hop.end is the failing record's offset = the end of the last good one
        if (ntx_out) *ntx_out = hop.R.size();
        if (consumed_out) *consumed_out = hop.end;
        if (hipError_t e = cc.join()) return -(int)e;  // every copy is issued
        if (int e = rest_group()) return e;
        for (const auto &r : late)
            if (int e = results_dma(*r.first, r.second)) return e;
        // only the streams this call queued work on (every wait is an API
        // round trip on the critical path of the call)
        MH_HIP(hipStreamSynchronize(st));
        if (d2h_used) MH_HIP(hipStreamSynchronize(c->d2h_stream));
        guard.streams.clear();
        // buf stays the caller's once we return
        if (nck) MH_HIP(cc.sync());
        return hop.rc;
    }
};

}  // namespace

int txlog_validate_core(mh_ctx *c, const uint8_t *buf, const uint8_t *dlog, uint64_t len,
                        HopLimits lim, uint64_t max_txs, uint64_t *ntx_out, uint64_t *consumed_out,
                        const TxlogOutputs &out, const HopView *parsed) {
    if (len && !buf) return MH_ERR_ILLEGAL_ARGUMENTS;
    TxlogCall call{c, buf, dlog, len, max_txs, lim, out, parsed};
    return call.validate(ntx_out, consumed_out);
}

// the three public forms: the context's lock taken, then the core
static int validate_locked(mh_ctx *c, const uint8_t *buf, const uint8_t *dlog, uint64_t len,
                           uint32_t max_entries, uint32_t max_key_len, uint64_t max_txs,
                           uint64_t *ntx_out, uint64_t *consumed_out, mh_tx_header *hdrs_out,
                           uint8_t *alh_out, int32_t *status_out, const HopView *parsed) {
    if (!c) return MH_ERR_ILLEGAL_ARGUMENTS;
    std::lock_guard<std::mutex> lk(c->mu);
    return txlog_validate_core(c, buf, dlog, len, HopLimits{max_entries, max_key_len}, max_txs, ntx_out,
                               consumed_out, TxlogOutputs{status_out, alh_out, hdrs_out}, parsed);
}

extern "C" int mh_txlog_validate(mh_ctx *c, const uint8_t *buf, uint64_t len, uint32_t max_entries,
                                 uint32_t max_key_len, uint64_t max_txs, uint64_t *ntx_out,
                                 uint64_t *consumed_out, mh_tx_header *hdrs_out, uint8_t *alh_out,
                                 int32_t *status_out) {
    return mh_guard([&]() -> int {
        return validate_locked(c, buf, nullptr, len, max_entries, max_key_len, max_txs, ntx_out,
                               consumed_out, hdrs_out, alh_out, status_out, nullptr);
    });
}

int txlog_validate_parsed(mh_ctx *c, const uint8_t *buf, uint64_t len, uint32_t max_entries,
                          uint32_t max_key_len, const HopView &pre, mh_tx_header *hdrs_out,
                          uint8_t *alh_out, int32_t *status_out) {
    return mh_guard([&]() -> int {
        const uint64_t nrec = pre.r1 - pre.r0;
        if ((nrec ? pre.all->R[pre.r1 - 1].alh + 32 - pre.base : 0) != len) return MH_ERR_ILLEGAL_STATE;
        uint64_t n = 0, used = 0;
        const int rc = validate_locked(c, buf, nullptr, len, max_entries, max_key_len, nrec, &n, &used,
                                       hdrs_out, alh_out, status_out, &pre);
        return rc == MH_OK && (n != nrec || used != len) ? MH_ERR_ILLEGAL_STATE : rc;
    });
}

extern "C" int mh_txlog_validate_resident(mh_ctx *c, const uint8_t *buf, const uint8_t *dlog,
                                          uint64_t len, uint32_t max_entries, uint32_t max_key_len,
                                          uint64_t max_txs, uint64_t *ntx_out,
                                          uint64_t *consumed_out, mh_tx_header *hdrs_out,
                                          uint8_t *alh_out, int32_t *status_out) {
    return mh_guard([&]() -> int {
        if (!c || (len && (!buf || !dlog))) return MH_ERR_ILLEGAL_ARGUMENTS;
        // the kernels stage 16-byte pieces up to 128 bytes past the last
        // record: the device allocation must extend len + 256 bytes
        if (len) hipSetDevice(c->device);
        if (len && !dev_range(dlog, len + 256)) return MH_ERR_ILLEGAL_ARGUMENTS;
        return validate_locked(c, buf, dlog, len, max_entries, max_key_len, max_txs, ntx_out,
                               consumed_out, hdrs_out, alh_out, status_out, nullptr);
    });
}
