// capi_internal.hpp -- host-side objects shared by the C-ABI translation
// units (capi.hip: htree / ahtree handles; capi_tx.hip: tx layer;
// txlog_hop.hip, capi_txlog.hip, capi_clog.hip: the tx-log read path).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <new>
#include <string>
#include <vector>

#include "mh_internal.hpp"

using namespace mh;

// Every extern "C" int entry point runs its body through mh_guard: a C++
// exception (std::bad_alloc from a host vector, std::system_error from a
// thread) becomes a status instead of crossing the C ABI.
template <class F>
inline int mh_guard(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return MH_ERR_OUT_OF_MEMORY;
    } catch (...) {
        return MH_ERR_ILLEGAL_STATE;
    }
}

#define MH_HIP(expr)                                        \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return -(int)e_;              \
    } while (0)

// Test-only fault sites (mh_debug_fail_at, include/immustore_merkle.h):
// true exactly once, when the armed countdown of `site` reaches zero.
bool mh_fault(int site);

// CSR offsets off[0..n] never run backwards (checked before a host wrapper
// rebases them and sizes the device copies from off[n] - off[0])
inline bool monotonic(const uint64_t *off, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return true;
}

static const uint8_t kEmptyRoot[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14,
                                       0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
                                       0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c,
                                       0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};

// ------------------------------------------------------------------ timing
struct EventTimer : Timer {
    struct Rec {
        std::string name;
        hipEvent_t a, b;
    };
    std::mutex mu;
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    bool enabled = false;
    hipEvent_t take() {
        hipEvent_t e;
        if (!pool.empty()) {
            e = pool.back();
            pool.pop_back();
        } else {
            hipEventCreate(&e);
        }
        return e;
    }
    // launches from several threads may interleave: end() closes the record
    // its own thread opened last (a stack per thread, so scopes may nest)
    std::unordered_map<std::thread::id, std::vector<size_t>> open;
    void begin(const char *name, hipStream_t st) override {
        std::lock_guard<std::mutex> g(mu);
        Rec r;
        r.name = name;
        r.a = take();
        r.b = take();
        hipEventRecord(r.a, st);
        open[std::this_thread::get_id()].push_back(recs.size());
        recs.push_back(r);
    }
    void end(hipStream_t st) override {
        std::lock_guard<std::mutex> g(mu);
        auto it = open.find(std::this_thread::get_id());
        if (it == open.end() || it->second.empty()) return;
        hipEventRecord(recs[it->second.back()].b, st);
        it->second.pop_back();
    }
    int sum(const char *prefix, double *ms, uint64_t *cnt) {
        std::lock_guard<std::mutex> g(mu);
        double tot = 0;
        uint64_t c = 0;
        size_t pl = prefix ? strlen(prefix) : 0;
        for (auto &r : recs) {
            if (pl && r.name.compare(0, pl, prefix) != 0) continue;
            hipError_t e = hipEventSynchronize(r.b);
            if (e != hipSuccess) return -(int)e;
            float x = 0;
            hipEventElapsedTime(&x, r.a, r.b);
            tot += x;
            c++;
        }
        if (ms) *ms = tot;
        if (cnt) *cnt = c;
        return MH_OK;
    }
    void reset() {
        std::lock_guard<std::mutex> g(mu);
        for (auto &r : recs) {
            hipEventSynchronize(r.b);
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        recs.clear();
        open.clear();
    }
    ~EventTimer() {
        for (auto &r : recs) {
            hipEventDestroy(r.a);
            hipEventDestroy(r.b);
        }
        for (auto e : pool) hipEventDestroy(e);
    }
};

// ------------------------------------------------------------------ buffers
struct DevBuf {
    void *p = nullptr;
    uint64_t cap = 0;
    hipError_t ensure(uint64_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        uint64_t c = std::max<uint64_t>(bytes + 64, 256);
        hipError_t e = hipMalloc(&p, c);
        if (e == hipSuccess) cap = c;
        return e;
    }
    template <class T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
    ~DevBuf() {
        if (p) hipFree(p);
    }
};

// Pinned host staging (hipHostMalloc), grown on demand.
struct PinBuf {
    void *p = nullptr;
    uint64_t cap = 0;
    hipError_t ensure(uint64_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (p) hipHostFree(p);
        p = nullptr;
        cap = 0;
        const uint64_t c = std::max<uint64_t>(bytes + 64, 4096);
        hipError_t e = hipHostMalloc(&p, c, hipHostMallocDefault);
        if (e == hipSuccess) cap = c;
        return e;
    }
    template <class T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
    ~PinBuf() {
        if (p) hipHostFree(p);
    }
};

struct mh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    EventTimer timer;
    std::mutex mu;  // guards scratch for mh_dev_* calls
    DevBuf s_hvals, s_msgoff, s_msgs, s_digests, s_idx, s_offs, s_ctr;
    DevBuf s_edge;        // ahtree frontier of a ranged append (64 x 32 B)
    DevBuf s_sort;        // length-class sort of ragged messages (varlen_kernels.hip)
    DevBuf s_tx, s_tree;  // tx layer (capi_tx.hip)
    DevBuf s_ventry;      // inclusion terms of VerifiableGet answers (capi_entry.hip); a group's
                          // entry arrays of mh_replicate_tx_batch (capi_repl.hip)
    DevBuf s_txlog;       // raw tx-log bytes of mh_txlog_validate
    DevBuf s_txpatch;     // the same + canonical metadata records (rare)
    DevBuf s_clog;        // mh_txlog_validate_clog's per-record arrays
    DevBuf s_ans, s_ans_tx, s_ans_ent, s_ans_out;  // mh_verifiable_answer_pb_batch: per request,
                                                   // per distinct tx, per entry, the bytes
    DevBuf s_exp, s_exp_ent, s_exp_out;  // mh_export_tx_batch: per tx, per entry, the blobs of
                                         // a call whose out is host memory
    DevBuf s_txs;  // mh_tx_answer_pb_batch: per variant (the rest of its scratch is s_ans*)
    uint64_t clog_wmax = 0;  // the widest record of its last resident call (the next launch's guess)
    // mh_txlog_validate's groups (one per copy chunk): device arrays and
    // pinned index staging of each, kept across calls
    std::deque<DevBuf> s_txg;
    std::deque<PinBuf> p_txg;
    PinBuf p_stage;       // host-built arrays of one call, staged for a single upload
    PinBuf p_small;       // a few words a kernel stores straight into host memory
    // second stream for host->device copies that overlap the compute stream
    // (chunked pipelines), its events, and the double-buffered chunk slots
    hipStream_t copy_stream = nullptr;
    hipStream_t copy_stream2 = nullptr;  // a second copy lane (ChunkCopier)
    hipStream_t d2h_stream = nullptr;  // device->host results of an early part of a call
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    DevBuf s_chunk[2];
    std::vector<hipEvent_t> ev_chunks;  // one per chunk of a pipelined call (arrivals)
    std::vector<hipEvent_t> ev_results; // one per group: its results are complete
    Timer *tm() { return timer.enabled ? &timer : nullptr; }
    // creates copy_stream and the events on first use (c->mu held)
    hipError_t copy_lane() {
        if (copy_stream) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&copy_stream2, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d2h_stream, hipStreamNonBlocking);
        for (int k = 0; k < 2 && e == hipSuccess; k++) {
            e = hipEventCreateWithFlags(&ev_copied[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_done[k], hipEventDisableTiming);
        }
        return e;
    }
    ~mh_ctx() {
        for (int k = 0; k < 2; k++) {
            if (ev_copied[k]) hipEventDestroy(ev_copied[k]);
            if (ev_done[k]) hipEventDestroy(ev_done[k]);
        }
        for (hipEvent_t e : ev_chunks) hipEventDestroy(e);
        for (hipEvent_t e : ev_results) hipEventDestroy(e);
        if (copy_stream) hipStreamDestroy(copy_stream);
        if (copy_stream2) hipStreamDestroy(copy_stream2);
        if (d2h_stream) hipStreamDestroy(d2h_stream);
    }
};

// the n-byte big-endian number at p (n <= 8)
inline uint64_t be_at(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}

// ---- the tx-log record hop (txlog_hop.hip), shared with the multi-device call
// Records of one stretch of a tx log (the structure readHeader / readEntry
// read, tx.go:419-603; no hashing).
// Per record: where it starts, where its stored Alh is, its entry count and
// the bytes of its entry-digest messages.  The headers themselves are only
// kept when asked (mh_txlog_scan); the validation path rebuilds them on the
// device from the raw record bytes (k_tx_hdr_from_raw).
struct HopRec {
    uint64_t rec, alh;
    uint32_t nent, pad;
};

// A record whose metadata is valid but not in the canonical form Go hashes
// (the reader re-serialises parsed metadata: KVMetadata.Bytes() in the entry
// digest, TxMetadata.Bytes() in the inner hash): the canonical bytes the
// device hashes instead.  kind 0: entry `entry` of the record, bytes = the
// whole entry record with canonical KV metadata; kind 1: the tx metadata.
struct HopPatch {
    uint64_t rec;  // index into HopOut::R
    uint32_t kind, entry;
    std::vector<uint8_t> bytes;
};

struct HopOut {
    std::vector<HopRec> R;
    std::vector<HopPatch> P;
    std::vector<mh_tx_header> H;  // want_headers only
    bool want_headers = false;
    uint64_t start = 0, end = 0;  // first record parsed / where parsing stopped
    int rc = MH_OK;
    bool stopped = false;  // EOF (id 0 / end of buffer) or a structural error
};

struct HopLimits {
    uint32_t max_entries, max_key_len;
};

// The whole hop of a run of records (no headers kept), as mh_txlog_validate
// runs it: out.R, out.P, out.rc (the structural status), out.end (consumed).
void txlog_hop(const uint8_t *buf, uint64_t len, uint64_t max_txs, const HopLimits &lim, HopOut &out,
               bool want_headers = false);
// Records [r0, r1) of a finished hop as a log of their own: their bytes start
// at all->R[r0].rec == base, and all->P[p0] is the first patch of a record
// >= r0.  Offsets and patch indices are rebased as the view is read.
struct HopView {
    const HopOut *all;
    size_t r0, r1, p0;
    uint64_t base;
};
// mh_txlog_validate with the record structure parsed already (capi_txlog.hip;
// pre: every record of [buf, buf + len), the last one ending at len): no host
// hop in the call.
int txlog_validate_parsed(mh_ctx *c, const uint8_t *buf, uint64_t len, uint32_t max_entries,
                          uint32_t max_key_len, const HopView &pre, mh_tx_header *hdrs_out,
                          uint8_t *alh_out, int32_t *status_out);

// ---- pieces the read-path calls share (capi_txlog.hip; capi_clog.hip)
// The caller's output arrays of a read-path call (each may be null), and where
// their records can be stored to: the one place that knows about pinned host
// memory, device memory and the kernels' 8-byte aligned headers.
struct TxlogOutputs {
    int32_t *status = nullptr;
    uint8_t *alh = nullptr;
    mh_tx_header *hdrs = nullptr;
    // Records [t0, t0 + nt) of each array as a kernel can store them: the
    // device alias of pinned host memory (one registration or allocation, word
    // aligned), the array itself when it is device memory (device_ok; bad when
    // its range is not inside one allocation), else null.  all: every array
    // the caller passed has such an address; aligned(): the headers' is a
    // multiple of 8 (the kernels store them as 64-bit words).
    struct Dst {
        uint32_t *st = nullptr, *alh = nullptr, *hd = nullptr;
        bool st_dev = false, alh_dev = false, hd_dev = false, bad = false, all = false;
        bool aligned() const { return ((uintptr_t)hd & 7) == 0; }
        // what a kernel stores its results through
        TxlogHostOut host_out() const { return TxlogHostOut{st, alh, reinterpret_cast<uint64_t *>(hd), 0}; }
    };
    Dst dst(uint64_t t0, uint64_t nt, bool device_ok) const;
    // "copy down": records [t0, t0 + nt) of the arrays d has no store address
    // for, from the device arrays st_src / alh_src / hd_src (indexed from t0)
    int copy_down(hipStream_t st, uint64_t t0, uint64_t nt, const Dst &d, const void *st_src,
                  const void *alh_src, const void *hd_src) const;
    // one re-validated record t (the cLog host fallback): into the outputs that
    // are device memory by copies on st, into those in host memory directly
    // (after the call's last wait)
    int put_device(hipStream_t st, const Dst &d, uint64_t t, const int32_t *s, const uint8_t *a,
                   const mh_tx_header *h) const;
    void put_host(const Dst &d, uint64_t t, int32_t s, const uint8_t *a, const mh_tx_header &h) const;
};

// Once a call's kernels are queued they may store into the caller's pinned or
// device arrays, and copies read the caller's log: every exit (errors
// included) waits for the streams listed here, so nothing touches caller
// memory after return.  Cleared once the call's own final waits ran.
struct StreamGuard {
    std::vector<hipStream_t> streams;
    ~StreamGuard() {
        for (hipStream_t s : streams) hipStreamSynchronize(s);
    }
};

// The device range [p, p + bytes) lies in one allocation of the current
// device (hipMemGetAddressRange), or the address is not device memory at all.
bool dev_range(const void *p, uint64_t bytes);
// q is device memory, and of `device` (capi_txlog.hip).
bool on_device(const void *q, int device);
// A resident store -- the fields mh_answer_store and mh_export_store share,
// and the value logs of the latter (nvlogs 0: none) -- checked once for
// mh_verifiable_answer_pb_batch, mh_export_tx_batch and mh_tx_answer_pb_batch
// (capi_txlog.hip); a call's own checks sit between the two.  By the arguments
// alone, no HIP call: the entry size, the vLog count, null logs of a store
// with txs, every vLog's bounds, data and 4-byte alignment.
bool store_args_ok(const mh_answer_store &s, const mh_export_vlog *vlogs, uint32_t nvlogs);
// Where it lies: the tx log, the cLog and every non-empty vLog on `device`
// (decided before the device is touched; then it is made the current one),
// each inside one allocation, the tx log and the vLogs with the 256 bytes of
// slack the kernels' block reads run into.
bool store_resident(const mh_answer_store &s, const mh_export_vlog *vlogs, uint32_t nvlogs, int device);
inline mh_answer_store store_prefix(const mh_export_store &s) {
    return {s.txlog, s.txlog_len, s.clog, s.ntx, s.clog_entry_size, s.max_entries, s.max_key_len};
}
// What a single-context batch call refuses by its arguments alone (n > 0; no
// HIP call, no lock, nothing written), stated beside that call.  Its mh_multi_*
// form runs the same check on the whole batch before any part starts.
bool htree_verify_args_ok(uint64_t n, const uint64_t *leaf, const uint64_t *width,
                          const uint64_t *term_off, const uint8_t *digests, const uint8_t *roots,
                          const uint8_t *ok);  // capi.hip
bool dual_proof_v2_args_ok(uint64_t n, const mh_tx_header *src_hdr, const mh_tx_header *tgt_hdr,
                           const uint64_t *incl_off, const uint8_t *incl_terms, const uint64_t *cons_off,
                           const uint8_t *cons_terms, const uint64_t *src, const uint64_t *tgt,
                           const uint8_t *src_alh, const uint8_t *tgt_alh,
                           const int32_t *status);  // capi_tx.hip
bool verify_values_args_ok(uint64_t n, const uint8_t *vals, const uint64_t *off, const uint8_t *hvals,
                           const int32_t *status);  // capi_values.hip
bool verified_get_args_ok(const mh_verified_get_batch &b, const int32_t *status, const uint8_t *ok,
                          const uint64_t *new_tx, const uint8_t *new_alh);  // capi_entry.hip
bool verified_tx_args_ok(const mh_verified_tx_batch &b, const int32_t *status, const uint8_t *ok,
                         const uint64_t *new_tx, const uint8_t *new_alh);  // capi_vtx.hip
// capi_commit.hip: mh_precommit_batch's own arguments; the entry offsets and
// byte pointers of transactions [t0, t1), which the single call checks chunk
// by chunk under the device work of the chunks before
bool precommit_args_ok(int version, uint64_t ntx, const uint64_t *tx_off, const uint64_t *key_off,
                       const uint8_t *md, const uint64_t *md_off, const uint64_t *val_off,
                       const uint8_t *hval_override, const uint8_t *use_override, const int32_t *status);
bool precommit_entries_ok(const uint64_t *tx_off, uint64_t t0, uint64_t t1, const uint8_t *keys,
                          const uint64_t *key_off, const uint8_t *md, const uint64_t *md_off,
                          const uint8_t *vals, const uint64_t *val_off);
// capi_doc.hip: mh_verify_document_batch's pointers, extents and byte pointers;
// every offset in order, which the single call checks while its copies run
bool document_args_ok(const mh_document_batch &B, const int32_t *status);
bool document_offsets_ordered(const mh_document_batch &B);

// the answers that fit are a prefix of the batch's bytes
inline uint64_t fit_prefix(const uint64_t *off, uint64_t n, uint64_t out_cap) {
    uint64_t fit = 0;
    for (uint64_t p = 0; p < n; p++)
        if (off[p + 1] <= out_cap) fit = off[p + 1];
    return fit;
}
// The copy chunks of a log of len bytes at `log`: chunk k is bytes [cut[k],
// cut[k + 1]).  One chunk for a resident log or one below 16 MiB, else
// txlog_weights() (5 : 2 : 1) for a pinned log and 3 : 1 for a pageable one,
// cut at multiples of 4 KiB.  *pinned: the whole log lies in one pinned
// allocation.
std::vector<uint64_t> txlog_chunk_cuts(const uint8_t *log, uint64_t len, bool resident, bool *pinned);
// mh_txlog_validate's body.  c->mu MUST be held by the caller (the public
// calls take it; the cLog call's host fallback holds it already).  buf: the
// log in host memory (the hop parses it); dlog: the same bytes already
// resident on the device (no copy; nullptr: copied from buf in chunks);
// parsed: the records, when the caller has hopped already (else nullptr).
int txlog_validate_core(mh_ctx *c, const uint8_t *buf, const uint8_t *dlog, uint64_t len,
                        HopLimits lim, uint64_t max_txs, uint64_t *ntx_out, uint64_t *consumed_out,
                        const TxlogOutputs &out, const HopView *parsed);

// mh_txlog_validate_clog's body (capi_clog.hip), same arguments and results.
// c->mu MUST be held by the caller.
int txlog_validate_clog_core(mh_ctx *c, const uint8_t *dlog, uint64_t len, const uint8_t *clog,
                             uint64_t ntx, uint32_t clog_entry_size, uint32_t max_entries,
                             uint32_t max_key_len, mh_tx_header *hdrs_out, uint8_t *alh_out,
                             int32_t *status_out, uint64_t *nbad_out, uint64_t *first_bad_out);

// Host-to-device copies of a call cut into chunks, issued from one helper
// thread (or two, chunk k on lane k % 2) onto the context's copy stream(s)
// with an event after each chunk.  A copy call from pinned memory holds its
// caller until the transfer is done, so every chunk boundary leaves the DMA
// engine idle for the next call's setup (60-100 us measured,
// profiles/txlog_copy_trace_r03.txt): few, large chunks.  The consumer
// waits for chunk k (wait(k): the copy and its event are enqueued) and then
// orders its stream after event ev(k).  c->mu must be held; both lanes start
// after everything queued on c->stream before start().
struct ChunkCopier {
    struct Piece {
        void *dst;
        const void *src;
        uint64_t bytes;
    };
    mh_ctx *c = nullptr;
    std::vector<std::vector<Piece>> chunks;
    std::mutex m;
    std::condition_variable cv;
    std::vector<uint8_t> done;  // chunk k enqueued (guarded by m)
    hipError_t err = hipSuccess;
    std::thread th[2];
    int lanes = 1;  // 1: one helper thread / copy stream; 2: two
    bool inline_issue = false;  // issue every copy from the caller (pinned sources: no blocking)

    bool started = false, synced = false;
    explicit ChunkCopier(mh_ctx *ctx) : c(ctx) {}
    // every copy is complete: none reads the caller's host memory any more
    // (the second lane's stream holds copies only with lanes == 2)
    hipError_t sync() {
        if (hipError_t e = join()) return e;
        if (started) {
            if (hipError_t e = hipStreamSynchronize(c->copy_stream)) return e;
            if (lanes == 2)
                if (hipError_t e = hipStreamSynchronize(c->copy_stream2)) return e;
        }
        synced = true;
        return hipSuccess;
    }
    // on every way out of the call: no copy may still read the caller's
    // host memory once it returns (an error path skips the final sync)
    ~ChunkCopier() {
        join();
        if (started && !synced) {
            hipStreamSynchronize(c->copy_stream);
            hipStreamSynchronize(c->copy_stream2);
        }
    }
    // chunks must be filled; events for every chunk must exist in c->ev_chunks
    hipError_t start() {
        done.assign(chunks.size(), 0);
        started = true;
        const bool idle = hipStreamQuery(c->stream) == hipSuccess;
        (void)hipGetLastError();  // hipErrorNotReady is not an error here
        // the copies overwrite device buffers that work queued earlier on the
        // context's stream may still read: the copy streams wait for it, unless
        // that stream is idle already (a cross-queue wait ahead of the first
        // copy delays its start: -20..-50 us per a14 call,
        // profiles/ab_txlog_wait0_flags_r04.txt; and the event itself is then
        // not recorded: ~3 us of host time ahead of the first copy)
        if (!idle) {
            if (hipError_t e = hipEventRecord(c->ev_done[0], c->stream)) return e;
            if (hipError_t e = hipStreamWaitEvent(c->copy_stream, c->ev_done[0], 0)) return e;
            if (hipError_t e = hipStreamWaitEvent(c->copy_stream2, c->ev_done[0], 0)) return e;
        }
        for (int j = 0; j < lanes; j++) {
            auto lane = [this, j]() {
                hipError_t e = hipSetDevice(c->device);
                hipStream_t s = j ? c->copy_stream2 : c->copy_stream;
                for (size_t k = (size_t)j; k < chunks.size(); k += (size_t)lanes) {
                    for (const Piece &p : chunks[k])
                        if (!e && p.bytes) e = hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyHostToDevice, s);
                    if (!e) e = hipEventRecord(c->ev_chunks[k], s);
                    std::lock_guard<std::mutex> g(m);
                    if (e) {
                        err = e;
                        cv.notify_all();
                        return;
                    }
                    done[k] = 1;
                    cv.notify_all();
                }
            };
            if (chunks.size() <= 1 || inline_issue) {  // no thread worth starting
                lane();
                continue;
            }
            try {
                th[j] = std::thread(lane);
            } catch (...) {
                lane();  // no thread: issue this lane's copies here
            }
        }
        return hipSuccess;
    }
    // chunk k's copies and event are enqueued (or an error happened)
    hipError_t wait(size_t k) {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return done[k] || err != hipSuccess; });
        return err;
    }
    // stream st waits until chunk k has landed (after wait(k) succeeded: its
    // copies and event are enqueued).  Events, not stream-written words:
    // ROCclr runs hipStreamWriteValue32 / WaitValue32 as blit kernels, no
    // faster (profiles/ab_txlog_wait0_flags_r04.txt)
    hipError_t stream_wait(hipStream_t st, size_t k) { return hipStreamWaitEvent(st, c->ev_chunks[k], 0); }
    // chunk k's copies and event are enqueued already (no waiting)
    bool issued(size_t k) {
        std::lock_guard<std::mutex> g(m);
        return done[k] || err != hipSuccess;
    }
    hipError_t join() {
        for (auto &t : th)
            if (t.joinable()) t.join();
        return err;
    }
};

// [a, b] (b >= a) lies inside ONE pinned host allocation: the allocation's
// address range as the runtime reports it for a (HIP_POINTER_ATTRIBUTE_
// RANGE_START_ADDR / _RANGE_SIZE, in the host or the device view of the
// allocation) must hold both ends.  Two separate hipHostMalloc blocks are not
// one allocation even when their device addresses are as far apart as their
// host addresses (on ROCm they usually are: same virtual address), and a copy
// of a span crossing them could read a gap.  Any query that
// fails means "no", i.e. one copy per array.
inline bool pinned_same_alloc(const void *a, const void *b) {
    hipPointerAttribute_t x;
    void *start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&x, a) != hipSuccess || x.type != hipMemoryTypeHost ||
        hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)a) !=
            hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)a) !=
            hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t s = (uintptr_t)start, ua = (uintptr_t)a, ub = (uintptr_t)b,
                    ud = (uintptr_t)x.devicePointer;
    if (ub < ua || !size) return false;
    uintptr_t off;
    if (ua >= s && ua - s < size)
        off = ua - s;
    else if (ud && ud >= s && ud - s < size)
        off = ud - s;
    else
        return false;
    return ub - ua < size - off;
}

// events for n chunks in c->ev_chunks
// Without the system-scope fence: every waiter on these events is a device
// stream (the host waits on streams), and the fence held each chunk's
// consumer ~4 us longer (-12..-19 us per a14 call in three interleaved
// rounds, profiles/ab_txlog_evfence_r04.txt).
inline hipError_t ensure_chunk_events(mh_ctx *c, size_t n) {
    const unsigned flags = hipEventDisableTiming | hipEventDisableSystemFence;
    while (c->ev_chunks.size() < n) {
        hipEvent_t e;
        if (hipError_t r = hipEventCreateWithFlags(&e, flags)) return r;
        c->ev_chunks.push_back(e);
    }
    return hipSuccess;
}

// The frame of the fused wire verifies (pb_decode.hip: DualProofV2 and
// DualProof v1 messages; capi_entry.hip, capi_vtx.hip: whole answers).
// The call is bound by the copy of the messages (1.8 GB for 10^6 DualProofV2
// at ~54 GB/s against ~11.5 ms of device work), so the batch is cut into
// chunks of MH_PB_CHUNK_MIB of messages (default 128): a ChunkCopier issues
// every chunk's copies on the context's copy stream and records one event per
// chunk, while the caller decodes and verifies chunk k on the compute stream
// as soon as its event fires -- only the last chunk's device work is exposed.
// open() checks the arguments, takes c->mu (held until the frame goes out of
// scope: declare the ChunkCopier after it), cuts the batch and makes the
// events; fill() lists the copies once the caller has laid out its buffer.
// A call that works group by group then calls group() and, per group,
// wait_group().
struct PbChunkFrame {
    std::unique_lock<std::mutex> lk;
    uint64_t n = 0, m0 = 0, mb = 0;  // messages, msg_off[0], message bytes
    uint64_t chunk_bytes = 128ull << 20;
    std::vector<uint64_t> cut{0};    // chunk k holds messages [cut[k], cut[k + 1])
    std::vector<uint64_t> longest;   // each chunk's longest message
    int nch = 0;
    std::vector<int> gcut{0};        // group(): the groups' first chunks
    int ng = 0;
    uint64_t group_n = 0, group_bytes = 0;  // messages / message bytes of the largest group
    const uint8_t *msgs = nullptr;
    const uint64_t *msg_off = nullptr;

    // The frame's arguments (n > 0; have_rest: the caller's other pointers are
    // all there), by the arguments alone: open() starts with it, and the
    // mh_multi_* forms run it on the whole batch before any part starts.
    static bool args_ok(uint64_t n, const uint8_t *msgs, const uint64_t *msg_off, bool have_rest) {
        if (!msg_off || !have_rest) return false;
        // a header's md_off is 32 bits over 2 n metadata slots
        if (2 * n * (uint64_t)kMdSlot > 0xffffffffull) return false;
        if (n > 0x7fffffffull) return false;  // hipcub's int item count
        if (!monotonic(msg_off, n)) return false;
        return msg_off[n] == msg_off[0] || msgs;
    }
    int open(mh_ctx *c, uint64_t n_, const uint8_t *msgs_, const uint64_t *msg_off_,
             bool have_rest) {
        if (!args_ok(n_, msgs_, msg_off_, have_rest)) return MH_ERR_ILLEGAL_ARGUMENTS;
        return open_checked(c, n_, msgs_, msg_off_);
    }
    // for a call whose own argument check ran args_ok already
    int open_checked(mh_ctx *c, uint64_t n_, const uint8_t *msgs_, const uint64_t *msg_off_) {
        n = n_, msgs = msgs_, msg_off = msg_off_;
        m0 = msg_off[0], mb = msg_off[n] - m0;
        lk = std::unique_lock<std::mutex>(c->mu);
        MH_HIP(hipSetDevice(c->device));
        MH_HIP(c->copy_lane());
        MH_HIP(c->p_small.ensure(64));
        // chunks: consecutive messages up to chunk_bytes (one at least)
        if (const char *e = getenv("MH_PB_CHUNK_MIB")) chunk_bytes = std::max(1, atoi(e)) * (1ull << 20);
        for (uint64_t i = 0; i < n;) {
            uint64_t j = i + 1, lm = msg_off[i + 1] - msg_off[i];
            while (j < n && msg_off[j + 1] - msg_off[i] <= chunk_bytes) {
                lm = std::max(lm, msg_off[j + 1] - msg_off[j]);
                j++;
            }
            cut.push_back(j);
            longest.push_back(lm);
            i = j;
        }
        nch = (int)cut.size() - 1;
        MH_HIP(ensure_chunk_events(c, nch));
        return MH_OK;
    }
    // groups: consecutive chunks decoded and verified by one set of launches
    // (group g holds chunks [gcut[g], gcut[g + 1])).  Every kernel of these
    // calls runs one message per lane, so a launch lasts as long as its
    // longest message takes one lane (~2.7 MB/s through both decode passes,
    // measured) however few messages it holds, while a chunk lands at
    // ~55 GB/s: launching per chunk pays that latency once per chunk for
    // nothing when messages are long (1 GiB of 44 KB messages, 312 KB the
    // longest: 1056 ms chunk by chunk, 8 x 115 ms of decode alone).  A group
    // therefore grows until its bytes take the link as long as its longest
    // message takes a lane, bytes >= ratio x longest (MH_PB_GROUP_RATIO,
    // default 16384; 0: every chunk alone): short messages keep the
    // chunk-by-chunk pipeline, long ones wait for more of the batch.
    // Sets gcut, ng and the largest group's sizes (what one group's scratch
    // is made for).
    void group() {
        uint64_t ratio = 16384;
        if (const char *e = getenv("MH_PB_GROUP_RATIO")) ratio = (uint64_t)std::max(0, atoi(e));
        for (int k = 0; k < nch;) {
            uint64_t bytes = 0, lm = 0;
            int j = k;
            do {
                bytes += msg_off[cut[j + 1]] - msg_off[cut[j]];
                lm = std::max(lm, longest[j]);
                j++;
            } while (j < nch && bytes / std::max<uint64_t>(lm, 1) < ratio);
            gcut.push_back(j);
            group_n = std::max(group_n, cut[j] - cut[k]);
            group_bytes = std::max(group_bytes, bytes);
            k = j;
        }
        ng = (int)gcut.size() - 1;
    }
    // chunk 0 carries the caller's per-message arrays whole (chunk0: offsets,
    // ids, Alh values, a request's keys ...: few large copies -- each copy call
    // costs the DMA engine ~0.1 ms of setup) and the first messages, chunk k
    // its messages; message byte msg_off[i] lands at d_msg + msg_off[i] - m0
    void fill(ChunkCopier &cc, uint8_t *d_msg, std::vector<ChunkCopier::Piece> chunk0) const {
        cc.chunks.resize(nch);
        cc.chunks[0] = std::move(chunk0);
        for (int k = 0; k < nch; k++) {
            const uint64_t lo = cut[k], hi = cut[k + 1];
            cc.chunks[k].push_back({d_msg + (msg_off[lo] - m0), msgs + msg_off[lo],
                                    msg_off[hi] - msg_off[lo]});
        }
    }
    // group g = messages [lo, lo + nk): the compute stream waits for its chunks
    int wait_group(mh_ctx *c, ChunkCopier &cc, int g, uint64_t &lo, uint64_t &nk) const {
        for (int k = gcut[g]; k < gcut[g + 1]; k++) {
            MH_HIP(cc.wait(k));
            MH_HIP(hipStreamWaitEvent(c->stream, c->ev_chunks[k], 0));
        }
        lo = cut[gcut[g]], nk = cut[gcut[g + 1]] - lo;
        return MH_OK;
    }
};

// events for the results of n groups in c->ev_results: default flags, i.e.
// WITH the system-scope release -- the copies that wait on them may read the
// results through a DMA engine rather than a kernel
inline hipError_t ensure_result_events(mh_ctx *c, size_t n) {
    while (c->ev_results.size() < n) {
        hipEvent_t e;
        if (hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return r;
        c->ev_results.push_back(e);
    }
    return hipSuccess;
}

struct mh_htree {
    mh_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;
    uint64_t max_width = 0;
    uint64_t width = 0;
    uint8_t root[32];
    DevBuf levels, in_a, in_b, in_c, off_a, off_b, off_c, ov, use, hv, msgoff, msgs, digests;
    DevBuf sort;  // length-class sort of ragged messages
    DevBuf w_in, w_out;  // wire formats (capi_wire.hip)
    void *pinned = nullptr;
    uint64_t pinned_cap = 0;
    LevelGeom geom;
};

struct mh_ahtree {
    mh_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;
    uint64_t size = 0;
    // every mh_ahtree_* call holds this for its whole duration, like the Go
    // AHtree's t.mutex (ahtree.go:60-84): readers (Root, proofs, dLog reads)
    // may run concurrently with a committer's Append, which can reallocate
    // the dLog.  Recursive: Append / Root call other locked entry points.
    std::recursive_mutex mu;
    DevBuf dlog, in, roots, idx, out, ctr;
    DevBuf w_in, w_out;  // wire formats (capi_wire.hip)
};

// room in t's dLog for new_size leaves (capi.hip; t->mu held): may move the
// dLog, keeping the nodes of t->size leaves
int aht_reserve(mh_ahtree *t, uint64_t new_size);

// Header preconditions shared by every entry point that reads headers.
inline int check_header(const mh_tx_header &h, uint64_t md_blob_len, bool have_blob) {
    if (h.version > 1) return MH_ERR_ILLEGAL_ARGUMENTS;
    if (h.md_len) {
        if (h.version == 0) return MH_ERR_METADATA_UNSUPPORTED;
        if (h.md_len > MH_MAX_TX_METADATA_LEN || !have_blob) return MH_ERR_ILLEGAL_ARGUMENTS;
        if ((uint64_t)h.md_off + h.md_len > md_blob_len) return MH_ERR_ILLEGAL_ARGUMENTS;
    }
    return MH_OK;
}

// ---------------------------------------------------------------- tx layer helpers
// Sub-allocations of one device scratch buffer (256-byte aligned).
struct Layout {
    uint64_t total = 0;
    uint64_t add(uint64_t bytes) {
        const uint64_t o = total;
        total = (total + bytes + 255) & ~255ull;
        return o;
    }
};

// The read-set stage of mh_verifiable_answer_pb_batch and mh_tx_answer_pb_batch
// (answer_read.hip): the txs a batch reads, every distinct one read and
// re-hashed once, the verdicts, links and entry counts of the asked ones.
// t->mu (if any) and c->mu are held, the device is set and a StreamGuard
// covers c->stream.  Three steps with the caller between them; each takes the
// Layout of one scratch buffer with the caller's own columns already in it,
// adds the stage's, makes the buffer and binds the stage's arrays of `a`:
//   requests(n, L)  c->s_ans      then the caller uploads kind / tx / since and its own
//   heads()         wait 1: D, D1 = max(D, 1) distinct txs
//   reads(S)        c->s_ans_tx   zeroed up to the re-hash's scratch; leaf_off scanned
struct AnsRead {
    mh_ctx *c;
    const mh_answer_store &s;
    AnsArrays &a;
    uint8_t *base = nullptr, *sb = nullptr;  // s_ans, s_ans_tx
    volatile uint64_t *hw = nullptr;         // p_small, where the waits read
    uint64_t W = 1, D1 = 1;
    uint64_t b_kind = 0, b_tx = 0, b_since = 0, b_dst = 0, b_dpo = 0, b_off = 0, b_dps = 0;
    uint8_t *scan = nullptr, *dscan = nullptr;  // scan temp of max(n, W) / D1 items
    size_t scan_bytes = 0, dscan_bytes = 0;
    int requests(uint64_t n, Layout &L);
    int heads();
    int reads(Layout &S);
};

// ---------------------------------------------------------------- many trees
// Level plan of a batch of htrees (htree.go:85-110 per tree): level 0 are the
// leaves of all trees back to back, every further level appends the nodes of
// the trees that still have more than one node.
struct TreePlan {
    std::vector<uint64_t> cur, prev, prevw;  // items, grouped by level
    struct Level {
        uint64_t base, nodes, item0, nitems;
    };
    std::vector<Level> levels;
    std::vector<uint64_t> root_idx;  // per tree: node index of the root, ~0 = empty tree
    uint64_t total_nodes = 0;

    void build(uint64_t ntrees, const uint64_t *leaf_off) {
        const uint64_t o0 = leaf_off[0];
        root_idx.assign(ntrees, ~0ull);
        struct Act {
            uint64_t t, base, w;
        };
        std::vector<Act> act, nxt;
        for (uint64_t t = 0; t < ntrees; t++) {
            const uint64_t w = leaf_off[t + 1] - leaf_off[t];
            if (w == 1) root_idx[t] = leaf_off[t] - o0;
            if (w > 1) act.push_back({t, leaf_off[t] - o0, w});
        }
        uint64_t next = leaf_off[ntrees] - o0;
        while (!act.empty()) {
            Level L{next, 0, cur.size(), act.size()};
            nxt.clear();
            for (const Act &a : act) {
                const uint64_t cw = (a.w + 1) / 2;
                cur.push_back(next);
                prev.push_back(a.base);
                prevw.push_back(a.w);
                if (cw == 1)
                    root_idx[a.t] = next;
                else
                    nxt.push_back({a.t, next, cw});
                next += cw;
                L.nodes += cw;
            }
            levels.push_back(L);
            act.swap(nxt);
        }
        total_nodes = next;
    }
};

// bytes of pinned staging run_tree_plan_on needs for plan P over ntrees trees
inline uint64_t plan_index_bytes(const TreePlan &P, uint64_t ntrees) {
    return (3 * P.cur.size() + ntrees) * 8;
}

// Leaves + levels + roots of a planned batch (capi_tx.hip).
// roots of many htrees over device digests (capi_tx.hip)
// innerHash / Alh of checked headers (capi_tx.hip); c->mu held by the caller.
int tx_alh_core(mh_ctx *c, uint64_t n, const mh_tx_header *hdrs, const uint8_t *md_blob,
                uint64_t md_blob_len, uint8_t *inner_out, uint8_t *alh_out);
// VerifyDualProofV2 (verification.go:303-372) over n proofs on the device
// (capi_tx.hip): THE statement of the V2 verifier, behind the array call and
// the wire call, as dual_proof_v1_core below is for v1.  Every array device
// memory, n entries; offsets and biased term pointers as in Dual1Arrays;
// status_in nullable, or status_out itself: a proof not MH_OK there keeps its
// status; scratch: dual_proof_v2_scratch_bytes(n), 256-byte aligned.
uint64_t dual_proof_v2_scratch_bytes(uint64_t n);
int dual_proof_v2_core(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *src_hdr,
                       const mh_tx_header *tgt_hdr, const uint8_t *md_blob,
                       const uint64_t *incl_off, const uint8_t *incl_terms,
                       const uint64_t *cons_off, const uint8_t *cons_terms, const uint64_t *src,
                       const uint64_t *tgt, const uint8_t *src_alh, const uint8_t *tgt_alh,
                       const int32_t *status_in, uint64_t md_blob_len, Dp1V0Metadata v0_md,
                       uint8_t *scratch, int32_t *status_out);
// VerifyDualProof (v1, verification.go:127-235) over nk decoded proofs that
// are on the device already (capi_tx.hip): THE statement of the v1 verifier,
// behind both mh_verify_dual_proof_batch (the caller's arrays, uploaded) and
// mh_verify_dual_proof_pb_batch (the decoder's arrays).  src / tgt / src_alh /
// tgt_alh / ok: device, nk entries; status (device, nullable): proofs whose
// decode status is not MH_OK are false; md_blob_len: the bytes behind
// o.md_blob; v0_md: the callers' one difference (Dp1V0Metadata); Q: nested
// proofs, o.off[kQ][nk] - o.off[kQ][0]; scratch: dual_proof_v1_scratch_bytes(
// nk, Q) device bytes, 256-byte aligned.  Only launches on st: no copy from or
// to the host, no synchronisation.
uint64_t dual_proof_v1_scratch_bytes(uint64_t nk, uint64_t Q);
int dual_proof_v1_core(hipStream_t st, Timer *tm, uint64_t nk, const Dual1Arrays &o,
                       const uint64_t *src, const uint64_t *tgt, const uint8_t *src_alh,
                       const uint8_t *tgt_alh, const int32_t *status, uint64_t md_blob_len,
                       Dp1V0Metadata v0_md, uint64_t Q, uint8_t *scratch, uint8_t *ok);
// The decode of a batch of DualProof (v1) messages on the device
// (pb_decode.hip, k_pbd_dual1): THE statement of that stage, behind
// mh_dual_proof_pb_decode_batch and the three fused verifies.  Two steps on
// c->stream with the caller between them: it knows the totals before any term
// is written, and makes the term area.
// The stage's regions for up to M proofs at a time, in the caller's Layout.
struct Dual1Scratch {
    uint64_t cnt, so, scan, hdr, md, tbl_alh, flags, lin;
    size_t scan_bytes;  // temp of one scan over M items, at scan (the caller's scans may use it)
    // scanned offset array j of a step over nk <= M proofs: nk + 1 entries
    uint64_t *off(uint8_t *base, int j, uint64_t nk) const {
        return (uint64_t *)(base + so) + (uint64_t)j * (nk + 1);
    }
};
Dual1Scratch dual1_decode_scratch(Layout &L, uint64_t M);
// Size step: message p is dmsg[beg[p] .. end[p]), or .. beg[p + 1]) with a
// null end.  Status, the counts and their scanned offsets (device); totals[j]
// = offset array j's last entry, on the host: the stream is synchronised.
int dual1_decode_size(mh_ctx *c, uint64_t nk, const uint8_t *dmsg, const uint64_t *beg,
                      const uint64_t *end, uint8_t *base, const Dual1Scratch &s, int32_t *status,
                      uint64_t totals[kCounts]);
// The term area those totals need, in the caller's Layout: the five lists,
// the nested terms, totals[kQ] + 1 nested offsets.
struct Dual1Terms {
    uint64_t terms[5], qterms, qoff;
};
Dual1Terms dual1_decode_terms(Layout &T, const uint64_t totals[kCounts]);
// Write step: everything of o, the terms at dt + t (device); same messages
// and status as the size step.
int dual1_decode_write(mh_ctx *c, uint64_t nk, const uint8_t *dmsg, const uint64_t *beg,
                       const uint64_t *end, uint8_t *base, const Dual1Scratch &s, uint8_t *dt,
                       const Dual1Terms &t, int32_t *status, Dual1Arrays &o);
// The decoders' kernels other translation units launch (pb_decode.hip).
// VerifiableEntry envelopes (k_pbd_ventry): message p is msgs[msg_off[p] ..
// msg_off[p + 1]); write = false: status and v.cnt, write = true: the rest of v
hipError_t launch_pbd_ventry(hipStream_t st, bool write, uint64_t n, const uint8_t *msgs,
                             const uint64_t *msg_off, const VentryArrays &v, int32_t *status);
// VerifiableTx envelopes (k_pbd_vtx): write = false: status, v.live and v.cnt,
// write = true: the rest of v
hipError_t launch_pbd_vtx(hipStream_t st, bool write, uint64_t n, const uint8_t *msgs,
                          const uint64_t *msg_off, const VtxArrays &v, int32_t *status);
// small read-backs by kernel stores into pinned host memory (out: device view)
hipError_t launch_put2_host(hipStream_t st, const uint64_t *a, const uint64_t *b, uint64_t *out);
int build_many_dev(mh_ctx *c, hipStream_t st, uint64_t ntrees, const uint64_t *leaf_off,
                   const uint8_t *d_dig, uint8_t *d_roots, DevBuf &s_lv, DevBuf &s_lo);
int run_tree_plan(mh_ctx *c, hipStream_t st, const TreePlan &P, uint64_t ntrees, uint64_t nleaves,
                  const uint8_t *d_digests, uint8_t *d_roots);
int run_tree_plan_on(DevBuf &scratch, hipStream_t st, Timer *tm, const TreePlan &P, uint64_t ntrees,
                     uint64_t nleaves, const uint8_t *d_digests, uint8_t *d_roots, uint8_t *pinned);
