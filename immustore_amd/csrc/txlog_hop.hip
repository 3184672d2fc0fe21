// txlog_hop.hip -- the host record hop of the tx-log read path (a14): the
// structure readHeader / readEntry read (tx.go:419-603), limits and metadata
// canonical forms, no hashing.  Host code only: nothing here calls the HIP
// runtime.  mh_txlog_scan is the hop on its own; the validation calls
// (capi_txlog.hip, capi_multi.hip) run txlog_hop() without headers.
#include <functional>

#include "capi_internal.hpp"

namespace {

// KVMetadata.unsafeReadFrom + Bytes() (kv_metadata.go:207-256): deleted(0),
// expiresAt(1, 8 bytes), nonIndexable(2); unknown codes and a short expiresAt
// are ErrCorruptedData; a repeated attribute replaces the earlier one; Bytes()
// writes the attributes in code order.
int kv_md_canonical(const uint8_t *md, uint64_t ml, uint8_t out[MH_MAX_KV_METADATA_LEN],
                    uint64_t *ol) {
    if (ml > MH_MAX_KV_METADATA_LEN) return MH_ERR_CORRUPTED_DATA;
    bool has[3] = {false, false, false};
    const uint8_t *exp = nullptr;
    for (uint64_t i = 0; i < ml;) {
        const uint8_t code = md[i++];
        if (code == 1) {
            if (ml - i < 8) return MH_ERR_CORRUPTED_DATA;
            exp = md + i;
            i += 8;
        } else if (code > 2) {
            return MH_ERR_CORRUPTED_DATA;
        }
        has[code] = true;
    }
    uint64_t o = 0;
    if (has[0]) out[o++] = 0;
    if (has[1]) {
        out[o++] = 1;
        memcpy(out + o, exp, 8);
        o += 8;
    }
    if (has[2]) out[o++] = 2;
    *ol = o;
    return MH_OK;
}

// TxMetadata.ReadFrom + Bytes() (tx_metadata.go:145-193): truncatedUptoTx(0,
// 8 bytes), extra(1, BE16 length + up to 256 bytes).  An extra running past
// the metadata (Go indexes past the slice) or longer than 256 bytes (Bytes()
// slices past its array) panics in Go: corrupted data here.
int tx_md_canonical(const uint8_t *md, uint64_t ml, uint8_t out[MH_MAX_TX_METADATA_LEN],
                    uint64_t *ol) {
    if (ml > MH_MAX_TX_METADATA_LEN) return MH_ERR_CORRUPTED_DATA;
    const uint8_t *trunc = nullptr, *extra = nullptr;
    uint64_t el = 0;
    for (uint64_t i = 0; i < ml;) {
        const uint8_t code = md[i++];
        if (code == 0) {
            if (ml - i < 8) return MH_ERR_CORRUPTED_DATA;
            trunc = md + i;
            i += 8;
        } else if (code == 1) {
            if (ml - i < 2) return MH_ERR_CORRUPTED_DATA;
            el = be_at(md + i, 2);
            i += 2;
            if (ml - i < el || el > 256) return MH_ERR_CORRUPTED_DATA;
            extra = md + i;
            i += el;
        } else {
            return MH_ERR_CORRUPTED_DATA;
        }
    }
    uint64_t o = 0;
    if (trunc) {
        out[o++] = 0;
        memcpy(out + o, trunc, 8);
        o += 8;
    }
    if (extra) {
        out[o++] = 1;
        out[o++] = (uint8_t)(el >> 8);
        out[o++] = (uint8_t)el;
        memcpy(out + o, extra, el);
        o += el;
    }
    *ol = o;
    return MH_OK;
}

// Parse the record at p.  Returns MH_OK and fills h / alh, or
// the structural error; *eof for an id-0 tail or a buffer too short for an id.
// Checks follow the reader's order (tx.go:419-588): lengths are read before
// the metadata they announce is parsed.  patches (may be null): where to note
// non-canonical metadata of this record (index rec).
int hop_record(const uint8_t *buf, uint64_t len, uint64_t p, const HopLimits &lim,
               mh_tx_header &h, uint64_t &alh, bool &eof,
               std::vector<HopPatch> *patches = nullptr, uint64_t rec = 0) {
    eof = false;
    if (p + 8 > len) { eof = true; return MH_OK; }
    memset(&h, 0, sizeof h);
    h.id = be_at(buf + p, 8);
    if (h.id == 0) { eof = true; return MH_OK; }  // preallocated tail, read as EOF (tx.go:427-430)
    if (p + 90 > len) return MH_ERR_TRUNCATED;
    h.ts = (int64_t)be_at(buf + p + 8, 8);
    h.bl_tx_id = be_at(buf + p + 16, 8);
    memcpy(h.bl_root, buf + p + 24, 32);
    memcpy(h.prev_alh, buf + p + 56, 32);
    h.version = (uint32_t)be_at(buf + p + 88, 2);
    uint64_t q = p + 90;
    uint8_t canon[MH_MAX_TX_METADATA_LEN];
    if (h.version == 0) {
        if (q + 2 > len) return MH_ERR_TRUNCATED;
        h.nentries = (uint32_t)be_at(buf + q, 2);
        q += 2;
    } else if (h.version == 1) {
        if (q + 2 > len) return MH_ERR_TRUNCATED;
        h.md_len = (uint32_t)be_at(buf + q, 2);
        q += 2;
        if (h.md_len > MH_MAX_TX_METADATA_LEN) return MH_ERR_CORRUPTED_DATA;
        if (q + h.md_len > len) return MH_ERR_TRUNCATED;
        uint64_t cl = 0;
        if (tx_md_canonical(buf + q, h.md_len, canon, &cl)) return MH_ERR_CORRUPTED_DATA;
        if (patches && (cl != h.md_len || memcmp(canon, buf + q, cl)))
            patches->push_back(HopPatch{rec, 1, 0, std::vector<uint8_t>(canon, canon + cl)});
        if (q + h.md_len + 4 > len) return MH_ERR_TRUNCATED;
        if (q > 0xffffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;
        h.md_off = (uint32_t)q;
        q += h.md_len;
        h.nentries = (uint32_t)be_at(buf + q, 4);
        q += 4;
    } else {
        return MH_ERR_CORRUPTED_UNKNOWN_VERSION;
    }
    if (h.nentries > lim.max_entries) return MH_ERR_CORRUPTED_MAX_ENTRIES;
    for (uint32_t e = 0; e < h.nentries; e++) {
        if (q + 2 > len) return MH_ERR_TRUNCATED;
        const uint64_t ml = be_at(buf + q, 2);
        if (q + 2 + ml > len) return MH_ERR_TRUNCATED;
        uint64_t cml = 0;
        if (ml && kv_md_canonical(buf + q + 2, ml, canon, &cml)) return MH_ERR_CORRUPTED_DATA;
        if (q + 2 + ml + 2 > len) return MH_ERR_TRUNCATED;
        const uint64_t kl = be_at(buf + q + 2 + ml, 2);
        if (kl > lim.max_key_len) return MH_ERR_CORRUPTED_MAX_KEYLEN;
        if (q + 4 + ml + kl + 12 + 32 > len) return MH_ERR_TRUNCATED;
        // a v0 header cannot carry KV metadata: TxEntryDigest_v1_1 fails the
        // read with ErrMetadataUnsupported (tx.go:690-693, via readEntry)
        if (h.version == 0 && ml > 0) return MH_ERR_METADATA_UNSUPPORTED;
        if (patches && ml && (cml != ml || memcmp(canon, buf + q + 2, cml))) {
            // the entry record re-serialised with canonical metadata
            std::vector<uint8_t> r(4 + cml + kl + 12 + 32);
            r[0] = (uint8_t)(cml >> 8);
            r[1] = (uint8_t)cml;
            memcpy(r.data() + 2, canon, cml);
            memcpy(r.data() + 2 + cml, buf + q + 2 + ml, 2 + kl + 12 + 32);
            patches->push_back(HopPatch{rec, 0, e, std::move(r)});
        }
        q += 4 + ml + kl + 12 + 32;
    }
    if (q + 32 > len) return MH_ERR_TRUNCATED;
    alh = q;
    return MH_OK;
}

// Records starting in [p, stop), at most max_recs of them.
void hop_range(const uint8_t *buf, uint64_t len, uint64_t p, uint64_t stop, uint64_t max_recs,
               const HopLimits &lim, HopOut &o) {
    o.start = p;
    while (p < stop && o.R.size() < max_recs) {
        mh_tx_header h;
        uint64_t alh = 0;
        bool eof = false;
        const size_t np = o.P.size();
        const int rc = hop_record(buf, len, p, lim, h, alh, eof, &o.P, o.R.size());
        if (rc != MH_OK || eof) {
            o.P.resize(np);  // patches of a record that did not parse
            o.rc = rc;
            o.stopped = true;
            break;
        }
        o.R.push_back(HopRec{p, alh, h.nentries, 0});
        if (o.want_headers) o.H.push_back(h);
        p = alh + 32;
    }
    o.end = p;
}

// A position that parses as 3 consecutive records with consecutive ids (or
// as records up to the end of the log or a zero tail): where a chunk's speculative parse
// starts.  Only a guess -- the merge accepts a chunk only if the previous
// chunk's parse ended exactly there.
bool zero_run(const uint8_t *buf, uint64_t len, uint64_t p, uint64_t n) {
    const uint64_t e = std::min(len, p + n);
    for (uint64_t k = p; k < e; k++)
        if (buf[k]) return false;
    return true;
}

uint64_t find_record_start(const uint8_t *buf, uint64_t len, uint64_t from, uint64_t to,
                           const HopLimits &lim0) {
    // bounded speculation: a 256 KiB window and candidate records of at most
    // 4096 entries (a miss only costs a sequential re-parse of the chunk)
    const HopLimits lim{std::min<uint32_t>(lim0.max_entries, 4096), lim0.max_key_len};
    to = std::min<uint64_t>(to, from + (256u << 10));
    for (uint64_t q = from; q < to; q++) {
        uint64_t p = q, prev_id = 0;
        int ok = 0;
        for (; ok < 3; ok++) {
            mh_tx_header h;
            uint64_t alh;
            bool eof;
            if (hop_record(buf, len, p, lim, h, alh, eof) != MH_OK) break;
            if (eof) {
                // the end of the log, or a zero-filled preallocated tail after at
                // least one record -- not 8 zero bytes inside a record (a zero
                // vOff field read as an id-0 "tail")
                if (p + 8 <= len && (ok == 0 || !zero_run(buf, len, p, 256))) break;
                ok = 3;
                break;
            }
            if (ok && h.id != prev_id + 1) break;
            prev_id = h.id;
            p = alh + 32;
        }
        if (ok >= 3) return q;
    }
    return ~0ull;
}

// Parked helper threads for the hop (started on first use, kept for the life
// of the process: a validation call runs the hop twice, and starting 15
// threads each time cost about as much as the hop over a quarter of the log).
// run(T, fn) calls fn(k) for k in [0, T): the caller takes tasks too, so a
// pool that could not start threads still finishes.  One run at a time; a
// concurrent caller (another context's hop) gets busy() and starts its own
// threads instead.
class HopPool {
  public:
    static HopPool &get() {
        static HopPool *p = new HopPool();  // never destroyed: its threads stay parked
        return *p;
    }
    bool try_run(unsigned T, const std::function<void(unsigned)> &fn) {
        std::unique_lock<std::mutex> call(call_mu, std::try_to_lock);
        if (!call.owns_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(mu);
            try {
                while (th.size() + 1 < T) {
                    th.emplace_back([this] { loop(); });
                    th.back().detach();
                }
            } catch (...) {  // fewer threads: the caller takes more tasks
            }
            job = &fn;
            next = 0;
            total = T;
            finished = 0;
            failed = false;
        }
        cv_go.notify_all();
        take();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return finished == total; });
        job = nullptr;
        if (failed) throw std::bad_alloc();
        return true;
    }

  private:
    std::mutex call_mu, mu;
    std::condition_variable cv_go, cv_done;
    std::vector<std::thread> th;
    const std::function<void(unsigned)> *job = nullptr;
    unsigned next = 0, total = 0, finished = 0;
    bool failed = false;
    // take tasks until none are left (caller and helpers alike)
    void take() {
        std::unique_lock<std::mutex> lk(mu);
        while (job && next < total) {
            const unsigned k = next++;
            const std::function<void(unsigned)> *f = job;
            lk.unlock();
            bool ok = true;
            try {
                (*f)(k);
            } catch (...) {
                ok = false;
            }
            lk.lock();
            failed |= !ok;
            if (++finished == total) cv_done.notify_all();
        }
    }
    void loop() {
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return job && next < total; });
            }
            take();
        }
    }
};

}  // namespace

// The whole hop: one thread below 1 MiB, else up to 16 threads parse chunks
// from speculated record starts; chunks whose start does not match the
// previous chunk's end are re-parsed sequentially, so the result is always
// the sequential parse's.
void txlog_hop(const uint8_t *buf, uint64_t len, uint64_t max_txs, const HopLimits &lim,
               HopOut &out, bool want_headers) {
    out.want_headers = want_headers;
    // threads: MH_HOP_THREADS from the environment (read once), default 16,
    // never more than the machine has
    static const unsigned kHopThreads = [] {
        const char *e = getenv("MH_HOP_THREADS");
        const long v = e ? strtol(e, nullptr, 10) : 16;
        return (unsigned)std::min(64l, std::max(1l, v));
    }();
    unsigned T = std::min(kHopThreads, std::max(1u, std::thread::hardware_concurrency()));
    // at least 512 KiB per thread (the threads are parked, not started per
    // call: a validation call hops each copy chunk separately, the smallest a
    // few MiB)
    T = (unsigned)std::min<uint64_t>(T, std::max<uint64_t>(1, len >> 19));
    if (T == 1) {
        hop_range(buf, len, 0, ~0ull, max_txs, lim, out);
        return;
    }
    std::vector<uint64_t> cut(T + 1);
    for (unsigned k = 0; k <= T; k++) cut[k] = len / T * k;
    cut[T] = ~0ull;
    std::vector<HopOut> part(T);
    for (auto &pt : part) pt.want_headers = want_headers;
    const std::function<void(unsigned)> work = [&](unsigned k) {
        const uint64_t s = k ? find_record_start(buf, len, cut[k], std::min(cut[k + 1], len), lim) : 0;
        if (s == ~0ull) {
            part[k].start = ~0ull;
            return;
        }
        hop_range(buf, len, s, cut[k + 1], max_txs, lim, part[k]);
    };
    if (!HopPool::get().try_run(T, work)) {
        std::vector<std::thread> th;
        unsigned started = 0;
        try {  // no thread (resource limits): the remaining chunks run on this one
            for (; started + 1 < T; started++) th.emplace_back(work, started + 1);
        } catch (...) {
        }
        work(0);
        for (unsigned k = started + 1; k < T; k++) work(k);
        for (auto &t : th) t.join();
    }
    uint64_t pos = 0;
    out.start = 0;
    for (unsigned k = 0; k < T; k++) {
        if (pos >= cut[k + 1]) continue;  // a record spanning this whole chunk
        HopOut redo, *o = &part[k];
        redo.want_headers = want_headers;
        if (o->start != pos) {            // speculation missed: parse this chunk for real
            hop_range(buf, len, pos, cut[k + 1], max_txs, lim, redo);
            o = &redo;
        }
        const uint64_t room = max_txs - out.R.size();
        const uint64_t take = std::min<uint64_t>(room, o->R.size());
        for (HopPatch &pt : o->P)
            if (pt.rec < take) {
                pt.rec += out.R.size();
                out.P.push_back(std::move(pt));
            }
        out.R.insert(out.R.end(), o->R.begin(), o->R.begin() + take);
        if (want_headers) out.H.insert(out.H.end(), o->H.begin(), o->H.begin() + take);
        // max_txs reached inside or at the end of this chunk: the sequential
        // parse stops before reading the next record, so whatever stopped this
        // chunk's parse after it is not an error of the result
        if (take < o->R.size() || out.R.size() == max_txs) {
            if (take) pos = out.R.back().alh + 32;
            break;
        }
        pos = o->end;
        if (o->stopped) {
            out.rc = o->rc;
            out.stopped = true;
            break;
        }
    }
    out.end = pos;
}

// Structure-only read of a run of tx records (host, no device): the record
// hop of mh_txlog_validate on its own.
extern "C" int mh_txlog_scan(const uint8_t *buf, uint64_t len, uint32_t max_entries,
                             uint32_t max_key_len, uint64_t max_txs, uint64_t *ntx_out,
                             uint64_t *consumed_out, mh_tx_header *hdrs_out,
                             uint64_t *alh_off_out) {
    return mh_guard([&]() -> int {
        if (len && !buf) return MH_ERR_ILLEGAL_ARGUMENTS;
        HopOut hop;
        txlog_hop(buf, len, max_txs, HopLimits{max_entries, max_key_len}, hop, hdrs_out != nullptr);
        const uint64_t ntx = hop.R.size();
        if (ntx_out) *ntx_out = ntx;
        if (consumed_out) *consumed_out = hop.end;
        if (hdrs_out && ntx) memcpy(hdrs_out, hop.H.data(), ntx * sizeof(mh_tx_header));
        if (alh_off_out)
            for (uint64_t k = 0; k < ntx; k++) alh_off_out[k] = hop.R[k].alh;
        return hop.rc;
    });
}
