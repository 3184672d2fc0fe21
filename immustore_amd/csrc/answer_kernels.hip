// answer_kernels.hip -- whole VerifiableTx / VerifiableEntry answers built on
// the device (capi_answer.hip drives them):
//
//   VerifiableTx     schema.proto:499-508   db.VerifiableTxByID   database.go:1462-1528
//   VerifiableEntry  schema.proto:523-532   db.VerifiableGet      database.go:817-896
//   Tx, TxEntry      schema.proto:451-481   TxToProto / TxEntryToProto database_protoconv.go:27-49
//   KVMetadata       schema.proto:483-497   KVMetadataToProto     database_protoconv.go:51-67
//   InclusionProof   schema.proto:534-543   Tx.Proof tx.go:357-368, htree.go:121-164
//
// The requests name txs; the kernels here find the txs a batch reads (a bitmap
// over the store, scanned and compacted: every distinct tx is read and hashed
// once), settle each request's status in Go's order, lay every message out in
// a size pass (length prefixes nest four deep) and write it: schema.Tx once
// per distinct asked tx, a lane per entry, then a wave per answer that copies
// it in and gathers the inclusion terms.  The DualProof bytes are the v1
// writer's (wire_kernels.hip) over the RankWindow this file fills.
//
// A tx record (immustore.go:1812-1924): id 8 | ts 8 | blTxID 8 | blRoot 32 |
// prevAlh 32 | version 2 | [v1: mdLen 2, md] | nentries 2 (v0) / 4 (v1) |
// entries | Alh 32; an entry: mdLen 2 | md | kLen 2 | key | vLen 4 | vOff 8 |
// hVal 32.  Entries are only walked in records that passed the structure
// pass of the read path, which checked every length against the log.
#include <algorithm>

#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "answer_common.hpp"
#include "pb_write.hpp"
#include "proof_walk.hpp"
#include "sha256_cdna.hpp"

namespace mh {

namespace {

// nodes of the flat level layout of a tree of width w (htree.go:85-110)
__device__ __forceinline__ uint64_t levels_len_dev(uint64_t w) {
    return w ? level_off(w, bits_len(w - 1) + 1) : 0;
}

// ---------------------------------------------------------------- the read set
// id and BlTxID of tx x as its record stores them, located by the cLog; false
// when the entry points outside the log (the record's verdict says why)
__device__ __forceinline__ bool ans_head(const AnsArrays &a, uint64_t x, uint64_t &id, uint64_t &bl) {
    const uint8_t *ce = a.clog + (x - 1) * a.es;
    const uint64_t off = be_dev(ce, 8), size = be_dev(ce + 8, 4);
    if (off > a.txlog_len || size > a.txlog_len - off || size < 24) return false;
    id = be_dev(a.txlog + off, 8);
    bl = be_dev(a.txlog + off + 16, 8);
    return true;
}

// txs lo .. hi, clipped to the store, a word of the bitmap at a time
__device__ __forceinline__ void ans_mark(const AnsArrays &a, uint64_t lo, uint64_t hi) {
    if (lo < 1) lo = 1;
    if (hi > a.ntx) hi = a.ntx;
    if (lo > hi) return;
    const uint64_t b0 = lo - 1, b1 = hi - 1;
    for (uint64_t w = b0 >> 6; w <= b1 >> 6; w++) {
        uint64_t m = ~0ull;
        if (w == b0 >> 6) m &= ~0ull << (b0 & 63);
        if (w == b1 >> 6) m &= ~0ull >> (63 - (b1 & 63));
        if ((a.bits[w] & m) != m) atomicOr((unsigned long long *)&a.bits[w], (unsigned long long)m);
    }
}

// Steps 1 and 2 (the ids) of the status list, and the reads of the request:
// T, S and what ImmuStore.DualProof(src, tgt) reads (immustore.go:2431, :2446,
// :2452).  The ranges are only followed when both heads can be read; when
// not, the request fails before its proof.
// The ranges come from id / BlTxID fields of records that are not validated
// yet.  In a sound store they are as long as the binary-linking lag of src and
// tgt; a record that claims another BlTxID can stretch them up to the whole
// store.  Everything is clipped to [1, N], so that is safe, and no tx is
// hashed twice for it, but it is not cheap: the call then re-hashes up to N
// records and RankWindow::check walks the claimed range once per request.
// The cost is what Go pays for the same record (its readers walk the same
// ranges); it is not capped here, because a cap would change the status of a
// request whose lag is honestly long.
__global__ __launch_bounds__(256) void k_ans_heads(const AnsArrays a) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const uint64_t T = a.tx[p], S = a.since[p], N = a.ntx;
    int32_t st = MH_OK;
    if (S > N) st = MH_ERR_ILLEGAL_STATE;              // database.go:1467
    else if (T == 0) st = MH_ERR_ILLEGAL_ARGUMENTS;    // immustore.go:2570
    else if (T > N) st = MH_ERR_TX_NOT_FOUND;          // immustore.go:3000
    a.pre[p] = st;
    if (st) return;
    ans_mark(a, T, T);
    if (S) ans_mark(a, S, S);
    uint64_t tid, tbl, rid, rbl;
    if (!ans_head(a, T, tid, tbl)) return;
    rid = tid, rbl = tbl;
    if (S && !ans_head(a, S, rid, rbl)) return;
    const bool fwd = S <= T;
    const uint64_t sid = fwd ? rid : tid, sbl = fwd ? rbl : tbl, gid = fwd ? tid : rid,
                   gbl = fwd ? tbl : rbl;
    if (gbl) ans_mark(a, gbl, gbl);
    ans_mark(a, sid > gbl ? sid : gbl, gid);
    ans_mark(a, sbl + 1, sid < gbl ? sid : gbl);
}

__global__ __launch_bounds__(256) void k_ans_popc(const AnsArrays a) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < a.words) a.wcnt[w] = (uint64_t)__popcll(a.bits[w]);
}

// a lane per tx of the store: a tx that is read puts its id and its cLog
// entry into its slot
__global__ __launch_bounds__(256) void k_ans_compact(const AnsArrays a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.ntx || !((a.bits[b >> 6] >> (b & 63)) & 1)) return;
    const uint64_t j = ans_slot(a, b + 1);
    a.ids[j] = b + 1;
    const uint8_t *src = a.clog + b * a.es;
    uint8_t *dst = a.gclog + j * a.es;
    for (uint32_t k = 0; k < a.es; k++) dst[k] = src[k];
}

// ---------------------------------------------------------------- verdicts
// Steps 2 and 3: ReadTx(T), ReadTxHeader(S) -- the record verdicts of the read
// path -- and the headers of DualProof(src, tgt).  A request that fails gets
// zero headers (the proof writer skips it: src.ID == 0).
__global__ __launch_bounds__(256) void k_ans_verdict(const AnsArrays a) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    int32_t st = a.pre[p];
    const uint64_t T = a.tx[p], S = a.since[p];
    uint64_t jt = 0, jr = 0;
    if (!st) {
        jt = jr = ans_slot(a, T);
        st = a.rst[jt];
        if (!st && S) {
            jr = ans_slot(a, S);
            st = a.rst[jr];
        }
    }
    a.pre[p] = st;
    a.leaf[p] = 0;
    uint64_t *ds = reinterpret_cast<uint64_t *>(a.hs + p), *dt = reinterpret_cast<uint64_t *>(a.ht + p);
    constexpr int kW = sizeof(MhTxHeader) / 8;
    if (st) {
        for (int k = 0; k < kW; k++) ds[k] = dt[k] = 0;
        return;
    }
    const bool fwd = S <= T;  // database.go:1506-1512
    const uint64_t *s = reinterpret_cast<const uint64_t *>(a.hd + (fwd ? jr : jt)),
                   *t = reinterpret_cast<const uint64_t *>(a.hd + (fwd ? jt : jr));
    for (int k = 0; k < kW; k++) {
        ds[k] = s[k];
        dt[k] = t[k];
    }
    atomicOr(a.flags + jt, a.kind[p] == MH_ANS_ENTRY ? 3u : 1u);
}

// tx_reader.go:87-89 for every slot whose predecessor holds the tx before it
__global__ __launch_bounds__(256) void k_ans_link(const AnsArrays a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.D) return;
    bool bad = false;
    if (j && a.ids[j - 1] + 1 == a.ids[j] && !a.rst[j] && !a.rst[j - 1]) {
        const uint8_t *x = a.hd[j].prev_alh, *y = a.alh + 32 * (j - 1);
        for (int k = 0; k < 32; k++) bad |= x[k] != y[k];
    }
    a.lnk[j] = bad;
}

// entries to index (and where they start) and tree nodes to build, per slot
__global__ __launch_bounds__(256) void k_ans_counts(const AnsArrays a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.D) return;
    const uint32_t f = a.flags[j];
    const uint64_t w = f & 1 ? a.hd[j].nentries : 0;
    a.ecnt[j] = w;
    a.ncnt[j] = f & 2 ? levels_len_dev(w) : 0;
    // (k_txe_index walks the entries from here; the read path took the record)
    a.ent_start[j] = w ? be_dev(a.gclog + j * a.es, 8) + (a.hd[j].version ? 96 + a.hd[j].md_len : 92) : 0;
}

// ---------------------------------------------------------------- trees
// The levels of the tx's htree in the flat layout (htree.go:85-110: an odd
// last node is promoted), one wave per tx an ENTRY request asks about.
// Not build_many_dev: its small-tree arm keeps the roots only, and its plan
// arm lays level l of ALL trees side by side from a plan built on the host out
// of leaf_off (D + 1 offsets down, three index arrays up, a wait), where an
// inclusion walk would need a base per tree and level; here each tree's nodes
// lie in the one layout htree_walk indexes, found by one scanned offset.
__global__ __launch_bounds__(64) void k_ans_trees(const AnsArrays a) {
    const uint64_t j = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t nn = a.lvl_off[j + 1] - a.lvl_off[j];
    if (!nn) return;
    const uint64_t w = a.leaf_off[j + 1] - a.leaf_off[j];
    uint8_t *lv = a.nodes + 32 * a.lvl_off[j];
    const uint8_t *dg = a.dig + 32 * a.leaf_off[j];
    for (uint64_t i = lane; i < w; i += 64) {
        uint32_t d[8], h[8];
        load_digest(dg + 32 * i, d);
        leaf_hash(d, h);
        store_digest(lv + 32 * i, h);
    }
    uint64_t pw = w, poff = 0;
    while (pw > 1) {
        __threadfence_block();
        __syncthreads();
        const uint64_t cw = (pw + 1) / 2, coff = poff + pw;
        for (uint64_t i = lane; i < cw; i += 64) {
            uint32_t l[8], r[8], h[8];
            load_digest(lv + 32 * (poff + 2 * i), l);
            if (2 * i + 1 < pw) {
                load_digest(lv + 32 * (poff + 2 * i + 1), r);
                node_hash(l, r, h);
                store_digest(lv + 32 * (coff + i), h);
            } else {
                store_digest(lv + 32 * (coff + i), l);
            }
        }
        pw = cw;
        poff = coff;
    }
}

// ---------------------------------------------------------------- entries
__global__ __launch_bounds__(256) void k_ans_esize(const AnsArrays a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    a.esz[e] = framed(ans_entry(a.txlog + a.rec_off[e]).body);
}

// Step 4, Tx.IndexOf (tx.go:361-368): the first entry whose key equals the
// asked key.  One wave per ENTRY request, a lane per entry.
__global__ __launch_bounds__(256) void k_ans_find(const AnsArrays a) {
    const uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= a.n || a.kind[p] != MH_ANS_ENTRY || a.pre[p]) return;  // wave-uniform
    const uint64_t j = ans_slot(a, a.tx[p]);
    const uint64_t e0 = a.leaf_off[j], w = a.leaf_off[j + 1] - e0;
    const uint8_t *key = a.keys + a.key_off[p];
    const uint64_t kl = a.key_off[p + 1] - a.key_off[p];
    uint64_t found = ~0ull;
    for (uint64_t i0 = 0; i0 < w && found == ~0ull; i0 += 64) {
        bool eq = false;
        if (i0 + lane < w) {
            const uint8_t *r = a.txlog + a.rec_off[e0 + i0 + lane];
            const uint32_t ml = ((uint32_t)r[0] << 8) | r[1];
            const uint32_t k2 = ((uint32_t)r[2 + ml] << 8) | r[3 + ml];
            eq = k2 == kl;
            for (uint32_t k = 0; eq && k < k2; k++) eq = r[4 + ml + k] == key[k];
        }
        const uint64_t m = __ballot(eq);
        if (m) found = i0 + (uint64_t)(__ffsll((unsigned long long)m) - 1);
    }
    if (lane == 0) {
        if (found == ~0ull)
            a.pre[p] = MH_ERR_KEY_NOT_FOUND;
        else
            a.leaf[p] = found;
    }
}

// ---------------------------------------------------------------- sizes
__global__ __launch_bounds__(256) void k_ans_txsize(const AnsArrays a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.D) return;
    uint64_t body = 0;
    uint32_t hsz = 0;
    if (a.flags[j] & 1) {
        const PbHdr h = pb_header(a.hd[j], a.txlog);
        if (!h.st) {  // (else the DualProof writer reports the metadata)
            hsz = framed(h.body);
            body = hsz + (a.epos[a.leaf_off[j + 1]] - a.epos[a.leaf_off[j]]);
        }
    }
    a.hsz[j] = hsz;
    a.txbody[j] = body;
}

// the layout of answer p (status MH_OK)
struct AnsLayout {
    uint64_t j, txb, dp, vtx, elen, leaf, width;
    uint32_t nterms, incl_body;
    uint64_t total;
};

__device__ inline AnsLayout ans_layout(const AnsArrays &a, uint64_t p) {
    AnsLayout L;
    L.j = ans_slot(a, a.tx[p]);
    L.txb = a.txbody[L.j];
    L.dp = a.dp_off[p + 1] - a.dp_off[p];
    L.vtx = framed_u64(L.txb) + framed_u64(L.dp);
    L.total = L.vtx;
    L.elen = L.leaf = L.width = 0;
    L.nterms = L.incl_body = 0;
    if (a.kind[p] == MH_ANS_ENTRY) {
        L.elen = a.entry_off[p + 1] - a.entry_off[p];
        L.leaf = a.leaf[p];
        L.width = a.leaf_off[L.j + 1] - a.leaf_off[L.j];
        L.nterms = htree_walk(L.leaf, L.width, [](uint32_t, uint64_t) {});
        L.incl_body = ((uint32_t)L.leaf ? 1 + vlen(i32v((uint32_t)L.leaf)) : 0) +
                      ((uint32_t)L.width ? 1 + vlen(i32v((uint32_t)L.width)) : 0) + 34 * L.nterms;
        L.total = (L.elen ? framed_u64(L.elen) : 0) + framed_u64(L.vtx) + framed(L.incl_body);
    }
    return L;
}

// Steps 4 to 7 joined: the request's status and its message length
__global__ __launch_bounds__(256) void k_ans_size(const AnsArrays a) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    int32_t st = a.pre[p] ? a.pre[p] : a.dst[p];
    uint64_t s = 0;
    if (!st) {
        const AnsLayout L = ans_layout(a, p);
        if (!L.txb)
            st = MH_ERR_CORRUPTED_DATA;  // header metadata the writer cannot encode
        else
            s = L.total;
    }
    a.status[p] = st;
    a.sizes[p] = s;
}

// ---------------------------------------------------------------- schema.Tx, once per tx
__global__ __launch_bounds__(256) void k_ans_tx_header(const AnsArrays a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.D || !a.txbody[j]) return;
    const PbHdr h = pb_header(a.hd[j], a.txlog);
    ByteWriter bw(a.txbuf + a.txpos[j]);
    put_header(bw, 0x0a, a.hd[j], h, a.txlog);
    bw.finish();
}

__global__ __launch_bounds__(256) void k_ans_tx_entries(const AnsArrays a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    uint64_t j = 0, hi = a.D;  // the slot of entry e: the last j with leaf_off[j] <= e
    while (hi - j > 1) {
        const uint64_t mid = j + (hi - j) / 2;
        if (a.leaf_off[mid] <= e) j = mid; else hi = mid;
    }
    if (!a.txbody[j]) return;
    const uint8_t *r = a.txlog + a.rec_off[e];
    const AnsEntry t = ans_entry(r);
    ByteWriter bw(a.txbuf + a.txpos[j] + a.hsz[j] + (a.epos[e] - a.epos[a.leaf_off[j]]));
    bw.put8(0x12);
    bw.varint(t.body);
    put_entry_fields(bw, r, t);
    bw.finish();
}

// ---------------------------------------------------------------- the answers
// One wave per answer: the length prefixes on lane 0, the caller's Entry and
// the encoded Tx copied by the wave, the inclusion terms a lane per term.
// Leaves where the DualProof goes in dpos[p].
__global__ __launch_bounds__(64) void k_ans_assemble(const AnsArrays a) {
    __shared__ uint64_t idx[64];
    const uint64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    a.dpos[p] = 0;
    if (a.status[p] != MH_OK) return;  // wave-uniform
    if (a.off[p + 1] > a.out_cap) {
        if (lane == 0) a.status[p] = MH_ERR_BUFFER_TOO_SMALL;
        return;
    }
    const AnsLayout L = ans_layout(a, p);
    const bool ent = a.kind[p] == MH_ANS_ENTRY;
    uint8_t *o = a.out + a.off[p];
    uint8_t *vtx = o;
    if (ent) {
        const uint64_t ef = L.elen ? framed_u64(L.elen) : 0;
        if (L.elen) {
            if (lane == 0) {
                ByteWriter bw(o);
                bw.put8(0x0a);
                bw.varint(L.elen);
                bw.finish();
            }
            wave_copy(o + 1 + vlen(L.elen), a.entries + a.entry_off[p], L.elen, lane);
        }
        if (lane == 0) {
            ByteWriter bw(o + ef);
            bw.put8(0x12);
            bw.varint(L.vtx);
            bw.finish();
        }
        vtx = o + ef + 1 + vlen(L.vtx);
    }
    uint8_t *txm = vtx + 1 + vlen(L.txb), *dpp = txm + L.txb;
    if (lane == 0) {
        ByteWriter bw(vtx);
        bw.put8(0x0a);
        bw.varint(L.txb);
        bw.finish();
        ByteWriter bd(dpp);
        bd.put8(0x12);
        bd.varint(L.dp);
        bd.finish();
        a.dpos[p] = (uint64_t)(dpp + 1 + vlen(L.dp) - a.out);
    }
    wave_copy(txm, a.txbuf + a.txpos[L.j], L.txb, lane);
    if (!ent) return;
    uint8_t *ip = vtx + L.vtx;
    if (lane == 0) {
        ByteWriter bw(ip);
        bw.put8(0x1a);
        bw.varint(L.incl_body);
        if ((uint32_t)L.leaf) { bw.put8(0x08); bw.varint(i32v((uint32_t)L.leaf)); }
        if ((uint32_t)L.width) { bw.put8(0x10); bw.varint(i32v((uint32_t)L.width)); }
        bw.finish();
        htree_walk(L.leaf, L.width, [&](uint32_t q, uint64_t node) {
            if (q < 64) idx[L.nterms - 1 - q] = node;
        });
    }
    __syncthreads();
    if ((uint32_t)lane < L.nterms) {
        uint8_t *rec = ip + framed(L.incl_body) - 34 * L.nterms + 34 * lane;
        uint32_t x[8];
        load_node(a.nodes + 32 * (a.lvl_off[L.j] + idx[lane]), x);
        put_rec34_as<1>(rec, 0x1a, x);
    }
}

}  // namespace

hipError_t launch_ans_heads(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_heads", k_ans_heads, grid_for(a.n, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_popc(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_popc", k_ans_popc, grid_for(a.words, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_compact(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_compact", k_ans_compact, grid_for(a.ntx, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_verdict(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_verdict", k_ans_verdict, grid_for(a.n, 256), 256, a);
    MH_LAUNCH("ans_link", k_ans_link, grid_for(a.D, 256), 256, a);
    MH_LAUNCH("ans_counts", k_ans_counts, grid_for(a.D, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_trees(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_trees", k_ans_trees, (unsigned)a.D, 64, a);
    return hipSuccess;
}

hipError_t launch_ans_find(hipStream_t st, Timer *tm, const AnsArrays &a) {
    if (a.E) MH_LAUNCH("ans_esize", k_ans_esize, grid_for(a.E, 256), 256, a);
    MH_LAUNCH("ans_find", k_ans_find, grid_for(a.n, 4), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_txsize(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_txsize", k_ans_txsize, grid_for(a.D, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_size(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_size", k_ans_size, grid_for(a.n, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_tx_write(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_tx_header", k_ans_tx_header, grid_for(a.D, 256), 256, a);
    if (a.E) MH_LAUNCH("ans_tx_entries", k_ans_tx_entries, grid_for(a.E, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_ans_assemble(hipStream_t st, Timer *tm, const AnsArrays &a) {
    MH_LAUNCH("ans_assemble", k_ans_assemble, (unsigned)a.n, 64, a);
    return hipSuccess;
}

}  // namespace mh
