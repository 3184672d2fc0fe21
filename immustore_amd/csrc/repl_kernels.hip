// repl_kernels.hip -- ImmuStore.ReplicateTx (immustore.go:2772-2932) on CDNA4
// for a run of exported txs: the wire grammar of ExportTx's bytes
// (:2621-2770), the rules of OngoingTx.set (ongoing_tx.go:242-267), the
// hashing of precommit (:1620-1632) and its checks against the exported header
// (:1649-1722).
//
//   TxHeader.ReadFrom, the entry and trailer walk   k_repl_struct, one tx per lane
//   repeated keys                                   k_repl_dup, one entry per lane
//   set / validateAgainst / validateEntries         k_repl_set, one tx per lane
//   hVal, TxEntryDigest_v1_1 / _v1_2                k_repl_leaf, one entry per lane
//   Eh against the header, TxHeader.Alh             k_repl_alh, one tx per lane
//   id, BlRoot == RootAt(BlTxID), PrevAlh           k_repl_verdict / k_repl_final
//
// Cost shape: k_repl_leaf is the call's hashing.  A lane runs (value bytes +
// 9 + 63) / 64 compressions for hVal and 1-3 (up to 17 for a 1 KiB key) for
// the digest, every block's 17 loads guarded to the field; a wave lasts as
// long as its longest value, so a batch of mixed value lengths pays the
// longest of every 64.  k_repl_struct walks a tx's bytes
// serially in one lane (a length is bounds-checked before it is followed, so
// no lane leaves its blob); k_repl_dup compares a key with the earlier keys
// of its tx, lengths first.
#include <algorithm>

#include "tx_alh.hpp"
#include "txlog_common.hpp"

namespace mh {

namespace {

inline unsigned blocks_for(uint64_t threads) { return (unsigned)((threads + 255) / 256); }

__device__ __forceinline__ uint64_t rp_be(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int k = 0; k < n; k++) v = v << 8 | p[k];
    return v;
}

// One exported tx b[0 .. L) at offset boff of the caller's bytes, exactly
// ReplicateTx's reads in its order (immustore.go:2773-2881, tx.go:166-247);
// every length is checked against L before it is followed.  WRITE (the tx
// parsed in the size pass): the header, its canonical metadata and the entry
// records as well.  Returns the status; nent: the entries of a tx that parsed.
template <bool WRITE>
__device__ int repl_parse(const uint8_t *b, uint64_t L, uint64_t boff, uint32_t &nent,
                          mh_tx_header *H, uint8_t *md_slot, uint32_t md_off, uint8_t *trunc_out,
                          mh_replicated_entry *ents) {
    nent = 0;
    if (L < 4) return MH_ERR_ILLEGAL_ARGUMENTS;  // :2773-2781
    const uint64_t hl = rp_be(b, 4);
    if (L < 4 + hl) return MH_ERR_ILLEGAL_ARGUMENTS;  // :2786
    const uint8_t *h = b + 4;
    if (hl < 124) return MH_ERR_ILLEGAL_ARGUMENTS;  // tx.go:168
    const uint64_t id = rp_be(h, 8);
    if (id < 1) return MH_ERR_ILLEGAL_ARGUMENTS;
    const uint32_t ver = (uint32_t)rp_be(h + 48, 2);
    uint64_t j = 50, ne = 0;
    uint32_t mdl = 0;
    const uint8_t *txmd = nullptr;
    if (ver == 0) {
        ne = rp_be(h + j, 2);
        j += 2;
    } else if (ver == 1) {
        mdl = (uint32_t)rp_be(h + j, 2);
        j += 2;
        if (hl < j + mdl + 4 || mdl > MH_MAX_TX_METADATA_LEN) return MH_ERR_CORRUPTED_DATA;
        bool canon;
        if (mdl && tx_md_check(h + j, mdl, &canon)) return MH_ERR_CORRUPTED_DATA;
        txmd = h + j;
        j += mdl;
        ne = rp_be(h + j, 4);
        j += 4;
    } else {
        return MH_ERR_NEWER_VERSION_OR_CORRUPTED;
    }
    if (ne < 1) return MH_ERR_ILLEGAL_ARGUMENTS;
    // Eh, BlTxID, BlRoot: Go zero-fills a short Eh / BlRoot and panics on a short BlTxID
    if (hl < j + 72) return MH_ERR_ILLEGAL_ARGUMENTS;
    const uint64_t bl = rp_be(h + j + 32, 8);
    if (bl >= id) return MH_ERR_ILLEGAL_ARGUMENTS;
    if (WRITE) {
        H->id = id;
        H->ts = (int64_t)rp_be(h + 40, 8);
        H->bl_tx_id = bl;
        for (int k = 0; k < 32; k++) {
            H->prev_alh[k] = h[8 + k];
            H->eh[k] = h[j + k];
            H->bl_root[k] = h[j + 40 + k];
        }
        H->version = ver;
        H->nentries = (uint32_t)ne;
        H->md_len = mdl ? tx_md_canon(txmd, mdl, md_slot) : 0;
        H->md_off = md_off;
    }
    uint64_t i = 4 + hl;
    for (uint64_t e = 0; e < ne; e++) {  // :2806-2856; each turn consumes >= 8 bytes of L
        if (L < i + 8) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint32_t kl = (uint32_t)rp_be(b + i, 2);
        i += 2;
        if (L < i + 6 + kl) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t kp = i;
        i += kl;
        const uint32_t ml = (uint32_t)rp_be(b + i, 2);
        i += 2;
        if (L < i + ml) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t mp = i;
        if (ml) {
            bool canon;
            if (kv_md_check(b + i, ml, &canon)) return MH_ERR_CORRUPTED_DATA;
            i += ml;
        }
        if (L < i + 4) return MH_ERR_ILLEGAL_ARGUMENTS;  // Go reads vLen past the blob: a panic
        const uint32_t vl = (uint32_t)rp_be(b + i, 4);
        i += 4;
        if (L < i + vl) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (WRITE) {
            mh_replicated_entry r;
            r.key_off = boff + kp;
            r.md_off = boff + mp;
            r.val_off = boff + i;
            r.key_len = kl;
            r.md_len = ml;
            r.val_len = vl;
            r.flags = 0;
            ents[e] = r;
        }
        i += vl;
    }
    bool trunc = false;
    if (i < L) {  // :2858-2877
        if (L < i + 2) return MH_ERR_ILLEGAL_ARGUMENTS;  // a 1-byte trailer: Go panics
        const uint32_t tl = (uint32_t)rp_be(b + i, 2);
        i += 2;
        if (L < i + tl) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (tl > 0 && b[i] > 1) return MH_ERR_ILLEGAL_TRUNCATION_ARGUMENT;
        if (tl == 0) return MH_ERR_ILLEGAL_ARGUMENTS;  // Go indexes v[0]
        trunc = b[i] == 1;
        i += tl;
    }
    if (i != L) return MH_ERR_ILLEGAL_ARGUMENTS;
    nent = (uint32_t)ne;
    if (WRITE) {
        *trunc_out = trunc;
        if (trunc)
            for (uint64_t e = 0; e < ne; e++) ents[e].flags = 1;
    }
    return MH_OK;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_repl_struct(ReplGroup g) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.nk) return;
    const uint64_t o = g.tx_off[p], L = g.tx_off[p + 1] - o;
    uint32_t nent;
    if (!WRITE) {
        const int st = repl_parse<false>(g.msgs + o, L, o, nent, nullptr, nullptr, 0, nullptr, nullptr);
        g.status[p] = st;
        g.cnt[p] = st == MH_OK ? nent : 0;
    } else {
        if (g.status[p] != MH_OK) return;
        const uint64_t slot = (g.first + p) * (uint64_t)kMdSlot;
        repl_parse<true>(g.msgs + o, L, o, nent, g.hdr + p, g.md_blob + slot, (uint32_t)slot,
                         g.trunc + p, g.ents + g.ent_off[p]);
    }
}

// the tx that owns group entry t: ent_off[p] <= t < ent_off[p + 1]
__device__ __forceinline__ uint64_t repl_owner(const ReplGroup &g, uint64_t t) {
    uint64_t lo = 0, hi = g.nk;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (g.ent_off[mid + 1] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// entriesByKey (ongoing_tx.go:263-264) decided on the keys themselves
__global__ __launch_bounds__(256) void k_repl_dup(uint64_t T, ReplGroup g) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t p = repl_owner(g, t);
    const mh_replicated_entry *r = g.ents + t;
    const uint32_t kl = r->key_len;
    const uint8_t *key = g.msgs + r->key_off;
    bool dup = false;
    for (uint64_t c = g.ent_off[p]; c < t && !dup; c++) {
        const mh_replicated_entry *e = g.ents + c;
        if (e->key_len != kl) continue;
        const uint8_t *ek = g.msgs + e->key_off;
        bool eq = true;
        for (uint32_t i = 0; eq && i < kl; i++) eq = ek[i] == key[i];
        dup = eq;
    }
    g.dup[t] = dup;
}

__global__ __launch_bounds__(256) void k_repl_set(ReplGroup g, ReplLimits lim) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.nk || g.status[p] != MH_OK) return;
    const bool trunc = g.trunc[p];
    uint64_t held = 0;  // len(tx.entries)
    bool any_md = false;
    int st = MH_OK;
    for (uint64_t e = g.ent_off[p]; e < g.ent_off[p + 1] && st == MH_OK; e++) {
        const mh_replicated_entry *r = g.ents + e;
        if (r->key_len == 0) st = MH_ERR_NULL_KEY;
        else if (r->key_len > lim.max_key_len) st = MH_ERR_MAX_KEY_LEN_EXCEEDED;
        else if (!trunc && r->val_len > lim.max_value_len) st = MH_ERR_MAX_VALUE_LEN_EXCEEDED;
        else if (!g.dup[e]) {
            if (held > lim.max_entries) st = MH_ERR_MAX_TX_ENTRIES_EXCEEDED;  // :265
            else held++;
        }
        any_md |= r->md_len != 0;
    }
    if (st == MH_OK && held != g.hdr[p].nentries) st = MH_ERR_ILLEGAL_ARGUMENTS;  // validateAgainst
    if (st == MH_OK && held > lim.max_entries) st = MH_ERR_MAX_TX_ENTRIES_EXCEEDED;  // validateEntries
    if (st == MH_OK && g.hdr[p].version == 0 && any_md) st = MH_ERR_METADATA_UNSUPPORTED;
    g.status[p] = st;
}

__global__ __launch_bounds__(256) void k_repl_leaf(uint64_t T, ReplGroup g) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t p = repl_owner(g, t);
    if (g.status[p] != MH_OK) return;
    const mh_replicated_entry r = g.ents[t];
    uint32_t hv[8], d[8], pre[4] = {0, 0, 0, 0}, plen = 0;
    const uint8_t *val = g.msgs + r.val_off;
    if (r.flags & 1) {  // digest(value): its first 32 bytes, zero-padded (:3666)
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                w = w << 8 | (4 * j + k < r.val_len ? (uint32_t)val[4 * j + k] : 0u);
            hv[j] = w;
        }
    } else {
        sha256_seg<false>(pre, 0, val, r.val_len, hv, hv);
    }
    if (g.hdr[p].version == 1) {
        // KVMetadata.Bytes(): deleted, expiresAt (the last one read), nonIndexable
        const uint8_t *md = g.msgs + r.md_off;
        bool del = false, ni = false;
        uint32_t ex = 0, has_ex = 0;
        for (uint32_t i = 0; i < r.md_len;) {
            const uint32_t code = md[i++];
            if (code == 0) del = true;
            else if (code == 2) ni = true;
            else {
                ex = i, has_ex = 1;
                i += 8;
            }
        }
        const uint32_t cl = (del ? 1u : 0u) + 9u * has_ex + (ni ? 1u : 0u);
        put_pre(pre, 1, cl);
        uint32_t k = 2;
        if (del) k++;  // the byte 0x00
        if (has_ex) {
            put_pre(pre, k++, 1);
            for (uint32_t i = 0; i < 8; i++) put_pre(pre, k++, md[ex + i]);
        }
        if (ni) put_pre(pre, k++, 2);
        put_pre(pre, k++, r.key_len >> 8);
        put_pre(pre, k++, r.key_len & 0xff);
        plen = k;
    }
    sha256_seg<true>(pre, plen, g.msgs + r.key_off, r.key_len, hv, d);
    store_digest(g.dig + 32 * t, d);
    store_digest(g.hv + 32 * t, hv);
}

__global__ __launch_bounds__(256) void k_repl_alh(ReplGroup g, ReplLimits lim) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.nk) return;
    uint2 *za = (uint2 *)(g.alh + 32 * p);
    int st = g.status[p];
    if (st == MH_OK) {
        const uint2 *eh = (const uint2 *)(g.roots + 32 * p);
        uint2 *he = (uint2 *)g.hdr[p].eh;
        uint32_t x = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x |= (eh[i].x ^ he[i].x) | (eh[i].y ^ he[i].y);
            he[i] = eh[i];  // the header as precommitted
        }
        if (x && !(lim.flags & MH_REPL_SKIP_INTEGRITY)) st = MH_ERR_ILLEGAL_ARGUMENTS;  // :1652
        g.status[p] = st;
    }
    if (st == MH_OK) {
        tx_alh_one(p, g.hdr[p], g.md_blob, g.roots + 32 * p, g.alh_msg + p * kTxInnerStride, nullptr,
                   nullptr, g.alh, nullptr);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) za[i] = make_uint2(0, 0);
    }
}

__global__ __launch_bounds__(256) void k_repl_verdict(uint64_t n, const int32_t *__restrict__ local,
                                                      const mh_tx_header *__restrict__ hdr,
                                                      const uint8_t *__restrict__ alh,
                                                      const uint8_t *__restrict__ dlog, uint64_t P,
                                                      ReplPrev prev, int32_t *__restrict__ full,
                                                      unsigned long long *first_bad) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int st = local[k];
    if (st == MH_OK) {
        const mh_tx_header *h = hdr + k;
        const uint64_t reached = P + k;  // had every earlier tx been accepted
        if (h->id <= reached) {
            st = MH_ERR_TX_ALREADY_COMMITTED;  // :1658
        } else if (h->id > reached + 1) {
            st = MH_ERR_TX_OUT_OF_ORDER;  // :1667, :1715
        } else {
            // RootAt(BlTxID), ahtree.go:749-771; BlTxID < id, so the node lies
            // in the `reached` leaves ahead of this tx
            const uint64_t bl = h->bl_tx_id;
            const uint2 *br = (const uint2 *)h->bl_root;
            uint32_t x = 0;
            if (bl) {
                const uint64_t idx = ahtree_nodes_upto_dev(bl - 1) + (uint64_t)__builtin_popcountll(bl - 1);
                const uint2 *r = (const uint2 *)(dlog + idx * 32);
#pragma unroll
                for (int i = 0; i < 4; i++) x |= (r[i].x ^ br[i].x) | (r[i].y ^ br[i].y);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) x |= br[i].x | br[i].y;
            }
            uint32_t y = 0;
            const uint2 *pa = (const uint2 *)h->prev_alh;
            if (k) {
                const uint2 *a = (const uint2 *)(alh + 32 * (k - 1));
#pragma unroll
                for (int i = 0; i < 4; i++) y |= (a[i].x ^ pa[i].x) | (a[i].y ^ pa[i].y);
            } else {
#pragma unroll
                for (int i = 0; i < 32; i++) y |= (uint32_t)(prev.alh[i] ^ h->prev_alh[i]);
            }
            if (x || y) st = MH_ERR_ILLEGAL_ARGUMENTS;  // :1684, :1719
        }
    }
    full[k] = st;
    if (st != MH_OK) atomicMin(first_bad, (unsigned long long)k);
}

__global__ __launch_bounds__(256) void k_repl_final(uint64_t n, const int32_t *__restrict__ local,
                                                    int32_t *__restrict__ full,
                                                    const unsigned long long *first_bad) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || k <= *first_bad) return;
    full[k] = local[k] != MH_OK ? local[k] : MH_ERR_TX_NOT_REACHED;
}

}  // namespace

hipError_t launch_repl_struct(hipStream_t st, Timer *tm, bool write, const ReplGroup &g) {
    if (!g.nk) return hipSuccess;
    TimerScope ts(tm, write ? "repl_struct_write" : "repl_struct_size", st);
    if (write) hipLaunchKernelGGL(k_repl_struct<true>, dim3(blocks_for(g.nk)), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_repl_struct<false>, dim3(blocks_for(g.nk)), dim3(256), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_repl_set(hipStream_t st, Timer *tm, uint64_t T, const ReplGroup &g,
                           const ReplLimits &lim) {
    if (!g.nk || !T) return hipSuccess;
    TimerScope ts(tm, "repl_set", st);
    hipLaunchKernelGGL(k_repl_dup, dim3(blocks_for(T)), dim3(256), 0, st, T, g);
    hipLaunchKernelGGL(k_repl_set, dim3(blocks_for(g.nk)), dim3(256), 0, st, g, lim);
    return hipGetLastError();
}

hipError_t launch_repl_leaf(hipStream_t st, Timer *tm, uint64_t T, const ReplGroup &g) {
    if (!T) return hipSuccess;
    TimerScope ts(tm, "repl_leaf", st);
    hipLaunchKernelGGL(k_repl_leaf, dim3(blocks_for(T)), dim3(256), 0, st, T, g);
    return hipGetLastError();
}

hipError_t launch_repl_alh(hipStream_t st, Timer *tm, const ReplGroup &g, const ReplLimits &lim) {
    if (!g.nk) return hipSuccess;
    TimerScope ts(tm, "repl_alh", st);
    hipLaunchKernelGGL(k_repl_alh, dim3(blocks_for(g.nk)), dim3(256), 0, st, g, lim);
    return hipGetLastError();
}

hipError_t launch_repl_verdict(hipStream_t st, Timer *tm, uint64_t n, const int32_t *local,
                               const mh_tx_header *hdr, const uint8_t *alh, const uint8_t *dlog,
                               uint64_t P, const ReplPrev &prev, int32_t *full,
                               unsigned long long *first_bad) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "repl_verdict", st);
    hipLaunchKernelGGL(k_repl_verdict, dim3(blocks_for(n)), dim3(256), 0, st, n, local, hdr, alh, dlog,
                       P, prev, full, first_bad);
    hipLaunchKernelGGL(k_repl_final, dim3(blocks_for(n)), dim3(256), 0, st, n, local, full, first_bad);
    return hipGetLastError();
}

}  // namespace mh
