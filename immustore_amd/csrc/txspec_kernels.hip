// txspec_kernels.hip -- db.serializeTx (database.go:1080-1231) on CDNA4 for the
// answers of db.TxByID (:1034-1063), db.TxScan (:1531-1583) and
// db.VerifiableTxByID (:1462-1528) under an EntriesSpec (capi_txspec.hip drives
// them).  The read set, the record re-hash and the DualProof are the answer
// path's (answer_kernels.hip, wire_kernels.hip); here the entries of the asked
// txs are classified by key[0] and action, ImmuStore.ReadValue (immustore.go:
// 3149-3179) reads every value where it lies in its value log, readValueAt
// (:3183-3240) checks it, and schema.Tx is laid down with the values as field 5
// of their TxEntry.
//
//   the slot and width of a variant's tx; no DualProof
//     for a TX request                              k_txs_variants, k_txs_heads
//   class, action, expiry, decodeOffset, the value's
//     availability, the TxEntry's length, the lowest
//     entry that fails without a hash               k_txs_plan, one item per lane
//   the entries' places, the Tx's length            k_txs_vsize, one variant per wave
//   statuses so far, the answers' lengths           k_txs_size, one request per lane
//   where each Tx is written                        k_txs_place, one variant per lane
//   TxHeader; key, hValue, vLen, metadata and the
//     tag and length of field 5                     k_txs_header, k_txs_entries
//   SHA-256 of the value against hVal, its bytes    k_txs_values, one value per lane
//   the value for the other variants of its group   k_txs_copy, one value per wave
//   the length prefixes, a shared Tx copied in      k_txs_assemble, one answer per wave
//   the statuses in Go's order                      k_txs_status, one request per lane
//
// A variant is a distinct (tx, actions) pair of the batch, a group a distinct
// (tx, classes read) pair: a Tx is laid out once per variant and a value hashed
// once per group, by the lanes of the group's first variant.  A variant one
// request asks for is written straight into that answer; one that several ask
// for goes to txbuf and a wave per answer copies it in.
//
// Cost shape: k_txs_values is the call's hashing, the value_lane (value_store.hpp)
// of export_kernels.hip's k_exp_values<true> with another destination
// (TxsValues): a lane runs (vLen + 9 + 63) / 64 compressions and stores each 64-byte block it has turned into message
// words, lanes take values in length-class order.  Every byte of a Tx is
// written by exactly one lane, and a dword only by the lane that owns all four
// of its bytes.
#include "answer_common.hpp"
#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "msg_walk.hpp"
#include "pb_write.hpp"
#include "sha256_cdna.hpp"
#include "txlog_common.hpp"
#include "value_store.hpp"

namespace mh {

namespace {

constexpr uint64_t kNoSlot = ~0ull;

// the entry record of item i of variant v
__device__ __forceinline__ const uint8_t *txs_record(const AnsArrays &a, const TxsArrays &x, uint64_t v,
                                                     uint64_t i) {
    return a.txlog + a.rec_off[a.leaf_off[x.vslot[v]] + (i - x.item_off[v])];
}

__global__ __launch_bounds__(256) void k_txs_variants(const AnsArrays a, const TxsArrays x) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= x.V) return;
    const uint64_t T = x.vtx[v];
    uint64_t j = kNoSlot, w = 0;
    // (a tx no request got as far as reading is not in the read set)
    if (T >= 1 && T <= a.ntx && ((a.bits[(T - 1) >> 6] >> ((T - 1) & 63)) & 1)) {
        j = ans_slot(a, T);
        w = a.ecnt[j];  // (0 unless a request read the tx: k_ans_verdict, k_ans_counts)
    }
    x.vslot[v] = j;
    x.vw[v] = w;
    x.early_idx[v] = kExpNone;
    x.early_st[v] = MH_OK;
}

// db.TxByID proves nothing: a TX request gets zero headers, which the DualProof
// writer skips (src.ID == 0)
__global__ __launch_bounds__(256) void k_txs_heads(const AnsArrays a, const TxsArrays x) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n || x.kind[p] == MH_TXA_VERIFIABLE) return;
    uint64_t *ds = reinterpret_cast<uint64_t *>(a.hs + p), *dt = reinterpret_cast<uint64_t *>(a.ht + p);
    for (int k = 0; k < (int)(sizeof(MhTxHeader) / 8); k++) ds[k] = dt[k] = 0;
}

// One entry under its variant's actions: serializeTx's switch on key[0], then
// ReadValue: expiry, the empty value, decodeOffset (immustore.go:1429-1431:
// Go's mask is 0xff << 55) and readValueAt's and multiapp.ReadAt's ways to
// io.EOF.
__global__ __launch_bounds__(256) void k_txs_plan(const AnsArrays a, const TxsArrays x) {
    const uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= x.I) return;
    const uint64_t v = owner_of(x.item_off, x.V, it);
    const uint8_t *r = txs_record(a, x, v, it);
    const AnsEntry t = ans_entry(r);
    const uint32_t mode = x.vmode[v];
    uint8_t kind = kTxsDigest;  // TxToProto: every entry
    int32_t fail = MH_OK;
    if (mode != kTxsNoSpec) {
        if (!t.kl) {
            kind = kTxsDrop;
            fail = MH_ERR_ILLEGAL_STATE;  // Go indexes e.Key()[0]
        } else {
            const uint8_t c = r[4 + t.ml];
            const uint32_t act = c == 0 ? mode & 3 : c == 1 ? (mode >> 2) & 3 : c == 2 ? (mode >> 4) & 3 : 0;
            kind = act == 1 ? kTxsDigest : act == 2 ? kTxsValue : kTxsDrop;
            if (act == 3) fail = MH_ERR_ILLEGAL_ARGUMENTS;  // SQL only (database.go:1225)
        }
    }
    uint64_t L = 0;
    const uint8_t *src = nullptr;
    if (kind == kTxsValue) {
        if (t.has_exp && (int64_t)t.exp <= x.now) {
            kind = kTxsDrop;  // ErrExpiredEntry: nothing is read
        } else if (!t.vlen) {
            kind = kTxsDigest;  // immustore.go:3162: no read, no digest check
        } else {
            const uint64_t voff = be_dev(r + 8 + t.ml + t.kl, 8);
            const uint32_t id = (uint32_t)(voff >> 56);
            const uint64_t at = voff & ~(0xffull << 55);
            if (id == 0) {
                fail = MH_ERR_EOF;  // :3186
            } else if (id > x.nvlogs) {
                fail = MH_ERR_ILLEGAL_STATE;
            } else {
                const ExpVlog g = x.vlogs[id - 1];
                if (at >= g.first_off && at <= g.end_off && t.vlen <= g.end_off - at) {
                    src = g.data + (at - g.first_off);
                    L = t.vlen;
                } else {
                    fail = MH_ERR_EOF;
                }
            }
            if (fail) kind = kTxsDrop;
        }
    }
    const uint64_t body = (uint64_t)t.body + (kind == kTxsValue ? 1 + vlen(L) + L : 0);
    const bool hash = kind == kTxsValue && x.vprim[v];
    x.ikind[it] = kind;
    x.ifail[it] = (uint8_t)fail;
    x.isz[it] = kind == kTxsDrop ? 0 : framed_u64(body);
    x.vsrc[it] = src;
    x.vlen[it] = hash ? L : 0;
    x.skip[it] = !hash;
    if (fail) atomicMin(x.early_idx + v, (uint32_t)(it - x.item_off[v]));
}

// One variant per wave: where its entries go, its Tx's length, the status of
// its lowest entry that fails without a hash
__global__ __launch_bounds__(256) void k_txs_vsize(const AnsArrays a, const TxsArrays x) {
    const uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (v >= x.V) return;  // wave-uniform
    const uint64_t i0 = x.item_off[v], w = x.item_off[v + 1] - i0;
    uint64_t ebytes = 0;
    for (uint64_t k0 = 0; k0 < w; k0 += 64) {
        const uint64_t k = k0 + lane;
        unsigned long long s = k < w ? x.isz[i0 + k] : 0;
        const unsigned long long own = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {  // inclusive scan across the wave
            const unsigned long long y = __shfl_up(s, d, 64);
            if ((int)lane >= d) s += y;
        }
        if (k < w) x.ipos[i0 + k] = ebytes + (s - own);
        ebytes += __shfl(s, 63, 64);
    }
    if (lane) return;
    const uint64_t j = x.vslot[v];
    const uint32_t ei = x.early_idx[v];
    uint64_t body = 0;
    uint32_t hsz = 0;
    if (j != kNoSlot && (a.flags[j] & 1)) {
        const PbHdr h = pb_header(a.hd[j], a.txlog);
        if (!h.st) {
            hsz = framed(h.body);
            body = hsz + ebytes;
        }
    }
    if (ei != kExpNone) x.early_st[v] = x.ifail[i0 + ei];
    x.vbody[v] = body;
    x.vhsz[v] = hsz;
    x.vshare[v] = x.vcnt[v] > 1 && body && ei == kExpNone ? body : 0;
}

// What is settled before a value is hashed: pre = the statuses ahead of
// serializeTx, status = those and the lowest entry that fails without a hash
// (such a request owns an empty range)
__global__ __launch_bounds__(256) void k_txs_size(const AnsArrays a, const TxsArrays x) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const bool ver = x.kind[p] == MH_TXA_VERIFIABLE;
    const uint64_t v = x.rv[p];
    int32_t pre = a.pre[p];
    if (!pre && ver) pre = a.dst[p];
    if (!pre && !x.vbody[v]) pre = MH_ERR_CORRUPTED_DATA;  // header metadata the writer cannot encode
    int32_t st = pre;
    uint64_t s = 0;
    if (!st) {
        if (x.early_idx[v] != kExpNone) st = x.early_st[v];
        else s = ver ? framed_u64(x.vbody[v]) + framed_u64(a.dp_off[p + 1] - a.dp_off[p]) : x.vbody[v];
    }
    a.pre[p] = pre;
    a.status[p] = st;
    a.sizes[p] = s;
}

__global__ __launch_bounds__(256) void k_txs_place(const AnsArrays a, const TxsArrays x) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= x.V) return;
    uint8_t *d = nullptr;
    if (x.vbody[v] && x.early_idx[v] == kExpNone) {
        if (x.vcnt[v] > 1) {
            d = x.txbuf + x.vpos[v];
        } else {
            const uint64_t p = x.vfirst[v];
            if (a.status[p] == MH_OK && a.off[p + 1] <= a.out_cap)
                d = a.out + a.off[p] + (x.kind[p] == MH_TXA_VERIFIABLE ? 1 + vlen(x.vbody[v]) : 0);
        }
    }
    x.vdst[v] = d;
}

__global__ __launch_bounds__(256) void k_txs_header(const AnsArrays a, const TxsArrays x) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= x.V || !x.vdst[v]) return;
    const uint64_t j = x.vslot[v];
    const PbHdr h = pb_header(a.hd[j], a.txlog);
    ByteWriter bw(x.vdst[v]);
    put_header(bw, 0x0a, a.hd[j], h, a.txlog);
    bw.finish();
}

// where the TxEntry of item it lies in its variant's Tx
__device__ __forceinline__ uint8_t *txs_entry_at(const TxsArrays &x, uint64_t v, uint64_t it) {
    return x.vdst[v] + x.vhsz[v] + x.ipos[it];
}

// TxEntryToProto, and for a value the tag and length of field 5: the value
// itself, the last bytes of its entry, is the value kernel's
__global__ __launch_bounds__(256) void k_txs_entries(const AnsArrays a, const TxsArrays x) {
    const uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= x.I || x.ikind[it] == kTxsDrop) return;
    const uint64_t v = owner_of(x.item_off, x.V, it);
    if (!x.vdst[v]) return;
    const uint8_t *r = txs_record(a, x, v, it);
    const AnsEntry t = ans_entry(r);
    const bool val = x.ikind[it] == kTxsValue;
    ByteWriter bw(txs_entry_at(x, v, it));
    bw.put8(0x12);
    bw.varint((uint64_t)t.body + (val ? 1 + vlen(t.vlen) + (uint64_t)t.vlen : 0));
    put_entry_fields(bw, r, t);
    if (val) {
        bw.put8(0x2a);
        bw.varint(t.vlen);
    }
    bw.finish();
}

// value_lane (value_store.hpp) over the items, their owners the variants: a
// digest that differs leaves the entry's index in gbad of its group (the lowest
// one); a value whose Tx is written is stored to its place.
struct TxsValues {
    static constexpr bool stores = true;
    const AnsArrays &a;
    const TxsArrays &x;
    uint64_t n;
    const uint8_t *idle;
    __device__ __forceinline__ bool skip(uint64_t i) const { return x.skip[i]; }
    __device__ __forceinline__ const uint8_t *src(uint64_t i) const { return x.vsrc[i]; }
    __device__ __forceinline__ uint64_t len(uint64_t i) const { return x.vlen[i]; }
    __device__ __forceinline__ uint64_t owner(uint64_t i) const {
        return owner_of(x.item_off, x.V, i);
    }
    __device__ __forceinline__ bool place(uint64_t i, uint64_t v, uint64_t L, uint8_t *&to) const {
        if (!x.vdst[v]) return false;
        to = txs_entry_at(x, v, i) + x.isz[i] - L;
        return true;
    }
    __device__ __forceinline__ const uint8_t *record(uint64_t i, uint64_t v) const {
        return txs_record(a, x, v, i);
    }
    __device__ __forceinline__ void differs(uint64_t i, uint64_t v) const {
        atomicMin(x.gbad + x.vgroup[v], (uint32_t)(i - x.item_off[v]));
    }
};

__global__ __launch_bounds__(256) void k_txs_values(const AnsArrays a, const TxsArrays x,
                                                    const uint32_t *__restrict__ perm) {
    value_lane(TxsValues{a, x, x.I, a.txlog}, perm);
}

// the value for a variant that is not its group's primary: one wave per value
__global__ __launch_bounds__(256) void k_txs_copy(const AnsArrays a, const TxsArrays x) {
    const uint64_t it = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (it >= x.I || x.ikind[it] != kTxsValue || !x.skip[it]) return;  // wave-uniform
    const uint64_t v = owner_of(x.item_off, x.V, it);
    if (!x.vdst[v]) return;
    const uint8_t *r = txs_record(a, x, v, it);
    const uint32_t ml = rd_be16(r), kl = rd_be16(r + 2 + ml);
    const uint64_t L = be_dev(r + 4 + ml + kl, 4);
    wave_copy(txs_entry_at(x, v, it) + x.isz[it] - L, x.vsrc[it], L, lane);
}

// One wave per answer: VerifiableTx's length prefixes on lane 0, a Tx that
// several requests share copied in by the wave.  Leaves where the DualProof
// goes in dpos[p] and MH_OK in wst[p] for the answers that take one.
__global__ __launch_bounds__(64) void k_txs_assemble(const AnsArrays a, const TxsArrays x) {
    const uint64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const bool ver = x.kind[p] == MH_TXA_VERIFIABLE;
    const bool written = a.status[p] == MH_OK && a.off[p + 1] <= a.out_cap;  // wave-uniform
    if (lane == 0) {
        a.dpos[p] = 0;
        x.wst[p] = written && ver ? MH_OK : MH_ERR_MAX_WIDTH_EXCEEDED;  // (any status: skipped)
    }
    if (!written) return;
    const uint64_t v = x.rv[p], body = x.vbody[v];
    uint8_t *o = a.out + a.off[p], *txm = o;
    if (ver) {
        const uint64_t dp = a.dp_off[p + 1] - a.dp_off[p];
        txm = o + 1 + vlen(body);
        uint8_t *dpp = txm + body;
        if (lane == 0) {
            ByteWriter bw(o);
            bw.put8(0x0a);
            bw.varint(body);
            bw.finish();
            ByteWriter bd(dpp);
            bd.put8(0x12);
            bd.varint(dp);
            bd.finish();
            a.dpos[p] = (uint64_t)(dpp + 1 + vlen(dp) - a.out);
        }
    }
    if (x.vcnt[v] > 1) wave_copy(txm, x.txbuf + x.vpos[v], body, lane);
}

// status[p], first match: what was settled ahead of serializeTx; the lowest
// entry that fails (a digest ahead of the failure without a hash decides); the
// answer's end against out_cap
__global__ __launch_bounds__(256) void k_txs_status(const AnsArrays a, const TxsArrays x) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const uint64_t v = x.rv[p];
    int32_t st = a.pre[p];
    if (st == MH_OK) {
        const uint32_t ei = x.early_idx[v], gb = x.gbad[x.vgroup[v]];
        if (gb < ei) st = MH_ERR_CORRUPTED_DATA;  // immustore.go:3235
        else if (ei != kExpNone) st = x.early_st[v];
    }
    if (st == MH_OK && a.off[p + 1] > a.out_cap) st = MH_ERR_BUFFER_TOO_SMALL;
    if (st == MH_OK && x.kind[p] == MH_TXA_VERIFIABLE) st = x.wst[p];  // (the writer's: never seen)
    a.status[p] = st;
}

}  // namespace

hipError_t launch_txs_variants(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_variants", k_txs_variants, grid_for(x.V, 256), 256, a, x);
    MH_LAUNCH("txs_heads", k_txs_heads, grid_for(a.n, 256), 256, a, x);
    return hipSuccess;
}

hipError_t launch_txs_plan(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_plan", k_txs_plan, grid_for(x.I, 256), 256, a, x);
    MH_LAUNCH("txs_vsize", k_txs_vsize, grid_for(x.V, 4), 256, a, x);
    return hipSuccess;
}

hipError_t launch_txs_size(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_size", k_txs_size, grid_for(a.n, 256), 256, a, x);
    return hipSuccess;
}

hipError_t launch_txs_write(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_place", k_txs_place, grid_for(x.V, 256), 256, a, x);
    MH_LAUNCH("txs_header", k_txs_header, grid_for(x.V, 256), 256, a, x);
    MH_LAUNCH("txs_entries", k_txs_entries, grid_for(x.I, 256), 256, a, x);
    return hipSuccess;
}

hipError_t launch_txs_values(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x,
                             const uint32_t *perm) {
    MH_LAUNCH("txs_values", k_txs_values, grid_for(x.I, 256), 256, a, x, perm);
    MH_LAUNCH("txs_copy", k_txs_copy, grid_for(x.I, 4), 256, a, x);
    return hipSuccess;
}

hipError_t launch_txs_assemble(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_assemble", k_txs_assemble, (unsigned)a.n, 64, a, x);
    return hipSuccess;
}

hipError_t launch_txs_status(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x) {
    MH_LAUNCH("txs_status", k_txs_status, grid_for(a.n, 256), 256, a, x);
    return hipSuccess;
}

}  // namespace mh
