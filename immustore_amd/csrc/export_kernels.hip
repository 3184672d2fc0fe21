// export_kernels.hip -- ImmuStore.ExportTx (immustore.go:2621-2770) on CDNA4 for
// a run of txs of a resident store (capi_export.hip drives them): the read
// path has re-hashed the records (mh_txlog_validate_clog's core); here every
// value is read where it lies in its value log, checked as readValueAt does
// (:3183-3240) and laid into the blob ExportTx writes.
//
//   entries to walk, where they start, scanned   k_exp_scan<true>, one workgroup
//   decodeOffset (:1429), the value's class,
//     the entry's size in the blob               k_exp_entry, one entry per lane
//   "partially truncated" (:2703, :2726),
//     TxMetadata.Bytes(), the blob's size        k_exp_tx, one tx per wave
//   off                                          k_exp_scan<false>, one workgroup
//   header and trailer                           k_exp_head, one tx per wave
//   key, KVMetadata.Bytes(), vLen / the hVal     k_exp_ent, one entry per lane
//   SHA-256 of the value against hVal, its copy  k_exp_values<true> (arm A), or
//                                                k_exp_values<false> + k_exp_copy (arm B):
//                                                value_lane (value_store.hpp) over ExpValues
//   the statuses in ExportTx's order             k_exp_status, one tx per lane
//
// A tx record (immustore.go:1812-1924): id 8 | ts 8 | blTxID 8 | blRoot 32 |
// prevAlh 32 | version 2 | [v1: mdLen 2, md] | nentries 2 (v0) / 4 (v1) |
// entries | Alh 32; an entry: mdLen 2 | md | kLen 2 | key | vLen 4 | vOff 8 |
// hVal 32.  Only records the read path accepted are walked: it checked every
// length against the log.  What it leaves to this file is read from the
// record itself (the version, the stored metadata); of its header only the
// rebuilt Eh is taken.
//
// Cost shape: k_exp_values is the call's hashing, k_sha_varlen's loop with the
// stores added (value_lane, shared with txspec_kernels.hip's k_txs_values).
// A lane runs (vLen + 9 + 63) / 64 compressions; lanes take
// values in length-class order, so a wave runs no idle blocks.  In arm A the
// lane also stores each 64-byte block it has just turned into message words:
// one v_perm_b32 per dword puts them on the destination's dword grid (the
// source alignment went into the message words, the destination's goes into
// these), four 16-byte stores a block, a lane's stores 64 bytes apart from the
// next lane's.  Every byte of a blob is written by exactly one lane, and a
// dword only by the lane that owns all four of its bytes: the ends of every
// piece are byte stores.
#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "msg_walk.hpp"
#include "sha256_cdna.hpp"
#include "txlog_common.hpp"
#include "value_store.hpp"

namespace mh {

namespace {

__device__ __forceinline__ void xp_put(uint8_t *&o, uint64_t v, int n) {  // big-endian, n bytes
    for (int k = n - 1; k >= 0; k--) *o++ = (uint8_t)(v >> (8 * k));
}

// what the blob needs of tx t's record
struct ExpRec {
    const uint8_t *r;  // the record
    uint32_t ver, sml, ne;
    const uint8_t *md;  // the stored tx metadata (sml bytes)
};

__device__ __forceinline__ ExpRec exp_rec(const ExpArrays &a, uint64_t t) {
    ExpRec x;
    x.r = a.txlog + be_dev(a.clog + t * a.es, 8);
    x.ver = (uint32_t)be_dev(x.r + 88, 2);
    x.sml = x.ver ? (uint32_t)be_dev(x.r + 90, 2) : 0;
    x.md = x.r + 92;
    x.ne = x.ver ? (uint32_t)be_dev(x.r + 92 + x.sml, 4) : (uint32_t)be_dev(x.r + 90, 2);
    return x;
}

// len(TxHeader.Bytes()), tx.go:103-164
__device__ __forceinline__ uint32_t exp_hdr_len(uint32_t ver, uint32_t mdl) {
    return ver ? 128 + mdl : 124;
}

// the blob of tx p is written: no entry failed before any hash, and it fits
__device__ __forceinline__ bool exp_written(const ExpArrays &a, uint64_t p) {
    return a.rst[p] == MH_OK && a.early_idx[p] == kExpNone && a.off[p + 1] <= a.out_cap;
}

// where entry e of tx p starts in out
__device__ __forceinline__ uint8_t *exp_entry_at(const ExpArrays &a, uint64_t p, uint64_t e,
                                                 uint32_t ver) {
    return a.out + a.off[p] + 4 + exp_hdr_len(ver, a.mdl[p]) + a.epos[e];
}

// Exclusive offsets of n per-tx counts in one launch of one workgroup: out[0] =
// 0, out[t + 1] = the sum of the first t + 1 counts.  A thread sums its run of
// ceil(n / 1024) txs, the 1024 sums are scanned in LDS, the thread writes its
// run's offsets.  COUNTS: the counts are the entries to walk (ecnt), computed
// here with where they start; else a.size.  (One launch of a few microseconds
// where a device-wide scan of so few items is three; a run of millions of txs
// pays a longer serial pass under hashing that dwarfs it.)
template <bool COUNTS>
__global__ __launch_bounds__(1024) void k_exp_scan(const ExpArrays a) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t run = (a.n + 1023) / 1024, lo = min(t * run, a.n), hi = min(lo + run, a.n);
    uint64_t *out = COUNTS ? a.leaf_off : a.off;
    uint64_t sum = 0;
    for (uint64_t p = lo; p < hi; p++) {
        uint64_t w;
        if (COUNTS) {
            uint64_t q = 0;
            w = 0;
            if (a.rst[p] == MH_OK) {
                const ExpRec x = exp_rec(a, p);
                w = x.ne;
                q = (uint64_t)(x.r - a.txlog) + (x.ver ? 96 + x.sml : 92);
            }
            a.ecnt[p] = w;
            a.ent_start[p] = q;
        } else {
            w = a.size[p];
        }
        sum += w;
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint64_t y = (int)t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    uint64_t at = part[t] - sum;
    for (uint64_t p = lo; p < hi; p++) {
        out[p] = at;
        at += COUNTS ? a.ecnt[p] : a.size[p];
    }
    if (t == 1023) out[a.n] = part[1023];
}

// One entry: decodeOffset (immustore.go:1429-1431: Go's mask is 0xff << 55),
// then readValueAt's and multiapp.ReadAt's ways to io.EOF
__global__ __launch_bounds__(256) void k_exp_entry(const ExpArrays a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const uint8_t *r = a.txlog + a.rec_off[e];
    const uint32_t ml = rd_be16(r), kl = rd_be16(r + 2 + ml);
    const uint8_t *f = r + 4 + ml + kl;
    const uint64_t vl = be_dev(f, 4), voff = be_dev(f + 4, 8);
    const uint32_t id = (uint32_t)(voff >> 56);
    const uint64_t at = voff & ~(0xffull << 55);
    uint8_t cls = kExpAvail;
    const uint8_t *src = a.txlog;  // an empty value: nothing is read
    if (vl) {
        if (id == 0) {
            cls = kExpTrunc;  // :3186
        } else if (id > a.nvlogs) {
            cls = kExpNoVlog;
        } else {
            const ExpVlog v = a.vlogs[id - 1];
            if (at >= v.first_off && at <= v.end_off && vl <= v.end_off - at) src = v.data + (at - v.first_off);
            else cls = kExpTrunc;
        }
    }
    uint8_t cmd[MH_MAX_KV_METADATA_LEN];
    const uint32_t cml = ml ? kv_md_canon(r + 2, ml, cmd) : 0;
    a.cls[e] = cls;
    a.vsrc[e] = cls == kExpAvail ? src : nullptr;
    a.esz[e] = 2 + kl + 2 + cml + 4 + (cls == kExpAvail ? vl : 32);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, m, 64));
    return x;
}

// One tx per wave.  The lowest entry that fails without a hash: a value log the
// store does not have, or a class other than entry 0's.  The values hashed are
// the available ones ahead of it (Go reads the entries in order and stops at
// the first error).
__global__ __launch_bounds__(256) void k_exp_tx(const ExpArrays a) {
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (t >= a.n) return;  // wave-uniform
    const uint64_t e0 = a.leaf_off[t], w = a.leaf_off[t + 1] - e0;
    const uint8_t c0 = w ? a.cls[e0] : (uint8_t)kExpAvail;
    uint32_t bad = kExpNone;
    for (uint64_t i = lane; i < w && bad == kExpNone; i += 64)
        if (a.cls[e0 + i] != c0 || c0 == kExpNoVlog) bad = (uint32_t)i;
    bad = wave_min_u32(bad);
    uint64_t ebytes = 0;  // of the entries so far
    for (uint64_t i0 = 0; i0 < w; i0 += 64) {
        const uint64_t i = i0 + lane, e = e0 + i;
        unsigned long long v = 0;
        if (i < w) {
            const bool hash = a.cls[e] == kExpAvail && i < bad;
            const uint8_t *f = a.txlog + a.rec_off[e];
            const uint32_t ml = rd_be16(f), kl = rd_be16(f + 2 + ml);
            a.skip[e] = !hash;
            a.vlen[e] = hash ? be_dev(f + 4 + ml + kl, 4) : 0;
            v = a.esz[e];
        }
        const unsigned long long own = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {  // inclusive scan across the wave
            const unsigned long long y = __shfl_up(v, d, 64);
            if ((int)lane >= d) v += y;
        }
        if (i < w) a.epos[e] = ebytes + (v - own);
        ebytes += __shfl(v, 63, 64);
    }
    if (lane) return;
    uint64_t size = 0;
    uint32_t mdl = 0;
    if (a.rst[t] == MH_OK) {
        const ExpRec x = exp_rec(a, t);
        if (x.sml) mdl = tx_md_canon(x.md, x.sml, a.md + t * (uint64_t)kMdSlot);
        if (bad == kExpNone) size = 4 + exp_hdr_len(x.ver, mdl) + ebytes + 3;
    }
    a.mdl[t] = mdl;
    a.early_idx[t] = bad;
    a.early_st[t] = bad == kExpNone ? MH_OK
                    : a.cls[e0 + bad] == kExpNoVlog ? MH_ERR_ILLEGAL_STATE
                                                    : MH_ERR_CORRUPTED_DATA;
    a.vbad[t] = kExpNone;
    a.trunc[t] = c0 == kExpTrunc;
    a.size[t] = size;
}

// BE32 len(hdr) | TxHeader.Bytes() (tx.go:103-164) ... BE16 1 | byte(truncated):
// one tx per wave, a byte per lane and turn (id, PrevAlh, ts, version, then v0
// BE16 nentries, v1 BE16 mdLen | md | BE32 nentries, then the rebuilt Eh,
// BlTxID, BlRoot)
__global__ __launch_bounds__(256) void k_exp_head(const ExpArrays a) {
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (t >= a.n || !exp_written(a, t)) return;  // wave-uniform
    const ExpRec x = exp_rec(a, t);
    const uint8_t *r = x.r, *md = a.md + t * (uint64_t)kMdSlot, *eh = a.hd[t].eh;
    const uint32_t mdl = a.mdl[t], hl = exp_hdr_len(x.ver, mdl), ver = x.ver, ne = x.ne;
    const uint32_t eh_at = hl - 72;  // within hdr
    uint8_t *o = a.out + a.off[t];
    for (uint32_t i = lane; i < 4 + hl; i += 64) {
        uint32_t v;
        if (i < 4) {
            v = hl >> (8 * (3 - i));
        } else {
            uint32_t h = i - 4;
            if (h < 8) v = r[h];                               // id
            else if (h < 40) v = r[48 + h];                    // PrevAlh
            else if (h < 48) v = r[h - 32];                    // ts
            else if (h < 50) v = ver >> (8 * (49 - h));
            else if (h >= eh_at) v = h - eh_at < 32 ? eh[h - eh_at] : r[16 + (h - eh_at - 32)];  // Eh; BlTxID, BlRoot
            else if (ver == 0) v = ne >> (8 * (51 - h));
            else if (h < 52) v = mdl >> (8 * (51 - h));
            else if (h < 52 + mdl) v = md[h - 52];
            else v = ne >> (8 * (eh_at - 1 - h));
        }
        o[i] = (uint8_t)v;
    }
    if (lane < 3) a.out[a.off[t + 1] - 3 + lane] = lane == 0 ? 0 : lane == 1 ? 1 : a.trunc[t];
}

// BE16 kLen | key | BE16 mdLen | KVMetadata.Bytes() | BE32 vLen, or for a
// truncated tx BE32 32 | hVal; an available value is the value kernel's
__global__ __launch_bounds__(256) void k_exp_ent(const ExpArrays a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const uint64_t p = owner_of(a.leaf_off, a.n, e);
    if (!exp_written(a, p)) return;
    const uint8_t *r = a.txlog + a.rec_off[e];
    const uint32_t ml = rd_be16(r), kl = rd_be16(r + 2 + ml);
    const uint8_t *key = r + 4 + ml, *f = key + kl, *hv = entry_hval(r);
    uint8_t *o = exp_entry_at(a, p, e, a.ver[e]);
    xp_put(o, kl, 2);
    for (uint32_t k = 0; k < kl; k++) *o++ = key[k];
    const uint32_t cml = ml ? kv_md_canon(r + 2, ml, o + 2) : 0;
    xp_put(o, cml, 2);
    o += cml;
    if (a.cls[e] == kExpAvail) {
        xp_put(o, be_dev(f, 4), 4);
    } else {
        xp_put(o, 32, 4);
        for (int k = 0; k < 32; k++) *o++ = hv[k];
    }
}

// value_lane (value_store.hpp) over the entries, their owners the txs: a digest
// that differs leaves the entry's index in vbad of its tx (the lowest one).
// COPY: a value whose blob is written is stored to its place; else the stores
// are compiled out.
template <bool COPY>
struct ExpValues {
    static constexpr bool stores = COPY;
    const ExpArrays &a;
    uint64_t n;
    const uint8_t *idle;
    __device__ __forceinline__ bool skip(uint64_t e) const { return a.skip[e]; }
    __device__ __forceinline__ const uint8_t *src(uint64_t e) const { return a.vsrc[e]; }
    __device__ __forceinline__ uint64_t len(uint64_t e) const { return a.vlen[e]; }
    __device__ __forceinline__ uint64_t owner(uint64_t e) const {
        return owner_of(a.leaf_off, a.n, e);
    }
    __device__ __forceinline__ bool place(uint64_t e, uint64_t p, uint64_t L, uint8_t *&to) const {
        if (!(L && exp_written(a, p))) return false;
        to = exp_entry_at(a, p, e, a.ver[e]) + a.esz[e] - L;
        return true;
    }
    __device__ __forceinline__ const uint8_t *record(uint64_t e, uint64_t) const {
        return a.txlog + a.rec_off[e];
    }
    __device__ __forceinline__ void differs(uint64_t e, uint64_t p) const {
        atomicMin(a.vbad + p, (uint32_t)(e - a.leaf_off[p]));
    }
};

template <bool COPY>
__global__ __launch_bounds__(256) void k_exp_values(const ExpArrays a, const uint32_t *__restrict__ perm) {
    value_lane(ExpValues<COPY>{a, a.E, a.txlog}, perm);
}

// arm B's copy: one wave per value whose blob is written
__global__ __launch_bounds__(256) void k_exp_copy(const ExpArrays a) {
    const uint64_t e = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= a.E || a.skip[e] || !a.vlen[e]) return;  // wave-uniform
    const uint64_t p = owner_of(a.leaf_off, a.n, e);
    if (!exp_written(a, p)) return;
    const uint64_t L = a.vlen[e];
    wave_copy(exp_entry_at(a, p, e, a.ver[e]) + a.esz[e] - L, a.vsrc[e], L, lane);
}

// status[k], first match: the record verdict; the lowest entry that fails (a
// digest ahead of the early failure decides); the blob's end against out_cap
__global__ __launch_bounds__(256) void k_exp_status(const ExpArrays a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    int32_t st = a.rst[t];
    if (st == MH_OK) {
        const uint32_t ei = a.early_idx[t], vb = a.vbad[t];
        if (vb < ei) st = MH_ERR_CORRUPTED_DATA;  // immustore.go:3235
        else if (ei != kExpNone) st = a.early_st[t];
    }
    if (st == MH_OK && a.off[t + 1] > a.out_cap) st = MH_ERR_BUFFER_TOO_SMALL;
    a.status[t] = st;
    a.trunc_out[t] = st == MH_OK ? a.trunc[t] : 0;
}

}  // namespace

hipError_t launch_exp_counts(hipStream_t st, Timer *tm, const ExpArrays &a) {
    TimerScope ts(tm, "exp_counts", st);
    hipLaunchKernelGGL(k_exp_scan<true>, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_exp_entries(hipStream_t st, Timer *tm, const ExpArrays &a) {
    MH_LAUNCH("exp_entry", k_exp_entry, grid_for(a.E, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_exp_sizes(hipStream_t st, Timer *tm, const ExpArrays &a) {
    MH_LAUNCH("exp_tx", k_exp_tx, grid_for(a.n, 4), 256, a);
    TimerScope ts(tm, "exp_offsets", st);
    hipLaunchKernelGGL(k_exp_scan<false>, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_exp_frame(hipStream_t st, Timer *tm, const ExpArrays &a) {
    MH_LAUNCH("exp_head", k_exp_head, grid_for(a.n, 4), 256, a);
    MH_LAUNCH("exp_keys", k_exp_ent, grid_for(a.E, 256), 256, a);
    return hipSuccess;
}

hipError_t launch_exp_values(hipStream_t st, Timer *tm, const ExpArrays &a, const uint32_t *perm,
                             char arm) {
    if (arm == 'A') {
        MH_LAUNCH("exp_values_store", k_exp_values<true>, grid_for(a.E, 256), 256, a, perm);
    } else {
        MH_LAUNCH("exp_values_hash", k_exp_values<false>, grid_for(a.E, 256), 256, a, perm);
        MH_LAUNCH("exp_copy", k_exp_copy, grid_for(a.E, 4), 256, a);
    }
    return hipSuccess;
}

hipError_t launch_exp_status(hipStream_t st, Timer *tm, const ExpArrays &a) {
    MH_LAUNCH("exp_status", k_exp_status, grid_for(a.n, 256), 256, a);
    return hipSuccess;
}

}  // namespace mh
