// answer_common.hpp -- what the answer writers share (answer_kernels.hip: whole
// VerifiableTx / VerifiableEntry answers; txspec_kernels.hip: the answers of
// TxByID / TxScan / VerifiableTxByID under an EntriesSpec): the slot of a tx in
// the call's read set, what TxEntryToProto makes of an entry record, and the
// entry's fields 1 to 4 as protobuf-go lays them down.  With export_kernels.hip
// they also share the launchers' grid and launch, the owner of an item and
// where an entry record keeps its hVal.
#pragma once
#include "mh_internal.hpp"
#include "pb_write.hpp"

namespace mh {

inline unsigned grid_for(uint64_t threads, unsigned block) {
    return (unsigned)((threads + block - 1) / block);
}

// One timed launch inside a launcher (st, tm in scope); an empty grid launches nothing
#define MH_LAUNCH(name, kernel, grid, block, ...)                                 \
    do {                                                                          \
        if (!(grid)) break;                                                       \
        TimerScope ts(tm, name, st);                                              \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);  \
        if (hipError_t e = hipGetLastError()) return e;                           \
    } while (0)

__device__ __forceinline__ uint64_t be_dev(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int k = 0; k < n; k++) v = v << 8 | p[k];
    return v;
}

// the owner of item i among n: off[p] <= i < off[p + 1]
__device__ __forceinline__ uint64_t owner_of(const uint64_t *off, uint64_t n, uint64_t i) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the hVal of the entry record r: mdLen 2 | md | kLen 2 | key | vLen 4 | vOff 8 | hVal 32
__device__ __forceinline__ const uint8_t *entry_hval(const uint8_t *r) {
    const uint32_t ml = ((uint32_t)r[0] << 8) | r[1];
    const uint8_t *k = r + 2 + ml;
    const uint32_t kl = ((uint32_t)k[0] << 8) | k[1];
    return r + 4 + ml + kl + 12;
}

__device__ __forceinline__ uint64_t ans_slot(const AnsArrays &a, uint64_t x) {
    const uint64_t b = x - 1, w = a.bits[b >> 6];
    return a.rank[b >> 6] + (uint64_t)__popcll(w & ((1ull << (b & 63)) - 1));
}

// what TxEntryToProto makes of an entry record
struct AnsEntry {
    uint32_t ml, kl, vlen;
    bool deleted = false, nonidx = false, has_exp = false;
    uint64_t exp = 0;
    uint32_t exp_body = 0, md_body = 0, body = 0;
};

__device__ inline AnsEntry ans_entry(const uint8_t *r) {
    AnsEntry e;
    e.ml = ((uint32_t)r[0] << 8) | r[1];
    e.kl = ((uint32_t)r[2 + e.ml] << 8) | r[3 + e.ml];
    e.vlen = (uint32_t)be_dev(r + 4 + e.ml + e.kl, 4);
    // KVMetadata.unsafeReadFrom (kv_metadata.go:221-256); the read path took the record
    for (uint32_t i = 0; i < e.ml;) {
        const uint8_t code = r[2 + i++];
        if (code == 0) {
            e.deleted = true;
        } else if (code == 1 && e.ml - i >= 8) {
            e.has_exp = true;
            e.exp = be_dev(r + 2 + i, 8);
            i += 8;
        } else if (code == 2) {
            e.nonidx = true;
        } else {
            break;
        }
    }
    if (e.ml) {
        if (e.deleted) e.md_body += 2;
        if (e.has_exp) {
            e.exp_body = e.exp ? 1 + vlen(e.exp) : 0;
            e.md_body += 2 + e.exp_body;
        }
        if (e.nonidx) e.md_body += 2;
    }
    e.body = (e.kl ? 1 + vlen(e.kl) + e.kl : 0) + 34 + (e.vlen ? 1 + vlen(i32v(e.vlen)) : 0) +
             (e.ml ? 1 + vlen(e.md_body) + e.md_body : 0);
    return e;
}

__device__ __forceinline__ uint64_t framed_u64(uint64_t body) { return 1 + vlen(body) + body; }

// key, hValue, vLen, metadata (TxEntryToProto, database_protoconv.go:27-49) of
// the entry record r; the tag and length of the entry are the caller's
__device__ inline void put_entry_fields(ByteWriter &bw, const uint8_t *r, const AnsEntry &t) {
    const uint8_t *key = r + 4 + t.ml, *hv = entry_hval(r);
    if (t.kl) {
        bw.put8(0x0a);
        bw.varint(t.kl);
        for (uint32_t k = 0; k < t.kl; k++) bw.put8(key[k]);
    }
    {  // hValue: always 32 bytes
        uint32_t x[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            x[k] = hv[4 * k] | (uint32_t)hv[4 * k + 1] << 8 | (uint32_t)hv[4 * k + 2] << 16 |
                   (uint32_t)hv[4 * k + 3] << 24;
        bw.finish();
        uint8_t *q = bw.pos();
        put_rec34_as<1>(q, 0x12, x);
        bw = ByteWriter(q + 34);
    }
    if (t.vlen) {
        bw.put8(0x18);
        bw.varint(i32v(t.vlen));
    }
    if (t.ml) {
        bw.put8(0x22);
        bw.varint(t.md_body);
        if (t.deleted) { bw.put8(0x08); bw.put8(1); }
        if (t.has_exp) {
            bw.put8(0x12);
            bw.put8(t.exp_body);
            if (t.exp) { bw.put8(0x08); bw.varint(t.exp); }
        }
        if (t.nonidx) { bw.put8(0x18); bw.put8(1); }
    }
}

}  // namespace mh
