// tx_alh.hpp -- TxHeader.innerHash / Alh (embedded/store/tx.go:249-319) of one
// header per lane, shared by k_tx_alh (tx_kernels.hip) and the VerifiableGet
// verifier (ventry_kernels.hip).
#pragma once
#include "digest_io.hpp"
#include "mh_internal.hpp"

namespace mh {

__device__ __forceinline__ uint32_t ld_be32_aligned(const uint8_t *p) {
    return bswap(*reinterpret_cast<const uint32_t *>(p));
}

// SHA256(BE64 id || prev[8 words] || inner[8 words]): 72 bytes, two blocks
// (tx.go:307-319, verification.go:32-38).
__device__ __forceinline__ void alh_hash(uint64_t id, const uint32_t prev[8],
                                         const uint32_t inner[8], uint32_t out[8]) {
    uint32_t w[16];
    w[0] = (uint32_t)(id >> 32);
    w[1] = (uint32_t)id;
#pragma unroll
    for (int j = 0; j < 8; j++) w[2 + j] = prev[j];
#pragma unroll
    for (int j = 0; j < 6; j++) w[10 + j] = inner[j];
    State s;
    s.init();
    compress(s, w);
    w[0] = inner[6];
    w[1] = inner[7];
    w[2] = 0x80000000u;
#pragma unroll
    for (int j = 3; j < 15; j++) w[j] = 0;
    w[15] = 72u * 8u;
    compress(s, w);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = s.h[j];
}

__device__ __forceinline__ void put_be(uint8_t *&o, uint64_t v, int n) {
    for (int k = n - 1; k >= 0; k--) *o++ = (uint8_t)(v >> (8 * k));
}

// One header per lane: innerHash (message assembled in the lane's scratch
// slot, <= 356 bytes) then Alh.  eh_src (nullable) replaces hdrs[p].eh;
// expect (nullable) turns the Alh into a pass / MH_ERR_CORRUPTED_DATA status.
// e: the stored Alh to compare against (nullable).
__device__ __forceinline__ void tx_alh_one(uint64_t p, const MhTxHeader &h,
                                           const uint8_t *__restrict__ md_blob,
                                           const uint8_t *__restrict__ eh, uint8_t *__restrict__ msg,
                                           const uint8_t *__restrict__ e,
                                           uint8_t *__restrict__ inner_out,
                                           uint8_t *__restrict__ alh_out,
                                           int32_t *__restrict__ status) {
    uint8_t *o = msg;
    put_be(o, (uint64_t)h.ts, 8);
    put_be(o, h.version, 2);
    if (h.version == 0) {
        put_be(o, h.nentries, 2);
    } else {
        put_be(o, h.md_len, 2);
        const uint8_t *md = md_blob + h.md_off;
        for (uint32_t k = 0; k < h.md_len; k++) *o++ = md[k];
        put_be(o, h.nentries, 4);
    }
    for (int k = 0; k < 32; k++) *o++ = eh[k];
    put_be(o, h.bl_tx_id, 8);
    for (int k = 0; k < 32; k++) *o++ = h.bl_root[k];
    uint32_t inner[8], prev[8], a[8];
    sha256_bytes(msg, (uint64_t)(o - msg), -1, inner);
#pragma unroll
    for (int j = 0; j < 8; j++) prev[j] = ld_be32_aligned(h.prev_alh + 4 * j);
    alh_hash(h.id, prev, inner, a);
    if (inner_out) store_digest(inner_out + p * 32, inner);
    if (alh_out) store_digest(alh_out + p * 32, a);
    if (status) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t v = ((uint32_t)e[4 * j] << 24) | ((uint32_t)e[4 * j + 1] << 16) |
                               ((uint32_t)e[4 * j + 2] << 8) | e[4 * j + 3];
            x |= v ^ a[j];
        }
        status[p] = x ? MH_ERR_CORRUPTED_DATA : MH_OK;
    }
}

}  // namespace mh
