// value_store.hpp -- a hashing lane's stores of the value it walks: the 64-byte
// blocks it has just turned into message words go to an arbitrarily aligned
// destination (export_kernels.hip: the blob of ExportTx; txspec_kernels.hip:
// field 5 of a TxEntry).
#pragma once
#include "digest_io.hpp"
#include "msg_walk.hpp"

namespace mh {

// Block b of a value (message words w, the last word of the block before in
// carry) onto the destination: the value's byte m goes to al + m, al the
// aligned address g = 0..3 bytes below its first byte, so dword q of that grid
// holds the value's bytes [4q - g, 4q - g + 4): the last g bytes of message
// word q - 1 and the first 4 - g of word q, in memory order -- one v_perm_b32.
// Only the dwords q0 <= q < q1 that lie wholly inside the value are stored.
__device__ __forceinline__ void store_block(uint32_t *al, uint32_t b, const uint32_t w[16], uint32_t carry,
                                            uint32_t sel, uint64_t q0, uint64_t q1) {
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = __builtin_amdgcn_perm(k ? w[k - 1] : carry, w[k], sel);
    const uint64_t qb = 16 * (uint64_t)b;
    uint32_t *d = al + qb;
    if (qb >= q0 && qb + 16 <= q1) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            u32x4_a4 x;
            x.x = v[4 * c + 0];
            x.y = v[4 * c + 1];
            x.z = v[4 * c + 2];
            x.w = v[4 * c + 3];
            *reinterpret_cast<u32x4_a4 *>(d + 4 * c) = x;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (qb + k >= q0 && qb + k < q1) d[k] = v[k];
    }
}

// where an available value goes, and the dwords of it that are whole
struct ExpDst {
    uint8_t *dst;
    uint64_t q0, q1, head, tail;  // bytes [0, head) and [tail, L) are byte stores
    uint32_t g;
};

__device__ __forceinline__ ExpDst exp_dst(uint8_t *dst, uint64_t L) {
    ExpDst d;
    d.dst = dst;
    d.g = (uint32_t)((uintptr_t)dst & 3);
    d.q0 = d.g ? 1 : 0;
    d.q1 = (L + d.g) >> 2;
    if (d.q1 <= d.q0) {
        d.q1 = d.q0 = 0;
        d.head = d.tail = L;  // a few bytes: no whole dword
    } else {
        d.head = (4 - d.g) & 3;
        d.tail = 4 * d.q1 - d.g;
    }
    return d;
}

}  // namespace mh
