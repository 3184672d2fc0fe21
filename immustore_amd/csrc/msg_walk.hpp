// msg_walk.hpp -- a lane's view of one message in memory for the ragged SHA-256
// kernels (varlen_kernels.hip, export_kernels.hip, txspec_kernels.hip): the 68-byte window of a
// block, loaded one block ahead, and the message words one v_perm_b32 per word
// makes of it (realigned and byte-swapped); the last two blocks of a message
// take the general form with the byte masks, the 0x80 pad and the bit length.
#pragma once

#include "mh_internal.hpp"
#include "sha256_cdna.hpp"

namespace mh {

// dword-aligned 16-byte load (gfx950 global loads need only dword alignment
// for multi-dword widths)
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void load_window(const uint32_t *q, uint32_t d[17]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const u32x4_a4 v = *reinterpret_cast<const u32x4_a4 *>(q + 4 * c);
        d[4 * c + 0] = v.x;
        d[4 * c + 1] = v.y;
        d[4 * c + 2] = v.z;
        d[4 * c + 3] = v.w;
    }
    d[16] = q[16];
}

// Byte mask of the first v bytes of a big-endian word (v clamped to 0..4).
__device__ __forceinline__ uint32_t hi_mask(int v) {
    return v >= 4 ? 0xffffffffu : (v <= 0 ? 0u : (0xffffffffu << (32 - 8 * v)));
}

__device__ __forceinline__ int clamp_rel(int64_t x) {
    return (int)(x < -8 ? -8 : (x > 72 ? 72 : x));
}

// Per-lane view of one message in memory for the value phase: p = first byte,
// L = length; the block builder keeps the next window prefetched.
struct MsgWalk {
    const uint32_t *q;      // dword holding p
    const uint32_t *qlast;  // dword holding the last byte
    uint32_t sel;           // v_perm selector of p's alignment
    uint64_t L;
    uint32_t d[17];         // window of the current block (loaded one block ahead)
    bool pre;               // d already holds this block's window

    __device__ __forceinline__ void init(const uint8_t *p, uint64_t len) {
        const uint32_t al = (uint32_t)((uintptr_t)p & 3);
        q = reinterpret_cast<const uint32_t *>(p - al);
        qlast = reinterpret_cast<const uint32_t *>((uintptr_t)(p + len - 1) & ~(uintptr_t)3);
        sel = 0x00010203u + al * 0x01010101u;
        L = len;
        pre = false;
    }

    // Message words of block b for the lanes with `on`.  fast (wave-uniform):
    // every active lane has >= 2 more blocks after b, so its 68-byte window
    // and the next one lie inside the message; the words are taken from d and
    // the same registers then receive the next block's window, which lands
    // under this block's compression.  Otherwise the general form (clamped
    // loads, byte masks, 0x80, bit length in the last block nb-1).
    __device__ __forceinline__ void block(uint32_t b, uint32_t nb, bool on, bool fast,
                                          uint32_t w[16]) {
        if (fast) {
            if (!pre && on) load_window(q + 16 * (uint64_t)b, d);
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = __builtin_amdgcn_perm(d[j + 1], d[j], sel);
            pre = on && b + 3 < nb;
            if (pre) load_window(q + 16 * (uint64_t)(b + 1), d);
            return;
        }
        pre = false;
        uint32_t x[17];
#pragma unroll
        for (int j = 0; j < 17; j++) x[j] = 0;
        if (on && L) {
            const uint32_t *qb = q + 16 * (uint64_t)b;
#pragma unroll
            for (int j = 0; j < 17; j++) x[j] = *(qb + j <= qlast ? qb + j : qlast);
        }
        const int r = clamp_rel((int64_t)L - 64 * (int64_t)b);  // data bytes left at block start
#pragma unroll
        for (int j = 0; j < 16; j++) {
            uint32_t y = __builtin_amdgcn_perm(x[j + 1], x[j], sel);
            const int v = r - 4 * j;  // valid bytes in this word
            y &= hi_mask(v);
            if (v >= 0 && v < 4) y |= 0x80u << (24 - 8 * v);
            w[j] = y;
        }
        if (b + 1 == nb) {
            const uint64_t bits = L * 8;
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
    }
};

}  // namespace mh
