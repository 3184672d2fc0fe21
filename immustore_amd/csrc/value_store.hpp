// value_store.hpp -- the hashing value lane of the calls that read values where
// they lie in a value log (export_kernels.hip: the blob of ExportTx;
// txspec_kernels.hip: field 5 of a TxEntry): value_lane, THE statement of
// k_exp_values' and k_txs_values' body, and the stores it makes of the value
// it walks -- the 64-byte blocks it has just turned into message words go to an
// arbitrarily aligned destination.
#pragma once
#include "answer_common.hpp"
#include "digest_io.hpp"
#include "msg_walk.hpp"
#include "txlog_common.hpp"

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

// One value per lane, in perm order (or input order when perm is null):
// SHA-256 of item i's value against the hVal its entry record stores
// (readValueAt, immustore.go:3235), and the value stored block by block from
// the message words where the caller wants it.  The caller's side is P, a
// struct of inline functions taken by value:
//   stores                      constant; false compiles the stores out (place is not asked)
//   n, idle                     the items; any readable address (a lane without a value)
//   skip(i), src(i), len(i)     item i is not hashed; else its bytes
//   uint64_t owner(i)           whose item it is
//   bool place(i, own, L, to)   the value is written, at `to`; false: only hashed
//   record(i, own)              its entry record
//   differs(i, own)             its digest is not that record's hVal
template <class P>
__device__ __forceinline__ void value_lane(const P p, const uint32_t *perm) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = g < p.n;
    const uint64_t gc = valid ? g : p.n - 1;
    const uint64_t i = perm ? (uint64_t)perm[gc] : gc;
    const bool live = valid && !p.skip(i);
    const uint64_t L = live ? p.len(i) : 0;
    const uint8_t *src = live ? p.src(i) : p.idle;
    const uint32_t nb = live ? (uint32_t)((L + 72) >> 6) : 0u;
    const uint32_t nbmax = wave_max_u32(nb);
    uint64_t own = 0;
    ExpDst d{};
    uint32_t *al = nullptr, sel = 0, carry = 0;
    bool copy = false;
    if (live) {
        own = p.owner(i);
        uint8_t *to = nullptr;
        if (P::stores && p.place(i, own, L, to)) {
            copy = true;
            d = exp_dst(to, L);
            al = reinterpret_cast<uint32_t *>(d.dst - d.g);
            sel = be_sel(d.g);
            for (uint64_t m = 0; m < d.head; m++) d.dst[m] = src[m];
            for (uint64_t m = d.tail; m < L; m++) d.dst[m] = src[m];
        }
    }
    MsgWalk mw;
    mw.init(src, L);
    State s;
    s.init();
#pragma unroll 1
    for (uint32_t b = 0; b < nbmax; b++) {
        const bool on = b < nb;
        uint32_t w[16];
        mw.block(b, nb, on, __ballot(on && b + 2 >= nb) == 0, w);
        if (P::stores && copy && on) {
            store_block(al, b, w, carry, sel, d.q0, d.q1);
            carry = w[15];
        }
        if (on) compress(s, w);
    }
    if (!live) return;
    const uint8_t *hv = entry_hval(p.record(i, own));
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) diff |= bswap(rd_le32(hv + 4 * j)) ^ s.h[j];
    if (diff) p.differs(i, own);
}

}  // namespace mh
