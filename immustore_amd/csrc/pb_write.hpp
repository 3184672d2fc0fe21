// pb_write.hpp -- the byte-level pieces of the protobuf writers, shared by
// wire_kernels.hip (proofs) and answer_kernels.hip (whole answers): varint
// sizes, the TxHeader / TxMetadata encoder, the dword-staged byte stream and
// the 34-byte digest field.
#pragma once
#include "mh_internal.hpp"

namespace mh {

__device__ __forceinline__ uint32_t vlen(uint64_t v) {
    return v ? (uint32_t)((63 - __clzll(v)) / 7 + 1) : 1u;
}
// int32 field value as protobuf-go encodes it (sign-extended to 64 bits)
__device__ __forceinline__ uint64_t i32v(uint32_t x) { return (uint64_t)(int64_t)(int32_t)x; }

// ------------------------------------------------------------ TxHeader
// TxMetadata.ReadFrom (tx_metadata.go:159-195) of the stored bytes, then
// TxMetadataToProto: truncatedTxID (attribute 0, BE64) and extra (attribute
// 1, BE16 length + bytes); a later attribute of the same code replaces an
// earlier one (Go map assignment).
struct PbHdr {
    uint32_t body = 0;      // TxHeader message length
    uint32_t md_body = 0;   // TxMetadata message length
    uint64_t trunc = 0;
    uint32_t extra_off = 0, extra_len = 0;
    bool has_md = false;
    int32_t st = MH_OK;
};

__device__ inline PbHdr pb_header(const MhTxHeader &h, const uint8_t *md_blob) {
    PbHdr r;
    if (h.md_len) {  // tx.go:483-501: mdLen == 0 leaves Metadata nil
        r.has_md = true;
        if (h.md_len > MH_MAX_TX_METADATA_LEN) {
            r.st = MH_ERR_CORRUPTED_DATA;
            return r;
        }
        const uint8_t *b = md_blob + h.md_off;
        uint32_t i = 0;
        while (i < h.md_len) {
            const uint8_t code = b[i++];
            if (code == 0) {
                if (h.md_len - i < 8) { r.st = MH_ERR_CORRUPTED_DATA; return r; }
                uint64_t v = 0;
                for (int k = 0; k < 8; k++) v = v << 8 | b[i + k];
                r.trunc = v;
                i += 8;
            } else if (code == 1) {
                if (h.md_len - i < 2) { r.st = MH_ERR_CORRUPTED_DATA; return r; }
                const uint32_t L = (uint32_t)b[i] << 8 | b[i + 1];
                if (h.md_len - i - 2 < L) { r.st = MH_ERR_CORRUPTED_DATA; return r; }
                r.extra_off = h.md_off + i + 2;
                r.extra_len = L;
                i += 2 + L;
            } else {
                r.st = MH_ERR_CORRUPTED_DATA;
                return r;
            }
        }
        if (r.trunc) r.md_body += 1 + vlen(r.trunc);
        if (r.extra_len) r.md_body += 1 + vlen(r.extra_len) + r.extra_len;
    }
    uint32_t s = 0;
    if (h.id) s += 1 + vlen(h.id);
    s += 34;                                            // prevAlh
    if (h.ts) s += 1 + vlen((uint64_t)h.ts);
    if (h.nentries) s += 1 + vlen(i32v(h.nentries));
    s += 34;                                            // eH
    if (h.bl_tx_id) s += 1 + vlen(h.bl_tx_id);
    s += 34;                                            // blRoot
    if (h.version) s += 1 + vlen(i32v(h.version));
    if (r.has_md) s += 1 + vlen(r.md_body) + r.md_body;
    r.body = s;
    return r;
}

__device__ __forceinline__ uint32_t framed(uint32_t body) { return 1 + vlen(body) + body; }

// ------------------------------------------------------------ byte streams
// One lane writes one message.  Bytes collect in a 32-bit register and leave
// as dword stores; only the partial words at the two ends of a run (shared
// with the neighbouring messages / records) are written byte by byte.
// global-memory pointer types: stores through them are global_* rather than
// flat_* (a pointer rebuilt from an integer or read from LDS is generic)
typedef __attribute__((address_space(1))) uint8_t g8;
typedef __attribute__((address_space(1))) uint32_t g32;

struct ByteWriter {
    g32 *w;            // dword that receives the pending bytes
    uint32_t acc = 0;  // pending bytes, little-endian
    uint32_t fill;     // bytes already in *w's slot (pending or not ours)
    uint32_t lo;       // first byte of the current word that is ours
    __device__ explicit ByteWriter(uint8_t *p)
        : w((g32 *)((g8 *)p - ((uintptr_t)p & 3))),
          fill((uint32_t)((uintptr_t)p & 3)), lo((uint32_t)((uintptr_t)p & 3)) {}
    __device__ __forceinline__ void flush_word() {  // fill == 4
        if (lo == 0) {
            *w = acc;
        } else {
            g8 *b = (g8 *)w;
            for (uint32_t k = lo; k < 4; k++) b[k] = (uint8_t)(acc >> (8 * k));
            lo = 0;
        }
        w++;
        acc = 0;
        fill = 0;
    }
    __device__ __forceinline__ void put8(uint32_t b) {
        acc |= (b & 0xff) << (8 * fill);
        if (++fill == 4) flush_word();
    }
    // 4 bytes, little-endian in x (a word as loaded from memory)
    __device__ __forceinline__ void put32(uint32_t x) {
        if (fill == 0) {
            acc = x;
            fill = 4;
            flush_word();
        } else {
            const uint32_t sh = 8 * fill;
            acc |= x << sh;
            const uint32_t rest = x >> (32 - sh);
            fill = 4;
            flush_word();
            acc = rest;
            fill = sh / 8;
        }
    }
    __device__ __forceinline__ void varint(uint64_t v) {
        while (v >= 0x80) {
            put8((uint32_t)(v | 0x80));
            v >>= 7;
        }
        put8((uint32_t)v);
    }
    __device__ __forceinline__ void finish() {  // the trailing partial word
        g8 *b = (g8 *)w;
        for (uint32_t k = lo; k < fill; k++) b[k] = (uint8_t)(acc >> (8 * k));
    }
    __device__ __forceinline__ uint8_t *pos() const { return (uint8_t *)((g8 *)w + fill); }
};

// A 34-byte field `tag, 32, d[0..31]` (repeated-bytes term or a header
// digest) at any alignment without divergent branches: the record is built
// as 9 little-endian words, funnel-shifted to the destination alignment a,
// and stored as 7-8 dwords plus predicated byte / short stores for the
// partial words at the two ends (a = 0: -/short, 1: byte+short/short+byte,
// 2: short/-, 3: byte/byte).
template <int AS>  // address space of the destination: 0 generic, 1 global
__device__ __forceinline__ void put_rec34_as(uint8_t *pg, uint32_t tag, const uint32_t d[8]) {
    typedef __attribute__((address_space(AS))) uint8_t b8;
    typedef __attribute__((address_space(AS))) uint16_t b16;
    typedef __attribute__((address_space(AS))) uint32_t b32;
    b8 *p = (b8 *)pg;
    uint32_t r[10];
    r[0] = (tag & 0xff) | (32u << 8) | (d[0] << 16);
#pragma unroll
    for (int k = 1; k < 8; k++) r[k] = (d[k - 1] >> 16) | (d[k] << 16);
    r[8] = d[7] >> 16;
    r[9] = 0;
    const uint32_t a = (uint32_t)((uintptr_t)p & 3);
    b32 *w = (b32 *)(p - a);
    uint32_t o[10];
    o[0] = r[0] << (8 * a);
#pragma unroll
    for (int j = 1; j < 10; j++)
        o[j] = a ? __builtin_amdgcn_alignbyte(r[j], r[j - 1], 4 - a) : r[j];
    b8 *wb = (b8 *)w;
    // word 0: ours from byte a
    if (a == 0) w[0] = o[0];
    if (a & 1) wb[a] = (uint8_t)(o[0] >> (8 * a));
    if (a == 1 || a == 2) *(b16 *)(wb + 2) = (uint16_t)(o[0] >> 16);
#pragma unroll
    for (int j = 1; j < 8; j++) w[j] = o[j];
    // word 8: ours up to byte a + 34 - 32
    if (a >= 2) w[8] = o[8];
    if (a <= 1) *(b16 *)(wb + 32) = (uint16_t)o[8];
    if (a == 1) wb[34] = (uint8_t)(o[8] >> 16);
    if (a == 3) wb[36] = (uint8_t)o[9];
}

__device__ __forceinline__ void put_rec34(uint8_t *p, uint32_t tag, const uint32_t d[8]) {
    put_rec34_as<0>(p, tag, d);
}

// 32-byte digest field (tag, length 32, bytes; d 8-byte aligned): the byte
// stream is closed, the field stored by put_rec34 and the stream reopened.
__device__ __forceinline__ void put_digest(ByteWriter &bw, uint32_t tag, const uint8_t *d) {
    const uint2 *q = reinterpret_cast<const uint2 *>(d);
    uint32_t x[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint2 v = q[k];
        x[2 * k] = v.x;
        x[2 * k + 1] = v.y;
    }
    bw.finish();
    uint8_t *p = bw.pos();
    put_rec34_as<1>(p, tag, x);
    bw = ByteWriter(p + 34);
}

// TxHeader as field `tag` of the enclosing message
__device__ inline void put_header(ByteWriter &bw, uint32_t tag, const MhTxHeader &h,
                                  const PbHdr &r, const uint8_t *md_blob) {
    bw.put8(tag);
    bw.varint(r.body);
    if (h.id) { bw.put8(0x08); bw.varint(h.id); }
    put_digest(bw, 0x12, h.prev_alh);
    if (h.ts) { bw.put8(0x18); bw.varint((uint64_t)h.ts); }
    if (h.nentries) { bw.put8(0x20); bw.varint(i32v(h.nentries)); }
    put_digest(bw, 0x2a, h.eh);
    if (h.bl_tx_id) { bw.put8(0x30); bw.varint(h.bl_tx_id); }
    put_digest(bw, 0x3a, h.bl_root);
    if (h.version) { bw.put8(0x40); bw.varint(i32v(h.version)); }
    if (r.has_md) {
        bw.put8(0x4a);
        bw.varint(r.md_body);
        if (r.trunc) { bw.put8(0x08); bw.varint(r.trunc); }
        if (r.extra_len) {
            bw.put8(0x12);
            bw.varint(r.extra_len);
            for (uint32_t q = 0; q < r.extra_len; q++) bw.put8(md_blob[r.extra_off + q]);
        }
    }
}

__device__ __forceinline__ void load_node(const uint8_t *node, uint32_t x[8]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(node);  // 32-byte nodes, 16-byte aligned
    const uint4 a = q[0], b = q[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}

}  // namespace mh
