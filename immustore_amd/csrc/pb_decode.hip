// pb_decode.hip -- DualProofV2 protobuf messages decoded on the device
// (the FromProto side of database_protoconv.go): what a
// client / auditor does with every VerifiableTxV2 answer before
// VerifyDualProofV2, for a batch of messages at once.
//
//   DualProofV2FromProto  database_protoconv.go:226-233   schema.proto:437-445
//   TxHeaderFromProto     :235-247                        schema.proto:349-378
//   TxMetadataFromProto   :249-262 (-> TxMetadata.Bytes(), tx_metadata.go:145-157)
//   DigestFromProto / DigestsFromProto  :293-305 (copy of up to 32 bytes)
//   InclusionProofFromProto  :123-129                    schema.proto:534-545
//   DualProofFromProto (v1)  :213-224, LinearProofFromProto :264-270,
//   LinearAdvanceProofFromProto :272-287                 schema.proto:388-434
//   proto.Unmarshal into schema.VerifiableEntry (a VerifiableGet answer, as
//   pkg/client/client.go:1140-1175 reads it)  schema.proto:208-246, 451-508
//
// proto3 wire format as protobuf-go's Unmarshal reads it: fields in any
// order; a scalar or bytes field seen twice keeps the last value; an embedded
// message seen twice is merged (its fields read in turn into the same value);
// a known field with an unexpected wire type, and unknown fields (groups
// included), are skipped; int32 values are the low 32 bits of the varint.
// Malformed bytes (truncation, an over-long varint, wire type 6 / 7, field
// number 0, an unmatched end group) -> MH_ERR_CORRUPTED_DATA.  A message
// without a source or target header -> MH_ERR_ILLEGAL_ARGUMENTS (Go's
// TxHeaderFromProto dereferences the nil header).
//
// One lane per message, two passes: the first validates and counts the
// inclusion / consistency terms and the canonical metadata bytes, the offsets
// are scanned (scan_offsets_u64), the second writes the headers, the terms and
// the metadata (packed: only the bytes that exist travel back to the host).
#include "capi_internal.hpp"

namespace {

constexpr uint32_t kMaxExtra = 256;                   // maxExtraLen, tx_metadata.go

struct PbIn {
    const uint8_t *p, *end;
    __device__ __forceinline__ bool varint(uint64_t &v) {
        v = 0;
        for (int i = 0; i < 10; i++) {
            if (p >= end) return false;
            const uint8_t b = *p++;
            if (i == 9 && b > 1) return false;  // beyond 64 bits (protowire)
            v |= (uint64_t)(b & 0x7f) << (7 * i);
            if (!(b & 0x80)) return true;
        }
        return false;
    }
    __device__ __forceinline__ bool bytes(const uint8_t *&q, uint64_t &len) {
        if (!varint(len) || len > (uint64_t)(end - p)) return false;
        q = p;
        p += len;
        return true;
    }
    __device__ __forceinline__ bool skip(uint64_t n) {
        if (n > (uint64_t)(end - p)) return false;
        p += n;
        return true;
    }
    __device__ __forceinline__ bool key(uint32_t &field, uint32_t &wt) {
        uint64_t k;
        if (!varint(k)) return false;
        field = (uint32_t)(k >> 3);
        wt = (uint32_t)(k & 7);
        return (k >> 3) != 0 && (k >> 3) < (1ull << 29);
    }
    // the value of an unknown (or mistyped) field; a group to its end
    __device__ __forceinline__ bool skip_value(uint32_t field, uint32_t wt) {
        uint64_t v;
        const uint8_t *q;
        switch (wt) {
        case 0: return varint(v);
        case 1: return skip(8);
        case 2: return bytes(q, v);
        case 5: return skip(4);
        case 3: return (p = skip_group(p, end, field)) != nullptr;
        default: return false;  // 4: an end group with no start; 6, 7
        }
    }
    // groups (deprecated, seen only as unknown fields) out of line, the reader
    // passed by value (a reference would pin the caller's reader to scratch):
    // -> the position after the group, nullptr if malformed
    static __device__ __noinline__ const uint8_t *skip_group(const uint8_t *p, const uint8_t *end,
                                                             uint32_t field) {
        PbIn in{p, end};
        return in.group_end(field) ? in.p : nullptr;
    }
    __device__ bool group_end(uint32_t field) {
        uint32_t stack[32];
        int depth = 0;
        uint32_t wt = 3;
        for (;;) {
            uint64_t v;
            const uint8_t *q;
            switch (wt) {
            case 0: if (!varint(v)) return false; break;
            case 1: if (!skip(8)) return false; break;
            case 2: if (!bytes(q, v)) return false; break;
            case 5: if (!skip(4)) return false; break;
            case 3:
                if (depth == 32) return false;
                stack[depth++] = field;
                break;
            case 4:
                if (depth == 0 || stack[depth - 1] != field) return false;
                depth--;
                break;
            default: return false;
            }
            if (depth == 0) return true;
            if (!key(field, wt)) return false;
        }
    }
};

// DigestFromProto: the first min(len, 32) bytes, zero padded, into an 8-byte
// aligned destination.  The usual 32-byte case reads nine aligned dwords and
// funnel-shifts them (v_alignbyte) instead of 32 byte loads; the read may run
// up to 3 bytes past the term, inside the padded message area.
__device__ __forceinline__ void digest_from(const uint8_t *q, uint64_t len, uint8_t *d) {
    uint32_t o[8];
    if (len >= 32) {
        const uint32_t *a = (const uint32_t *)((uintptr_t)q & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)((uintptr_t)q & 3);
        uint32_t w[9];
#pragma unroll
        for (int i = 0; i < 9; i++) w[i] = a[i];
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t v = 0;
            for (int j = 0; j < 4; j++)
                if ((uint64_t)(4 * i + j) < len) v |= (uint32_t)q[4 * i + j] << (8 * j);
            o[i] = v;
        }
    }
    uint2 *dd = (uint2 *)d;
#pragma unroll
    for (int i = 0; i < 4; i++) dd[i] = make_uint2(o[2 * i], o[2 * i + 1]);
}

struct MdState {
    bool present = false;
    uint64_t trunc = 0;
    const uint8_t *extra = nullptr;
    uint64_t extra_len = 0;
};

// TxMetadata fields into md (merged)
__device__ __forceinline__ bool parse_md(const uint8_t *q, uint64_t len, MdState &md) {
    PbIn in{q, q + len};
    md.present = true;
    while (in.p < in.end) {
        uint32_t f, wt;
        if (!in.key(f, wt)) return false;
        if (f == 1 && wt == 0) {
            if (!in.varint(md.trunc)) return false;
        } else if (f == 2 && wt == 2) {
            if (!in.bytes(md.extra, md.extra_len)) return false;
        } else if (!in.skip_value(f, wt)) {
            return false;
        }
    }
    return true;
}

// TxHeader fields (merged); WRITE: stored straight into the output header h
// (zeroed by the caller), else only validated.  md receives the metadata.
template <bool WRITE>
__device__ __forceinline__ bool parse_header(const uint8_t *q, uint64_t len, mh_tx_header *h,
                                             MdState &md) {
    PbIn in{q, q + len};
    while (in.p < in.end) {
        uint32_t f, wt;
        if (!in.key(f, wt)) return false;
        uint64_t v;
        const uint8_t *b;
        uint64_t bl;
        if (wt == 0 && (f == 1 || f == 3 || f == 4 || f == 6 || f == 8)) {
            if (!in.varint(v)) return false;
            if (WRITE) {
                if (f == 1) h->id = v;
                else if (f == 3) h->ts = (int64_t)v;
                else if (f == 4) h->nentries = (uint32_t)v;  // int32: the low 32 bits
                else if (f == 6) h->bl_tx_id = v;
                else h->version = (uint32_t)v;
            }
        } else if (wt == 2 && (f == 2 || f == 5 || f == 7)) {
            if (!in.bytes(b, bl)) return false;
            if (WRITE) digest_from(b, bl, f == 2 ? h->prev_alh : (f == 5 ? h->eh : h->bl_root));
        } else if (wt == 2 && f == 9) {
            if (!in.bytes(b, bl) || !parse_md(b, bl, md)) return false;
        } else if (!in.skip_value(f, wt)) {
            return false;
        }
    }
    return true;
}

// TxMetadataFromProto + Bytes(): truncatedUptoTx (code 0, BE64) when > 0,
// then extra (code 1, BE16 length) when 1..256 bytes (WithExtra rejects
// longer data, and the call's error is ignored)
__device__ __forceinline__ uint32_t md_len(const MdState &md) {
    if (!md.present) return 0;
    return (md.trunc > 0 ? 9u : 0u) +
           (md.extra_len > 0 && md.extra_len <= kMaxExtra ? 3u + (uint32_t)md.extra_len : 0u);
}

__device__ void md_write(const MdState md, uint8_t *out) {  // by value: keeps the caller's state out of scratch
    uint32_t k = 0;
    if (!md.present) return;
    if (md.trunc > 0) {
        out[k++] = 0;
        for (int j = 7; j >= 0; j--) out[k++] = (uint8_t)(md.trunc >> (8 * j));
    }
    if (md.extra_len > 0 && md.extra_len <= kMaxExtra) {
        out[k++] = 1;
        out[k++] = (uint8_t)(md.extra_len >> 8);
        out[k++] = (uint8_t)md.extra_len;
        for (uint64_t j = 0; j < md.extra_len; j++) out[k++] = md.extra[j];
    }
}

// One DualProofV2 message per lane.  WRITE = false: validate, count the
// inclusion / consistency terms and the canonical metadata bytes of the two
// headers; WRITE = true: headers, terms and metadata at the scanned offsets.
// The two headers live in separate variables (no dynamically indexed local
// arrays: those would go to scratch).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pbd_dual(uint64_t n, const uint8_t *__restrict__ msgs,
                                                  const uint64_t *__restrict__ msg_off,
                                                  uint64_t *__restrict__ cnt_i, uint64_t *__restrict__ cnt_c,
                                                  uint64_t *__restrict__ cnt_m,
                                                  const uint64_t *__restrict__ incl_off,
                                                  const uint64_t *__restrict__ cons_off,
                                                  const uint64_t *__restrict__ md_off,
                                                  uint8_t *__restrict__ incl_terms,
                                                  uint8_t *__restrict__ cons_terms,
                                                  mh_tx_header *__restrict__ src_hdr,
                                                  mh_tx_header *__restrict__ tgt_hdr,
                                                  uint8_t *__restrict__ md_blob,
                                                  int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t o0 = msg_off[p], o1 = msg_off[p + 1] >= o0 ? msg_off[p + 1] : o0;
    mh_tx_header *hs = WRITE ? src_hdr + p : nullptr, *ht = WRITE ? tgt_hdr + p : nullptr;
    // the write pass re-reads only what the first pass accepted: a malformed
    // message was given no term or metadata slots and decodes to zero headers
    const bool corrupt = WRITE && status[p] == MH_ERR_CORRUPTED_DATA;
    if (WRITE) {
        *hs = mh_tx_header{};
        *ht = mh_tx_header{};
    }
    PbIn in{msgs + o0, corrupt ? msgs + o0 : msgs + o1};
    MdState ms, mt;
    bool have_s = false, have_t = false;
    uint64_t ki = 0, kc = 0;
    uint8_t *ti = WRITE ? incl_terms + 32 * incl_off[p] : nullptr;
    uint8_t *tc = WRITE ? cons_terms + 32 * cons_off[p] : nullptr;
    bool ok = true;
    while (ok && in.p < in.end) {
        uint32_t f, wt;
        if (!in.key(f, wt)) {
            ok = false;
            break;
        }
        const uint8_t *b;
        uint64_t bl;
        if (wt == 2 && f == 1) {
            ok = in.bytes(b, bl) && parse_header<WRITE>(b, bl, hs, ms);
            have_s = true;
        } else if (wt == 2 && f == 2) {
            ok = in.bytes(b, bl) && parse_header<WRITE>(b, bl, ht, mt);
            have_t = true;
        } else if (wt == 2 && f == 3) {
            ok = in.bytes(b, bl);
            if (WRITE) digest_from(b, bl, ti + 32 * ki);
            ki++;
        } else if (wt == 2 && f == 4) {
            ok = in.bytes(b, bl);
            if (WRITE) digest_from(b, bl, tc + 32 * kc);
            kc++;
        } else {
            ok = in.skip_value(f, wt);
        }
    }
    if (!WRITE) {
        const int32_t st = !ok ? MH_ERR_CORRUPTED_DATA
                               : (!have_s || !have_t) ? MH_ERR_ILLEGAL_ARGUMENTS : MH_OK;
        status[p] = st;
        // a malformed message contributes no terms and no metadata
        cnt_i[p] = ok ? ki : 0;
        cnt_c[p] = ok ? kc : 0;
        cnt_m[p] = ok ? md_len(ms) + md_len(mt) : 0;
        return;
    }
    const uint64_t m0 = md_off[p];
    const uint32_t ls = corrupt ? 0u : md_len(ms), lt = corrupt ? 0u : md_len(mt);
    hs->md_off = (uint32_t)m0;
    hs->md_len = ls;
    ht->md_off = (uint32_t)(m0 + ls);
    ht->md_len = lt;
    if (ls) md_write(ms, md_blob + m0);
    if (lt) md_write(mt, md_blob + m0 + ls);
}

// One InclusionProof message per lane (InclusionProofFromProto,
// database_protoconv.go:123-129): Leaf / Width are int32 on the wire and Go
// ints after the conversion (sign-extended; stored as their 64-bit pattern).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pbd_incl(uint64_t n, const uint8_t *__restrict__ msgs,
                                                  const uint64_t *__restrict__ msg_off,
                                                  uint64_t *__restrict__ cnt,
                                                  const uint64_t *__restrict__ term_off,
                                                  uint8_t *__restrict__ terms,
                                                  uint64_t *__restrict__ leaf,
                                                  uint64_t *__restrict__ width,
                                                  int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t o0 = msg_off[p], o1 = msg_off[p + 1] >= o0 ? msg_off[p + 1] : o0;
    const bool corrupt = WRITE && status[p] == MH_ERR_CORRUPTED_DATA;
    PbIn in{msgs + o0, corrupt ? msgs + o0 : msgs + o1};
    uint64_t lf = 0, wd = 0, k = 0;
    uint8_t *t = WRITE ? terms + 32 * term_off[p] : nullptr;
    bool ok = true;
    while (ok && in.p < in.end) {
        uint32_t f, wt;
        if (!in.key(f, wt)) {
            ok = false;
            break;
        }
        uint64_t v;
        const uint8_t *b;
        if (wt == 0 && (f == 1 || f == 2)) {
            ok = in.varint(v);
            const uint64_t x = (uint64_t)(int64_t)(int32_t)(uint32_t)v;  // int(int32)
            if (f == 1) lf = x;
            else wd = x;
        } else if (wt == 2 && f == 3) {
            ok = in.bytes(b, v);
            if (WRITE) digest_from(b, v, t + 32 * k);
            k++;
        } else {
            ok = in.skip_value(f, wt);
        }
    }
    if (!WRITE) {
        status[p] = ok ? MH_OK : MH_ERR_CORRUPTED_DATA;
        cnt[p] = ok ? k : 0;
        return;
    }
    leaf[p] = corrupt ? 0 : lf;
    width[p] = corrupt ? 0 : wd;
}

// ---------------------------------------------------------------- DualProof (v1)
// DualProofFromProto (database_protoconv.go:213-224) with LinearProofFromProto
// (:264-270; not nil-checked: a message without linearProof panics in Go ->
// MH_ERR_ILLEGAL_ARGUMENTS) and LinearAdvanceProofFromProto (:272-287; nil ->
// has_advance 0; only the nested InclusionProofs' terms are kept).  The
// per-message counts (kI .. kMd) and the arrays the write pass fills
// (Dual1Arrays, offsets from 0) are declared in mh_internal.hpp.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pbd_dual1(uint64_t n, const uint8_t *__restrict__ msgs,
                                                   const uint64_t *__restrict__ msg_off,
                                                   const uint64_t *__restrict__ msg_end,
                                                   uint64_t *__restrict__ cnt,  // kCounts x n
                                                   Dual1Arrays o, int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (WRITE && p == 0) o.qoff[o.off[kQ][n]] = o.off[kQT][n];  // the nested proofs' closing offset
    // message p is [msg_off[p], msg_off[p + 1]), or, begin-and-end form (the
    // DualProof ranges k_pbd_ventry located), [msg_off[p], msg_end[p])
    const uint64_t o0 = msg_off[p], oe = msg_end ? msg_end[p] : msg_off[p + 1];
    const uint64_t o1 = oe >= o0 ? oe : o0;
    const bool corrupt = WRITE && status[p] == MH_ERR_CORRUPTED_DATA;
    mh_tx_header *hs = WRITE ? o.src_hdr + p : nullptr, *ht = WRITE ? o.tgt_hdr + p : nullptr;
    if (WRITE) {
        *hs = mh_tx_header{};
        *ht = mh_tx_header{};
        uint2 *z = (uint2 *)(o.tbl_alh + 32 * p);
        for (int i = 0; i < 4; i++) z[i] = make_uint2(0, 0);
    }
    PbIn in{msgs + o0, corrupt ? msgs + o0 : msgs + o1};
    MdState ms, mt;
    bool have_s = false, have_t = false, have_lin = false, have_adv = false;
    // running counts (plain scalars: an array or a capturing lambda here sends
    // the readers to scratch)
    uint64_t ki = 0, kc = 0, kl = 0, kln = 0, ka = 0, kq = 0, kqt = 0;
    uint64_t lsrc = 0, ltgt = 0;
    bool ok = true;
#define PBD_TERM(J, CNT, B, BL)                                                          \
    do {                                                                                 \
        if (WRITE) digest_from(B, BL, o.terms[J] + 32 * (o.off[J][p] + CNT));            \
        CNT++;                                                                           \
    } while (0)
    while (ok && in.p < in.end) {
        uint32_t f, wt;
        if (!in.key(f, wt)) {
            ok = false;
            break;
        }
        const uint8_t *b;
        uint64_t bl;
        if (wt == 2 && f == 1) {
            ok = in.bytes(b, bl) && parse_header<WRITE>(b, bl, hs, ms);
            have_s = true;
        } else if (wt == 2 && f == 2) {
            ok = in.bytes(b, bl) && parse_header<WRITE>(b, bl, ht, mt);
            have_t = true;
        } else if (wt == 2 && f == 3) {
            if ((ok = in.bytes(b, bl))) PBD_TERM(kI, ki, b, bl);
        } else if (wt == 2 && f == 4) {
            if ((ok = in.bytes(b, bl))) PBD_TERM(kC, kc, b, bl);
        } else if (wt == 2 && f == 5) {
            if ((ok = in.bytes(b, bl)) && WRITE) digest_from(b, bl, o.tbl_alh + 32 * p);
        } else if (wt == 2 && f == 6) {
            if ((ok = in.bytes(b, bl))) PBD_TERM(kL, kl, b, bl);
        } else if (wt == 2 && f == 7) {  // LinearProof (merged)
            have_lin = true;
            if (!(ok = in.bytes(b, bl))) break;
            PbIn li{b, b + bl};
            while (ok && li.p < li.end) {
                uint32_t g, gt;
                if (!li.key(g, gt)) {
                    ok = false;
                    break;
                }
                const uint8_t *c;
                uint64_t cl;
                if (gt == 0 && g == 1) ok = li.varint(lsrc);
                else if (gt == 0 && g == 2) ok = li.varint(ltgt);
                else if (gt == 2 && g == 3) {
                    if ((ok = li.bytes(c, cl))) PBD_TERM(kLin, kln, c, cl);
                } else ok = li.skip_value(g, gt);
            }
        } else if (wt == 2 && f == 8) {  // LinearAdvanceProof (merged)
            have_adv = true;
            if (!(ok = in.bytes(b, bl))) break;
            PbIn ai{b, b + bl};
            while (ok && ai.p < ai.end) {
                uint32_t g, gt;
                if (!ai.key(g, gt)) {
                    ok = false;
                    break;
                }
                const uint8_t *c;
                uint64_t cl;
                if (gt == 2 && g == 1) {
                    if ((ok = ai.bytes(c, cl))) PBD_TERM(kAdv, ka, c, cl);
                } else if (gt == 2 && g == 2) {  // one more InclusionProof: its terms
                    if (!(ok = ai.bytes(c, cl))) break;
                    if (WRITE) o.qoff[o.off[kQ][p] + kq] = o.off[kQT][p] + kqt;
                    kq++;
                    PbIn qi{c, c + cl};
                    while (ok && qi.p < qi.end) {
                        uint32_t h, htp;
                        if (!qi.key(h, htp)) {
                            ok = false;
                            break;
                        }
                        const uint8_t *d;
                        uint64_t dl;
                        if (htp == 2 && h == 3) {
                            if ((ok = qi.bytes(d, dl))) {
                                if (WRITE) digest_from(d, dl, o.qterms + 32 * (o.off[kQT][p] + kqt));
                                kqt++;
                            }
                        } else ok = qi.skip_value(h, htp);  // leaf / width: not kept
                    }
                } else ok = ai.skip_value(g, gt);
            }
        } else {
            ok = in.skip_value(f, wt);
        }
    }
#undef PBD_TERM
    if (!WRITE) {
        status[p] = !ok ? MH_ERR_CORRUPTED_DATA
                        : (!have_s || !have_t || !have_lin) ? MH_ERR_ILLEGAL_ARGUMENTS : MH_OK;
        const uint64_t v[kCounts] = {ki, kc, kl, kln, ka, kq, kqt, md_len(ms) + md_len(mt)};
#pragma unroll
        for (int j = 0; j < kCounts; j++) cnt[(uint64_t)j * n + p] = ok ? v[j] : 0;
        return;
    }
    o.has_lin[p] = !corrupt && have_lin;
    o.has_adv[p] = !corrupt && have_adv;
    o.lin_src[p] = corrupt ? 0 : lsrc;
    o.lin_tgt[p] = corrupt ? 0 : ltgt;
    const uint64_t m0 = o.off[kMd][p];
    const uint32_t ls = corrupt ? 0u : md_len(ms), lt = corrupt ? 0u : md_len(mt);
    hs->md_off = (uint32_t)m0;
    hs->md_len = ls;
    ht->md_off = (uint32_t)(m0 + ls);
    ht->md_len = lt;
    if (ls) md_write(ms, o.md_blob + m0);
    if (lt) md_write(mt, o.md_blob + m0 + ls);
}

// ---------------------------------------------------------------- VerifiableEntry
// proto.Unmarshal into schema.VerifiableEntry (schema.proto:208-246, 277-293,
// 344-434, 451-508, 534-545) as pkg/client reads a VerifiableGet answer
// (client.go:1140-1175): the whole closure of the message is validated --
// Go unmarshals Tx.entries / kvEntries / zEntries and the signature too, and a
// malformed field there fails the answer -- and the fields verifiedGet reads
// are located.  A schema table (message -> field -> kind, child message) and
// an explicit stack of enclosing messages replace one hand-written loop per
// message type; the stack lives in LDS (8 levels x 256 lanes: a dynamically
// indexed local array would go to scratch).
enum : uint32_t {
    vVE = 0, vEntry, vRef, vKvmd, vExp, vVtx, vTx, vHdr, vTxmd, vTxEntry, vZEntry, vSig, vDual,
    vLin, vAdv, vIncl, vMsgs
};
// field kinds: 0 unknown, fV varint, fB bytes, f8 fixed64, fM + child message
enum : uint8_t { fV = 1, fB = 2, f8 = 3, fM = 16 };
constexpr uint32_t kVeFields = 10;  // field numbers 1..9
__device__ __constant__ static const uint8_t kVeSchema[vMsgs][kVeFields] = {
    /* VerifiableEntry    */ {0, fM + vEntry, fM + vVtx, fM + vIncl, 0, 0, 0, 0, 0, 0},
    /* Entry              */ {0, fV, fB, fB, fM + vRef, fM + vKvmd, fV, fV, 0, 0},
    /* Reference          */ {0, fV, fB, fV, fM + vKvmd, fV, 0, 0, 0, 0},
    /* KVMetadata         */ {0, fV, fM + vExp, fV, 0, 0, 0, 0, 0, 0},
    /* Expiration         */ {0, fV, 0, 0, 0, 0, 0, 0, 0, 0},
    /* VerifiableTx       */ {0, fM + vTx, fM + vDual, fM + vSig, 0, 0, 0, 0, 0, 0},
    /* Tx                 */ {0, fM + vHdr, fM + vTxEntry, fM + vEntry, fM + vZEntry, 0, 0, 0, 0, 0},
    /* TxHeader           */ {0, fV, fB, fV, fV, fB, fV, fB, fV, fM + vTxmd},
    /* TxMetadata         */ {0, fV, fB, 0, 0, 0, 0, 0, 0, 0},
    /* TxEntry            */ {0, fB, fB, fV, fM + vKvmd, fB, 0, 0, 0, 0},
    /* ZEntry             */ {0, fB, fB, fM + vEntry, f8, fV, 0, 0, 0, 0},
    /* Signature          */ {0, fB, fB, 0, 0, 0, 0, 0, 0, 0},
    /* DualProof          */ {0, fM + vHdr, fM + vHdr, fB, fB, fB, fB, fM + vLin, fM + vAdv, 0},
    /* LinearProof        */ {0, fV, fV, fB, 0, 0, 0, 0, 0, 0},
    /* LinearAdvanceProof */ {0, fB, fM + vIncl, 0, 0, 0, 0, 0, 0, 0},
    /* InclusionProof     */ {0, fV, fV, fB, 0, 0, 0, 0, 0, 0},
};
// What a message is to verifiedGet: only the answer's own entry, reference,
// metadata, tx header, dual proof and inclusion proof are read; the same
// message types below Tx.kvEntries / zEntries are validated and nothing more.
enum : uint32_t {
    rNone = 0, rRoot, rEntry, rRef, rEmd, rRmd, rEexp, rRexp, rVtx, rTx, rHdr, rDual, rIncl
};
__device__ __forceinline__ uint32_t ve_child_role(uint32_t role, uint32_t f) {
    switch (role * 16 + f) {
    case rRoot * 16 + 1: return rEntry;
    case rRoot * 16 + 2: return rVtx;
    case rRoot * 16 + 3: return rIncl;
    case rEntry * 16 + 4: return rRef;
    case rEntry * 16 + 5: return rEmd;
    case rRef * 16 + 4: return rRmd;
    case rEmd * 16 + 2: return rEexp;
    case rRmd * 16 + 2: return rRexp;
    case rVtx * 16 + 1: return rTx;
    case rVtx * 16 + 2: return rDual;
    case rTx * 16 + 1: return rHdr;
    default: return rNone;
    }
}
enum : uint32_t {  // what was seen (sub-messages) and the metadata flags
    hEntry = 1u << 0, hVtx = 1u << 1, hIncl = 1u << 2, hRef = 1u << 3, hTx = 1u << 4,
    hHdr = 1u << 5, hDual = 1u << 6, hDs = 1u << 7, hDt = 1u << 8, hLin = 1u << 9,
    eDel = 1u << 10, eExp = 1u << 11, eNix = 1u << 12, rDel = 1u << 13, rExp = 1u << 14,
    rNix = 1u << 15
};
constexpr int kVeDepth = 8;  // VerifiableEntry > VerifiableTx > Tx > ZEntry > Entry > Reference
                             // > KVMetadata > Expiration: 7 messages below the root
// The stack of enclosing messages of the envelope kernels (k_pbd_ventry,
// k_pbd_vtx): kVeDepth x 256 words of LDS, lane t's level d at stk[d * 256 +
// t]; a frame is the parent's end (relative to the message, 40 bits), its
// schema row and its role.
__device__ __forceinline__ void ve_push(uint64_t *stk, uint32_t &depth, const uint8_t *base,
                                        const uint8_t *end, uint32_t msg, uint32_t role) {
    stk[depth++ * 256 + threadIdx.x] =
        (uint64_t)(end - base) | (uint64_t)msg << 40 | (uint64_t)role << 48;
}
__device__ __forceinline__ void ve_pop(const uint64_t *stk, uint32_t &depth, const uint8_t *base,
                                       const uint8_t *&end, uint32_t &msg, uint32_t &role) {
    const uint64_t x = stk[--depth * 256 + threadIdx.x];
    end = base + (x & 0xffffffffffull);
    msg = (uint32_t)(x >> 40) & 0xff;
    role = (uint32_t)(x >> 48);
}

// One VerifiableEntry per lane.  WRITE = false: validate, status, count the
// inclusion terms and the DualProof bytes to concatenate; WRITE = true: info,
// terms, concatenations and the DualProof range.  Every read goes through the
// reader of the innermost open message, whose end never exceeds its parent's:
// nothing is read outside [msg_off[p], msg_off[p + 1]) whatever the lengths
// inside claim (DigestFromProto's aligned read of a term may touch up to 3
// bytes beside it, as in the other decoders).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pbd_ventry(uint64_t n, const uint8_t *__restrict__ msgs,
                                                    const uint64_t *__restrict__ msg_off,
                                                    VentryArrays v, int32_t *__restrict__ status) {
    __shared__ uint64_t stk[kVeDepth * 256];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t o0 = msg_off[p], o1 = msg_off[p + 1] >= o0 ? msg_off[p + 1] : o0;
    // the write pass re-reads only what the first pass gave MH_OK
    const bool skip = WRITE && status[p] != MH_OK;
    const uint8_t *base = msgs + o0;
    PbIn in{base, skip ? base : msgs + o1};
    uint32_t msg = vVE, role = rRoot, depth = 0, seen = 0;
    uint64_t etx = 0, rtx = 0, rat = 0, eexp = 0, rexp = 0, lf = 0, wd = 0, kt = 0;
    const uint8_t *kb = base, *vb = base;
    uint64_t kl = 0, vl = 0;
    int32_t ver = 0;
    uint64_t ndual = 0, dlen = 0, dbeg = 0, cpos = 0;
    const uint64_t c0 = WRITE ? v.cat_off[p] : 0, clen = WRITE ? v.cat_off[p + 1] - c0 : 0;
    uint8_t *terms = WRITE ? v.terms + 32 * v.term_off[p] : nullptr;
    bool ok = true;
    for (;;) {
        if (in.p == in.end) {  // the innermost message is read: back to its parent
            if (depth == 0) break;
            ve_pop(stk, depth, base, in.end, msg, role);
            continue;
        }
        uint32_t f, wt;
        if (!(ok = in.key(f, wt))) break;
        const uint32_t kind = f < kVeFields ? kVeSchema[msg][f] : 0;
        if (kind == fV && wt == 0) {
            uint64_t x;
            if (!(ok = in.varint(x))) break;
            const uint32_t b = x != 0;  // protowire.DecodeBool
            switch (role * 16 + f) {
            case rEntry * 16 + 1: etx = x; break;
            case rRef * 16 + 1: rtx = x; break;
            case rRef * 16 + 3: rat = x; break;
            case rEmd * 16 + 1: seen = (seen & ~eDel) | (b ? eDel : 0); break;
            case rEmd * 16 + 3: seen = (seen & ~eNix) | (b ? eNix : 0); break;
            case rRmd * 16 + 1: seen = (seen & ~rDel) | (b ? rDel : 0); break;
            case rRmd * 16 + 3: seen = (seen & ~rNix) | (b ? rNix : 0); break;
            case rEexp * 16 + 1: eexp = x; break;
            case rRexp * 16 + 1: rexp = x; break;
            case rHdr * 16 + 8: ver = (int32_t)(uint32_t)x; break;  // int32: the low 32 bits
            case rIncl * 16 + 1: lf = (uint64_t)(int64_t)(int32_t)(uint32_t)x; break;
            case rIncl * 16 + 2: wd = (uint64_t)(int64_t)(int32_t)(uint32_t)x; break;
            default: break;
            }
        } else if (kind == fB && wt == 2) {
            const uint8_t *b;
            uint64_t bl;
            if (!(ok = in.bytes(b, bl))) break;
            if (role == rEntry && f == 2) kb = b, kl = bl;
            else if (role == rEntry && f == 3) vb = b, vl = bl;
            else if (role == rIncl && f == 3) {
                if (WRITE) digest_from(b, bl, terms + 32 * kt);
                kt++;
            }
        } else if (kind >= fM && wt == 2) {
            uint64_t len;
            if (!(ok = in.varint(len) && len <= (uint64_t)(in.end - in.p) && depth < kVeDepth))
                break;
            switch (role * 16 + f) {
            case rRoot * 16 + 1: seen |= hEntry; break;
            case rRoot * 16 + 2: seen |= hVtx; break;
            case rRoot * 16 + 3: seen |= hIncl; break;
            case rEntry * 16 + 4: seen |= hRef; break;
            case rEmd * 16 + 2: seen |= eExp; break;
            case rRmd * 16 + 2: seen |= rExp; break;
            case rVtx * 16 + 1: seen |= hTx; break;
            case rTx * 16 + 1: seen |= hHdr; break;
            case rDual * 16 + 1: seen |= hDs; break;
            case rDual * 16 + 2: seen |= hDt; break;
            case rDual * 16 + 7: seen |= hLin; break;
            case rVtx * 16 + 2:  // one more occurrence of the DualProof
                seen |= hDual;
                ndual++;
                dlen += len;
                dbeg = (uint64_t)(in.p - msgs);
                if (WRITE && clen) {
                    for (uint64_t j = 0; j < len && cpos < clen; j++) v.cat[c0 + cpos++] = in.p[j];
                }
                break;
            default: break;
            }
            ve_push(stk, depth, base, in.end, msg, role);
            in.end = in.p + len;
            role = ve_child_role(role, f);
            msg = kind - fM;
        } else if (kind == f8 && wt == 1) {
            if (!(ok = in.skip(8))) break;
        } else if (!(ok = in.skip_value(f, wt))) {
            break;
        }
    }
    if (!WRITE) {
        // Go's order: Unmarshal; the nil dereferences of client.go:1145;
        // EntrySpecDigestFor; the nil dereferences of :1150-1161 and of
        // DualProofFromProto (as k_pbd_dual1 reports them)
        const bool have_hdr = (seen & (hVtx | hTx | hHdr)) == (hVtx | hTx | hHdr);
        const uint32_t rest = hIncl | hDual | hDs | hDt | hLin | hEntry;
        const int32_t st = !ok ? MH_ERR_CORRUPTED_DATA
                           : !have_hdr ? MH_ERR_ILLEGAL_ARGUMENTS
                           : (ver != 0 && ver != 1) ? MH_ERR_UNSUPPORTED_TX_VERSION
                           : (seen & rest) != rest ? MH_ERR_ILLEGAL_ARGUMENTS : MH_OK;
        status[p] = st;
        v.cnt[p] = st == MH_OK ? kt : 0;
        v.cnt[n + p] = st == MH_OK && (v.cat_all || ndual > 1) ? dlen : 0;
        return;
    }
    mh_verifiable_entry_info *o = v.info + p;
    uint2 *z = (uint2 *)o;
    static_assert(sizeof(mh_verifiable_entry_info) == 96, "info is zeroed in 8-byte words");
#pragma unroll
    for (int i = 0; i < 12; i++) z[i] = make_uint2(0, 0);
    if (skip) {
        v.dual_beg[p] = v.dual_end[p] = o0;
        return;
    }
    const bool ref = seen & hRef;
    o->entry_tx = etx;
    o->ref_tx = rtx;
    o->ref_at_tx = rat;
    o->key_pos = (uint64_t)(kb - msgs);
    o->key_len = kl;
    o->value_pos = (uint64_t)(vb - msgs);
    o->value_len = vl;
    o->leaf = lf;
    o->width = wd;
    o->tx_version = ver;
    o->has_ref = ref;
    // KVMetadataFromProto + KVMetadata.Bytes() (kv_metadata.go:207-219) of the
    // metadata EncodeEntrySpec / EncodeReference gets
    const bool del = seen & (ref ? rDel : eDel), ex = seen & (ref ? rExp : eExp),
               nix = seen & (ref ? rNix : eNix);
    const uint64_t at = ref ? rexp : eexp;
    uint32_t k = 0;
    if (del) o->md[k++] = 0;
    if (ex) {
        o->md[k++] = 1;
        for (int j = 7; j >= 0; j--) o->md[k++] = (uint8_t)(at >> (8 * j));
    }
    if (nix) o->md[k++] = 2;
    o->md_len = (uint8_t)k;
    // the DualProof: in place when it occurred once, else its concatenation
    const uint64_t cb = (uint64_t)(v.cat - msgs) + c0;
    v.dual_beg[p] = clen ? cb : (ndual == 1 ? dbeg : o0);
    v.dual_end[p] = clen ? cb + clen : (ndual == 1 ? dbeg + dlen : o0);
}

// ---------------------------------------------------------------- VerifiableTx
// proto.Unmarshal into schema.VerifiableTx as pkg/client reads the answer of a
// verified write (VerifiedSet client.go:1337-1391, SetAll streams.go:205-260,
// VerifiedSetReferenceAt :1716-1770, VerifiedZAddAt :1882-1940) or of
// VerifiedTxByID (:1554-1583): the envelope pass rooted one level below
// k_pbd_ventry's, over the same schema table (kVeSchema) and the same LDS
// stack (ve_push / ve_pop).
// Beyond what that kernel reads, the roles of Tx.entries, their KVMetadata and
// the header's TxMetadata:
enum : uint32_t { rTxEntry = rIncl + 1, rTmd, rTexp, rHmd };
__device__ __forceinline__ uint32_t vtx_child_role(uint32_t role, uint32_t f) {
    switch (role * 16 + f) {
    case rTx * 16 + 2: return rTxEntry;
    case rTxEntry * 16 + 4: return rTmd;
    case rTmd * 16 + 2: return rTexp;
    case rHdr * 16 + 9: return rHmd;
    default: return ve_child_role(role, f);
    }
}

// One VerifiableTx per lane.  WRITE = false: validate, status (the whole
// ladder of the call, include/immustore_merkle.h: it depends on no hash), the
// live flag (status MH_OK and the count rule held) and the DualProof bytes to
// concatenate; WRITE = true: the tx header with its canonical metadata, the
// DualProof range, and for a live write answer one VtxRec per entry i < K at
// slot spec_off[p] + i (TxFromProto, database_protoconv.go:69-95, keeps key,
// hValue and metadata of every entry).  Entries beyond K are validated and
// counted only.  Reads stay inside the message as in k_pbd_ventry.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pbd_vtx(uint64_t n, const uint8_t *__restrict__ msgs,
                                                 const uint64_t *__restrict__ msg_off, VtxArrays v,
                                                 int32_t *__restrict__ status) {
    __shared__ uint64_t stk[kVeDepth * 256];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t o0 = msg_off[p], o1 = msg_off[p + 1] >= o0 ? msg_off[p + 1] : o0;
    const uint32_t kind = v.kind[p];
    const uint64_t s0 = v.spec_off[p], K = v.spec_off[p + 1] - s0;
    const bool skip = WRITE && status[p] != MH_OK;
    const bool rec_on = WRITE && !skip && kind != MH_VTX_TX_BY_ID && v.live[p];
    VtxRec *recs = WRITE ? v.recs + (s0 - v.spec_base) : nullptr;
    mh_tx_header *h = WRITE ? v.hdr + p : nullptr;
    if (WRITE) *h = mh_tx_header{};
    const uint8_t *base = msgs + o0;
    PbIn in{base, skip ? base : msgs + o1};
    uint32_t msg = vVtx, role = rVtx, depth = 0, seen = 0;
    uint64_t nent = 0, hn = 0;
    int32_t ver = 0;
    MdState md;
    // the open TxEntry: key, hValue, KVMetadata flags (eDel / eExp / eNix)
    const uint8_t *ekb = base, *ehb = base;
    uint64_t ekl = 0, ehl = 0, eexp = 0;
    uint32_t ef = 0;
    uint64_t ndual = 0, dlen = 0, dbeg = 0, cpos = 0;
    const uint64_t c0 = WRITE ? v.cat_off[p] : 0, clen = WRITE ? v.cat_off[p + 1] - c0 : 0;
    bool ok = true;
    for (;;) {
        if (in.p == in.end) {  // the innermost message is read: back to its parent
            if (depth == 0) break;
            if (role == rTxEntry) {  // one more element of Tx.entries
                if (rec_on && nent < K) {
                    VtxRec *r = recs + nent;
                    digest_from(ehb, ehl, r->hv);
                    r->key_pos = (uint64_t)(ekb - msgs);
                    r->key_len = ekl;
                    // KVMetadataFromProto + KVMetadata.Bytes() (kv_metadata.go:207-219)
                    uint32_t k = 0;
                    if (ef & eDel) r->md[k++] = 0;
                    if (ef & eExp) {
                        r->md[k++] = 1;
                        for (int j = 7; j >= 0; j--) r->md[k++] = (uint8_t)(eexp >> (8 * j));
                    }
                    if (ef & eNix) r->md[k++] = 2;
                    r->md_len = (uint8_t)k;
                }
                nent++;
            }
            ve_pop(stk, depth, base, in.end, msg, role);
            continue;
        }
        uint32_t f, wt;
        if (!(ok = in.key(f, wt))) break;
        const uint32_t fk = f < kVeFields ? kVeSchema[msg][f] : 0;
        if (fk == fV && wt == 0) {
            uint64_t x;
            if (!(ok = in.varint(x))) break;
            const uint32_t b = x != 0;  // protowire.DecodeBool
            switch (role * 16 + f) {
            case rHdr * 16 + 1: if (WRITE) h->id = x; break;
            case rHdr * 16 + 3: if (WRITE) h->ts = (int64_t)x; break;
            case rHdr * 16 + 4: hn = (uint32_t)x; break;  // int32: the low 32 bits
            case rHdr * 16 + 6: if (WRITE) h->bl_tx_id = x; break;
            case rHdr * 16 + 8: ver = (int32_t)(uint32_t)x; break;
            case rHmd * 16 + 1: md.trunc = x; break;
            case rTmd * 16 + 1: ef = (ef & ~eDel) | (b ? eDel : 0); break;
            case rTmd * 16 + 3: ef = (ef & ~eNix) | (b ? eNix : 0); break;
            case rTexp * 16 + 1: eexp = x; break;
            default: break;
            }
        } else if (fk == fB && wt == 2) {
            const uint8_t *b;
            uint64_t bl;
            if (!(ok = in.bytes(b, bl))) break;
            switch (role * 16 + f) {
            case rHdr * 16 + 2: if (WRITE) digest_from(b, bl, h->prev_alh); break;
            case rHdr * 16 + 5: if (WRITE) digest_from(b, bl, h->eh); break;
            case rHdr * 16 + 7: if (WRITE) digest_from(b, bl, h->bl_root); break;
            case rHmd * 16 + 2: md.extra = b, md.extra_len = bl; break;
            case rTxEntry * 16 + 1: ekb = b, ekl = bl; break;
            case rTxEntry * 16 + 2: ehb = b, ehl = bl; break;
            default: break;
            }
        } else if (fk >= fM && wt == 2) {
            uint64_t len;
            if (!(ok = in.varint(len) && len <= (uint64_t)(in.end - in.p) && depth < kVeDepth))
                break;
            switch (role * 16 + f) {
            case rVtx * 16 + 1: seen |= hTx; break;
            case rTx * 16 + 1: seen |= hHdr; break;
            case rHdr * 16 + 9: md.present = true; break;
            case rTx * 16 + 2:
                ekb = ehb = base;
                ekl = ehl = eexp = 0;
                ef = 0;
                break;
            case rTmd * 16 + 2: ef |= eExp; break;
            case rDual * 16 + 1: seen |= hDs; break;
            case rDual * 16 + 2: seen |= hDt; break;
            case rDual * 16 + 7: seen |= hLin; break;
            case rVtx * 16 + 2:  // one more occurrence of the DualProof
                seen |= hDual;
                ndual++;
                dlen += len;
                dbeg = (uint64_t)(in.p - msgs);
                if (WRITE && clen) {
                    for (uint64_t j = 0; j < len && cpos < clen; j++) v.cat[c0 + cpos++] = in.p[j];
                }
                break;
            default: break;
            }
            ve_push(stk, depth, base, in.end, msg, role);
            in.end = in.p + len;
            role = vtx_child_role(role, f);
            msg = fk - fM;
        } else if (fk == f8 && wt == 1) {
            if (!(ok = in.skip(8))) break;
        } else if (!(ok = in.skip_value(f, wt))) {
            break;
        }
    }
    if (!WRITE) {
        const bool plain = kind == MH_VTX_SET || kind == MH_VTX_SET_ALL;
        const bool have_hdr = (seen & (hTx | hHdr)) == (hTx | hHdr);
        const uint32_t all = hDual | hDs | hDt | hLin;
        const uint32_t need = kind == MH_VTX_TX_BY_ID || v.state_tx[p] > 0 ? all : (hDual | hDt);
        // Nentries is an int32 on the wire, len(kvs) an int
        const bool cnt_ok = plain ? ((int64_t)(int32_t)(uint32_t)hn == (int64_t)K && nent == K)
                                  : hn == 1;
        int32_t st = MH_OK;
        bool live = false;
        if (!ok) st = MH_ERR_CORRUPTED_DATA;
        else if (kind == MH_VTX_TX_BY_ID) {
            st = (seen & need) != need ? MH_ERR_ILLEGAL_ARGUMENTS : MH_OK;
            live = st == MH_OK;
        } else if (!have_hdr) st = MH_ERR_ILLEGAL_ARGUMENTS;
        else if (!cnt_ok) st = MH_OK;  // Go: ErrCorruptedData; the verdict is ok = 0
        else if (nent == 0) st = MH_ERR_ILLEGAL_ARGUMENTS;  // tx.Entries() slices past the end
        else if (ver != 0 && ver != 1) st = MH_ERR_UNSUPPORTED_TX_VERSION;
        else if ((seen & need) != need) st = MH_ERR_ILLEGAL_ARGUMENTS;
        else live = true;
        status[p] = st;
        v.live[p] = live;
        v.cnt[p] = st == MH_OK && ndual > 1 ? dlen : 0;
        return;
    }
    if (skip) {
        v.dual_beg[p] = v.dual_end[p] = o0;
        return;
    }
    h->nentries = (uint32_t)hn;
    h->version = (uint32_t)ver;
    // TxMetadataFromProto + Bytes(), in this header's own slot
    const uint32_t ml = md_len(md);
    h->md_off = (uint32_t)(p * kMdSlot);
    h->md_len = ml;
    if (ml) md_write(md, v.md_blob + p * kMdSlot);
    const uint64_t cb = (uint64_t)(v.cat - msgs) + c0;
    v.dual_beg[p] = clen ? cb : (ndual == 1 ? dbeg : o0);
    v.dual_end[p] = clen ? cb + clen : (ndual == 1 ? dbeg + dlen : o0);
}

// Two device words into pinned host memory by a kernel store: a small
// read-back without a DMA copy, which would queue behind the large
// host-to-device chunks in flight on the copy engine.
__global__ void k_put2_host(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                            volatile uint64_t *out) {
    if (threadIdx.x == 0) {
        out[0] = *a;
        out[1] = *b;
        __threadfence_system();
    }
}

// The eight totals of a group (entry n of each scanned offset array, kI ..
// kMd) into pinned host memory, as k_put2_host does for two.  so holds the
// kCounts offset arrays back to back, n + 1 entries each.
__global__ void k_put8_host(const uint64_t *__restrict__ so, uint64_t n, volatile uint64_t *out) {
    if (threadIdx.x < kCounts) {
        out[threadIdx.x] = so[(uint64_t)threadIdx.x * (n + 1) + n];
        __threadfence_system();
    }
}

}  // namespace

// write = false: status and the kCounts x n counts, write = true: o at its
// scanned offsets
static hipError_t launch_pbd_dual1(hipStream_t st, bool write, uint64_t n, const uint8_t *msgs,
                                   const uint64_t *beg, const uint64_t *end, uint64_t *cnt,
                                   const Dual1Arrays &o, int32_t *status) {
    if (!n) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (write)
        hipLaunchKernelGGL(k_pbd_dual1<true>, dim3(grid), dim3(256), 0, st, n, msgs, beg, end,
                           nullptr, o, status);
    else
        hipLaunchKernelGGL(k_pbd_dual1<false>, dim3(grid), dim3(256), 0, st, n, msgs, beg, end, cnt,
                           Dual1Arrays{}, status);
    return hipGetLastError();
}

Dual1Scratch dual1_decode_scratch(Layout &L, uint64_t M) {
    Dual1Scratch s;
    s.cnt = L.add(kCounts * M * 8);
    s.so = L.add(kCounts * (M + 1) * 8);
    s.scan_bytes = pb_scan_temp_bytes(M);
    s.scan = L.add(s.scan_bytes);
    s.hdr = L.add(2 * M * sizeof(mh_tx_header));
    s.md = L.add(2 * M * (uint64_t)kMdSlot);
    s.tbl_alh = L.add(M * 32);
    s.flags = L.add(2 * M);
    s.lin = L.add(2 * M * 8);
    return s;
}

int dual1_decode_size(mh_ctx *c, uint64_t nk, const uint8_t *dmsg, const uint64_t *beg,
                      const uint64_t *end, uint8_t *base, const Dual1Scratch &s, int32_t *status,
                      uint64_t totals[kCounts]) {
    hipStream_t st = c->stream;
    MH_HIP(c->p_small.ensure(kCounts * 8));
    uint64_t *cnt = (uint64_t *)(base + s.cnt);
    {
        TimerScope ts(c->tm(), "pbd_dual1_size", st);
        MH_HIP(launch_pbd_dual1(st, false, nk, dmsg, beg, end, cnt, Dual1Arrays{}, status));
    }
    for (int j = 0; j < kCounts; j++)
        MH_HIP(scan_offsets_u64(st, nk, cnt + j * nk, s.off(base, j, nk), base + s.scan,
                                s.scan_bytes));
    // the totals size the term area: stored by a kernel into pinned memory
    // (the DMA engine is busy with the next chunks)
    volatile uint64_t *tot = c->p_small.as<volatile uint64_t>();
    hipLaunchKernelGGL(k_put8_host, dim3(1), dim3(64), 0, st, s.off(base, 0, nk), nk,
                       (uint64_t *)c->p_small.p);
    MH_HIP(hipGetLastError());
    MH_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < kCounts; j++) totals[j] = tot[j];
    return MH_OK;
}

Dual1Terms dual1_decode_terms(Layout &T, const uint64_t totals[kCounts]) {
    Dual1Terms t;
    for (int j = 0; j < 5; j++) t.terms[j] = T.add(totals[j] * 32);
    t.qterms = T.add(totals[kQT] * 32);
    t.qoff = T.add((totals[kQ] + 1) * 8);
    return t;
}

int dual1_decode_write(mh_ctx *c, uint64_t nk, const uint8_t *dmsg, const uint64_t *beg,
                       const uint64_t *end, uint8_t *base, const Dual1Scratch &s, uint8_t *dt,
                       const Dual1Terms &t, int32_t *status, Dual1Arrays &o) {
    for (int j = 0; j < kCounts; j++) o.off[j] = s.off(base, j, nk);
    for (int j = 0; j < 5; j++) o.terms[j] = dt + t.terms[j];
    o.qterms = dt + t.qterms;
    o.qoff = (uint64_t *)(dt + t.qoff);
    o.src_hdr = (mh_tx_header *)(base + s.hdr);
    o.tgt_hdr = o.src_hdr + nk;
    o.md_blob = base + s.md;
    o.tbl_alh = base + s.tbl_alh;
    o.has_lin = base + s.flags;
    o.has_adv = base + s.flags + nk;
    o.lin_src = (uint64_t *)(base + s.lin);
    o.lin_tgt = o.lin_src + nk;
    TimerScope ts(c->tm(), "pbd_dual1_write", c->stream);
    MH_HIP(launch_pbd_dual1(c->stream, true, nk, dmsg, beg, end, nullptr, o, status));
    return MH_OK;
}

hipError_t launch_pbd_ventry(hipStream_t st, bool write, uint64_t n, const uint8_t *msgs,
                             const uint64_t *msg_off, const VentryArrays &v, int32_t *status) {
    if (!n) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (write)
        hipLaunchKernelGGL(k_pbd_ventry<true>, dim3(grid), dim3(256), 0, st, n, msgs, msg_off, v,
                           status);
    else
        hipLaunchKernelGGL(k_pbd_ventry<false>, dim3(grid), dim3(256), 0, st, n, msgs, msg_off, v,
                           status);
    return hipGetLastError();
}

hipError_t launch_pbd_vtx(hipStream_t st, bool write, uint64_t n, const uint8_t *msgs,
                          const uint64_t *msg_off, const VtxArrays &v, int32_t *status) {
    if (!n) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (write)
        hipLaunchKernelGGL(k_pbd_vtx<true>, dim3(grid), dim3(256), 0, st, n, msgs, msg_off, v, status);
    else
        hipLaunchKernelGGL(k_pbd_vtx<false>, dim3(grid), dim3(256), 0, st, n, msgs, msg_off, v,
                           status);
    return hipGetLastError();
}

hipError_t launch_put2_host(hipStream_t st, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    hipLaunchKernelGGL(k_put2_host, dim3(1), dim3(64), 0, st, a, b, out);
    return hipGetLastError();
}

extern "C" int mh_dual_proof_v2_pb_decode_batch(
    mh_ctx *c, uint64_t n, const uint8_t *msgs, const uint64_t *msg_off, mh_tx_header *src_hdr,
    mh_tx_header *tgt_hdr, uint8_t *md_blob, uint64_t *incl_off, uint8_t *incl_terms,
    uint64_t incl_cap, uint64_t *cons_off, uint8_t *cons_terms, uint64_t cons_cap,
    int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c || (n && (!msg_off || !src_hdr || !tgt_hdr || !md_blob || !incl_off || !cons_off ||
                         !status)))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) {
            if (incl_off) incl_off[0] = 0;
            if (cons_off) cons_off[0] = 0;
            return MH_OK;
        }
        if (2 * n * (uint64_t)kMdSlot > 0xffffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // md_off
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (!monotonic(msg_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t m0 = msg_off[0], mb = msg_off[n] - m0;
        if (mb && !msgs) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        Layout L;
        const uint64_t b_msg = L.add(mb + 16), b_off = L.add((n + 1) * 8), b_ni = L.add(n * 8),
                       b_nc = L.add(n * 8), b_nm = L.add(n * 8), b_io = L.add((n + 1) * 8),
                       b_co = L.add((n + 1) * 8), b_mo = L.add((n + 1) * 8), b_st = L.add(n * 4),
                       b_scan = L.add(pb_scan_temp_bytes(n)),
                       b_h = L.add(2 * n * sizeof(mh_tx_header)),
                       b_md = L.add(2 * n * (uint64_t)kMdSlot);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        if (mb) MH_HIP(hipMemcpyAsync(base + b_msg, msgs + m0, mb, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        const unsigned grid = (unsigned)((n + 255) / 256);
        const uint8_t *dmsg = base + b_msg - m0;
        uint64_t *io = (uint64_t *)(base + b_io), *co = (uint64_t *)(base + b_co),
                 *mo = (uint64_t *)(base + b_mo);
        hipLaunchKernelGGL(k_pbd_dual<false>, dim3(grid), dim3(256), 0, st, n, dmsg,
                           (const uint64_t *)(base + b_off), (uint64_t *)(base + b_ni),
                           (uint64_t *)(base + b_nc), (uint64_t *)(base + b_nm), nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           (int32_t *)(base + b_st));
        MH_HIP(hipGetLastError());
        const uint64_t cnt[3] = {b_ni, b_nc, b_nm};
        uint64_t *outs[3] = {io, co, mo};
        for (int k = 0; k < 3; k++)
            MH_HIP(scan_offsets_u64(st, n, (const uint64_t *)(base + cnt[k]), outs[k], base + b_scan));
        uint64_t md_total = 0;
        MH_HIP(hipMemcpyAsync(incl_off, io, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(cons_off, co, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(&md_total, mo + n, 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, base + b_st, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        const uint64_t ti = incl_off[n], tc = cons_off[n];
        if (ti > incl_cap || tc > cons_cap) return MH_ERR_BUFFER_TOO_SMALL;
        if ((ti && !incl_terms) || (tc && !cons_terms)) return MH_ERR_ILLEGAL_ARGUMENTS;
        DevBuf &tb = c->s_tree;
        MH_HIP(tb.ensure(std::max<uint64_t>(ti + tc, 1) * 32));
        uint8_t *dti = tb.as<uint8_t>(), *dtc = dti + ti * 32;
        hipLaunchKernelGGL(k_pbd_dual<true>, dim3(grid), dim3(256), 0, st, n, dmsg,
                           (const uint64_t *)(base + b_off), nullptr, nullptr, nullptr, io, co, mo,
                           dti, dtc, (mh_tx_header *)(base + b_h),
                           (mh_tx_header *)(base + b_h) + n, base + b_md, (int32_t *)(base + b_st));
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(src_hdr, base + b_h, n * sizeof(mh_tx_header), hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(tgt_hdr, base + b_h + n * sizeof(mh_tx_header),
                              n * sizeof(mh_tx_header), hipMemcpyDeviceToHost, st));
        if (md_total) MH_HIP(hipMemcpyAsync(md_blob, base + b_md, md_total, hipMemcpyDeviceToHost, st));
        if (ti) MH_HIP(hipMemcpyAsync(incl_terms, dti, ti * 32, hipMemcpyDeviceToHost, st));
        if (tc) MH_HIP(hipMemcpyAsync(cons_terms, dtc, tc * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

extern "C" int mh_htree_inclusion_proof_pb_decode_batch(mh_ctx *c, uint64_t n, const uint8_t *msgs,
                                                        const uint64_t *msg_off, uint64_t *leaf,
                                                        uint64_t *width, uint64_t *term_off,
                                                        uint8_t *terms, uint64_t term_cap,
                                                        int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c || (n && (!msg_off || !leaf || !width || !term_off || !status)))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) {
            if (term_off) term_off[0] = 0;
            return MH_OK;
        }
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (!monotonic(msg_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t m0 = msg_off[0], mb = msg_off[n] - m0;
        if (mb && !msgs) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        Layout L;
        const uint64_t b_msg = L.add(mb + 16), b_off = L.add((n + 1) * 8), b_cnt = L.add(n * 8),
                       b_to = L.add((n + 1) * 8), b_st = L.add(n * 4),
                       b_scan = L.add(pb_scan_temp_bytes(n)),
                       b_lw = L.add(2 * n * 8);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        if (mb) MH_HIP(hipMemcpyAsync(base + b_msg, msgs + m0, mb, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        const unsigned grid = (unsigned)((n + 255) / 256);
        const uint8_t *dmsg = base + b_msg - m0;
        uint64_t *to = (uint64_t *)(base + b_to), *lw = (uint64_t *)(base + b_lw);
        hipLaunchKernelGGL(k_pbd_incl<false>, dim3(grid), dim3(256), 0, st, n, dmsg,
                           (const uint64_t *)(base + b_off), (uint64_t *)(base + b_cnt), nullptr,
                           nullptr, nullptr, nullptr, (int32_t *)(base + b_st));
        MH_HIP(hipGetLastError());
        MH_HIP(scan_offsets_u64(st, n, (const uint64_t *)(base + b_cnt), to, base + b_scan));
        MH_HIP(hipMemcpyAsync(term_off, to, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, base + b_st, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        const uint64_t tt = term_off[n];
        if (tt > term_cap) return MH_ERR_BUFFER_TOO_SMALL;
        if (tt && !terms) return MH_ERR_ILLEGAL_ARGUMENTS;
        DevBuf &tb = c->s_tree;
        MH_HIP(tb.ensure(std::max<uint64_t>(tt, 1) * 32));
        hipLaunchKernelGGL(k_pbd_incl<true>, dim3(grid), dim3(256), 0, st, n, dmsg,
                           (const uint64_t *)(base + b_off), nullptr, to, tb.as<uint8_t>(), lw,
                           lw + n, (int32_t *)(base + b_st));
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(leaf, lw, n * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(width, lw + n, n * 8, hipMemcpyDeviceToHost, st));
        if (tt) MH_HIP(hipMemcpyAsync(terms, tb.as<uint8_t>(), tt * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

extern "C" int mh_dual_proof_pb_decode_batch(mh_ctx *c, uint64_t n, const uint8_t *msgs,
                                             const uint64_t *msg_off, mh_dual_proof_decoded *out,
                                             int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c || !out) return MH_ERR_ILLEGAL_ARGUMENTS;
        uint64_t *offs[kCounts - 1] = {out->incl_off,   out->cons_off,           out->last_off,
                                       out->linear_off, out->advance_off,        out->advance_incl_first,
                                       nullptr};  // nested term offsets: advance_incl_off below
        if (n && (!msg_off || !status || !out->src_hdr || !out->tgt_hdr || !out->md_blob ||
                  !out->target_bl_tx_alh || !out->has_linear || !out->linear_src ||
                  !out->linear_tgt || !out->has_advance || !out->advance_incl_off))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        for (int j = 0; j < kQT; j++)
            if (!offs[j]) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) {
            for (int j = 0; j < kQT; j++) offs[j][0] = 0;
            if (out->advance_incl_off) out->advance_incl_off[0] = 0;
            out->nested_proofs = out->nested_terms = 0;
            return MH_OK;
        }
        if (2 * n * (uint64_t)kMdSlot > 0xffffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // md_off
        if (n > 0x7fffffffull) return MH_ERR_ILLEGAL_ARGUMENTS;  // hipcub's int item count
        if (!monotonic(msg_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t m0 = msg_off[0], mb = msg_off[n] - m0;
        if (mb && !msgs) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        Layout L;
        const uint64_t b_msg = L.add(mb + 16), b_off = L.add((n + 1) * 8), b_st = L.add(n * 4);
        const Dual1Scratch ds = dual1_decode_scratch(L, n);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        if (mb) MH_HIP(hipMemcpyAsync(base + b_msg, msgs + m0, mb, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        const uint8_t *dmsg = base + b_msg - m0;
        const uint64_t *doff = (const uint64_t *)(base + b_off);
        int32_t *dst = (int32_t *)(base + b_st);
        uint64_t totals[kCounts];
        if (int e = dual1_decode_size(c, n, dmsg, doff, nullptr, base, ds, dst, totals)) return e;
        // the offsets and the statuses leave on every return
        for (int j = 0; j < kQT; j++)
            MH_HIP(hipMemcpyAsync(offs[j], ds.off(base, j, n), (n + 1) * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(status, dst, n * 4, hipMemcpyDeviceToHost, st));
        out->nested_proofs = totals[kQ];
        out->nested_terms = totals[kQT];
        const uint64_t caps[kCounts - 1] = {out->incl_cap,   out->cons_cap,        out->last_cap,
                                            out->linear_cap, out->advance_cap,     out->advance_incl_cap,
                                            out->advance_incl_terms_cap};
        uint8_t *hterms[5] = {out->incl_terms, out->cons_terms, out->last_terms, out->linear_terms,
                              out->advance_terms};
        int rc = MH_OK;  // a short capacity is reported before a missing pointer
        for (int j = 0; j < 5; j++)
            if (totals[j] && !hterms[j]) rc = MH_ERR_ILLEGAL_ARGUMENTS;
        if (totals[kQT] && !out->advance_incl_terms) rc = MH_ERR_ILLEGAL_ARGUMENTS;
        for (int j = 0; j < kCounts - 1; j++)
            if (totals[j] > caps[j]) rc = MH_ERR_BUFFER_TOO_SMALL;
        if (rc) {  // the copies above still write the caller's arrays
            MH_HIP(hipStreamSynchronize(st));
            return rc;
        }
        Layout T;
        const Dual1Terms dterms = dual1_decode_terms(T, totals);
        DevBuf &tb = c->s_tree;
        MH_HIP(tb.ensure(T.total + 8));
        uint8_t *dt = tb.as<uint8_t>();
        Dual1Arrays o;
        if (int e = dual1_decode_write(c, n, dmsg, doff, nullptr, base, ds, dt, dterms, dst, o))
            return e;
        const size_t hb = n * sizeof(mh_tx_header);
        MH_HIP(hipMemcpyAsync(out->src_hdr, o.src_hdr, hb, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->tgt_hdr, o.tgt_hdr, hb, hipMemcpyDeviceToHost, st));
        if (totals[kMd])
            MH_HIP(hipMemcpyAsync(out->md_blob, o.md_blob, totals[kMd], hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->target_bl_tx_alh, o.tbl_alh, n * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->has_linear, o.has_lin, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->has_advance, o.has_adv, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->linear_src, o.lin_src, n * 8, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->linear_tgt, o.lin_tgt, n * 8, hipMemcpyDeviceToHost, st));
        for (int j = 0; j < 5; j++)
            if (totals[j])
                MH_HIP(hipMemcpyAsync(hterms[j], o.terms[j], totals[j] * 32, hipMemcpyDeviceToHost, st));
        if (totals[kQT])
            MH_HIP(hipMemcpyAsync(out->advance_incl_terms, o.qterms, totals[kQT] * 32,
                                  hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(out->advance_incl_off, o.qoff, (totals[kQ] + 1) * 8,
                              hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

// DualProofV2 straight from the wire, in the chunk frame of PbChunkFrame
// (capi_internal.hpp): chunk k is decoded and verified by dual_proof_v2_core
// (capi_tx.hip; with kDp1V0MetadataDropped) on the compute stream as soon as
// its copy has landed.  The verifier's scratch is sized for the largest chunk
// and reused chunk after chunk (one compute stream orders them).
extern "C" int mh_verify_dual_proof_v2_pb_batch(mh_ctx *c, uint64_t n, const uint8_t *msgs,
                                                const uint64_t *msg_off, const uint64_t *src,
                                                const uint64_t *tgt, const uint8_t *src_alh,
                                                const uint8_t *tgt_alh, int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) return MH_OK;
        PbChunkFrame F;
        if (int e = F.open(c, n, msgs, msg_off, src && tgt && src_alh && tgt_alh && status)) return e;
        const std::vector<uint64_t> &cut = F.cut;
        const uint64_t m0 = F.m0, mb = F.mb, chunk_bytes = F.chunk_bytes;
        const int nch = F.nch;
        hipStream_t st = c->stream;
        uint64_t max_nk = 0;
        for (int k = 0; k < nch; k++) max_nk = std::max(max_nk, cut[k + 1] - cut[k]);
        const size_t scan_bytes = pb_scan_temp_bytes(max_nk);
        Layout L;
        // caller arrays (xa: the source Alh values, then the target ones), the
        // decode's arrays (per-chunk offset arrays hold n_k + 1 entries at
        // [lo + k, hi + k]), then one chunk's verifier scratch
        const uint64_t nc = n + (uint64_t)nch;
        const uint64_t b_msg = L.add(mb + 16), b_off = L.add((n + 1) * 8), b_src = L.add(n * 8),
                       b_tgt = L.add(n * 8), b_xa = L.add(2 * n * 32), b_cnt = L.add(3 * n * 8),
                       b_io = L.add(nc * 8), b_co = L.add(nc * 8), b_mo = L.add(nc * 8),
                       b_st = L.add(n * 4), b_scan = L.add(scan_bytes),
                       b_hd = L.add(2 * n * sizeof(mh_tx_header)),
                       b_md = L.add(2 * n * (uint64_t)kMdSlot),
                       b_core = L.add(dual_proof_v2_scratch_bytes(max_nk));
        MH_HIP(c->s_tx.ensure(L.total));
        // term area reused chunk after chunk: a well-formed term costs >= 34
        // message bytes (tag, length, 32-byte digest), so this rarely grows;
        // sized from the batch itself when it is smaller than one chunk
        DevBuf &tb = c->s_tree;
        MH_HIP(tb.ensure(std::max<uint64_t>(std::min(mb, chunk_bytes) / 34 + 64, 1) * 32));
        uint8_t *base = c->s_tx.as<uint8_t>();
        ChunkCopier cc(c);
        F.fill(cc, base + b_msg,
               {{base + b_off, msg_off, (n + 1) * 8},
                {base + b_src, src, n * 8},
                {base + b_tgt, tgt, n * 8},
                {base + b_xa, src_alh, n * 32},
                {base + b_xa + n * 32, tgt_alh, n * 32}});
        MH_HIP(cc.start());
        const uint8_t *dmsg = base + b_msg - m0;
        int32_t *dst_all = (int32_t *)(base + b_st);
        for (int k = 0; k < nch; k++) {
            MH_HIP(cc.wait(k));
            MH_HIP(hipStreamWaitEvent(st, c->ev_chunks[k], 0));
            const uint64_t lo = cut[k], nk = cut[k + 1] - lo;
            const unsigned grid = (unsigned)((nk + 255) / 256);
            const uint64_t *doff = (const uint64_t *)(base + b_off) + lo;
            uint64_t *cnt = (uint64_t *)(base + b_cnt);
            uint64_t *io = (uint64_t *)(base + b_io) + lo + k, *co = (uint64_t *)(base + b_co) + lo + k,
                     *mo = (uint64_t *)(base + b_mo) + lo + k;
            int32_t *dst = dst_all + lo;
            uint8_t *md = base + b_md + 2 * lo * (uint64_t)kMdSlot;
            // decode: validate + count, scans
            hipLaunchKernelGGL(k_pbd_dual<false>, dim3(grid), dim3(256), 0, st, nk, dmsg, doff,
                               cnt + lo, cnt + n + lo, cnt + 2 * n + lo, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, dst);
            MH_HIP(hipGetLastError());
            uint64_t *outs[3] = {io, co, mo};
            for (int q = 0; q < 3; q++)
                MH_HIP(scan_offsets_u64(st, nk, cnt + q * n + lo, outs[q], base + b_scan, scan_bytes));
            // the chunk's term totals size its term area: one small read-back
            // (waits for this chunk only; later chunks keep copying), stored
            // by a kernel into pinned memory rather than copied by the DMA
            // engine that is busy with the next chunks
            volatile uint64_t *tot = c->p_small.as<volatile uint64_t>();
            MH_HIP(launch_put2_host(st, io + nk, co + nk, (uint64_t *)c->p_small.p));
            MH_HIP(hipStreamSynchronize(st));
            MH_HIP(tb.ensure(std::max<uint64_t>(tot[0] + tot[1], 1) * 32));
            uint8_t *dti = tb.as<uint8_t>(), *dtc = dti + tot[0] * 32;
            mh_tx_header *hd = (mh_tx_header *)(base + b_hd) + 2 * lo;
            hipLaunchKernelGGL(k_pbd_dual<true>, dim3(grid), dim3(256), 0, st, nk, dmsg, doff,
                               nullptr, nullptr, nullptr, io, co, mo, dti, dtc, hd, hd + nk, md, dst);
            MH_HIP(hipGetLastError());
            // VerifyDualProofV2 (verification.go:303-370)
            if (int e = dual_proof_v2_core(st, c->tm(), nk, hd, hd + nk, md, io, dti, co, dtc,
                                           (const uint64_t *)(base + b_src) + lo,
                                           (const uint64_t *)(base + b_tgt) + lo,
                                           base + b_xa + lo * 32, base + b_xa + (n + lo) * 32, dst,
                                           2 * nk * (uint64_t)kMdSlot, kDp1V0MetadataDropped,
                                           base + b_core, dst))
                return e;
        }
        MH_HIP(cc.join());
        MH_HIP(hipMemcpyAsync(status, dst_all, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

// DualProof (v1) straight from the wire: the chunk frame of the V2 call above
// (PbChunkFrame) and its groups, the decode stage of
// mh_dual_proof_pb_decode_batch (dual1_decode_size / _write) into device
// scratch, then dual_proof_v1_core (capi_tx.hip) -- the verifier behind
// mh_verify_dual_proof_batch too -- over the decoded arrays, with
// kDp1V0MetadataDropped: a v0 header's metadata bytes are not hashed.  The
// decode scratch is sized for the largest group of chunks and reused
// group after group (one compute stream orders them); only status and ok
// leave the device.
extern "C" int mh_verify_dual_proof_pb_batch(mh_ctx *c, uint64_t n, const uint8_t *msgs,
                                             const uint64_t *msg_off, const uint64_t *src,
                                             const uint64_t *tgt, const uint8_t *src_alh,
                                             const uint8_t *tgt_alh, int32_t *status, uint8_t *ok) {
    return mh_guard([&]() -> int {
        if (!c) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (n == 0) return MH_OK;
        PbChunkFrame F;
        if (int e = F.open(c, n, msgs, msg_off, src && tgt && src_alh && tgt_alh && status && ok))
            return e;
        hipStream_t st = c->stream;
        F.group();
        Layout L;
        // the caller's arrays and the results, whole; then one group's decode
        const uint64_t b_msg = L.add(F.mb + 16), b_off = L.add((n + 1) * 8), b_src = L.add(n * 8),
                       b_tgt = L.add(n * 8), b_xa = L.add(2 * n * 32), b_st = L.add(n * 4),
                       b_ok = L.add(n);
        const Dual1Scratch ds = dual1_decode_scratch(L, F.group_n);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        ChunkCopier cc(c);
        F.fill(cc, base + b_msg,
               {{base + b_off, msg_off, (n + 1) * 8},
                {base + b_src, src, n * 8},
                {base + b_tgt, tgt, n * 8},
                {base + b_xa, src_alh, n * 32},
                {base + b_xa + n * 32, tgt_alh, n * 32}});
        MH_HIP(cc.start());
        const uint8_t *dmsg = base + b_msg - F.m0;
        int32_t *dst_all = (int32_t *)(base + b_st);
        DevBuf &tb = c->s_tree;
        for (int g = 0; g < F.ng; g++) {
            uint64_t lo, nk;
            if (int e = F.wait_group(c, cc, g, lo, nk)) return e;
            const uint64_t *doff = (const uint64_t *)(base + b_off) + lo;
            int32_t *dst = dst_all + lo;
            uint64_t totals[kCounts];
            if (int e = dual1_decode_size(c, nk, dmsg, doff, nullptr, base, ds, dst, totals)) return e;
            // the term area, then the verifier's scratch
            const uint64_t Q = totals[kQ];
            Layout T;
            const Dual1Terms dterms = dual1_decode_terms(T, totals);
            const uint64_t t_core = T.add(dual_proof_v1_scratch_bytes(nk, Q));
            MH_HIP(tb.ensure(T.total + 8));
            uint8_t *dt = tb.as<uint8_t>();
            Dual1Arrays o;
            if (int e = dual1_decode_write(c, nk, dmsg, doff, nullptr, base, ds, dt, dterms, dst, o))
                return e;
            // VerifyDualProof (verification.go:127-235)
            if (int e = dual_proof_v1_core(st, c->tm(), nk, o, (const uint64_t *)(base + b_src) + lo,
                                           (const uint64_t *)(base + b_tgt) + lo,
                                           base + b_xa + lo * 32, base + b_xa + (n + lo) * 32, dst,
                                           2 * nk * (uint64_t)kMdSlot, kDp1V0MetadataDropped, Q,
                                           dt + t_core, base + b_ok + lo))
                return e;
        }
        MH_HIP(cc.join());
        MH_HIP(hipMemcpyAsync(status, dst_all, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(ok, base + b_ok, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}
