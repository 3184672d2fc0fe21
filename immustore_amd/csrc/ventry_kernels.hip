// ventry_kernels.hip -- the hashing of a verified get on CDNA4, one answer
// per lane: what pkg/client's verifiedGet (pkg/client/client.go:1158-1199)
// computes between the decode of a VerifiableGet answer and VerifyDualProof.
//
//   database.EncodeEntrySpec / EncodeReference   pkg/database/meta.go:54-89
//   store.EntrySpecDigest_v0 / _v1               embedded/store/verification.go:257-302
//   htree.VerifyInclusion                        embedded/htree/htree.go:166-195
//   TxHeader.Alh                                 embedded/store/tx.go:249-319
//
// The envelope pass (k_pbd_ventry, pb_decode.hip) has located the fields and
// the DualProof decoder (k_pbd_dual1) has written the two headers; this
// kernel hashes the value where it lies in the message, builds the digest,
// walks the inclusion proof against the Eh of the header that is the entry's
// transaction, hashes that header, and leaves the arguments of
// dual_proof_v1_core (capi_tx.hip).
//
// Cost shape: a lane runs 1 + (prefix + value bytes + 9) / 64 compressions
// for the value, 2-3 for the digest, 1 + 2 per inclusion term, and 4-7 for
// the header; a wave lasts as long as its longest value, so a batch of mixed
// value lengths pays the longest of every 64.
#include <algorithm>

#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "tx_alh.hpp"

namespace mh {

namespace {

__global__ __launch_bounds__(256) void k_ventry_verify(uint64_t n, VentryVerify v) {
    extern __shared__ uint32_t tab[];
    node_tab_init(tab);
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint2 *za = (uint2 *)(v.src_alh + 32 * p), *zb = (uint2 *)(v.tgt_alh + 32 * p);
    if (v.status[p] != MH_OK) {  // nothing located: a dead proof for the verifier
        v.src[p] = v.tgt[p] = 0;
        v.incl_ok[p] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) za[i] = zb[i] = make_uint2(0, 0);
        return;
    }
    const mh_verifiable_entry_info *e = v.info + p;
    const uint64_t S = v.state_tx[p], at = v.at_tx[p];
    const bool ref = e->has_ref;
    const uint64_t vtx = at ? at : (ref ? e->ref_tx : e->entry_tx);  // client.go:1158-1172
    // hVal = SHA256(0x00 || value), or, a reference (meta.go:81-89),
    // SHA256(0x01 || BE64(atTx) || 0x00 || entry.key)
    uint32_t hv[8], dg[8];
    {
        uint32_t pre[4] = {0, 0, 0, 0};
        const uint64_t rat = e->ref_at_tx;
        if (ref) {
            pre[0] = 0x01000000u | (uint32_t)(rat >> 40);
            pre[1] = (uint32_t)(rat >> 8);
            pre[2] = (uint32_t)(rat & 0xff) << 24;
        }
        const uint8_t *b = v.msgs + (ref ? e->key_pos : e->value_pos);
        sha256_seg<false>(pre, ref ? 10u : 1u, b, ref ? e->key_len : e->value_len, hv, hv);
    }
    // EntrySpecDigest_v1: BE16 mdLen || md || BE16 kLen || key || hVal with key
    // = 0x00 || kReq.Key; _v0: key || hVal (metadata ignored)
    {
        const uint64_t k0 = v.key_off[p], k1 = max(v.key_off[p + 1], k0), kl = k1 - k0;
        uint32_t pre[4] = {0, 0, 0, 0}, plen = 1;  // v0: the key's 0x00 prefix
        if (e->tx_version == 1) {
            const uint32_t ml = min((uint32_t)e->md_len, (uint32_t)MH_MAX_KV_METADATA_LEN);
            put_pre(pre, 1, ml);
            for (uint32_t i = 0; i < ml; i++) put_pre(pre, 2 + i, e->md[i]);
            const uint32_t klen = (uint32_t)((kl + 1) & 0xffff);  // uint16(kLen)
            put_pre(pre, 2 + ml, klen >> 8);
            put_pre(pre, 3 + ml, klen & 0xff);
            plen = 5 + ml;  // the key's 0x00 prefix is byte 4 + ml
        }
        sha256_seg<true>(pre, plen, v.keys + k0, kl, hv, dg);
    }
    // htree.VerifyInclusion, as k_htree_verify walks it (Go's signed ints)
    uint32_t calc[8];
    leaf_hash(dg, calc);
    int64_t i = (int64_t)e->leaf, r = (int64_t)(e->width - 1);
    const uint64_t t0 = v.term_off[p], t1 = max(v.term_off[p + 1], t0);
    for (uint64_t t = t0; t < t1; t++) {
        uint32_t term[8], l[8], rr[8];
        load_digest(v.terms + t * 32, term);
        const bool calc_left = (i % 2 == 0) && (i != r);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            l[j] = calc_left ? calc[j] : term[j];
            rr[j] = calc_left ? term[j] : calc[j];
        }
        node_hash_tab(l, rr, calc, tab);
        i /= 2;
        r /= 2;
    }
    // the entry's transaction is the target of the proof when the state is
    // not ahead of it, else its source (client.go:1177-1191)
    const bool fwd = S <= vtx;
    const mh_tx_header *h = fwd ? v.tgt_hdr + p : v.src_hdr + p;
    uint32_t x = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) x |= calc[j] ^ bswap(((const uint32_t *)h->eh)[j]);
    // Alh of that header; one that Go cannot hash (tx.go:283-286) fails the answer
    const bool hashable = h->version <= 1;
    uint8_t *mine = fwd ? v.tgt_alh : v.src_alh, *theirs = fwd ? v.src_alh : v.tgt_alh;
    if (hashable) {
        tx_alh_one(p, *h, v.md_blob, h->eh, v.alh_msg + p * kTxInnerStride, nullptr, nullptr, mine,
                   nullptr);
    } else {
        uint2 *z = (uint2 *)(mine + 32 * p);
#pragma unroll
        for (int j = 0; j < 4; j++) z[j] = make_uint2(0, 0);
    }
    copy32_a8(theirs + 32 * p, v.state_alh + 32 * p);
    v.src[p] = fwd ? S : vtx;
    v.tgt[p] = fwd ? vtx : S;
    v.incl_ok[p] = (i == r) && x == 0 && hashable;
}

__global__ __launch_bounds__(256) void k_ventry_verdict(
    uint64_t n, const int32_t *__restrict__ status, const uint64_t *__restrict__ state_tx,
    const uint8_t *__restrict__ incl_ok, const uint8_t *__restrict__ dual_ok,
    const uint64_t *__restrict__ tgt, const uint8_t *__restrict__ tgt_alh, uint8_t *__restrict__ ok,
    uint64_t *__restrict__ new_tx, uint8_t *__restrict__ new_alh) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    // client.go:1193-1213: the inclusion, then the dual proof unless there is
    // no state yet
    const bool r = status[p] == MH_OK && incl_ok[p] && (state_tx[p] == 0 || dual_ok[p]);
    ok[p] = r;
    new_tx[p] = r ? tgt[p] : 0;
    const uint2 *a = (const uint2 *)(tgt_alh + 32 * p);
    uint2 *o = (uint2 *)(new_alh + 32 * p);
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = r ? a[j] : make_uint2(0, 0);
}

// ---------------------------------------------------------------- VerifiableTx
// What pkg/client does with the answer of a verified write between the decode
// and VerifyDualProof (VerifiedSet client.go:1341-1376, streamVerifiedSet
// streams.go:209-246, VerifiedSetReferenceAt :1720-1755, VerifiedZAddAt
// :1886-1921), one lane per spec slot, then one per answer.
//
//   TxFromProto / BuildHashTree     database_protoconv.go:69-95, tx.go:332-355
//   TxEntryDigest_v0 / _v1          embedded/store/tx.go:690-731
//   Tx.IndexOf / Tx.Proof           tx.go:361-386
//   EncodeKey / EncodeEntrySpec / EncodeReference   pkg/database/meta.go:50-89
//   EntrySpecDigest_v0 / _v1        embedded/store/verification.go:257-302

// the answer that owns absolute slot a: spec_off[p] <= a < spec_off[p + 1]
__device__ __forceinline__ uint64_t vtx_owner(const VtxVerify &v, uint64_t a) {
    uint64_t lo = 0, hi = v.nk;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (v.spec_off[mid + 1] <= a) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// BE16 mdLen || md || BE16 kLen (|| 0x00 with pfx) as a register prefix -> its length
__device__ __forceinline__ uint32_t vtx_head(uint32_t (&pre)[4], const uint8_t *md, uint32_t ml,
                                             uint64_t klen, uint32_t pfx) {
    put_pre(pre, 1, ml);
    for (uint32_t i = 0; i < ml; i++) put_pre(pre, 2 + i, md[i]);
    put_pre(pre, 2 + ml, (uint32_t)(klen >> 8) & 0xff);  // uint16(kLen)
    put_pre(pre, 3 + ml, (uint32_t)klen & 0xff);
    return 4 + ml + pfx;
}

// d_i = TxEntryDigest of entry i as the wire gives it, the key hashed where it
// lies in the message
__global__ __launch_bounds__(256) void k_vtx_leaf(uint64_t T, VtxVerify v) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t p = vtx_owner(v, v.spec_off[0] + t);
    if (!v.live[p]) return;
    const VtxRec *r = v.recs + t;
    const uint32_t ver = v.hdr[p].version;
    const uint32_t ml = min((uint32_t)r->md_len, (uint32_t)MH_MAX_KV_METADATA_LEN);
    uint32_t hv[8], d[8], pre[4] = {0, 0, 0, 0}, plen = 0;
    load_digest(r->hv, hv);
    if (ver == 1) plen = vtx_head(pre, r->md, ml, r->key_len, 0);
    sha256_seg<true>(pre, plen, v.msgs + r->key_pos, r->key_len, hv, d);
    store_digest(v.dig + 32 * t, d);
    v.dok[t] = ver == 1 || ml == 0;  // ErrMetadataUnsupported, tx.go:692-700
}

// x_i = EntrySpecDigest of the request's spec i, j_i = Tx.IndexOf(its key),
// xok = x_i == d_{j_i}: what VerifyInclusion of the tree's own proof decides
__global__ __launch_bounds__(256) void k_vtx_spec(uint64_t T, VtxVerify v) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t a = v.spec_off[0] + t, p = vtx_owner(v, a);
    if (!v.live[p]) return;
    const uint32_t kind = v.kind[p], ver = v.hdr[p].version;
    const uint64_t k0 = v.key_off[a], kl = max(v.key_off[a + 1], k0) - k0;
    const uint64_t v0 = v.val_off[a];
    const uint64_t vl = kind == MH_VTX_ZADD ? 0 : max(v.val_off[a + 1], v0) - v0;
    uint32_t hv[8], x[8];
    {
        uint32_t pre[4] = {0, 0, 0, 0}, plen = kind == MH_VTX_ZADD ? 0u : 1u;
        if (kind == MH_VTX_REFERENCE) {  // 0x01 || BE64(atTx) || 0x00 || referenced key
            const uint64_t at = v.at_tx[p];
            pre[0] = 0x01000000u | (uint32_t)(at >> 40);
            pre[1] = (uint32_t)(at >> 8);
            pre[2] = (uint32_t)(at & 0xff) << 24;
            plen = 10;
        }
        sha256_seg<false>(pre, plen, v.vals + v0, vl, hv, hv);
    }
    const uint32_t pfx = kind == MH_VTX_ZADD ? 0u : 1u;  // EncodeKey's 0x00
    {
        const bool plain = kind == MH_VTX_SET || kind == MH_VTX_SET_ALL;
        const VtxRec *r = v.recs + t;  // the metadata of the entry at the spec's position
        const uint32_t ml = plain ? min((uint32_t)r->md_len, (uint32_t)MH_MAX_KV_METADATA_LEN) : 0u;
        uint32_t pre[4] = {0, 0, 0, 0}, plen = pfx;
        if (ver == 1) plen = vtx_head(pre, r->md, ml, kl + pfx, pfx);
        sha256_seg<true>(pre, plen, v.keys + k0, kl, hv, x);
    }
    const uint64_t s0 = v.spec_off[p], K = v.spec_off[p + 1] - s0, g0 = s0 - v.spec_off[0];
    const uint8_t *key = v.keys + k0;
    uint64_t j = K;
    for (uint64_t c = 0; c < K && j == K; c++) {
        const VtxRec *e = v.recs + g0 + c;
        if (e->key_len != kl + pfx) continue;
        const uint8_t *ek = v.msgs + e->key_pos;
        bool eq = !pfx || ek[0] == 0;
        for (uint64_t i = 0; eq && i < kl; i++) eq = ek[pfx + i] == key[i];
        if (eq) j = c;
    }
    uint32_t diff = 1;
    if (j < K) {
        uint32_t d[8];
        load_digest(v.dig + 32 * (g0 + j), d);
        diff = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) diff |= d[i] ^ x[i];
    }
    v.xok[t] = diff == 0;
}

// One answer per lane: the AND of its slots, the deleted / v0-metadata / Eh
// rules, the Alh of the tx header with the rebuilt Eh, and the arguments of
// dual_proof_v1_core; VerifiedTxByID's choice of sides (client.go:1559-1569)
__global__ __launch_bounds__(256) void k_vtx_answer(VtxVerify v) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= v.nk) return;
    uint2 *za = (uint2 *)(v.src_alh + 32 * p), *zb = (uint2 *)(v.tgt_alh + 32 * p),
          *ze = (uint2 *)(v.eh_out + 32 * p);
#pragma unroll
    for (int i = 0; i < 4; i++) za[i] = zb[i] = ze[i] = make_uint2(0, 0);
    v.src[p] = v.tgt[p] = 0;
    v.pre_ok[p] = 0;
    if (v.status[p] != MH_OK || !v.live[p]) return;
    const uint64_t S = v.state_tx[p];
    const uint32_t kind = v.kind[p];
    if (kind == MH_VTX_TX_BY_ID) {
        const uint64_t t = v.at_tx[p];
        const bool fwd = S <= t;
        const mh_tx_header *h = fwd ? v.tgt_hdr + p : v.src_hdr + p;
        const bool hashable = h->version <= 1;  // innerHash panics otherwise (tx.go:283-286)
        uint8_t *mine = fwd ? v.tgt_alh : v.src_alh, *theirs = fwd ? v.src_alh : v.tgt_alh;
        if (hashable)
            tx_alh_one(p, *h, v.dual_md, h->eh, v.alh_msg + p * kTxInnerStride, nullptr, nullptr,
                       mine, nullptr);
        copy32_a8(theirs + 32 * p, v.state_alh + 32 * p);
        v.src[p] = fwd ? S : t;
        v.tgt[p] = fwd ? t : S;
        v.pre_ok[p] = hashable;
        return;
    }
    const uint64_t g0 = v.spec_off[p] - v.spec_off[0], K = v.spec_off[p + 1] - v.spec_off[p];
    uint32_t built = 1, all = 1;
    for (uint64_t c = 0; c < K; c++) {
        built &= v.dok[g0 + c];
        all &= v.xok[g0 + c];
    }
    if (!built) return;  // the tree was never built: tx.Proof fails
    const VtxRec *r0 = v.recs + g0;
    if (kind == MH_VTX_SET && r0->md_len && r0->md[0] == 0) all = 0;  // md.Deleted(), client.go:1355
    const uint2 *eh = (const uint2 *)(v.roots + 32 * p), *th = (const uint2 *)(v.tgt_hdr[p].eh);
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ze[i] = eh[i];
        x |= (eh[i].x ^ th[i].x) | (eh[i].y ^ th[i].y);
    }
    tx_alh_one(p, v.hdr[p], v.md_blob, v.roots + 32 * p, v.alh_msg + p * kTxInnerStride, nullptr,
               nullptr, v.tgt_alh, nullptr);
    copy32_a8(v.src_alh + 32 * p, v.state_alh + 32 * p);
    v.src[p] = S;
    v.tgt[p] = v.hdr[p].id;
    v.pre_ok[p] = all && x == 0;
}

}  // namespace

hipError_t launch_vtx_leaf(hipStream_t st, Timer *tm, uint64_t T, const VtxVerify &v) {
    if (!T) return hipSuccess;
    TimerScope ts(tm, "vtx_leaf", st);
    hipLaunchKernelGGL(k_vtx_leaf, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, T, v);
    return hipGetLastError();
}

hipError_t launch_vtx_spec(hipStream_t st, Timer *tm, uint64_t T, const VtxVerify &v) {
    if (!T) return hipSuccess;
    TimerScope ts(tm, "vtx_spec", st);
    hipLaunchKernelGGL(k_vtx_spec, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, T, v);
    return hipGetLastError();
}

hipError_t launch_vtx_answer(hipStream_t st, Timer *tm, const VtxVerify &v) {
    if (!v.nk) return hipSuccess;
    TimerScope ts(tm, "vtx_answer", st);
    hipLaunchKernelGGL(k_vtx_answer, dim3((unsigned)((v.nk + 255) / 256)), dim3(256), 0, st, v);
    return hipGetLastError();
}

hipError_t launch_ventry_verify(hipStream_t st, Timer *tm, uint64_t nk, const VentryVerify &v) {
    if (!nk) return hipSuccess;
    TimerScope ts(tm, "ventry_verify", st);
    hipLaunchKernelGGL(k_ventry_verify, dim3((unsigned)((nk + 255) / 256)), dim3(256),
                       kNodeTabBytes, st, nk, v);
    return hipGetLastError();
}

hipError_t launch_ventry_verdict(hipStream_t st, Timer *tm, uint64_t nk, const int32_t *status,
                                 const uint64_t *state_tx, const uint8_t *incl_ok,
                                 const uint8_t *dual_ok, const uint64_t *tgt,
                                 const uint8_t *tgt_alh, uint8_t *ok, uint64_t *new_tx,
                                 uint8_t *new_alh) {
    if (!nk) return hipSuccess;
    TimerScope ts(tm, "ventry_verdict", st);
    hipLaunchKernelGGL(k_ventry_verdict, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, nk,
                       status, state_tx, incl_ok, dual_ok, tgt, tgt_alh, ok, new_tx, new_alh);
    return hipGetLastError();
}

}  // namespace mh
