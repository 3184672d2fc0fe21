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

// byte k (0..15) of a 16-byte big-endian register prefix |= b
__device__ __forceinline__ void put_pre(uint32_t (&pre)[4], uint32_t k, uint32_t b) {
    const uint32_t x = b << (24 - 8 * (k & 3));
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) pre[w] |= (k >> 2) == w ? x : 0u;
}

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

}  // namespace

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
