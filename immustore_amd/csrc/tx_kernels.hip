// tx_kernels.hip -- the transaction layer around the Merkle path on CDNA4.
//
//   TxHeader.innerHash / Alh             embedded/store/tx.go:249-319        (a7)
//   advanceLinearHash / VerifyLinearProof embedded/store/verification.go:32-64 (a13)
//   leafFor                              embedded/store/verification.go:237-242
//   many small htrees at once            htree.BuildWith (htree.go:68-113) per tx,
//                                        for the read path (tx.go:605-630, a14)
//                                        and for concurrent BuildHashTree calls
//                                        (tx.go:332-355, immustore.go:1632)
//   entry-digest messages from raw tx-log records (tx.go:520-588 + 690-731)
//
// Everything is one message (or one chain) per lane; the per-tx work is a few
// compressions, so these kernels are latency/occupancy shaped rather than
// roofline shaped, and they exist so that no hashing of this layer runs on
// the host.
#include <algorithm>
#include <mutex>
#include <vector>

#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "tx_alh.hpp"

namespace mh {

static inline unsigned grid_for(uint64_t threads, unsigned block) {
    return (unsigned)((threads + block - 1) / block);
}

__global__ __launch_bounds__(256) void k_tx_alh(uint64_t n, const MhTxHeader *__restrict__ hdrs,
                                                const uint8_t *__restrict__ md_blob,
                                                const uint8_t *__restrict__ eh_src,
                                                uint8_t *__restrict__ scratch,
                                                const uint8_t *__restrict__ expect,
                                                const uint64_t *__restrict__ expect_off,
                                                uint8_t *__restrict__ inner_out,
                                                uint8_t *__restrict__ alh_out,
                                                int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const MhTxHeader &h = hdrs[p];
    tx_alh_one(p, h, md_blob, eh_src ? eh_src + p * 32 : h.eh, scratch + p * kTxInnerStride,
               status ? expect + (expect_off ? expect_off[p] : p * 32) : nullptr, inner_out,
               alh_out, status);
}

// leafFor(d) = SHA256(0x00 || d)  (verification.go:237-242, ahtree.go:288-292)
__global__ __launch_bounds__(256) void k_leaf_for(uint64_t n, const uint8_t *__restrict__ in,
                                                  uint8_t *__restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t d[8], h[8];
    load_digest(in + p * 32, d);
    leaf_hash(d, h);
    store_digest(out + p * 32, h);
}

__global__ __launch_bounds__(256) void k_select32(uint64_t n, const uint8_t *__restrict__ sel,
                                                  const uint8_t *__restrict__ x,
                                                  const uint8_t *__restrict__ y,
                                                  uint8_t *__restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint4 *s = reinterpret_cast<const uint4 *>((sel[p] ? x : y) + p * 32);
    uint4 *d = reinterpret_cast<uint4 *>(out + p * 32);
    d[0] = s[0];
    d[1] = s[1];
}

// VerifyLinearProof (verification.go:40-64), one proof per lane.
__global__ __launch_bounds__(256) void k_linear_verify(
    uint64_t n, const uint64_t *__restrict__ psrc, const uint64_t *__restrict__ ptgt,
    const uint64_t *__restrict__ src, const uint64_t *__restrict__ tgt,
    const uint64_t *__restrict__ term_off, const uint8_t *__restrict__ terms,
    const uint8_t *__restrict__ src_alh, const uint8_t *__restrict__ tgt_alh,
    uint8_t *__restrict__ ok) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t s = psrc[p], t = ptgt[p], t0 = term_off[p], t1 = term_off[p + 1];
    bool res = s == src[p] && t == tgt[p] && s != 0 && s <= t && t1 > t0 && (t1 - t0) == t - s + 1;
    uint32_t c[8], x[8];
    if (res) {
        load_digest(terms + t0 * 32, c);
        load_digest(src_alh + p * 32, x);
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) d |= c[j] ^ x[j];
        res = d == 0;
    }
    if (res) {
        for (uint64_t i = 1; i < t1 - t0; i++) {
            uint32_t term[8];
            load_digest(terms + (t0 + i) * 32, term);
            alh_hash(s + i, c, term, c);
        }
        load_digest(tgt_alh + p * 32, x);
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) d |= c[j] ^ x[j];
        res = d == 0;
    }
    ok[p] = res ? 1 : 0;
}

// VerifyLinearAdvanceProof chain (verification.go:106-121) for every proof of
// a batch (the three-way state of verification.go:90-104 stays on the
// device, no proof is compacted away).  Lane p runs only when state[p] == 0,
// which promises cnt[p] + 1 terms from term_off[p] and cnt[p] nested proofs
// from first[p]; any other lane touches no term and no leaf.  calc starts at
// terms[0] (Alh of start+1); before every advance the current calc is written
// to leaves_src[first[p] - first[0] + k] (its leafFor must be included in the
// target tree at index start+1+k), then calc = advanceLinearHash(calc,
// start+2+k, terms[k+1]).  ok[p] = (final calc == end_alh[p]).
__global__ __launch_bounds__(256) void k_advance_chain_gated(
    uint64_t n, const uint8_t *__restrict__ state, const uint64_t *__restrict__ start,
    const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ term_off,
    const uint8_t *__restrict__ terms, const uint64_t *__restrict__ first,
    const uint8_t *__restrict__ end_alh, uint8_t *__restrict__ leaves_src,
    uint8_t *__restrict__ ok) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (state[p] != 0) {
        ok[p] = 0;
        return;
    }
    const uint64_t t0 = term_off[p], c0 = cnt[p], s = start[p], f = first[p] - first[0];
    uint32_t c[8], x[8];
    load_digest(terms + t0 * 32, c);
    for (uint64_t k = 0; k < c0; k++) {
        store_digest(leaves_src + (f + k) * 32, c);
        uint32_t term[8];
        load_digest(terms + (t0 + k + 1) * 32, term);
        alh_hash(s + 2 + k, c, term, c);
    }
    load_digest(end_alh + p * 32, x);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d |= c[j] ^ x[j];
    ok[p] = d == 0;
}

// ------------------------------------------- VerifyDualProof (v1) around the checks
// Everything of store.VerifyDualProof (verification.go:127-235) that is not a
// hash: the argument checks and operands before the checks, the verdict after
// them.  dual_proof_v1_core (capi_tx.hip) strings them together.

// check_header's rule (capi_internal.hpp) on a header's fields; v0_md: what a
// v0 header with metadata means to this caller (Dp1V0Metadata)
__device__ __forceinline__ bool dp1_header_ok(uint32_t version, uint32_t md_len, uint32_t md_off,
                                              uint64_t md_blob_len, bool have_blob, int v0_md) {
    if (version > 1) return false;
    if (md_len == 0) return true;
    if (version == 0) return v0_md == kDp1V0MetadataDropped;
    return md_len <= MH_MAX_TX_METADATA_LEN && have_blob && (uint64_t)md_off + md_len <= md_blob_len;
}

// VerifyDualProof's argument checks (verification.go:128-138) and the
// operands of every later check, one proof per lane.  A header that cannot be
// hashed (dp1_header_ok) kills the proof; a dead proof's headers are hashed as
// empty v1 headers so that the Alh kernel's reads stay inside md_blob, and so
// is the metadata of every v0 header (innerHash never reads it, tx.go:258-263;
// with kDp1V0MetadataRefused such a proof is dead already).  The advance
// proof's state is verification.go:90-104 with both lengths taken from the
// offsets: state 0 promises the chain kernel end - start terms and the nested
// kernels end - start - 1 proofs, all inside this proof's own ranges.
__global__ __launch_bounds__(256) void k_dp1_prep(uint64_t n, Dual1Arrays o,
                                                  const uint64_t *__restrict__ src,
                                                  const uint64_t *__restrict__ tgt,
                                                  const uint8_t *__restrict__ src_alh,
                                                  const uint8_t *__restrict__ tgt_alh,
                                                  const int32_t *__restrict__ status,
                                                  uint64_t md_blob_len, int v0_md, Dp1Ops w) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    // headers read field by field and copied memory to memory: a header held
    // in a local struct lands in scratch
    const mh_tx_header *sh = o.src_hdr + p, *th = o.tgt_hdr + p;
    const uint64_t s = src[p], t = tgt[p], sid = sh->id, tid = th->id, sbl_id = sh->bl_tx_id;
    const uint32_t sv = sh->version, tv = th->version;
    const bool have_blob = o.md_blob != nullptr;
    const bool alive = (!status || status[p] == MH_OK) && sid == s && tid == t && sid != 0 &&
                       sid <= tid &&
                       dp1_header_ok(sv, sh->md_len, sh->md_off, md_blob_len, have_blob, v0_md) &&
                       dp1_header_ok(tv, th->md_len, th->md_off, md_blob_len, have_blob, v0_md);
    const uint64_t tbl_id = th->bl_tx_id;
    const bool a_branch = s < tbl_id;  // verification.go:191 vs :211
    const uint8_t *sa = src_alh + 32 * p, *tba = o.tbl_alh + 32 * p;
    w.alive[p] = alive;
    w.ii[p] = s;
    w.ij[p] = tbl_id;
    w.ci[p] = sbl_id;
    w.ls[p] = a_branch ? tbl_id : s;
    copy32_a8(w.x + 32 * p, sa);
    copy32_a8(w.x + 32 * (n + p), tgt_alh + 32 * p);
    copy32_a8(w.sbl + 32 * p, sh->bl_root);
    copy32_a8(w.tbl + 32 * p, th->bl_root);
    copy32_a8(w.lin_sa + 32 * p, a_branch ? tba : sa);
    copy32_a8(w.end_alh + 32 * p, a_branch ? sa : tba);
    const uint64_t start = sbl_id, end = a_branch ? s : tbl_id;
    uint8_t state;
    if (end < start) state = 2;
    else if (end <= start + 1) state = 1;
    else if (!o.has_adv[p] || o.off[kAdv][p + 1] - o.off[kAdv][p] != end - start ||
             o.off[kQ][p + 1] - o.off[kQ][p] != end - start - 1)
        state = 2;
    else state = 0;
    w.a_state[p] = state;
    w.a_start[p] = start;
    w.a_cnt[p] = state == 0 ? end - start - 1 : 0;
    static_assert(sizeof(mh_tx_header) % 8 == 0, "headers are copied in 8-byte words");
    const uint2 *hs = (const uint2 *)sh, *ht = (const uint2 *)th;
    uint2 *ds = (uint2 *)(w.hh + p), *dd = (uint2 *)(w.hh + n + p);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(mh_tx_header) / 8; i++) {
        ds[i] = hs[i];
        dd[i] = ht[i];
    }
    if (!alive) w.hh[p].version = w.hh[n + p].version = 1;
    if (!alive || sv == 0) w.hh[p].md_len = 0;
    if (!alive || tv == 0) w.hh[n + p].md_len = 0;
}

// Operands of the nested InclusionProofs (verification.go:108-115), one lane
// per proof: lane q is nested proof first[0] + q, and its proof p is the one
// with first[p] <= first[0] + q < first[p + 1].  The q of a proof whose chain
// is not run gets i = j = 0, which the ahtree kernel rejects before it reads
// a term.
__global__ __launch_bounds__(256) void k_dp1_nested(uint64_t nq, uint64_t n,
                                                    const uint64_t *__restrict__ first,
                                                    const uint8_t *__restrict__ a_state,
                                                    const uint64_t *__restrict__ a_start,
                                                    const uint64_t *__restrict__ ij,
                                                    const uint8_t *__restrict__ tbl,
                                                    uint64_t *__restrict__ qi, uint64_t *__restrict__ qj,
                                                    uint8_t *__restrict__ qroot) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint64_t g = first[0] + q;
    uint64_t lo = 0, hi = n;  // first[lo] <= g < first[hi] throughout
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const bool run = a_state[lo] == 0;
    qi[q] = run ? a_start[lo] + 1 + (g - first[lo]) : 0;
    qj[q] = run ? ij[lo] : 0;
    copy32_a8(qroot + 32 * q, tbl + 32 * lo);
}

// The verdict in Go's order (verification.go:140-235), one proof per lane,
// the AND over its nested proofs included.
__global__ __launch_bounds__(256) void k_dp1_verdict(
    uint64_t n, const uint8_t *__restrict__ alive, const int32_t *__restrict__ ast,
    const uint64_t *__restrict__ ii, const uint64_t *__restrict__ ij, const uint64_t *__restrict__ ci,
    const uint8_t *__restrict__ oki, const uint8_t *__restrict__ okc, const uint8_t *__restrict__ okl,
    const uint8_t *__restrict__ has_lin, const uint8_t *__restrict__ oklin,
    const uint8_t *__restrict__ a_state, const uint64_t *__restrict__ a_cnt,
    const uint64_t *__restrict__ first, const uint8_t *__restrict__ aok,
    const uint8_t *__restrict__ qok, uint8_t *__restrict__ ok) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool r = alive[p] && ast[p] == MH_OK && ast[n + p] == MH_OK;
    if (r && ii[p] < ij[p]) r = oki[p];
    if (r && ci[p] > 0) r = okc[p];
    if (r && ij[p] > 0) r = okl[p];
    if (r) r = has_lin[p] && oklin[p];
    if (r) {
        const uint8_t state = a_state[p];
        if (state == 0) {
            r = aok[p];
            const uint64_t f = first[p] - first[0], c0 = a_cnt[p];
            for (uint64_t x = 0; x < c0 && r; x++) r = qok[f + x];
        } else {
            r = state == 1;
        }
    }
    ok[p] = r ? 1 : 0;
}

// ------------------------------------------- VerifyDualProofV2 around the checks
// The same for store.VerifyDualProofV2 (verification.go:303-372), strung
// together by dual_proof_v2_core: the argument checks in Go's order
// (:305-316), then the headers that cannot be hashed, and the operands.  Dead
// proofs and v0 metadata are hashed as in k_dp1_prep.
__global__ __launch_bounds__(256) void k_dpv2_prep(
    uint64_t n, const mh_tx_header *__restrict__ src_hdr, const mh_tx_header *__restrict__ tgt_hdr,
    bool have_blob, const uint64_t *__restrict__ src, const uint64_t *__restrict__ tgt,
    const uint8_t *__restrict__ src_alh, const uint8_t *__restrict__ tgt_alh,
    const int32_t *status_in, uint64_t md_blob_len, int v0_md, mh_tx_header *__restrict__ hh,
    uint8_t *__restrict__ x, uint64_t *ii, uint64_t *ij, uint64_t *ci, uint8_t *sel, uint8_t *sbl,
    uint8_t *tbl, int32_t *status_out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    // headers read field by field and copied memory to memory (see k_dp1_prep)
    const mh_tx_header *sh = src_hdr + p, *th = tgt_hdr + p;
    const uint64_t s = src[p], t = tgt[p], sid = sh->id;
    const uint32_t sv = sh->version, tv = th->version;
    int32_t r = status_in ? status_in[p] : MH_OK;
    if (r == MH_OK) {
        if (sid == 0 || sid != s || th->id != t) r = MH_ERR_ILLEGAL_ARGUMENTS;
        else if (s > t) r = MH_ERR_SOURCE_TX_NEWER;
        else if (!dp1_header_ok(sv, sh->md_len, sh->md_off, md_blob_len, have_blob, v0_md) ||
                 !dp1_header_ok(tv, th->md_len, th->md_off, md_blob_len, have_blob, v0_md))
            r = MH_ERR_ILLEGAL_ARGUMENTS;
    }
    status_out[p] = r;
    dpv2_operands(p, s, sh, th, ii, ij, ci, sel, sbl, tbl);
    copy32_a8(x + 32 * p, src_alh + 32 * p);
    copy32_a8(x + 32 * (n + p), tgt_alh + 32 * p);
    const uint2 *hs = (const uint2 *)sh, *ht = (const uint2 *)th;
    uint2 *ds = (uint2 *)(hh + p), *dd = (uint2 *)(hh + n + p);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(mh_tx_header) / 8; i++) {
        ds[i] = hs[i];
        dd[i] = ht[i];
    }
    if (r != MH_OK) hh[p].version = hh[n + p].version = 1;
    if (r != MH_OK || sv == 0) hh[p].md_len = 0;
    if (r != MH_OK || tv == 0) hh[n + p].md_len = 0;
}

// verification.go:318-370 after the Alh values and the two ahtree proofs
__global__ __launch_bounds__(256) void k_dpv2_verdict(uint64_t n, const mh_tx_header *__restrict__ hh,
                                                      const uint64_t *__restrict__ src,
                                                      const uint64_t *__restrict__ tgt,
                                                      const int32_t *__restrict__ ast,
                                                      const uint8_t *__restrict__ oki,
                                                      const uint8_t *__restrict__ okc,
                                                      int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || status[p] != MH_OK) return;
    status[p] = (ast[p] != MH_OK || ast[n + p] != MH_OK)
                    ? MH_ERR_ILLEGAL_ARGUMENTS  // :318-326
                    : dpv2_ladder(hh + p, hh + n + p, src[p] == tgt[p], oki[p], okc[p]);
}

// Entry digest (tx.go:690-731) -- and, with leaf != 0, its htree leaf
// SHA256(0x00 || digest) (htree.go:79-83) -- hashed in place from the raw
// tx-log entry record (sha256_skip12): no message buffer, no offsets scan.
__device__ __forceinline__ void txe_digest_one(const uint8_t *__restrict__ r, uint8_t ver,
                                               uint32_t d[8]) {
    const uint32_t ml = ((uint32_t)r[0] << 8) | r[1];
    const uint32_t kl = ((uint32_t)r[2 + ml] << 8) | r[3 + ml];
    if (ver == 1)
        sha256_skip12(r, 4 + ml + kl, d);
    else
        sha256_skip12(r + 4 + ml, kl, d);
}

__global__ __launch_bounds__(256) void k_txe_leaf(uint64_t n, const uint8_t *__restrict__ buf,
                                                  const uint64_t *__restrict__ rec_off,
                                                  const uint8_t *__restrict__ ver, int leaf,
                                                  uint8_t *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t d[8];
    txe_digest_one(buf + rec_off[e], ver[e], d);
    if (leaf) {
        uint32_t h[8];
        leaf_hash(d, h);
        store_digest(out + e * 32, h);
    } else {
        store_digest(out + e * 32, d);
    }
}

// TxHeader of each record from the raw tx-log bytes (the fields readHeader
// reads, tx.go:419-518; the host hop already validated the structure), plus
// the offset of its first entry.  md_off is relative to the log buffer.
// returns the offset of the record's first entry
__device__ __forceinline__ uint64_t tx_hdr_one(const uint8_t *__restrict__ buf, uint64_t p,
                                               MhTxHeader &h) {
    const uint8_t *r = buf + p;
    auto be = [&](int o, int n) {
        uint64_t v = 0;
        for (int k = 0; k < n; k++) v = v << 8 | r[o + k];
        return v;
    };
    h.id = be(0, 8);
    h.ts = (int64_t)be(8, 8);
    h.bl_tx_id = be(16, 8);
    for (int k = 0; k < 32; k++) {
        h.bl_root[k] = r[24 + k];
        h.prev_alh[k] = r[56 + k];
        h.eh[k] = 0;
    }
    h.version = (uint32_t)be(88, 2);
    uint64_t q = 90;
    if (h.version == 0) {
        h.nentries = (uint32_t)be(90, 2);
        h.md_len = 0;
        h.md_off = 0;
        q = 92;
    } else {
        h.md_len = (uint32_t)be(90, 2);
        h.md_off = (uint32_t)(p + 92);
        h.nentries = (uint32_t)be(92 + h.md_len, 4);
        q = 96 + h.md_len;
    }
    return p + q;
}

__global__ __launch_bounds__(256) void k_tx_hdr_from_raw(uint64_t ntx, const uint8_t *__restrict__ buf,
                                                         const uint64_t *__restrict__ rec_off,
                                                         MhTxHeader *__restrict__ hdrs,
                                                         uint64_t *__restrict__ ent_start) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntx) return;
    MhTxHeader h;
    ent_start[t] = tx_hdr_one(buf, rec_off[t], h);
    hdrs[t] = h;
}

__global__ __launch_bounds__(256) void k_put_eh(uint64_t n, const uint8_t *__restrict__ eh,
                                                MhTxHeader *__restrict__ hdrs) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    for (int k = 0; k < 32; k++) hdrs[t].eh[k] = eh[t * 32 + k];
}

hipError_t launch_tx_hdr_from_raw(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                                  const uint64_t *rec_off, MhTxHeader *hdrs, uint64_t *ent_start) {
    if (!ntx) return hipSuccess;
    TimerScope ts(tm, "tx_hdr_from_raw", st);
    hipLaunchKernelGGL(k_tx_hdr_from_raw, dim3(grid_for(ntx, 256)), dim3(256), 0, st, ntx, buf,
                       rec_off, hdrs, ent_start);
    return hipGetLastError();
}

// Up to three runs of 64-bit words from pinned host memory into HBM, read by
// the kernel over PCIe: a small upload that does not queue behind the large
// host-to-device copies the DMA engine is busy with (the tx-log chunks).
__global__ __launch_bounds__(256) void k_fetch_host(HostRuns r) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (int k = 0; k < 3; k++)
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.n[k]; i += stride)
            r.dst[k][i] = r.src[k][i];
}

hipError_t launch_fetch_host(hipStream_t st, const HostRuns &r) {
    const uint64_t m = std::max(r.n[0], std::max(r.n[1], r.n[2]));
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_fetch_host, dim3((unsigned)std::min<uint64_t>(grid_for(m, 256), 1024)),
                       dim3(256), 0, st, r);
    return hipGetLastError();
}

// Up to three runs of 32-bit words from HBM into pinned host memory by
// kernel stores over PCIe: results that do not wait for the DMA engine.  A
// run whose ends are 16-byte aligned goes in 16-byte stores (4-byte stores
// reach only ~25 GB/s over the link).
__global__ __launch_bounds__(256) void k_store_host(HostWordRuns r) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < 3; k++) {
        const uint64_t n = r.n[k];
        if ((((uintptr_t)r.src[k] | (uintptr_t)r.dst[k]) & 15) == 0) {
            const uint4 *s = reinterpret_cast<const uint4 *>(r.src[k]);
            uint4 *d = reinterpret_cast<uint4 *>(r.dst[k]);
            for (uint64_t i = tid; i < n / 4; i += stride) d[i] = s[i];
            for (uint64_t i = (n & ~3ull) + tid; i < n; i += stride) r.dst[k][i] = r.src[k][i];
        } else {
            for (uint64_t i = tid; i < n; i += stride) r.dst[k][i] = r.src[k][i];
        }
    }
    __threadfence_system();
}

hipError_t launch_store_host(hipStream_t st, const HostWordRuns &r) {
    const uint64_t m = std::max(r.n[0], std::max(r.n[1], r.n[2]));
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_store_host, dim3((unsigned)std::min<uint64_t>(grid_for(m / 4 + 1, 256), 1024)),
                       dim3(256), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_put_eh(hipStream_t st, uint64_t n, const uint8_t *eh, MhTxHeader *hdrs) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_put_eh, dim3(grid_for(n, 256)), dim3(256), 0, st, n, eh, hdrs);
    return hipGetLastError();
}

// Entry index of a run of tx records (tx.go:520-588 readEntry, structure
// only), one lane per tx: the host hop already validated every length, so
// the lane walks its entries from ent_start[t] and records each entry's
// record offset and header version for k_txe_leaf.
__global__ __launch_bounds__(256) void k_txe_index(uint64_t ntx, const uint8_t *__restrict__ buf,
                                                   const MhTxHeader *__restrict__ hdrs,
                                                   const uint64_t *__restrict__ ent_start,
                                                   const uint64_t *__restrict__ leaf_off,
                                                   uint64_t *__restrict__ rec_off,
                                                   uint8_t *__restrict__ ver) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntx) return;
    const uint8_t v = (uint8_t)hdrs[t].version;
    uint64_t q = ent_start[t];
    for (uint64_t e = leaf_off[t]; e < leaf_off[t + 1]; e++) {
        const uint32_t ml = ((uint32_t)buf[q] << 8) | buf[q + 1];
        const uint32_t kl = ((uint32_t)buf[q + 2 + ml] << 8) | buf[q + 3 + ml];
        rec_off[e] = q;
        ver[e] = v;
        q += 4 + ml + kl + 12 + 32;
    }
}

hipError_t launch_txe_index(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                            const MhTxHeader *hdrs, const uint64_t *ent_start,
                            const uint64_t *leaf_off, uint64_t *rec_off, uint8_t *ver) {
    if (!ntx) return hipSuccess;
    TimerScope ts(tm, "txe_index", st);
    hipLaunchKernelGGL(k_txe_index, dim3(grid_for(ntx, 256)), dim3(256), 0, st, ntx, buf, hdrs,
                       ent_start, leaf_off, rec_off, ver);
    return hipGetLastError();
}

__global__ void k_txlog_patch(uint64_t ne, const uint64_t *__restrict__ e_idx,
                              const uint64_t *__restrict__ e_off, uint64_t *__restrict__ rec_off,
                              uint64_t nh, const uint64_t *__restrict__ h_idx,
                              const uint64_t *__restrict__ h_val, MhTxHeader *__restrict__ hdrs) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ne) rec_off[e_idx[t]] = e_off[t];
    if (t < nh) {
        hdrs[h_idx[t]].md_off = (uint32_t)h_val[t];
        hdrs[h_idx[t]].md_len = (uint32_t)(h_val[t] >> 32);
    }
}

hipError_t launch_txlog_patch(hipStream_t st, uint64_t ne, const uint64_t *e_idx,
                              const uint64_t *e_off, uint64_t *rec_off, uint64_t nh,
                              const uint64_t *h_idx, const uint64_t *h_val, MhTxHeader *hdrs) {
    const uint64_t n = std::max(ne, nh);
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_txlog_patch, dim3(grid_for(n, 256)), dim3(256), 0, st, ne, e_idx, e_off,
                       rec_off, nh, h_idx, h_val, hdrs);
    return hipGetLastError();
}

__device__ __constant__ static const uint8_t kEmptyRootDev[32] = {
    0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
    0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};

// Roots of many small htrees, one lane per tree, level by level in place
// over the tree's own leaf range (exactly htree.go:85-110: node k of the next
// level = H(node 2k, node 2k+1) written to slot k -- slots 2k, 2k+1 >= k are
// read first -- and an odd last node promoted to slot (w-1)/2).  nodes holds
// the leaf hashes of all trees back to back and is consumed.  Width 0 gives
// SHA256(nil) (htree.go:73-77).  For batches whose widest tree is small
// (immudb txs: a handful of entries) this replaces the host tree plan.
__global__ __launch_bounds__(256) void k_small_roots(uint64_t ntrees,
                                                     const uint64_t *__restrict__ leaf_off,
                                                     uint8_t *__restrict__ nodes,
                                                     uint8_t *__restrict__ roots) {
    extern __shared__ uint32_t tab[];
    node_tab_init(tab);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrees) return;
    uint8_t *lv = nodes + (leaf_off[t] - leaf_off[0]) * 32;
    uint64_t w = leaf_off[t + 1] - leaf_off[t];
    const uint4 *src;
    if (w == 0) {
        src = reinterpret_cast<const uint4 *>(kEmptyRootDev);
    } else {
        while (w > 1) {
            const uint64_t half = w / 2;
            for (uint64_t k = 0; k < half; k++) {
                uint32_t a[8], b[8], h[8];
                load_digest(lv + 64 * k, a);
                load_digest(lv + 64 * k + 32, b);
                node_hash_tab(a, b, h, tab);
                store_digest(lv + 32 * k, h);
            }
            if (w & 1) {  // promote the odd last node
                const uint4 *q = reinterpret_cast<const uint4 *>(lv + 32 * (w - 1));
                uint4 *d = reinterpret_cast<uint4 *>(lv + 32 * half);
                const uint4 x = q[0], y = q[1];
                d[0] = x;
                d[1] = y;
            }
            w = (w + 1) / 2;
        }
        src = reinterpret_cast<const uint4 *>(lv);
    }
    uint4 *d = reinterpret_cast<uint4 *>(roots + t * 32);
    d[0] = src[0];
    d[1] = src[1];
}

// The same roots with one WAVE per tree (width <= 64): lane k holds node k of
// the current level in LDS, every level's nodes are hashed at once, so a tree
// costs ceil(log2 w) node-hash latencies instead of w - 1 -- for the small
// batches of a group commit, where the lane-per-tree kernel is one lone
// wave walking each tree serially.
__global__ __launch_bounds__(256) void k_small_roots_wave(uint64_t ntrees,
                                                          const uint64_t *__restrict__ leaf_off,
                                                          const uint8_t *__restrict__ nodes,
                                                          uint8_t *__restrict__ roots) {
    __shared__ uint32_t lvl[4][64][9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * 4 + wv;
    if (t >= ntrees) return;  // wave-uniform
    const uint8_t *lv = nodes + (leaf_off[t] - leaf_off[0]) * 32;
    uint64_t w = leaf_off[t + 1] - leaf_off[t];
    if (w == 0) {
        if (lane < 2)
            reinterpret_cast<uint4 *>(roots + t * 32)[lane] =
                reinterpret_cast<const uint4 *>(kEmptyRootDev)[lane];
        return;
    }
    uint32_t(*L)[9] = lvl[wv];
    if ((uint64_t)lane < w) {
        uint32_t d[8];
        load_digest(lv + 32 * lane, d);
#pragma unroll
        for (int j = 0; j < 8; j++) L[lane][j] = d[j];
    }
    while (w > 1) {  // htree.go:85-110, level by level
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint64_t half = w / 2;
        uint32_t a[8], b[8], h[8];
        const bool hash = (uint64_t)lane < half, promote = (w & 1) && (uint64_t)lane == half;
        if (hash || promote) {
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] = L[promote ? w - 1 : 2 * lane][j];
        }
        if (hash) {
#pragma unroll
            for (int j = 0; j < 8; j++) b[j] = L[2 * lane + 1][j];
            node_hash_g(a, b, h);
        } else {
            copy8(h, a);
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (hash || promote) {
#pragma unroll
            for (int j = 0; j < 8; j++) L[lane][j] = h[j];
        }
        w = (w + 1) / 2;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) {
        uint32_t r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = L[0][j];
        store_digest(roots + t * 32, r);
    }
}

// The same roots for MANY small trees, level-parallel: a 256-thread
// workgroup takes TPW = 512 / P consecutive trees (P = the widest tree rounded
// up to a power of two, <= 64), their leaves in LDS at stride P, and hashes
// every node of a level at once -- node j of tree k at level l on thread
// k * (P >> l) + j, so level 1 keeps all 256 threads busy (for trees of the
// widest width), each further level half as many -- double-buffered in LDS
// (htree.go:85-110: pairs hashed, an odd last node promoted).  Against one
// lane per tree (k_small_roots: w - 1 dependent node hashes on a lone wave
// per SIMD) the work is the same but spread over 8x the waves.
__global__ __launch_bounds__(256) void k_small_roots_pack(uint64_t ntrees,
                                                          const uint64_t *__restrict__ leaf_off,
                                                          const uint8_t *__restrict__ nodes,
                                                          uint8_t *__restrict__ roots, int lgp) {
    __shared__ uint32_t buf[2][512][9];  // +1 word pad: 2j / 2j+1 reads spread over the banks
    const int P = 1 << lgp, TPW = 512 >> lgp;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TPW;
    const uint64_t o0 = leaf_off[0];
    for (int i = tid; i < TPW * P; i += 256) {
        const int k = i >> lgp, j = i & (P - 1);
        const uint64_t t = t0 + k;
        if (t >= ntrees) continue;
        const uint64_t lo = leaf_off[t], w = leaf_off[t + 1] - lo;
        if ((uint64_t)j < w) {
            uint32_t d[8];
            load_digest(nodes + (lo - o0 + j) * 32, d);
#pragma unroll
            for (int q = 0; q < 8; q++) buf[0][i][q] = d[q];
        }
    }
    int cur = 0;
    for (int l = 1; l <= lgp; l++) {
        __syncthreads();
        const int S = P >> l;  // node slots per tree at level l
        if (tid < TPW * S) {
            const int k = tid / S, j = tid - k * S;
            const uint64_t t = t0 + k;
            if (t < ntrees) {
                const uint64_t w = leaf_off[t + 1] - leaf_off[t];
                const uint64_t wp = (w + (1ull << (l - 1)) - 1) >> (l - 1);  // width at level l-1
                const int a = k * P + 2 * j;
                if ((uint64_t)(2 * j + 1) < wp) {
                    uint32_t x[8], y[8], h[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        x[q] = buf[cur][a][q];
                        y[q] = buf[cur][a + 1][q];
                    }
                    node_hash_g(x, y, h);
#pragma unroll
                    for (int q = 0; q < 8; q++) buf[cur ^ 1][k * P + j][q] = h[q];
                } else if ((uint64_t)(2 * j) < wp) {  // odd last node: promoted
#pragma unroll
                    for (int q = 0; q < 8; q++) buf[cur ^ 1][k * P + j][q] = buf[cur][a][q];
                }
            }
        }
        cur ^= 1;
    }
    __syncthreads();
    if (tid < TPW) {
        const uint64_t t = t0 + tid;
        if (t < ntrees) {
            if (leaf_off[t + 1] == leaf_off[t]) {  // width 0: SHA256(nil), htree.go:73-77
                reinterpret_cast<uint4 *>(roots + t * 32)[0] = reinterpret_cast<const uint4 *>(kEmptyRootDev)[0];
                reinterpret_cast<uint4 *>(roots + t * 32)[1] = reinterpret_cast<const uint4 *>(kEmptyRootDev)[1];
            } else {
                uint32_t r[8];
#pragma unroll
                for (int q = 0; q < 8; q++) r[q] = buf[cur][tid * P][q];
                store_digest(roots + t * 32, r);
            }
        }
    }
}

hipError_t launch_small_roots(hipStream_t st, Timer *tm, uint64_t ntrees, const uint64_t *leaf_off,
                              uint8_t *nodes, uint8_t *roots, uint64_t wmax) {
    if (!ntrees) return hipSuccess;
    TimerScope ts(tm, "small_roots", st);
    if (ntrees <= 2048) {
        // few trees: latency-bound, a wave per tree
        hipLaunchKernelGGL(k_small_roots_wave, dim3(grid_for(ntrees, 4)), dim3(256), 0, st, ntrees,
                           leaf_off, nodes, roots);
    } else if (wmax <= 64) {
        int lgp = 0;
        while ((1ull << lgp) < wmax) lgp++;
        lgp = std::max(lgp, 1);
        const uint64_t tpw = 512 >> lgp;
        hipLaunchKernelGGL(k_small_roots_pack, dim3(grid_for(ntrees, (unsigned)tpw)), dim3(256), 0,
                           st, ntrees, leaf_off, nodes, roots, lgp);
    } else {
        hipLaunchKernelGGL(k_small_roots, dim3(grid_for(ntrees, 256)), dim3(256), kNodeTabBytes, st,
                           ntrees, leaf_off, nodes, roots);
    }
    return hipGetLastError();
}

// The levels above a row of w <= 64 inner nodes in ONE launch
// (mh_dev_htree_reduce_nodes for the all-gathered shard roots of a multi-GPU
// build, w = ranks): one wave, node k of the current level on lane k in LDS,
// every level's nodes hashed at once (htree.go:85-110: pairs, an odd last
// node promoted) and written to levels in the flat level-major layout
// (level 0 = the input row), the root to root.  Replaces a copy kernel, the
// level launches and a device-to-device copy per build.
__global__ __launch_bounds__(64) void k_reduce_small(const uint8_t *__restrict__ nodes, uint32_t w,
                                                     uint8_t *__restrict__ levels,
                                                     uint8_t *__restrict__ root) {
    __shared__ uint32_t L[64][9];
    const uint32_t lane = threadIdx.x;
    if (lane < w) {
        uint32_t d[8];
        load_digest(nodes + 32 * lane, d);
#pragma unroll
        for (int j = 0; j < 8; j++) L[lane][j] = d[j];
        store_digest(levels + 32 * lane, d);
    }
    uint64_t off = w;
    while (w > 1) {
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint32_t half = w / 2;
        uint32_t a[8], b[8], h[8];
        const bool hash = lane < half, promote = (w & 1) && lane == half;
        if (hash || promote) {
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] = L[promote ? w - 1 : 2 * lane][j];
        }
        if (hash) {
#pragma unroll
            for (int j = 0; j < 8; j++) b[j] = L[2 * lane + 1][j];
            node_hash_g(a, b, h);
        } else {
            copy8(h, a);
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (hash || promote) {
#pragma unroll
            for (int j = 0; j < 8; j++) L[lane][j] = h[j];
            store_digest(levels + 32 * (off + lane), h);
        }
        w = (w + 1) / 2;
        off += w;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0 && root) {
        uint32_t r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = L[0][j];
        store_digest(root, r);
    }
}

hipError_t launch_reduce_small(hipStream_t st, const uint8_t *nodes, uint64_t w, uint8_t *levels,
                               uint8_t *root) {
    if (w == 0 || w > kSmallTreeMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_reduce_small, dim3(1), dim3(64), 0, st, nodes, (uint32_t)w, levels, root);
    return hipGetLastError();
}

// ---------------------------------------------------------------- many trees
// Level l of a batch of independent htrees.  Item k describes one tree that
// still has > 1 node at level l-1: its nodes at level l are written at
// cur_base[k] .. cur_base[k] + ceil(prev_w[k] / 2), its level-(l-1) nodes
// live at prev_base[k].  Thread i finds its item by binary search over
// cur_base (sorted) and pairs (or promotes) exactly as htree.go:85-110.
__global__ __launch_bounds__(256) void k_seg_level(uint64_t nnodes, uint64_t level_base,
                                                   uint32_t nitems,
                                                   const uint64_t *__restrict__ cur_base,
                                                   const uint64_t *__restrict__ prev_base,
                                                   const uint64_t *__restrict__ prev_w,
                                                   uint8_t *__restrict__ nodes) {
    extern __shared__ uint32_t tab[];
    node_tab_init(tab);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnodes;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = level_base + i;
        uint32_t lo = 0, hi = nitems - 1;
        while (lo < hi) {  // last k with cur_base[k] <= g
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (cur_base[mid] <= g)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint64_t j = g - cur_base[lo];
        const uint64_t lpos = prev_base[lo] + 2 * j;
        uint32_t a[8], o[8];
        load_digest(nodes + lpos * 32, a);
        if (2 * j + 1 < prev_w[lo]) {
            uint32_t b[8];
            load_digest(nodes + (lpos + 1) * 32, b);
            node_hash_tab(a, b, o, tab);
        } else {
            copy8(o, a);
        }
        store_digest(nodes + g * 32, o);
    }
}

__global__ __launch_bounds__(256) void k_gather32(uint64_t n, const uint8_t *__restrict__ src,
                                                  const uint64_t *__restrict__ idx,
                                                  uint8_t *__restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t k = idx[p];
    const uint4 *s = reinterpret_cast<const uint4 *>(k == ~0ull ? kEmptyRootDev : src + k * 32);
    uint4 *d = reinterpret_cast<uint4 *>(out + p * 32);
    d[0] = s[0];
    d[1] = s[1];
}

// ---------------------------------------------------------------- launchers
hipError_t launch_tx_alh(hipStream_t st, Timer *tm, uint64_t n, const MhTxHeader *hdrs,
                         const uint8_t *md_blob, const uint8_t *eh_src, uint8_t *scratch,
                         const uint8_t *expect, const uint64_t *expect_off, uint8_t *inner_out,
                         uint8_t *alh_out, int32_t *status) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "tx_alh", st);
    hipLaunchKernelGGL(k_tx_alh, dim3(grid_for(n, 256)), dim3(256), 0, st, n, hdrs, md_blob,
                       eh_src, scratch, expect, expect_off, inner_out, alh_out, status);
    return hipGetLastError();
}

hipError_t launch_leaf_for(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *in, uint8_t *out) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "leaf_for", st);
    hipLaunchKernelGGL(k_leaf_for, dim3(grid_for(n, 256)), dim3(256), 0, st, n, in, out);
    return hipGetLastError();
}

hipError_t launch_select32(hipStream_t st, uint64_t n, const uint8_t *sel, const uint8_t *x,
                           const uint8_t *y, uint8_t *out) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_select32, dim3(grid_for(n, 256)), dim3(256), 0, st, n, sel, x, y, out);
    return hipGetLastError();
}

hipError_t launch_linear_verify(hipStream_t st, Timer *tm, uint64_t n, const uint64_t *psrc,
                                const uint64_t *ptgt, const uint64_t *src, const uint64_t *tgt,
                                const uint64_t *term_off, const uint8_t *terms,
                                const uint8_t *src_alh, const uint8_t *tgt_alh, uint8_t *ok) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "linear_verify", st);
    hipLaunchKernelGGL(k_linear_verify, dim3(grid_for(n, 256)), dim3(256), 0, st, n, psrc, ptgt,
                       src, tgt, term_off, terms, src_alh, tgt_alh, ok);
    return hipGetLastError();
}

hipError_t launch_advance_chain_gated(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *state,
                                      const uint64_t *start, const uint64_t *cnt,
                                      const uint64_t *term_off, const uint8_t *terms,
                                      const uint64_t *first, const uint8_t *end_alh,
                                      uint8_t *leaves_src, uint8_t *ok) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "advance_chain", st);
    hipLaunchKernelGGL(k_advance_chain_gated, dim3(grid_for(n, 256)), dim3(256), 0, st, n, state,
                       start, cnt, term_off, terms, first, end_alh, leaves_src, ok);
    return hipGetLastError();
}

hipError_t launch_dp1_prep(hipStream_t st, Timer *tm, uint64_t n, const Dual1Arrays &o,
                           const uint64_t *src, const uint64_t *tgt, const uint8_t *src_alh,
                           const uint8_t *tgt_alh, const int32_t *status, uint64_t md_blob_len,
                           Dp1V0Metadata v0_md, const Dp1Ops &w) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "dp1_prep", st);
    hipLaunchKernelGGL(k_dp1_prep, dim3(grid_for(n, 256)), dim3(256), 0, st, n, o, src, tgt, src_alh,
                       tgt_alh, status, md_blob_len, (int)v0_md, w);
    return hipGetLastError();
}

hipError_t launch_dp1_nested(hipStream_t st, Timer *tm, uint64_t nq, uint64_t n,
                             const uint64_t *first, const Dp1Ops &w, uint64_t *qi, uint64_t *qj,
                             uint8_t *qroot) {
    if (!nq) return hipSuccess;
    TimerScope ts(tm, "dp1_nested", st);
    hipLaunchKernelGGL(k_dp1_nested, dim3(grid_for(nq, 256)), dim3(256), 0, st, nq, n, first,
                       w.a_state, w.a_start, w.ij, w.tbl, qi, qj, qroot);
    return hipGetLastError();
}

hipError_t launch_dp1_verdict(hipStream_t st, Timer *tm, uint64_t n, const Dp1Ops &w,
                              const Dp1Results &r, const uint8_t *has_lin, const uint64_t *first,
                              uint8_t *ok) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "dp1_verdict", st);
    hipLaunchKernelGGL(k_dp1_verdict, dim3(grid_for(n, 256)), dim3(256), 0, st, n, w.alive, r.ast,
                       w.ii, w.ij, w.ci, r.oki, r.okc, r.okl, has_lin, r.oklin, w.a_state, w.a_cnt,
                       first, r.aok, r.qok, ok);
    return hipGetLastError();
}

hipError_t launch_dpv2_prep(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *src_hdr,
                            const mh_tx_header *tgt_hdr, bool have_blob, const uint64_t *src,
                            const uint64_t *tgt, const uint8_t *src_alh, const uint8_t *tgt_alh,
                            const int32_t *status_in, uint64_t md_blob_len, Dp1V0Metadata v0_md,
                            mh_tx_header *hh, uint8_t *x, uint64_t *ii, uint64_t *ij,
                            uint64_t *ci, uint8_t *sel, uint8_t *sbl, uint8_t *tbl,
                            int32_t *status_out) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "dpv2_prep", st);
    hipLaunchKernelGGL(k_dpv2_prep, dim3(grid_for(n, 256)), dim3(256), 0, st, n, src_hdr, tgt_hdr,
                       have_blob, src, tgt, src_alh, tgt_alh, status_in, md_blob_len, (int)v0_md, hh,
                       x, ii, ij, ci, sel, sbl, tbl, status_out);
    return hipGetLastError();
}

hipError_t launch_dpv2_proofs(hipStream_t st, Timer *tm, uint64_t n, const uint64_t *ii,
                              const uint64_t *ij, const uint64_t *ci, const uint8_t *sel,
                              const uint8_t *sbl, const uint8_t *tbl, const uint8_t *src_alh_x,
                              const uint64_t *incl_off, const uint8_t *incl_terms,
                              const uint64_t *cons_off, const uint8_t *cons_terms, uint8_t *leaf,
                              uint8_t *ca, uint8_t *oki, uint8_t *okc) {
    if (hipError_t e = launch_leaf_for(st, tm, n, src_alh_x, leaf)) return e;
    if (hipError_t e = launch_ahtree_verify(st, tm, MH_AHT_INCLUSION, n, ii, ij, incl_off,
                                            incl_terms, leaf, tbl, oki, nullptr))
        return e;
    if (hipError_t e = launch_select32(st, n, sel, leaf, sbl, ca)) return e;
    return launch_ahtree_verify(st, tm, MH_AHT_CONSISTENCY, n, ci, ij, cons_off, cons_terms, ca,
                                tbl, okc, nullptr);
}

hipError_t launch_dpv2_verdict(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *hh,
                               const uint64_t *src, const uint64_t *tgt, const int32_t *ast,
                               const uint8_t *oki, const uint8_t *okc, int32_t *status) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "dpv2_verdict", st);
    hipLaunchKernelGGL(k_dpv2_verdict, dim3(grid_for(n, 256)), dim3(256), 0, st, n, hh, src, tgt,
                       ast, oki, okc, status);
    return hipGetLastError();
}

hipError_t launch_txe_leaf(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *buf,
                           const uint64_t *rec_off, const uint8_t *ver, bool leaf, uint8_t *out) {
    if (!n) return hipSuccess;
    TimerScope ts(tm, "txe_leaf", st);
    hipLaunchKernelGGL(k_txe_leaf, dim3(grid_for(n, 256)), dim3(256), 0, st, n, buf, rec_off, ver,
                       leaf ? 1 : 0, out);
    return hipGetLastError();
}

hipError_t launch_seg_level(hipStream_t st, Timer *tm, uint64_t nnodes, uint64_t level_base,
                            uint32_t nitems, const uint64_t *cur_base, const uint64_t *prev_base,
                            const uint64_t *prev_w, uint8_t *nodes) {
    if (!nnodes || !nitems) return hipSuccess;
    TimerScope ts(tm, "seg_level", st);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess)
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(nnodes, 256), (uint64_t)cus * 8);
    hipLaunchKernelGGL(k_seg_level, dim3(grid), dim3(256), kNodeTabBytes, st, nnodes, level_base,
                       nitems, cur_base, prev_base, prev_w, nodes);
    return hipGetLastError();
}

hipError_t launch_gather32(hipStream_t st, uint64_t n, const uint8_t *src, const uint64_t *idx,
                           uint8_t *out) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather32, dim3(grid_for(n, 256)), dim3(256), 0, st, n, src, idx, out);
    return hipGetLastError();
}

}  // namespace mh
