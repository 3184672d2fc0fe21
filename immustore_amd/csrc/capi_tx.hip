// capi_tx.hip -- C ABI of the transaction layer (include/immustore_merkle.h,
// "tx layer" section): header Alh (a7), linear and dual proofs (a13) and
// many-tree htree builds (a3 over many txs).  The tx-log read path (a14) is in
// txlog_hop.hip (host record hop), capi_txlog.hip and capi_clog.hip.
//
// Host code here lays out device buffers and (DualProofV2)
// combines per-proof verdicts; every SHA-256 runs in tx_kernels.hip /
// verify_kernels.hip / htree_kernels.hip.  VerifyDualProof (v1) is stated
// once, in dual_proof_v1_core, and runs on the device from its argument
// checks to its verdict.
#include <cstring>
#include <cstdlib>
#include <vector>

#include "capi_internal.hpp"

// Leaves + levels + roots of a planned batch on `st`.  d_digests: E x 32 on
// the device; d_roots: ntrees x 32.  run_tree_plan uses the ctx's s_tree
// scratch, run_tree_plan_on the caller's.
int run_tree_plan(mh_ctx *c, hipStream_t st, const TreePlan &P, uint64_t ntrees, uint64_t nleaves,
                  const uint8_t *d_digests, uint8_t *d_roots) {
    return run_tree_plan_on(c->s_tree, st, c->tm(), P, ntrees, nleaves, d_digests, d_roots, nullptr);
}

int run_tree_plan_on(DevBuf &scratch, hipStream_t st, Timer *tm, const TreePlan &P, uint64_t ntrees,
                     uint64_t nleaves, const uint8_t *d_digests, uint8_t *d_roots, uint8_t *pinned) {
    Layout L;
    const uint64_t nitems = P.cur.size();
    const uint64_t b_nodes = L.add(std::max<uint64_t>(P.total_nodes, 1) * 32);
    const uint64_t b_cur = L.add(nitems * 8), b_prev = L.add(nitems * 8),
                   b_prevw = L.add(nitems * 8), b_root = L.add(ntrees * 8);
    MH_HIP(scratch.ensure(L.total));
    uint8_t *base = scratch.as<uint8_t>();
    uint8_t *nodes = base + b_nodes;
    // index arrays: straight from the plan's vectors, or through `pinned`
    // (plan_index_bytes(P, ntrees) bytes the caller keeps alive until `st`
    // has passed this point) so the copies stay asynchronous
    const uint64_t *src_cur = P.cur.data(), *src_prev = P.prev.data(),
                   *src_prevw = P.prevw.data(), *src_root = P.root_idx.data();
    if (pinned) {
        uint64_t *q = reinterpret_cast<uint64_t *>(pinned);
        memcpy(q, src_cur, nitems * 8);
        memcpy(q + nitems, src_prev, nitems * 8);
        memcpy(q + 2 * nitems, src_prevw, nitems * 8);
        memcpy(q + 3 * nitems, src_root, ntrees * 8);
        src_cur = q;
        src_prev = q + nitems;
        src_prevw = q + 2 * nitems;
        src_root = q + 3 * nitems;
    }
    if (nitems) {
        MH_HIP(hipMemcpyAsync(base + b_cur, src_cur, nitems * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_prev, src_prev, nitems * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_prevw, src_prevw, nitems * 8, hipMemcpyHostToDevice, st));
    }
    MH_HIP(hipMemcpyAsync(base + b_root, src_root, ntrees * 8, hipMemcpyHostToDevice, st));
    MH_HIP(launch_leaf_for(st, tm, nleaves, d_digests, nodes));  // htree.go:79-83
    for (const auto &lv : P.levels)
        MH_HIP(launch_seg_level(st, tm, lv.nodes, lv.base, (uint32_t)lv.nitems,
                                (const uint64_t *)(base + b_cur) + lv.item0,
                                (const uint64_t *)(base + b_prev) + lv.item0,
                                (const uint64_t *)(base + b_prevw) + lv.item0, nodes));
    MH_HIP(launch_gather32(st, ntrees, nodes, (const uint64_t *)(base + b_root), d_roots));
    return MH_OK;
}


// ------------------------------------------------------------------ a7
// innerHash / Alh of n checked headers (tx.go:249-319); c->mu held by the
// caller.  From pinned host memory the header copy is one DMA.
int tx_alh_core(mh_ctx *c, uint64_t n, const mh_tx_header *hdrs, const uint8_t *md_blob,
                uint64_t md_blob_len, uint8_t *inner_out, uint8_t *alh_out) {
    MH_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    Layout L;
    const uint64_t b_h = L.add(n * sizeof(mh_tx_header)), b_md = L.add(md_blob_len),
                   b_s = L.add(n * kTxInnerStride), b_in = L.add(n * 32), b_a = L.add(n * 32);
    MH_HIP(c->s_tx.ensure(L.total));
    uint8_t *base = c->s_tx.as<uint8_t>();
    MH_HIP(hipMemcpyAsync(base + b_h, hdrs, n * sizeof(mh_tx_header), hipMemcpyHostToDevice, st));
    if (md_blob && md_blob_len)
        MH_HIP(hipMemcpyAsync(base + b_md, md_blob, md_blob_len, hipMemcpyHostToDevice, st));
    MH_HIP(launch_tx_alh(st, c->tm(), n, (const MhTxHeader *)(base + b_h), base + b_md, nullptr,
                         base + b_s, nullptr, nullptr, base + b_in, base + b_a, nullptr));
    if (inner_out) MH_HIP(hipMemcpyAsync(inner_out, base + b_in, n * 32, hipMemcpyDeviceToHost, st));
    MH_HIP(hipMemcpyAsync(alh_out, base + b_a, n * 32, hipMemcpyDeviceToHost, st));
    MH_HIP(hipStreamSynchronize(st));
    return MH_OK;
}

extern "C" int mh_tx_alh_batch(mh_ctx *c, uint64_t n, const mh_tx_header *hdrs,
                               const uint8_t *md_blob, uint64_t md_blob_len, uint8_t *inner_out,
                               uint8_t *alh_out) {
    return mh_guard([&]() -> int {
        if (!c || (n && (!hdrs || !alh_out))) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!n) return MH_OK;
        for (uint64_t k = 0; k < n; k++)
            if (int e = check_header(hdrs[k], md_blob_len, md_blob != nullptr)) return e;
        std::lock_guard<std::mutex> lk(c->mu);
        return tx_alh_core(c, n, hdrs, md_blob, md_blob_len, inner_out, alh_out);
    });
}

extern "C" int mh_dev_tx_alh_batch(mh_ctx *c, uint64_t n, const mh_tx_header *hdrs,
                                   const uint8_t *md_blob, const uint8_t *eh, uint8_t *scratch,
                                   uint8_t *inner_out, uint8_t *alh_out) {
    return mh_guard([&]() -> int {
        if (!c || (n && (!hdrs || !scratch || !alh_out))) return MH_ERR_ILLEGAL_ARGUMENTS;
        // store_digest: uint4 stores (eh, md_blob and scratch are read and written byte by byte)
        if (((uintptr_t)inner_out | (uintptr_t)alh_out) & 15) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!n) return MH_OK;
        hipSetDevice(c->device);
        MH_HIP(launch_tx_alh(c->stream, c->tm(), n, hdrs, md_blob, eh, scratch, nullptr, nullptr,
                             inner_out, alh_out, nullptr));
        return MH_OK;
    });
}

// ------------------------------------------------------------------ a3 x many
// Roots of many htrees over device digests d_dig (leaf_off: host, ntrees + 1,
// rebased so leaf_off[0] is d_dig's first digest) into device d_roots, on st;
// scratch: two device buffers of the caller (the small-tree leaves + offsets).
int build_many_dev(mh_ctx *c, hipStream_t st, uint64_t ntrees, const uint64_t *leaf_off,
                   const uint8_t *d_dig, uint8_t *d_roots, DevBuf &s_lv, DevBuf &s_lo) {
    const uint64_t E = leaf_off[ntrees] - leaf_off[0];
    uint64_t wmax = 0;
    for (uint64_t t = 0; t < ntrees; t++) wmax = std::max(wmax, leaf_off[t + 1] - leaf_off[t]);
    if (small_roots_fit(ntrees, wmax)) {  // one lane (or wave) per tree, no host plan
        MH_HIP(s_lv.ensure(std::max<uint64_t>(E, 1) * 32));
        MH_HIP(s_lo.ensure((ntrees + 1) * 8));
        MH_HIP(hipMemcpyAsync(s_lo.p, leaf_off, (ntrees + 1) * 8, hipMemcpyHostToDevice, st));
        MH_HIP(launch_leaf_for(st, c->tm(), E, d_dig, s_lv.as<uint8_t>()));  // htree.go:79-83
        MH_HIP(launch_small_roots(st, c->tm(), ntrees, s_lo.as<uint64_t>(), s_lv.as<uint8_t>(),
                                  d_roots, wmax));
        // leaf_off is the caller's host memory: done with it before returning
        MH_HIP(hipStreamSynchronize(st));
    } else {
        TreePlan P;
        P.build(ntrees, leaf_off);
        if (int e = run_tree_plan(c, st, P, ntrees, E, d_dig, d_roots)) return e;
        MH_HIP(hipStreamSynchronize(st));  // the plan's host vectors go out of scope
    }
    return MH_OK;
}

extern "C" int mh_htree_build_many(mh_ctx *c, uint64_t ntrees, const uint64_t *leaf_off,
                                   const uint8_t *digests, uint8_t *roots) {
    return mh_guard([&]() -> int {
        if (!c || (ntrees && (!leaf_off || !roots))) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!ntrees) return MH_OK;
        for (uint64_t t = 0; t < ntrees; t++)
            if (leaf_off[t + 1] < leaf_off[t]) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t E = leaf_off[ntrees] - leaf_off[0];
        if (E && !digests) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        hipSetDevice(c->device);
        hipStream_t st = c->stream;
        Layout L;
        const uint64_t b_d = L.add(std::max<uint64_t>(E, 1) * 32), b_r = L.add(ntrees * 32);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        if (E)
            MH_HIP(hipMemcpyAsync(base + b_d, digests + leaf_off[0] * 32, E * 32,
                                  hipMemcpyHostToDevice, st));
        if (int e = build_many_dev(c, st, ntrees, leaf_off, base + b_d, base + b_r, c->s_digests,
                                   c->s_offs))
            return e;
        MH_HIP(hipMemcpyAsync(roots, base + b_r, ntrees * 32, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

// ------------------------------------------------------------------ a13
extern "C" int mh_verify_linear_proof_batch(mh_ctx *c, uint64_t n, const uint64_t *proof_src,
                                            const uint64_t *proof_tgt, const uint64_t *term_off,
                                            const uint8_t *terms, const uint64_t *src,
                                            const uint64_t *tgt, const uint8_t *src_alh,
                                            const uint8_t *tgt_alh, uint8_t *ok) {
    return mh_guard([&]() -> int {
        if (!c || (n && (!proof_src || !proof_tgt || !term_off || !src || !tgt || !src_alh ||
                         !tgt_alh || !ok)))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!n) return MH_OK;
        if (!monotonic(term_off, n)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t nterms = term_off[n] - term_off[0];
        if (nterms && !terms) return MH_ERR_ILLEGAL_ARGUMENTS;
        std::lock_guard<std::mutex> lk(c->mu);
        hipSetDevice(c->device);
        hipStream_t st = c->stream;
        std::vector<uint64_t> to(n + 1);
        for (uint64_t p = 0; p <= n; p++) to[p] = term_off[p] - term_off[0];
        Layout L;
        const uint64_t b_ps = L.add(n * 8), b_pt = L.add(n * 8), b_s = L.add(n * 8),
                       b_t = L.add(n * 8), b_off = L.add((n + 1) * 8), b_terms = L.add(nterms * 32),
                       b_sa = L.add(n * 32), b_ta = L.add(n * 32), b_ok = L.add(n);
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        MH_HIP(hipMemcpyAsync(base + b_ps, proof_src, n * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_pt, proof_tgt, n * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_s, src, n * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_t, tgt, n * 8, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_off, to.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (nterms)
            MH_HIP(hipMemcpyAsync(base + b_terms, terms + term_off[0] * 32, nterms * 32,
                                  hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_sa, src_alh, n * 32, hipMemcpyHostToDevice, st));
        MH_HIP(hipMemcpyAsync(base + b_ta, tgt_alh, n * 32, hipMemcpyHostToDevice, st));
        MH_HIP(launch_linear_verify(st, c->tm(), n, (const uint64_t *)(base + b_ps),
                                    (const uint64_t *)(base + b_pt), (const uint64_t *)(base + b_s),
                                    (const uint64_t *)(base + b_t), (const uint64_t *)(base + b_off),
                                    base + b_terms, base + b_sa, base + b_ta, base + b_ok));
        MH_HIP(hipMemcpyAsync(ok, base + b_ok, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}

// ---- VerifyDualProofV2: the one verifier behind the array and wire calls
namespace {

// dual_proof_v2_core's scratch: the operands k_dpv2_prep writes, the Alh
// kernel's message area and every check's result
struct Dpv2Scratch {
    uint64_t hh, s, x, ast, sbl, tbl, leaf, ca, ii, ij, ci, sel, oki, okc, total;
    explicit Dpv2Scratch(uint64_t n) {
        Layout L;
        hh = L.add(2 * n * sizeof(mh_tx_header)), s = L.add(2 * n * kTxInnerStride);
        x = L.add(2 * n * 32), ast = L.add(2 * n * 4);
        sbl = L.add(n * 32), tbl = L.add(n * 32), leaf = L.add(n * 32), ca = L.add(n * 32);
        ii = L.add(n * 8), ij = L.add(n * 8), ci = L.add(n * 8);
        sel = L.add(n), oki = L.add(n), okc = L.add(n);
        total = L.total;
    }
};

}  // namespace

uint64_t dual_proof_v2_scratch_bytes(uint64_t n) { return Dpv2Scratch(n).total; }

int dual_proof_v2_core(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *src_hdr,
                       const mh_tx_header *tgt_hdr, const uint8_t *md_blob,
                       const uint64_t *incl_off, const uint8_t *incl_terms,
                       const uint64_t *cons_off, const uint8_t *cons_terms, const uint64_t *src,
                       const uint64_t *tgt, const uint8_t *src_alh, const uint8_t *tgt_alh,
                       const int32_t *status_in, uint64_t md_blob_len, Dp1V0Metadata v0_md,
                       uint8_t *scratch, int32_t *status_out) {
    const Dpv2Scratch S(n);
    auto U = [&](uint64_t off) { return (uint64_t *)(scratch + off); };
    mh_tx_header *hh = (mh_tx_header *)(scratch + S.hh);
    int32_t *ast = (int32_t *)(scratch + S.ast);
    uint8_t *x = scratch + S.x, *sel = scratch + S.sel, *sbl = scratch + S.sbl,
            *tbl = scratch + S.tbl, *oki = scratch + S.oki, *okc = scratch + S.okc;
    // argument checks (:305-316, and the header rules) and every operand
    MH_HIP(launch_dpv2_prep(st, tm, n, src_hdr, tgt_hdr, md_blob != nullptr, src, tgt, src_alh,
                            tgt_alh, status_in, md_blob_len, v0_md, hh, x, U(S.ii), U(S.ij),
                            U(S.ci), sel, sbl, tbl, status_out));
    // Alh of both headers vs the given ones (:318-326)
    MH_HIP(launch_tx_alh(st, tm, 2 * n, hh, md_blob, nullptr, scratch + S.s, x, nullptr, nullptr,
                         nullptr, ast));
    // inclusion and consistency (:342-370), then the verdict
    MH_HIP(launch_dpv2_proofs(st, tm, n, U(S.ii), U(S.ij), U(S.ci), sel, sbl, tbl, x, incl_off,
                              incl_terms, cons_off, cons_terms, scratch + S.leaf, scratch + S.ca,
                              oki, okc));
    MH_HIP(launch_dpv2_verdict(st, tm, n, hh, src, tgt, ast, oki, okc, status_out));
    return MH_OK;
}

bool dual_proof_v2_args_ok(uint64_t n, const mh_tx_header *src_hdr, const mh_tx_header *tgt_hdr,
                           const uint64_t *incl_off, const uint8_t *incl_terms,
                           const uint64_t *cons_off, const uint8_t *cons_terms, const uint64_t *src,
                           const uint64_t *tgt, const uint8_t *src_alh, const uint8_t *tgt_alh,
                           const int32_t *status) {
    if (!src_hdr || !tgt_hdr || !incl_off || !cons_off || !src || !tgt || !src_alh || !tgt_alh ||
        !status)
        return false;
    if (!monotonic(incl_off, n) || !monotonic(cons_off, n)) return false;
    return (incl_off[n] == incl_off[0] || incl_terms) && (cons_off[n] == cons_off[0] || cons_terms);
}

// The caller's per-proof arrays are packed whole into one pinned staging area
// laid out like their device copies and go up in ONE copy; the offsets keep
// their base and the term pointers are biased.  The statuses come back there.
extern "C" int mh_verify_dual_proof_v2_batch(mh_ctx *c, uint64_t n, const mh_tx_header *sh,
                                             const mh_tx_header *th, const uint8_t *md_blob,
                                             uint64_t md_blob_len, const uint64_t *incl_off,
                                             const uint8_t *incl_terms, const uint64_t *cons_off,
                                             const uint8_t *cons_terms, const uint64_t *src,
                                             const uint64_t *tgt, const uint8_t *src_alh,
                                             const uint8_t *tgt_alh, int32_t *status) {
    return mh_guard([&]() -> int {
        if (!c) return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!n) return MH_OK;
        if (!dual_proof_v2_args_ok(n, sh, th, incl_off, incl_terms, cons_off, cons_terms, src, tgt,
                                   src_alh, tgt_alh, status))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t ni = incl_off[n] - incl_off[0], nc = cons_off[n] - cons_off[0];
        const uint64_t md_bytes = md_blob ? md_blob_len : 0, hb = n * sizeof(mh_tx_header);
        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        // the packed arrays first (one contiguous upload), then device-only data
        Layout L;
        const uint64_t b_h = L.add(2 * hb), b_src = L.add(n * 8), b_tgt = L.add(n * 8),
                       b_alh = L.add(2 * n * 32), b_io = L.add((n + 1) * 8),
                       b_co = L.add((n + 1) * 8);
        const uint64_t up_bytes = L.total;
        const uint64_t b_st = L.add(n * 4), b_md = L.add(md_bytes), b_it = L.add(ni * 32),
                       b_ct = L.add(nc * 32), b_core = L.add(dual_proof_v2_scratch_bytes(n));
        MH_HIP(c->p_stage.ensure(b_st + n * 4));
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *hp = c->p_stage.as<uint8_t>(), *base = c->s_tx.as<uint8_t>();
        memcpy(hp + b_h, sh, hb);
        memcpy(hp + b_h + hb, th, hb);
        memcpy(hp + b_src, src, n * 8);
        memcpy(hp + b_tgt, tgt, n * 8);
        memcpy(hp + b_alh, src_alh, n * 32);
        memcpy(hp + b_alh + n * 32, tgt_alh, n * 32);
        memcpy(hp + b_io, incl_off, (n + 1) * 8);
        memcpy(hp + b_co, cons_off, (n + 1) * 8);
        MH_HIP(hipMemcpyAsync(base, hp, up_bytes, hipMemcpyHostToDevice, st));
        if (ni) MH_HIP(hipMemcpyAsync(base + b_it, incl_terms + incl_off[0] * 32, ni * 32,
                                      hipMemcpyHostToDevice, st));
        if (nc) MH_HIP(hipMemcpyAsync(base + b_ct, cons_terms + cons_off[0] * 32, nc * 32,
                                      hipMemcpyHostToDevice, st));
        if (md_bytes)
            MH_HIP(hipMemcpyAsync(base + b_md, md_blob, md_bytes, hipMemcpyHostToDevice, st));
        // check_header's rule: a v0 header with metadata fails the proof
        const mh_tx_header *dh = (const mh_tx_header *)(base + b_h);
        if (int e = dual_proof_v2_core(
                st, c->tm(), n, dh, dh + n, md_blob ? base + b_md : nullptr,
                (const uint64_t *)(base + b_io), base + b_it - incl_off[0] * 32,
                (const uint64_t *)(base + b_co), base + b_ct - cons_off[0] * 32,
                (const uint64_t *)(base + b_src), (const uint64_t *)(base + b_tgt), base + b_alh,
                base + b_alh + n * 32, nullptr, md_bytes, kDp1V0MetadataRefused, base + b_core,
                (int32_t *)(base + b_st)))
            return e;
        MH_HIP(hipMemcpyAsync(hp + b_st, base + b_st, n * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        memcpy(status, hp + b_st, n * 4);
        return MH_OK;
    });
}

// ---- VerifyDualProof (v1): the one verifier behind the array and wire calls
namespace {

// dual_proof_v1_core's scratch: the operands k_dp1_prep writes, the Alh
// kernel's message area and every check's result
struct Dp1Scratch {
    uint64_t hh, s, x, ast, sbl, tbl, lsa, end, lfa, lft, ii, ij, ci, ls, a_start, a_cnt, alive,
        a_state, oki, okc, okl, oklin, aok, qsrc, qleaf, qi, qj, qroot, qok, total;
    Dp1Scratch(uint64_t n, uint64_t Q) {
        Layout L;
        hh = L.add(2 * n * sizeof(mh_tx_header)), s = L.add(2 * n * kTxInnerStride);
        x = L.add(2 * n * 32), ast = L.add(2 * n * 4);
        sbl = L.add(n * 32), tbl = L.add(n * 32), lsa = L.add(n * 32), end = L.add(n * 32);
        lfa = L.add(n * 32), lft = L.add(n * 32);
        ii = L.add(n * 8), ij = L.add(n * 8), ci = L.add(n * 8), ls = L.add(n * 8);
        a_start = L.add(n * 8), a_cnt = L.add(n * 8), alive = L.add(n), a_state = L.add(n);
        oki = L.add(n), okc = L.add(n), okl = L.add(n), oklin = L.add(n), aok = L.add(n);
        qsrc = L.add(Q * 32), qleaf = L.add(Q * 32), qi = L.add(Q * 8), qj = L.add(Q * 8);
        qroot = L.add(Q * 32), qok = L.add(Q);
        total = L.total;
    }
};

}  // namespace

uint64_t dual_proof_v1_scratch_bytes(uint64_t nk, uint64_t Q) { return Dp1Scratch(nk, Q).total; }

int dual_proof_v1_core(hipStream_t st, Timer *tm, uint64_t nk, const Dual1Arrays &o,
                       const uint64_t *src, const uint64_t *tgt, const uint8_t *src_alh,
                       const uint8_t *tgt_alh, const int32_t *status, uint64_t md_blob_len,
                       Dp1V0Metadata v0_md, uint64_t Q, uint8_t *scratch, uint8_t *ok) {
    const Dp1Scratch S(nk, Q);
    auto U = [&](uint64_t off) { return (uint64_t *)(scratch + off); };
    Dp1Ops w;
    w.hh = (mh_tx_header *)(scratch + S.hh);
    w.x = scratch + S.x;
    w.sbl = scratch + S.sbl;
    w.tbl = scratch + S.tbl;
    w.lin_sa = scratch + S.lsa;
    w.end_alh = scratch + S.end;
    w.ii = U(S.ii);
    w.ij = U(S.ij);
    w.ci = U(S.ci);
    w.ls = U(S.ls);
    w.a_start = U(S.a_start);
    w.a_cnt = U(S.a_cnt);
    w.alive = scratch + S.alive;
    w.a_state = scratch + S.a_state;
    int32_t *ast = (int32_t *)(scratch + S.ast);
    uint8_t *lfa = scratch + S.lfa, *lft = scratch + S.lft, *oki = scratch + S.oki,
            *okc = scratch + S.okc, *okl = scratch + S.okl, *oklin = scratch + S.oklin,
            *aok = scratch + S.aok, *qsrc = scratch + S.qsrc, *qleaf = scratch + S.qleaf,
            *qroot = scratch + S.qroot, *qok = scratch + S.qok;
    // argument checks (:128-138, and the header rules) and every operand
    MH_HIP(launch_dp1_prep(st, tm, nk, o, src, tgt, src_alh, tgt_alh, status, md_blob_len, v0_md, w));
    // header Alh (:140-148)
    MH_HIP(launch_tx_alh(st, tm, 2 * nk, w.hh, o.md_blob, nullptr, scratch + S.s, w.x, nullptr,
                         nullptr, nullptr, ast));
    // inclusion / consistency / last inclusion (:150-189)
    MH_HIP(launch_leaf_for(st, tm, nk, w.x, lfa));
    MH_HIP(launch_leaf_for(st, tm, nk, o.tbl_alh, lft));
    MH_HIP(launch_ahtree_verify(st, tm, MH_AHT_INCLUSION, nk, w.ii, w.ij, o.off[kI], o.terms[kI],
                                lfa, w.tbl, oki, nullptr));
    MH_HIP(launch_ahtree_verify(st, tm, MH_AHT_CONSISTENCY, nk, w.ci, w.ij, o.off[kC],
                                o.terms[kC], w.sbl, w.tbl, okc, nullptr));
    MH_HIP(launch_ahtree_verify(st, tm, MH_AHT_LAST_INCLUSION, nk, w.ij, w.ij, o.off[kL],
                                o.terms[kL], lft, w.tbl, okl, nullptr));
    // linear proof (:192 / :213)
    MH_HIP(launch_linear_verify(st, tm, nk, o.lin_src, o.lin_tgt, w.ls, tgt, o.off[kLin],
                                o.terms[kLin], w.lin_sa, tgt_alh, oklin));
    // linear advance proof (:90-121): the chain, then the nested inclusion proofs
    MH_HIP(launch_advance_chain_gated(st, tm, nk, w.a_state, w.a_start, w.a_cnt, o.off[kAdv],
                                      o.terms[kAdv], o.off[kQ], w.end_alh, qsrc, aok));
    MH_HIP(launch_dp1_nested(st, tm, Q, nk, o.off[kQ], w, U(S.qi), U(S.qj), qroot));
    MH_HIP(launch_leaf_for(st, tm, Q, qsrc, qleaf));
    MH_HIP(launch_ahtree_verify(st, tm, MH_AHT_INCLUSION, Q, U(S.qi), U(S.qj), o.qoff, o.qterms,
                                qleaf, qroot, qok, nullptr));
    const Dp1Results r{ast, oki, okc, okl, oklin, aok, qok};
    MH_HIP(launch_dp1_verdict(st, tm, nk, w, r, o.has_lin, o.off[kQ], ok));
    return MH_OK;
}

// The caller's arrays go up as they are, one copy each; the offset arrays
// keep their base (x_off[0] != 0 for a slice of a larger batch) and the term
// pointers are biased instead (Dual1Arrays).
extern "C" int mh_verify_dual_proof_batch(mh_ctx *c, const mh_dual_proof_batch *B, uint8_t *ok) {
    return mh_guard([&]() -> int {
        if (!c || !B || (B->n && !ok)) return MH_ERR_ILLEGAL_ARGUMENTS;
        const uint64_t n = B->n;
        if (!n) return MH_OK;
        if (!B->src_hdr || !B->tgt_hdr || !B->incl_off || !B->cons_off || !B->target_bl_tx_alh ||
            !B->last_off || !B->has_linear || !B->linear_src || !B->linear_tgt || !B->linear_off ||
            !B->has_advance || !B->advance_off || !B->advance_incl_first || !B->advance_incl_off ||
            !B->src || !B->tgt || !B->src_alh || !B->tgt_alh)
            return MH_ERR_ILLEGAL_ARGUMENTS;
        if (!monotonic(B->incl_off, n) || !monotonic(B->cons_off, n) ||
            !monotonic(B->last_off, n) || !monotonic(B->linear_off, n) ||
            !monotonic(B->advance_off, n) || !monotonic(B->advance_incl_first, n))
            return MH_ERR_ILLEGAL_ARGUMENTS;
        // the nested proofs of this batch and their term offsets
        const uint64_t q0 = B->advance_incl_first[0], Q = B->advance_incl_first[n] - q0;
        const uint64_t *nested_off = B->advance_incl_off + q0;
        if (!monotonic(nested_off, Q)) return MH_ERR_ILLEGAL_ARGUMENTS;
        // CSR lists in the order of Dual1Arrays::terms, the nested terms last
        const uint64_t *off[6] = {B->incl_off,   B->cons_off,    B->last_off,
                                  B->linear_off, B->advance_off, nested_off};
        const uint8_t *terms[6] = {B->incl_terms,   B->cons_terms,    B->last_terms,
                                   B->linear_terms, B->advance_terms, B->advance_incl_terms};
        uint64_t cnt[6];  // terms of each list
        for (int j = 0; j < 6; j++) {
            cnt[j] = j < 5 ? off[j][n] - off[j][0] : Q ? off[j][Q] - off[j][0] : 0;
            if (cnt[j] && !terms[j]) return MH_ERR_ILLEGAL_ARGUMENTS;
        }
        const uint64_t md_bytes = B->md_blob ? B->md_blob_len : 0;

        std::lock_guard<std::mutex> lk(c->mu);
        MH_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        Layout L;
        uint64_t b_off[6], b_terms[6];
        for (int j = 0; j < 6; j++) {
            b_off[j] = L.add(((j < 5 ? n : Q) + 1) * 8);
            b_terms[j] = L.add(cnt[j] * 32);
        }
        const uint64_t b_h = L.add(2 * n * sizeof(mh_tx_header)), b_md = L.add(md_bytes),
                       b_tba = L.add(n * 32), b_flags = L.add(2 * n), b_lin = L.add(2 * n * 8),
                       b_first = L.add((n + 1) * 8), b_src = L.add(n * 8), b_tgt = L.add(n * 8),
                       b_alh = L.add(2 * n * 32), b_ok = L.add(n),
                       b_core = L.add(dual_proof_v1_scratch_bytes(n, Q));
        MH_HIP(c->s_tx.ensure(L.total));
        uint8_t *base = c->s_tx.as<uint8_t>();
        auto h2d = [&](uint64_t at, const void *p, uint64_t bytes) -> hipError_t {
            return bytes ? hipMemcpyAsync(base + at, p, bytes, hipMemcpyHostToDevice, st)
                         : hipSuccess;
        };
        uint8_t *d_terms[6];  // biased: list j's term t is at d_terms[j] + 32 * t
        for (int j = 0; j < 6; j++) {
            const uint64_t entries = j < 5 ? n + 1 : Q ? Q + 1 : 0, t0 = entries ? off[j][0] : 0;
            MH_HIP(h2d(b_off[j], off[j], entries * 8));
            MH_HIP(h2d(b_terms[j], cnt[j] ? terms[j] + t0 * 32 : nullptr, cnt[j] * 32));
            d_terms[j] = base + b_terms[j] - t0 * 32;
        }
        Dual1Arrays o{};
        for (int j = 0; j < 5; j++) {
            o.off[j] = (const uint64_t *)(base + b_off[j]);
            o.terms[j] = d_terms[j];
        }
        o.off[kQ] = (const uint64_t *)(base + b_first);
        o.qoff = (uint64_t *)(base + b_off[5]);
        o.qterms = d_terms[5];
        o.src_hdr = (mh_tx_header *)(base + b_h);
        o.tgt_hdr = o.src_hdr + n;
        o.md_blob = B->md_blob ? base + b_md : nullptr;
        o.tbl_alh = base + b_tba;
        o.has_lin = base + b_flags;
        o.has_adv = base + b_flags + n;
        o.lin_src = (uint64_t *)(base + b_lin);
        o.lin_tgt = o.lin_src + n;
        MH_HIP(h2d(b_h, B->src_hdr, n * sizeof(mh_tx_header)));
        MH_HIP(h2d(b_h + n * sizeof(mh_tx_header), B->tgt_hdr, n * sizeof(mh_tx_header)));
        MH_HIP(h2d(b_md, B->md_blob, md_bytes));
        MH_HIP(h2d(b_tba, B->target_bl_tx_alh, n * 32));
        MH_HIP(h2d(b_flags, B->has_linear, n));
        MH_HIP(h2d(b_flags + n, B->has_advance, n));
        MH_HIP(h2d(b_lin, B->linear_src, n * 8));
        MH_HIP(h2d(b_lin + n * 8, B->linear_tgt, n * 8));
        MH_HIP(h2d(b_first, B->advance_incl_first, (n + 1) * 8));
        MH_HIP(h2d(b_src, B->src, n * 8));
        MH_HIP(h2d(b_tgt, B->tgt, n * 8));
        MH_HIP(h2d(b_alh, B->src_alh, n * 32));
        MH_HIP(h2d(b_alh + n * 32, B->tgt_alh, n * 32));
        if (int e = dual_proof_v1_core(st, c->tm(), n, o, (const uint64_t *)(base + b_src),
                                       (const uint64_t *)(base + b_tgt), base + b_alh,
                                       base + b_alh + n * 32, nullptr, md_bytes,
                                       kDp1V0MetadataRefused, Q, base + b_core, base + b_ok))
            return e;
        MH_HIP(hipMemcpyAsync(ok, base + b_ok, n, hipMemcpyDeviceToHost, st));
        MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    });
}
