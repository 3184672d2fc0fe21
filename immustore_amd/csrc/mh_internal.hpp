// mh_internal.hpp -- shared declarations between the kernel translation units
// and the C-ABI implementation (capi.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/immustore_merkle.h"

namespace mh {

// S(x) = sum_{i<x} popcount(i): process the set bits of x from the top; the
// j-th set bit b (j = 1 for the highest) contributes b*2^(b-1) + (j-1)*2^b.
__host__ __device__ inline uint64_t popsum_below(uint64_t x) {
    uint64_t s = 0, j = 0;
    while (x) {
        const int b = 63 - __builtin_clzll(x);
        s += (b ? ((uint64_t)b << (b - 1)) : 0) + (j << b);
        j++;
        x &= ~(1ull << b);
    }
    return s;
}

// nodesUpto(n) = n + S(n)           (ahtree.go:492-511)
// nodesUntil(n) = nodesUpto(n - 1)  (ahtree.go:485-490)
__host__ __device__ inline uint64_t until_from_s(uint64_t n, uint64_t s_n) {
    return (n - 1) + s_n - (uint64_t)__builtin_popcountll(n - 1);
}

// nodesUpto(n) for device code (proof_kernels.hip)
__host__ __device__ inline uint64_t ahtree_nodes_upto_dev(uint64_t n) { return n + popsum_below(n); }


constexpr int kMaxLevels = 66;

// Level-major flat layout of an htree of width n (embedded/htree/htree.go:
// levels[l] holds ceil(n/2^l) used nodes; promoted odd nodes are copied up).
struct LevelGeom {
    uint64_t n = 0;
    int nlevels = 0;                // number of levels incl. root level
    uint64_t off[kMaxLevels] = {};  // offset (in 32-byte nodes) of level l
    uint64_t width[kMaxLevels] = {};
    uint64_t total = 0;             // total nodes
    void init(uint64_t n_);
};

// Kernel arguments passed by value (fits in the 4 KB kernarg segment).
struct LevelArgs {
    uint64_t off[kMaxLevels];
    uint64_t width[kMaxLevels];
};

struct KWTable {
    uint32_t kw[64];
};

// Compute K[t]+W[t] of the padding block of a message of `len` bytes whose
// length is a multiple of 64 (constant schedule: 0x80, zeros, bit length).
void pad_block_kw(uint64_t len, KWTable *out);

// ---------------------------------------------------------------- launchers
// All return hipError_t (hipSuccess == 0) and enqueue on `st`.
// Per-kernel timing hook (ctx-level); may be null.
struct Timer {
    virtual void begin(const char *name, hipStream_t st) = 0;
    virtual void end(hipStream_t st) = 0;
    virtual ~Timer() {}
};

struct TimerScope {
    Timer *tm;
    hipStream_t st;
    TimerScope(Timer *t, const char *name, hipStream_t s) : tm(t), st(s) {
        if (tm) tm->begin(name, st);
    }
    ~TimerScope() {
        if (tm) tm->end(st);
    }
};

hipError_t launch_entries_fixed(hipStream_t st, Timer *tm, int version, uint64_t n,
                                const uint8_t *keys, uint32_t key_len, const uint8_t *vals,
                                uint32_t val_len, uint8_t *hvals_out, uint8_t *levels,
                                const LevelGeom &g, int *lanes_levels_done);
bool entries_fixed_supported(int version, const uint8_t *keys, uint32_t key_len,
                             const uint8_t *vals, uint32_t val_len);

// SHA-256 of n ragged byte ranges buf[off[i] .. off[i+1]) (varlen_kernels.hip);
// override32[i] replaces message i where use_override[i] != 0.  scratch
// (sha_varlen_scratch_bytes(n), device, stream-ordered on st) lets the
// messages be bucketed by block count first; null hashes them in input order.
size_t sha_varlen_scratch_bytes(uint64_t n);
hipError_t launch_sha256_csr(hipStream_t st, Timer *tm, const uint8_t *buf, const uint64_t *off,
                             uint64_t n, const uint8_t *override32, const uint8_t *use_override,
                             uint8_t *out32, uint8_t *scratch);
// The bucketing alone, for a kernel of another file that walks messages of
// lengths len[i] (skip[i] != 0: no block, sorted last): the order in scratch,
// or null when the batch is too small to profit (input order).
const uint32_t *sha_varlen_order(hipStream_t st, Timer *tm, const uint64_t *len, const uint8_t *skip,
                                 uint64_t n, uint8_t *scratch, hipError_t *err);
// readValueAt's integrity check (immustore.go:3235) over a batch: status[i] =
// MH_OK iff off[i+1] - off[i] == exp_len[i] (exp_len may be null) and
// SHA256(buf[off[i] .. off[i+1])) == expect[i], else MH_ERR_CORRUPTED_DATA.
hipError_t launch_verify_values(hipStream_t st, Timer *tm, const uint8_t *buf, const uint64_t *off,
                                uint64_t n, const uint64_t *exp_len, const uint8_t *expect,
                                int32_t *status, uint8_t *scratch);
// Fused ragged entries (varlen_kernels.hip): hVal (or override) -> hvals_out
// (may be null), entry digest (tx.go:690-731) -> out32, or its htree leaf when
// leaf is set (level 0 of the tree).  scratch as for launch_sha256_csr.
// ver_e (device, n bytes, may be null): per-entry digest version instead of
// `version` (a v0 entry's metadata is then not hashed).  override32 with a
// null use_override overrides every entry (val_off / vals may be null).
hipError_t launch_entries_varlen(hipStream_t st, Timer *tm, int version, uint64_t n,
                                 const uint8_t *keys, const uint64_t *key_off, const uint8_t *md,
                                 const uint64_t *md_off, const uint8_t *vals,
                                 const uint64_t *val_off, const uint8_t *override32,
                                 const uint8_t *use_override, uint8_t *hvals_out, uint8_t *out32,
                                 bool leaf, uint8_t *scratch, const uint8_t *ver_e = nullptr);
// Leaves from digests (htree.go:79-83) + in-lane levels up to log2(LPL).
hipError_t launch_leaves_from_digests(hipStream_t st, Timer *tm, const uint8_t *digests,
                                      uint64_t n, uint8_t *levels, const LevelGeom &g,
                                      int *levels_done);
// Copy nodes into level 0 (no leaf hashing): used for reducing subtree roots.
// Reduce levels [from, top] in place (htree.go:85-110).
hipError_t launch_reduce(hipStream_t st, Timer *tm, uint8_t *levels, const LevelGeom &g,
                         int from_level, uint8_t *root = nullptr);

// Generic helpers
hipError_t launch_fill_random(hipStream_t st, uint8_t *dst, uint64_t nbytes, uint64_t seed);
hipError_t launch_fill_keys_be64(hipStream_t st, uint8_t *dst, uint64_t n, uint64_t first);
hipError_t launch_iota_offsets(hipStream_t st, uint64_t *off, uint64_t n, uint64_t stride);
hipError_t launch_gather_nodes(hipStream_t st, const uint8_t *src, const uint64_t *idx, uint64_t n,
                               uint8_t *dst);

// ---- verification (embedded/htree/htree.go:166-195, ahtree/verification.go)
hipError_t launch_htree_verify(hipStream_t st, Timer *tm, uint64_t np, const uint64_t *leaf,
                               const uint64_t *width, const uint64_t *term_off,
                               const uint8_t *terms, const uint8_t *digests, const uint8_t *roots,
                               uint8_t *ok);
hipError_t launch_ahtree_verify(hipStream_t st, Timer *tm, int kind, uint64_t np,
                                const uint64_t *i, const uint64_t *j, const uint64_t *term_off,
                                const uint8_t *terms, const uint8_t *a, const uint8_t *b,
                                uint8_t *ok, uint8_t *eval_out);

// ---- ahtree batch append (embedded/ahtree/ahtree.go:246-373)
// work_ctr: 4 bytes of device memory private to this launch's stream order
// (the spine kernel's work queue; reset on `st` before the launch).
// Optional appendable record streams of the appended payloads (SURVEY.md
// 8(f) row 4): pLog records BE32 len || payload at plog + i*(4+plen), cLog
// entries BE64 (p_off0 + i*(4+plen)) || BE32 len at clog + i*12.
struct AhtLogs {
    uint8_t *plog = nullptr;
    uint8_t *clog = nullptr;
    uint64_t p_off0 = 0;
};
// The left edge of an append range (n0, ...] whose dLog buffer does not hold
// the nodes before it: every node such a range reads that ends at or before
// lo is a peak of lo (node(lo with the bits below l cleared, l) for a set bit
// l of lo, ahtree.go:296-322), so the 64-slot frontier fr[l] (device, 32 B
// per level, only set bits of lo meaningful) replaces the old dLog.  lo = 0:
// no edge, every node from the dLog.
struct AhtEdge {
    const uint8_t *fr = nullptr;
    uint64_t lo = 0;
};
hipError_t launch_ahtree_append(hipStream_t st, Timer *tm, uint8_t *dlog, uint64_t n0,
                                const uint8_t *payloads, uint64_t m, uint32_t plen,
                                uint8_t *roots_out, uint32_t *work_ctr,
                                const AhtLogs &lg = AhtLogs(), const AhtEdge &edge = AhtEdge());
// The three phases of launch_ahtree_append, for sharded appends.
// dlog == nullptr: records only.
hipError_t launch_ahtree_leaves(hipStream_t st, Timer *tm, uint8_t *dlog, uint64_t n0,
                                const uint8_t *payloads, uint64_t m, uint32_t plen,
                                const AhtLogs &lg = AhtLogs());
hipError_t launch_ahtree_perfect(hipStream_t st, Timer *tm, uint8_t *dlog, uint64_t n0,
                                 uint64_t n_end, int lmin, int lmax,
                                 const AhtEdge &edge = AhtEdge());
hipError_t launch_ahtree_spine(hipStream_t st, Timer *tm, uint8_t *dlog, uint64_t n0, uint64_t m,
                               uint8_t *roots_out, uint32_t *work_ctr,
                               const AhtEdge &edge = AhtEdge());
hipError_t launch_ahtree_put_shard_roots(hipStream_t st, Timer *tm, uint8_t *dlog, int level,
                                         uint64_t count, const uint8_t *roots);

// Ranged multi-device append (capi_multi.hip): the batch (n0, n0 + total] is
// cut at multiples of S = 2^k into G <= 64 device ranges (b[d], b[d+1]]; a
// device keeps only its own dLog range.  Pieces are the aligned blocks of S
// appends; piece E ends at E*S and its level-k root is node(E*S, k).
constexpr int kAhtMaxRanges = 64;
struct AhtTopArgs {
    int k = 0;                           // shard bits: S = 2^k
    int nlev = 0;                        // levels of the piece tree (l' = 0 .. nlev-1)
    int G = 0;                           // device ranges
    uint64_t n0 = 0;                     // old size
    uint64_t lo = 0, hi = 0;             // this device's range (lo, hi]
    uint64_t N0 = 0, Pend = 0, Pmax = 0; // floor(n0/S), floor((n0+total)/S), pieces per send slot
    uint64_t lev_off[64] = {};           // slot offset of piece level l' in the top buffer
    uint64_t pe0[kAhtMaxRanges + 1] = {};  // floor(b[d]/S), d = 0..G
};
// the level-k roots of this device's pieces E in (pe0[d], pe0[d+1]] into send
hipError_t launch_ahtree_gather_pieces(hipStream_t st, const uint8_t *dlog, int k, uint64_t e0,
                                       uint64_t count, uint8_t *send);
// piece tree over the all-gathered piece roots and the old peaks of n0 (levels
// >= k), the nodes above level k that end in (lo, hi] into dlog, and this
// device's frontier (peaks of lo) into fr (lo > n0 only)
hipError_t launch_ahtree_top(hipStream_t st, const AhtTopArgs &a, const uint8_t *recv,
                             const uint8_t *peaks_n0, uint8_t *top, uint8_t *dlog, uint8_t *fr);
// the 64-slot frontier (32 B per level) by value, written to dst on st
struct AhtSlots {
    uint8_t b[64 * 32];
};
hipError_t launch_ahtree_put_slots(hipStream_t st, const AhtSlots &s, uint8_t *dst);
// the peaks of n from a device dLog into the 64-slot frontier layout
hipError_t launch_ahtree_peaks(hipStream_t st, const uint8_t *dlog, uint64_t n, uint8_t *fr);

// host-side index math shared with the C API
uint64_t ahtree_nodes_upto(uint64_t n);
uint64_t ahtree_nodes_until(uint64_t n);


// ---------------------------------------------------------------- tx layer
typedef mh_tx_header MhTxHeader;
constexpr uint64_t kTxInnerStride = 384;  // >= 8+2+2+268+4+32+8+32 (tx.go:249-302)

hipError_t launch_tx_alh(hipStream_t st, Timer *tm, uint64_t n, const MhTxHeader *hdrs,
                         const uint8_t *md_blob, const uint8_t *eh_src, uint8_t *scratch,
                         const uint8_t *expect, const uint64_t *expect_off, uint8_t *inner_out,
                         uint8_t *alh_out, int32_t *status);
hipError_t launch_leaf_for(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *in, uint8_t *out);
hipError_t launch_select32(hipStream_t st, uint64_t n, const uint8_t *sel, const uint8_t *x,
                           const uint8_t *y, uint8_t *out);
hipError_t launch_linear_verify(hipStream_t st, Timer *tm, uint64_t n, const uint64_t *psrc,
                                const uint64_t *ptgt, const uint64_t *src, const uint64_t *tgt,
                                const uint64_t *term_off, const uint8_t *terms,
                                const uint8_t *src_alh, const uint8_t *tgt_alh, uint8_t *ok);
// the VerifyLinearAdvanceProof chain over every proof of a batch: lane p runs
// only when state[p] == 0 (its lengths checked by whoever set the state) and
// otherwise reads no term and writes ok[p] = 0.  first: the proofs' nested
// offsets (n + 1); leaves_src is indexed from first[0]
hipError_t launch_advance_chain_gated(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *state,
                                      const uint64_t *start, const uint64_t *cnt,
                                      const uint64_t *term_off, const uint8_t *terms,
                                      const uint64_t *first, const uint8_t *end_alh,
                                      uint8_t *leaves_src, uint8_t *ok);

// ---- VerifyDualProof (v1, verification.go:127-235) over device arrays
// Per-proof counts of a DualProof (v1) and the CSR offset arrays scanned from
// them: the five term lists, the nested InclusionProofs of the advance proof
// and their terms, the canonical metadata bytes.
enum : int { kI = 0, kC, kL, kLin, kAdv, kQ, kQT, kMd, kCounts };
// A decoder's metadata blob: header p's canonical bytes start at p * kMdSlot.
constexpr uint32_t kMdSlot = MH_MAX_TX_METADATA_LEN;

// A batch of decoded DualProofs on the device, in the layout of
// mh_dual_proof_batch: what the decoder's write pass (pb_decode.hip) fills and
// what dual_proof_v1_core (capi_tx.hip) verifies.  off[j] has n + 1 entries
// and need not start at 0: terms[j] + 32 * off[j][p] is proof p's first term,
// so a caller whose offsets start at off[j][0] passes terms[j] biased by
// -32 * off[j][0].  off[kQ] are the proofs' first nested proofs
// (advance_incl_first); qoff holds off[kQ][n] - off[kQ][0] + 1 term offsets,
// entry 0 for nested proof off[kQ][0], into qterms (biased like terms[]).
// off[kQT] and off[kMd] are the decoder's own (null for any other caller).
struct Dual1Arrays {
    const uint64_t *off[kCounts];
    uint8_t *terms[5];  // incl, cons, last, linear, advance
    uint8_t *qterms;
    uint64_t *qoff;
    mh_tx_header *src_hdr, *tgt_hdr;
    uint8_t *md_blob;  // null: no blob, every header with metadata is refused
    uint8_t *tbl_alh, *has_lin, *has_adv;
    uint64_t *lin_src, *lin_tgt;
};

// The one intended difference between the callers of a dual-proof verifier
// (v1 and V2 alike): what a v0 header that carries metadata means.  Go's
// innerHash never reads a v0 header's metadata (tx.go:258-263), so for headers
// decoded from the wire it is dropped and the proof goes on; the array calls
// keep check_header's rule (MH_ERR_METADATA_UNSUPPORTED) and the proof fails.
enum Dp1V0Metadata : int { kDp1V0MetadataDropped = 0, kDp1V0MetadataRefused = 1 };

struct Dp1Ops {        // per-proof operands of one batch (n entries unless noted)
    mh_tx_header *hh;  // 2 n: the headers the Alh kernel hashes, sources then targets
    uint8_t *x;        // 2 n x 32: the caller's Alh values in the same order
    uint8_t *sbl, *tbl, *lin_sa, *end_alh;  // x 32
    uint64_t *ii, *ij, *ci, *ls, *a_start, *a_cnt;
    uint8_t *alive, *a_state;  // a_state: 0 run the chain, 1 true, 2 false
};
// argument checks + operands (k_dp1_prep); status may be null (every proof decoded)
hipError_t launch_dp1_prep(hipStream_t st, Timer *tm, uint64_t n, const Dual1Arrays &o,
                           const uint64_t *src, const uint64_t *tgt, const uint8_t *src_alh,
                           const uint8_t *tgt_alh, const int32_t *status, uint64_t md_blob_len,
                           Dp1V0Metadata v0_md, const Dp1Ops &w);
// operands of the nq nested inclusion proofs, indexed from first[0]
hipError_t launch_dp1_nested(hipStream_t st, Timer *tm, uint64_t nq, uint64_t n,
                             const uint64_t *first, const Dp1Ops &w, uint64_t *qi, uint64_t *qj,
                             uint8_t *qroot);
struct Dp1Results {  // per-check results: n each, qok per nested proof from first[0]
    const int32_t *ast;  // 2 n
    const uint8_t *oki, *okc, *okl, *oklin, *aok, *qok;
};
hipError_t launch_dp1_verdict(hipStream_t st, Timer *tm, uint64_t n, const Dp1Ops &w,
                              const Dp1Results &r, const uint8_t *has_lin, const uint64_t *first,
                              uint8_t *ok);

// ---- whole VerifiableGet answers (client.go:1119-1234) over device arrays
// What the envelope pass (k_pbd_ventry, pb_decode.hip) leaves per message of
// a group of nk: the size pass fills cnt (the inclusion terms, then the bytes
// of a DualProof that has to be concatenated: cat_all ? every DualProof : one
// that occurs more than once), the write pass info, the terms at term_off,
// the concatenations at cat + cat_off, and the DualProof range of every
// message as [dual_beg, dual_end) relative to the msgs pointer -- in place, or
// inside cat, which must therefore lie in the allocation msgs points into.
struct VentryArrays {
    mh_verifiable_entry_info *info;
    uint64_t *cnt;                        // 2 x nk
    const uint64_t *term_off, *cat_off;   // nk + 1 each
    uint8_t *terms, *cat;
    uint64_t *dual_beg, *dual_end;        // nk each
    int cat_all;
};
// The hashing of verifiedGet, one answer per lane (k_ventry_verify,
// ventry_kernels.hip): value hash, EntrySpecDigest, htree.VerifyInclusion
// against the Eh of the decoded header that is the entry's tx, that header's
// Alh; writes the arguments of dual_proof_v1_core.  keys biased like msgs
// (keys + key_off[p] is answer p's key); hdrs: o's headers and metadata after
// the DualProof write pass; alh_msg: nk x kTxInnerStride bytes of scratch.
struct VentryVerify {
    const uint8_t *msgs, *keys;
    const uint64_t *key_off, *at_tx, *state_tx;
    const uint8_t *state_alh;
    const int32_t *status;  // the envelope pass's
    const mh_verifiable_entry_info *info;
    const uint64_t *term_off;
    const uint8_t *terms;
    const mh_tx_header *src_hdr, *tgt_hdr;
    const uint8_t *md_blob;
    uint8_t *alh_msg;
    uint64_t *src, *tgt;         // out: VerifyDualProof's ids
    uint8_t *src_alh, *tgt_alh;  // out: and Alh values, nk x 32 each
    uint8_t *incl_ok;            // out: inclusion holds and the header could be hashed
};
hipError_t launch_ventry_verify(hipStream_t st, Timer *tm, uint64_t nk, const VentryVerify &v);
// ok = status OK && incl_ok && (state_tx == 0 || dual_ok); new_tx / new_alh =
// tgt / tgt_alh where ok, zeros elsewhere
hipError_t launch_ventry_verdict(hipStream_t st, Timer *tm, uint64_t nk, const int32_t *status,
                                 const uint64_t *state_tx, const uint8_t *incl_ok,
                                 const uint8_t *dual_ok, const uint64_t *tgt,
                                 const uint8_t *tgt_alh, uint8_t *ok, uint64_t *new_tx,
                                 uint8_t *new_alh);

// ---- whole VerifiableTx answers (capi_vtx.hip)
// One Tx.entries element i < K of a live write answer, at slot spec_off[p] + i
// (k_pbd_vtx's write pass): DigestFromProto(hValue), where its key lies in the
// messages, and KVMetadataFromProto(metadata).Bytes().
struct VtxRec {
    uint8_t hv[32];
    uint64_t key_pos, key_len;
    uint8_t md_len, md[MH_MAX_KV_METADATA_LEN];
    uint8_t pad_[4];
};
static_assert(sizeof(VtxRec) == 64, "records are 16-byte aligned for load_digest");
// The envelope pass of a group of nk VerifiableTx answers (k_pbd_vtx).  kind /
// spec_off / state_tx: the group's slices of the caller's arrays (spec_off
// absolute, recs[0] is slot spec_base = spec_off[0]).  Size pass: status, live,
// cnt (DualProof bytes to concatenate, as VentryArrays); write pass: hdr (the
// tx header, its canonical metadata at md_blob + p x MH_MAX_TX_METADATA_LEN),
// recs, cat and the DualProof range relative to msgs.
struct VtxArrays {
    const uint8_t *kind;
    const uint64_t *spec_off, *state_tx;
    uint64_t spec_base;
    uint64_t *cnt;
    const uint64_t *cat_off;
    uint8_t *cat;
    uint64_t *dual_beg, *dual_end;
    mh_tx_header *hdr;
    uint8_t *md_blob;
    uint8_t *live;
    VtxRec *recs;
};
// The per-slot hashing (k_vtx_leaf, k_vtx_spec) and the per-answer step
// (k_vtx_answer) between the envelope pass and dual_proof_v1_core
// (ventry_kernels.hip).  Per-answer arrays are the group's slices; key_off /
// val_off are indexed by the absolute slot, keys / vals biased like msgs; recs
// / dig / dok / xok start at the group's first slot.
struct VtxVerify {
    uint64_t nk;
    const uint8_t *msgs, *keys, *vals;
    const uint64_t *spec_off, *key_off, *val_off;
    const uint8_t *kind;
    const uint64_t *at_tx, *state_tx;
    const uint8_t *state_alh;
    const int32_t *status;
    const uint8_t *live;
    const mh_tx_header *hdr;     // tx.header of every answer
    const uint8_t *md_blob;      // and its metadata
    const VtxRec *recs;
    uint8_t *dig;                // d_i, 32 bytes a slot
    uint8_t *dok, *xok;          // a slot: d_i could be built / x_i == d_{j_i}
    const uint8_t *roots;        // Eh' of every answer (after build_many_dev)
    const mh_tx_header *src_hdr, *tgt_hdr;  // the DualProof's, after its write pass
    const uint8_t *dual_md;
    uint8_t *alh_msg;            // nk x kTxInnerStride bytes of scratch
    uint64_t *src, *tgt;         // out: VerifyDualProof's ids
    uint8_t *src_alh, *tgt_alh;  // out: and Alh values
    uint8_t *pre_ok;             // out: everything before VerifyDualProof holds
    uint8_t *eh_out;             // out: Eh' (zeros where it was not reached)
};
hipError_t launch_vtx_leaf(hipStream_t st, Timer *tm, uint64_t T, const VtxVerify &v);
hipError_t launch_vtx_spec(hipStream_t st, Timer *tm, uint64_t T, const VtxVerify &v);
hipError_t launch_vtx_answer(hipStream_t st, Timer *tm, const VtxVerify &v);

// ---- exported txs replicated onto a follower's tree (capi_repl.hip,
// repl_kernels.hip).  One group of nk txs: tx p is msgs[tx_off[p] ..
// tx_off[p + 1]) (msgs biased like the callers' offsets); per-tx arrays are
// the group's slices, per-entry arrays start at the group's first entry.
struct ReplLimits {
    uint32_t max_entries, max_key_len, max_value_len, flags;
};
struct ReplGroup {
    uint64_t nk, first;         // txs of the group, the batch index of its first
    const uint8_t *msgs;
    const uint64_t *tx_off;     // nk + 1
    int32_t *status;            // the envelope-through-Eh verdict
    uint64_t *cnt;              // size pass: entries of a tx that parsed, else 0
    const uint64_t *ent_off;    // nk + 1, scanned from cnt
    mh_tx_header *hdr;          // write pass; md_off = (first + p) x kMdSlot
    uint8_t *md_blob;           // the whole batch's (canonical TxMetadata.Bytes())
    uint8_t *trunc;             // write pass: the trailer says truncated
    mh_replicated_entry *ents;  // write pass
    uint8_t *dup;               // an earlier entry of the tx has the same key
    uint8_t *dig, *hv;          // entry digests / hVal, 32 bytes an entry
    const uint8_t *roots;       // built Eh of every tx (after build_many_dev)
    uint8_t *alh;               // Alh of a tx with status MH_OK, else zeros
    uint8_t *alh_msg;           // nk x kTxInnerStride bytes of scratch
};
// the wire grammar: write = false status and cnt, write = true hdr, md_blob,
// trunc, ents of the txs still MH_OK
hipError_t launch_repl_struct(hipStream_t st, Timer *tm, bool write, const ReplGroup &g);
// dup, then OngoingTx.set / validateAgainst / validateEntries per tx (status)
hipError_t launch_repl_set(hipStream_t st, Timer *tm, uint64_t T, const ReplGroup &g,
                           const ReplLimits &lim);
// hVal and entry digest of every entry of a tx still MH_OK
hipError_t launch_repl_leaf(hipStream_t st, Timer *tm, uint64_t T, const ReplGroup &g);
// Eh against the exported one, hdr.eh = the built one, the Alh
hipError_t launch_repl_alh(hipStream_t st, Timer *tm, const ReplGroup &g, const ReplLimits &lim);
// The chain and linking verdicts of all n txs against dlog = the P resident
// leaves + the n candidate Alh leaves: full[k] = local[k], or the id / BlRoot
// / PrevAlh verdict had every earlier tx been accepted; then a = the first k
// with full[k] != MH_OK (n: none) into *first_bad, and every tx behind a gets
// local[k] or MH_ERR_TX_NOT_REACHED.
struct ReplPrev {
    uint8_t alh[32];
};
hipError_t launch_repl_verdict(hipStream_t st, Timer *tm, uint64_t n, const int32_t *local,
                               const mh_tx_header *hdr, const uint8_t *alh, const uint8_t *dlog,
                               uint64_t P, const ReplPrev &prev, int32_t *full,
                               unsigned long long *first_bad);

// ---- ImmuStore.ExportTx for a run of txs (capi_export.hip, export_kernels.hip).
// Every array device memory.  Per tx (n, or n + 1 where noted) and per entry
// of the txs whose record verdict is MH_OK (E).
struct ExpVlog {  // value log k + 1: data[0] is its byte first_off
    const uint8_t *data;
    uint64_t first_off, end_off;
};
enum : uint8_t { kExpAvail = 0, kExpTrunc = 1, kExpNoVlog = 2 };  // an entry's class
constexpr uint32_t kExpNone = 0xffffffffu;  // "no entry" in early_idx / vbad
struct ExpArrays {
    uint64_t n, E;
    const uint8_t *txlog, *clog;  // clog: the entry of the run's first tx
    uint32_t es, nvlogs;
    const ExpVlog *vlogs;
    // per tx: the read path's results, then what the export derives
    const MhTxHeader *hd;
    const int32_t *rst;
    uint64_t *ecnt, *ent_start, *leaf_off /* n + 1 */;
    uint8_t *md;          // n x kMdSlot: TxMetadata.Bytes()
    uint32_t *mdl;        // its length
    uint32_t *early_idx;  // the lowest entry that fails without a hash (kExpNone: none)
    int32_t *early_st;    // and its status
    uint32_t *vbad;       // the lowest entry whose value digest differs (atomicMin)
    uint8_t *trunc;       // entry 0's class is kExpTrunc
    uint64_t *size, *off /* n + 1 */;
    int32_t *status;
    uint8_t *trunc_out;
    // per entry
    uint64_t *rec_off;
    uint8_t *ver, *cls;
    uint64_t *esz, *epos;  // bytes of the entry in its blob, and of the tx's entries ahead of it
    const uint8_t **vsrc;  // an available value where it lies (null: none to hash)
    uint64_t *vlen;        // bytes to hash: the bucketing's lengths
    uint8_t *skip;         // no value to hash
    uint8_t *out;
    uint64_t out_cap;  // the caller's: a blob that ends beyond it is not written
};
// ecnt, ent_start and leaf_off from the records and verdicts
hipError_t launch_exp_counts(hipStream_t st, Timer *tm, const ExpArrays &a);
// per entry: class, size, value pointer; then per tx: the class rule, the
// canonical metadata, the blob size, off
hipError_t launch_exp_entries(hipStream_t st, Timer *tm, const ExpArrays &a);
hipError_t launch_exp_sizes(hipStream_t st, Timer *tm, const ExpArrays &a);
// everything of the blobs but the available values
hipError_t launch_exp_frame(hipStream_t st, Timer *tm, const ExpArrays &a);
// the values: hashed, compared, copied.  arm 'A': the hashing lane stores its
// blocks; 'B': hash-only lanes, then a wave per value copies.  perm: the
// bucketing's order or null
hipError_t launch_exp_values(hipStream_t st, Timer *tm, const ExpArrays &a, const uint32_t *perm,
                             char arm);
hipError_t launch_exp_status(hipStream_t st, Timer *tm, const ExpArrays &a);

// len bytes by the whole wave: 16-byte stores where the destination allows,
// bytes at the two ends
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t len, int lane) {
    const uint64_t head = min(len, (uint64_t)((16 - ((uintptr_t)dst & 15)) & 15));
    for (uint64_t i = lane; i < head; i += 64) dst[i] = src[i];
    const uint64_t nq = (len - head) / 16;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    const uint8_t *s = src + head;
    for (uint64_t q = lane; q < nq; q += 64) {
        uint4 v;
        __builtin_memcpy(&v, s + 16 * q, 16);
        d4[q] = v;
    }
    for (uint64_t i = head + 16 * nq + lane; i < len; i += 64) dst[i] = src[i];
}

__device__ __forceinline__ void copy32_a8(uint8_t *d, const uint8_t *s) {  // both 8-byte aligned
    const uint2 *a = (const uint2 *)s;
    uint2 *b = (uint2 *)d;
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = a[i];
}

// ---- VerifyDualProofV2 (verification.go:303-372) over device arrays
// Its rules, each written once, for k_dpv2_prep / k_dpv2_verdict and the
// document verifier's kernels (capi_doc.hip).  The operands of proof p's two
// ahtree proofs (:342-370); headers in device memory, sbl / tbl n x 32
__device__ __forceinline__ void dpv2_operands(uint64_t p, uint64_t src, const mh_tx_header *sh,
                                              const mh_tx_header *th, uint64_t *ii, uint64_t *ij,
                                              uint64_t *ci, uint8_t *sel, uint8_t *sbl,
                                              uint8_t *tbl) {
    ii[p] = src;
    ij[p] = th->bl_tx_id;
    sel[p] = src == 1;  // consistency of leafFor(sourceAlh) itself, :354-357
    ci[p] = src == 1 ? src : sh->bl_tx_id;
    copy32_a8(sbl + 32 * p, sh->bl_root);
    copy32_a8(tbl + 32 * p, th->bl_root);
}
// The status of a proof that passed the argument and Alh checks (:328-370)
__device__ __forceinline__ int32_t dpv2_ladder(const mh_tx_header *sh, const mh_tx_header *th,
                                               bool same_id, bool oki, bool okc) {
    if (sh->id - 1 != sh->bl_tx_id || th->id - 1 != th->bl_tx_id)
        return MH_ERR_UNEXPECTED_LINKING;  // :328-330
    if (same_id) return MH_OK;             // :332-334
    return !oki ? MH_ERR_INCLUSION_NOT_VALID : !okc ? MH_ERR_CONSISTENCY_NOT_VALID : MH_OK;
}

// argument checks + operands (k_dpv2_prep): hh 2 n headers for the Alh kernel
// and x 2 n x 32 Alh values, sources then targets; have_blob as for
// dp1_header_ok; status_in may be null or status_out
hipError_t launch_dpv2_prep(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *src_hdr,
                            const mh_tx_header *tgt_hdr, bool have_blob, const uint64_t *src,
                            const uint64_t *tgt, const uint8_t *src_alh, const uint8_t *tgt_alh,
                            const int32_t *status_in, uint64_t md_blob_len, Dp1V0Metadata v0_md,
                            mh_tx_header *hh, uint8_t *x, uint64_t *ii, uint64_t *ij,
                            uint64_t *ci, uint8_t *sel, uint8_t *sbl, uint8_t *tbl,
                            int32_t *status_out);
// leafFor(sourceAlh) (:346), inclusion, select, consistency; leaf / ca n x 32
hipError_t launch_dpv2_proofs(hipStream_t st, Timer *tm, uint64_t n, const uint64_t *ii,
                              const uint64_t *ij, const uint64_t *ci, const uint8_t *sel,
                              const uint8_t *sbl, const uint8_t *tbl, const uint8_t *src_alh_x,
                              const uint64_t *incl_off, const uint8_t *incl_terms,
                              const uint64_t *cons_off, const uint8_t *cons_terms, uint8_t *leaf,
                              uint8_t *ca, uint8_t *oki, uint8_t *okc);
// the verdict of every proof still MH_OK (:318-370); ast: the 2 n Alh statuses
hipError_t launch_dpv2_verdict(hipStream_t st, Timer *tm, uint64_t n, const mh_tx_header *hh,
                               const uint64_t *src, const uint64_t *tgt, const int32_t *ast,
                               const uint8_t *oki, const uint8_t *okc, int32_t *status);
// roots of many htrees (widths leaf_off[t+1]-leaf_off[t], small), one lane
// each, in place over nodes = their leaf hashes back to back
constexpr uint64_t kSmallTreeMax = 64;
// launch_small_roots covers every batch whose widest tree has <= 64 leaves
// without a host tree plan: a wave per tree for <= 2048 trees (latency), the
// level-parallel packed kernel for more (every node of a level at once,
// 512 / P trees per workgroup); wider trees go through the host tree plan
// (k_seg_level).
inline bool small_roots_fit(uint64_t ntrees, uint64_t wmax) {
    (void)ntrees;
    return wmax <= kSmallTreeMax;
}
// wmax: the widest tree (<= kSmallTreeMax picks the level-parallel kernel
// for many trees)
hipError_t launch_small_roots(hipStream_t st, Timer *tm, uint64_t ntrees, const uint64_t *leaf_off,
                              uint8_t *nodes, uint8_t *roots, uint64_t wmax);
// the levels above a row of 1 <= w <= 64 nodes (flat level-major, level 0 =
// the row) and their root, one single-wave launch
hipError_t launch_reduce_small(hipStream_t st, const uint8_t *nodes, uint64_t w, uint8_t *levels,
                               uint8_t *root);
// headers + first-entry offsets of tx records from the raw log (md_off relative to buf)
hipError_t launch_tx_hdr_from_raw(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                                  const uint64_t *rec_off, MhTxHeader *hdrs, uint64_t *ent_start);
// non-canonical metadata of a tx log: rec_off[e_idx[k]] = e_off[k];
// hdrs[h_idx[k]].md_off / md_len = low / high 32 bits of h_val[k]
hipError_t launch_txlog_patch(hipStream_t st, uint64_t ne, const uint64_t *e_idx,
                              const uint64_t *e_off, uint64_t *rec_off, uint64_t nh,
                              const uint64_t *h_idx, const uint64_t *h_val, MhTxHeader *hdrs);
hipError_t launch_put_eh(hipStream_t st, uint64_t n, const uint8_t *eh, MhTxHeader *hdrs);
// The fused a14 kernels (tx.go:533-630 per record, one launch for a group of
// records): headers, entry walk, entry digests + leaves, each tx's htree, Eh,
// innerHash + Alh against the stored Alh (statuses).  Arrays are indexed from
// the group's first record; leaf_off has ntx + 1 entries (nullable for
// k_txlog_lanes: the entry count is then the header's, checked by the
// structure pre-pass).  pre (nullable): the pre-pass statuses -- a record with
// pre[t] != 0 is not walked, its status is pre[t] and its Alh / Eh / header 0.
// ho (device addresses of pinned host arrays, or device arrays, each member
// nullable, indexed like the device arrays): results written there by the
// kernel too.  hdrs 8-byte aligned, alh / status 4-byte.
struct TxlogHostOut {
    uint32_t *status = nullptr;
    uint32_t *alh = nullptr;
    uint64_t *hdrs = nullptr;
    int eh_only = 0;  // of hdrs, only the Eh words (the host writes the rest)
};
// one wave per 64 / L records (k_txlog_wave, txlog_wave.hip), wmax <= 64;
// h_rec_off / h_alh_off: host-readable copies of rec_off / alh_off (the
// wave's LDS staging is sized from them)
hipError_t launch_txlog_wave(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                             const uint64_t *rec_off, const uint64_t *alh_off,
                             const uint64_t *leaf_off, const int32_t *pre, MhTxHeader *hdrs,
                             uint8_t *eh_out, uint8_t *alh_out, int32_t *status,
                             const TxlogHostOut &ho, uint64_t wmax, const uint64_t *h_rec_off,
                             const uint64_t *h_alh_off);
// every record on 1-16 lanes, each lane's subtree serial (k_txlog_lanes,
// txlog_lanes.hip), wmax <= kTxlLanesMaxEntries; log_len: the log's length
// (the checking build's range).  wmax_dev (nullable): the widest record as the
// structure pass found it on the device; wmax is then the launch shape (an
// upper bound of it, or a guess), the kernel takes the entries per lane from
// wmax_dev -- and if that is wider than the shape, does nothing but set
// *redo (device, required with wmax_dev) for the caller to launch again.
constexpr uint64_t kTxlLanesMaxEntries = 1024;
hipError_t launch_txlog_lanes(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                              const uint64_t *rec_off, const uint64_t *alh_off,
                              const uint64_t *leaf_off, const int32_t *pre, MhTxHeader *hdrs,
                              uint8_t *eh_out, uint8_t *alh_out, int32_t *status,
                              const TxlogHostOut &ho, uint64_t wmax, uint64_t log_len,
                              const uint64_t *wmax_dev = nullptr, uint64_t *redo = nullptr);
// The device structure pass over tx-log records (txlog_struct.hip), one lane
// per record, every check of the host hop (tx.go:419-588) on the device bytes:
//  * clog != null (mh_txlog_validate_clog): record t at the offset of cLog
//    entry t (BE64 offset || BE32 size [|| Alh], clog_es = 12 or 44 bytes,
//    immustore.go:122-123, 2569-2597); writes rec_off / alh_off / leaf_off
//    (leaf_off[t] = t's entry count, not a prefix);
//  * clog == null (mh_txlog_validate_resident): rec_off / alh_off / leaf_off
//    (prefix) from the host hop; the device bytes must parse to the same
//    structure, else the record is MH_ERR_CORRUPTED_DATA.
// pre[t]: the record's status (0, or the reader's error), kTxlNeedsHost for a
// record whose metadata is valid but not canonical or that is wider than the
// lanes kernel takes (the host re-validates those).  stats (device, zeroed by
// the caller): [0] widest accepted record, [1] records needing the host.
// lim (cLog mode, <= len): the bytes landed so far -- a record whose read runs
// past lim while lim < len needs the whole log and is left to the host
// (kTxlNeedsHost).
// Check mode: a record the device bytes give otherwise is MH_ERR_CORRUPTED_DATA.
constexpr int32_t kTxlNeedsHost = 0x40000000;
hipError_t launch_txlog_struct(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                               uint64_t len, uint64_t lim, const uint8_t *clog, uint32_t clog_es,
                               uint64_t *rec_off, uint64_t *alh_off, uint64_t *leaf_off,
                               uint32_t max_entries, uint32_t max_key_len, int32_t *pre,
                               uint64_t *stats);
// pre[t] = MH_ERR_CORRUPTED_DATA where a and b differ over record t's bytes
// [rec_off[t], alh_off[t] + 32), else MH_OK
hipError_t launch_txlog_bytes_cmp(hipStream_t st, uint64_t ntx, const uint8_t *a, const uint8_t *b,
                                  const uint64_t *rec_off, const uint64_t *alh_off, int32_t *pre);
// status[t] = pre[t] and the Alh zeroed where pre[t] != 0
hipError_t launch_txlog_apply_pre(hipStream_t st, uint64_t ntx, const int32_t *pre, int32_t *status,
                                  uint8_t *alh);
// stats[2] += the number of non-OK statuses, stats[3] = min(stats[3], the
// first non-OK record)
hipError_t launch_txlog_status_summary(hipStream_t st, uint64_t ntx, const int32_t *status,
                                       uint64_t *stats);
// up to three runs of words pinned host memory -> HBM by a kernel (k_fetch_host)
struct HostRuns {
    const uint64_t *src[3];
    uint64_t *dst[3];
    uint64_t n[3];
};
hipError_t launch_fetch_host(hipStream_t st, const HostRuns &r);
// up to three runs of 32-bit words HBM -> pinned host memory by a kernel (k_store_host)
struct HostWordRuns {
    const uint32_t *src[3];
    uint32_t *dst[3];
    uint64_t n[3];
};
hipError_t launch_store_host(hipStream_t st, const HostWordRuns &r);
hipError_t launch_txe_index(hipStream_t st, Timer *tm, uint64_t ntx, const uint8_t *buf,
                            const MhTxHeader *hdrs, const uint64_t *ent_start,
                            const uint64_t *leaf_off, uint64_t *rec_off, uint8_t *ver);
// entry digests (leaf = false) or their htree leaves, hashed in place from
// the raw tx-log entry records (k_txe_leaf)
hipError_t launch_txe_leaf(hipStream_t st, Timer *tm, uint64_t n, const uint8_t *buf,
                           const uint64_t *rec_off, const uint8_t *ver, bool leaf, uint8_t *out);
hipError_t launch_seg_level(hipStream_t st, Timer *tm, uint64_t nnodes, uint64_t level_base,
                            uint32_t nitems, const uint64_t *cur_base, const uint64_t *prev_base,
                            const uint64_t *prev_w, uint8_t *nodes);
// idx[p] == ~0 writes SHA256(nil) (the empty tree's root, htree.go:73-77)
hipError_t launch_gather32(hipStream_t st, uint64_t n, const uint8_t *src, const uint64_t *idx,
                           uint8_t *out);

// ---------------------------------------------------------------- proofs on the device
hipError_t launch_htree_proof(hipStream_t st, Timer *tm, const uint8_t *levels, uint64_t w,
                              uint64_t n, const uint64_t *leaf, uint8_t *terms, uint32_t max_terms,
                              uint32_t *nterms, int32_t *status);
hipError_t launch_ahtree_proof(hipStream_t st, Timer *tm, int kind, const uint8_t *dlog,
                               uint64_t size, uint64_t n, const uint64_t *i, const uint64_t *j,
                               uint8_t *terms, uint32_t max_terms, uint32_t *nterms,
                               int32_t *status);

// ---------------------------------------------------------------- wire formats (wire_kernels.hip)
// phase bit 1: sizes + status + off[0..n]; bit 2: write messages
uint64_t pb_scratch_bytes(uint64_t n);
// exclusive-offset scan: out[0] = 0, out[k+1] = sum in[0..k]; temp: pb_scan_temp_bytes(n)
size_t pb_scan_temp_bytes(uint64_t n);
hipError_t scan_offsets_u64(hipStream_t st, uint64_t n, const uint64_t *in, uint64_t *out,
                            uint8_t *temp);
// the same with temp made for more items than n: temp_bytes is the size it was made with
hipError_t scan_offsets_u64(hipStream_t st, uint64_t n, const uint64_t *in, uint64_t *out,
                            uint8_t *temp, size_t temp_bytes);
hipError_t launch_pb_dual_v2(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                             uint64_t size, uint64_t n, const MhTxHeader *src,
                             const MhTxHeader *tgt, const uint8_t *md_blob, uint8_t *out,
                             uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch);
hipError_t launch_pb_inclusion(hipStream_t st, Timer *tm, int phase, const uint8_t *levels,
                               uint64_t w, uint64_t n, const uint64_t *leaf, uint8_t *out,
                               uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch);
// DualProof (v1): scratch = pb_dual_v1_scratch_bytes(n); alh / inner = the digest
// window of txs first_tx .. first_tx + count - 1 (device, 16-byte aligned)
uint64_t pb_dual_v1_scratch_bytes(uint64_t n);
hipError_t launch_pb_dual_v1(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                             uint64_t size, uint64_t n, const MhTxHeader *src,
                             const MhTxHeader *tgt, const uint8_t *md_blob, uint64_t first_tx,
                             uint64_t count, const uint8_t *alh, const uint8_t *inner, uint8_t *out,
                             uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch);

// ---------------------------------------------------------------- whole answers (answer_kernels.hip)
// The txs one mh_verifiable_answer_pb_batch call reads, as a bitmap over
// [1, ntx] (bit x - 1 of bits: tx x is read) with rank[w] = the set bits below
// word w: tx x lies in slot rank[(x-1)/64] + popcount(bits below it) of the
// compacted per-tx arrays.  It is the DualProof (v1) writer's digest window
// in that call: rst[slot] is the record's verdict, lnk[slot] != 0 says that the
// stored PrevAlh is not the Alh of the tx before it (tx_reader.go:87-89).
struct RankWindow {
    const uint64_t *bits, *rank;
    const int32_t *rst;
    const uint8_t *lnk;
    uint64_t ntx;
    const uint64_t *pos;  // phase 2: where message p goes in `out`
#ifdef __HIPCC__
    __device__ __forceinline__ bool has(uint64_t x) const {
        return x >= 1 && x <= ntx && ((bits[(x - 1) >> 6] >> ((x - 1) & 63)) & 1);
    }
    __device__ __forceinline__ uint64_t slot(uint64_t x) const {  // has(x)
        const uint64_t b = x - 1, w = bits[b >> 6];
        return rank[b >> 6] + (uint64_t)__popcll(w & ((1ull << (b & 63)) - 1));
    }
    // the reads of txs lo .. hi in the reader's order: a record's verdict, then
    // its link to the one before (lo <= hi)
    __device__ __forceinline__ int32_t check(uint64_t lo, uint64_t hi) const {
        if (lo < 1 || hi > ntx) return MH_ERR_TX_NOT_FOUND;
        if (!has(lo)) return MH_ERR_ILLEGAL_STATE;
        const uint64_t s = slot(lo);
        for (uint64_t k = lo; k <= hi; k++) {
            if (!has(k)) return MH_ERR_ILLEGAL_STATE;  // not in the call's read set: never seen
            const uint64_t j = s + (k - lo);
            if (rst[j]) return rst[j];
            if (k > lo && lnk[j]) return MH_ERR_CORRUPTED_TX_DATA;
        }
        return MH_OK;
    }
    __device__ __forceinline__ uint64_t at(uint64_t p, const uint64_t *) const { return pos[p]; }
#endif
};
hipError_t launch_pb_dual_v1_ranked(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                                    uint64_t size, uint64_t n, const MhTxHeader *src,
                                    const MhTxHeader *tgt, const uint8_t *md_blob,
                                    const RankWindow &win, const uint8_t *alh, const uint8_t *inner,
                                    uint8_t *out, uint64_t *off, int32_t *status, uint8_t *scratch);

// Every device array of one mh_verifiable_answer_pb_batch call.  n requests,
// D distinct txs read (slots), E entries of the asked txs.
struct AnsArrays {
    // the store
    const uint8_t *txlog, *clog;
    uint64_t txlog_len, ntx;
    uint32_t es;
    // requests
    uint64_t n;
    const uint8_t *kind;
    const uint64_t *tx, *since;
    const uint8_t *keys, *entries;
    const uint64_t *key_off, *entry_off;
    int32_t *pre;           // steps 1-4 of the status list
    MhTxHeader *hs, *ht;    // DualProof(src, tgt)
    uint64_t *leaf;         // ENTRY: the key's entry in its tx
    const int32_t *dst;     // the DualProof writer's status
    const uint64_t *dp_off; // and its message lengths
    uint64_t *sizes, *dpos;
    const uint64_t *off;
    int32_t *status;
    // the read set
    uint64_t words;         // of bits
    uint64_t *bits, *wcnt, *rank;
    // slots
    uint64_t D;
    uint64_t *ids;
    uint8_t *gclog;
    MhTxHeader *hd;
    uint8_t *alh, *inner;
    int32_t *rst;
    uint8_t *lnk;
    uint32_t *flags;        // 1: asked, 2: asked by an ENTRY request
    uint64_t *ecnt, *ncnt, *txbody;
    const uint64_t *leaf_off, *lvl_off, *txpos;
    uint32_t *hsz;          // framed TxHeader bytes
    uint64_t *ent_start;    // where the record's first entry lies in the log
    // entries
    uint64_t E;
    uint64_t *rec_off, *esz;
    const uint64_t *epos;
    uint8_t *ver;
    uint8_t *dig, *nodes, *txbuf, *out;
    uint64_t out_cap;
};
hipError_t launch_ans_heads(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_popc(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_compact(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_verdict(hipStream_t st, Timer *tm, const AnsArrays &a);   // + links, counts
hipError_t launch_ans_trees(hipStream_t st, Timer *tm, const AnsArrays &a);     // levels of the ENTRY txs
hipError_t launch_ans_find(hipStream_t st, Timer *tm, const AnsArrays &a);      // Tx.IndexOf + entry sizes
hipError_t launch_ans_txsize(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_size(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_tx_write(hipStream_t st, Timer *tm, const AnsArrays &a);
hipError_t launch_ans_assemble(hipStream_t st, Timer *tm, const AnsArrays &a);

// ---- mh_tx_answer_pb_batch (capi_txspec.hip, txspec_kernels.hip): what the
// call keeps beside the AnsArrays of its read set.  A variant is a distinct
// (tx, actions) pair of the batch: its schema.Tx is laid out once.  A group is
// a distinct (tx, classes read) pair: its values are hashed once, by the lanes
// of its first variant (the primary).  An item is an entry of a variant's tx.
enum : uint8_t { kTxsDrop = 0, kTxsDigest = 1, kTxsValue = 2 };  // what an item contributes
constexpr uint8_t kTxsNoSpec = 0xff;  // a variant's mode: TxToProto; else kv | z << 2 | sql << 4
struct TxsArrays {
    const ExpVlog *vlogs;
    uint32_t nvlogs;
    int64_t now;
    // per request
    const uint8_t *kind;  // MH_TXA_*
    const uint32_t *rv;   // its variant
    int32_t *wst;         // the DualProof writer's phase 2: MH_OK where the answer is written
    // per variant (V, or V + 1 where noted), the first six from the host
    uint64_t V;
    const uint64_t *vtx;
    const uint8_t *vmode, *vprim;
    const uint32_t *vgroup, *vfirst, *vcnt;  // its group, its first request, its requests
    uint64_t *vslot;      // the tx's slot in the read set (~0: none)
    uint64_t *vw, *item_off /* V + 1 */;
    uint32_t *early_idx;  // the lowest entry that fails without a hash (kExpNone: none)
    int32_t *early_st;
    uint64_t *vbody;      // schema.Tx bytes (0: a header the writer cannot encode)
    uint32_t *vhsz;       // of them the framed TxHeader
    uint64_t *vshare, *vpos /* V + 1 */;  // bytes in txbuf (a variant of several requests), scanned
    uint8_t **vdst;       // where its schema.Tx is written (null: nowhere)
    uint32_t *gbad;       // per group: the lowest entry whose value digest differs (atomicMin)
    // per item
    uint64_t I;
    uint8_t *ikind, *ifail;  // kTxs*; the status of an entry that fails without a hash
    uint64_t *isz, *ipos;    // framed TxEntry bytes, and those of the variant's entries ahead
    const uint8_t **vsrc;    // a value to write where it lies
    uint64_t *vlen;          // bytes to hash: the bucketing's lengths (0 off the primary)
    uint8_t *skip;
    uint8_t *txbuf;
};
hipError_t launch_txs_variants(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
hipError_t launch_txs_plan(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
hipError_t launch_txs_size(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
hipError_t launch_txs_write(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
hipError_t launch_txs_values(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x,
                             const uint32_t *perm);
hipError_t launch_txs_assemble(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
hipError_t launch_txs_status(hipStream_t st, Timer *tm, const AnsArrays &a, const TxsArrays &x);
}  // namespace mh
