/*
 * immustore_merkle.h -- C ABI of the MI355X Merkle-hash engine for immudb.
 *
 * Drop-in boundary for ONE hot path of codenotary/immudb: the per-transaction
 * binary hash tree (embedded/htree), the entry hashing that feeds it
 * (value hash + TxEntryDigest + leaf hash), the cross-transaction append-only
 * tree (embedded/ahtree) and the proof re-hash of both.  The reference is Go;
 * it has no FFI for this path, so the replacement is a cgo shim that keeps the
 * Go signatures and forwards here (see INTEGRATION.md for the shim).
 *
 * Conventions (inherited from the Go reference):
 *  - every function returns an int status: MH_OK, a positive MH_ERR_* that
 *    mirrors one of the Go sentinel errors, or a negative HIP runtime error
 *    (-hipError_t).  Nothing aborts, throws or exits across this ABI.
 *  - digests are 32 raw bytes (Go [sha256.Size]byte); "levels" is the flat
 *    level-major copy of Go's HTree.levels: level l holds ceil(n/2^l) nodes
 *    (including the promoted odd node) starting at node mh_htree_level_offset.
 *  - mh_htree handles are not synchronised (like Go's HTree, one per pooled
 *    Tx, tx.go:70); use one per goroutine.  mh_ahtree handles ARE
 *    synchronised like Go's AHtree (t.mutex, ahtree.go:60-84): every
 *    mh_ahtree_* call holds the handle's lock, so readers (root, proofs,
 *    dLog reads) may run concurrently with appends.  A device pointer from
 *    mh_ahtree_dlog_device is valid only until the next append that grows
 *    the dLog.  An mh_ctx may be shared by many handles, and
 *    calls on different handles of one context may run concurrently from
 *    different threads (the context's scratch is locked and used on its own
 *    stream only).
 *  - mh_dev_* functions take DEVICE pointers, are asynchronous on the
 *    context's stream and allocate only to grow the context's scratch, on
 *    first use or on a larger batch (mh_dev_sha256_batch,
 *    mh_dev_htree_build_entries*, the mh_dev_ahtree_* appends; the growth is
 *    made under the context's lock); all other functions take HOST pointers
 *    and return after the result is in host memory.
 */
#ifndef IMMUSTORE_MERKLE_H
#define IMMUSTORE_MERKLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden visibility: only these entry points are
 * exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MH_ABI_VERSION 1

/* status codes */
#define MH_OK 0
#define MH_ERR_MAX_WIDTH_EXCEEDED 1  /* htree.ErrMaxWidthExceeded   htree.go:25 */
#define MH_ERR_ILLEGAL_ARGUMENTS 2   /* htree/ahtree.ErrIllegalArguments htree.go:26, ahtree.go:35 */
#define MH_ERR_ILLEGAL_STATE 3       /* htree.ErrIllegalState       htree.go:27 */
#define MH_ERR_EMPTY_TREE 4          /* ahtree.ErrEmptyTree         ahtree.go:42 */
#define MH_ERR_UNEXISTENT_DATA 5     /* ahtree.ErrUnexistentData    ahtree.go:44 */
#define MH_ERR_METADATA_UNSUPPORTED 6 /* store.ErrMetadataUnsupported tx.go:692 */
#define MH_ERR_CANNOT_RESET_TO_LARGER 7 /* ahtree.ErrCannotResetToLargerSize ahtree.go:45 */
#define MH_ERR_NO_DEVICE 8           /* no usable gfx950 device / library not initialised */
#define MH_ERR_OUT_OF_MEMORY 9
/* transaction layer (embedded/store) */
#define MH_ERR_SOURCE_TX_NEWER 10       /* store.ErrSourceTxNewerThanTargetTx immustore.go:101 */
#define MH_ERR_UNEXPECTED_LINKING 11    /* store.ErrUnexpectedLinkingError immustore.go:53 */
#define MH_ERR_INCLUSION_NOT_VALID 12   /* "inclusion proof does NOT validate" verification.go:349 */
#define MH_ERR_CONSISTENCY_NOT_VALID 13 /* "consistency proof does NOT validate" verification.go:368 */
#define MH_ERR_CORRUPTED_DATA 14        /* store.ErrCorruptedData immustore.go:77 (ALH mismatch, tx.go:625) */
#define MH_ERR_CORRUPTED_MAX_ENTRIES 15 /* ErrCorruptedTxDataMaxTxEntriesExceeded immustore.go:72 */
#define MH_ERR_CORRUPTED_MAX_KEYLEN 16  /* ErrCorruptedTxDataMaxKeyLenExceeded immustore.go:75 */
#define MH_ERR_CORRUPTED_UNKNOWN_VERSION 17 /* ErrCorruptedTxDataUnknownHeaderVersion immustore.go:74 */
#define MH_ERR_TRUNCATED 18             /* record cut short (io.ErrUnexpectedEOF from the reader) */
#define MH_ERR_BUFFER_TOO_SMALL 19      /* output capacity below the encoded size (wire formats) */
#define MH_ERR_INVALID_PROOF 20         /* store.ErrInvalidProof immustore.go:114 */
#define MH_ERR_UNSUPPORTED_TX_VERSION 21 /* store.ErrUnsupportedTxVersion immustore.go:90 */
#define MH_ERR_INVALID_PROOF_ENTRY 22   /* store.ErrInvalidProof from VerifyDocument's entry /
                                           hash-value check (pkg/verification/verification.go:60-76),
                                           i.e. raised BEFORE the document decode (:78-110) */
#define MH_ERR_COLLECTIVE 23            /* RCCL unavailable or a collective failed (mh_multi_*) */
#define MH_ERR_CORRUPTED_TX_DATA 24     /* store.ErrCorruptedTxData immustore.go:71 (binary linking
                                         * mismatch, immustore.go:2416) */
#define MH_ERR_TX_NOT_FOUND 25          /* store.ErrTxNotFound immustore.go:85 (a tx outside the
                                         * digest window of mh_*_dual_proof_pb_batch) */
/* the follower's ReplicateTx (mh_replicate_tx_batch) */
#define MH_ERR_NEWER_VERSION_OR_CORRUPTED 26 /* store.ErrNewerVersionOrCorruptedData immustore.go:91 */
#define MH_ERR_ILLEGAL_TRUNCATION_ARGUMENT 27 /* store.ErrIllegalTruncationArgument immustore.go:111 */
#define MH_ERR_NULL_KEY 28                /* store.ErrNullKey immustore.go:60 */
#define MH_ERR_MAX_KEY_LEN_EXCEEDED 29    /* store.ErrMaxKeyLenExceeded immustore.go:61 */
#define MH_ERR_MAX_VALUE_LEN_EXCEEDED 30  /* store.ErrMaxValueLenExceeded immustore.go:62 */
#define MH_ERR_MAX_TX_ENTRIES_EXCEEDED 31 /* store.ErrMaxTxEntriesLimitExceeded immustore.go:59 */
#define MH_ERR_TX_ALREADY_COMMITTED 32    /* store.ErrTxAlreadyCommitted immustore.go:58 */
#define MH_ERR_TX_OUT_OF_ORDER 33         /* "attempt to commit a tx in wrong order"
                                           * (store.ErrUnexpectedError immustore.go:89, :1716) */
#define MH_ERR_TX_NOT_REACHED 34          /* a tx behind the first refused one of its batch (no Go
                                           * sentinel: ReplicateTx is never called for it) */

#define MH_ERR_KEY_NOT_FOUND 35            /* store.ErrKeyNotFound from Tx.IndexOf, tx.go:361-368 */
#define MH_ERR_EOF 36  /* io.EOF from readValueAt (immustore.go:3187) or the vLog's ReadAt:
                          the value is not stored / not resident */

#define MH_MAX_TX_METADATA_LEN 268 /* maxTxMetadataLen tx_metadata.go:36-39 */
#define MH_MAX_KV_METADATA_LEN 11  /* maxKVMetadataLen kv_metadata.go:41-43 */

/* ahtree verification kinds (embedded/ahtree/verification.go) */
#define MH_AHT_INCLUSION 0      /* VerifyInclusion      verification.go:21 */
#define MH_AHT_CONSISTENCY 1    /* VerifyConsistency    verification.go:58 */
#define MH_AHT_LAST_INCLUSION 2 /* VerifyLastInclusion  verification.go:111 */

typedef struct mh_ctx mh_ctx;

/* TxHeader (embedded/store/tx.go:103-117) as a plain C struct.  md_len bytes of
 * TxMetadata.Bytes() (version 1 only) live at md_blob + md_off, md_blob being
 * the buffer passed next to the headers.  136 bytes, 8-byte aligned. */
typedef struct mh_tx_header {
    uint64_t id;
    int64_t ts;
    uint64_t bl_tx_id;
    uint8_t bl_root[32];
    uint8_t prev_alh[32];
    uint8_t eh[32];
    uint32_t version; /* 0 or 1 (TxHeader.Version) */
    uint32_t nentries;
    uint32_t md_len;
    uint32_t md_off;
} mh_tx_header;
typedef struct mh_htree mh_htree;
typedef struct mh_ahtree mh_ahtree;

int mh_abi_version(void);
const char *mh_status_string(int status);
int mh_device_count(int *count);

/* ---------------------------------------------------------------- context */
/* device_ordinal: HIP device; hip_stream: an existing hipStream_t to run on,
 * or NULL to create a private non-blocking stream. */
int mh_ctx_create(int device_ordinal, void *hip_stream, mh_ctx **out);
int mh_ctx_destroy(mh_ctx *ctx);
int mh_ctx_synchronize(mh_ctx *ctx);
void *mh_ctx_stream(mh_ctx *ctx);
/* Per-kernel timing with HIP events recorded around every launch on the
 * stream it runs on.  mh_ctx_timing synchronises and reports the total
 * milliseconds and launch count of kernels whose name starts with `prefix`. */
int mh_ctx_set_timing(mh_ctx *ctx, int enable);
int mh_ctx_timing(mh_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches);
int mh_ctx_timing_reset(mh_ctx *ctx);

/* TEST ONLY: fault injection for error-path tests.  The next `countdown`-th
 * time (1 = the next time) the library passes fault site `site`, it fails
 * there as if the HIP / RCCL call at that point had failed.  countdown 0
 * disarms the site.  Sites: MH_FAULT_RCCL_GROUP (inside the RCCL group of a
 * multi-device all-gather, after ncclGroupStart), MH_FAULT_TXLOG_AFTER_GROUP
 * (mh_txlog_validate, after the first chunk group's kernels were queued),
 * MH_FAULT_RCCL_GROUP_LATE (the same all-gather after every device's
 * collective was queued: the clique is aborted and the handle refuses every
 * later collective).  No reference counterpart: production callers never arm
 * it. */
#define MH_FAULT_RCCL_GROUP 1
#define MH_FAULT_TXLOG_AFTER_GROUP 2
#define MH_FAULT_RCCL_GROUP_LATE 3
int mh_debug_fail_at(int site, int countdown);

/* device memory helpers, so that a cgo caller needs no HIP headers */
int mh_dev_alloc(mh_ctx *ctx, uint64_t bytes, void **dptr);
int mh_dev_free(mh_ctx *ctx, void *dptr);
int mh_host_alloc_pinned(uint64_t bytes, void **hptr); /* pinned staging arena */
int mh_host_free_pinned(void *hptr);
int mh_memcpy_h2d(mh_ctx *ctx, void *dst, const void *src, uint64_t bytes); /* async */
int mh_memcpy_d2h(mh_ctx *ctx, void *dst, const void *src, uint64_t bytes); /* async */
/* deterministic synthetic data: splitmix64 words, word w = mix(seed + (w+1)*gamma) */
int mh_dev_fill_random(mh_ctx *ctx, void *dptr, uint64_t nbytes, uint64_t seed);
/* keys[i] = BE64(first + i)  (immustore_test.go:1844-1849 key shape) */
int mh_dev_fill_keys_be64(mh_ctx *ctx, void *dptr, uint64_t n, uint64_t first);

/* ------------------------------------------------------------------ htree */
/* Flat level layout (htree.go:45-66 capacity, :85-110 used widths). */
uint64_t mh_htree_levels_len(uint64_t n);
uint64_t mh_htree_level_offset(uint64_t n, int level);

/* htree.New(maxWidth)                                 htree.go:45-66 */
int mh_htree_new(mh_ctx *ctx, uint64_t max_width, mh_htree **out);
int mh_htree_free(mh_htree *t);
/* (*HTree).BuildWith(digests)                         htree.go:68-113 */
int mh_htree_build_with(mh_htree *t, const uint8_t *digests, uint64_t n);
/* value hash loop immustore.go:1620-1630 + Tx.BuildHashTree tx.go:332-355:
 * version 0 -> TxEntryDigest_v1_1, 1 -> TxEntryDigest_v1_2 (tx.go:321-330).
 * CSR inputs: *_off arrays have n+1 entries; md/md_off may be NULL (no KV
 * metadata); hval_override (n*32) + use_override (n bytes) model
 * EntrySpec.IsValueTruncated (may be NULL); hvals_out (n*32) may be NULL. */
int mh_htree_build_entries(mh_htree *t, int version, uint64_t n, const uint8_t *keys,
                           const uint64_t *key_off, const uint8_t *md, const uint64_t *md_off,
                           const uint8_t *vals, const uint64_t *val_off,
                           const uint8_t *hval_override, const uint8_t *use_override,
                           uint8_t *hvals_out);
/* (*HTree).Root()                                      htree.go:115-117 */
int mh_htree_root(mh_htree *t, uint8_t root[32]);
int mh_htree_width(mh_htree *t, uint64_t *width);
/* (*HTree).InclusionProof(i): terms leaf-side first   htree.go:121-164 */
int mh_htree_inclusion_proof(mh_htree *t, uint64_t i, uint8_t *terms, uint32_t cap,
                             uint32_t *nterms);
/* copy of the used levels (mh_htree_levels_len(width) nodes) */
int mh_htree_levels(mh_htree *t, uint8_t *out, uint64_t cap_nodes);
/* Many (*HTree).InclusionProof calls at once (htree.go:121-164), generated on
 * the device from the tree's resident levels: proof p (leaf[p]) gets nterms[p]
 * terms at terms + p * max_terms * 32, Go order (leaf side first);
 * status[p] = MH_OK or MH_ERR_ILLEGAL_ARGUMENTS (leaf >= width, or more than
 * max_terms terms; ceil(log2 width) always suffices). */
int mh_htree_inclusion_proof_batch(mh_htree *t, uint64_t n, const uint64_t *leaf, uint8_t *terms,
                                   uint32_t max_terms, uint32_t *nterms, int32_t *status);
/* device pointer of the handle's level buffer (device-resident consumers) */
int mh_htree_levels_device(mh_htree *t, const uint8_t **dptr);

/* htree.VerifyInclusion batch (htree.go:166-195; store.VerifyInclusion
 * verification.go:28-30).  Proof p has terms [term_off[p], term_off[p+1]).
 * leaf / width are the bits of Go ints (values >= 2^63 are negative and take
 * Go's signed % and /).  ok[p] = 1 if it verifies.  Host pointers. */
int mh_htree_verify_inclusion_batch(mh_ctx *ctx, uint64_t nproofs, const uint64_t *leaf,
                                    const uint64_t *width, const uint64_t *term_off,
                                    const uint8_t *terms, const uint8_t *digests,
                                    const uint8_t *roots, uint8_t *ok);

/* ------------------------------------------------- htree, device-resident */
/* Alignment of device digest arrays.  The kernels move a 32-byte digest as two
 * 16-byte vector accesses, so every device array of digests named below as
 * "16-byte aligned" must start on a 16-byte boundary; a call given a lesser
 * pointer returns MH_ERR_ILLEGAL_ARGUMENTS before anything is launched or
 * written.  Arrays of other types need the alignment of their element type
 * (uint64_t offsets 8, uint32_t / int32_t 4); byte arrays (message and value
 * bytes, keys, metadata, ok flags, protobuf output) take any alignment unless
 * a call says otherwise.  A call writes only the bytes its contract names:
 * an output of n rows is written inside its n rows and nowhere else. */
/* BuildWith over device digests. levels: mh_htree_levels_len(n)*32 bytes.
 * digests and levels 16-byte aligned; root (32 bytes, may be NULL) 16-byte
 * aligned as well: the kernels that finish a tree store it as a digest. */
int mh_dev_htree_build_digests(mh_ctx *ctx, const uint8_t *digests, uint64_t n, uint8_t *levels,
                               uint8_t *root);
/* Fused value hash + entry digest + leaf + all levels for fixed-stride
 * entries without KV metadata (BASELINE configs C1/C2/C4): key i at
 * keys + i*key_len, value i at vals + i*val_len.  keys / vals: any alignment
 * (a 16-byte aligned vals with val_len % 16 == 0 takes the fast loads).
 * hvals_out (n*32, may be NULL), levels and root: 16-byte aligned. */
int mh_dev_htree_build_entries_fixed(mh_ctx *ctx, int version, uint64_t n, const uint8_t *keys,
                                     uint32_t key_len, const uint8_t *vals, uint32_t val_len,
                                     uint8_t *hvals_out, uint8_t *levels, uint8_t *root);
/* General CSR variant (device arrays); scratch is allocated by the context.
 * keys / md / vals / use_override: any alignment.  hval_override, hvals_out,
 * levels and root: 16-byte aligned. */
int mh_dev_htree_build_entries(mh_ctx *ctx, int version, uint64_t n, const uint8_t *keys,
                               const uint64_t *key_off, const uint8_t *md, const uint64_t *md_off,
                               const uint8_t *vals, const uint64_t *val_off,
                               const uint8_t *hval_override, const uint8_t *use_override,
                               uint8_t *hvals_out, uint8_t *levels, uint8_t *root);
/* Reduce w given nodes (e.g. all-gathered per-GPU subtree roots) to a root
 * with htree's pairing rule; nodes are copied to level 0 of `levels`
 * (mh_htree_levels_len(w)*32 bytes) without leaf hashing.  nodes, levels and
 * root: 16-byte aligned. */
int mh_dev_htree_reduce_nodes(mh_ctx *ctx, const uint8_t *nodes, uint64_t w, uint8_t *levels,
                              uint8_t *root);
/* SHA-256 of n byte ranges buf[off[i], off[i+1]) -> out (n*32).  buf: any
 * alignment; out: 16-byte aligned. */
int mh_dev_sha256_batch(mh_ctx *ctx, const uint8_t *buf, const uint64_t *off, uint64_t n,
                        uint8_t *out);
/* The read-side value integrity check of ImmuStore.readValueAt
 * (embedded/store/immustore.go:3183-3240, the check at :3235) over a batch:
 * value i is vals[off[i], off[i+1]) -- the n_i bytes the vLog or the value
 * cache returned for a buffer of the entry's stored length vlen[i] -- and
 * status[i] = MH_OK, or MH_ERR_CORRUPTED_DATA when n_i != vlen[i] or
 * SHA256(value) != hvals[i] (32 bytes per entry), exactly as Go rejects it
 * ("value length or digest mismatch").  vlen may be NULL (lengths not
 * checked).  Host variant: host memory in and out, synchronous; the value
 * bytes go up in ~64 MiB chunks on a copy stream while the previous chunk is
 * checked; *ncorrupted (may be NULL) = entries not MH_OK.  Device variant:
 * every pointer device memory, asynchronous on the context stream; vals any
 * alignment, hvals 16-byte aligned; status[0..n) is written and nothing else. */
int mh_verify_values_batch(mh_ctx *ctx, uint64_t n, const uint8_t *vals, const uint64_t *off,
                           const uint64_t *vlen, const uint8_t *hvals, int32_t *status,
                           uint64_t *ncorrupted);
int mh_dev_verify_values_batch(mh_ctx *ctx, uint64_t n, const uint8_t *vals, const uint64_t *off,
                               const uint64_t *vlen, const uint8_t *hvals, int32_t *status);
/* Device variants of the batch proof generators: every pointer is device
 * memory (levels of a tree of `width` leaves / a dLog of `size` appends).
 * Of `terms` they write the nterms[p] terms of a row with status[p] == MH_OK
 * and nothing else: a refused row and the rest of a good one keep the caller's
 * bytes.  The host variants hand those bytes back as zero.  nterms[p] and
 * status[p] are written for every row (nterms[p] = the proof's length even
 * when it exceeds max_terms, 0 for a row refused for its arguments).
 * levels / dlog and terms: 16-byte aligned.  The verifier's terms, digests and
 * roots: 16-byte aligned; ok: n bytes, any alignment. */
int mh_dev_htree_inclusion_proof_batch(mh_ctx *ctx, const uint8_t *levels, uint64_t width,
                                       uint64_t n, const uint64_t *leaf, uint8_t *terms,
                                       uint32_t max_terms, uint32_t *nterms, int32_t *status);
int mh_dev_ahtree_proof_batch(mh_ctx *ctx, int kind, const uint8_t *dlog, uint64_t size,
                              uint64_t n, const uint64_t *i, const uint64_t *j, uint8_t *terms,
                              uint32_t max_terms, uint32_t *nterms, int32_t *status);
int mh_dev_htree_verify_inclusion_batch(mh_ctx *ctx, uint64_t nproofs, const uint64_t *leaf,
                                        const uint64_t *width, const uint64_t *term_off,
                                        const uint8_t *terms, const uint8_t *digests,
                                        const uint8_t *roots, uint8_t *ok);

/* ----------------------------------------------------------------- ahtree */
/* In-memory append-only tree whose dLog (ahtree.go:60-84, tree/NNNNNNNN.sha) lives
 * in HBM.  No pLog/cLog files: persistence stays with the Go appendables, which
 * mh_ahtree_append_batch_logs feeds with ready-made record streams. */
int mh_ahtree_new(mh_ctx *ctx, mh_ahtree **out);
int mh_ahtree_free(mh_ahtree *t);
/* (*AHtree).Append(d)                                   ahtree.go:246-373 */
int mh_ahtree_append(mh_ahtree *t, const uint8_t *payload, uint64_t plen, uint64_t *n,
                     uint8_t h[32]);
/* m fixed-size payloads appended in order (syncBinaryLinking batch,
 * immustore.go:1198-1232). roots_out (m*32, RootAt(n0+1..n0+m)) may be NULL. */
int mh_ahtree_append_batch(mh_ahtree *t, const uint8_t *payloads, uint64_t m, uint32_t plen,
                           uint8_t *roots_out);
/* mh_ahtree_append_batch that also returns the batch's appendable records
 * (SURVEY.md 8(f) row 4), ready for the Go appendables' Append calls of
 * (*AHtree).Append: plog_out (m*(4+plen) bytes, the data/NNNNNNNN.dat
 * stream: BE32 plen || payload per append, ahtree.go:266-282) and clog_out
 * (m*12 bytes, the commit/NNNNNNNN.di stream: BE64 pLog offset || BE32 plen,
 * ahtree.go:341-351); p_off0 = the pLog size before the batch (t.pLogSize).
 * The dLog bytes of the batch are mh_ahtree_dlog(nodes_upto(n0),
 * nodes_upto(n0+m) - nodes_upto(n0)).  Either output may be NULL. */
int mh_ahtree_append_batch_logs(mh_ahtree *t, const uint8_t *payloads, uint64_t m, uint32_t plen,
                                uint64_t p_off0, uint8_t *plog_out, uint8_t *clog_out,
                                uint8_t *roots_out);
int mh_ahtree_size(mh_ahtree *t, uint64_t *size);
/* (*AHtree).Root / RootAt                                ahtree.go:727-771 */
int mh_ahtree_root(mh_ahtree *t, uint64_t *n, uint8_t root[32]);
int mh_ahtree_root_at(mh_ahtree *t, uint64_t n, uint8_t root[32]);
/* (*AHtree).InclusionProof / ConsistencyProof            ahtree.go:525-651 */
int mh_ahtree_inclusion_proof(mh_ahtree *t, uint64_t i, uint64_t j, uint8_t *terms, uint32_t cap,
                              uint32_t *nterms);
int mh_ahtree_consistency_proof(mh_ahtree *t, uint64_t i, uint64_t j, uint8_t *terms,
                                uint32_t cap, uint32_t *nterms);
/* (*AHtree).ResetSize                                     ahtree.go:375-458 */
/* Many (*AHtree).InclusionProof (kind MH_AHT_INCLUSION, ahtree.go:525-577) or
 * ConsistencyProof (MH_AHT_CONSISTENCY, :579-651) calls at once, generated on
 * the device from the resident dLog; layout as mh_htree_inclusion_proof_batch;
 * status[p]: MH_OK, MH_ERR_ILLEGAL_ARGUMENTS (i > j, or > max_terms terms),
 * MH_ERR_UNEXISTENT_DATA (j > size or j == 0).  128 terms always suffice. */
int mh_ahtree_proof_batch(mh_ahtree *t, int kind, uint64_t n, const uint64_t *i,
                          const uint64_t *j, uint8_t *terms, uint32_t max_terms, uint32_t *nterms,
                          int32_t *status);
int mh_ahtree_reset_size(mh_ahtree *t, uint64_t new_size);
/* copy dLog digests [first, first+count) (the tree/NNNNNNNN.sha byte stream) */
int mh_ahtree_dlog(mh_ahtree *t, uint64_t first, uint64_t count, uint8_t *out);
int mh_ahtree_dlog_device(mh_ahtree *t, const uint8_t **dptr);

/* Device-resident batch append: dlog (16-byte aligned) holds nodesUpto(n0)
 * digests and has room for nodesUpto(n0+m); payloads m*plen bytes, any
 * alignment.  The call writes the nodes [nodesUpto(n0), nodesUpto(n0+m)) and
 * the m rows of roots_out (16-byte aligned, may be NULL); the nodes below
 * nodesUpto(n0) stay as they are. */
int mh_dev_ahtree_append_batch(mh_ctx *ctx, uint8_t *dlog, uint64_t n0, const uint8_t *payloads,
                               uint64_t m, uint32_t plen, uint8_t *roots_out);
/* Device variants of the appendable records: fused into the append's leaf
 * phase (the payload is read once), or alone (e.g. per rank of a sharded
 * append: rank r passes p_off0 + r*S*(4+plen)).  plog / clog: device memory
 * of m*(4+plen) / m*12 bytes, any alignment, either may be NULL. */
int mh_dev_ahtree_append_batch_logs(mh_ctx *ctx, uint8_t *dlog, uint64_t n0,
                                    const uint8_t *payloads, uint64_t m, uint32_t plen,
                                    uint64_t p_off0, uint8_t *plog, uint8_t *clog,
                                    uint8_t *roots_out);
int mh_dev_ahtree_log_records(mh_ctx *ctx, const uint8_t *payloads, uint64_t m, uint32_t plen,
                              uint64_t p_off0, uint8_t *plog, uint8_t *clog);
uint64_t mh_ahtree_nodes_upto(uint64_t n); /* ahtree.go:492-511 */
/* The appendable framing around those streams, host
 * code.  An ahtree's data/ tree/ commit/ logs are multiapps
 * (ahtree.go:106-140): file id holds logical bytes [id*file_size,
 * (id+1)*file_size) (multi_app.go:208-214, named "%08d.<dat|sha|di>") behind
 * a singleapp header BE32 len(m) || m (single_app.go:116-171), m =
 * appendable.Metadata.Bytes() (metadata.go:33-80) of { COMPRESSION_FORMAT,
 * COMPRESSION_LEVEL, PREALLOC_SIZE (omitted when prealloc_size < 0, as in
 * files written before it existed), WRAPPED_METADATA = { FILE_SIZE,
 * WRAPPED_METADATA = { VERSION: 1 } } }; Go writes each level's entries in
 * map order, any order reads back the same -- here in the order shown.
 * *len = the header size; MH_ERR_BUFFER_TOO_SMALL when out is NULL or cap is
 * below it. */
int mh_ahtree_log_header(uint64_t file_size, int64_t prealloc_size, int32_t compression_format,
                         int32_t compression_level, uint8_t *out, uint64_t cap, uint64_t *len);
/* appendable.Metadata.Bytes() of n (key, value) pairs in the given order. */
int mh_appendable_metadata(uint32_t n, const char *const *keys, const uint8_t *const *vals,
                           const uint64_t *val_len, uint8_t *out, uint64_t cap, uint64_t *len);
/* Logical log bytes [off, off+n) split at file boundaries: segment k =
 * seg[4k .. 4k+3] = (file id, byte position in that file = header_len + off
 * within the file, offset in the source range, length).  *nseg = the count
 * (seg may be NULL to ask for it); MH_ERR_BUFFER_TOO_SMALL if cap < *nseg. */
int mh_multiapp_segments(uint64_t off, uint64_t n, uint64_t file_size, uint64_t header_len,
                         uint64_t *seg, uint32_t cap, uint32_t *nseg);

/* dLog index of node(n, level) = nodesUntil(n) + level (ahtree.go:460-462). */
uint64_t mh_ahtree_node_index(uint64_t n, int level);

/* Sharded batch append.  mh_dev_ahtree_append_batch in three
 * phases so that G ranks can append one global batch together: rank r owns
 * appends (n0 + r*S, n0 + (r+1)*S], S = 2^shard_bits, n0 a multiple of S, and
 * keeps a dLog indexed like the global one (it only fills its own range and
 * the nodes above shard level).  Every perfect node of level <= shard_bits
 * and every spine node of a rank lies inside its range except the nodes
 * above shard level, which are built from the G shard roots.
 *  1. mh_dev_ahtree_append_local: leaves + perfect nodes of levels
 *     1..shard_bits ending in (n0, n0 + m];
 *  2. all-gather the 32-byte shard roots, dLog[mh_ahtree_node_index((r+1)*S
 *     + n0, shard_bits)] of every complete shard (RCCL, 32 B per rank);
 *  3. mh_dev_ahtree_put_shard_roots (count = complete shards before the
 *     global end, roots in shard order, for a batch starting at n0 = 0) writes
 *     them and the perfect nodes above them; mh_dev_ahtree_append_spine then
 *     finishes the rank's appends.  The rank's dLog range is byte-identical to
 *     a single-device append of the whole batch.
 * dlog, roots and roots_out (m x 32, may be NULL): 16-byte aligned.  Of dlog
 * the three calls write nodes of the rank's own range and the nodes above
 * shard level, each with the value the whole batch gives it, and no other. */
int mh_dev_ahtree_append_local(mh_ctx *ctx, uint8_t *dlog, uint64_t n0, const uint8_t *payloads,
                               uint64_t m, uint32_t plen, int shard_bits);
int mh_dev_ahtree_put_shard_roots(mh_ctx *ctx, uint8_t *dlog, int shard_bits, uint64_t count,
                                  const uint8_t *roots);
int mh_dev_ahtree_append_spine(mh_ctx *ctx, uint8_t *dlog, uint64_t n0, uint64_t m,
                               uint8_t *roots_out);

/* One device, the dLog kept as a RANGE (the replay of syncBinaryLinking,
 * immustore.go:1198-1232, with no copy of the old dLog on the device):
 * append m payloads onto a tree of size n0 whose peaks (as for
 * mh_multi_ahtree_append_batch, host memory, NULL when n0 == 0) are given;
 * dlog_range (device, 16-byte aligned) receives the new digests
 * [nodesUpto(n0), nodesUpto(n0 + m)) from its start, roots_out (16-byte
 * aligned, may be NULL) RootAt after each append.  Asynchronous on the context stream. */
int mh_dev_ahtree_append_range(mh_ctx *ctx, uint8_t *dlog_range, uint64_t n0,
                               const uint8_t *peaks, const uint8_t *payloads, uint64_t m,
                               uint32_t plen, uint8_t *roots_out);
/* The popcount(n) peaks of a tree of size n, lowest level first, from a
 * device dLog indexed from 0 (synchronous; peaks_out in host memory). */
int mh_dev_ahtree_peaks(mh_ctx *ctx, const uint8_t *dlog, uint64_t n, uint8_t *peaks_out);

/* ahtree proof re-hash, batch (verification.go).  kind = MH_AHT_*.
 * INCLUSION:      a = leaf (leafFor(alh)), b = root of j
 * CONSISTENCY:    a = root of i, b = root of j
 * LAST_INCLUSION: a = leaf, b = root (j ignored)
 * ok[p] = Verify*(...) ; eval_out (np*32 for INCLUSION / LAST, np*64 for
 * CONSISTENCY = ci||cj) may be NULL.  eval_out[p] is Go's EvalInclusion /
 * EvalConsistency / EvalLastInclusion of the proof wherever the verifier
 * walks it.  Where it answers without a walk -- i > j, i == 0, or i < j with
 * no terms (verification.go:22-24, :59-61), and for CONSISTENCY also i == j
 * with no terms (:63-65, where Go's Eval would index an empty proof) --
 * eval_out[p] is the leaf a[p] unchanged for INCLUSION and 64 zero bytes for
 * CONSISTENCY.  LAST_INCLUSION always walks, i == 0 included (ok[p] = 0).
 * Device variant: terms, a, b and eval_out 16-byte aligned; ok: nproofs bytes,
 * any alignment. */
int mh_ahtree_verify_batch(mh_ctx *ctx, int kind, uint64_t nproofs, const uint64_t *i,
                           const uint64_t *j, const uint64_t *term_off, const uint8_t *terms,
                           const uint8_t *a, const uint8_t *b, uint8_t *ok, uint8_t *eval_out);
int mh_dev_ahtree_verify_batch(mh_ctx *ctx, int kind, uint64_t nproofs, const uint64_t *i,
                               const uint64_t *j, const uint64_t *term_off, const uint8_t *terms,
                               const uint8_t *a, const uint8_t *b, uint8_t *ok,
                               uint8_t *eval_out);

/* ---------------------------------------------------------------- tx layer
 * SURVEY.md 8(a) a7 (header hashes), a13 (linear / dual proofs), a14 (tx-log
 * read-path validation) and a3 for many trees at once.  Hashing runs on the
 * device; the host side parses records and combines verdicts. */

/* TxHeader.Alh for n headers (tx.go:249-319: innerHash then
 * SHA256(BE64 id || prevAlh || innerHash)).  inner_out may be NULL.
 * Replaces per-header hdr.Alh() calls (tx.go:307, verification.go:141-150,
 * 317-325).  MH_ERR_ILLEGAL_ARGUMENTS: version not 0/1, md on a v0 header or
 * md_len > MH_MAX_TX_METADATA_LEN, md outside md_blob. */
int mh_tx_alh_batch(mh_ctx *ctx, uint64_t n, const mh_tx_header *hdrs, const uint8_t *md_blob,
                    uint64_t md_blob_len, uint8_t *inner_out, uint8_t *alh_out);
/* Device variant: hdrs / md_blob / outputs in device memory; eh (nullable,
 * n x 32) replaces hdrs[k].eh (e.g. Eh just built on the device).  scratch:
 * n * 384 bytes of device memory.  The headers' fields are not validated.
 * hdrs: 8-byte aligned (its struct); md_blob, eh and scratch: any alignment
 * (byte accesses); inner_out and alh_out: 16-byte aligned. */
int mh_dev_tx_alh_batch(mh_ctx *ctx, uint64_t n, const mh_tx_header *hdrs, const uint8_t *md_blob,
                        const uint8_t *eh, uint8_t *scratch, uint8_t *inner_out, uint8_t *alh_out);

/* Many independent htrees in one pass (Tx.BuildHashTree tx.go:332-355 over
 * many txs, e.g. the MaxConcurrency concurrent commits at immustore.go:1632):
 * tree t is digests[leaf_off[t] .. leaf_off[t+1]) and gets roots[t]
 * (width 0 -> SHA256(nil), htree.go:73-77).  leaf_off has ntrees + 1 entries. */
int mh_htree_build_many(mh_ctx *ctx, uint64_t ntrees, const uint64_t *leaf_off,
                        const uint8_t *digests, uint8_t *roots);

/* VerifyLinearProof (verification.go:40-64) for n proofs: proof p has
 * SourceTxID proof_src[p], TargetTxID proof_tgt[p] and terms
 * terms[term_off[p] .. term_off[p+1]); it is checked against src[p], tgt[p],
 * src_alh[p], tgt_alh[p].  ok[p] = 1 iff it verifies. */
int mh_verify_linear_proof_batch(mh_ctx *ctx, uint64_t n, const uint64_t *proof_src,
                                 const uint64_t *proof_tgt, const uint64_t *term_off,
                                 const uint8_t *terms, const uint64_t *src, const uint64_t *tgt,
                                 const uint8_t *src_alh, const uint8_t *tgt_alh, uint8_t *ok);

/* VerifyDualProofV2 (verification.go:304-372) for n proofs.  Proof p:
 * src_hdr[p], tgt_hdr[p] (md in md_blob), InclusionProof terms
 * incl_terms[incl_off[p] .. incl_off[p+1]), ConsistencyProof terms
 * cons_terms[cons_off[p] ..), checked against src[p], tgt[p], src_alh[p],
 * tgt_alh[p].  status[p] = MH_OK or the Go error: MH_ERR_ILLEGAL_ARGUMENTS,
 * MH_ERR_SOURCE_TX_NEWER, MH_ERR_UNEXPECTED_LINKING,
 * MH_ERR_INCLUSION_NOT_VALID, MH_ERR_CONSISTENCY_NOT_VALID. */
int mh_verify_dual_proof_v2_batch(mh_ctx *ctx, uint64_t n, const mh_tx_header *src_hdr,
                                  const mh_tx_header *tgt_hdr, const uint8_t *md_blob,
                                  uint64_t md_blob_len, const uint64_t *incl_off,
                                  const uint8_t *incl_terms, const uint64_t *cons_off,
                                  const uint8_t *cons_terms, const uint64_t *src,
                                  const uint64_t *tgt, const uint8_t *src_alh,
                                  const uint8_t *tgt_alh, int32_t *status);

/* pkg/verification.VerifyDocument (pkg/verification/verification.go:37-196),
 * the hashing part, for n documents: replaces the per-document Go calls of a
 * client verifying many ProofDocumentResponses.  The caller keeps what is not
 * hashing: the document-id lookup and encodedKeyForDocument (:50-58), the
 * EncodedDocument decode and proto.Equal against the caller's document
 * (:78-110, which Go runs between the entry check and the htree) and the
 * signature check of the new state (:199-205).
 * Document d:
 *   doc[doc_off[d] .. doc_off[d+1])              proof.EncodedDocument
 *   doc_key[doc_key_off[d] .. doc_key_off[d+1])  encodedKeyForDocument(...)
 *   tx_hdr[d]                                    VerifiableTx.Tx.Header (its Eh is checked)
 *   entries ent_off[d] .. ent_off[d+1] of the flat entry arrays (offsets index
 *   ekey_off / emd_off / ehval directly): key ekeys[ekey_off[e] .. ekey_off[e+1]),
 *   KVMetadata.Bytes() emd[emd_off[e] .. emd_off[e+1]) (emd_off may be NULL:
 *   no metadata), HValue ehval[32 e]
 *   src_hdr[d], tgt_hdr[d], InclusionProof incl_terms[incl_off[d] .. incl_off[d+1]),
 *   ConsistencyProof cons_terms[cons_off[d] ..)  VerifiableTx.DualProof (V2)
 *   known_tx_id[d] (0: no known state), known_alh[32 d]  knownState
 * Tx metadata of every header lives in md_blob (mh_tx_header.md_off).
 * status[d]: MH_OK; MH_ERR_INVALID_PROOF_ENTRY (:60-76); MH_ERR_UNSUPPORTED_TX_VERSION
 * (:118-121); MH_ERR_INVALID_PROOF (Eh :137-139, headers :146-163, known state
 * :165-183); MH_ERR_ILLEGAL_ARGUMENTS for a header Go cannot hash (its
 * innerHash panics); or the VerifyDualProofV2 status.  target_alh_out[32 d]
 * (may be NULL): the new state's TxHash (the target header's Alh) when OK,
 * zeros otherwise. */
typedef struct mh_document_batch {
    uint64_t n;
    const uint8_t *doc;
    const uint64_t *doc_off;
    const uint8_t *doc_key;
    const uint64_t *doc_key_off;
    const mh_tx_header *tx_hdr;
    const uint64_t *ent_off;
    const uint8_t *ekeys;
    const uint64_t *ekey_off;
    const uint8_t *emd;
    const uint64_t *emd_off;
    const uint8_t *ehval;
    const mh_tx_header *src_hdr;
    const mh_tx_header *tgt_hdr;
    const uint8_t *md_blob;
    uint64_t md_blob_len;
    const uint64_t *incl_off;
    const uint8_t *incl_terms;
    const uint64_t *cons_off;
    const uint8_t *cons_terms;
    const uint64_t *known_tx_id;
    const uint8_t *known_alh;
} mh_document_batch;
int mh_verify_document_batch(mh_ctx *ctx, const mh_document_batch *batch, int32_t *status,
                             uint8_t *target_alh_out);

/* VerifyDualProof (verification.go:127-235: v1 proofs with linear and
 * linear-advance parts) for n proofs, all arrays host memory, term lists as
 * CSR (x_off has n + 1 entries, terms x_terms[x_off[p] .. x_off[p+1])).
 * The linear-advance inclusion proofs of proof p are nested proofs
 * advance_incl_first[p] .. advance_incl_first[p+1]) whose terms are
 * advance_incl_terms[advance_incl_off[q] .. advance_incl_off[q+1]).
 * has_linear / has_advance = 0 stand for Go's nil proofs.  ok[p] = 1 iff the
 * proof verifies (the Go function returns bool); a header that cannot be
 * hashed (version above 1, metadata on a version-0 header, metadata outside
 * md_blob) makes it 0.  No offset array need start at 0 (a slice of a larger
 * batch: advance the per-proof pointers, keep the term pointers); each must be
 * monotonic, advance_incl_off over [advance_incl_first[0],
 * advance_incl_first[n]], else MH_ERR_ILLEGAL_ARGUMENTS.  The arrays go up as
 * they are and the whole check runs on the device. */
typedef struct mh_dual_proof_batch {
    uint64_t n;
    const mh_tx_header *src_hdr;
    const mh_tx_header *tgt_hdr;
    const uint8_t *md_blob;
    uint64_t md_blob_len;
    const uint64_t *incl_off;
    const uint8_t *incl_terms;
    const uint64_t *cons_off;
    const uint8_t *cons_terms;
    const uint8_t *target_bl_tx_alh; /* n x 32 (DualProof.TargetBlTxAlh) */
    const uint64_t *last_off;
    const uint8_t *last_terms;
    const uint8_t *has_linear;
    const uint64_t *linear_src; /* LinearProof.SourceTxID */
    const uint64_t *linear_tgt; /* LinearProof.TargetTxID */
    const uint64_t *linear_off;
    const uint8_t *linear_terms;
    const uint8_t *has_advance;
    const uint64_t *advance_off;
    const uint8_t *advance_terms;
    const uint64_t *advance_incl_first;
    const uint64_t *advance_incl_off;
    const uint8_t *advance_incl_terms;
    const uint64_t *src;
    const uint64_t *tgt;
    const uint8_t *src_alh;
    const uint8_t *tgt_alh;
} mh_dual_proof_batch;
int mh_verify_dual_proof_batch(mh_ctx *ctx, const mh_dual_proof_batch *b, uint8_t *ok);

/* The wire side of v1: DualProofFromProto (database_protoconv.go:213-224,
 * LinearProofFromProto :264-270, LinearAdvanceProofFromProto :272-287) over n
 * DualProof messages msgs[msg_off[p] .. msg_off[p+1]), on the device, into the
 * arrays of mh_dual_proof_batch (same names and layout; tx metadata packed into
 * md_blob as for mh_dual_proof_v2_pb_decode_batch).  status[p]: MH_OK;
 * MH_ERR_CORRUPTED_DATA (not a valid encoding: zero headers, no terms);
 * MH_ERR_ILLEGAL_ARGUMENTS (a header or the linear proof missing: Go's
 * conversion dereferences them).  Capacities are in terms, advance_incl_cap in
 * nested InclusionProofs; when one is short the n + 1 offset arrays and the
 * statuses are written and MH_ERR_BUFFER_TOO_SMALL is returned (the size query;
 * nested_proofs / nested_terms report the nested totals on every return). */
typedef struct mh_dual_proof_decoded {
    mh_tx_header *src_hdr;        /* n */
    mh_tx_header *tgt_hdr;        /* n */
    uint8_t *md_blob;             /* room for 2n x MH_MAX_TX_METADATA_LEN */
    uint8_t *target_bl_tx_alh;    /* n x 32 */
    uint8_t *has_linear;          /* n */
    uint64_t *linear_src;         /* n */
    uint64_t *linear_tgt;         /* n */
    uint8_t *has_advance;         /* n */
    uint64_t *incl_off, *cons_off, *last_off, *linear_off, *advance_off; /* n + 1 each */
    uint64_t *advance_incl_first; /* n + 1 */
    uint64_t *advance_incl_off;   /* advance_incl_cap + 1 */
    uint8_t *incl_terms, *cons_terms, *last_terms, *linear_terms, *advance_terms;
    uint8_t *advance_incl_terms;
    uint64_t incl_cap, cons_cap, last_cap, linear_cap, advance_cap;
    uint64_t advance_incl_cap, advance_incl_terms_cap;
    uint64_t nested_proofs, nested_terms; /* out */
} mh_dual_proof_decoded;
int mh_dual_proof_pb_decode_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                  const uint64_t *msg_off, mh_dual_proof_decoded *out,
                                  int32_t *status);

/* Tx-log read path (Tx.readFrom tx.go:388-630: readHeader, readEntry,
 * buildAndValidateHtree) over buf = back-to-back tx records as written by
 * immustore.go:1812-1924.  Parses up to max_txs records, stopping at id 0 (a
 * preallocated tail) or at the first structural error, which is returned
 * (MH_ERR_CORRUPTED_* / MH_ERR_TRUNCATED) with *consumed = that record's
 * offset; then, on the device, rebuilds every entry digest, every tx's htree
 * (Eh) and Alh and compares it with the stored one: status[k] = MH_OK or
 * MH_ERR_CORRUPTED_DATA ("ALH mismatch", tx.go:625).  Optional outputs
 * (capacity max_txs): hdrs (md_off relative to buf, eh = rebuilt Eh) and
 * alh (recomputed).  Of hdrs, alh and status the rows [0, *ntx) are written;
 * the rows from *ntx up to the capacity keep the caller's bytes (pageable,
 * pinned or device memory alike).  KV / tx metadata are parsed as the reader parses them
 * (KVMetadata.unsafeReadFrom kv_metadata.go:221-256, TxMetadata.ReadFrom
 * tx_metadata.go:159-193): unknown attribute codes, short payloads and an
 * extra running past the metadata stop the parse with MH_ERR_CORRUPTED_DATA;
 * valid metadata is hashed in its re-serialized form (Bytes(), attributes in
 * code order, a repeated attribute's last value), as Go hashes it -- records
 * whose stored metadata is not already in that form (never written by immudb)
 * are hashed from canonical copies placed after the log on the device. */
/* The record structure alone (host only, no hashing, no device): the same
 * parse as mh_txlog_validate (readHeader / readEntry limits and errors,
 * tx.go:419-603) returning the headers (eh zero) and the offset of each
 * record's stored Alh.  Long runs are parsed by several threads from
 * speculated record starts; the result is always the sequential parse's. */
int mh_txlog_scan(const uint8_t *buf, uint64_t len, uint32_t max_entries, uint32_t max_key_len,
                  uint64_t max_txs, uint64_t *ntx, uint64_t *consumed, mh_tx_header *hdrs,
                  uint64_t *alh_off);
int mh_txlog_validate(mh_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t max_entries,
                      uint32_t max_key_len, uint64_t max_txs, uint64_t *ntx, uint64_t *consumed,
                      mh_tx_header *hdrs, uint8_t *alh, int32_t *status);
/* The same check of a log that is ALREADY in device memory -- the caller
 * re-validating what it just wrote or keeps resident (a scrub of the tx log,
 * the indexer's readTx of recent txs, embedded/store/indexer.go:570, tx.go:
 * 388-630): buf is the host copy the record hop parses, dlog (device, on the
 * context's device) the same len bytes, read by the kernels in place -- no
 * host->device copy.  The device allocation holding dlog must extend at least
 * 256 bytes past dlog + len (checked: MH_ERR_ILLEGAL_ARGUMENTS).  Outputs and
 * statuses as mh_txlog_validate.  The kernels never walk a length of dlog:
 * every record's structure in dlog is checked on the device against the host
 * copy's first, and a record whose resident bytes give another structure (or
 * differ from buf, for records the fused kernels do not take) is
 * MH_ERR_CORRUPTED_DATA with its Alh zeroed -- a drifted resident log is
 * reported per record, never a fault. */
int mh_txlog_validate_resident(mh_ctx *ctx, const uint8_t *buf, const uint8_t *dlog, uint64_t len,
                               uint32_t max_entries, uint32_t max_key_len, uint64_t max_txs,
                               uint64_t *ntx, uint64_t *consumed, mh_tx_header *hdrs,
                               uint8_t *alh, int32_t *status);
/* The same check of a log already in device memory, indexed by the store's
 * commit log instead of a host copy (no host hop, no host->device copy of the
 * log): ImmuStore.readTx for txs 1..ntx of the cLog (immustore.go:3048-3060 ->
 * txOffsetAndSize :2569-2597 -> Tx.readFrom tx.go:388-630).  clog holds ntx
 * commit-log entries of clog_entry_size bytes (12: BE64 tx offset || BE32 tx
 * size, cLogEntrySizeV1; 44: + the tx's Alh, cLogEntrySizeV2,
 * immustore.go:122-123) -- the entries after the appendable header, in device
 * or host memory.  dlog: the tx-log data (after its appendable header), len
 * bytes, either on the context's device, its allocation extending 256 bytes
 * past it, or in host memory (pinned -- the cgo shim's arena -- or pageable):
 * then it is copied up in chunks (5 : 2 : 1 from 16 MiB, as
 * mh_txlog_validate) and, when the cLog entries are in log order, the records
 * ending in each chunk are checked as soon as it lands.  Record t is parsed where entry t points, on to the end of the log as Go's
 * reader does; status[t] (each output nullable; device, pinned or pageable
 * memory, capacity ntx):
 *   MH_ERR_TRUNCATED        the record runs past len / reads as an id-0 tail
 *                           (readTx's "unexpected EOF", ErrCorruptedTxData);
 *   MH_ERR_CORRUPTED_*, MH_ERR_METADATA_UNSUPPORTED  the reader's structural
 *                           errors, as mh_txlog_validate reports them;
 *   MH_ERR_CORRUPTED_DATA   ALH mismatch (tx.go:625); or the record does not
 *                           end exactly at offset + size, or a 44-byte entry's
 *                           Alh differs (the open path's cLog checks,
 *                           immustore.go:458-528);
 * with hdrs (md_off relative to dlog, eh rebuilt) and alh as mh_txlog_validate
 * for valid records, zeros for records with a structural error.  *nbad: the
 * number of non-OK records, *first_bad: the first (ntx when none).  Returns
 * MH_OK when the call ran.  Records with metadata not in Go's canonical form
 * or with more than 1024 entries (and, for a host log, records whose read runs
 * past their chunk) are re-validated on the host bytes of that record alone
 * (mh_txlog_validate). */
int mh_txlog_validate_clog(mh_ctx *ctx, const uint8_t *dlog, uint64_t len, const uint8_t *clog,
                           uint64_t ntx, uint32_t clog_entry_size, uint32_t max_entries,
                           uint32_t max_key_len, mh_tx_header *hdrs, uint8_t *alh,
                           int32_t *status, uint64_t *nbad, uint64_t *first_bad);

/* ------------------------------------------------------------ commit path */
/* the hashing of ImmuStore.precommit / preCommitWith
 * (immustore.go:1620-1632 and 2301-2313: hVal = SHA256(value), or
 * EntrySpec.HashValue when IsValueTruncated, then Tx.BuildHashTree
 * tx.go:332-355 -> header Eh) for a batch of transactions, plus the
 * replicated-tx check `tx.header.Eh != hdr.Eh` (immustore.go:1649-1654).
 * A pipe owns a copy stream, a compute stream and three slots of device /
 * pinned buffers; a batch is cut into chunks of whole transactions
 * (~chunk_bytes of keys + values each, 0 = 64 MiB) whose host->device copies
 * run back to back under the hashing of the previous chunks.  Outputs in
 * pinned memory receive the device->host copies directly.  Not synchronised:
 * one pipe per goroutine. */
typedef struct mh_commit_pipe mh_commit_pipe;
int mh_commit_pipe_new(mh_ctx *ctx, uint64_t chunk_bytes, mh_commit_pipe **out);
int mh_commit_pipe_free(mh_commit_pipe *p);
/* Transaction t owns entries [tx_off[t], tx_off[t+1]) (tx_off: ntx + 1
 * entries, ascending); entry e has key keys[key_off[e] .. key_off[e+1]), KV
 * metadata (KVMetadata.Bytes(), kv_metadata.go:207-219) md[md_off[e] ..
 * md_off[e+1]) and value vals[val_off[e] .. val_off[e+1]) -- offsets index
 * the host arrays directly; md / md_off may both be NULL (no metadata).
 * hval_override + use_override (both or neither) model IsValueTruncated.
 * Outputs, host memory: hvals_out[e - tx_off[0]] (may be NULL), eh_out[t]
 * (may be NULL) and status[t]: MH_OK; MH_ERR_MAX_WIDTH_EXCEEDED if the tx has
 * more than max_width entries (htree.go:69-71; 0 = no limit);
 * MH_ERR_METADATA_UNSUPPORTED for KV metadata under version 0 (tx.go:691-693);
 * MH_ERR_ILLEGAL_ARGUMENTS if expect_eh (ntx x 32, may be NULL) differs from
 * the built Eh ("entries hash (Eh) differs", immustore.go:1651).  eh_out is
 * zeroed for the first two.  Pinned inputs (mh_host_alloc_pinned) make the
 * copies asynchronous DMA; pageable inputs work at the runtime's staged rate. */
int mh_precommit_batch(mh_commit_pipe *p, int version, uint64_t max_width, uint64_t ntx,
                       const uint64_t *tx_off, const uint8_t *keys, const uint64_t *key_off,
                       const uint8_t *md, const uint64_t *md_off, const uint8_t *vals,
                       const uint64_t *val_off, const uint8_t *hval_override,
                       const uint8_t *use_override, const uint8_t *expect_eh, uint8_t *hvals_out,
                       uint8_t *eh_out, int32_t *status);

/* ------------------------------------------------------------ follower path */
/* ImmuStore.ReplicateTx (immustore.go:2772-2932) for a run of exported txs in
 * one device pass: the bytes ExportTx wrote (:2621-2770) are parsed, every
 * value hashed where it lies, each tx's hash tree rebuilt, and the precommit
 * checks against the exported header (:1560-1755) decided against t, the
 * follower's ahtree (size P = the last precommitted tx id; dLog resident).
 * Tx k is txs[tx_off[k] .. tx_off[k+1]):
 *   BE32 hdrLen | TxHeader.Bytes() (tx.go:103-164) |
 *   per entry BE16 kLen | key | BE16 mdLen | md | BE32 vLen | value |
 *   [BE16 tLen | tLen bytes, the first one 1 = values truncated]
 * status[k] is what ReplicateTx would return for tx k had every earlier tx of
 * the batch been applied; the first failing check decides, in Go's order:
 *  envelope (:2773-2796): empty, < 4 bytes, < 4 + hdrLen bytes
 *                                          -> MH_ERR_ILLEGAL_ARGUMENTS
 *  TxHeader.ReadFrom (tx.go:166-247): < 124 bytes, id 0 -> ILLEGAL_ARGUMENTS;
 *    v1 with len < i + mdLen + 4 or mdLen > 268, TxMetadata.ReadFrom errors
 *    (as mh_txlog_validate) -> MH_ERR_CORRUPTED_DATA; version above 1 ->
 *    MH_ERR_NEWER_VERSION_OR_CORRUPTED; NEntries 0, BlTxID >= id ->
 *    ILLEGAL_ARGUMENTS.  A v1 header that ends inside Eh, BlTxID or BlRoot ->
 *    ILLEGAL_ARGUMENTS (Go zero-fills a short Eh / BlRoot and panics on a
 *    short BlTxID).  Bytes after BlRoot inside hdrLen are ignored, as in Go.
 *  entries (:2806-2856), i the read position, len the blob's length:
 *    len < i + 8; after kLen, len < i + 6 + kLen; after mdLen, len < i +
 *    mdLen; after vLen, len < i + vLen -> ILLEGAL_ARGUMENTS (the first two
 *    are looser than the bytes read: they count 6 bytes of lengths);
 *    KVMetadata.unsafeReadFrom errors -> CORRUPTED_DATA; a vLen word that
 *    would be read past the blob (metadata used up the slack; Go panics) ->
 *    ILLEGAL_ARGUMENTS.
 *  trailer (:2858-2881): none = not truncated; a 1-byte trailer (Go panics),
 *    len < i + tLen, tLen == 0 (Go indexes v[0]) -> ILLEGAL_ARGUMENTS; v[0] >
 *    1 -> MH_ERR_ILLEGAL_TRUNCATION_ARGUMENT; bytes left over ->
 *    ILLEGAL_ARGUMENTS.
 *  OngoingTx.set per entry in order (ongoing_tx.go:242-267): empty key ->
 *    MH_ERR_NULL_KEY; key > max_key_len -> MH_ERR_MAX_KEY_LEN_EXCEEDED; value
 *    > max_value_len (not truncated txs only) -> MH_ERR_MAX_VALUE_LEN_EXCEEDED;
 *    a new key while more than max_entries are held ->
 *    MH_ERR_MAX_TX_ENTRIES_EXCEEDED.  A key that repeats replaces the earlier
 *    entry (compared byte for byte), so validateAgainst (:798) fails the tx
 *    with ILLEGAL_ARGUMENTS; more than max_entries distinct keys ->
 *    MAX_TX_ENTRIES_EXCEEDED (validateEntries immustore.go:3243).
 *  hashing (:1620-1632): hVal = SHA256(value), or for a truncated tx the
 *    first 32 bytes of "value", zero-padded (digest, :3666); the entry digest
 *    of the header's version, KV metadata in its re-serialised form; KV
 *    metadata under version 0 -> MH_ERR_METADATA_UNSUPPORTED; Eh = the root.
 *  against the exported header (:1649-1722), R = P + k the id reached so far:
 *    built Eh != hdr.Eh unless MH_REPL_SKIP_INTEGRITY -> ILLEGAL_ARGUMENTS;
 *    id <= R -> MH_ERR_TX_ALREADY_COMMITTED; id > R + 1 ->
 *    MH_ERR_TX_OUT_OF_ORDER (Go waits in WaitFor for the txs between and
 *    fails "wrong order" only under concurrent writers: a batch cannot wait);
 *    BlRoot != RootAt(BlTxID) over the P resident leaves plus the Alh of
 *    every earlier tx of the batch (zeros for BlTxID 0) -> ILLEGAL_ARGUMENTS;
 *    PrevAlh != the Alh reached so far (prev_alh, then the computed Alh of
 *    the tx before) -> ILLEGAL_ARGUMENTS.
 * The tx's Alh is TxHeader.Alh() over the header as precommitted: the built
 * Eh, even when it was not compared.  *accepted = a, the length of the all-OK
 * prefix; unless MH_REPL_DRY_RUN exactly those a Alh values are appended to t
 * (the dLog bytes of mh_ahtree_append_batch), nothing else of t changes.  Tx a
 * keeps its verdict; every later tx gets its own envelope-through-Eh verdict
 * if that is an error, else MH_ERR_TX_NOT_REACHED.
 * Outputs (host memory), for every tx whose bytes parsed (zeros otherwise):
 * hdrs[k] with md_off into md_blob (slot k x MH_MAX_TX_METADATA_LEN, canonical
 * bytes) and eh = the built Eh once the tx was hashed (else the exported one);
 * alh[32 k] for a tx whose envelope-through-Eh verdict is MH_OK; ent_off[k] ..
 * ent_off[k+1]) its entries in ents / hvals (md_off / md_len: the bytes as
 * exported).  ents == NULL: no entry outputs.  ents_cap too small returns
 * MH_ERR_BUFFER_TOO_SMALL with the needed count in ent_off[n], t untouched.
 * NULL t / b / status / accepted, a non-monotonic tx_off, n >= 2^31 or above
 * the md_blob frame (2 n x 268 < 2^32) return MH_ERR_ILLEGAL_ARGUMENTS before
 * any device work.  The blobs go up once in the chunks and groups of
 * mh_verify_dual_proof_pb_batch (MH_PB_CHUNK_MIB, MH_PB_GROUP_RATIO); the
 * host never reads them. */
#define MH_REPL_SKIP_INTEGRITY 1u /* ReplicateTx's skipIntegrityCheck: Eh is not compared (immustore.go:1650-1654) */
#define MH_REPL_DRY_RUN        2u /* verdicts and outputs only; the tree is left as it was */

typedef struct mh_replicated_entry { /* where entry e lies in its blob, offsets relative to txs */
    uint64_t key_off, md_off, val_off;
    uint32_t key_len, md_len, val_len, flags; /* flags bit 0: value truncated (val is the 32-byte hash) */
} mh_replicated_entry;

typedef struct mh_replicate_batch {
    uint64_t n;              /* exported txs, in the order they are to be applied */
    const uint8_t *txs;      /* the ExportTx byte strings back to back; host memory, pinned or pageable */
    const uint64_t *tx_off;  /* n + 1 */
    uint32_t max_entries, max_key_len, max_value_len; /* the store's options */
    uint32_t flags;
    uint8_t prev_alh[32];    /* the follower's inmemPrecommittedAlh (SHA256(nil) on an empty store, immustore.go:464) */
} mh_replicate_batch;

int mh_replicate_tx_batch(mh_ahtree *t, const mh_replicate_batch *b,
                          int32_t *status /*n*/, uint64_t *accepted,
                          mh_tx_header *hdrs /*n, nullable*/, uint8_t *md_blob /*n*MH_MAX_TX_METADATA_LEN, nullable*/,
                          uint8_t *alh /*n*32, nullable*/,
                          uint64_t *ent_off /*n+1, nullable*/, mh_replicated_entry *ents, uint64_t ents_cap,
                          uint8_t *hvals /*ents_cap*32, nullable*/);

/* Group commit of single transactions (the concurrent committers of
 * precommit, immustore.go:1620-1632: each hashes its own tx before taking the
 * store lock at :1689, up to MaxConcurrency = 30 at once, options.go:35).
 * mh_commit_queue_submit hashes ONE transaction -- hVal per entry
 * (immustore.go:1624-1629), entry digests and the htree (tx.go:332-355) --
 * and blocks until its results are ready; a worker thread coalesces the
 * transactions submitted within wait_us (or max_txs of them) into one
 * mh_precommit_batch.  Arguments of submit are those of one tx of
 * mh_precommit_batch (offsets index the arrays directly; n + 1 of each);
 * expect_eh (32 bytes, may be NULL) is ReplicateTx's Eh (immustore.go:1649-1654).
 * Returns the tx's status (MH_OK, MH_ERR_MAX_WIDTH_EXCEEDED,
 * MH_ERR_METADATA_UNSUPPORTED, MH_ERR_ILLEGAL_ARGUMENTS for an Eh mismatch)
 * or an error of the batch.  Thread-safe: call submit from any number of
 * threads. */
typedef struct mh_commit_queue mh_commit_queue;
int mh_commit_queue_new(mh_ctx *ctx, int version, uint64_t max_width, uint32_t max_txs,
                        uint32_t wait_us, mh_commit_queue **out);
int mh_commit_queue_free(mh_commit_queue *q);
int mh_commit_queue_submit(mh_commit_queue *q, uint64_t n, const uint8_t *keys,
                           const uint64_t *key_off, const uint8_t *md, const uint64_t *md_off,
                           const uint8_t *vals, const uint64_t *val_off,
                           const uint8_t *hval_override, const uint8_t *use_override,
                           const uint8_t *expect_eh, uint8_t *hvals_out, uint8_t *eh_out);
/* batches run and transactions hashed so far */
int mh_commit_queue_stats(mh_commit_queue *q, uint64_t *batches, uint64_t *txs);

/* ------------------------------------------------------------ multi-GPU
 * one process (a cgo caller) driving K devices, one mh_ctx
 * (HIP stream) per device, an RCCL clique over them (ncclCommInitAll; RCCL is
 * loaded on first use, MH_ERR_COLLECTIVE if it is missing).  The htree leaves
 * are cut into power-of-two aligned shards of S entries (mh_multi_shard_plan:
 * S = next power of two >= ceil(n / K), shard g = [gS, min((g+1)S, n)),
 * G = ceil(n / S) <= K shards); device g builds its shard's subtree with every
 * level (exactly the global levels 0..log2 S of that range, htree.go:85-110),
 * the G subtree roots are all-gathered over RCCL (32 bytes per device) and the
 * top ceil(log2 G) levels are reduced over them.  A device may be listed more
 * than once (more shards than devices); the roots are then gathered with
 * device-to-device copies instead of RCCL. */
typedef struct mh_multi mh_multi;
int mh_multi_create(int ndev, const int *devices, mh_multi **out);
int mh_multi_destroy(mh_multi *m);
int mh_multi_size(mh_multi *m, int *ndev);
/* the context of device d (for mh_dev_alloc / fills / copies on that device) */
mh_ctx *mh_multi_ctx(mh_multi *m, int d);
int mh_multi_synchronize(mh_multi *m);
int mh_multi_shard_plan(uint64_t n, int ndev, uint64_t *shard, uint64_t *nshards);
/* Tx.BuildHashTree over n fixed-shape entries (value hash loop
 * immustore.go:1620-1630 + tx.go:332-355 + htree.go:68-113) across the K
 * devices, HOST memory in and out (as mh_htree_build_entries with fixed
 * strides): hvals_out (n x 32, may be NULL), levels_out (the flat level-major
 * layout, mh_htree_levels_len(n) x 32, may be NULL), root. */
int mh_multi_htree_build_entries_fixed(mh_multi *m, int version, uint64_t n, const uint8_t *keys,
                                       uint32_t key_len, const uint8_t *vals, uint32_t val_len,
                                       uint8_t *hvals_out, uint8_t *levels_out, uint8_t root[32]);
/* The general (CSR) form of the same build (mh_htree_build_entries' inputs:
 * ragged keys / KV metadata / values, IsValueTruncated overrides), host
 * memory in and out: each shard's byte ranges and offsets go to its device. */
int mh_multi_htree_build_entries(mh_multi *m, int version, uint64_t n, const uint8_t *keys,
                                 const uint64_t *key_off, const uint8_t *md,
                                 const uint64_t *md_off, const uint8_t *vals,
                                 const uint64_t *val_off, const uint8_t *hval_override,
                                 const uint8_t *use_override, uint8_t *hvals_out,
                                 uint8_t *levels_out, uint8_t root[32]);
/* Device-resident variant (BASELINE configs[3]): device d holds entries
 * [d n_per_dev, (d+1) n_per_dev) of a K * n_per_dev-entry tree (n_per_dev a
 * power of two when K > 1) in keys[d] / vals[d]; it writes its subtree's levels
 * to levels[d] (mh_htree_levels_len(n_per_dev) nodes), hVals to hvals_out[d]
 * (array may be NULL), the top levels over the K gathered roots to
 * top_levels[d] (mh_htree_levels_len(K) nodes) and the GLOBAL root to root[d]
 * -- every device ends with the same top levels and root.  Asynchronous on the
 * devices' context streams (mh_multi_synchronize). */
int mh_multi_dev_htree_build_entries_fixed(mh_multi *m, int version, uint64_t n_per_dev,
                                           const uint8_t *const *keys, uint32_t key_len,
                                           const uint8_t *const *vals, uint32_t val_len,
                                           uint8_t *const *hvals_out, uint8_t *const *levels,
                                           uint8_t *const *top_levels, uint8_t *const *root);
/* ahtree AppendBatch of `total` payloads (plen bytes each) onto a tree of
 * size n0 across the K devices (ahtree.go:246-373; BASELINE configs[2] at
 * scale, and the replay of syncBinaryLinking, immustore.go:1198-1232, which
 * resumes at aht.Size()+1 on every open, :686-693).  The batch
 * (n0, n0 + total] is cut at multiples of S = 2^k (S <= total / 8K) into
 * G <= K nearly equal ranges (mh_ahtree_range_plan); device d appends range
 * d and keeps ONLY that range's digests: dLog indices
 * [mh_ahtree_nodes_upto(b[d]), mh_ahtree_nodes_upto(b[d+1])).  Every node a
 * range reads outside itself is a peak of its left end (the perfect subtree
 * of a set bit of b[d]); the old tree's peaks come from the caller and the
 * others are built on the devices from the ranges' level-k piece roots,
 * all-gathered over RCCL (32 B per piece, tens of pieces per device).
 * peaks: the popcount(n0) peaks of the old tree, lowest level first, in host
 * memory -- peak l is node(n0 with the bits below l cleared, l) =
 * dLog[mh_ahtree_node_index(n0 & ~(2^l - 1), l)] for every set bit l of n0
 * (NULL when n0 == 0; mh_dev_ahtree_peaks reads them from a resident dLog).
 * Device variant: payloads[d] holds range d's b[d+1] - b[d] payloads and
 * dlog[d] the room for its digests (16-byte aligned); roots_out (may be NULL,
 * or hold NULL entries) receives RootAt after each append of range d.
 * Ranges d >= G are unused.  Asynchronous on the devices' context streams.
 * Host variant: payloads and dlog_out (the NEW digests only,
 * (nodesUpto(n0 + total) - nodesUpto(n0)) x 32 bytes = what Append writes to
 * tree/NNNNNNNN.sha, may be NULL) in host memory, root = RootAt(n0 + total);
 * total == 0 -> MH_ERR_UNEXISTENT_DATA for an empty tree (ahtree.go:727-745),
 * MH_ERR_ILLEGAL_ARGUMENTS otherwise. */
int mh_multi_dev_ahtree_append_batch(mh_multi *m, uint64_t n0, const uint8_t *peaks,
                                     uint64_t total, const uint8_t *const *payloads, uint32_t plen,
                                     uint8_t *const *dlog, uint8_t *const *roots_out);
int mh_multi_ahtree_append_batch(mh_multi *m, uint64_t n0, const uint8_t *peaks,
                                 const uint8_t *payloads, uint64_t total, uint32_t plen,
                                 uint8_t *dlog_out, uint8_t root[32]);
/* The range plan of those calls (host only): bounds[0..*nranges] (room for
 * ndev + 1 values; bounds[0] = n0, bounds[*nranges] = n0 + total, the others
 * multiples of 2^*shard_bits), range d = (bounds[d], bounds[d+1]] on device d.
 * ndev <= 64. */
int mh_ahtree_range_plan(uint64_t n0, uint64_t total, int ndev, int *shard_bits, uint64_t *bounds,
                         int *nranges);
/* The same ranged append with ONE PROCESS PER DEVICE (torch.distributed /
 * any launcher whose ranks exchange bytes themselves): rank r of `world`
 * appends range r of mh_ahtree_range_plan(n0, total, world) -- the same
 * digests mh_multi_dev_ahtree_append_batch leaves on device r -- in two calls
 * around one all-gather the caller runs (ahtree.go:246-373):
 *  1. mh_dev_ahtree_range_local: leaves + perfect nodes of the range and its
 *     pieces' level-k roots into `send` (device, send_bytes);
 *  2. the caller all-gathers send_bytes from every rank, in rank order, into
 *     `recv` (device, world x send_bytes; skipped when the plan has one range);
 *  3. mh_dev_ahtree_range_finish: the piece tree above level k, the rank's
 *     frontier and its spines; roots_out (may be NULL) gets RootAt after each
 *     append of the range.
 * send_bytes / work_bytes from mh_ahtree_range_sizes; `work` (device,
 * 16-byte aligned) is this rank's scratch and must be kept between the two
 * calls; payloads / dlog_range as for the device variant above (range r's
 * payloads, room for its new digests).  peaks (host) on EVERY rank when
 * n0 > 0.  A rank past the plan's ranges (r >= nranges) does nothing but
 * still joins the all-gather.  Asynchronous on the context stream. */
int mh_ahtree_range_sizes(uint64_t n0, uint64_t total, int ndev, uint64_t *send_bytes,
                          uint64_t *work_bytes);
int mh_dev_ahtree_range_local(mh_ctx *ctx, uint64_t n0, const uint8_t *peaks, uint64_t total,
                              int world, int rank, const uint8_t *payloads, uint32_t plen,
                              uint8_t *dlog_range, uint8_t *work, uint8_t *send);
int mh_dev_ahtree_range_finish(mh_ctx *ctx, uint64_t n0, const uint8_t *peaks, uint64_t total,
                               int world, int rank, const uint8_t *recv, uint8_t *dlog_range,
                               uint8_t *work, uint8_t *roots_out);
/* The PCIe-bound batch paths over the K devices: the batch is cut into K
 * contiguous parts -- by index for proofs, at record boundaries (nearly equal
 * bytes) for a tx log -- and part d runs the single-context call on device d
 * from its own thread, over its own PCIe link; outputs land side by side,
 * byte-equal to one single-context call over the whole batch (K = 1 IS that
 * call).  The single-context call's argument check runs on the whole batch
 * before any part starts, so MH_ERR_ILLEGAL_ARGUMENTS comes back with no
 * output byte written, and the limits a call puts on n (the wire and answer
 * calls: n <= 2^31 - 1 and 2 n metadata slots within 32 bits) hold for the
 * whole batch, not per part.  Arguments, statuses and outputs as mh_htree_verify_inclusion_batch
 * (htree.go:166-195), mh_verify_dual_proof_v2_batch (verification.go:303-372)
 * and mh_txlog_validate (tx.go:388-630; the replay of
 * immustore.go:1198-1223 and the indexer's readTx, indexer.go:570: every
 * record carries its prevAlh, so the parts are independent).  For the tx log
 * the host hop finds the record boundaries once first (mh_txlog_scan's status
 * is the call's); a header's md_off stays relative to buf. */
int mh_multi_htree_verify_inclusion_batch(mh_multi *m, uint64_t n, const uint64_t *leaf,
                                          const uint64_t *width, const uint64_t *term_off,
                                          const uint8_t *terms, const uint8_t *digests,
                                          const uint8_t *roots, uint8_t *ok);
int mh_multi_verify_dual_proof_v2_batch(mh_multi *m, uint64_t n, const mh_tx_header *src_hdr,
                                        const mh_tx_header *tgt_hdr, const uint8_t *md_blob,
                                        uint64_t md_blob_len, const uint64_t *incl_off,
                                        const uint8_t *incl_terms, const uint64_t *cons_off,
                                        const uint8_t *cons_terms, const uint64_t *src,
                                        const uint64_t *tgt, const uint8_t *src_alh,
                                        const uint8_t *tgt_alh, int32_t *status);
int mh_multi_txlog_validate(mh_multi *m, const uint8_t *buf, uint64_t len, uint32_t max_entries,
                            uint32_t max_key_len, uint64_t max_txs, uint64_t *ntx,
                            uint64_t *consumed, mh_tx_header *hdrs, uint8_t *alh,
                            int32_t *status);
/* More PCIe-bound batches over the K devices, each part on its own link, cut
 * into parts of nearly equal input bytes: readValueAt's hVal check
 * (immustore.go:3183-3240; *ncorrupted summed over the parts), the fused
 * DualProofV2 wire verify (database_protoconv.go:226-262 +
 * verification.go:303-372), and precommit's hashing (immustore.go:1620-1632;
 * whole transactions per part, each device with its own commit pipe made on
 * first use).  Arguments and outputs as mh_verify_values_batch,
 * mh_verify_dual_proof_v2_pb_batch and mh_precommit_batch. */
int mh_multi_verify_values_batch(mh_multi *m, uint64_t n, const uint8_t *vals, const uint64_t *off,
                                 const uint64_t *vlen, const uint8_t *hvals, int32_t *status,
                                 uint64_t *ncorrupted);
int mh_multi_verify_dual_proof_v2_pb_batch(mh_multi *m, uint64_t n, const uint8_t *msgs,
                                           const uint64_t *msg_off, const uint64_t *src,
                                           const uint64_t *tgt, const uint8_t *src_alh,
                                           const uint8_t *tgt_alh, int32_t *status);
/* The fused DualProof (v1) wire verify over the devices, split by message
 * bytes like the V2 form; arguments and outputs as
 * mh_verify_dual_proof_pb_batch (context 0 alone when K == 1 or n < K). */
int mh_multi_verify_dual_proof_pb_batch(mh_multi *m, uint64_t n, const uint8_t *msgs,
                                        const uint64_t *msg_off, const uint64_t *src,
                                        const uint64_t *tgt, const uint8_t *src_alh,
                                        const uint8_t *tgt_alh, int32_t *status, uint8_t *ok);
/* VerifyDocument's hashing part (verification.go:37-196) over the devices:
 * parts of nearly equal entries + document bytes, as mh_verify_document_batch. */
int mh_multi_verify_document_batch(mh_multi *m, const mh_document_batch *batch, int32_t *status,
                                   uint8_t *target_alh_out);
int mh_multi_precommit_batch(mh_multi *m, int version, uint64_t max_width, uint64_t ntx,
                             const uint64_t *tx_off, const uint8_t *keys, const uint64_t *key_off,
                             const uint8_t *md, const uint64_t *md_off, const uint8_t *vals,
                             const uint64_t *val_off, const uint8_t *hval_override,
                             const uint8_t *use_override, const uint8_t *expect_eh,
                             uint8_t *hvals_out, uint8_t *eh_out, int32_t *status);

/* ------------------------------------------------------------ wire formats
 * proofs as the protobuf messages the gRPC server sends
 * (pkg/api/schema/schema.proto, Go conversion pkg/api/schema/database_protoconv.go,
 * marshalled as protobuf-go does: field-number order, proto3 zero values
 * omitted), generated AND encoded on the device from the resident tree, so a
 * batch of VerifiableGet / VerifiableTxByIdV2 answers is one device->host
 * copy of ready-to-send bytes.  Message p is out[off[p] .. off[p+1]) (off has
 * n + 1 entries, off[0] = 0); a message that fails is empty and status[p]
 * holds the Go error.  If out_cap < off[n] nothing is written to out, off and
 * status are filled and MH_ERR_BUFFER_TOO_SMALL is returned (call again with
 * a buffer of off[n] bytes). */

/* The other direction, on the device: DualProofV2FromProto
 * (database_protoconv.go:226-262, TxHeaderFromProto, TxMetadataFromProto,
 * DigestsFromProto :293-305) over n DualProofV2 messages, message p =
 * msgs[msg_off[p] .. msg_off[p+1]), read as protobuf-go's Unmarshal does
 * (any field order, last scalar wins, repeated headers merged, unknown and
 * mistyped fields skipped).  Outputs are the arguments of
 * mh_verify_dual_proof_v2_batch: src_hdr / tgt_hdr (n each), md_blob (room for
 * 2n x MH_MAX_TX_METADATA_LEN bytes; the canonical TxMetadata.Bytes() of
 * every header packed in message order, source before target, located by each
 * header's md_off / md_len), incl_off / cons_off (n + 1 each) and the
 * terms (32 bytes each, DigestFromProto: shorter terms zero-padded, longer
 * truncated).  status[p]: MH_OK, MH_ERR_CORRUPTED_DATA (not a valid encoding;
 * no terms), MH_ERR_ILLEGAL_ARGUMENTS (a header missing: Go dereferences the
 * nil header).  If incl_cap / cons_cap (terms) are below incl_off[n] /
 * cons_off[n], only the offsets and statuses are written and
 * MH_ERR_BUFFER_TOO_SMALL is returned.  n <= 8 013 008 (32-bit md_off). */
int mh_dual_proof_v2_pb_decode_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                     const uint64_t *msg_off, mh_tx_header *src_hdr,
                                     mh_tx_header *tgt_hdr, uint8_t *md_blob, uint64_t *incl_off,
                                     uint8_t *incl_terms, uint64_t incl_cap, uint64_t *cons_off,
                                     uint8_t *cons_terms, uint64_t cons_cap, int32_t *status);
/* InclusionProofFromProto (database_protoconv.go:123-129) over n InclusionProof
 * messages (msgs / msg_off as above), on the device -> the arguments of
 * mh_htree_verify_inclusion_batch: leaf[p] / width[p] (the wire's int32 as a
 * Go int: sign-extended, stored as its 64-bit pattern; htree verification
 * takes them with Go's signed arithmetic), term_off (n + 1) and the terms (32
 * bytes each, DigestFromProto).  status[p]: MH_OK or MH_ERR_CORRUPTED_DATA
 * (no terms, leaf = width = 0).  term_cap < term_off[n]: offsets and statuses
 * only, MH_ERR_BUFFER_TOO_SMALL. */
/* What a client auditing many VerifiableTxV2 answers does per answer --
 * DualProofV2FromProto then store.VerifyDualProofV2 (verification.go:303-372)
 * -- for n DualProofV2 messages in one call, entirely on the device: the
 * messages go up once, only the statuses come back.  status[p] is
 * mh_dual_proof_v2_pb_decode_batch's failure for message p (CORRUPTED_DATA,
 * ILLEGAL_ARGUMENTS) or else mh_verify_dual_proof_v2_batch's verdict on the
 * decoded proof with (src[p], tgt[p], src_alh[32 p], tgt_alh[32 p]), except
 * that a version-0 header's metadata is ignored, as Go's innerHash ignores it
 * (tx.go:258-263; mh_verify_dual_proof_v2_batch rejects a v0 header with
 * md_len > 0, a combination the tx log cannot hold but a message can). */
int mh_verify_dual_proof_v2_pb_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                     const uint64_t *msg_off, const uint64_t *src,
                                     const uint64_t *tgt, const uint8_t *src_alh,
                                     const uint8_t *tgt_alh, int32_t *status);
/* The same for DualProof (v1), the proof VerifiableGet / VerifiableSet /
 * VerifiableTxById answer with: DualProofFromProto then store.VerifyDualProof
 * (verification.go:127-235) for n messages in one device pass -- message p =
 * msgs[msg_off[p] .. msg_off[p+1]) (host memory, pageable or pinned; msg_off[0]
 * need not be 0) goes up once, in chunks of MH_PB_CHUNK_MIB MiB (default 128,
 * the variable the V2 call reads), and only n statuses and n verdict bytes
 * come back.  Consecutive chunks are decoded and verified together until
 * their bytes reach MH_PB_GROUP_RATIO (default 16384; 0: every chunk alone)
 * times their longest message: one lane reads one message, so a launch lasts
 * as long as its longest message however few it holds.  status[p] is exactly mh_dual_proof_pb_decode_batch's status for
 * message p: MH_OK, MH_ERR_CORRUPTED_DATA, or MH_ERR_ILLEGAL_ARGUMENTS (a
 * header or the linear proof missing).  ok[p] is 1 iff status[p] == MH_OK and
 * Go's VerifyDualProof(proof, src[p], tgt[p], src_alh[32 p], tgt_alh[32 p])
 * returns true on the decoded proof.  Both this call and
 * mh_verify_dual_proof_batch run one device verifier (dual_proof_v1_core,
 * csrc/capi_tx.hip) and give one verdict, with a single difference: here a
 * version-0 header's metadata is ignored, as Go's innerHash ignores it
 * (tx.go:258-263), while the array call refuses such a header (ok = 0).  A
 * header version above 1 gives ok = 0 in both.  A message without LinearAdvanceProof is verified as Go verifies a
 * nil one (true only where verification.go:90-97 needs none): nothing is
 * fetched, FillMissingLinearAdvanceProof is the caller's business.  n == 0
 * returns MH_OK; null pointers, a non-monotonic msg_off and n above the limits
 * of the V2 call (n <= 8 013 008) return MH_ERR_ILLEGAL_ARGUMENTS. */
int mh_verify_dual_proof_pb_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                  const uint64_t *msg_off, const uint64_t *src,
                                  const uint64_t *tgt, const uint8_t *src_alh,
                                  const uint8_t *tgt_alh, int32_t *status, uint8_t *ok);

/* ------------------------------------------- whole VerifiableGet answers
 * What pkg/client does with every VerifiableGet answer (verifiedGet,
 * pkg/client/client.go:1119-1234) before the state signature check, for n
 * answers in one device pass: proto.Unmarshal into schema.VerifiableEntry,
 * EncodeEntrySpec / EncodeReference (pkg/database/meta.go:54-89) with
 * KVMetadataFromProto (database_protoconv.go:97-113), the value hash and
 * EntrySpecDigest_v0 / _v1 (embedded/store/verification.go:244-302),
 * htree.VerifyInclusion against the Eh of the proof header that is the
 * entry's transaction, the choice of source and target from the client's
 * state, VerifyDualProof (verification.go:127-235) and the new state.
 * FillMissingLinearAdvanceProof (a network fetch) stays with the caller, as
 * for mh_verify_dual_proof_pb_batch; SQL VerifyRow is not covered (the
 * verified writes and VerifiedTxByID: mh_verify_verifiable_tx_pb_batch).
 *
 * Answer p is the VerifiableEntry message msgs[msg_off[p] .. msg_off[p+1])
 * for the request key keys[key_off[p] .. key_off[p+1]) (kReq.Key, without
 * the 0x00 prefix), kReq.AtTx at_tx[p], and the client's state (state_tx[p],
 * state_alh[32 p]); state_tx 0 means no state yet.  All host memory, pageable
 * or pinned; msg_off[0] / key_off[0] need not be 0.  Everything goes up once,
 * through the chunks and groups of mh_verify_dual_proof_pb_batch
 * (MH_PB_CHUNK_MIB, MH_PB_GROUP_RATIO); only status, ok, new_tx and new_alh
 * come back.
 *
 * status[p], first match, in Go's order:
 *   MH_ERR_CORRUPTED_DATA          proto.Unmarshal would fail
 *   MH_ERR_ILLEGAL_ARGUMENTS       verifiableTx, its tx, or the tx's header
 *                                  absent (nil dereference, client.go:1145)
 *   MH_ERR_UNSUPPORTED_TX_VERSION  int(Tx.Header.Version) not 0 or 1
 *   MH_ERR_ILLEGAL_ARGUMENTS       inclusionProof, verifiableTx.dualProof, one
 *                                  of its headers or its linearProof, or
 *                                  entry absent
 *   MH_OK                          otherwise; the verdict is ok[p]
 * MH_ERR_CORRUPTED_DATA means what protobuf-go means: the whole closure of
 * VerifiableEntry is validated (Entry, Reference, KVMetadata, Expiration,
 * VerifiableTx, Tx, TxHeader, TxMetadata, TxEntry, ZEntry, Signature,
 * DualProof, LinearProof, LinearAdvanceProof, InclusionProof), the parts the
 * verifier never reads (Tx.entries, Tx.kvEntries, Tx.zEntries, signature)
 * included.  Merge rule: fields in any order; of a scalar or bytes field the
 * last occurrence wins; occurrences of an embedded message are merged
 * (entry, referencedBy, the metadata messages and inclusionProof are walked
 * occurrence by occurrence, inclusion terms appended); unknown and mistyped
 * fields and groups are skipped but must be well formed; a 10-byte varint
 * whose last byte is above 1 is an error.  When verifiableTx.dualProof occurs
 * more than once the merged DualProof is the parse of the occurrences'
 * concatenation, in order.
 *
 * ok[p] = 1 iff status[p] == MH_OK and verifiedGet returns no error before
 * the signature check.  With S = state_tx[p]: vTx = at_tx ? at_tx : (the
 * reference's tx if referencedBy is present, else entry.tx); the EntrySpec is
 * key 0x00 || kReq.Key, metadata and value 0x00 || entry.value of the entry,
 * or, for a reference, the reference's metadata and value 0x01 ||
 * BE64(ref.atTx) || 0x00 || entry.key; KVMetadata bytes 0x00 if deleted,
 * 0x01 || BE64(expiresAt) if the expiration message is present (an empty one
 * counts), 0x02 if nonIndexable; the digest is EntrySpecDigest_v1, or _v0
 * (metadata ignored, not refused) for a version-0 tx header.  If S <= vTx:
 * eh = the target header's EH, (src, srcAlh, tgt, tgtAlh) = (S, state_alh,
 * vTx, TargetTxHeader.Alh()); otherwise eh = the source header's EH and
 * (vTx, SourceTxHeader.Alh(), S, state_alh).  htree.VerifyInclusion(proof,
 * digest, eh) must hold (leaf / width the wire's int32 sign-extended, Go's
 * signed walk, as mh_htree_verify_inclusion_batch), and, if S > 0,
 * VerifyDualProof(proof, src, tgt, srcAlh, tgtAlh) as
 * mh_verify_dual_proof_pb_batch runs it (v0 header metadata ignored, a header
 * version above 1 gives ok = 0, a missing LinearAdvanceProof verified as
 * nil).  new_tx[p] = tgt and new_alh[32 p] = tgtAlh when ok[p] = 1, zeros
 * otherwise.  n == 0 returns MH_OK; null pointers, a non-monotonic msg_off /
 * key_off and n above the V2 call's limit return MH_ERR_ILLEGAL_ARGUMENTS. */
typedef struct mh_verified_get_batch {
    uint64_t n;
    const uint8_t *msgs;
    const uint64_t *msg_off;  /* n + 1 */
    const uint8_t *keys;
    const uint64_t *key_off;  /* n + 1 */
    const uint64_t *at_tx;    /* n: kReq.AtTx */
    const uint64_t *state_tx; /* n: state.TxId (0: no state yet) */
    const uint8_t *state_alh; /* n x 32: DigestFromProto(state.TxHash) */
} mh_verified_get_batch;
int mh_verify_verifiable_entry_pb_batch(mh_ctx *ctx, const mh_verified_get_batch *b,
                                        int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                        uint8_t *new_alh);
/* The same over the clique's devices, split by message bytes as
 * mh_multi_verify_dual_proof_pb_batch (context 0 alone when K == 1 or n < K). */
int mh_multi_verify_verifiable_entry_pb_batch(mh_multi *m, const mh_verified_get_batch *b,
                                              int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                              uint8_t *new_alh);
/* The envelope pass of the call above on its own (proto.Unmarshal into
 * schema.VerifiableEntry, client.go:1140-1175's reads of it), for composition
 * with mh_htree_verify_inclusion_batch and mh_verify_dual_proof_pb_batch:
 * status[p] as above; info[p] (all zero unless status[p] == MH_OK): entry.tx,
 * the reference's tx / atTx and has_ref, where entry.key / entry.value lie in
 * msgs (index of the first byte, length; the last occurrence), the
 * KVMetadata.Bytes() that count (the reference's if has_ref), the tx header's
 * version, the inclusion proof's leaf / width (int32 sign-extended, 64-bit
 * pattern); the inclusion terms (32 bytes each, DigestFromProto) at
 * incl_terms[32 incl_off[p] ..); the merged DualProof message at
 * dual_bytes[dual_off[p] .. dual_off[p+1]), ready for
 * mh_verify_dual_proof_pb_batch.  incl_cap (terms) or dual_cap (bytes) short:
 * the offsets, statuses and info are written and MH_ERR_BUFFER_TOO_SMALL is
 * returned. */
typedef struct mh_verifiable_entry_info {
    uint64_t entry_tx, ref_tx, ref_at_tx;
    uint64_t key_pos, key_len, value_pos, value_len;
    uint64_t leaf, width;
    int32_t tx_version;
    uint8_t has_ref;
    uint8_t md_len; /* <= MH_MAX_KV_METADATA_LEN */
    uint8_t md[MH_MAX_KV_METADATA_LEN];
    uint8_t pad_[7];
} mh_verifiable_entry_info; /* 96 bytes */
typedef struct mh_verifiable_entry_decoded {
    mh_verifiable_entry_info *info; /* n */
    uint64_t *incl_off;             /* n + 1 */
    uint8_t *incl_terms;
    uint64_t incl_cap;
    uint64_t *dual_off;             /* n + 1 */
    uint8_t *dual_bytes;
    uint64_t dual_cap;
} mh_verifiable_entry_decoded;
int mh_verifiable_entry_pb_decode_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                        const uint64_t *msg_off,
                                        mh_verifiable_entry_decoded *out, int32_t *status);

/* ------------------------------------------- whole VerifiableTx answers
 * What pkg/client does with the schema.VerifiableTx answer of a verified
 * write or of VerifiedTxByID, up to but not including the signature check and
 * SetState, for n answers in one device pass:
 *   MH_VTX_SET        VerifiedSet             pkg/client/client.go:1337-1391
 *   MH_VTX_SET_ALL    streamVerifiedSet       pkg/client/streams.go:205-260
 *   MH_VTX_REFERENCE  VerifiedSetReferenceAt  client.go:1716-1770
 *   MH_VTX_ZADD       VerifiedZAddAt          client.go:1882-1940
 *   MH_VTX_TX_BY_ID   VerifiedTxByID          client.go:1554-1583 (and the
 *                     auditor, pkg/client/auditor/auditor.go:294-312)
 * A write is verified against the transaction rebuilt from the wire:
 * TxFromProto (pkg/api/schema/database_protoconv.go:69-95) builds the hash
 * tree of the TxEntry records, overwrites the header's Eh with its root, the
 * entries the client sent are checked against that tree, the rebuilt Eh
 * against the DualProof's target header, and the new state's Alh comes from
 * the rebuilt header.  SQL VerifyRow is not covered.
 *
 * Answer p is msgs[msg_off[p] .. msg_off[p+1]) of kind[p]; it owns the specs
 * spec_off[p] .. spec_off[p+1]) (K = their number), spec t with key
 * keys[key_off[t] .. key_off[t+1]) and value vals[val_off[t] .. val_off[t+1]),
 * key_off / val_off indexed by the spec's absolute number:
 *   SET        K = 1   raw key, raw value
 *   REFERENCE  K = 1   raw key, the referenced key; at_tx[p] = atTx
 *   ZADD       K = 1   the finished WrapZAddReferenceAt key
 *                      (pkg/database/meta.go:98-117), taken verbatim; no value
 *   SET_ALL    K >= 1  raw key, raw value
 *   TX_BY_ID   K = 0   at_tx[p] = the requested tx
 * The prefixes of EncodeKey / EncodeEntrySpec / EncodeReference
 * (meta.go:50-89) are added on the device.  state_tx[p] / state_alh[32 p]: the
 * client's state, tx 0 = none yet.  All host memory, pageable or pinned; no
 * *_off[0] need be 0.  Everything goes up once through the chunks and groups
 * of mh_verify_dual_proof_pb_batch (MH_PB_CHUNK_MIB, MH_PB_GROUP_RATIO), chunk
 * 0 carrying the request arrays; only status, ok, new_tx, new_alh and eh_out
 * come back.  n == 0 returns MH_OK; a null pointer, a non-monotonic offset
 * array, a kind outside the enum, a K that breaks the table and n above the
 * VerifiableGet call's limit return MH_ERR_ILLEGAL_ARGUMENTS.
 *
 * proto.Unmarshal into schema.VerifiableTx follows the merge rules of the
 * VerifiableGet call: fields in any order; the last scalar or bytes
 * occurrence wins; embedded messages merge; Tx.entries occurrences append in
 * wire order across merged tx occurrences; a dualProof that occurs more than
 * once is the parse of the concatenation; unknown and mistyped fields and
 * groups are skipped but must be well formed; a 10-byte varint whose last
 * byte is above 1 is an error; the whole closure is validated, kvEntries,
 * zEntries and signature included.
 *
 * status[p], first match; it depends on the structure alone, never on a hash
 * (S = state_tx[p]):
 *   1 MH_ERR_CORRUPTED_DATA          Unmarshal would fail
 *   2 write kinds: MH_ERR_ILLEGAL_ARGUMENTS when tx or tx.header is absent
 *     (the nil dereference of client.go:1337 / 1716 / 1882, streams.go:205)
 *   3 write kinds, the count rule: SET / SET_ALL need int32(header.nentries)
 *     == K and len(entries) == K, REFERENCE / ZADD header.nentries == 1.
 *     Failing it is MH_OK with ok = 0 (Go: ErrCorruptedData) and nothing
 *     below is looked at
 *   4 REFERENCE / ZADD without any entry: MH_ERR_ILLEGAL_ARGUMENTS
 *     (tx.Entries() slices past the end inside BuildHashTree)
 *   5 write kinds: int(header.version) not 0 or 1 gives
 *     MH_ERR_UNSUPPORTED_TX_VERSION (BuildHashTree's error is ignored by
 *     TxFromProto; EntrySpecDigestFor returns this one)
 *   6 MH_ERR_ILLEGAL_ARGUMENTS when a DualProof part Go would dereference is
 *     missing.  Write kinds: dualProof or its targetTxHeader; with S > 0 also
 *     sourceTxHeader or linearProof (DualProofFromProto runs only then).
 *     TX_BY_ID: dualProof, either header or linearProof (client.go:1554 runs
 *     it unconditionally); its tx is not looked at.  For a write kind Go
 *     reaches this dereference only after a passing inclusion check and
 *     returns ErrCorruptedData where that check fails; ok is 0 either way,
 *     and the status stays independent of hashes.
 *   7 MH_OK
 *
 * ok[p] of a write kind = 1 iff status[p] == MH_OK, the count rule held and
 * all of this holds.  Entry i < K of Tx.entries gives key_i, hv_i =
 * DigestFromProto(hValue) and md_i = KVMetadataFromProto(metadata).Bytes()
 * (the byte rules of the VerifiableGet call; no metadata: empty).
 *   TxEntryDigest (embedded/store/tx.go:690-731): version 1 d_i = SHA256(
 *     BE16(len md_i) || md_i || BE16(len key_i mod 2^16) || key_i || hv_i),
 *     version 0 d_i = SHA256(key_i || hv_i); version 0 with a non-empty md_i
 *     gives ok = 0 (ErrMetadataUnsupported leaves the tree unbuilt, tx.Proof
 *     fails; eh_out stays zero).
 *   Eh' = the htree root over d_0 .. d_{K-1} (embedded/htree/htree.go:68-113);
 *     eh_out[32 p] = Eh' whenever it is built, zeros otherwise.
 *   Spec i: SET / SET_ALL key 0x00 || key, value 0x00 || value, metadata md_i
 *     by position i (tx.Entries()[i].Metadata(), client.go:1353,
 *     streams.go:224); REFERENCE key 0x00 || key, value 0x01 || BE64(at_tx)
 *     || 0x00 || value, no metadata; ZADD the key verbatim, the empty value
 *     (hVal = SHA256 of nothing), no metadata.  SET alone gives ok = 0 when
 *     md_0 has the deleted attribute (client.go:1355).  x_i =
 *     EntrySpecDigest_v0 / _v1 (embedded/store/verification.go:257-302; v0
 *     ignores metadata); j_i = the first j < K with key_j equal to the spec's
 *     key (Tx.IndexOf, tx.go:361-368), none: ok = 0; x_i == d_{j_i} is
 *     required, which is what VerifyInclusion of the tree's own proof for
 *     leaf j_i decides.
 *   Eh' == DigestFromProto(dualProof.targetTxHeader.eH).
 *   tgt = header.id, tgtAlh = Alh() of the tx header with Eh' in place of the
 *     wire's eH (TxMetadata as for the headers of
 *     mh_verify_dual_proof_pb_batch; version 0 drops it).  If S > 0:
 *     VerifyDualProof(proof, S, tgt, state_alh, tgtAlh) as that call runs it
 *     (a header version above 1 gives ok = 0, a missing LinearAdvanceProof is
 *     verified as nil).
 * ok[p] of TX_BY_ID (client.go:1554-1583), t = at_tx[p]: if S <= t (src,
 * srcAlh, tgt, tgtAlh) = (S, state_alh, t, Target.Alh()), else (t,
 * Source.Alh(), S, state_alh); with S > 0 the DualProof must verify, S == 0
 * gives ok = 1.
 * new_tx[p] / new_alh[32 p] = tgt / tgtAlh when ok[p] = 1, zeros otherwise. */
enum { MH_VTX_SET = 0, MH_VTX_SET_ALL = 1, MH_VTX_REFERENCE = 2, MH_VTX_ZADD = 3, MH_VTX_TX_BY_ID = 4 };
typedef struct mh_verified_tx_batch {
    uint64_t n;
    const uint8_t *msgs;
    const uint64_t *msg_off;  /* n + 1: VerifiableTx messages */
    const uint8_t *kind;      /* n: MH_VTX_* */
    const uint64_t *spec_off; /* n + 1: answer p owns specs spec_off[p] .. spec_off[p+1] */
    const uint8_t *keys;
    const uint64_t *key_off;  /* T + 1, T = total specs */
    const uint8_t *vals;
    const uint64_t *val_off;  /* T + 1 */
    const uint64_t *at_tx;    /* n: REFERENCE atTx; TX_BY_ID the requested tx; else ignored */
    const uint64_t *state_tx; /* n: state.TxId, 0 = no state yet */
    const uint8_t *state_alh; /* n x 32 */
} mh_verified_tx_batch;
int mh_verify_verifiable_tx_pb_batch(mh_ctx *ctx, const mh_verified_tx_batch *b, int32_t *status,
                                     uint8_t *ok, uint64_t *new_tx, uint8_t *new_alh,
                                     uint8_t *eh_out /* n x 32, may be NULL */);
/* The same over the clique's devices, split by message bytes as
 * mh_multi_verify_verifiable_entry_pb_batch (context 0 alone when K == 1 or
 * n < K, K the devices). */
int mh_multi_verify_verifiable_tx_pb_batch(mh_multi *m, const mh_verified_tx_batch *b,
                                           int32_t *status, uint8_t *ok, uint64_t *new_tx,
                                           uint8_t *new_alh, uint8_t *eh_out);

int mh_htree_inclusion_proof_pb_decode_batch(mh_ctx *ctx, uint64_t n, const uint8_t *msgs,
                                             const uint64_t *msg_off, uint64_t *leaf,
                                             uint64_t *width, uint64_t *term_off, uint8_t *terms,
                                             uint64_t term_cap, int32_t *status);

/* InclusionProof messages (schema.proto:534-540, InclusionProofToProto
 * database_protoconv.go:115-121) of (*HTree).InclusionProof(leaf[p])
 * (htree.go:121-164) over the tree's last build; status[p] MH_OK or
 * MH_ERR_ILLEGAL_ARGUMENTS (leaf >= width). */
int mh_htree_inclusion_proof_pb_batch(mh_htree *t, uint64_t n, const uint64_t *leaf, uint8_t *out,
                                      uint64_t out_cap, uint64_t *off, int32_t *status);
/* DualProofV2 messages (schema.proto:437-445; DualProofV2ToProto /
 * TxHeaderToProto / TxMetadataToProto database_protoconv.go:152-193) of
 * ImmuStore.DualProofV2(src[p], tgt[p]) (immustore.go:2356-2387: the ahtree
 * InclusionProof(src.ID, tgt.BlTxID) and ConsistencyProof(max(1,
 * src.BlTxID), tgt.BlTxID)) over t's dLog.  Header metadata (md_len bytes of
 * TxMetadata.Bytes() at md_blob + md_off) is re-encoded as the TxMetadata
 * message; md_len == 0 is Go's nil Metadata (a header read from the tx log,
 * tx.go:483-501).  status[p]: MH_OK, MH_ERR_ILLEGAL_ARGUMENTS (src.ID == 0),
 * MH_ERR_SOURCE_TX_NEWER, MH_ERR_UNEXPECTED_LINKING, MH_ERR_UNEXISTENT_DATA
 * (tgt.BlTxID beyond the tree), MH_ERR_CORRUPTED_DATA (metadata bytes). */
int mh_ahtree_dual_proof_v2_pb_batch(mh_ahtree *t, uint64_t n, const mh_tx_header *src,
                                     const mh_tx_header *tgt, const uint8_t *md_blob,
                                     uint64_t md_blob_len, uint8_t *out, uint64_t out_cap,
                                     uint64_t *off, int32_t *status);
/* Device variants (all pointers device memory, asynchronous, no allocation):
 * scratch = mh_pb_scratch_size(n) bytes; messages beyond out_cap get status
 * MH_ERR_BUFFER_TOO_SMALL.  phase: 1 = sizes + offsets only, 2 = write only
 * (after a phase-1 call with the same inputs), 3 = both.  off[0..n] and
 * status[0..n) are written whatever out_cap is (off[n] sizes a retry); of out
 * only the bytes [off[p], off[p+1]) of messages with status MH_OK, all below
 * out_cap: a refused message and everything from out_cap on keep the caller's
 * bytes.  scratch is unspecified inside its own mh_pb_scratch_size(n) bytes.
 * out: any alignment. */
uint64_t mh_pb_scratch_size(uint64_t n);
int mh_dev_htree_inclusion_proof_pb_batch(mh_ctx *ctx, int phase, const uint8_t *levels,
                                          uint64_t width, uint64_t n, const uint64_t *leaf,
                                          uint8_t *out, uint64_t out_cap, uint64_t *off,
                                          int32_t *status, void *scratch);
int mh_dev_dual_proof_v2_pb_batch(mh_ctx *ctx, int phase, const uint8_t *dlog, uint64_t size,
                                  uint64_t n, const mh_tx_header *src, const mh_tx_header *tgt,
                                  const uint8_t *md_blob, uint8_t *out, uint64_t out_cap,
                                  uint64_t *off, int32_t *status, void *scratch);

/* DualProof (v1) messages (schema.proto:388-434; DualProofToProto,
 * LinearProofToProto, LinearAdvanceProofToProto database_protoconv.go:131-211)
 * of ImmuStore.DualProof(src[p], tgt[p]) with its LinearProof and
 * LinearAdvanceProof (immustore.go:2394-2562): the answer of VerifiableGet,
 * VerifiableSet, VerifiableTxById and the SQL / sorted-set variants
 * (pkg/database/database.go:805,881).  Replaces the per-proof Go walk over
 * the tree and the tx log plus the marshalling; same contract as
 * mh_ahtree_dual_proof_v2_pb_batch (block comment above).
 * The ahtree parts -- InclusionProof(src.ID, tgt.BlTxID), ConsistencyProof(
 * src.BlTxID, tgt.BlTxID), InclusionProof(tgt.BlTxID, tgt.BlTxID) and the
 * LinearAdvanceProof's InclusionProof(k, tgt.BlTxID) (ahtree.go:525-597) --
 * are taken from t's dLog.  The linear parts are Alh / innerHash values of
 * whole txs, which the dLog does not hold (a leaf is SHA-256(0x00 || Alh)):
 * the caller passes a digest window, alh[32 k] and inner[32 k] of tx
 * first_tx + k for k < count, exactly the alh_out / inner_out of
 * mh_tx_alh_batch over those headers.  Nothing is hashed; the call gathers and
 * encodes.  A tx the proof needs outside the window is Go's ErrTxNotFound.
 * status[p], first match in Go's order: MH_ERR_ILLEGAL_ARGUMENTS (src.ID == 0:
 * the store holds no tx 0 and Go would walk the tree from leaf 0 -- a
 * deliberate narrowing, as for DualProofV2), MH_ERR_SOURCE_TX_NEWER (src.ID >
 * tgt.ID; or from LinearProof / LinearAdvanceProof, :2473, :2515),
 * MH_ERR_UNEXISTENT_DATA (tgt.BlTxID beyond the tree), MH_ERR_CORRUPTED_TX_DATA
 * (src.BlTxID > tgt.BlTxID, :2416), MH_ERR_TX_NOT_FOUND, MH_ERR_CORRUPTED_DATA
 * (metadata bytes).  Lengths are 64-bit: the linear parts have no cap but
 * out_cap.  TargetBlTxAlh is always written (32 zero bytes when tgt.BlTxID ==
 * 0: the Go field is a slice of an array); a nil LinearAdvanceProof is omitted;
 * nested InclusionProofs carry terms only. */
int mh_ahtree_dual_proof_pb_batch(mh_ahtree *t, uint64_t n, const mh_tx_header *src,
                                  const mh_tx_header *tgt, const uint8_t *md_blob,
                                  uint64_t md_blob_len, uint64_t first_tx, uint64_t count,
                                  const uint8_t *alh, const uint8_t *inner, uint8_t *out,
                                  uint64_t out_cap, uint64_t *off, int32_t *status);
/* Device variant of ImmuStore.DualProof + DualProofToProto (all pointers
 * device memory, asynchronous, no allocation; phase as above): dlog holds the
 * tree of `size` leaves, alh / inner (16-byte aligned) are the digest window
 * as mh_dev_tx_alh_batch writes it, scratch = mh_pb_dual_scratch_size(n)
 * bytes.  n < 2^31.  Phase 1 leaves the per-message part counts and
 * sub-message lengths in scratch: a phase-2 call needs that same scratch,
 * untouched, with the same off and status (else MH_ERR_ILLEGAL_STATE at
 * best).  A message that phase 2 marked MH_ERR_BUFFER_TOO_SMALL keeps that
 * status until phase 1 runs again. */
uint64_t mh_pb_dual_scratch_size(uint64_t n);
int mh_dev_dual_proof_pb_batch(mh_ctx *ctx, int phase, const uint8_t *dlog, uint64_t size,
                               uint64_t n, const mh_tx_header *src, const mh_tx_header *tgt,
                               const uint8_t *md_blob, uint64_t first_tx, uint64_t count,
                               const uint8_t *alh, const uint8_t *inner, uint8_t *out,
                               uint64_t out_cap, uint64_t *off, int32_t *status, void *scratch);

/* ------------------------------------------------------- whole answers, generated */
/* The server's half of the verified reads: whole schema.VerifiableTx
 * (schema.proto:499-508) and schema.VerifiableEntry (:523-532) messages of a
 * store whose tx log, commit log and ahtree are resident on the device, n
 * requests in one device pass.  MH_ANS_TX is the answer of db.VerifiableTxByID
 * with a nil EntriesSpec (pkg/database/database.go:1462-1528) and, once the
 * write is committed, of db.VerifiableSet (:767-814), VerifiableSetReference
 * (reference.go:118) and VerifiableZAdd (sorted_set.go:238):
 * VerifiableTx{tx: TxToProto(tx), dualProof}.  MH_ANS_ENTRY is the answer of
 * db.VerifiableGet (database.go:817-896): VerifiableEntry{entry, verifiableTx,
 * inclusionProof}; the index lookup and the value read stay with the caller,
 * who passes the marshalled schema.Entry, embedded verbatim as field 1 (an
 * empty range omits the field), and the key as the tx stores it
 * (EncodeKey(vKey)).  Request p yields out[off[p] .. off[p + 1]).
 *
 * Marshalling as protobuf-go: TxToProto / TxEntryToProto / KVMetadataToProto
 * (database_protoconv.go:27-67) -- key, hValue (always 32 bytes), vLen as
 * int32(vLen) (a stored length >= 2^31 is the 10-byte varint of the negative
 * value), metadata present iff the stored mdLen > 0 (deleted, expiration.
 * expiresAt = the stored seconds, nonIndexable); the header as the DualProof
 * writer encodes TxHeaderToProto (eH = the rebuilt Eh, nil metadata when mdLen
 * == 0); signature, kvEntries and zEntries never written; inclusionProof as
 * mh_htree_inclusion_proof_pb_batch; dualProof exactly the bytes of
 * mh_ahtree_dual_proof_pb_batch for the same (source, target) -- but the digest
 * window is not an argument: every tx the proof reads (tgt.BlTxID, [max(src.ID,
 * tgt.BlTxID), tgt.ID], [src.BlTxID + 1, min(src.ID, tgt.BlTxID)] when that
 * advance proof is not nil; immustore.go:2431, :2472-2510, :2514-2562) is read
 * from the resident log through the cLog and re-hashed, each distinct tx once
 * per call.
 *
 * status[p], first match in Go's order (N = s->ntx, S = prove_since[p], T =
 * tx[p]):
 *   MH_ERR_ILLEGAL_STATE      S > N (database.go:772, :822, :1467);
 *   MH_ERR_ILLEGAL_ARGUMENTS  T == 0 (ReadTx, immustore.go:2570);
 *   MH_ERR_TX_NOT_FOUND       T > N (immustore.go:3000);
 *   the record verdict of tx T, exactly the status mh_txlog_validate_clog gives
 *     that cLog entry; then, S > 0, the verdict of tx S (ReadTxHeader
 *     re-hashes, immustore.go:3062-3095; with S == 0 the root header is T's);
 *   MH_ERR_KEY_NOT_FOUND      ENTRY: no entry of T has the key (Tx.IndexOf,
 *     tx.go:361-368; the first equal key decides the leaf);
 *   the statuses of mh_ahtree_dual_proof_pb_batch for (src, tgt) = (root, T)
 *     when S <= T, else (T, root) (database.go:1506-1512), where a tx that
 *     cannot be read gives its record verdict at the place Go reaches it (the
 *     lowest failing tx of a range) and a tx of a range whose stored PrevAlh is
 *     not the Alh of the tx before it MH_ERR_CORRUPTED_TX_DATA
 *     (tx_reader.go:87-89);
 *   MH_ERR_BUFFER_TOO_SMALL   the message ends beyond out_cap (off[] is complete
 *     for all n all the same: off[n] sizes a retry);
 *   MH_OK.
 * A failed request writes no byte and leaves the other answers as they are.
 * n == 0 is MH_OK.  MH_ERR_ILLEGAL_ARGUMENTS before any device work: a null
 * pointer, key_off / entry_off running backwards, a kind outside the enum, a
 * TX request with key bytes, clog_entry_size not 12 or 44, n >= 2^31, ntx >=
 * 2^36, txlog or clog not on the ahtree's context's device or txlog's
 * allocation not 256 bytes longer than txlog_len; and, once the read set is
 * known, a batch that reads 2^31 or more distinct txs.  Locks: the tree's lock
 * first, then its context's, both held for the whole call (the order of
 * mh_replicate_tx_batch; all scratch of the call is the context's), so calls
 * on trees of one context run one after the other; t is not changed.  A cLog
 * entry that points outside the log is that record's status, never a fault.
 * Cost: every distinct tx read is re-hashed once per call.  The read set is
 * derived from the BlTxID fields the records store: as long as the
 * binary-linking lag of src and tgt in a sound store, up to the whole store
 * for a record that claims another BlTxID (clipped, safe, and as costly as
 * the walk Go does for that record).  A call with out_cap = 0 runs the whole
 * pass except the writes to learn off[n]: a caller that knows an upper bound
 * passes it and calls again only when a status is MH_ERR_BUFFER_TOO_SMALL. */
enum { MH_ANS_TX = 0, MH_ANS_ENTRY = 1 };

typedef struct mh_answer_store { /* a resident store, all on the ahtree's context's device */
    const uint8_t *txlog;        /* tx-log data after its appendable header; the allocation
                                    extends >= 256 bytes past txlog + txlog_len (checked) */
    uint64_t txlog_len;
    const uint8_t *clog;         /* ntx commit-log entries, device memory */
    uint64_t ntx;                /* = the committed tx id (CommittedAlh) */
    uint32_t clog_entry_size;    /* 12 or 44 */
    uint32_t max_entries, max_key_len;
} mh_answer_store;

typedef struct mh_answer_batch { /* host memory, pageable or pinned */
    uint64_t n;
    const uint8_t *kind;         /* n: MH_ANS_* */
    const uint64_t *tx;          /* n: the tx to read (req.Tx / txhdr.Id / vTxID) */
    const uint64_t *prove_since; /* n: ProveSinceTx */
    const uint8_t *keys;         /* ENTRY: the key as stored in the tx (EncodeKey(vKey)) */
    const uint64_t *key_off;     /* n + 1; TX requests own an empty range */
    const uint8_t *entries;      /* ENTRY: the caller's marshalled schema.Entry, embedded */
    const uint64_t *entry_off;   /* n + 1; verbatim as field 1; empty = field omitted */
} mh_answer_batch;

int mh_verifiable_answer_pb_batch(mh_ahtree *t, const mh_answer_store *s, const mh_answer_batch *b,
                                  uint8_t *out, uint64_t out_cap, uint64_t *off, int32_t *status);

/* ------------------------------------------------------------ leader path */
/* ImmuStore.ExportTx(txID, allowPrecommitted, skipIntegrityCheck = false, tx)
 * (immustore.go:2621-2770) for the consecutive txs first_tx .. first_tx +
 * count - 1 of a store whose tx log, commit log and value logs are resident
 * on ctx's device, in one device pass: readTx re-hashes every record (entry
 * digests, hash tree, innerHash, Alh; tx.go:388-630), readValueAt reads every
 * value from its value log and compares its SHA-256 with the entry's stored
 * hVal (:3183-3240), and the bytes mh_replicate_tx_batch takes are written.
 * Tx k of the run yields out[off[k] .. off[k + 1]):
 *   BE32 len(hdr) | hdr | entries | BE16 1 | byte(truncated)
 *   hdr = TxHeader.Bytes() (tx.go:103-164): id, PrevAlh, ts, version, then v0
 *     BE16 nentries, v1 BE16 mdLen | TxMetadata.Bytes() | BE32 nentries, then
 *     Eh -- the rebuilt root, the log does not store it --, BlTxID, BlRoot;
 *   an entry = BE16 kLen | key | BE16 mdLen | KVMetadata.Bytes() | BE32 vLen |
 *     value (the record stores the metadata ahead of the key); in a truncated
 *     tx BE32 32 | hVal instead of vLen | value.
 * Metadata is written as Go re-serialises it (each attribute once, in code
 * order), whatever form the record stores.
 * A value's place is decodeOffset(vOff) (:1429-1431): value log id = bits
 * 56..63, offset = vOff with bits 55..62 cleared (Go's mask is 0xff << 55).
 *   vLen == 0: nothing is read, the value is available (hVal must be
 *     SHA256(nil));
 *   vLen > 0, id 0: truncated (io.EOF, :3186);
 *   vLen > 0, id in 1..nvlogs: available iff [offset, offset + vLen) lies
 *     wholly inside [first_off, end_off) of vlogs[id - 1], else truncated
 *     (multiapp.ReadAt's io.EOF for a missing chunk or a short read);
 *   vLen > 0, id > nvlogs: MH_ERR_ILLEGAL_STATE (Go indexes past s.vLogs).
 * status[k], first match:
 *   the record verdict of the tx, exactly the status mh_txlog_validate_clog
 *     gives that cLog entry (a cLog entry that points outside the log
 *     included: a status, never a fault);
 *   the status of the lowest entry that fails: MH_ERR_ILLEGAL_STATE as above;
 *     MH_ERR_CORRUPTED_DATA for an available value whose SHA-256 is not the
 *     stored hVal (:3235), and for an entry whose class (available /
 *     truncated) is not entry 0's ("partially truncated transaction", :2703,
 *     :2726; an empty value in an otherwise truncated tx is one);
 *   MH_ERR_BUFFER_TOO_SMALL  the blob ends beyond out_cap;
 *   MH_OK.
 * off[] depends on the records and on what is resident, never on a hash, and
 * is complete for all count whatever out_cap is: a call with out_cap = 0 runs
 * the pass without the writes and leaves the size of a second call in
 * off[count].  A tx that fails on its record, on a value log it names or on
 * the class rule owns an empty range; one that fails on a value digest keeps
 * its sized range with unspecified contents: the caller must not send it.
 * The blobs of the other txs are never disturbed; no byte of out outside the
 * written blobs is touched.  truncated[k] (nullable) is the trailer byte of an
 * MH_OK tx, else 0.
 * out is host memory (pageable or pinned) or memory of ctx's device (detected;
 * then nothing is copied down); off, status, truncated are host memory.
 * count == 0 is MH_OK with off[0] = 0.  MH_ERR_ILLEGAL_ARGUMENTS before any
 * device work: a null ctx / s / off / status (out with out_cap > 0; txlog,
 * clog with ntx > 0; vlogs with nvlogs > 0; data of a non-empty vLog),
 * first_tx == 0, clog_entry_size not 12 or 44, nvlogs > 127 (MaxParallelIO),
 * count >= 2^31, a vLog with end_off < first_off or with data not 4-byte
 * aligned (a value's first dword is read from its aligned address), and --
 * after the next check -- txlog, clog or a non-empty vLog's data not on ctx's
 * device, txlog's allocation not 256 bytes longer than txlog_len, a vLog's
 * not 256 bytes longer than end_off - first_off.  first_tx + count - 1 > ntx
 * returns MH_ERR_TX_NOT_FOUND (immustore.go:3000).  The context's lock is
 * held for the whole pass, so calls on one context run one after the other.
 * No load touches a vLog outside [data, data + (end_off - first_off) + 256).
 * Not covered: skipIntegrityCheck = true (Go then exports a zero Eh and
 * hashes nothing); stores with EMBEDDED_VALUES.  Records with more than 1024
 * entries or with metadata that is valid but not canonical are exported like
 * any other: their verdict comes from the read path's host fallback, and the
 * blob's metadata is re-serialised on the device. */
typedef struct mh_export_vlog {  /* one value log, or the resident part of it */
    const uint8_t *data;         /* device; data[0] is the vLog's byte first_off */
    uint64_t first_off, end_off; /* bytes [first_off, end_off) are resident */
} mh_export_vlog;

typedef struct mh_export_store {
    const uint8_t *txlog;        /* as mh_answer_store (256 bytes of slack, checked) */
    uint64_t txlog_len;
    const uint8_t *clog;         /* ntx commit-log entries, device memory */
    uint64_t ntx;                /* committed or precommitted: the caller decides */
    uint32_t clog_entry_size;    /* 12 or 44 */
    uint32_t max_entries, max_key_len;
    const mh_export_vlog *vlogs; /* host array; value log id k is vlogs[k - 1] */
    uint32_t nvlogs;             /* <= 127 */
} mh_export_store;

int mh_export_tx_batch(mh_ctx *ctx, const mh_export_store *s, uint64_t first_tx, uint64_t count,
                       uint8_t *out, uint64_t out_cap, uint64_t *off /* count + 1 */,
                       int32_t *status /* count */, uint8_t *truncated /* count, nullable */);

/* ------------------------------------------- tx answers under an EntriesSpec */
/* db.TxByID (pkg/database/database.go:1034-1063), one item of db.TxScan's
 * TxList (:1531-1583) and db.VerifiableTxByID (:1462-1528) for n requests over
 * a store whose tx log, commit log and value logs are resident on ctx's
 * device, in one device pass: ReadTx re-hashes the record, db.serializeTx
 * (:1080-1231) walks its entries under the request's EntriesSpec,
 * ImmuStore.ReadValue (immustore.go:3149-3179) reads every asked value where
 * it lies in its value log and readValueAt (:3183-3240) compares its SHA-256
 * with the entry's stored hVal.  MH_TXA_TX yields the marshalled schema.Tx,
 * MH_TXA_VERIFIABLE the marshalled schema.VerifiableTx{tx, dualProof}; request
 * p owns out[off[p] .. off[p + 1]).  The store is mh_export_tx_batch's; t is
 * the ahtree over the store's Alh values as for mh_verifiable_answer_pb_batch,
 * must live on ctx and may be NULL iff no request is VERIFIABLE.
 *
 * has_spec[p] == 0 (req.EntriesSpec is nil, database.go:1081-1083):
 *   TxToProto(tx): every entry with key, hValue, vLen and metadata, whatever
 *   its key's first byte; the actions are ignored.  A VERIFIABLE request then
 *   yields exactly the bytes of mh_verifiable_answer_pb_batch for MH_ANS_TX
 *   with the same (tx, prove_since).
 * has_spec[p] == 1: the header is TxHeaderToProto (eH = the rebuilt root);
 *   the entries are walked in record order and classified by key[0]
 *   (database.go:1092-1227): 0 (SetKeyPrefix) takes kv_action[p], 1
 *   (SortedSetKeyPrefix) z_action[p], 2 (SQLPrefix) sql_action[p]; any other
 *   first byte drops the entry; an empty key is MH_ERR_ILLEGAL_STATE at that
 *   entry's place in the order (Go indexes e.Key()[0] and panics).  Per action
 *   (schema.EntryTypeAction; MH_TXA_NO_SPEC: that EntryTypeSpec is nil):
 *     MH_TXA_NO_SPEC, EXCLUDE (0)  dropped;
 *     ONLY_DIGEST (1)  TxEntryToProto(e) appended to Tx.entries;
 *     RAW_VALUE (2)    ReadValue(e), then TxEntryToProto(e) with value (field
 *                      5) appended to Tx.entries;
 *     RESOLVE (3)      SQL: MH_ERR_ILLEGAL_ARGUMENTS ("sql entry resolution is
 *                      not supported", :1225), reached only when the tx has an
 *                      SQL entry and no earlier entry failed.  kv / z: needs the
 *                      index and is not covered: the whole call returns
 *                      MH_ERR_ILLEGAL_ARGUMENTS before any device work.
 * ReadValue (immustore.go:3149-3179), in this order:
 *   metadata with an expiration and expiresAt <= now_unix (!expiresAt.After(
 *     now), whole seconds): ErrExpiredEntry: the entry is dropped, nothing is
 *     read, no error (database.go:1104-1106);
 *   vLen == 0: no read and no digest check (:3162-3169 returns before
 *     readValueAt): field 5 is omitted, the entry is written as ONLY_DIGEST
 *     writes it -- unlike mh_export_tx_batch, whose empty values are hashed;
 *   vLen > 0: the availability classes of mh_export_tx_batch: vLog id 0, or a
 *     range not wholly inside [first_off, end_off) of vlogs[id - 1]:
 *     MH_ERR_EOF; id > nvlogs: MH_ERR_ILLEGAL_STATE; else SHA-256 of the value
 *     against the stored hVal, a mismatch is MH_ERR_CORRUPTED_DATA (:3235).
 * The first failing entry in record order decides the tx's status: a value
 * that is never read (excluded, digest-only, expired, behind an earlier
 * failure in Go's order) raises nothing, and the status is the lowest failing
 * entry's whatever order the lanes ran in.
 * Marshalling as protobuf-go, as for mh_verifiable_answer_pb_batch; TxEntry's
 * fields in number order, so value is the last field of its entry; Tx.entries
 * may be empty (only the header is written); kvEntries, zEntries and the
 * server's signature are never written.
 *
 * status[p], first match (N = s->ntx, S = prove_since[p], T = tx[p]):
 *   TX:         MH_ERR_ILLEGAL_ARGUMENTS T == 0 (immustore.go:2570);
 *               MH_ERR_TX_NOT_FOUND T > N (:3000); the record verdict of tx T;
 *   VERIFIABLE: exactly the order of mh_verifiable_answer_pb_batch:
 *               MH_ERR_ILLEGAL_STATE S > N first (database.go:1467), then T,
 *               the verdicts of T and S, the DualProof statuses (ahead of the
 *               serialization, as :1514-1522 runs them);
 *   both:       MH_ERR_CORRUPTED_DATA for header metadata the writer cannot
 *               encode; the serializeTx status above; MH_ERR_BUFFER_TOO_SMALL
 *               (the answer ends beyond out_cap); MH_OK.
 * Sizes never depend on a hash: off[] is complete for all n whatever out_cap
 * is (out_cap = 0 sizes the output and still hashes: a digest status comes
 * ahead of MH_ERR_BUFFER_TOO_SMALL).  A request that fails ahead of
 * serializeTx, or whose tx has an entry that fails without a hash, owns an
 * empty range -- also when a lower entry's digest decides its status; one
 * that fails on a value digest alone keeps its sized range with unspecified
 * contents.  No byte of out outside the written answers is touched.  No load
 * leaves [data, data + (end_off - first_off) + 256) of a vLog or the tx log's
 * slack.
 * out is host memory (pageable or pinned) or memory of ctx's device (detected;
 * then nothing is copied down); off and status are host memory.  n == 0 is
 * MH_OK with off[0] = 0.  MH_ERR_ILLEGAL_ARGUMENTS before any device work: a
 * null ctx / s / b / off / status / request array (out with out_cap > 0), a
 * kind or an action outside its enum, a VERIFIABLE request with t == NULL, t
 * not on ctx, n >= 2^31, ntx >= 2^36, and the store checks of
 * mh_export_tx_batch (clog_entry_size, nvlogs, the 256 bytes of slack, the
 * 4-byte alignment of vLog data, everything on ctx's device).  Locks: the
 * tree's first when t is given, then the context's, both for the whole call.
 * Cost: a tx asked by several requests is located and re-hashed once per call
 * (a TX request also reads the record its BlTxID names, as the shared read set
 * does for a proof); a schema.Tx is laid out once per distinct (tx, actions)
 * and a value hashed once per distinct (tx, set of classes read), not once per
 * request.
 * Not covered: kv / z RESOLVE, stores with EMBEDDED_VALUES, the server's
 * signature of the state, a mh_multi_* form. */
enum { MH_TXA_TX = 0,          /* schema.Tx: db.TxByID (database.go:1034-1063), one item of
                                  db.TxScan's TxList (:1531-1583) */
       MH_TXA_VERIFIABLE = 1   /* schema.VerifiableTx: db.VerifiableTxByID (:1462-1528) */ };
#define MH_TXA_NO_SPEC 0xff    /* that EntryTypeSpec is nil */

typedef struct mh_tx_answer_batch {   /* host memory, pageable or pinned */
    uint64_t n;
    const uint8_t  *kind;         /* n: MH_TXA_* */
    const uint64_t *tx;           /* n */
    const uint64_t *prove_since;  /* n: VERIFIABLE only, else ignored */
    const uint8_t  *has_spec;     /* n: 0 = req.EntriesSpec is nil -> TxToProto */
    const uint8_t  *kv_action;    /* n: schema.EntryTypeAction value (0..3) or MH_TXA_NO_SPEC */
    const uint8_t  *z_action;     /* n */
    const uint8_t  *sql_action;   /* n */
    int64_t now_unix;             /* time.Now().Unix() for ExpiredAt, one per batch */
} mh_tx_answer_batch;

int mh_tx_answer_pb_batch(mh_ctx *ctx, mh_ahtree *t /* may be NULL iff no request is VERIFIABLE */,
                          const mh_export_store *s, const mh_tx_answer_batch *b,
                          uint8_t *out, uint64_t out_cap, uint64_t *off /* n + 1 */, int32_t *status /* n */);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IMMUSTORE_MERKLE_H */
