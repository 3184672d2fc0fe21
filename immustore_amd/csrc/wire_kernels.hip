// wire_kernels.hip -- proofs as protobuf messages, built on the device
// (wire formats; 8(f) row 3, DualProofV2 assembly).
//
// The gRPC server turns every proof into a message of pkg/api/schema/schema.proto
// (Go: pkg/api/schema/database_protoconv.go) and marshals it with protobuf-go.
// These kernels produce the same bytes directly from the device-resident tree:
//
//   InclusionProof  schema.proto:534-540   InclusionProofToProto  database_protoconv.go:115-121
//                   terms = (*HTree).InclusionProof(leaf)          htree.go:121-164
//   DualProofV2     schema.proto:437-445   DualProofV2ToProto     database_protoconv.go:152-159
//   TxHeader        schema.proto:349-367   TxHeaderToProto        database_protoconv.go:161-177
//   TxMetadata      schema.proto:380-383   TxMetadataToProto      database_protoconv.go:179-193
//                   proofs of ImmuStore.DualProofV2                immustore.go:2356-2387
//
// proto3 encoding as protobuf-go marshals generated messages: fields in field
// number order, scalar zero values and empty bytes omitted, sub-messages
// present whenever the Go pointer is non-nil, int32 / int64 negatives as
// 10-byte two's-complement varints.  Every tag here is one byte (field < 16).
//
// Two passes, one lane per message: k_pb_*_size (status, byte size and term
// counts; no memory reads beyond the headers), an inclusive scan of the sizes
// (hipcub) into off[1..n], then k_pb_*_write (headers streamed through a
// register-staged ByteWriter as dword stores; the 34-byte term records built
// per round in LDS and written by the whole wave, staged_records).  Measured
// on MI355X, 10^6 DualProofV2 over a 2^24-append tree: one wave per message
// doing the walks and header encoding itself, 25 ms (64x the serial index
// math); index lists stored by the size pass + one wave per message
// materialising dwords, 8.1 ms; one lane per message storing its own records,
// 4.5 ms (64 scattered lines per store); records staged per wave, 4 per lane
// per round, 3.0 ms (8 per round: 3.7 ms, LDS occupancy; 2: 4.0 ms, flush
// overhead).
#include <algorithm>
#include <cstdlib>

#include <hipcub/hipcub.hpp>

#include "digest_io.hpp"
#include "mh_internal.hpp"
#include "pb_write.hpp"
#include "proof_walk.hpp"

namespace mh {

// vlen / i32v, PbHdr / pb_header / framed (TxHeader), ByteWriter, put_rec34,
// put_digest, put_header and load_node are in pb_write.hpp.

// ------------------------------------------------------------ DualProofV2
// ImmuStore.DualProofV2 (immustore.go:2356-2387) checks and proof bounds.
struct PbDual {
    PbHdr s, t;
    uint64_t ii = 0, ij = 0, ci = 0;  // InclusionProof(ii, ij), ConsistencyProof(ci, ij)
    bool proofs = false;
    int32_t st = MH_OK;
};

__device__ inline PbDual pb_dual(const MhTxHeader &src, const MhTxHeader &tgt,
                                 const uint8_t *md_blob, uint64_t size) {
    PbDual d;
    if (src.id == 0) { d.st = MH_ERR_ILLEGAL_ARGUMENTS; return d; }
    if (src.id > tgt.id) { d.st = MH_ERR_SOURCE_TX_NEWER; return d; }
    if (src.id - 1 != src.bl_tx_id || tgt.id - 1 != tgt.bl_tx_id) {
        d.st = MH_ERR_UNEXPECTED_LINKING;
        return d;
    }
    if (src.id < tgt.id) {
        d.proofs = true;
        d.ii = src.id;
        d.ij = tgt.bl_tx_id;
        d.ci = src.bl_tx_id > 1 ? src.bl_tx_id : 1;  // maxUint64(1, sourceTxHdr.BlTxID)
        // (*AHtree).InclusionProof / ConsistencyProof (ahtree.go:525-545, 579-597):
        // i <= j holds here; j beyond the tree is ErrUnexistentData
        if (d.ij > size) { d.st = MH_ERR_UNEXISTENT_DATA; return d; }
    }
    d.s = pb_header(src, md_blob);
    if (d.s.st) { d.st = d.s.st; return d; }
    d.t = pb_header(tgt, md_blob);
    if (d.t.st) { d.st = d.t.st; return d; }
    return d;
}

__global__ __launch_bounds__(256) void k_pb_dual_size(const uint8_t *__restrict__ dlog, uint64_t size,
                                                      uint64_t n, const MhTxHeader *__restrict__ src,
                                                      const MhTxHeader *__restrict__ tgt,
                                                      const uint8_t *__restrict__ md_blob,
                                                      uint64_t *__restrict__ sizes,
                                                      uint32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const PbDual d = pb_dual(src[p], tgt[p], md_blob, size);
    uint64_t s = 0;
    uint32_t ni = 0, nc = 0;
    if (!d.st) {
        if (d.proofs) {
            ni = ahtree_walk(false, d.ii, d.ij, [](uint32_t, uint64_t) {});
            nc = ahtree_walk(true, d.ci, d.ij, [](uint32_t, uint64_t) {});
        }
        s = framed(d.s.body) + framed(d.t.body) + 34ull * (ni + nc);
    }
    sizes[p] = s;
    cnt[2 * p] = ni;
    cnt[2 * p + 1] = nc;
    status[p] = d.st;
}

// ------------------------------------------------------------ byte streams
// ByteWriter, put_rec34 / put_digest and put_header: pb_write.hpp.

// ------------------------------------------------------------ staged term records
// Each lane owns one message, but its term records leave through LDS: per
// round a lane builds up to kRpr records of its walk in its LDS slot -- in
// message order, at the byte alignment of their global destination -- and
// then the wave writes every lane's span (up to 272 contiguous bytes) with
// all 64 lanes storing consecutive dwords.  One message per lane keeps the
// serial index walks parallel; the staging turns 64 scattered lines per
// store instruction into 2-3 contiguous ones.
#ifndef MH_PB_RPR
#define MH_PB_RPR 4  // A/B (tools/pb_ab.sh): 4 beats 8 (LDS occupancy) and 2 (flush overhead)
#endif
constexpr uint32_t kRpr = MH_PB_RPR;  // records per lane per round
constexpr uint32_t kSlotBytes = (3 + kRpr * 34 + 15) / 16 * 16;  // + alignment bytes, 16-byte rows

// Records q = 0 .. cnt-1 of the walk `gen` (walk order) go to
// rec_base + 34 * (cnt - 1 - q) (proof order, proof_walk.hpp).  Wave-uniform
// control flow: every lane of the wave calls this (inactive lanes with cnt 0).
// A walk that ends before `cnt` terms (the size pass and the writer would
// disagree -- never seen, the two forms are tested against each other) reads
// node 0 instead of faulting and sets *bad.
template <class Gen>
__device__ __forceinline__ void staged_records(uint8_t *rec_base, uint32_t cnt, uint32_t tag,
                                               Gen &gen, const uint8_t *__restrict__ nodes,
                                               uint8_t *wave_lds, int lane, bool *bad) {
    uint8_t *slot = wave_lds + lane * kSlotBytes;
    uint32_t done = 0;
    while (__any(done < cnt)) {
        const uint32_t cr = done < cnt ? min(kRpr, cnt - done) : 0;
        uint8_t *g = rec_base + 34ull * (cnt - done - cr);  // span start (message order)
        const uint32_t a = (uint32_t)((uintptr_t)g & 3);
        // gather in pairs (two node loads in flight), build in LDS
        for (uint32_t k = 0; k < cr; k += 2) {
            uint32_t x[8], y[8];
            uint64_t n0 = gen.next();
            uint64_t n1 = k + 1 < cr ? gen.next() : n0;
            if (n0 == ~0ull || n1 == ~0ull) {
                *bad = true;
                n0 = n1 = 0;
            }
            load_node(nodes + n0 * 32, x);
            load_node(nodes + n1 * 32, y);
            put_rec34(slot + a + 34 * (cr - 1 - k), tag, x);
            if (k + 1 < cr) put_rec34(slot + a + 34 * (cr - 2 - k), tag, y);
        }
        done += cr;
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are done
        __builtin_amdgcn_wave_barrier();
        const uint64_t ga = (uint64_t)(uintptr_t)g;
        const uint32_t len = 34 * cr;
        for (int sl = 0; sl < 64; sl++) {  // span of lane sl, read with v_readlane (scalar)
            const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)len, sl);
            if (!ls) continue;
            const uint64_t gs =
                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ga >> 32), sl) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ga, sl);
            const uint32_t as = (uint32_t)(gs & 3);
            const uint32_t nd = (as + ls + 3) / 4;
            g32 *gw = (g32 *)(uintptr_t)(gs - as);
            const uint32_t *lw = reinterpret_cast<const uint32_t *>(wave_lds + sl * kSlotBytes);
            for (uint32_t d = lane; d < nd; d += 64) {
                const uint32_t lo = d == 0 ? as : 0;
                const uint32_t hi = min(4u, as + ls - 4 * d);
                const uint32_t v = lw[d];
                if (lo == 0 && hi == 4) {
                    gw[d] = v;
                } else {
                    g8 *gb = (g8 *)(gw + d);
                    for (uint32_t e = lo; e < hi; e++) gb[e] = (uint8_t)(v >> (8 * e));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();  // every span is out before the slots are rebuilt
    }
}

// ------------------------------------------------------------ wave-dense term records
// The records of a wave's 64 messages written record-parallel: each lane
// walks its own proof (the loop form, proof_walk.hpp) into an LDS index list
// -- the lists of the wave back to back, at the wave's exclusive prefix of the
// term counts -- and then the wave writes the flattened records with one
// lane per 34-byte record, consecutive records on consecutive lanes, two
// records per lane in flight.  Node indices are 32-bit: the host takes this
// path only when the tree has fewer than 2^32 nodes (else staged_records).
// Lists that do not fit kIdxCap go in chunks of whole messages.
#ifndef MH_PB_IDXCAP
#define MH_PB_IDXCAP 4096
#endif
constexpr uint32_t kIdxCap = MH_PB_IDXCAP;
#ifndef MH_PB_UNROLL
#define MH_PB_UNROLL 2
#endif
constexpr uint32_t kPbUnroll = MH_PB_UNROLL;  // records per lane in flight
static_assert(kIdxCap >= 256, "a message's list (<= 130 terms) must fit a chunk");
struct WaveRecLds {
    uint32_t idx[kIdxCap];
    uint32_t pre[65];
    uint64_t base[64];
};

// walk(emit) runs the loop-form walk of the calling lane and returns its term
// count; emit(q, node) gets the terms in walk order (proof position cnt-1-q).
// Called by the whole wave (blockDim 64); lanes without records pass cnt 0.
template <class Walk>
__device__ __forceinline__ void wave_records(uint8_t *rec_base, uint32_t cnt, uint32_t tag,
                                             Walk &&walk, const uint8_t *__restrict__ nodes,
                                             WaveRecLds &L, int lane, bool *bad) {
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += y;
    }
    const uint32_t excl = incl - cnt;
    __syncthreads();  // a previous call's records are out of L
    L.pre[lane] = excl;
    if (lane == 63) L.pre[64] = incl;
    L.base[lane] = (uint64_t)(uintptr_t)rec_base;
    uint32_t m0 = 0;
    while (m0 < 64) {
        const uint32_t base0 = (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)m0);
        const uint64_t fit = __ballot(lane >= (int)m0 && incl - base0 <= kIdxCap);
        const uint32_t m1 = m0 + max(1u, (uint32_t)__popcll(fit));
        const uint32_t T =
            min(kIdxCap, (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(m1 - 1)) - base0);
        __syncthreads();  // the previous chunk's records are out of L.idx
        if ((uint32_t)lane >= m0 && (uint32_t)lane < m1 && cnt) {
            uint32_t *dst = L.idx + (excl - base0);
            const uint32_t c = walk([&](uint32_t q, uint64_t node) {
                if (q < cnt) dst[cnt - 1 - q] = (uint32_t)node;
            });
            if (c != cnt || cnt > kIdxCap) {  // size pass and writer disagree: never seen
                for (uint32_t k = 0; k < min(cnt, kIdxCap); k++) dst[k] = 0;
                *bad = true;
            }
        }
        __syncthreads();
        uint32_t m = m0;
        auto locate = [&](uint32_t r) {  // message of flattened record r (m only moves forward)
            while (m + 1 < m1 && L.pre[m + 1] - base0 <= r) m++;
            return m;
        };
        for (uint32_t r0 = 0; r0 < T; r0 += 64 * kPbUnroll) {
            uint32_t x[kPbUnroll][8];
            uint8_t *pr[kPbUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kPbUnroll; u++) {  // kPbUnroll gathers in flight
                const uint32_t r = r0 + 64 * u + lane;
                pr[u] = nullptr;
                if (r < T) {
                    const uint32_t mr = locate(r);
                    pr[u] = reinterpret_cast<uint8_t *>(L.base[mr]) + 34ull * (r - (L.pre[mr] - base0));
                    load_node(nodes + (uint64_t)L.idx[r] * 32, x[u]);
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kPbUnroll; u++)
                if (pr[u]) put_rec34_as<1>(pr[u], tag, x[u]);  // global stores
        }
        m0 = m1;
    }
}

// DualProofV2 writer over wave_records: one wave per block, lane per message
// for the headers (ByteWriter) and the walks.
__global__ __launch_bounds__(64) void k_pb_dual_write_w(const uint8_t *__restrict__ dlog,
                                                        uint64_t size, uint64_t n,
                                                        const MhTxHeader *__restrict__ src,
                                                        const MhTxHeader *__restrict__ tgt,
                                                        const uint8_t *__restrict__ md_blob,
                                                        const uint64_t *__restrict__ off,
                                                        const uint32_t *__restrict__ cnt,
                                                        uint8_t *__restrict__ out, uint64_t out_cap,
                                                        int32_t *__restrict__ status) {
    __shared__ WaveRecLds L;
    const uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const int lane = threadIdx.x;
    bool active = p < n && status[p] == MH_OK;
    if (active && off[p + 1] > out_cap) {
        status[p] = MH_ERR_BUFFER_TOO_SMALL;
        active = false;
    }
    uint8_t *rec = out;
    uint32_t ni = 0, nc = 0;
    uint64_t ii = 1, ij = 1, ci = 1;
    if (active) {
        const MhTxHeader &S = src[p], &T = tgt[p];
        const PbDual d = pb_dual(S, T, md_blob, size);
        uint8_t *o = out + off[p];
        ByteWriter bw(o);
        put_header(bw, 0x0a, S, d.s, md_blob);
        put_header(bw, 0x12, T, d.t, md_blob);
        bw.finish();
        rec = o + framed(d.s.body) + framed(d.t.body);
        if (d.proofs) {
            ni = cnt[2 * p];
            nc = cnt[2 * p + 1];
            ii = d.ii;
            ij = d.ij;
            ci = d.ci;
        }
    }
    if (!__any(ni + nc > 0)) return;  // wave-uniform (one wave per block)
    bool bad = false;
    wave_records(rec, ni, 0x1a, [&](auto &&emit) { return ahtree_walk(false, ii, ij, emit); },
                 dlog, L, lane, &bad);
    wave_records(rec + 34ull * ni, nc, 0x22,
                 [&](auto &&emit) { return ahtree_walk(true, ci, ij, emit); }, dlog, L, lane, &bad);
    if (bad) status[p] = MH_ERR_ILLEGAL_STATE;
}

// One lane per message: header fields streamed from registers, term records
// staged per wave (staged_records).
__global__ __launch_bounds__(256) void k_pb_dual_write(const uint8_t *__restrict__ dlog, uint64_t size,
                                                       uint64_t n, const MhTxHeader *__restrict__ src,
                                                       const MhTxHeader *__restrict__ tgt,
                                                       const uint8_t *__restrict__ md_blob,
                                                       const uint64_t *__restrict__ off,
                                                       const uint32_t *__restrict__ cnt,
                                                       uint8_t *__restrict__ out, uint64_t out_cap,
                                                       int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[256 * kSlotBytes];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint8_t *wave_lds = lds + (threadIdx.x & ~63) * kSlotBytes;
    bool active = p < n && status[p] == MH_OK;
    if (active && off[p + 1] > out_cap) {
        status[p] = MH_ERR_BUFFER_TOO_SMALL;
        active = false;
    }
    uint8_t *rec = out;
    uint32_t ni = 0, nc = 0;
    uint64_t ii = 1, ij = 1, ci = 1;
    if (active) {
        const MhTxHeader &S = src[p], &T = tgt[p];
        const PbDual d = pb_dual(S, T, md_blob, size);
        uint8_t *o = out + off[p];
        ByteWriter bw(o);
        put_header(bw, 0x0a, S, d.s, md_blob);
        put_header(bw, 0x12, T, d.t, md_blob);
        bw.finish();
        rec = o + framed(d.s.body) + framed(d.t.body);
        if (d.proofs) {
            ni = cnt[2 * p];
            nc = cnt[2 * p + 1];
            ii = d.ii;
            ij = d.ij;
            ci = d.ci;
        }
    }
    if (!__any(ni + nc > 0)) return;  // wave-uniform from here on
    bool bad = false;
    AhtreeWalk gi(false, ii, ij);
    staged_records(rec, ni, 0x1a, gi, dlog, wave_lds, lane, &bad);
    AhtreeWalk gc(true, ci, ij);
    staged_records(rec + 34ull * ni, nc, 0x22, gc, dlog, wave_lds, lane, &bad);
    if (bad) status[p] = MH_ERR_ILLEGAL_STATE;
}

// ------------------------------------------------------------ InclusionProof (htree)
__device__ __forceinline__ uint32_t pb_incl_prefix(uint64_t leaf, uint64_t w) {
    // Leaf: int32(iproof.Leaf), Width: int32(iproof.Width)
    const uint32_t l = (uint32_t)leaf, ww = (uint32_t)w;
    return (l ? 1 + vlen(i32v(l)) : 0) + (ww ? 1 + vlen(i32v(ww)) : 0);
}

__global__ __launch_bounds__(256) void k_pb_incl_size(uint64_t w, uint64_t n,
                                                      const uint64_t *__restrict__ leaf,
                                                      uint64_t *__restrict__ sizes,
                                                      uint32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t i = leaf[p];
    if (i >= w) {  // htree.go:122-124
        sizes[p] = 0;
        cnt[2 * p] = 0;
        status[p] = MH_ERR_ILLEGAL_ARGUMENTS;
        return;
    }
    const uint32_t c = htree_walk(i, w, [](uint32_t, uint64_t) {});
    sizes[p] = pb_incl_prefix(i, w) + 34ull * c;
    cnt[2 * p] = c;
    status[p] = MH_OK;
}

__global__ __launch_bounds__(256) void k_pb_incl_write(const uint8_t *__restrict__ levels, uint64_t w,
                                                       uint64_t n, const uint64_t *__restrict__ leaf,
                                                       const uint64_t *__restrict__ off,
                                                       const uint32_t *__restrict__ cnt,
                                                       uint8_t *__restrict__ out, uint64_t out_cap,
                                                       int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[256 * kSlotBytes];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint8_t *wave_lds = lds + (threadIdx.x & ~63) * kSlotBytes;
    bool active = p < n && status[p] == MH_OK;
    if (active && off[p + 1] > out_cap) {
        status[p] = MH_ERR_BUFFER_TOO_SMALL;
        active = false;
    }
    uint8_t *rec = out;
    uint32_t c = 0;
    uint64_t i = 0;
    if (active) {
        i = leaf[p];
        uint8_t *o = out + off[p];
        ByteWriter bw(o);
        if ((uint32_t)i) { bw.put8(0x08); bw.varint(i32v((uint32_t)i)); }
        if ((uint32_t)w) { bw.put8(0x10); bw.varint(i32v((uint32_t)w)); }
        bw.finish();
        rec = o + pb_incl_prefix(i, w);
        c = cnt[2 * p];
    }
    if (!__any(c > 0)) return;
    bool bad = false;
    HtreeWalk g(i, active ? w : 0);
    staged_records(rec, c, 0x1a, g, levels, wave_lds, lane, &bad);
    if (bad) status[p] = MH_ERR_ILLEGAL_STATE;
}

__global__ __launch_bounds__(64) void k_pb_incl_write_w(const uint8_t *__restrict__ levels,
                                                        uint64_t w, uint64_t n,
                                                        const uint64_t *__restrict__ leaf,
                                                        const uint64_t *__restrict__ off,
                                                        const uint32_t *__restrict__ cnt,
                                                        uint8_t *__restrict__ out, uint64_t out_cap,
                                                        int32_t *__restrict__ status) {
    __shared__ WaveRecLds L;
    __shared__ uint64_t loff[64];  // level_off(w, l): one table per block
    const uint64_t p = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const int lane = threadIdx.x;
    loff[lane] = level_off(w, lane);
    bool active = p < n && status[p] == MH_OK;
    if (active && off[p + 1] > out_cap) {
        status[p] = MH_ERR_BUFFER_TOO_SMALL;
        active = false;
    }
    uint8_t *rec = out;
    uint32_t c = 0;
    uint64_t i = 0;
    if (active) {
        i = leaf[p];
        uint8_t *o = out + off[p];
        ByteWriter bw(o);
        if ((uint32_t)i) { bw.put8(0x08); bw.varint(i32v((uint32_t)i)); }
        if ((uint32_t)w) { bw.put8(0x10); bw.varint(i32v((uint32_t)w)); }
        bw.finish();
        rec = o + pb_incl_prefix(i, w);
        c = cnt[2 * p];
    }
    if (!__any(c > 0)) return;
    bool bad = false;
    wave_records(rec, c, 0x1a,
                 [&](auto &&emit) {
                     return htree_walk_lo(i, w, [&](int l) { return loff[l]; }, emit);
                 },
                 levels, L, lane, &bad);
    if (bad) status[p] = MH_ERR_ILLEGAL_STATE;
}

// ------------------------------------------------------------ launchers
size_t pb_scan_temp_bytes(uint64_t n) {
    size_t bytes = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const uint64_t *)nullptr,
                                     (uint64_t *)nullptr, (int)(n ? n : 1), (hipStream_t)0);
    return bytes;
}

// scratch: sizes[n] (u64) | term counts[2n] (u32) | scan temp
uint64_t pb_scratch_bytes(uint64_t n) {
    return 2 * ((n * 8 + 255) & ~255ull) + ((pb_scan_temp_bytes(n) + 255) & ~255ull) + 256;
}

// in[0..n) -> out[0..n] with out[0] = 0, out[k+1] = in[0] + ... + in[k]
hipError_t scan_offsets_u64(hipStream_t st, uint64_t n, const uint64_t *in, uint64_t *out,
                            uint8_t *temp, size_t temp_bytes) {
    if (hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), st)) return e;
    if (!n) return hipSuccess;
    return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out + 1, (int)n, st);
}

hipError_t scan_offsets_u64(hipStream_t st, uint64_t n, const uint64_t *in, uint64_t *out,
                            uint8_t *temp) {
    return scan_offsets_u64(st, n, in, out, temp, pb_scan_temp_bytes(n));
}

// sizes -> off[0..n] (off[0] = 0)
static hipError_t pb_offsets(hipStream_t st, uint64_t n, const uint64_t *sizes, uint64_t *off,
                             uint8_t *temp) {
    if (hipError_t e = hipMemsetAsync(off, 0, sizeof(uint64_t), st)) return e;
    size_t bytes = pb_scan_temp_bytes(n);
    return hipcub::DeviceScan::InclusiveSum(temp, bytes, sizes, off + 1, (int)n, st);
}

static inline unsigned grid_for(uint64_t threads, unsigned block) {
    return (unsigned)((threads + block - 1) / block);
}

// MH_PB_STAGED=1 in the environment (read per launch) forces the staged
// writers, the path of trees with >= 2^32 nodes, so the tests cover both.
static bool pb_force_staged() {
    const char *e = getenv("MH_PB_STAGED");
    return e && e[0] == '1';
}

hipError_t launch_pb_dual_v2(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                             uint64_t size, uint64_t n, const MhTxHeader *src,
                             const MhTxHeader *tgt, const uint8_t *md_blob, uint8_t *out,
                             uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch) {
    if (!n) return hipMemsetAsync(off, 0, sizeof(uint64_t), st);
    uint64_t *sizes = reinterpret_cast<uint64_t *>(scratch);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch + ((n * 8 + 255) & ~255ull));
    uint8_t *temp = scratch + 2 * ((n * 8 + 255) & ~255ull);
    if (phase & 1) {
        TimerScope ts(tm, "pb_dual_size", st);
        hipLaunchKernelGGL(k_pb_dual_size, dim3(grid_for(n, 256)), dim3(256), 0, st, dlog, size, n,
                           src, tgt, md_blob, sizes, cnt, status);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = pb_offsets(st, n, sizes, off, temp)) return e;
    }
    if (phase & 2) {
        TimerScope ts(tm, "pb_dual_write", st);
        if (ahtree_nodes_upto(size) < (1ull << 32) && !pb_force_staged())  // 32-bit node indices
            hipLaunchKernelGGL(k_pb_dual_write_w, dim3(grid_for(n, 64)), dim3(64), 0, st, dlog,
                               size, n, src, tgt, md_blob, off, cnt, out, out_cap, status);
        else
            hipLaunchKernelGGL(k_pb_dual_write, dim3(grid_for(n, 256)), dim3(256), 0, st, dlog,
                               size, n, src, tgt, md_blob, off, cnt, out, out_cap, status);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_pb_inclusion(hipStream_t st, Timer *tm, int phase, const uint8_t *levels,
                               uint64_t w, uint64_t n, const uint64_t *leaf, uint8_t *out,
                               uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch) {
    if (!n) return hipMemsetAsync(off, 0, sizeof(uint64_t), st);
    uint64_t *sizes = reinterpret_cast<uint64_t *>(scratch);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch + ((n * 8 + 255) & ~255ull));
    uint8_t *temp = scratch + 2 * ((n * 8 + 255) & ~255ull);
    if (phase & 1) {
        TimerScope ts(tm, "pb_incl_size", st);
        hipLaunchKernelGGL(k_pb_incl_size, dim3(grid_for(n, 256)), dim3(256), 0, st, w, n, leaf,
                           sizes, cnt, status);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = pb_offsets(st, n, sizes, off, temp)) return e;
    }
    if (phase & 2) {
        TimerScope ts(tm, "pb_incl_write", st);
        if (w < (1ull << 31) && !pb_force_staged())  // < 2^32 level nodes: 32-bit indices
            hipLaunchKernelGGL(k_pb_incl_write_w, dim3(grid_for(n, 64)), dim3(64), 0, st, levels,
                               w, n, leaf, off, cnt, out, out_cap, status);
        else
            hipLaunchKernelGGL(k_pb_incl_write, dim3(grid_for(n, 256)), dim3(256), 0, st, levels,
                               w, n, leaf, off, cnt, out, out_cap, status);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------ DualProof (v1)
//   DualProof           schema.proto:388-434   DualProofToProto          database_protoconv.go:131-142
//   LinearProof                                LinearProofToProto        database_protoconv.go:195-201
//   LinearAdvanceProof                         LinearAdvanceProofToProto database_protoconv.go:203-211
//   proofs of ImmuStore.DualProof / LinearProof / LinearAdvanceProof     immustore.go:2394-2562
//
// The answer VerifiableGet / VerifiableSet / VerifiableTxById send.  Its
// ahtree parts are index walks over the dLog as in DualProofV2; its linear
// parts are Alh / innerHash values of whole runs of txs, which the dLog does
// not hold (a leaf is SHA-256(0x00 || Alh)): they are gathered from the
// caller's digest window (first_tx, count, alh, inner: what mh_tx_alh_batch
// wrote for txs first_tx .. first_tx + count - 1).  Nothing is hashed here.
//
// Messages run from a few hundred bytes to hundreds of KiB, so one wave
// takes one message in both passes.  The checks, the header sizes and the
// three top-level walks are wave-uniform (every lane repeats them: for short
// messages the wave does one lane's work); only the advance part is spread,
// the size pass putting the term counts of the a1 - a0 - 1 nested inclusion
// proofs on the lanes (lanes over k, wave sum).  The write pass
// writes every run of 34-byte records with a lane per record (wave_run34)
// and the nested proofs of the advance part a round of up to 64 at a time,
// lane per proof for the walk, wave prefix sum for the starts, lane per
// record for the stores.  Node indices are 64-bit throughout: one writer
// for every tree size.
struct PbDual1 {
    PbHdr s, t;
    uint64_t bl = 0;          // tgt.BlTxID: the tree size of every ahtree proof
    uint64_t ls = 0, lt = 0;  // LinearProof(ls, lt)
    uint64_t a0 = 0, a1 = 0;  // LinearAdvanceProof(a0, a1, bl)
    bool incl = false, cons = false, last = false, adv = false;
    int32_t st = MH_OK;
};

// what the size pass leaves for the writer
struct PbDual1Parts {
    uint64_t adv_body;    // LinearAdvanceProof message length
    uint32_t ni, nc, nl;  // InclusionProof / ConsistencyProof / LastInclusionProof terms
    uint32_t pad;
};

// txs lo .. hi (lo <= hi) are in the digest window
__device__ __forceinline__ bool pb_in_window(uint64_t first, uint64_t count, uint64_t lo, uint64_t hi) {
    return count && lo >= first && hi - first < count;
}

// Where the writer finds the Alh / innerHash of a tx.  DenseWindow: the public
// calls' digest window (tx x at slot x - first).  RankWindow (mh_internal.hpp):
// the compacted list of mh_verifiable_answer_pb_batch.  check(lo, hi): the
// status of reading txs lo .. hi in order (MH_OK: every one is there);
// slot(x): where tx x lies in alh / inner -- a run of txs that check() passed
// lies in consecutive slots; at(p, off): where message p goes in `out`.
struct DenseWindow {
    uint64_t first, count;
    __device__ __forceinline__ int32_t check(uint64_t lo, uint64_t hi) const {
        return pb_in_window(first, count, lo, hi) ? MH_OK : MH_ERR_TX_NOT_FOUND;
    }
    __device__ __forceinline__ uint64_t slot(uint64_t x) const { return x - first; }
    __device__ __forceinline__ uint64_t at(uint64_t p, const uint64_t *off) const { return off[p]; }
};

// The checks of ImmuStore.DualProof in Go's order; the first that fires is
// the status.  src.ID == 0 is refused (the store holds no tx 0; Go would walk
// the tree from leaf 0), as for DualProofV2.
template <class W>
__device__ inline PbDual1 pb_dual1(const MhTxHeader &src, const MhTxHeader &tgt,
                                   const uint8_t *md_blob, uint64_t size, const W &win) {
    PbDual1 d;
    if (src.id == 0) { d.st = MH_ERR_ILLEGAL_ARGUMENTS; return d; }
    if (src.id > tgt.id) { d.st = MH_ERR_SOURCE_TX_NEWER; return d; }
    d.bl = tgt.bl_tx_id;
    // (*AHtree).InclusionProof / ConsistencyProof (ahtree.go:525-545, 579-597):
    // i <= j holds at every call below; j beyond the tree is ErrUnexistentData
    d.incl = src.id < d.bl;
    if (d.incl && d.bl > size) { d.st = MH_ERR_UNEXISTENT_DATA; return d; }
    if (src.bl_tx_id > d.bl) { d.st = MH_ERR_CORRUPTED_TX_DATA; return d; }  // immustore.go:2416
    d.cons = src.bl_tx_id > 0;
    if (d.cons && d.bl > size) { d.st = MH_ERR_UNEXISTENT_DATA; return d; }
    d.last = d.bl > 0;
    if (d.last) {
        if (const int32_t e = win.check(d.bl, d.bl)) { d.st = e; return d; }
        if (d.bl > size) { d.st = MH_ERR_UNEXISTENT_DATA; return d; }
    }
    d.ls = src.id > d.bl ? src.id : d.bl;  // immustore.go:2446, :2472-2475
    d.lt = tgt.id;
    if (d.ls > d.lt) { d.st = MH_ERR_SOURCE_TX_NEWER; return d; }
    if (const int32_t e = win.check(d.ls, d.lt)) { d.st = e; return d; }
    d.a0 = src.bl_tx_id;                   // immustore.go:2452-2456, :2514-2521
    d.a1 = src.id < d.bl ? src.id : d.bl;
    if (d.a1 < d.a0) { d.st = MH_ERR_SOURCE_TX_NEWER; return d; }
    d.adv = d.a1 - d.a0 > 1;
    if (d.adv)
        if (const int32_t e = win.check(d.a0 + 1, d.a1)) { d.st = e; return d; }
    d.s = pb_header(src, md_blob);
    if (d.s.st) { d.st = d.s.st; return d; }
    d.t = pb_header(tgt, md_blob);
    if (d.t.st) { d.st = d.t.st; return d; }
    return d;
}

__device__ __forceinline__ uint64_t framed64(uint64_t body) { return 1 + vlen(body) + body; }

// LinearProof message length: sourceTxId, TargetTxId (both > 0) and lt - ls + 1 terms
__device__ __forceinline__ uint64_t pb_linear_body(uint64_t ls, uint64_t lt) {
    return 2 + vlen(ls) + vlen(lt) + 34 * (lt - ls + 1);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Size pass: one wave per message, 4 per block.  Reads the headers and their
// metadata only.
template <class W>
__global__ __launch_bounds__(256) void k_pb_dual1_size(uint64_t size, uint64_t n,
                                                       const MhTxHeader *__restrict__ src,
                                                       const MhTxHeader *__restrict__ tgt,
                                                       const uint8_t *__restrict__ md_blob,
                                                       const W win,
                                                       uint64_t *__restrict__ sizes,
                                                       PbDual1Parts *__restrict__ parts,
                                                       int32_t *__restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= n) return;  // wave-uniform
    const MhTxHeader &S = src[p], &T = tgt[p];
    const PbDual1 d = pb_dual1(S, T, md_blob, size, win);
    auto none = [](uint32_t, uint64_t) {};
    PbDual1Parts pt = {0, 0, 0, 0, 0};
    uint64_t s = 0;
    if (!d.st) {
        if (d.incl) pt.ni = ahtree_walk(false, S.id, d.bl, none);
        if (d.cons) pt.nc = ahtree_walk(true, S.bl_tx_id, d.bl, none);
        if (d.last) pt.nl = ahtree_walk(false, d.bl, d.bl, none);
        s = framed(d.s.body) + framed(d.t.body) + 34ull * (pt.ni + pt.nc + 1 + pt.nl) +
            framed64(pb_linear_body(d.ls, d.lt));
        if (d.adv) {  // nested proofs k = a0+1 .. a1-1, lanes over k
            const uint64_t np = d.a1 - d.a0 - 1;
            uint64_t nested = 0;
            for (uint64_t q = lane; q < np; q += 64)
                nested += framed64(34ull * ahtree_walk(false, d.a0 + 1 + q, d.bl, none));
            pt.adv_body = 34 * (d.a1 - d.a0) + wave_sum_u64(nested);
            s += framed64(pt.adv_body);
        }
    }
    if (lane == 0) {
        sizes[p] = s;
        parts[p] = pt;
        status[p] = d.st;
    }
}

// cnt records of 34 bytes, lane per record, two gathers per lane in flight.
// at(r, dst, tag) gives the 32 source bytes of record r (16-byte aligned;
// nullptr: zeros), where it goes and its tag; a lane sees its r ascending.
// Called by the whole wave.
template <class At>
__device__ __forceinline__ void wave_run34(uint64_t cnt, int lane, At &&at) {
    for (uint64_t r0 = 0; r0 < cnt; r0 += 128) {
        uint32_t x[2][8], tag[2] = {0, 0};
        uint8_t *pr[2] = {nullptr, nullptr};
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint64_t r = r0 + 64 * u + lane;
            if (r < cnt) {
                const uint8_t *s = at(r, pr[u], tag[u]);
                if (s) {
                    load_node(s, x[u]);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) x[u][k] = 0;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (pr[u]) put_rec34_as<1>(pr[u], tag[u], x[u]);
    }
}

// A/B on MI355X (profiles/ab_dualv1_idxcap.txt; 10^5 messages of ~3 KB over a
// 2^20-append tree): 2048 entries (17 KB of LDS per one-wave block, 9 waves per
// CU) 3.04 ms, 512 entries 2.17 ms.  Long advance parts take more rounds for it.
#ifndef MH_PB1_IDXCAP
#define MH_PB1_IDXCAP 512
#endif
constexpr uint32_t kIdx1Cap = MH_PB1_IDXCAP;
// one round holds min(64, kIdx1Cap / maxc) nested proofs of up to maxc <= 64
// terms each; the top-level lists (<= 64 + 130 + 64 terms) share the array
static_assert(kIdx1Cap >= 320, "the top-level lists must fit");
struct Wave1Lds {
    uint64_t idx[kIdx1Cap];  // dLog node indices
    uint64_t base[64];       // first record of nested proof `lane`
    uint32_t pre[65];        // exclusive prefix of the nested term counts
};

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

// Write pass: one wave (one block) per message.
template <class W>
__global__ __launch_bounds__(64) void k_pb_dual1_write(const uint8_t *__restrict__ dlog,
                                                       uint64_t size, uint64_t n,
                                                       const MhTxHeader *__restrict__ src,
                                                       const MhTxHeader *__restrict__ tgt,
                                                       const uint8_t *__restrict__ md_blob,
                                                       const W win,
                                                       const uint8_t *__restrict__ alh,
                                                       const uint8_t *__restrict__ inner,
                                                       const uint64_t *__restrict__ off,
                                                       const PbDual1Parts *__restrict__ parts,
                                                       uint8_t *__restrict__ out, uint64_t out_cap,
                                                       int32_t *__restrict__ status) {
    __shared__ Wave1Lds L;
    const uint64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    // everything up to the record loops is wave-uniform
    if (p >= n || status[p] != MH_OK) return;
    if (off[p + 1] > out_cap) {
        if (lane == 0) status[p] = MH_ERR_BUFFER_TOO_SMALL;
        return;
    }
    const MhTxHeader &S = src[p], &T = tgt[p];
    const PbDual1 d = pb_dual1(S, T, md_blob, size, win);
    const PbDual1Parts pt = parts[p];
    const uint32_t ni = pt.ni, nc = pt.nc, nl = pt.nl;
    const uint32_t nrec = ni + nc + 1 + nl;  // inclusion | consistency | TargetBlTxAlh | last
    if (d.st || nrec > kIdx1Cap) {           // phase 2 without its phase 1: never seen
        if (lane == 0) status[p] = MH_ERR_ILLEGAL_STATE;
        return;
    }
    uint8_t *o = out + win.at(p, off);
    const uint32_t hs = framed(d.s.body);
    uint8_t *rec = o + hs + framed(d.t.body);
    uint8_t *lin = rec + 34ull * nrec;
    const uint64_t lin_body = pb_linear_body(d.ls, d.lt);
    uint8_t *lin_terms = lin + 1 + vlen(lin_body) + 2 + vlen(d.ls) + vlen(d.lt);
    uint8_t *adv = lin + framed64(lin_body);

    // the byte streams: the two headers on lanes 0 and 1, the sub-message
    // prefixes on lane 2
    if (lane < 2) {
        const MhTxHeader &H = lane ? T : S;
        ByteWriter bw(lane ? o + hs : o);
        put_header(bw, lane ? 0x12 : 0x0a, H, lane ? d.t : d.s, md_blob);
        bw.finish();
    } else if (lane == 2) {
        ByteWriter bw(lin);
        bw.put8(0x3a);
        bw.varint(lin_body);
        bw.put8(0x08);
        bw.varint(d.ls);
        bw.put8(0x10);
        bw.varint(d.lt);
        bw.finish();
        if (d.adv) {
            ByteWriter ba(adv);
            ba.put8(0x42);
            ba.varint(pt.adv_body);
            ba.finish();
        }
    }

    // the three top-level walks on lanes 0..2, proof order into L.idx
    bool bad = false;
    if (lane < 3) {
        const bool c1 = lane == 1;
        const uint64_t i = lane == 0 ? S.id : c1 ? S.bl_tx_id : d.bl;
        const uint32_t cnt = lane == 0 ? ni : c1 ? nc : nl;
        const uint32_t at = lane == 0 ? 0 : c1 ? ni : ni + nc + 1;
        if (cnt) {
            const uint32_t c = ahtree_walk(c1, i, d.bl, [&](uint32_t q, uint64_t node) {
                if (q < cnt) L.idx[at + cnt - 1 - q] = node;
            });
            bad = c != cnt;
        }
    }
    __syncthreads();
    if (__any(bad)) {  // size pass and writer disagree: never seen; no index is read
        if (lane == 0) status[p] = MH_ERR_ILLEGAL_STATE;
        return;
    }
    wave_run34(nrec, lane, [&](uint64_t r, uint8_t *&dst, uint32_t &tag) -> const uint8_t * {
        dst = rec + 34 * r;
        if (r == ni + nc) {  // TargetBlTxAlh: always present, zeros without a BlTxID
            tag = 0x2a;
            return d.last ? alh + 32 * win.slot(d.bl) : nullptr;
        }
        tag = r < ni ? 0x1a : r < ni + nc ? 0x22 : 0x32;
        return dlog + 32 * L.idx[r];
    });
    // LinearProof.terms: Alh(ls), innerHash(ls + 1 .. lt)
    const uint64_t ls_slot = win.slot(d.ls);
    wave_run34(d.lt - d.ls + 1, lane, [&](uint64_t q, uint8_t *&dst, uint32_t &tag) {
        dst = lin_terms + 34 * q;
        tag = 0x1a;
        return (q ? inner : alh) + 32 * (ls_slot + q);
    });
    if (!d.adv) return;

    // LinearAdvanceProof.linearProofTerms: Alh(a0 + 1), innerHash(a0 + 2 .. a1)
    const uint64_t na = d.a1 - d.a0, a_slot = win.slot(d.a0 + 1);
    uint8_t *adv_terms = adv + 1 + vlen(pt.adv_body);
    wave_run34(na, lane, [&](uint64_t q, uint8_t *&dst, uint32_t &tag) {
        dst = adv_terms + 34 * q;
        tag = 0x0a;
        return (q ? inner : alh) + 32 * (a_slot + q);
    });
    // LinearAdvanceProof.inclusionProofs: InclusionProof(k, bl), k = a0+1 .. a1-1
    uint8_t *cur = adv_terms + 34 * na;
    const uint32_t maxc = (uint32_t)bits_len(d.bl - 1);  // >= 1 (bl >= 2); terms of one walk
    const uint32_t P = min(64u, kIdx1Cap / maxc);        // proofs per round
    for (uint64_t k0 = 0; k0 < na - 1; k0 += P) {
        const bool on = (uint32_t)lane < P && k0 + lane < na - 1;
        __syncthreads();  // the previous round's records are out of L
        uint32_t c = 0;
        if (on)  // walk order into the lane's slot
            c = ahtree_walk(false, d.a0 + 1 + k0 + lane, d.bl, [&](uint32_t q, uint64_t node) {
                if (q < maxc) L.idx[lane * maxc + q] = node;
            });
        if (c > maxc) {  // cannot happen: one term per bit of bl - 1 at most
            bad = true;
            c = 0;
        }
        const uint32_t plen = 1 + vlen(34ull * c);  // 0x12, length
        const uint32_t sz = on ? plen + 34 * c : 0;
        const uint32_t ic = wave_incl_scan_u32(c, lane), is = wave_incl_scan_u32(sz, lane);
        uint8_t *mine = cur + (is - sz);
        L.pre[lane] = ic - c;
        if (lane == 63) L.pre[64] = ic;
        L.base[lane] = (uint64_t)(uintptr_t)(mine + plen);
        if (on) {  // nested InclusionProof: terms only (leaf and width are zero)
            g8 *b = (g8 *)mine;
            uint32_t v = 34 * c;
            *b++ = 0x12;
            while (v >= 0x80) {
                *b++ = (uint8_t)(v | 0x80);
                v >>= 7;
            }
            *b = (uint8_t)v;
        }
        __syncthreads();
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
        uint32_t m = 0;
        wave_run34(total, lane, [&](uint64_t r, uint8_t *&dst, uint32_t &tag) {
            while (m + 1 < 64 && L.pre[m + 1] <= r) m++;  // proof of record r (only forward)
            const uint32_t q = (uint32_t)r - L.pre[m], cm = L.pre[m + 1] - L.pre[m];
            dst = reinterpret_cast<uint8_t *>(L.base[m]) + 34 * q;
            tag = 0x1a;
            return dlog + 32 * L.idx[m * maxc + (cm - 1 - q)];
        });
        cur += (uint32_t)__builtin_amdgcn_readlane((int)is, 63);
    }
    if (__any(bad) || cur != adv + framed64(pt.adv_body))
        if (lane == 0) status[p] = MH_ERR_ILLEGAL_STATE;
}

uint64_t pb_dual_v1_scratch_bytes(uint64_t n) {
    return ((n * 8 + 255) & ~255ull) + ((n * sizeof(PbDual1Parts) + 255) & ~255ull) +
           ((pb_scan_temp_bytes(n) + 255) & ~255ull) + 256;
}

// scratch: sizes[n] (u64) | parts[n] | scan temp
template <class W>
static hipError_t pb_dual_v1_run(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                                 uint64_t size, uint64_t n, const MhTxHeader *src,
                                 const MhTxHeader *tgt, const uint8_t *md_blob, const W &win,
                                 const uint8_t *alh, const uint8_t *inner, uint8_t *out,
                                 uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch) {
    if (!n) return hipMemsetAsync(off, 0, sizeof(uint64_t), st);
    uint64_t *sizes = reinterpret_cast<uint64_t *>(scratch);
    PbDual1Parts *parts = reinterpret_cast<PbDual1Parts *>(scratch + ((n * 8 + 255) & ~255ull));
    uint8_t *temp = reinterpret_cast<uint8_t *>(parts) + ((n * sizeof(PbDual1Parts) + 255) & ~255ull);
    if (phase & 1) {
        TimerScope ts(tm, "pb_dual1_size", st);
        hipLaunchKernelGGL(k_pb_dual1_size<W>, dim3(grid_for(n, 4)), dim3(256), 0, st, size, n, src,
                           tgt, md_blob, win, sizes, parts, status);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = pb_offsets(st, n, sizes, off, temp)) return e;
    }
    if (phase & 2) {
        TimerScope ts(tm, "pb_dual1_write", st);
        hipLaunchKernelGGL(k_pb_dual1_write<W>, dim3((unsigned)n), dim3(64), 0, st, dlog, size, n,
                           src, tgt, md_blob, win, alh, inner, off, parts, out, out_cap, status);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_pb_dual_v1(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                             uint64_t size, uint64_t n, const MhTxHeader *src,
                             const MhTxHeader *tgt, const uint8_t *md_blob, uint64_t first_tx,
                             uint64_t count, const uint8_t *alh, const uint8_t *inner, uint8_t *out,
                             uint64_t out_cap, uint64_t *off, int32_t *status, uint8_t *scratch) {
    return pb_dual_v1_run(st, tm, phase, dlog, size, n, src, tgt, md_blob,
                          DenseWindow{first_tx, count}, alh, inner, out, out_cap, off, status,
                          scratch);
}

// The same writer over the compacted list of one mh_verifiable_answer_pb_batch
// call: phase 1 leaves message p's length in off[p + 1] - off[p], phase 2
// writes it at out + win.pos[p] (the caller has checked that it fits).
hipError_t launch_pb_dual_v1_ranked(hipStream_t st, Timer *tm, int phase, const uint8_t *dlog,
                                    uint64_t size, uint64_t n, const MhTxHeader *src,
                                    const MhTxHeader *tgt, const uint8_t *md_blob,
                                    const RankWindow &win, const uint8_t *alh, const uint8_t *inner,
                                    uint8_t *out, uint64_t *off, int32_t *status, uint8_t *scratch) {
    return pb_dual_v1_run(st, tm, phase, dlog, size, n, src, tgt, md_blob, win, alh, inner, out,
                          ~0ull, off, status, scratch);
}

}  // namespace mh
