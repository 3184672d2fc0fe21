"""CPU reference of mh_verify_dual_proof_pb_batch for one message: what a
client does with a schema.DualProof answer -- proto.Unmarshal +
DualProofFromProto (database_protoconv.go:213-287) + store.VerifyDualProof
(embedded/store/verification.go:127-235) -- from the protobuf runtime (with
Go's varint and DigestFromProto rules, test_gpu_pb_decode.expect_v1) and the C
oracle's verifier."""
import struct

import numpy as np

from tx_util import TX_HEADER

MAX_EXTRA = 256  # maxExtraLen, tx_metadata.go


def _header(h):
    """TxHeaderFromProto -> (TX_HEADER record with md_off 0, its metadata's
    Bytes()); a version-0 header's metadata is dropped, as innerHash never
    reads it (tx.go:258-263)."""
    md = b""
    if h.HasField("metadata") and (h.version & 0xFFFFFFFF) != 0:
        if h.metadata.truncatedTxID > 0:
            md += b"\x00" + struct.pack(">Q", h.metadata.truncatedTxID)
        if 0 < len(h.metadata.extra) <= MAX_EXTRA:
            md += b"\x01" + struct.pack(">H", len(h.metadata.extra)) + h.metadata.extra
    r = np.zeros(1, TX_HEADER)[0]
    r["id"], r["ts"], r["bl_tx_id"] = h.id, h.ts, h.blTxId
    for f, v in (("bl_root", h.blRoot), ("prev_alh", h.prevAlh), ("eh", h.eH)):
        r[f] = np.frombuffer((bytes(v) + bytes(32))[:32], np.uint8)
    r["version"], r["nentries"] = h.version & 0xFFFFFFFF, h.nentries & 0xFFFFFFFF
    r["md_len"] = len(md)
    return r, md


def reference(wire, orc, raw, src, tgt, src_alh, tgt_alh):
    """-> (status, ok): status as mh_dual_proof_pb_decode_batch gives it (0,
    2 = a header or the linear proof missing, 14 = not a valid encoding); ok =
    status 0 and VerifyDualProof true.  A header version above 1 (Go's
    innerHash panics) is false."""
    from test_gpu_pb_decode import expect_v1
    st, e = expect_v1(wire, raw)
    if st != 0:
        return st, False
    M = wire.MSG["DualProof"].FromString(raw)
    sh, smd = _header(M.sourceTxHeader)
    th, tmd = _header(M.targetTxHeader)
    if int(sh["version"]) > 1 or int(th["version"]) > 1:
        return 0, False
    th["md_off"] = len(smd)
    lap = (e["advance"], e["nested"]) if e["has_advance"] else None
    ok = orc.verify_dual_proof(sh, th, smd + tmd, e["incl"], e["cons"], e["tbl"], e["last"],
                               e["linear"], lap, int(src), int(tgt), bytes(src_alh), bytes(tgt_alh))
    return 0, bool(ok)
