"""CPU restatement of the DualProof (v1) generator and its protobuf message
(ImmuStore.DualProof / LinearProof / LinearAdvanceProof, immustore.go:2394-2562;
DualProofToProto, database_protoconv.go:131-211), the checker of
mh_ahtree_dual_proof_pb_batch / mh_dev_dual_proof_pb_batch, plus the synthetic
store the GPU tests run over.  Proofs come from the C oracle's ahtree, Alh and
innerHash from the caller's digest window, the bytes from the protobuf runtime
(dual_v1_msg over wire.MSG)."""
import functools

import numpy as np

from tx_util import TX_HEADER

OK = 0
ERR_ILLEGAL_ARGUMENTS = 2
ERR_UNEXISTENT_DATA = 5
ERR_SOURCE_TX_NEWER = 10
ERR_CORRUPTED_DATA = 14
ERR_BUFFER_TOO_SMALL = 19
ERR_CORRUPTED_TX_DATA = 24
ERR_TX_NOT_FOUND = 25


def _md(r, blob):
    return blob[int(r["md_off"]):int(r["md_off"]) + int(r["md_len"])]


def go_dual_proof_parts(src, tgt, blob, aht, first_tx, alhs, inners):
    """ImmuStore.DualProof(src, tgt) over the oracle ahtree `aht` and the digest
    window alhs / inners (txs first_tx .. first_tx + len(alhs) - 1), the checks
    in Go's order -> (status, parts); parts are the first nine arguments of
    orc.verify_dual_proof / dual_v1_msg: (src, tgt, blob, incl, cons,
    TargetBlTxAlh, last, (ls, tgt id, linear terms), None or (advance terms,
    nested inclusion proofs))."""
    import wire
    sid, tid = int(src["id"]), int(tgt["id"])
    sbl, bl = int(src["bl_tx_id"]), int(tgt["bl_tx_id"])
    size, count = aht.size, len(alhs)

    def have(lo, hi):
        return count > 0 and lo >= first_tx and hi < first_tx + count

    def proof(fn, i, j):
        st, t = fn(i, j)
        assert st == 0, (i, j, st)
        return [bytes(x) for x in t]

    if sid == 0:  # the store holds no tx 0 (the library's narrowing, as for V2)
        return ERR_ILLEGAL_ARGUMENTS, None
    if sid > tid:
        return ERR_SOURCE_TX_NEWER, None
    incl = []
    if sid < bl:
        if bl > size:
            return ERR_UNEXISTENT_DATA, None
        incl = proof(aht.inclusion_proof, sid, bl)
    if sbl > bl:
        return ERR_CORRUPTED_TX_DATA, None
    cons = []
    if sbl > 0:
        if bl > size:
            return ERR_UNEXISTENT_DATA, None
        cons = proof(aht.consistency_proof, sbl, bl)
    tbl, last = bytes(32), []
    if bl > 0:
        if not have(bl, bl):
            return ERR_TX_NOT_FOUND, None
        tbl = bytes(alhs[bl - first_tx])
        if bl > size:
            return ERR_UNEXISTENT_DATA, None
        last = proof(aht.inclusion_proof, bl, bl)
    ls = max(sid, bl)
    if ls > tid:
        return ERR_SOURCE_TX_NEWER, None
    if not have(ls, tid):
        return ERR_TX_NOT_FOUND, None
    lin = (ls, tid, [bytes(alhs[ls - first_tx])] +
           [bytes(inners[k - first_tx]) for k in range(ls + 1, tid + 1)])
    a0, a1 = sbl, min(sid, bl)
    if a1 < a0:
        return ERR_SOURCE_TX_NEWER, None
    lap = None
    if a1 > a0 + 1:
        if not have(a0 + 1, a1):
            return ERR_TX_NOT_FOUND, None
        terms = [bytes(alhs[a0 + 1 - first_tx])] + \
            [bytes(inners[k - first_tx]) for k in range(a0 + 2, a1 + 1)]
        lap = (terms, [proof(aht.inclusion_proof, k, bl) for k in range(a0 + 1, a1)])
    for h in (src, tgt):
        md = _md(h, blob)
        if md and wire.parse_tx_metadata(md)[0]:
            return ERR_CORRUPTED_DATA, None
    return OK, (src, tgt, blob, incl, cons, tbl, last, lin, lap)


def go_dual_proof(src, tgt, blob, aht, first_tx, alhs, inners):
    """-> (status, the schema.DualProof message bytes; empty when it fails)"""
    import wire
    from test_gpu_pb_decode import dual_v1_msg
    st, parts = go_dual_proof_parts(src, tgt, blob, aht, first_tx, alhs, inners)
    return st, (dual_v1_msg(wire, parts) if st == OK else b"")


def dual_v1_marshal(parts):
    """DualProofToProto + Marshal (database_protoconv.go:131-211) of
    go_dual_proof_parts' parts over wire.MSG: the bytes of
    test_gpu_pb_decode.dual_v1_msg (held equal by test_dual_v1_gen_cpu.py)
    without importing a test module, for bench_workloads.py's sample check."""
    import wire
    sh, th, blob, incl, cons, tbl, last, lin, lap = parts
    M = wire.MSG["DualProof"]()
    for r, dst in ((sh, M.sourceTxHeader), (th, M.targetTxHeader)):
        st, h = wire.tx_header_msg({
            "id": int(r["id"]), "ts": int(r["ts"]), "bltxid": int(r["bl_tx_id"]),
            "blroot": r["bl_root"].tobytes(), "prevalh": r["prev_alh"].tobytes(),
            "eh": r["eh"].tobytes(), "version": int(r["version"]),
            "nentries": int(r["nentries"]), "md": _md(r, blob)})
        assert st == 0
        dst.CopyFrom(h)
    M.inclusionProof.extend(incl)
    M.consistencyProof.extend(cons)
    M.targetBlTxAlh = tbl
    M.lastInclusionProof.extend(last)
    M.linearProof.SetInParent()
    M.linearProof.sourceTxId, M.linearProof.TargetTxId = lin[0], lin[1]
    M.linearProof.terms.extend(lin[2])
    if lap is not None:
        M.LinearAdvanceProof.SetInParent()
        M.LinearAdvanceProof.linearProofTerms.extend(lap[0])
        for ip in lap[1]:
            M.LinearAdvanceProof.inclusionProofs.add(terms=ip)
    return M.SerializeToString()


# ------------------------------------------------------------ synthetic store
N_TX = 3000


def bl_of(k):
    """BlTxID of tx k: lags by 1..4 txs, except two long runs that hold it
    (700 and 71 txs: linear and advance parts of hundreds of terms).
    Monotone; txs 1..3 have none."""
    if 200 <= k <= 899:
        return 199
    if 1500 <= k <= 1570:
        return 1499
    return max(0, k - 1 - (k % 4))


class Store:
    pass


@functools.lru_cache(maxsize=None)
def synthetic_store():
    """A consistent chain of N_TX txs built with the oracle: prevAlh chain,
    BlRoot = RootAt(BlTxID), leaves = Alh; header fields and metadata vary as
    test_gpu_formats._random_headers does.  As in a Go store, a header keeps
    its metadata bytes as stored while its Alh is over their re-serialised
    form (TxMetadata.ReadFrom then Bytes(), tx.go:300-319).  -> Store with
    recs, blob, alhs, inners (lists of bytes), the oracle ahtree, and crecs /
    cblob: the same headers with the re-serialised metadata (what the oracle's
    verifier, which hashes the bytes it is given, must see)."""
    import oracle as orc
    from test_gpu_pb_decode import _canonical_md
    crecs, cblob = np.zeros(N_TX, TX_HEADER), bytearray()
    rng = np.random.default_rng(1905)
    recs = np.zeros(N_TX, TX_HEADER)
    blob = bytearray()
    aht = orc.AHtree(N_TX)
    alhs, inners = [], []
    prev = orc.sha256(b"")
    for k in range(1, N_TX + 1):
        r = recs[k - 1]
        r["id"] = k
        r["bl_tx_id"] = bl_of(k)
        if bl_of(k):
            st, root = aht.root_at(bl_of(k))
            assert st == 0
            r["bl_root"] = np.frombuffer(root, np.uint8)
        r["prev_alh"] = np.frombuffer(prev, np.uint8)
        r["eh"] = rng.integers(0, 256, 32, dtype=np.uint8)
        r["ts"] = int(rng.integers(-2**40, 2**40)) if k % 7 else 0
        r["version"] = 1 if k % 5 else 0
        ne = [0, 1, 127, 128, 300, 2**31 + 5, 2**32 - 1][k % 7]
        r["nentries"] = ne if r["version"] else ne & 0xFFFF  # v0 stores 16 bits
        md = b""
        if r["version"] == 1 and k % 3:
            kind = k % 4
            if kind == 0:
                md = bytes([0]) + int(rng.integers(0, 2**63)).to_bytes(8, "big")
            elif kind == 1:
                ln = int(rng.integers(0, 257))
                md = bytes([1]) + ln.to_bytes(2, "big") + rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            elif kind == 2:
                md = bytes([0]) + bytes(8) + bytes([1, 0, 0])  # zero id, empty extra
            else:
                md = bytes([0]) + (200).to_bytes(8, "big") + bytes([1, 0, 3]) + b"abc"
        r["md_len"], r["md_off"] = len(md), len(blob)
        blob += md
        crecs[k - 1] = r
        canon = _canonical_md(md)
        crecs[k - 1]["md_len"], crecs[k - 1]["md_off"] = len(canon), len(cblob)
        cblob += canon
        st, inner, alh = orc.tx_header_alh(crecs[k - 1], bytes(cblob))
        assert st == 0, k
        aht.append(alh)
        alhs.append(alh)
        inners.append(inner)
        prev = alh
    s = Store()
    s.recs, s.blob, s.alhs, s.inners, s.aht = recs, bytes(blob), alhs, inners, aht
    s.crecs, s.cblob = crecs, bytes(cblob)
    return s


# the pairs that hit a boundary of the writer exactly
BOUNDARY_PAIRS = [
    (1, 1), (500, 500), (N_TX, N_TX),           # src == tgt
    (1, 2), (2, 3), (1, 3),                     # tgt.BlTxID == 0: zero TargetBlTxAlh
    (3, 4), (4, 5), (199, 200),                 # nil advance proof
    (7, 9),                                     # nested proofs of <= 3 terms: 1-byte lengths
    (263, 1000), (264, 1000), (265, 1000),      # 63, 64, 65 nested proofs
    (327, 1000), (328, 1000), (329, 1000),      # 127, 128, 129: the second round
    (301, 1000), (302, 1000), (303, 1000),      # 101, 102, 103 nested proofs
    (680, 1000), (681, 1000), (682, 1000),      # 481, 482, 483 advance terms
    (899, 1000), (899, 900),                    # 700 advance terms, 699 nested proofs
] + [(s, 1000) for s in range(232, 256)] + [    # advance body across 16 383 bytes; 50..52 nested
                                                # proofs: a writer round holds 51 of 10 terms
    (200, 680), (200, 681), (200, 682),         # linear body across 16 383 bytes
    (200, 899), (150, 899),                     # 700 linear terms
    (1570, 2000), (1500, 1570), (1499, 1571),   # the second run
    (1, N_TX), (2999, N_TX),
]


@functools.lru_cache(maxsize=None)
def synthetic_pairs():
    rng = np.random.default_rng(77)
    tgt = rng.integers(1, N_TX + 1, 400)
    pairs = [(int(rng.integers(1, t + 1)), int(t)) for t in tgt]
    return tuple(pairs + BOUNDARY_PAIRS)


@functools.lru_cache(maxsize=None)
def synthetic_expected():
    """(status, parts) of every synthetic pair over the whole-store window."""
    s = synthetic_store()
    return tuple(go_dual_proof_parts(s.recs[a - 1], s.recs[b - 1], s.blob, s.aht, 1, s.alhs, s.inners)
                 for a, b in synthetic_pairs())


@functools.lru_cache(maxsize=None)
def synthetic_messages():
    import wire
    from test_gpu_pb_decode import dual_v1_msg
    return tuple(dual_v1_msg(wire, p) if st == OK else b"" for st, p in synthetic_expected())


def varint_len(v):
    return max(1, (v.bit_length() + 6) // 7)


def linear_body_len(lin):
    return 1 + varint_len(lin[0]) + 1 + varint_len(lin[1]) + 34 * len(lin[2])


def advance_body_len(lap):
    return 34 * len(lap[0]) + sum(1 + varint_len(34 * len(ip)) + 34 * len(ip) for ip in lap[1])


# ------------------------------------------------------------ status cases
SMALL = 2990  # leaves of the tree the status cases run over: the window reaches past it


def windows():
    """name -> (first_tx, alhs, inners): the whole store, and txs 150 .. 1000"""
    s = synthetic_store()
    return {"full": (1, s.alhs, s.inners), "sub": (150, s.alhs[149:1000], s.inners[149:1000])}


@functools.lru_cache(maxsize=None)
def small_tree():
    import oracle as orc
    s = synthetic_store()
    o = orc.AHtree(SMALL)
    o.append_batch(np.stack([np.frombuffer(a, np.uint8) for a in s.alhs[:SMALL]]))
    return o


@functools.lru_cache(maxsize=None)
def status_cases():
    """One hand-made pair per rule of ImmuStore.DualProof's order, and the pairs
    where two rules hold and the earlier one wins, over small_tree() -> tuple of
    (name, the restatement's status, the status worked out by hand,
    (src, tgt, blob, window name, the restatement's bytes))."""
    s = synthetic_store()
    blob = s.blob + b"\x05"  # an attribute code TxMetadata.ReadFrom rejects

    def hdr(k, **kw):
        r = s.recs[k - 1].copy()
        for f, v in kw.items():
            r[f] = v
        return r

    cases = [
        ("1: src.id == 0", hdr(5, id=0), hdr(9), "full", ERR_ILLEGAL_ARGUMENTS),
        ("2: source newer", hdr(10), hdr(5), "full", ERR_SOURCE_TX_NEWER),
        ("3: inclusion beyond the tree", hdr(10), hdr(3000, bl_tx_id=2995), "full", ERR_UNEXISTENT_DATA),
        ("4: binary linking mismatch", hdr(100, bl_tx_id=500), hdr(300), "full", ERR_CORRUPTED_TX_DATA),
        ("5: consistency beyond the tree", hdr(2996, bl_tx_id=10), hdr(2999, bl_tx_id=2995), "full",
         ERR_UNEXISTENT_DATA),
        ("6: TargetBlTxAlh outside the window", hdr(120, bl_tx_id=0), hdr(160, bl_tx_id=100), "sub",
         ERR_TX_NOT_FOUND),
        ("6: last inclusion beyond the tree", hdr(2996, bl_tx_id=0), hdr(2999, bl_tx_id=2995), "full",
         ERR_UNEXISTENT_DATA),
        ("7: linear source newer (tgt.bl > tgt.id)", hdr(10), hdr(20, bl_tx_id=25), "full",
         ERR_SOURCE_TX_NEWER),
        ("7: linear part outside the window", hdr(990), hdr(1001), "sub", ERR_TX_NOT_FOUND),
        ("8: advance source newer", hdr(10, bl_tx_id=15), hdr(30), "full", ERR_SOURCE_TX_NEWER),
        ("8: advance part outside the window", hdr(151), hdr(160), "sub", ERR_TX_NOT_FOUND),
        ("9: metadata", hdr(11, version=1, md_off=len(s.blob), md_len=1), hdr(12), "full",
         ERR_CORRUPTED_DATA),
        ("3 before 4", hdr(10, bl_tx_id=5000), hdr(2999, id=4000, bl_tx_id=3500), "full",
         ERR_UNEXISTENT_DATA),
        ("4 before 6's window miss", hdr(120, bl_tx_id=110), hdr(160, bl_tx_id=100), "sub",
         ERR_CORRUPTED_TX_DATA),
        ("6's window miss before tgt.bl > size", hdr(2000, id=3400, bl_tx_id=0),
         hdr(3000, id=3500, bl_tx_id=3300), "full", ERR_TX_NOT_FOUND),
        ("ok in the small tree", hdr(263), hdr(1000), "full", OK),
        ("ok in the sub window", hdr(265), hdr(1000), "sub", OK),
    ]
    w = windows()
    out = []
    for name, a, b, win, want in cases:
        st, raw = go_dual_proof(a, b, blob, small_tree(), *w[win])
        out.append((name, st, want, (a, b, blob, win, raw)))
    return tuple(out)
