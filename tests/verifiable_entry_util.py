"""CPU side of the VerifiableGet answer tests (TEST INFRASTRUCTURE ONLY):

* the protobuf descriptor of schema.VerifiableEntry's closure (16 messages
  with VerifiableEntry itself: the six proof messages of oracle/wire.py and ten
  declared here in the same pool), checked field by field against the
  reference's compiled descriptor (tests/golden/schema_fields_entry.json,
  written by tests/golden/make_golden_entry.py);
* a restatement of the server, db.VerifiableGet (pkg/database/database.go:
  817-896) with TxToProto-shaped Tx (database_protoconv.go:27-49), over a small
  synthetic store built with the C oracle;
* reference(): what pkg/client's verifiedGet (pkg/client/client.go:1119-1234)
  does with one answer before the signature check, composed from the protobuf
  runtime (with Go's varint rule), the C oracle and
  dual_v1_verify_util.reference.  Every expectation of
  tests/test_gpu_verifiable_entry.py comes from it.
"""
import functools
import struct

import numpy as np

from tx_util import TX_HEADER

OK, ERR_ILLEGAL_ARGUMENTS, ERR_CORRUPTED_DATA, ERR_UNSUPPORTED_TX_VERSION = 0, 2, 14, 21


# ------------------------------------------------------------------ descriptor
def _build():
    from google.protobuf import descriptor_pb2, message_factory
    import wire
    _F = descriptor_pb2.FieldDescriptorProto
    pool = wire.MSG["TxHeader"].DESCRIPTOR.file.pool
    fdp = descriptor_pb2.FileDescriptorProto(name="immudb_schema_entry.proto",
                                             package="immudb.schema", syntax="proto3",
                                             dependency=[wire.MSG["TxHeader"].DESCRIPTOR.file.name])

    def msg(name, fields):
        m = fdp.message_type.add(name=name)
        for fname, num, ftype, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=ftype, label=label)
            if tname:
                f.type_name = ".immudb.schema." + tname

    O_, R_ = _F.LABEL_OPTIONAL, _F.LABEL_REPEATED
    U64, BYT, MSG_, BOOL = _F.TYPE_UINT64, _F.TYPE_BYTES, _F.TYPE_MESSAGE, _F.TYPE_BOOL
    msg("Expiration", [("expiresAt", 1, _F.TYPE_INT64, O_, None)])
    msg("KVMetadata", [("deleted", 1, BOOL, O_, None),
                       ("expiration", 2, MSG_, O_, "Expiration"),
                       ("nonIndexable", 3, BOOL, O_, None)])
    msg("Reference", [("tx", 1, U64, O_, None), ("key", 2, BYT, O_, None),
                      ("atTx", 3, U64, O_, None), ("metadata", 4, MSG_, O_, "KVMetadata"),
                      ("revision", 5, U64, O_, None)])
    msg("Entry", [("tx", 1, U64, O_, None), ("key", 2, BYT, O_, None), ("value", 3, BYT, O_, None),
                  ("referencedBy", 4, MSG_, O_, "Reference"),
                  ("metadata", 5, MSG_, O_, "KVMetadata"), ("expired", 6, BOOL, O_, None),
                  ("revision", 7, U64, O_, None)])
    msg("TxEntry", [("key", 1, BYT, O_, None), ("hValue", 2, BYT, O_, None),
                    ("vLen", 3, _F.TYPE_INT32, O_, None), ("metadata", 4, MSG_, O_, "KVMetadata"),
                    ("value", 5, BYT, O_, None)])
    msg("ZEntry", [("set", 1, BYT, O_, None), ("key", 2, BYT, O_, None),
                   ("entry", 3, MSG_, O_, "Entry"), ("score", 4, _F.TYPE_DOUBLE, O_, None),
                   ("atTx", 5, U64, O_, None)])
    msg("Tx", [("header", 1, MSG_, O_, "TxHeader"), ("entries", 2, MSG_, R_, "TxEntry"),
               ("kvEntries", 3, MSG_, R_, "Entry"), ("zEntries", 4, MSG_, R_, "ZEntry")])
    msg("Signature", [("publicKey", 1, BYT, O_, None), ("signature", 2, BYT, O_, None)])
    msg("VerifiableTx", [("tx", 1, MSG_, O_, "Tx"), ("dualProof", 2, MSG_, O_, "DualProof"),
                         ("signature", 3, MSG_, O_, "Signature")])
    msg("VerifiableEntry", [("entry", 1, MSG_, O_, "Entry"),
                            ("verifiableTx", 2, MSG_, O_, "VerifiableTx"),
                            ("inclusionProof", 3, MSG_, O_, "InclusionProof")])
    pool.Add(fdp)
    out = {n: wire.MSG[n] for n in ("TxMetadata", "TxHeader", "InclusionProof", "DualProof",
                                    "LinearProof", "LinearAdvanceProof")}
    for m in fdp.message_type:
        out[m.name] = message_factory.GetMessageClass(
            pool.FindMessageTypeByName("immudb.schema." + m.name))
    return out


@functools.lru_cache(maxsize=None)
def messages():
    """name -> message class of the 16 messages of the closure"""
    return _build()


NEW_MESSAGES = ("VerifiableEntry", "Entry", "Reference", "KVMetadata", "Expiration",
                "VerifiableTx", "Tx", "TxEntry", "ZEntry", "Signature")


# ------------------------------------------------------------ Go's varint rule
def go_varints_ok(b, desc):
    """test_gpu_pb_decode._go_varints_ok over a descriptor: protobuf-go rejects a
    10-byte varint whose last byte is above 1, the python runtime drops the
    excess bits.  Every varint Unmarshal reads is walked -- keys, scalars,
    lengths, unknown fields and groups, and every known sub-message of `desc`
    (a google.protobuf Descriptor) recursively; all else is the runtime's."""
    def varint(i):
        v = 0
        for k in range(10):
            if i >= len(b):
                raise IndexError
            c = b[i]
            i += 1
            if k == 9 and c > 1:
                raise OverflowError
            v |= (c & 0x7f) << (7 * k)
            if not c & 0x80:
                return v, i
        raise OverflowError
    try:
        i, groups = 0, []
        while i < len(b):
            key, i = varint(i)
            f, wt = key >> 3, key & 7
            if wt == 0:
                _, i = varint(i)
            elif wt == 1:
                i += 8
            elif wt == 5:
                i += 4
            elif wt == 2:
                ln, i = varint(i)
                sub, i = b[i:i + ln], i + ln
                fd = desc.fields_by_number.get(f) if not groups else None
                if fd is not None and fd.message_type is not None and i <= len(b) and \
                        not go_varints_ok(sub, fd.message_type):
                    return False
            elif wt == 3:
                groups.append(f)
            elif wt == 4 and groups:
                groups.pop()
            if i > len(b):
                return True  # truncated: the runtime's parse rejects it too
        return True
    except OverflowError:
        return False
    except IndexError:
        return True


# ------------------------------------------------------------------ the client
def d32(b):
    return (bytes(b) + bytes(32))[:32]


def kv_metadata_bytes(md):
    """KVMetadataFromProto (database_protoconv.go:97-113) then Bytes()
    (kv_metadata.go:207-219); md: a KVMetadata message or None"""
    if md is None:
        return b""
    out = b""
    if md.deleted:
        out += b"\x00"
    if md.HasField("expiration"):
        out += b"\x01" + struct.pack(">q", md.expiration.expiresAt)
    if md.nonIndexable:
        out += b"\x02"
    return out


def entry_spec(orc, M, key, version):
    """EncodeEntrySpec / EncodeReference (meta.go:54-89) of the parsed answer M
    for request key `key`, then EntrySpecDigest_v0 / _v1
    (verification.go:257-302) -> (the entry's tx or the reference's, digest)"""
    e = M.entry
    if not e.HasField("referencedBy"):
        tx, md = e.tx, kv_metadata_bytes(e.metadata if e.HasField("metadata") else None)
        value = b"\x00" + e.value
    else:
        r = e.referencedBy
        tx, md = r.tx, kv_metadata_bytes(r.metadata if r.HasField("metadata") else None)
        value = b"\x01" + struct.pack(">Q", r.atTx) + b"\x00" + e.key
    k = b"\x00" + bytes(key)
    hval = orc.sha256(value)
    if version == 0:  # metadata ignored, not refused
        return tx, orc.sha256(k + hval)
    msg = struct.pack(">H", len(md)) + md + struct.pack(">H", len(k) & 0xffff) + k + hval
    if len(k) < 1 << 16:  # the oracle's statement of the same digest, where it can write kLen
        st, d = orc.entry_digest(1, k, md, hval)
        assert st == 0 and d == orc.sha256(msg)
    return tx, orc.sha256(msg)


def parse(raw):
    """proto.Unmarshal into schema.VerifiableEntry and the nil / version rules of
    client.go:1145-1161 in Go's order -> (status, the parsed message or None)"""
    from google.protobuf.message import DecodeError
    VE = messages()["VerifiableEntry"]
    if not go_varints_ok(raw, VE.DESCRIPTOR):
        return ERR_CORRUPTED_DATA, None
    try:
        M = VE.FromString(raw)
    except DecodeError:
        return ERR_CORRUPTED_DATA, None
    vt = M.verifiableTx
    if not (M.HasField("verifiableTx") and vt.HasField("tx") and vt.tx.HasField("header")):
        return ERR_ILLEGAL_ARGUMENTS, None
    if vt.tx.header.version not in (0, 1):  # int32, signed
        return ERR_UNSUPPORTED_TX_VERSION, None
    D = vt.dualProof
    if not (M.HasField("inclusionProof") and vt.HasField("dualProof") and
            D.HasField("sourceTxHeader") and D.HasField("targetTxHeader") and
            D.HasField("linearProof") and M.HasField("entry")):
        return ERR_ILLEGAL_ARGUMENTS, None
    return OK, M


def expect_decode(raw):
    """what mh_verifiable_entry_pb_decode_batch must give for `raw`, from the
    protobuf runtime -> (status, None or dict: entry_tx, has_ref, ref_tx,
    ref_at_tx, key, value, md, version, leaf, width (64-bit patterns), terms,
    dual (the merged DualProof message))"""
    st, M = parse(raw)
    if st:
        return st, None
    e, u = M.entry, (1 << 64) - 1
    ref = e.HasField("referencedBy")
    mdm = e.referencedBy if ref else e
    return OK, {"entry_tx": e.tx, "has_ref": ref, "ref_tx": e.referencedBy.tx,
                "ref_at_tx": e.referencedBy.atTx, "key": e.key, "value": e.value,
                "md": kv_metadata_bytes(mdm.metadata if mdm.HasField("metadata") else None),
                "version": M.verifiableTx.tx.header.version,
                "leaf": M.inclusionProof.leaf & u, "width": M.inclusionProof.width & u,
                "terms": [d32(t) for t in M.inclusionProof.terms],
                "dual": M.verifiableTx.dualProof}


def reference(raw, key, at_tx, S, state_alh):
    """verifiedGet before the signature check (client.go:1119-1213) for one
    answer -> (status, ok, new_tx, new_alh)."""
    import oracle as orc
    import wire
    from dual_v1_verify_util import _header
    from dual_v1_verify_util import reference as dual_reference
    none = (False, 0, bytes(32))
    st, M = parse(raw)
    if st:
        return (st,) + none
    D, version = M.verifiableTx.dualProof, M.verifiableTx.tx.header.version
    tx, digest = entry_spec(orc, M, key, version)
    vtx = at_tx if at_tx else tx
    fwd = S <= vtx
    hdr = D.targetTxHeader if fwd else D.sourceTxHeader
    rec, md = _header(hdr)
    if int(rec["version"]) > 1:  # innerHash panics (tx.go:283-286)
        return (OK,) + none
    st, _, alh = orc.tx_header_alh(rec, md)
    assert st == 0
    src, src_alh, tgt, tgt_alh = (S, bytes(state_alh), vtx, alh) if fwd else \
        (vtx, alh, S, bytes(state_alh))
    ip = M.inclusionProof
    u = (1 << 64) - 1
    ok = orc.htree_verify_inclusion(ip.leaf & u, ip.width & u, [d32(t) for t in ip.terms], digest,
                                    d32(hdr.eH))
    if ok and S > 0:
        dst, ok = dual_reference(wire, orc, D.SerializeToString(), src, tgt, src_alh, tgt_alh)
        assert dst == 0
    return (OK, True, tgt, tgt_alh) if ok else (OK,) + none


# ------------------------------------------------------------------ the server
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 1024)
N_TX = 48
VALUE_LENS = (0, 1, 54, 55, 56, 62, 63, 64, 118, 119, 127, 4096)  # the prefixed value's padding edges
REF_KEY_LENS = (45, 46, 54, 109)      # 10 + len = 55, 56, 64, 119
V1_KEY_LENS = (0, 1, 18, 19, 20, 1023)  # with 0 / 1 / 9 / 10 / 11 metadata bytes: 55 | 56 bytes
V0_KEY_LENS = (0, 22, 23, 24)         # 1 + len + 32 = 55, 56, 57
MD_KINDS = {0: (False, None, False), 1: (True, None, False), 9: (False, 7, False),
            10: (True, 7, False), 11: (True, 7, True)}  # by Bytes() length
EXPIRES = (0, 1, -1, 2 ** 63 - 1)


def bl_of(k):
    """BlTxID of tx k lags 1 to 4 txs (as dual_v1_gen_util.bl_of)"""
    return max(0, k - 1 - (k % 4))


def asked_leaves(w):
    """first, last (the node every odd level promotes: level 0 of an odd
    width, level 3 of 1000), its left neighbour, one in the middle"""
    return sorted({0, w - 1, max(w - 2, 0), w // 2})


class Slot:
    """one entry of the store that answers are asked for"""
    def __init__(self, tx, leaf, key, md, value=None, ref_key=None, at_tx=0):
        self.tx, self.leaf, self.key, self.md = tx, leaf, bytes(key), md
        self.value, self.ref_key, self.at_tx = value, ref_key, at_tx

    @property
    def is_ref(self):
        return self.ref_key is not None

    def stored_value(self):
        if self.is_ref:
            return b"\x01" + struct.pack(">Q", self.at_tx) + b"\x00" + self.ref_key
        return b"\x00" + self.value

    def md_bytes(self):
        d, e, n = self.md
        return (b"\x00" if d else b"") + (b"\x01" + struct.pack(">q", e) if e is not None else b"") + \
            (b"\x02" if n else b"")


def _specs(rng):
    """the entry contents the tests ask for, per header version -> (v1, v0)
    lists of Slot keyword dicts"""
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    none = (False, None, False)
    v1, v0 = [], []
    for n in VALUE_LENS:
        v1.append(dict(key=rb(8), md=none, value=rb(n)))
        v0.append(dict(key=rb(9), md=none, value=rb(n)))
    for n in REF_KEY_LENS:
        v1.append(dict(key=rb(7), md=none, ref_key=rb(n), at_tx=int(rng.integers(0, 1 << 62))))
        v0.append(dict(key=rb(7), md=none, ref_key=rb(n), at_tx=0))
    for kl in V1_KEY_LENS:
        for ml, md in MD_KINDS.items():
            v1.append(dict(key=rb(kl), md=md, value=rb(5)))
    for kl in V0_KEY_LENS:
        v0.append(dict(key=rb(kl), md=none, value=rb(3)))
    for d in (False, True):
        for e in (None, 1234567):
            for n in (False, True):  # all 8 flag combinations, on a value and on a reference
                v1.append(dict(key=rb(6), md=(d, e, n), value=rb(10)))
                v1.append(dict(key=rb(6), md=(d, e, n), ref_key=rb(12), at_tx=3))
    for e in EXPIRES:
        v1.append(dict(key=rb(5), md=(False, e, False), value=rb(9)))
    v0.append(dict(key=rb(5), md=(True, 77, True), value=rb(9)))       # metadata on a v0 answer:
    v0.append(dict(key=rb(5), md=(False, 0, False), ref_key=rb(4), at_tx=9))  # ignored
    return v1, v0


class Store:
    pass


@functools.lru_cache(maxsize=None)
def store(value_len=None):
    """48 txs: header versions alternate (and swap with every cycle of WIDTHS, so
    both versions meet every width), BlTxID lags 1-4, widths cycle through
    WIDTHS; the asked leaves hold the contents of _specs,
    the others random digests.  -> Store with recs / blob (TX_HEADER records
    with canonical metadata), alhs, inners, aht (oracle ahtree), levels[k]
    (the tx's htree levels), width[k], digests[k], slots (list of Slot).
    value_len (tools/bench_verified_get.py): every plain value has that length."""
    import oracle as orc
    rng = np.random.default_rng(4242)
    specs = {1: _specs(rng)[0], 0: None}
    specs[0] = _specs(np.random.default_rng(4243))[1]
    pos = {0: 0, 1: 0}
    s = Store()
    s.recs, blob = np.zeros(N_TX, TX_HEADER), bytearray()
    s.alhs, s.inners, s.levels, s.width, s.digests, s.slots = [], [], {}, {}, {}, []
    s.aht = orc.AHtree(N_TX)
    prev = orc.sha256(b"")
    for k in range(1, N_TX + 1):
        ver = (k + (k - 1) // len(WIDTHS)) % 2
        w = WIDTHS[(k - 1) % len(WIDTHS)]
        dig = rng.integers(0, 256, (w, 32), dtype=np.uint8)
        for leaf in asked_leaves(w):
            kw = specs[ver][pos[ver] % len(specs[ver])]
            pos[ver] += 1
            sl = Slot(k, leaf, **kw)
            if value_len is not None and not sl.is_ref:
                sl.value = rng.integers(0, 256, value_len, dtype=np.uint8).tobytes()
            hval = orc.sha256(sl.stored_value())
            key = b"\x00" + sl.key
            if ver == 0:
                d = orc.sha256(key + hval)
            else:
                md = sl.md_bytes()
                d = orc.sha256(struct.pack(">H", len(md)) + md + struct.pack(">H", len(key)) + key + hval)
            dig[leaf] = np.frombuffer(d, np.uint8)
            s.slots.append(sl)
        lv, root = orc.htree_build(dig)
        s.levels[k], s.width[k], s.digests[k] = lv, w, dig
        r = s.recs[k - 1]
        r["id"], r["bl_tx_id"], r["version"], r["nentries"] = k, bl_of(k), ver, w
        r["ts"] = 1700000000 + k
        if bl_of(k):
            st, broot = s.aht.root_at(bl_of(k))
            assert st == 0
            r["bl_root"] = np.frombuffer(broot, np.uint8)
        r["prev_alh"] = np.frombuffer(prev, np.uint8)
        r["eh"] = np.frombuffer(root, np.uint8)
        md = b""
        if ver == 1 and k % 3 == 0:  # tx metadata on some v1 headers
            md = b"\x00" + struct.pack(">Q", k)
        r["md_len"], r["md_off"] = len(md), len(blob)
        blob += md
        st, inner, alh = orc.tx_header_alh(r, bytes(blob))
        assert st == 0
        s.aht.append(alh)
        s.alhs.append(alh)
        s.inners.append(inner)
        prev = alh
    s.blob = bytes(blob)
    assert pos[1] >= len(specs[1]) and pos[0] >= len(specs[0]), (pos, len(specs[1]), len(specs[0]))
    return s


def _kvmd(M, md):
    """KVMetadataToProto (database_protoconv.go:51-67); no attribute: nil"""
    d, e, n = md
    if not d and e is None and not n:
        return
    M.SetInParent()
    M.deleted, M.nonIndexable = d, n
    if e is not None:
        M.expiration.SetInParent()
        M.expiration.expiresAt = e


@functools.lru_cache(maxsize=None)
def _tx_proto(k, s):
    """TxToProto (database_protoconv.go:27-49) of tx k of store s: header and
    entries (key, hValue, vLen, metadata; the unasked leaves carry made-up keys)"""
    import oracle as orc
    import wire
    from test_gpu_formats import _rec_hdr
    T = messages()["Tx"]()
    T.header.CopyFrom(wire.tx_header_msg(_rec_hdr(s.recs[k - 1], s.blob))[1])
    asked = {sl.leaf: sl for sl in s.slots if sl.tx == k}
    for j in range(s.width[k]):
        e = T.entries.add()
        if j in asked:
            sl = asked[j]
            e.key, e.vLen = b"\x00" + sl.key, len(sl.stored_value())
            e.hValue = orc.sha256(sl.stored_value())
            _kvmd(e.metadata, sl.md)
        else:
            e.key, e.hValue, e.vLen = b"\x00k%d" % j, s.digests[k][j].tobytes(), j
    return T


def proof_pair(sl, S):
    """the (source, target) txs of the DualProof db.VerifiableGet asks the store
    for (database.go:855-881)"""
    root = sl.tx if S == 0 else S
    return (root, sl.tx) if S <= sl.tx else (sl.tx, root)


def answer(sl, S, mutate=None, s=None, dual=None):
    """db.VerifiableGet (database.go:817-896) for slot sl with ProveSinceTx = S
    -> the VerifiableEntry message (not serialised); mutate(M) edits it first.
    s: the store (default store()); dual: the marshalled DualProof of
    proof_pair(sl, S) made elsewhere (the device's), else the restatement's"""
    import oracle as orc
    import wire
    import dual_v1_gen_util as G
    s = s or store()
    msgs = messages()
    M = msgs["VerifiableEntry"]()
    e = M.entry
    e.SetInParent()
    if sl.is_ref:  # the target entry's tx / key, and what refers to it
        e.tx, e.key, e.value = max(1, sl.tx - 1), sl.ref_key, b"the referenced value"
        e.referencedBy.tx, e.referencedBy.key, e.referencedBy.atTx = sl.tx, sl.key, sl.at_tx
        _kvmd(e.referencedBy.metadata, sl.md)
        e.revision = 1
    else:
        e.tx, e.key, e.value = sl.tx, sl.key, sl.value
        _kvmd(e.metadata, sl.md)
        e.revision = 2
    vtx = sl.tx
    st, terms = orc.htree_inclusion_proof(s.levels[vtx], s.width[vtx], sl.leaf)
    assert st == 0
    M.inclusionProof.SetInParent()
    M.inclusionProof.leaf, M.inclusionProof.width = sl.leaf, s.width[vtx]
    M.inclusionProof.terms.extend(bytes(t) for t in terms)
    if dual is None:
        from test_gpu_pb_decode import dual_v1_msg
        a, b = proof_pair(sl, S)
        st, parts = G.go_dual_proof_parts(s.recs[a - 1], s.recs[b - 1], s.blob, s.aht, 1, s.alhs,
                                          s.inners)
        assert st == 0, (a, b, st)
        dual = dual_v1_msg(wire, parts)
    M.verifiableTx.tx.CopyFrom(_tx_proto(vtx, s))
    M.verifiableTx.dualProof.ParseFromString(dual)
    if mutate:
        mutate(M)
    return M


def state_alh(S):
    return store().alhs[S - 1] if S else bytes(32)


# ---------------------------------------------------------------- hostile set
def hostile_set():
    """~1500 single-byte mutations and truncations of good answers (fixed
    seed), as test_gpu_dual_v1_verify's hostile fixture builds them -> list of
    (raw, key, at_tx, S, state_alh).  The mix -- a third untouched or mutated
    inside a bytes payload that no check reads (a TxEntry of the Tx), a third
    mutated anywhere, a third truncated or mutated near the front -- keeps each
    outcome (corrupt; decoded and refused; accepted) above 5 % of the set."""
    import oracle as orc
    s = store()
    rng = np.random.default_rng(2025)
    small = [sl for sl in s.slots if s.width[sl.tx] <= 65]
    out = []
    for k in range(500):
        sl = small[int(rng.integers(0, len(small)))]
        S = int(rng.choice([0, max(sl.tx - 1, 0), sl.tx, min(sl.tx + 1, N_TX), N_TX]))
        raw = answer(sl, S).SerializeToString()
        args = (sl.key, 0, S, state_alh(S))
        if k % 3 == 0:
            out.append((raw,) + args)  # untouched
        else:  # one bit inside the hValue of the entry's TxEntry: read by nobody
            b = bytearray(raw)
            i = raw.index(orc.sha256(sl.stored_value()))
            b[i + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
            out.append((bytes(b),) + args)
        b = bytearray(raw)
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((bytes(b),) + args)
        if k % 2 == 0:
            b = bytearray(raw)
            b[int(rng.integers(0, min(len(b), 300)))] ^= 1 << int(rng.integers(0, 8))
            out.append((bytes(b),) + args)
        else:
            out.append((raw[:int(rng.integers(0, len(raw)))],) + args)
    return out


# ------------------------------------------------------------------ test cases
# Every case is (name, raw, key, at_tx, S, state_alh); what must come out is
# reference()'s business alone.
def tag(f, wt):
    return varint(f << 3 | wt)


def varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([v & 0x7f | 0x80])
        v >>= 7
    return out + bytes([v])


def ld(f, payload):
    return tag(f, 2) + varint(len(payload)) + bytes(payload)


def split_fields(raw):
    """the top-level fields of a well-formed message without groups ->
    [(field, wire type, the field's bytes, its payload)]"""
    out, i = [], 0
    while i < len(raw):
        j, key, sh = i, 0, 0
        while True:
            key |= (raw[j] & 0x7f) << sh
            sh += 7
            j += 1
            if not raw[j - 1] & 0x80:
                break
        f, wt = key >> 3, key & 7
        if wt == 0:
            k = j
            while raw[k] & 0x80:
                k += 1
            k += 1
            pay = raw[j:k]
        elif wt == 1:
            k, pay = j + 8, raw[j:j + 8]
        elif wt == 5:
            k, pay = j + 4, raw[j:j + 4]
        else:
            assert wt == 2
            ln, sh, k = 0, 0, j
            while True:
                ln |= (raw[k] & 0x7f) << sh
                sh += 7
                k += 1
                if not raw[k - 1] & 0x80:
                    break
            pay, k = raw[k:k + ln], k + ln
        out.append((f, wt, raw[i:k], pay))
        i = k
    return out


def reverse_fields(raw, desc):
    """the same message with its fields in reverse order, in every known
    sub-message too; occurrences of one field keep their order (terms)"""
    groups = {}
    for f, wt, whole, pay in split_fields(raw):
        fd = desc.fields_by_number.get(f)
        if wt == 2 and fd is not None and fd.message_type is not None:
            whole = ld(f, reverse_fields(pay, fd.message_type))
        groups.setdefault(f, []).append(whole)
    return b"".join(b"".join(groups[f]) for f in reversed(list(groups)))


def _slot(version, ref=False, md_len=None, width_max=65, width_min=2):
    s = store()
    for sl in s.slots:
        if int(s.recs[sl.tx - 1]["version"]) == version and sl.is_ref == ref and \
                width_min <= s.width[sl.tx] <= width_max and 3 < sl.tx < N_TX - 1 and \
                (md_len is None or len(sl.md_bytes()) == md_len):
            return sl
    raise LookupError((version, ref, md_len))


def _case(name, raw, sl, S, at_tx=0, key=None, salh=None):
    return (name, bytes(raw), sl.key if key is None else key, at_tx, S,
            state_alh(S) if salh is None else salh)


def good_cases():
    """every asked entry of the store (all widths and leaves, the padding edges
    of value / reference / digest message, the metadata kinds), from the tx
    before it; every third also from no state, itself, the next and the last"""
    out = []
    for i, sl in enumerate(store().slots):
        for S in ([sl.tx - 1] if i % 3 else sorted({0, sl.tx - 1, sl.tx, min(sl.tx + 1, N_TX), N_TX})):
            out.append(_case("tx %d leaf %d S %d" % (sl.tx, sl.leaf, S),
                             answer(sl, S).SerializeToString(), sl, S))
    return out


def state_cases():
    out = []
    for sl in (_slot(1), _slot(0), _slot(1, ref=True), _slot(0, ref=True)):
        for S in sorted({0, sl.tx - 1, sl.tx, sl.tx + 1, N_TX}):
            raw = answer(sl, S).SerializeToString()
            for at in (0, sl.tx, sl.tx + 1):
                out.append(_case("tx %d S %d at %d" % (sl.tx, S, at), raw, sl, S, at_tx=at))
            out.append(_case("tx %d S %d wrong alh" % (sl.tx, S), raw, sl, S,
                             salh=bytes([1]) + state_alh(S)[1:]))
            out.append(_case("tx %d S %d alh of another tx" % (sl.tx, S), raw, sl, S,
                             salh=state_alh(max(1, S - 1) if S != 1 else 2)))
    return out


def tamper_cases():
    out = []

    def flip(b, i=0, bit=1):
        b = bytearray(b or b"\0")
        b[i] ^= bit
        return bytes(b)

    for sl in (_slot(1, md_len=11), _slot(0), _slot(1, ref=True), _slot(0, ref=True),
               _slot(1, width_min=1000, width_max=1024)):
        S = sl.tx - 2
        edits = {
            "value": lambda M: setattr(M.entry, "value", flip(M.entry.value, -1)),
            "entry.key": lambda M: setattr(M.entry, "key", flip(M.entry.key, 0, 0x80)),
            "ref.atTx": lambda M: setattr(M.entry.referencedBy, "atTx", M.entry.referencedBy.atTx ^ 1),
            "entry.tx": lambda M: setattr(M.entry, "tx", M.entry.tx + 1),
            "ref.tx": lambda M: setattr(M.entry.referencedBy, "tx", M.entry.referencedBy.tx + 1),
            "md deleted": lambda M: setattr((M.entry.referencedBy if sl.is_ref else M.entry).metadata,
                                            "deleted", not (M.entry.referencedBy if sl.is_ref
                                                            else M.entry).metadata.deleted),
            "md nonIndexable": lambda M: setattr(
                (M.entry.referencedBy if sl.is_ref else M.entry).metadata, "nonIndexable",
                not (M.entry.referencedBy if sl.is_ref else M.entry).metadata.nonIndexable),
            "md expiration": lambda M: (M.entry.referencedBy if sl.is_ref
                                        else M.entry).metadata.expiration.SetInParent(),
            "incl term": lambda M: M.inclusionProof.terms.__setitem__(
                0, flip(M.inclusionProof.terms[0], 31)),
            "target EH": lambda M: setattr(M.verifiableTx.dualProof.targetTxHeader, "eH", flip(
                M.verifiableTx.dualProof.targetTxHeader.eH, 5, 0x10)),
            "source EH": lambda M: setattr(M.verifiableTx.dualProof.sourceTxHeader, "eH", flip(
                M.verifiableTx.dualProof.sourceTxHeader.eH, 5, 0x10)),
            "dual term": lambda M: M.verifiableTx.dualProof.linearProof.terms.__setitem__(
                0, flip(M.verifiableTx.dualProof.linearProof.terms[0], 7, 2)),
            "dual last term": lambda M: M.verifiableTx.dualProof.lastInclusionProof.__setitem__(
                0, flip(M.verifiableTx.dualProof.lastInclusionProof[0], 7, 2)),
            "leaf / width swapped": lambda M: (
                lambda l, w: (setattr(M.inclusionProof, "leaf", w), setattr(M.inclusionProof, "width", l)))(
                M.inclusionProof.leaf, M.inclusionProof.width),
            "leaf -1": lambda M: setattr(M.inclusionProof, "leaf", -1),
            "width 0": lambda M: setattr(M.inclusionProof, "width", 0),
            "width -1": lambda M: setattr(M.inclusionProof, "width", -1),
            "one term more": lambda M: M.inclusionProof.terms.append(bytes(32)),
            "one term fewer": lambda M: M.inclusionProof.terms.pop(),
            "a short term": lambda M: M.inclusionProof.terms.__setitem__(0, M.inclusionProof.terms[0][:31]),
            "tx header v2 in the proof": lambda M: setattr(M.verifiableTx.dualProof.targetTxHeader,
                                                           "version", 2),
            "tx version of the other digest": lambda M: setattr(
                M.verifiableTx.tx.header, "version", 1 - M.verifiableTx.tx.header.version),
        }
        out.append(_case("untampered", answer(sl, S).SerializeToString(), sl, S))
        for name, fn in edits.items():
            for S2 in (S, 0, sl.tx + 1):
                out.append(_case("%s (tx %d S %d)" % (name, sl.tx, S2),
                                 answer(sl, S2, fn).SerializeToString(), sl, S2))
        out.append(_case("request key", answer(sl, S).SerializeToString(), sl, S,
                         key=flip(sl.key, 0, 1)))
        out.append(_case("request key longer", answer(sl, S).SerializeToString(), sl, S,
                         key=sl.key + b"\0"))
    return out


def encoding_cases():
    out = []
    D = {n: c.DESCRIPTOR for n, c in messages().items()}
    for sl in (_slot(1, md_len=11), _slot(0, ref=True), _slot(1, ref=True)):
        for S in (sl.tx - 2, sl.tx + 1, 0):
            M = answer(sl, S)
            raw = M.SerializeToString()
            E, VT, IP = (M.entry.SerializeToString(), M.verifiableTx.SerializeToString(),
                         M.inclusionProof.SerializeToString())
            TX, DP = M.verifiableTx.tx.SerializeToString(), M.verifiableTx.dualProof.SerializeToString()

            def c(name, b):
                out.append(_case("%s (tx %d S %d)" % (name, sl.tx, S), b, sl, S))

            c("plain", raw)
            c("reversed", reverse_fields(raw, D["VerifiableEntry"]))
            ef = [w for _, _, w, _ in split_fields(E)]
            c("entry in two", ld(1, b"".join(ef[:2])) + ld(2, VT) + ld(3, IP) + ld(1, b"".join(ef[2:])))
            c("entry in two, a field overridden",
              ld(1, E) + ld(2, VT) + ld(3, IP) + ld(1, ld(3, b"another value") + tag(1, 0) + varint(1)))
            c("entry overridden back", ld(1, ld(3, b"another value") + ld(2, b"k")) + ld(1, E) +
              ld(2, VT) + ld(3, IP))
            pf = [w for _, _, w, _ in split_fields(IP)]
            c("inclusionProof in two", ld(1, E) + ld(3, b"".join(pf[:3])) + ld(2, VT) +
              ld(3, b"".join(pf[3:])))
            c("inclusionProof in two, terms swapped", ld(1, E) + ld(3, b"".join(pf[3:])) + ld(2, VT) +
              ld(3, b"".join(pf[:3])))
            df = [w for _, _, w, _ in split_fields(DP)]
            h = len(df) // 2
            c("verifiableTx twice", ld(1, E) + ld(2, ld(1, TX) + ld(2, b"".join(df[:h]))) + ld(3, IP) +
              ld(2, ld(2, b"".join(df[h:]))))
            c("dualProof twice", ld(1, E) + ld(2, ld(1, TX) + ld(2, b"".join(df[:h])) +
                                               ld(2, b"".join(df[h:]))) + ld(3, IP))
            c("dualProof three times, the first empty",
              ld(1, E) + ld(2, ld(2, b"") + ld(2, b"".join(df[:1])) + ld(1, TX) +
                           ld(2, b"".join(df[1:]))) + ld(3, IP))
            # a header in two occurrences across the two halves: merged field by field
            sh = [w for _, _, w, _ in split_fields(
                M.verifiableTx.dualProof.sourceTxHeader.SerializeToString())]
            rest = b"".join(w for f, _, w, _ in split_fields(DP) if f != 1)
            c("dualProof twice, its source header in two",
              ld(1, E) + ld(2, ld(1, TX) + ld(2, ld(1, b"".join(sh[:3]))) +
                           ld(2, ld(1, b"".join(sh[3:])) + rest)) + ld(3, IP))
            c("dualProof twice, the second overrides a header id",
              ld(1, E) + ld(2, ld(1, TX) + ld(2, DP) + ld(2, ld(2, tag(1, 0) + varint(1)))) + ld(3, IP))
            unk = tag(20, 0) + varint(300) + ld(21, b"xyz") + tag(22, 5) + bytes(4) + tag(23, 1) + bytes(8)
            grp = tag(30, 3) + tag(1, 0) + varint(7) + tag(31, 3) + ld(2, b"in") + tag(31, 4) + tag(30, 4)
            c("unknown fields", unk + ld(1, E + unk) + ld(2, VT + unk) + ld(3, IP + unk) + unk)
            c("unknown group", grp + ld(1, grp + E) + ld(2, VT) + ld(3, IP + grp))
            c("mistyped known fields", tag(1, 0) + varint(5) + ld(1, E + ld(1, b"\x01\x02") + tag(2, 0) +
                                                                varint(9) + tag(4, 5) + bytes(4)) +
              ld(2, VT + tag(2, 1) + bytes(8)) + ld(3, IP + ld(1, b"\x07") + tag(3, 0) + varint(1)))
            c("10-byte varint, 64 bits", raw + tag(20, 0) + b"\xff" * 9 + b"\x01")
            c("10-byte varint overflow", raw + tag(20, 0) + b"\xff" * 9 + b"\x02")
            c("10-byte varint overflow in entry.tx", ld(1, tag(1, 0) + b"\x80" * 9 + b"\x02") + raw)
            c("varint overflow inside Tx.entries", ld(1, E) + ld(3, IP) + ld(2, ld(
                1, TX + ld(2, tag(3, 0) + b"\xff" * 9 + b"\x7f")) + ld(2, DP)))
            c("11-byte varint", raw + tag(20, 0) + b"\x80" * 10 + b"\x01")
            # the parts nobody reads, well formed, to full depth ...
            deep = ld(3, ld(4, ld(4, ld(2, tag(1, 0) + varint(5)) + tag(1, 0) + b"\x01")) +
                      tag(1, 0) + varint(4))
            good_tx = TX + ld(2, ld(1, b"k") + ld(4, tag(1, 0) + b"\x01")) + ld(3, deep[2:]) + \
                ld(4, ld(1, b"set") + deep + tag(4, 1) + bytes(8) + tag(5, 0) + varint(3))
            c("kvEntries / zEntries / signature", ld(1, E) + ld(2, ld(1, good_tx) + ld(2, DP) + ld(
                3, ld(1, b"pk") + ld(2, b"sig"))) + ld(3, IP))
            # ... and malformed: one bad byte each
            c("Tx.entries: key runs past its TxEntry", ld(1, E) + ld(2, ld(1, TX + ld(2, b"\x0a\x05ab")) +
                                                                   ld(2, DP)) + ld(3, IP))
            c("Tx.kvEntries: bad wire type", ld(1, E) + ld(2, ld(1, TX + ld(3, b"\x0e")) + ld(2, DP)) +
              ld(3, IP))
            c("Tx.zEntries: score cut short", ld(1, E) + ld(2, ld(1, TX + ld(4, tag(4, 1) + bytes(7))) +
                                                          ld(2, DP)) + ld(3, IP))
            c("Tx.zEntries: nested expiration cut", ld(1, E) + ld(2, ld(1, TX + ld(
                4, ld(3, ld(4, ld(4, ld(2, b"\x08")))))) + ld(2, DP)) + ld(3, IP))
            c("signature: length past the end", ld(1, E) + ld(2, VT + ld(3, b"\x0a\x7f")) + ld(3, IP))
            c("signature: field number 0", ld(1, E) + ld(2, VT + ld(3, b"\x00\x00")) + ld(3, IP))
            c("end group without a start", raw + tag(9, 4))
            c("group closed by another field", raw + tag(9, 3) + tag(8, 4))
            c("sub-message longer than its parent",
              ld(1, E) + ld(2, tag(1, 2) + varint(len(TX) + 5) + TX) + ld(3, IP))
            c("truncated", raw[:-3])
            c("empty", b"")
            # each nil case of the status table
            hdr = M.verifiableTx.tx.header.SerializeToString()
            c("no verifiableTx", ld(1, E) + ld(3, IP))
            c("no tx", ld(1, E) + ld(2, ld(2, DP)) + ld(3, IP))
            c("no header", ld(1, E) + ld(2, ld(1, b"".join(
                w for f, _, w, _ in split_fields(TX) if f != 1)) + ld(2, DP)) + ld(3, IP))
            c("empty header", ld(1, E) + ld(2, ld(1, ld(1, b"")) + ld(2, DP)) + ld(3, IP))
            c("no inclusionProof", ld(1, E) + ld(2, VT))
            c("empty inclusionProof", ld(1, E) + ld(2, VT) + ld(3, b""))
            c("no dualProof", ld(1, E) + ld(2, ld(1, TX)) + ld(3, IP))
            for f, what in ((1, "source header"), (2, "target header"), (7, "linearProof")):
                part = b"".join(w for g, _, w, _ in split_fields(DP) if g != f)
                c("no " + what, ld(1, E) + ld(2, ld(1, TX) + ld(2, part)) + ld(3, IP))
            c("no LinearAdvanceProof", ld(1, E) + ld(2, ld(1, TX) + ld(2, b"".join(
                w for g, _, w, _ in split_fields(DP) if g != 8))) + ld(3, IP))
            c("no entry", ld(2, VT) + ld(3, IP))
            c("empty entry", ld(1, b"") + ld(2, VT) + ld(3, IP))
            c("no header and version unknown: nil first", ld(1, E) + ld(3, IP) + ld(2, ld(2, DP)))
            for v in (2, -1, 1 << 32, (1 << 32) + 1 - 2 * int(M.verifiableTx.tx.header.version)):
                h2 = hdr + tag(8, 0) + varint(v & ((1 << 64) - 1))
                c("tx header version %d" % v, ld(1, E) + ld(3, IP) + ld(2, ld(1, ld(1, h2)) + ld(2, DP)))
                c("tx header version %d, no entry" % v, ld(3, IP) + ld(2, ld(1, ld(1, h2)) + ld(2, DP)))
    return out
