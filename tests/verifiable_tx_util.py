"""CPU side of the VerifiableTx answer tests (TEST INFRASTRUCTURE ONLY):

* a synthetic store built with the C oracle in which every entry is a real
  key / value / metadata (plain values, references, sorted-set entries);
* a restatement of the server: db.VerifiableSet / VerifiableSetReference /
  VerifiableZAdd / VerifiableTxById (pkg/database/database.go:767-814 and their
  neighbours): TxToProto (database_protoconv.go:27-49) plus the DualProof of
  (ProveSinceTx, or the tx itself if ProveSinceTx is 0; the tx);
* reference(): what pkg/client does with one such answer before the signature
  check -- VerifiedSet (client.go:1337-1391), streamVerifiedSet (streams.go:
  205-260), VerifiedSetReferenceAt (client.go:1716-1770), VerifiedZAddAt
  (:1882-1940), VerifiedTxByID (:1554-1583) -- composed from the protobuf
  runtime (with Go's varint rule), the C oracle (sha256, htree_build,
  tx_header_alh) and dual_v1_verify_util.reference.  Every expectation of
  tests/test_gpu_verifiable_tx.py comes from it, eh_out included.
"""
import functools
import struct

import numpy as np

from tx_util import TX_HEADER
from verifiable_entry_util import (EXPIRES, MD_KINDS, V1_KEY_LENS, VALUE_LENS, WIDTHS, d32,
                                   go_varints_ok, kv_metadata_bytes, ld, messages, reverse_fields,
                                   split_fields, tag, varint)

OK, ERR_ILLEGAL_ARGUMENTS, ERR_CORRUPTED_DATA, ERR_UNSUPPORTED_TX_VERSION = 0, 2, 14, 21
SET, SET_ALL, REFERENCE, ZADD, TX_BY_ID = range(5)
WRITE_KINDS = (SET, SET_ALL, REFERENCE, ZADD)
Z32 = bytes(32)
NONE_MD = (False, None, False)


# ------------------------------------------------------------------ the client
def entry_digest(orc, version, key, md, hv):
    """TxEntryDigest_v0 / _v1 (tx.go:690-731) and, on the same bytes,
    EntrySpecDigest_v0 / _v1 (verification.go:257-302; v0 ignores metadata)"""
    if version == 0:
        return orc.sha256(key + hv)
    msg = struct.pack(">H", len(md)) + md + struct.pack(">H", len(key) & 0xffff) + key + hv
    if len(key) < 1 << 16:  # the oracle's statement of the same digest, where it can write kLen
        st, d = orc.entry_digest(1, key, md, hv)
        assert st == 0 and d == orc.sha256(msg)
    return orc.sha256(msg)


def spec_entry(kind, key, value, at_tx, md):
    """EncodeEntrySpec / EncodeReference / EncodeZAdd (meta.go:54-96) of one
    request spec -> (key, metadata bytes, value)"""
    if kind in (SET, SET_ALL):
        return b"\x00" + bytes(key), md, b"\x00" + bytes(value)
    if kind == REFERENCE:
        return b"\x00" + bytes(key), b"", b"\x01" + struct.pack(">Q", at_tx) + b"\x00" + bytes(value)
    return bytes(key), b"", b""


def reference(raw, kind, specs, at_tx, S, state_alh):
    """One answer -> (status, ok, new_tx, new_alh, eh).  specs: the (key,
    value) pairs the answer owns."""
    import oracle as orc
    import wire
    from google.protobuf.message import DecodeError
    from dual_v1_verify_util import _header
    from dual_v1_verify_util import reference as dual_reference
    VT = messages()["VerifiableTx"]

    def out(st, ok=False, tx=0, alh=Z32, eh=Z32):
        return (st, ok, tx if ok else 0, alh if ok else Z32, eh)

    if not go_varints_ok(raw, VT.DESCRIPTOR):
        return out(ERR_CORRUPTED_DATA)
    try:
        M = VT.FromString(raw)
    except DecodeError:
        return out(ERR_CORRUPTED_DATA)
    D, K = M.dualProof, len(specs)
    state_alh = bytes(state_alh)
    if kind == TX_BY_ID:  # client.go:1554-1583
        if not (M.HasField("dualProof") and D.HasField("sourceTxHeader") and
                D.HasField("targetTxHeader") and D.HasField("linearProof")):
            return out(ERR_ILLEGAL_ARGUMENTS)
        fwd = S <= at_tx
        rec, md = _header(D.targetTxHeader if fwd else D.sourceTxHeader)
        if int(rec["version"]) > 1:  # innerHash panics (tx.go:283-286)
            return out(OK)
        st, _, alh = orc.tx_header_alh(rec, md)
        assert st == 0
        src, src_alh, tgt, tgt_alh = (S, state_alh, at_tx, alh) if fwd else (at_tx, alh, S, state_alh)
        ok = True
        if S > 0:
            _, ok = dual_reference(wire, orc, D.SerializeToString(), src, tgt, src_alh, tgt_alh)
        return out(OK, ok, tgt, tgt_alh)
    if not (M.HasField("tx") and M.tx.HasField("header")):
        return out(ERR_ILLEGAL_ARGUMENTS)
    h, ents = M.tx.header, M.tx.entries
    plain = kind in (SET, SET_ALL)
    if not ((h.nentries == K and len(ents) == K) if plain else h.nentries == 1):
        return out(OK)  # Go: ErrCorruptedData
    if not plain and len(ents) == 0:
        return out(ERR_ILLEGAL_ARGUMENTS)
    if h.version not in (0, 1):  # int32, signed
        return out(ERR_UNSUPPORTED_TX_VERSION)
    if not (M.HasField("dualProof") and D.HasField("targetTxHeader")):
        return out(ERR_ILLEGAL_ARGUMENTS)
    if S > 0 and not (D.HasField("sourceTxHeader") and D.HasField("linearProof")):
        return out(ERR_ILLEGAL_ARGUMENTS)
    # TxFromProto: the tree of the wire's entries
    keys = [bytes(e.key) for e in ents[:K]]
    mds = [kv_metadata_bytes(e.metadata if e.HasField("metadata") else None) for e in ents[:K]]
    if h.version == 0 and any(mds):  # ErrMetadataUnsupported: no tree, tx.Proof fails
        return out(OK)
    d = [entry_digest(orc, h.version, keys[i], mds[i], d32(ents[i].hValue)) for i in range(K)]
    _, eh = orc.htree_build(np.frombuffer(b"".join(d), np.uint8).reshape(K, 32))
    eh = bytes(eh)
    ok = True
    for i, (key, value) in enumerate(specs):
        skey, smd, sval = spec_entry(kind, key, value, at_tx, mds[i] if plain else b"")
        x = entry_digest(orc, h.version, skey, smd, orc.sha256(sval))
        if skey not in keys or d[keys.index(skey)] != x:  # Tx.IndexOf: the first match
            ok = False
    if kind == SET and mds[0][:1] == b"\x00":  # md.Deleted(), client.go:1355
        ok = False
    if eh != d32(D.targetTxHeader.eH):
        ok = False
    rec, md = _header(h)
    rec["eh"] = np.frombuffer(eh, np.uint8)
    st, _, alh = orc.tx_header_alh(rec, md)
    assert st == 0
    if ok and S > 0:
        _, ok = dual_reference(wire, orc, D.SerializeToString(), S, h.id, state_alh, alh)
    return out(OK, ok, h.id, alh, eh)


# ------------------------------------------------------------------ the server
def zadd_key(zset, score, key, at_tx):
    """WrapZAddReferenceAt (pkg/database/meta.go:98-117) over EncodeKey(key)"""
    ek = b"\x00" + bytes(key)
    return (b"\x01" + struct.pack(">Q", len(zset)) + bytes(zset) + struct.pack(">d", score) +
            struct.pack(">Q", len(ek)) + ek + struct.pack(">Q", at_tx))


class Ent:
    """one entry of the store: what was written and how it is stored"""
    def __init__(self, kind, key, value=b"", md=NONE_MD, at_tx=0, zset=b"", score=0.0):
        self.kind, self.key, self.value, self.md = kind, bytes(key), bytes(value), md
        self.at_tx, self.zset, self.score = at_tx, bytes(zset), score

    def md_bytes(self):
        d, e, n = self.md
        return (b"\x00" if d else b"") + (b"\x01" + struct.pack(">q", e) if e is not None else b"") + \
            (b"\x02" if n else b"")

    def spec(self):
        """the (key, value) pair the request passes for this entry"""
        if self.kind == ZADD:
            return zadd_key(self.zset, self.score, self.key, self.at_tx), b""
        return self.key, self.value

    def stored(self):
        return spec_entry(self.kind, *self.spec(), self.at_tx, self.md_bytes())[::2]


def bl_of(k):
    """BlTxID of tx k lags 1 to 4 txs (as dual_v1_gen_util.bl_of)"""
    return max(0, k - 1 - (k % 4))


def _one_entry_txs(rng):
    """(version, Ent) of the one-entry txs: the padding-edge value, key and
    metadata lengths of verifiable_entry_util, one reference and one ZADD
    entry per version"""
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    for ver in (0, 1):
        out.append((ver, Ent(REFERENCE, rb(7), rb(46), at_tx=int(rng.integers(0, 1 << 62)))))
        out.append((ver, Ent(ZADD, rb(9), zset=rb(5), score=-1.5 * ver + 0.25, at_tx=ver * 11)))
    for i, n in enumerate(VALUE_LENS):
        out.append((i % 2, Ent(SET, rb(8), rb(n))))
    for kl in V1_KEY_LENS:
        for md in MD_KINDS.values():
            out.append((1, Ent(SET, rb(kl), rb(5), md=md)))
    for e in EXPIRES:
        out.append((1, Ent(SET, rb(5), rb(9), md=(False, e, False))))
    return out


class Store:
    pass


N_WIDE = 2 * len(WIDTHS)


@functools.lru_cache(maxsize=None)
def store(value_len=None, widths=None):
    """N_WIDE txs whose widths cycle twice through WIDTHS (64 / 65 are the two
    sides of small_roots_fit, the only width at which build_many_dev changes
    arms; launch_small_roots' own arms go by the number of trees), header
    versions alternating and swapping with the cycle so both versions meet
    every width, then the one-entry txs of _one_entry_txs.  BlTxID lags 1-4,
    every third v1 header carries tx metadata.  Wide txs hold short values
    (every 5th v1 entry some metadata).  -> Store with recs / blob (TX_HEADER,
    canonical metadata), alhs, inners, aht, ents[k] (list of Ent), ver[k].
    value_len / widths (tools/bench_verified_set.py): every plain value has
    that length / only wide txs of those widths, version 1."""
    import oracle as orc
    rng = np.random.default_rng(5151)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    plan = []
    if widths is None:
        for k in range(1, N_WIDE + 1):
            plan.append(((k + (k - 1) // len(WIDTHS)) % 2, WIDTHS[(k - 1) % len(WIDTHS)], None))
        plan += [(ver, 1, e) for ver, e in _one_entry_txs(rng)]
    else:
        plan = [(1, w, None) for w in widths]
    mdk = list(MD_KINDS.values())
    s = Store()
    n = len(plan)
    s.recs, blob = np.zeros(n, TX_HEADER), bytearray()
    s.alhs, s.inners, s.ents, s.ver = [], [], {}, {}
    s.aht = orc.AHtree(n)
    prev = orc.sha256(b"")
    for k, (ver, w, one) in enumerate(plan, 1):
        if one is not None:
            ents = [one]
        else:
            ents = [Ent(SET, b"k%d/%d/" % (k, j) + rb(j % 7),
                        rb(value_len if value_len is not None else 1 + j % 16),
                        md=mdk[j % len(mdk)] if ver == 1 and j % 5 == 4 and widths is None else NONE_MD)
                    for j in range(w)]
        dig = np.zeros((w, 32), np.uint8)
        for j, e in enumerate(ents):
            ek, ev = e.stored()
            dig[j] = np.frombuffer(entry_digest(orc, ver, ek, e.md_bytes(), orc.sha256(ev)), np.uint8)
        _, root = orc.htree_build(dig)
        s.ents[k], s.ver[k] = ents, ver
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
    s.blob, s.n = bytes(blob), n
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
def tx_proto(k, s):
    """TxToProto (database_protoconv.go:27-49) of tx k of store s"""
    import oracle as orc
    import wire
    from test_gpu_formats import _rec_hdr
    T = messages()["Tx"]()
    T.header.CopyFrom(wire.tx_header_msg(_rec_hdr(s.recs[k - 1], s.blob))[1])
    for ent in s.ents[k]:
        e = T.entries.add()
        ek, ev = ent.stored()
        e.key, e.hValue, e.vLen = ek, orc.sha256(ev), len(ev)
        _kvmd(e.metadata, ent.md)
    return T


def proof_pair(k, S):
    """the (source, target) txs of the DualProof the server builds for tx k
    with ProveSinceTx = S"""
    root = k if S == 0 else S
    return (root, k) if S <= k else (k, root)


@functools.lru_cache(maxsize=None)
def dual_msg(a, b, s):
    import wire
    import dual_v1_gen_util as G
    from test_gpu_pb_decode import dual_v1_msg
    st, parts = G.go_dual_proof_parts(s.recs[a - 1], s.recs[b - 1], s.blob, s.aht, 1, s.alhs, s.inners)
    assert st == 0, (a, b, st)
    return dual_v1_msg(wire, parts)


def answer(k, S, mutate=None, s=None):
    """the VerifiableTx message (not serialised) the server sends for tx k with
    ProveSinceTx = S; mutate(M) edits it first"""
    s = s or store()
    M = messages()["VerifiableTx"]()
    M.tx.CopyFrom(tx_proto(k, s))
    M.dualProof.ParseFromString(dual_msg(*proof_pair(k, S), s))
    if mutate:
        mutate(M)
    return M


def state_alh(S, s=None):
    return (s or store()).alhs[S - 1] if S else Z32


def request(k, kind, s=None):
    """(kind, specs, at_tx) of the request tx k answers under `kind`"""
    s = s or store()
    ents = s.ents[k]
    if kind == TX_BY_ID:
        return kind, (), k
    if kind == SET_ALL:
        return kind, tuple(e.spec() for e in ents), 0
    return kind, (ents[0].spec(),), ents[0].at_tx if kind == REFERENCE else 0


def own_kind(k, s=None):
    """the kind a one-entry tx was written under"""
    return (s or store()).ents[k][0].kind


# ------------------------------------------------------------------ test cases
# Every case is (name, raw, kind, specs, at_tx, S, state_alh); what must come
# out is reference()'s business alone.
def case(name, raw, k, kind, S, s=None, specs=None, at_tx=None, salh=None):
    kd, sp, at = request(k, kind, s)
    return (name, bytes(raw), kd, sp if specs is None else tuple(specs), at if at_tx is None else at_tx,
            S, state_alh(S, s) if salh is None else salh)


def one_entry_txs(s=None):
    s = s or store()
    return [k for k in range(1, s.n + 1) if len(s.ents[k]) == 1]


def pick(kind, version, s=None, lo=4):
    """a one-entry tx written under `kind` with that header version"""
    s = s or store()
    for k in one_entry_txs(s):
        if k >= lo and k < s.n - 1 and own_kind(k, s) == kind and s.ver[k] == version:
            return k
    raise LookupError((kind, version))


def wide(width, version, s=None):
    s = s or store()
    for k in range(1, N_WIDE + 1):
        if len(s.ents[k]) == width and s.ver[k] == version:
            return k
    raise LookupError((width, version))


def good_cases():
    """every tx of plain values as SET_ALL (K = width), every one-entry tx under its kind,
    TX_BY_ID for every tx from both sides"""
    s = store()
    out = []
    for k in range(1, s.n + 1):
        S = k - 1
        raw = answer(k, S).SerializeToString()
        if all(e.kind == SET for e in s.ents[k]):
            out.append(case("tx %d SET_ALL S %d" % (k, S), raw, k, SET_ALL, S))
        if len(s.ents[k]) == 1:
            out.append(case("tx %d own kind S %d" % (k, S), raw, k, own_kind(k), S))
        out.append(case("tx %d TX_BY_ID S %d" % (k, S), raw, k, TX_BY_ID, S))
        S = min(k + 1, s.n)
        out.append(case("tx %d TX_BY_ID S %d" % (k, S), answer(k, S).SerializeToString(), k,
                        TX_BY_ID, S))
    return out


def state_cases():
    s = store()
    out = []
    for k, kind in ((pick(SET, 1), SET), (pick(SET, 0), SET), (pick(REFERENCE, 1), REFERENCE),
                    (pick(ZADD, 0), ZADD), (wide(17, 1), SET_ALL), (wide(65, 0), SET_ALL),
                    (pick(SET, 1), TX_BY_ID), (wide(5, 0), TX_BY_ID)):
        for S in sorted({0, k - 1, k, k + 1, s.n}):
            raw = answer(k, S).SerializeToString()
            out.append(case("tx %d kind %d S %d" % (k, kind, S), raw, k, kind, S))
            out.append(case("tx %d kind %d S %d wrong alh" % (k, kind, S), raw, k, kind, S,
                            salh=bytes([1]) + state_alh(S)[1:]))
            out.append(case("tx %d kind %d S %d alh of another tx" % (k, kind, S), raw, k, kind, S,
                            salh=state_alh(max(1, S - 1) if S != 1 else 2)))
            if kind == TX_BY_ID:
                for at in (k - 1, k + 1):
                    out.append(case("tx %d asked as %d S %d" % (k, at, S), raw, k, kind, S, at_tx=at))
    return out


def flip(b, i=0, bit=1):
    b = bytearray(b or b"\0")
    b[i] ^= bit
    return bytes(b)


def tamper_cases():
    """one edit each, at S = 0 and S > 0"""
    s = store()
    out = []

    def both(name, k, kind, fn=None, **kw):
        for S in (0, k - 2):
            out.append(case("%s (tx %d kind %d S %d)" % (name, k, kind, S),
                            answer(k, S, fn).SerializeToString(), k, kind, S, **kw))

    def ent(M, i):
        return M.tx.entries[i]

    # what the client sent
    for ver in (0, 1):
        k = pick(SET, ver)
        key, val = s.ents[k][0].spec()
        both("untampered", k, SET)
        both("sent value", k, SET, specs=[(key, flip(val, -1))])
        both("sent value longer", k, SET, specs=[(key, val + b"\0")])
        both("sent key", k, SET, specs=[(flip(key, 0, 0x80), val)])
        both("sent key longer", k, SET, specs=[(key + b"\0", val)])
        k = pick(REFERENCE, ver)
        key, val = s.ents[k][0].spec()
        both("untampered", k, REFERENCE)
        both("referenced key", k, REFERENCE, specs=[(key, flip(val, 3, 4))])
        both("at_tx", k, REFERENCE, at_tx=s.ents[k][0].at_tx ^ 1)
        both("reference asked as SET", k, SET)
        k = pick(ZADD, ver)
        key, _ = s.ents[k][0].spec()
        both("untampered", k, ZADD)
        for i in (0, 9, len(key) - 1):
            both("ZADD key byte %d" % i, k, ZADD, specs=[(flip(key, i), b"")])
        both("ZADD asked with a value: ignored", k, ZADD, specs=[(key, b"v")])
    # one bit of one entry's hValue or key, first / middle / last leaf
    for w, ver in ((3, 0), (3, 1), (64, 0), (65, 1), (1000, 0), (1000, 1)):
        k = wide(w, ver)
        for i in (0, w // 2, w - 1):
            both("hValue of leaf %d" % i, k, SET_ALL,
                 lambda M, i=i: setattr(ent(M, i), "hValue", flip(ent(M, i).hValue, 31, 0x40)))
            both("key of leaf %d" % i, k, SET_ALL,
                 lambda M, i=i: setattr(ent(M, i), "key", flip(ent(M, i).key, -1, 2)))
    # an entry's metadata
    k = pick(SET, 1)
    both("deleted on SET", k, SET, lambda M: setattr(ent(M, 0).metadata, "deleted", True))
    both("deleted on SET_ALL", k, SET_ALL, lambda M: setattr(ent(M, 0).metadata, "deleted", True))
    both("expiration added", k, SET, lambda M: ent(M, 0).metadata.expiration.SetInParent())
    both("nonIndexable", k, SET, lambda M: setattr(ent(M, 0).metadata, "nonIndexable", True))
    both("empty metadata message", k, SET, lambda M: ent(M, 0).metadata.SetInParent())
    k = pick(SET, 0)
    both("version 0 with entry metadata", k, SET,
         lambda M: setattr(ent(M, 0).metadata, "nonIndexable", True))
    both("version 0 with an empty metadata message", k, SET, lambda M: ent(M, 0).metadata.SetInParent())
    k = wide(9, 0)
    both("version 0 with metadata on the last entry", k, SET_ALL,
         lambda M: setattr(ent(M, 8).metadata, "deleted", True))
    # counts and order
    for k, kind in ((pick(SET, 1), SET), (wide(4, 0), SET_ALL), (wide(17, 1), SET_ALL),
                    (pick(REFERENCE, 1), REFERENCE), (pick(ZADD, 0), ZADD)):
        both("nentries + 1", k, kind, lambda M: setattr(M.tx.header, "nentries", M.tx.header.nentries + 1))
        both("nentries - 1", k, kind, lambda M: setattr(M.tx.header, "nentries", M.tx.header.nentries - 1))
        both("nentries 0", k, kind, lambda M: setattr(M.tx.header, "nentries", 0))
        both("an entry appended", k, kind, lambda M: M.tx.entries.add(key=b"\x00more", hValue=Z32))
        both("an entry dropped", k, kind, lambda M: M.tx.entries.pop())
        both("the first entry dropped", k, kind, lambda M: M.tx.entries.pop(0))

    def retarget(M):
        """the target header's eH follows the edited entries, so that without a
        state only the spec checks decide (with one, the DualProof refuses)"""
        K = len(M.tx.entries)
        eh = reference(M.SerializeToString(), SET_ALL, ((b"", b""),) * K, 0, 0, Z32)[4]
        M.dualProof.targetTxHeader.eH = eh

    def swap(i, j):
        def fn(M):
            a, b = ent(M, i).SerializeToString(), ent(M, j).SerializeToString()
            ent(M, i).ParseFromString(b)
            ent(M, j).ParseFromString(a)
            retarget(M)
        return fn

    k = wide(7, 1)
    both("entries 0 / 1 swapped, equal metadata", k, SET_ALL, swap(0, 1))
    both("entries 3 / 4 swapped, different metadata", k, SET_ALL, swap(3, 4))
    both("entries 0 / 6 swapped, version 0", wide(7, 0), SET_ALL, swap(0, 6))

    def dup(i, j, also_hv):
        def fn(M):  # entry j takes entry i's key (and hValue): a duplicate key
            ent(M, j).key = ent(M, i).key
            if also_hv:
                ent(M, j).hValue = ent(M, i).hValue
                ent(M, j).metadata.CopyFrom(ent(M, i).metadata)
                if not ent(M, i).HasField("metadata"):
                    ent(M, j).ClearField("metadata")
            retarget(M)
        return fn

    k = wide(5, 1)
    sp = list(request(k, SET_ALL)[1])
    both("duplicate keys, the first matching", k, SET_ALL, dup(1, 2, True), specs=sp[:2] + [sp[1]] + sp[3:])
    both("duplicate keys, only the second matching", k, SET_ALL, dup(2, 1, False),
         specs=sp[:1] + [sp[2]] + sp[2:])
    # headers
    k = wide(8, 1)
    for kk, kind in ((pick(SET, 0), SET), (k, SET_ALL), (pick(ZADD, 1), ZADD)):
        both("wire eH flipped: must not matter", kk, kind,
             lambda M: setattr(M.tx.header, "eH", flip(M.tx.header.eH, 5, 0x10)))
        both("wire eH empty: must not matter", kk, kind, lambda M: M.tx.header.ClearField("eH"))
        both("target header eH flipped", kk, kind,
             lambda M: setattr(M.dualProof.targetTxHeader, "eH", flip(M.dualProof.targetTxHeader.eH, 5, 0x10)))
        both("header id", kk, kind, lambda M: setattr(M.tx.header, "id", M.tx.header.id + 1))
        both("header ts", kk, kind, lambda M: setattr(M.tx.header, "ts", M.tx.header.ts + 1))
        both("header blTxId", kk, kind, lambda M: setattr(M.tx.header, "blTxId", M.tx.header.blTxId + 1))
        both("header blRoot", kk, kind, lambda M: setattr(M.tx.header, "blRoot", flip(M.tx.header.blRoot, 0, 1)))
        both("header prevAlh", kk, kind,
             lambda M: setattr(M.tx.header, "prevAlh", flip(M.tx.header.prevAlh, 31, 1)))
        both("header version of the other digest", kk, kind,
             lambda M: setattr(M.tx.header, "version", 1 - M.tx.header.version))
        both("header metadata", kk, kind,
             lambda M: setattr(M.tx.header.metadata, "truncatedTxID", M.tx.header.metadata.truncatedTxID + 5))
        both("header metadata extra", kk, kind, lambda M: setattr(M.tx.header.metadata, "extra", b"xy"))
        both("header metadata extra too long: dropped", kk, kind,
             lambda M: setattr(M.tx.header.metadata, "extra", bytes(257)))
        both("dual linear term", kk, kind, lambda M: M.dualProof.linearProof.terms.__setitem__(
            0, flip(M.dualProof.linearProof.terms[0], 7, 2)))
        both("dual target header ts", kk, kind, lambda M: setattr(
            M.dualProof.targetTxHeader, "ts", M.dualProof.targetTxHeader.ts + 1))
        both("dual target header version 2", kk, kind,
             lambda M: setattr(M.dualProof.targetTxHeader, "version", 2))
        for v in (2, -1, 1 << 32):
            hv = varint(v & ((1 << 64) - 1))

            def setver(raw, hv=hv):  # on the wire: the runtime's int32 cannot hold 2^32
                f = {f: pay for f, _, _, pay in split_fields(raw)}
                tx = {f: pay for f, _, _, pay in split_fields(f[1])}
                rest = b"".join(w for g, _, w, _ in split_fields(f[1]) if g != 1)
                return ld(1, ld(1, tx[1] + tag(8, 0) + hv) + rest) + ld(2, f[2])

            for S in (0, kk - 2):
                out.append(case("header version %d (tx %d kind %d S %d)" % (v, kk, kind, S),
                                setver(answer(kk, S).SerializeToString()), kk, kind, S))
    for kk in (pick(SET, 1), wide(8, 0)):
        for S in (kk - 2, kk + 1):
            for name, fn in (
                    ("TX_BY_ID: its tx is not looked at", lambda M: M.ClearField("tx")),
                    ("TX_BY_ID: target header ts", lambda M: setattr(
                        M.dualProof.targetTxHeader, "ts", M.dualProof.targetTxHeader.ts + 1)),
                    ("TX_BY_ID: source header ts", lambda M: setattr(
                        M.dualProof.sourceTxHeader, "ts", M.dualProof.sourceTxHeader.ts + 1)),
                    ("TX_BY_ID: target header version 2", lambda M: setattr(
                        M.dualProof.targetTxHeader, "version", 2)),
                    ("TX_BY_ID: source header version 2", lambda M: setattr(
                        M.dualProof.sourceTxHeader, "version", 2))):
                out.append(case("%s (tx %d S %d)" % (name, kk, S), answer(kk, S, fn).SerializeToString(),
                                kk, TX_BY_ID, S))
    return out


def encoding_cases():
    """verifiable_entry_util.encoding_cases re-rooted at VerifiableTx, every nil
    case of the status table, and the masked cases"""
    out = []
    D = {n: c.DESCRIPTOR for n, c in messages().items()}
    for k, kind in ((pick(SET, 1), SET), (wide(4, 0), SET_ALL), (pick(REFERENCE, 0), REFERENCE),
                    (pick(ZADD, 1), ZADD), (wide(3, 1), TX_BY_ID)):
        for S in (k - 2, 0):
            M = answer(k, S)
            raw = M.SerializeToString()
            TX, DP = M.tx.SerializeToString(), M.dualProof.SerializeToString()
            HDR = M.tx.header.SerializeToString()
            ENTS = b"".join(w for f, _, w, _ in split_fields(TX) if f == 2)

            def c(name, b):
                out.append(case("%s (tx %d kind %d S %d)" % (name, k, kind, S), b, k, kind, S))

            c("plain", raw)
            c("reversed", reverse_fields(raw, D["VerifiableTx"]))
            hf = [w for _, _, w, _ in split_fields(HDR)]
            c("tx in two: header, then entries", ld(1, ld(1, HDR)) + ld(2, DP) + ld(1, ENTS))
            e0 = len(split_fields(ENTS)[0][2])  # the first entry, then the others
            c("tx in two: entries split across occurrences",
              ld(1, ld(1, HDR) + ENTS[:e0]) + ld(2, DP) + ld(1, ENTS[e0:]))
            c("header in two", ld(1, ld(1, b"".join(hf[:3])) + ENTS + ld(1, b"".join(hf[3:]))) + ld(2, DP))
            c("header in two, a field overridden",
              ld(1, ld(1, HDR) + ENTS) + ld(2, DP) + ld(1, ld(1, tag(3, 0) + varint(5))))
            c("header overridden back", ld(1, ld(1, tag(3, 0) + varint(5) + ld(2, b"p"))) +
              ld(1, ld(1, HDR) + ENTS) + ld(2, DP))
            c("an entry's key overridden inside the entry",
              ld(1, ld(1, HDR) + ld(2, ld(1, b"other")) + ENTS) + ld(2, DP))
            df = [w for _, _, w, _ in split_fields(DP)]
            h = len(df) // 2
            c("dualProof twice", ld(1, TX) + ld(2, b"".join(df[:h])) + ld(2, b"".join(df[h:])))
            c("dualProof three times, the first empty",
              ld(2, b"") + ld(2, b"".join(df[:1])) + ld(1, TX) + ld(2, b"".join(df[1:])))
            sh = [w for _, _, w, _ in split_fields(M.dualProof.sourceTxHeader.SerializeToString())]
            rest = b"".join(w for f, _, w, _ in split_fields(DP) if f != 1)
            c("dualProof twice, its source header in two",
              ld(1, TX) + ld(2, ld(1, b"".join(sh[:3]))) + ld(2, ld(1, b"".join(sh[3:])) + rest))
            c("dualProof twice, the second overrides the target eH",
              ld(1, TX) + ld(2, DP) + ld(2, ld(2, ld(5, Z32))))
            unk = tag(20, 0) + varint(300) + ld(21, b"xyz") + tag(22, 5) + bytes(4) + tag(23, 1) + bytes(8)
            grp = tag(30, 3) + tag(1, 0) + varint(7) + tag(31, 3) + ld(2, b"in") + tag(31, 4) + tag(30, 4)
            c("unknown fields", unk + ld(1, unk + ld(1, HDR + unk) + ENTS + unk) + ld(2, DP + unk) + unk)
            c("unknown group", grp + ld(1, grp + TX) + ld(2, DP) + grp)
            c("mistyped known fields", tag(1, 0) + varint(5) + ld(1, TX + tag(1, 0) + varint(9) +
                                                                tag(2, 5) + bytes(4)) +
              ld(2, DP + tag(1, 1) + bytes(8)) + tag(2, 0) + varint(1))
            c("mistyped header fields", ld(1, ld(1, HDR + ld(1, b"\x01\x02") + tag(5, 0) + varint(9) +
                                                 ld(8, b"\x07")) + ENTS) + ld(2, DP))
            c("10-byte varint, 64 bits", raw + tag(20, 0) + b"\xff" * 9 + b"\x01")
            c("10-byte varint overflow", raw + tag(20, 0) + b"\xff" * 9 + b"\x02")
            c("10-byte varint overflow in header.id", ld(1, ld(1, tag(1, 0) + b"\x80" * 9 + b"\x02")) + raw)
            c("varint overflow inside Tx.entries", ld(1, TX + ld(2, tag(3, 0) + b"\xff" * 9 + b"\x7f")) +
              ld(2, DP))
            c("11-byte varint", raw + tag(20, 0) + b"\x80" * 10 + b"\x01")
            # the parts nobody reads, well formed, to full depth ...
            deep = ld(3, ld(4, ld(4, ld(2, tag(1, 0) + varint(5)) + tag(1, 0) + b"\x01")) +
                      tag(1, 0) + varint(4))
            good_tx = TX + ld(3, deep[2:]) + \
                ld(4, ld(1, b"set") + deep + tag(4, 1) + bytes(8) + tag(5, 0) + varint(3))
            c("kvEntries / zEntries / signature", ld(1, good_tx) + ld(2, DP) + ld(
                3, ld(1, b"pk") + ld(2, b"sig")))
            c("vLen and value of an entry: read by nobody",
              ld(1, ld(1, HDR) + b"".join(ld(2, p + tag(3, 0) + varint(77) + ld(5, b"val"))
                                         for _, _, _, p in split_fields(ENTS))) + ld(2, DP))
            # ... and malformed: one bad byte each
            c("Tx.entries: key runs past its TxEntry", ld(1, TX + ld(2, b"\x0a\x05ab")) + ld(2, DP))
            c("Tx.entries: metadata expiration cut", ld(1, TX + ld(2, ld(4, ld(2, b"\x08")))) + ld(2, DP))
            c("Tx.kvEntries: bad wire type", ld(1, TX + ld(3, b"\x0e")) + ld(2, DP))
            c("Tx.zEntries: score cut short", ld(1, TX + ld(4, tag(4, 1) + bytes(7))) + ld(2, DP))
            c("Tx.zEntries: nested expiration cut", ld(1, TX + ld(
                4, ld(3, ld(4, ld(4, ld(2, b"\x08")))))) + ld(2, DP))
            c("header metadata cut", ld(1, ld(1, HDR + ld(9, b"\x12\x05ab")) + ENTS) + ld(2, DP))
            c("signature: length past the end", raw + ld(3, b"\x0a\x7f"))
            c("signature: field number 0", raw + ld(3, b"\x00\x00"))
            c("dualProof: nested inclusion proof cut", ld(1, TX) + ld(2, DP + ld(8, ld(2, b"\x1a\x21"))))
            c("end group without a start", raw + tag(9, 4))
            c("group closed by another field", raw + tag(9, 3) + tag(8, 4))
            c("sub-message longer than its parent", ld(1, tag(1, 2) + varint(len(HDR) + 5) + HDR) + ld(2, DP))
            c("truncated", raw[:-3])
            c("truncated inside the tx", raw[:len(TX) // 2])
            c("empty", b"")
            # each nil case of the status table
            c("no tx", ld(2, DP))
            c("no header", ld(1, ENTS) + ld(2, DP))
            c("empty header", ld(1, ld(1, b"") + ENTS) + ld(2, DP))
            c("empty tx", ld(1, b"") + ld(2, DP))
            c("no entries", ld(1, ld(1, HDR)) + ld(2, DP))
            c("no dualProof", ld(1, TX))
            c("empty dualProof", ld(1, TX) + ld(2, b""))
            for f, what in ((1, "source header"), (2, "target header"), (7, "linearProof")):
                part = b"".join(w for g, _, w, _ in split_fields(DP) if g != f)
                c("no " + what, ld(1, TX) + ld(2, part))
            c("no LinearAdvanceProof", ld(1, TX) + ld(2, b"".join(
                w for g, _, w, _ in split_fields(DP) if g != 8)))
            # the masked cases
            two = HDR + tag(8, 0) + varint(2)
            c("count failure with version 2",
              ld(1, ld(1, two + tag(4, 0) + varint(len(split_fields(ENTS)) + 1)) + ENTS) + ld(2, DP))
            c("no header and version unknown: nil first", ld(2, DP) + ld(1, ENTS))
            c("no entries with version 2", ld(1, ld(1, two)) + ld(2, DP))
            c("version 2 and no dualProof: the version first", ld(1, ld(1, two) + ENTS))
            first = split_fields(ENTS)[0]
            bad = ld(2, first[3] + ld(2, Z32))  # the first entry's hValue replaced
            c("inclusion failure with no dualProof",
              ld(1, ld(1, HDR) + bad + ENTS[len(first[2]):]))
            c("inclusion failure with no target header", ld(1, ld(1, HDR) + bad + ENTS[len(first[2]):]) +
              ld(2, b"".join(w for g, _, w, _ in split_fields(DP) if g != 2)))
    return out


@functools.lru_cache(maxsize=None)
def hostile_set():
    """~1500 answers (fixed seed), built like verifiable_entry_util.hostile_set:
    a third untouched or harmlessly edited (vLen, kvEntries, entries beyond K of
    a REFERENCE answer), a third with one byte mutated anywhere, a third
    truncated or with one bit flipped near the front.  Small txs and one-entry
    txs: in a short message a random byte more often hits structure than
    payload, which keeps each outcome (corrupt; decoded and refused; accepted)
    above 5 % of the set (tests/test_verifiable_tx_cpu.py holds it there)."""
    s = store()
    rng = np.random.default_rng(2026)
    small = [(k, SET_ALL) for k in range(4, N_WIDE + 1) if len(s.ents[k]) <= 9] + \
        [(k, own_kind(k)) for k in one_entry_txs() if 4 <= k < s.n - 1] + \
        [(k, TX_BY_ID) for k in one_entry_txs() if 4 <= k < s.n - 1][::3]
    out = []
    for i in range(500):
        k, kind = small[int(rng.integers(0, len(small)))]
        S = int(rng.choice([0, k - 1, k - 1, k - 2, k, min(k + 1, s.n), s.n]))
        M = answer(k, S)
        raw = M.SerializeToString()

        def put(b, S=S, k=k, kind=kind):
            out.append(case("hostile %d" % len(out), b, k, kind, S))

        if i % 3 == 0:
            put(raw)
        elif i % 3 == 1:  # bytes nobody reads
            M2 = answer(k, S)
            M2.tx.entries[int(rng.integers(0, len(M2.tx.entries)))].vLen = int(rng.integers(0, 1 << 20))
            M2.tx.kvEntries.add(key=b"kv", value=rng.integers(0, 256, 9, dtype=np.uint8).tobytes())
            put(M2.SerializeToString())
        else:
            M2 = answer(k, S)
            if kind in (REFERENCE, ZADD):
                M2.tx.entries.add(key=b"\x00beyond K", hValue=rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            else:
                M2.tx.kvEntries.add(key=b"k")
            put(M2.SerializeToString())
        b = bytearray(raw)
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        put(bytes(b))
        if i % 2 == 0:
            b = bytearray(raw)
            b[int(rng.integers(0, min(len(b), 300)))] ^= 1 << int(rng.integers(0, 8))
            put(bytes(b))
        else:
            put(raw[:int(rng.integers(0, len(raw)))])
    return out


@functools.lru_cache(maxsize=None)
def expectations(cases_fn):
    """the cases of one generator with reference()'s answers, computed once"""
    cases = cases_fn()
    return cases, [reference(*c[1:]) for c in cases]


def check(got, cases, want):
    """got: (status, ok, new_tx, new_alh, eh) arrays of the device"""
    st, ok, ntx, nalh, eh = got
    bad = []
    for i, (c, w) in enumerate(zip(cases, want)):
        g = (int(st[i]), bool(ok[i]), int(ntx[i]), bytes(nalh[i]), bytes(eh[i]))
        if g != w:
            bad.append((c[0], g[:3], w[:3], g[3] == w[3], g[4] == w[4]))
    assert not bad, (len(bad), bad[:8])


def columns(cases):
    """-> the arguments of txlayer.verify_verifiable_tx_pb_batch"""
    return ([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
            [c[4] for c in cases], [c[5] for c in cases], [c[6] for c in cases])
