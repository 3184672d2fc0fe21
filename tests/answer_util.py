"""CPU side of the generated-answer tests (TEST INFRASTRUCTURE ONLY): what
mh_verifiable_answer_pb_batch must return, restated from the Go server.

* AnsStore: a tx log (immustore.go:1812-1924 record bytes) and its commit log
  parsed in Python; per tx the header with the rebuilt Eh, Alh and innerHash
  from the C oracle, the record verdict from oracle.txlog_validate_clog.
* expect(): db.VerifiableTxByID (database.go:1462-1528) / db.VerifiableGet
  (:817-896) for one request, the statuses in Go's order; the DualProof from
  dual_v1_gen_util.go_dual_proof_parts, the messages from the descriptor-built
  classes of verifiable_entry_util.messages(), serialised deterministically.
* synthetic(): a consistent store of 60 txs with real entries (see its
  docstring) written as record bytes.

The issue asks for one tx whose Tx body is exactly 127, 128, 16383 and 16384
bytes.  A Tx body holds a TxHeader (>= 112 bytes) and a TxEntry (>= 38), so
127 and 128 cannot be met by a Tx: the one-byte / two-byte length edge is put
on two TxEntry bodies (127 and 128 bytes) instead, and the two-byte /
three-byte edge on two Tx bodies (16383 and 16384), all in the one store.
"""
import functools
import struct

import numpy as np

import dual_v1_gen_util as G
from tx_util import TX_HEADER, clog_for, record_spans
from verifiable_entry_util import bl_of, messages

OK, ILLEGAL_ARGUMENTS, ILLEGAL_STATE, UNEXISTENT_DATA = 0, 2, 3, 5
SOURCE_TX_NEWER, CORRUPTED_DATA, TRUNCATED, BUFFER_TOO_SMALL = 10, 14, 18, 19
CORRUPTED_TX_DATA, TX_NOT_FOUND, KEY_NOT_FOUND = 24, 25, 35
ANS_TX, ANS_ENTRY = 0, 1


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def md_flags(md):
    """stored KVMetadata bytes -> (deleted, expiresAt or None, nonIndexable)"""
    d, e, n, i = False, None, False, 0
    while i < len(md):
        c = md[i]
        i += 1
        if c == 0:
            d = True
        elif c == 1:
            e, = struct.unpack_from(">q", md, i)
            i += 8
        elif c == 2:
            n = True
        else:
            raise ValueError("kv metadata")
    return d, e, n


def md_bytes(d, e, n):
    return (b"\x00" if d else b"") + (b"\x01" + struct.pack(">q", e) if e is not None else b"") + \
        (b"\x02" if n else b"")


def _fill_kvmd(M, md):
    """KVMetadataToProto (database_protoconv.go:51-67) of non-empty stored bytes"""
    d, e, n = md_flags(md)
    M.SetInParent()
    M.deleted, M.nonIndexable = d, n
    if e is not None:
        M.expiration.SetInParent()
        M.expiration.expiresAt = e


class AnsTx:
    pass


class AnsStore:
    """raw: the tx-log data; clog: its commit log (es bytes per entry); aht: the
    oracle ahtree the answers' proofs come from (default: over this log's own
    Alh values -- a mutated log passes the pristine store's)."""

    def __init__(self, raw, clog, es=12, aht=None):
        import oracle as orc
        self.raw, self.clog, self.es = bytes(raw), bytes(clog), es
        self.ntx = len(clog) // es
        spans = record_spans(self.raw)
        assert len(spans) >= self.ntx
        self.rst = [int(x) for x in orc.txlog_validate_clog(self.raw, self.clog, es)[1]]
        self.recs = np.zeros(self.ntx, TX_HEADER)
        self.txs, self.alhs, self.inners = [], [], []
        for k in range(self.ntx):
            t = self._parse(orc, spans[k][0], self.recs[k])
            self.txs.append(t)
            st, inner, alh = orc.tx_header_alh(self.recs[k], self.raw)
            assert st == 0
            self.inners.append(bytes(inner))
            self.alhs.append(bytes(alh))
        if aht is None:
            aht = orc.AHtree(max(self.ntx, 1))
            for a in self.alhs:
                aht.append(a)
        self.aht = aht

    def _parse(self, orc, p, r):
        raw = self.raw
        r["id"], r["ts"], r["bl_tx_id"] = struct.unpack_from(">QqQ", raw, p)
        r["bl_root"] = np.frombuffer(raw[p + 24:p + 56], np.uint8)
        r["prev_alh"] = np.frombuffer(raw[p + 56:p + 88], np.uint8)
        ver, = struct.unpack_from(">H", raw, p + 88)
        if ver == 0:
            ne, = struct.unpack_from(">H", raw, p + 90)
            q, ml = p + 92, 0
        else:
            ml, = struct.unpack_from(">H", raw, p + 90)
            ne, = struct.unpack_from(">I", raw, p + 92 + ml)
            q = p + 96 + ml
        r["version"], r["nentries"], r["md_len"], r["md_off"] = ver, ne, ml, p + 92 if ml else 0
        t = AnsTx()
        t.entries, digs = [], []
        for _ in range(ne):
            m_, = struct.unpack_from(">H", raw, q)
            md = raw[q + 2:q + 2 + m_]
            k_, = struct.unpack_from(">H", raw, q + 2 + m_)
            key = raw[q + 4 + m_:q + 4 + m_ + k_]
            vlen, voff = struct.unpack_from(">IQ", raw, q + 4 + m_ + k_)
            hv = raw[q + 16 + m_ + k_:q + 48 + m_ + k_]
            t.entries.append((md, key, vlen, hv))
            st, d = orc.entry_digest(ver, key, md, hv)
            assert st == 0
            digs.append(bytes(d))
            q += 48 + m_ + k_
        t.width = ne
        t.levels, root = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))
        r["eh"] = np.frombuffer(bytes(root), np.uint8)
        return t

    # ---- the messages
    @functools.lru_cache(maxsize=None)
    def tx_proto(self, T):
        """TxToProto (database_protoconv.go:27-49) of tx T, serialised"""
        import wire
        r = self.recs[T - 1]
        M = messages()["Tx"]()
        st, h = wire.tx_header_msg({
            "id": int(r["id"]), "ts": int(r["ts"]), "bltxid": int(r["bl_tx_id"]),
            "blroot": r["bl_root"].tobytes(), "prevalh": r["prev_alh"].tobytes(),
            "eh": r["eh"].tobytes(), "version": int(r["version"]),
            "nentries": int(r["nentries"]), "md": G._md(r, self.raw)})
        assert st == 0
        M.header.CopyFrom(h)
        for md, key, vlen, hv in self.txs[T - 1].entries:
            e = M.entries.add()
            e.key, e.hValue, e.vLen = key, hv, _i32(vlen)
            if md:
                _fill_kvmd(e.metadata, md)
        return M.SerializeToString(deterministic=True)

    def _read(self, lo, hi):
        """the tx reader over [lo, hi] (tx_reader.go:69-101): the first failing
        read, or an Alh link that does not hold"""
        for k in range(lo, hi + 1):
            if k < 1 or k > self.ntx:
                return TX_NOT_FOUND
            if self.rst[k - 1]:
                return self.rst[k - 1]
            if k > lo and self.recs[k - 1]["prev_alh"].tobytes() != self.alhs[k - 2]:
                return CORRUPTED_TX_DATA
        return OK

    @functools.lru_cache(maxsize=None)
    def dual(self, a, b):
        """ImmuStore.DualProof(tx a, tx b) (immustore.go:2394-2562) with its reads
        -> (status, marshalled DualProof)"""
        src, tgt = self.recs[a - 1], self.recs[b - 1]
        sid, tid = int(src["id"]), int(tgt["id"])
        sbl, bl, size = int(src["bl_tx_id"]), int(tgt["bl_tx_id"]), self.aht.size
        if sid == 0:
            return ILLEGAL_ARGUMENTS, b""
        if sid > tid:
            return SOURCE_TX_NEWER, b""
        if sid < bl and bl > size:
            return UNEXISTENT_DATA, b""
        if sbl > bl:
            return CORRUPTED_TX_DATA, b""
        if sbl > 0 and bl > size:
            return UNEXISTENT_DATA, b""
        if bl > 0:
            st = self._read(bl, bl)
            if st:
                return st, b""
            if bl > size:
                return UNEXISTENT_DATA, b""
        ls = max(sid, bl)
        if ls > tid:
            return SOURCE_TX_NEWER, b""
        st = self._read(ls, tid)
        if st:
            return st, b""
        a0, a1 = sbl, min(sid, bl)
        if a1 < a0:
            return SOURCE_TX_NEWER, b""
        if a1 > a0 + 1:
            st = self._read(a0 + 1, a1)
            if st:
                return st, b""
        st, parts = G.go_dual_proof_parts(src, tgt, self.raw, self.aht, 1, self.alhs, self.inners)
        if st:
            return st, b""
        return OK, G.dual_v1_marshal(parts)

    def index_of(self, T, key):
        for j, e in enumerate(self.txs[T - 1].entries):
            if e[1] == bytes(key):
                return j
        return None

    def expect(self, kind, T, S, key=b"", entry=b""):
        """one request -> (status, message bytes; empty when it fails)"""
        import oracle as orc
        N = self.ntx
        if S > N:
            return ILLEGAL_STATE, b""
        if T == 0:
            return ILLEGAL_ARGUMENTS, b""
        if T > N:
            return TX_NOT_FOUND, b""
        if self.rst[T - 1]:
            return self.rst[T - 1], b""
        if S > 0 and self.rst[S - 1]:
            return self.rst[S - 1], b""
        leaf = None
        if kind == ANS_ENTRY:
            leaf = self.index_of(T, key)
            if leaf is None:
                return KEY_NOT_FOUND, b""
        root = T if S == 0 else S
        a, b = (root, T) if S <= T else (T, root)
        st, dual = self.dual(a, b)
        if st:
            return st, b""
        Ms = messages()
        V = Ms["VerifiableTx"]()
        V.tx.ParseFromString(self.tx_proto(T))
        V.dualProof.ParseFromString(dual)
        if kind == ANS_TX:
            return OK, V.SerializeToString(deterministic=True)
        E = Ms["VerifiableEntry"]()
        if entry:
            E.entry.ParseFromString(bytes(entry))
        E.verifiableTx.CopyFrom(V)
        t = self.txs[T - 1]
        st, terms = orc.htree_inclusion_proof(t.levels, t.width, leaf)
        assert st == 0
        E.inclusionProof.SetInParent()
        E.inclusionProof.leaf, E.inclusionProof.width = leaf, t.width
        E.inclusionProof.terms.extend(bytes(x) for x in terms)
        return OK, E.SerializeToString(deterministic=True)

    def state_alh(self, S):
        return self.alhs[S - 1] if S else bytes(32)

    def entry_msg(self, T, j):
        """the schema.Entry db.VerifiableGet would wrap for entry j of tx T
        (a plain value stored as 0x00 || value under EncodeKey(key))"""
        md, key, _, _ = self.txs[T - 1].entries[j]
        E = messages()["Entry"]()
        E.tx, E.key, E.value, E.revision = T, key[1:], self.values[(T, j)], 1
        if md:
            _fill_kvmd(E.metadata, md)
        return E.SerializeToString(deterministic=True)


def fixture_store(fx, es=12):
    """one of the Go-written stores of tests/golden/immudb_fixtures.json"""
    import oracle as orc
    raw = bytes.fromhex(fx["txlog"])
    n = len(fx["txs"])
    clog = clog_for(raw, record_spans(raw, n), es)
    if es == 12:
        assert clog == bytes.fromhex(fx["txi"])
    pay = np.stack([np.frombuffer(bytes.fromhex(p), np.uint8) for p in fx["aht_payloads"]])
    aht = orc.AHtree(len(pay))
    aht.append_batch(pay)
    return AnsStore(raw, clog, es, aht)


# ------------------------------------------------------------------ the synthetic store
N_TX = 60
WIDTHS = (1, 2, 3, 5, 64, 65, 1000, 1024)
VLENS = (0, 1, 1 << 31, (1 << 32) - 1)
EXPIRES = (0, 1, -1, 1 << 62)
TX_BODY_TUNED = {13: 16383, 21: 16384}     # tx -> its schema.Tx body length
ENTRY_BODY_TUNED = {(14, 7): 127, (14, 8): 128}  # (tx, entry) -> its TxEntry body length
DUP_TX, DUP_FIRST, DUP_SECOND = 5, 10, 40  # tx 5: entry 40 repeats entry 10's key


def _version(k):
    return (k + (k - 1) // len(WIDTHS)) % 2


def _txmd(k):
    return b"\x00" + struct.pack(">Q", k) if _version(k) == 1 and k % 3 == 0 else b""


def _entry_md(k, j):
    if _version(k) == 0:
        return b""
    c = (j + k) % 8
    e = EXPIRES[(j // 8) % 4] if c & 2 else None
    return md_bytes(bool(c & 1), e, bool(c & 4))


def _key_len(k, j):
    if j % 97 == 5:
        return 1024
    if j % 13 == 3:
        return 100
    return 5 + (j * 7 + k) % 9


def _key(k, j, L=None):
    """stored key of entry j of tx k: 0x00 || user key, unique inside the tx"""
    if k == 1:
        return b"\x00"                      # 1 byte
    if k == 2:
        return (b"\x00a", b"\x00ab")[j]     # 2 and 3 bytes, the first a proper prefix of the second
    L = L or _key_len(k, j)
    return (b"\x00" + struct.pack(">HH", k, j) + bytes((k * 31 + j * 7 + i) & 0xff for i in range(L)))[:L]


def _entry_size(L, md, vlen):
    """framed TxEntry bytes for a key of L bytes"""
    e = messages()["TxEntry"]()
    e.key, e.hValue, e.vLen = b"k" * L, bytes(32), _i32(vlen)
    if md:
        _fill_kvmd(e.metadata, md)
    body = e.ByteSize()
    return body, 1 + len(_varint(body)) + body


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7f | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _header_size(k, w):
    import wire
    st, h = wire.tx_header_msg({"id": k, "ts": 1700000000 + k, "bltxid": bl_of(k), "blroot": bytes(32),
                                "prevalh": bytes(32), "eh": bytes(32), "version": _version(k),
                                "nentries": w, "md": _txmd(k)})
    assert st == 0
    b = h.ByteSize()
    return 1 + len(_varint(b)) + b


def _key_lens(k, w):
    """the key lengths of tx k, tuned where the store promises a body length"""
    lens = [len(_key(k, j)) for j in range(w)]
    vl = lambda j: VLENS[(j + k) % 4]  # noqa: E731
    for (tk, j), want in ENTRY_BODY_TUNED.items():
        if tk == k:
            hit = [L for L in range(5, 1025) if _entry_size(L, _entry_md(k, j), vl(j))[0] == want]
            assert hit, (k, j, want)
            lens[j] = hit[0]
    if k in TX_BODY_TUNED:
        want = TX_BODY_TUNED[k]
        size = lambda j, L: _entry_size(L, _entry_md(k, j), vl(j))[1]  # noqa: E731
        total = lambda: _header_size(k, w) + sum(size(j, lens[j]) for j in range(2, w))  # noqa: E731
        j = 2
        while want - total() > 1800:  # long keys until two tuned ones can close the gap
            lens[j] = 1000
            j += 1
        rest = total()
        hit = [(a, b) for a in range(5, 1025, 37) for b in range(5, 1025)
               if rest + size(0, a) + size(1, b) == want]
        assert hit, (k, want)
        lens[0], lens[1] = hit[0]
    return lens


@functools.lru_cache(maxsize=None)
def synthetic_log():
    """-> (raw tx-log bytes, values {(tx, entry): value}).  60 txs: widths cycle
    through WIDTHS; header versions 0 and 1 (swapping with every cycle, so both
    meet every width); tx metadata on every third v1 header; BlTxID lags 0-4
    (verifiable_entry_util.bl_of) with BlRoot from the oracle ahtree; stored
    keys of 1 to 1024 bytes; on v1 entries all eight KV-metadata flag
    combinations with expiresAt in EXPIRES; vLen in VLENS; the tuned bodies and
    the duplicate key named above."""
    import oracle as orc
    raw, values = bytearray(), {}
    aht = orc.AHtree(N_TX)
    prev = orc.sha256(b"")
    for k in range(1, N_TX + 1):
        ver, w, txmd = _version(k), WIDTHS[(k - 1) % len(WIDTHS)], _txmd(k)
        lens = _key_lens(k, w)
        ents, digs = bytearray(), []
        for j in range(w):
            key, md = _key(k, j, lens[j]), _entry_md(k, j)
            if k == DUP_TX and j == DUP_SECOND:
                key = _key(k, DUP_FIRST, lens[DUP_FIRST])
            value = b"value %d.%d" % (k, j)
            values[(k, j)] = value
            hv = orc.sha256(b"\x00" + value)
            st, d = orc.entry_digest(ver, key, md, hv)
            assert st == 0
            digs.append(bytes(d))
            ents += struct.pack(">H", len(md)) + md + struct.pack(">H", len(key)) + key
            ents += struct.pack(">IQ", VLENS[(j + k) % 4], 1000 * k + j) + hv
        eh = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))[1]
        bl = bl_of(k)
        blroot = bytes(32)
        if bl:
            st, blroot = aht.root_at(bl)
            assert st == 0
            blroot = bytes(blroot)
        ts = 1700000000 + k
        st, inner = orc.tx_inner_hash(ts, ver, txmd, w, eh, bl, blroot)
        assert st == 0
        alh = orc.tx_alh(k, prev, inner)
        hdr = struct.pack(">QqQ", k, ts, bl) + blroot + bytes(prev) + struct.pack(">H", ver)
        hdr += struct.pack(">H", w) if ver == 0 else struct.pack(">H", len(txmd)) + txmd + \
            struct.pack(">I", w)
        raw += hdr + ents + bytes(alh)
        aht.append(alh)
        prev = alh
    return bytes(raw), values


@functools.lru_cache(maxsize=None)
def synthetic(es=12):
    raw, values = synthetic_log()
    s = AnsStore(raw, clog_for(raw, record_spans(raw, N_TX), es), es)
    s.values = values
    assert not any(s.rst), s.rst
    return s


def asked_leaves(w):
    """first, last (the node every odd level promotes: width 5 leaf 4, width
    1000 leaf 999 at level 3), its left neighbour, one in the middle"""
    return sorted({0, w - 1, max(w - 2, 0), w // 2})


def synthetic_requests(s):
    """about 600 requests of both kinds -> list of (kind, T, S, key, entry):
    every tx as TX and, by the asked leaves, as ENTRY with S spread over the
    store; a hundred requests sharing one S; the same tx asked as TX and as
    ENTRY; repeats."""
    reqs = []
    N = s.ntx
    for T in range(1, N + 1):
        for S in (0, 1, max(T - 1, 1), T, min(T + 1, N), N, (T * 7) % N + 1):
            reqs.append((ANS_TX, T, S, b"", b""))
        w = s.txs[T - 1].width
        for i, j in enumerate(asked_leaves(w)):
            if T == DUP_TX and j == DUP_SECOND:
                continue
            S = (0, 1, T, N, (T * 11 + j) % N + 1)[(T + i) % 5]
            reqs.append((ANS_ENTRY, T, S, s.txs[T - 1].entries[j][1], s.entry_msg(T, j)))
    for i in range(100):  # one client state shared by a hundred requests
        T = i % N + 1
        reqs.append((ANS_TX, T, 17, b"", b"") if i % 2 else
                    (ANS_ENTRY, T, 17, s.txs[T - 1].entries[0][1], b""))
    reqs += reqs[:20]
    return reqs


def columns(reqs):
    return ([r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs], [r[3] for r in reqs],
            [r[4] for r in reqs])
