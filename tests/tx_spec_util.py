"""CPU side of the EntriesSpec answer tests (TEST INFRASTRUCTURE ONLY):
mh_tx_answer_pb_batch's contract (include/immustore_merkle.h) restated in
Python from the Go server.

* SpecStore: an export_util.ExpStore (tx log, commit log, value-log windows)
  with the answer_util.AnsStore over the same logs (headers with the rebuilt
  Eh, Alh values, the DualProof restatement the answer tests use).
* serialize_tx(): db.serializeTx (database.go:1080-1231) with
  ImmuStore.ReadValue / readValueAt (immustore.go:3149-3240), the message
  built with the protobuf runtime from verifiable_entry_util.messages() and
  serialised by it; hashes through the C oracle.
* expect_one() / expect(): db.TxByID (:1034-1063) and db.VerifiableTxByID
  (:1462-1528) per request, the statuses in Go's order, then off.
* synthetic(): a consistent chain of about 40 txs written as record bytes (see
  its docstring).  Every expectation of tests/test_gpu_tx_spec.py comes from
  expect() over it, never from the library.
"""
import functools
import struct

import numpy as np

import answer_util as A
import export_util as X
from verifiable_entry_util import messages

OK, ILLEGAL_ARGUMENTS, ILLEGAL_STATE, CORRUPTED_DATA = 0, 2, 3, 14
BUFFER_TOO_SMALL, TX_NOT_FOUND, EOF = 19, 25, 36
TXA_TX, TXA_VERIFIABLE = 0, 1
EXCLUDE, ONLY_DIGEST, RAW_VALUE, RESOLVE = 0, 1, 2, 3  # schema.EntryTypeAction
NOW = 1800000000


class SpecStore:
    def __init__(self, exp):
        self.exp = exp
        self.ntx = exp.ntx

    @functools.cached_property
    def ans(self):
        a = A.AnsStore(self.exp.raw, self.exp.clog, self.exp.es)
        a.rst = list(self.exp.rst)  # (the ExpStore's verdicts know its max_entries)
        return a

    @functools.lru_cache(maxsize=None)
    def entries(self, T):
        """the entries of tx T as its record stores them: (md, key, vlen, voff, hval)"""
        raw = self.exp.raw
        p, = struct.unpack_from(">Q", self.exp.clog, (T - 1) * self.exp.es)
        ver, = struct.unpack_from(">H", raw, p + 88)
        if ver == 0:
            ne, = struct.unpack_from(">H", raw, p + 90)
            q = p + 92
        else:
            ml, = struct.unpack_from(">H", raw, p + 90)
            ne, = struct.unpack_from(">I", raw, p + 92 + ml)
            q = p + 96 + ml
        out = []
        for _ in range(ne):
            m_, = struct.unpack_from(">H", raw, q)
            k_, = struct.unpack_from(">H", raw, q + 2 + m_)
            vlen, voff = struct.unpack_from(">IQ", raw, q + 4 + m_ + k_)
            out.append((raw[q + 2:q + 2 + m_], raw[q + 4 + m_:q + 4 + m_ + k_], vlen, voff,
                        raw[q + 16 + m_ + k_:q + 48 + m_ + k_]))
            q += 48 + m_ + k_
        return out

    def header_msg(self, T):
        """TxHeaderToProto of tx T's header, Eh the rebuilt root"""
        import dual_v1_gen_util as G
        import wire
        r = self.ans.recs[T - 1]
        st, h = wire.tx_header_msg({
            "id": int(r["id"]), "ts": int(r["ts"]), "bltxid": int(r["bl_tx_id"]),
            "blroot": r["bl_root"].tobytes(), "prevalh": r["prev_alh"].tobytes(),
            "eh": r["eh"].tobytes(), "version": int(r["version"]),
            "nentries": int(r["nentries"]), "md": G._md(r, self.exp.raw)})
        assert st == 0
        return h


def _entry_msg(M, md, key, vlen, hv):
    """TxEntryToProto (database_protoconv.go:39-49) appended to M.entries"""
    e = M.entries.add()
    e.key, e.hValue, e.vLen = key, hv, A._i32(vlen)
    if md:
        A._fill_kvmd(e.metadata, md)
    return e


def read_value(store, md, vlen, voff, hv, now):
    """ImmuStore.ReadValue (immustore.go:3149-3179) -> (status, value or None,
    expired)"""
    import oracle as orc
    if md:
        _, exp, _ = A.md_flags(md)
        if exp is not None and exp <= now:  # !expiresAt.After(now)
            return OK, None, True
    if vlen == 0:
        return OK, None, False  # no read, no digest check
    cls, val = store.exp.value_class(vlen, voff)
    if cls == X.TRUNC:
        return EOF, None, False
    if cls == X.NOVLOG:
        return ILLEGAL_STATE, None, False
    if orc.sha256(val) != hv:
        return CORRUPTED_DATA, None, False
    return OK, val, False


@functools.lru_cache(maxsize=None)
def serialize_tx(store, T, spec, now=NOW):
    """db.serializeTx(tx T, spec) -> (status, marshalled schema.Tx, sized).
    spec: None (nil EntriesSpec) or (kv, z, sql), each an action or None (a nil
    EntryTypeSpec).  status: that of the first failing entry in record order.
    sized: no entry fails without a hash, so the answer keeps its range; bytes:
    the message when status is OK, else -- sized -- as many zero bytes as the
    message would have."""
    if spec is None:
        return OK, store.ans.tx_proto(T), True
    M = messages()["Tx"]()
    M.header.CopyFrom(store.header_msg(T))
    status, sized = OK, True
    for md, key, vlen, voff, hv in store.entries(T):
        st, early = OK, False
        if not key:
            st, early = ILLEGAL_STATE, True  # Go: e.Key()[0] panics
        else:
            act = spec[key[0]] if key[0] <= 2 else None
            if act is None or act == EXCLUDE:
                continue
            if act == ONLY_DIGEST:
                _entry_msg(M, md, key, vlen, hv)
                continue
            if act == RESOLVE:
                assert key[0] == 2, "kv / z RESOLVE is refused before any device work"
                st, early = ILLEGAL_ARGUMENTS, True
            else:
                st, val, expired = read_value(store, md, vlen, voff, hv, now)
                if expired:
                    continue
                early = st in (EOF, ILLEGAL_STATE)
                if st == OK or st == CORRUPTED_DATA:
                    e = _entry_msg(M, md, key, vlen, hv)
                    if vlen:
                        e.value = val if st == OK else bytes(vlen)
        if st and not status:
            status = st
        sized = sized and not early
    if not sized:
        return status, b"", False
    msg = M.SerializeToString(deterministic=True)
    return status, (msg if status == OK else bytes(len(msg))), True


def expect_one(store, kind, T, S, spec, now=NOW):
    """one request -> (status, message bytes (b"" unless OK), length of its range)"""
    N = store.ntx
    a = store.ans
    dual = b""
    if kind == TXA_VERIFIABLE:
        if S > N:
            return ILLEGAL_STATE, b"", 0
    if T == 0:
        return ILLEGAL_ARGUMENTS, b"", 0
    if T > N:
        return TX_NOT_FOUND, b"", 0
    if a.rst[T - 1]:
        return a.rst[T - 1], b"", 0
    if kind == TXA_VERIFIABLE:
        if S > 0 and a.rst[S - 1]:
            return a.rst[S - 1], b"", 0
        root = T if S == 0 else S
        x, y = (root, T) if S <= T else (T, root)
        st, dual = a.dual(x, y)
        if st:
            return st, b"", 0
    st, tx, sized = serialize_tx(store, T, spec, now)
    if not sized:
        return st, b"", 0
    if kind == TXA_TX:
        return st, (tx if st == OK else b""), len(tx)
    V = messages()["VerifiableTx"]()
    if st == OK:
        V.tx.ParseFromString(tx)
        V.dualProof.ParseFromString(dual)
        msg = V.SerializeToString(deterministic=True)
        return OK, msg, len(msg)
    framed = lambda n: 1 + len(A._varint(n)) + n  # noqa: E731
    return st, b"", framed(len(tx)) + framed(len(dual))


def expect(store, reqs, out_cap=None, now=NOW):
    """reqs: (kind, T, S, spec) -> (status[n] int32, off[n + 1] uint64, messages)"""
    st, off, msgs = [], [0], []
    for r in reqs:
        s, m, size = expect_one(store, *r, now=now)
        off.append(off[-1] + size)
        if s == OK and out_cap is not None and off[-1] > out_cap:
            s, m = BUFFER_TOO_SMALL, b""
        st.append(s)
        msgs.append(m)
    return np.array(st, np.int32), np.array(off, np.uint64), msgs


def columns(reqs):
    return ([r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs], [r[3] for r in reqs])


# ------------------------------------------------------------------ the synthetic store
VALUE_LENS = (0, 1, 3, 4, 5, 54, 55, 56, 63, 64, 65, 119, 120, 127, 128, 4096)
WIDTHS = (0, 1, 2, 3, 64, 65, 257, 1100)
PREFIXES = (0, 1, 2, 3, 0xff)
EXPIRES = (NOW - 1, NOW, NOW + 1, 0, -5)
ALL_RAW = (RAW_VALUE, RAW_VALUE, RAW_VALUE)
ENTRY_BODIES = (127, 128)       # TxEntry bodies with a value, one tx
TX_BODIES = (16383, 16384)      # Tx bodies under ALL_RAW, a tx each
V2_FIRST = 3000                 # vLog 2 is resident from this byte on


def _exp_md(e):
    return b"\x01" + struct.pack(">q", e)


def _entry_body(key_len, md, vlen, with_value):
    e = messages()["TxEntry"]()
    e.key, e.hValue, e.vLen = b"k" * key_len, bytes(32), A._i32(vlen)
    if md:
        A._fill_kvmd(e.metadata, md)
    if with_value and vlen:
        e.value = bytes(vlen)
    return e.ByteSize()


def _framed(n):
    return 1 + len(A._varint(n)) + n


def _header_framed(txid, ver, ne):
    import wire
    st, h = wire.tx_header_msg({"id": txid, "ts": 1700000000 + txid, "bltxid": txid - 1,
                                "blroot": bytes(32), "prevalh": bytes(32), "eh": bytes(32),
                                "version": ver, "nentries": ne, "md": b""})
    assert st == 0
    return _framed(h.ByteSize())


class Synthetic:
    """store (SpecStore), roles (tx numbers by name), corrupt (the tx whose
    record verdict is not OK)"""


@functools.lru_cache(maxsize=None)
def synthetic(seed=17):
    """A consistent chain (every Alh, BlRoot and Eh real; BlTxID = id - 1) of
    about 40 txs over two value logs, vLog 2 resident from V2_FIRST on only:

    * widths WIDTHS (1100: the read path validates it on a host copy), header
      versions 0 and 1, key prefixes 0, 1, 2, 3 and 0xff mixed inside every
      tx of more than one entry, the value lengths of VALUE_LENS (every one
      also four to a tx through both vLogs);
    * four txs of eight entries whose values lie at every source alignment
      behind keys of 5 to 8 bytes: with the answers' varying offsets every
      destination alignment is met (the GPU test asserts it);
    * TxEntry bodies of 127 and 128 bytes (with their value), Tx bodies of
      16383 and 16384 bytes under ALL_RAW;
    * expirations at NOW - 1, NOW, NOW + 1, 0 and negative;
    * vLen == 0 with an hVal that is not SHA256(nil);
    * values with vLog id 0, behind the window's start, straddling its end,
      and with an id above nvlogs; an empty key;
    * one flipped value byte in the lowest entry, in the highest, in an
      excluded class and behind one, in an expired entry and behind one, ahead
      of and behind an SQL entry;
    * one record whose stored Alh is flipped (its verdict is not OK; the tx
      behind it reads it in every DualProof).
    """
    import oracle as orc
    rng = np.random.default_rng(seed)
    rb = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))  # noqa: E731
    v1, v2 = bytearray(), bytearray(rb(V2_FIRST))
    logs = {1: v1, 2: v2}
    tree = orc.AHtree(64)
    prev = orc.sha256(b"")
    raw, spans = bytearray(), []
    S = Synthetic()
    S.roles = {}

    def put(vid, val, align=None, flip=False):
        log = logs[vid]
        if align is not None:
            log += rb((align - len(log)) & 3)
        at = len(log)
        log += val
        if flip:
            log[at + len(val) // 2] ^= 0x10
        return X.encode_offset(at, vid)

    def key(prefix, n):
        return bytes([prefix]) + rb(n - 1)

    def add(ver, ents, role=None):
        """ents: dicts md, key, val, and optionally voff (else vLog 1), vid,
        align, flip, hval, vlen"""
        nonlocal prev
        txid = len(spans) + 1
        recs = []
        for e in ents:
            val = e.get("val", b"")
            voff = e.get("voff")
            if voff is None:
                voff = put(e.get("vid", 1), val, e.get("align"), e.get("flip", False)) if val else 0
            recs.append((e.get("md", b""), e["key"], e.get("vlen", len(val)), voff,
                         e.get("hval", orc.sha256(val))))
        rec, alh = X._record(orc, txid, prev, tree, ver, b"", recs, 1700000000 + txid)
        spans.append((len(raw), len(raw) + len(rec)))
        raw.extend(rec)
        tree.append(alh)
        prev = alh
        if role:
            S.roles[role] = txid
        return txid

    k = 0

    def width_tx(w):
        nonlocal k
        ver = 0 if w in (2, 64) else 1
        ents = []
        for _ in range(w):
            L = VALUE_LENS[k % len(VALUE_LENS)] if w < 64 else VALUE_LENS[k % 13]
            md = b"" if ver == 0 or k % 3 else (b"\x00", b"\x02", _exp_md(EXPIRES[(k // 3) % 5]))[(k // 3) % 3]
            ents.append(dict(md=md, key=key(PREFIXES[k % 5], 2 + k % 11), val=rb(L), vid=1 + (k & 1) * (L > 0)))
            k += 1
        add(ver, ents, role="width_%d" % w)

    for w in WIDTHS[1:4]:
        width_tx(w)
    # -- the record whose verdict is not OK, and a plain tx behind it
    S.corrupt = add(1, [dict(key=key(0, 6), val=rb(10))], role="corrupt")
    add(1, [dict(key=key(0, 6), val=rb(10)), dict(key=key(1, 9), val=rb(70))], role="behind_corrupt")
    for w in WIDTHS[4:]:
        width_tx(w)
    width_tx(0)
    for i in range(0, len(VALUE_LENS), 4):  # every value length, four to a tx, through both vLogs
        add(1, [dict(key=key(PREFIXES[(i + j) % 3], 3 + j), val=rb(L), vid=1 + (j & 1))
                for j, L in enumerate(VALUE_LENS[i:i + 4])])
    for sa in range(4):  # the alignment grid
        ents = []
        for da in range(4):
            for L in (1 + (sa + da) % 3, 200 + 13 * sa + 5 * da):
                vid = 1 + ((sa + da) & 1)
                ents.append(dict(key=key(da % 3, 5 + da), val=rb(L), vid=vid, align=sa))
        add(1, ents, role="align_%d" % sa)
    # -- TxEntry bodies of 127 / 128 bytes with the value inside
    ents = []
    for want in ENTRY_BODIES:
        hit = [kl for kl in range(2, 90) if _entry_body(kl, b"", 60, True) == want]
        assert hit
        ents.append(dict(key=key(0, hit[0]), val=rb(60)))
    S.entry_tuned = add(1, ents, role="entry_bodies")
    # -- Tx bodies of 16383 / 16384 bytes under ALL_RAW
    S.tx_tuned = {}
    for want in TX_BODIES:
        txid = len(spans) + 1
        fixed = _header_framed(txid, 1, 4) + 3 * _framed(_entry_body(6, b"", 4096, True))
        hit = [(kl, L) for kl in range(5, 9) for L in range(3600, 4096)
               if fixed + _framed(_entry_body(kl, b"", L, True)) == want]
        assert hit, want
        kl, L = hit[0]
        add(1, [dict(key=key(j % 3, 6), val=rb(4096), vid=1 + (j & 1)) for j in range(3)] +
            [dict(key=key(0, kl), val=rb(L))], role="tx_body_%d" % want)
        S.tx_tuned[txid] = want
    # -- expirations; an empty value whose hVal is not SHA256(nil)
    add(1, [dict(md=_exp_md(e), key=key(j % 3, 7), val=rb(20 + j)) for j, e in enumerate(EXPIRES)] +
        [dict(md=b"\x00" + _exp_md(NOW + 100) + b"\x02", key=key(0, 7), val=rb(9))], role="expirations")
    add(1, [dict(key=key(0, 5), val=rb(8)), dict(key=key(0, 6), hval=rb(32)),
            dict(key=key(1, 6), hval=rb(32)), dict(key=key(2, 4), val=rb(3))], role="empty_value")
    # -- values that are not there: each in the z class, a kv value ahead, an SQL one behind
    tail = rb(64)
    at_tail = len(v2)
    v2 += tail
    for role, voff, val in (("id_zero", 0, rb(12)),
                            ("behind_window", X.encode_offset(100, 2), bytes(v2[100:133])),
                            ("straddle_end", X.encode_offset(at_tail + 30, 2), tail[30:] + rb(6)),
                            ("no_such_vlog", X.encode_offset(64, 3), rb(8))):
        add(1, [dict(key=key(0, 5), val=rb(11)), dict(key=key(1, 5), val=val, voff=voff),
                dict(key=key(2, 5), val=rb(13))], role=role)
    add(1, [dict(key=key(0, 5), val=bytes(tail[40:]), voff=X.encode_offset(at_tail + 40, 2))], role="exact_end")
    add(1, [dict(key=key(0, 5), val=rb(11)), dict(key=b"", val=rb(5)), dict(key=key(0, 5), val=rb(7))],
        role="empty_key")
    # -- one flipped value byte
    kv = lambda n, **kw: dict(key=key(0, 6), val=rb(n), **kw)  # noqa: E731
    add(1, [kv(70, flip=True), kv(5), kv(130)], role="flip_lowest")
    add(1, [kv(70), kv(5), kv(130, flip=True)], role="flip_highest")
    add(1, [dict(key=key(1, 6), val=rb(66), flip=True), kv(9)], role="flip_in_excluded")
    add(1, [dict(key=key(1, 6), val=rb(66)), kv(9, flip=True)], role="flip_behind_excluded")
    add(1, [kv(40, md=_exp_md(NOW - 1), flip=True), kv(9)], role="flip_in_expired")
    add(1, [kv(40, md=_exp_md(NOW - 1)), kv(9, flip=True)], role="flip_behind_expired")
    add(1, [kv(33, flip=True), dict(key=key(2, 6), val=rb(12))], role="flip_ahead_of_sql")
    add(1, [dict(key=key(2, 6), val=rb(12)), kv(33, flip=True)], role="flip_behind_sql")
    raw[spans[S.corrupt - 1][1] - 1] ^= 1  # the stored Alh of that record
    from tx_util import clog_for
    exp = X.ExpStore(bytes(raw), clog_for(bytes(raw), spans),
                     [(0, bytes(v1)), (V2_FIRST, bytes(v2[V2_FIRST:]))], max_entries=2048)
    S.store = SpecStore(exp)
    return S


def triples():
    """the action triples of the parity test: all 16 kv x z combinations of
    {nil, EXCLUDE, ONLY_DIGEST, RAW_VALUE} with sql RAW_VALUE, then sql in {nil,
    EXCLUDE, ONLY_DIGEST, RESOLVE} with kv = z = RAW_VALUE"""
    acts = (None, EXCLUDE, ONLY_DIGEST, RAW_VALUE)
    out = [(kv, z, RAW_VALUE) for kv in acts for z in acts]
    out += [(RAW_VALUE, RAW_VALUE, sql) for sql in (None, EXCLUDE, ONLY_DIGEST, RESOLVE)]
    return out
