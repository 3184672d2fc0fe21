"""CPU side of the export tests (TEST INFRASTRUCTURE ONLY): mh_export_tx_batch's
contract (include/immustore_merkle.h) restated in Python over the C oracle and
replicate_util.export_tx / header_bytes.

* ExpStore: a tx log (immustore.go:1812-1924 record bytes), its commit log and
  its value logs (each the resident window [first_off, end_off) of one vLog);
  the record verdicts from oracle.txlog_validate_clog, the rebuilt Eh from the
  oracle's entry digests and hash tree.
* expect(): ImmuStore.ExportTx (immustore.go:2621-2770) per tx of a run, the
  statuses in Go's order, off, truncated and the blobs.
* go_store(): a Go-written store of tests/golden/immudb_fixtures.json, its
  vLog 1 rebuilt from each entry's (voff, value).
* synthetic(): a consistent chain of about 50 txs written as record bytes (see
  its docstring); every expectation of tests/test_gpu_export.py comes from
  expect() over these stores or mutated copies of them.
"""
import struct

import numpy as np

import replicate_util as R
from tx_util import clog_for, record_spans

OK, ILLEGAL_ARGUMENTS, ILLEGAL_STATE, CORRUPTED_DATA, BUFFER_TOO_SMALL, TX_NOT_FOUND = 0, 2, 3, 14, 19, 25
AVAIL, TRUNC, NOVLOG = 0, 1, 2
MASK64 = (1 << 64) - 1


def decode_offset(voff):
    """decodeOffset (immustore.go:1429-1431): Go's mask is 0xff << 55"""
    return (voff >> 56) & 0xff, voff & ~(0xff << 55) & MASK64


def encode_offset(off, vlog_id):
    return (vlog_id << 56) | off


class ExpStore:
    """raw: the tx-log data; clog: its commit log (es bytes an entry); vlogs:
    [(first_off, bytes)], value log k + 1 = vlogs[k], resident [first_off,
    first_off + len(bytes))."""

    def __init__(self, raw, clog, vlogs, es=12, max_entries=1024):
        self.raw, self.clog, self.es, self.max_entries = bytes(raw), bytes(clog), es, max_entries
        self.vlogs = [(int(f), bytes(b)) for f, b in vlogs]
        self.ntx = len(self.clog) // es
        self._rst = None

    def clone(self, raw=None, clog=None, vlogs=None):
        return ExpStore(self.raw if raw is None else raw, self.clog if clog is None else clog,
                        self.vlogs if vlogs is None else vlogs, self.es, self.max_entries)

    @property
    def rst(self):
        """the record verdicts through the existing tx-log oracle"""
        if self._rst is None:
            import oracle as orc
            self._rst = [int(x) for x in orc.txlog_validate_clog(self.raw, self.clog, self.es,
                                                                   self.max_entries)[1]]
        return self._rst

    def record(self, t):
        """tx t (1-based) of a record whose verdict is OK -> (header dict with
        canonical metadata and the rebuilt Eh, entries [(md canonical, key, vlen,
        voff, hval)])"""
        import oracle as orc
        raw = self.raw
        p, = struct.unpack_from(">Q", self.clog, (t - 1) * self.es)
        txid, ts, bl = struct.unpack_from(">QqQ", raw, p)
        ver, = struct.unpack_from(">H", raw, p + 88)
        if ver == 0:
            ne, = struct.unpack_from(">H", raw, p + 90)
            q, md = p + 92, b""
        else:
            ml, = struct.unpack_from(">H", raw, p + 90)
            md = R.tx_md_canon(raw[p + 92:p + 92 + ml])
            ne, = struct.unpack_from(">I", raw, p + 92 + ml)
            q = p + 96 + ml
        ents, digs = [], []
        for _ in range(ne):
            m_, = struct.unpack_from(">H", raw, q)
            kmd = R.kv_md_canon(raw[q + 2:q + 2 + m_])
            k_, = struct.unpack_from(">H", raw, q + 2 + m_)
            key = raw[q + 4 + m_:q + 4 + m_ + k_]
            vlen, voff = struct.unpack_from(">IQ", raw, q + 4 + m_ + k_)
            hv = raw[q + 16 + m_ + k_:q + 48 + m_ + k_]
            ents.append((kmd, key, vlen, voff, hv))
            st, d = orc.entry_digest(ver, key, kmd, hv)
            assert st == 0
            digs.append(bytes(d))
            q += 48 + m_ + k_
        eh = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))[1] if ne \
            else orc.sha256(b"")
        h = dict(id=txid, prev_alh=raw[p + 56:p + 88], ts=ts, version=ver, md=md, nentries=ne,
                 eh=bytes(eh), bl_tx_id=bl, bl_root=raw[p + 24:p + 56])
        return h, ents

    def value_class(self, vlen, voff):
        """-> (class, the value's bytes when available)"""
        if vlen == 0:
            return AVAIL, b""
        vid, at = decode_offset(voff)
        if vid == 0:
            return TRUNC, None  # io.EOF, immustore.go:3186
        if vid > len(self.vlogs):
            return NOVLOG, None
        first, data = self.vlogs[vid - 1]
        if at < first or at + vlen > first + len(data):
            return TRUNC, None  # multiapp.ReadAt: a missing chunk or a short read
        return AVAIL, data[at - first:at - first + vlen]

    def export_one(self, t):
        """ExportTx(t) -> (status, blob, truncated, sized): the blob is b"" and
        sized False unless the tx is written or fails on a value digest alone
        (sized: it then keeps its range, contents unspecified)"""
        import oracle as orc
        if self.rst[t - 1]:
            return self.rst[t - 1], b"", 0, False
        h, ents = self.record(t)
        status, early = OK, False
        out, cls0 = [], None
        for i, (md, key, vlen, voff, hv) in enumerate(ents):
            cls, val = self.value_class(vlen, voff)
            if i == 0:
                cls0 = cls
            st = OK
            if cls == NOVLOG:
                st, early = ILLEGAL_STATE, True
            else:
                if cls == AVAIL and orc.sha256(val) != hv:
                    st = CORRUPTED_DATA  # immustore.go:3235
                if cls != cls0:
                    st, early = CORRUPTED_DATA, True  # :2703, :2726
            if st and not status:
                status = st  # the lowest entry that fails
            out.append((key, md, val if cls == AVAIL else hv))
        if early:
            return status, b"", 0, False
        trunc = cls0 == TRUNC
        blob = R.export_tx(h, out, trunc)
        return status, blob, (1 if trunc and not status else 0), True

    def expect(self, first_tx=1, count=None, out_cap=None):
        """-> dict(status, off, truncated, blobs, sized): blobs[k] is b"" unless
        status[k] is OK; sized[k]: the range is not empty"""
        count = self.ntx - first_tx + 1 if count is None else count
        status, off, trunc, blobs, sized = [], [0], [], [], []
        for t in range(first_tx, first_tx + count):
            st, blob, tr, sz = self.export_one(t)
            off.append(off[-1] + len(blob))
            if st == OK and out_cap is not None and off[-1] > out_cap:
                st, tr = BUFFER_TOO_SMALL, 0
            status.append(st)
            trunc.append(tr)
            blobs.append(blob if st == OK else b"")
            sized.append(sz)
        return dict(status=np.array(status, np.int32), off=np.array(off, np.uint64),
                    truncated=np.array(trunc, np.uint8), blobs=blobs, sized=sized)


# ------------------------------------------------------------------ stores
def go_store(fx, es=12):
    """A Go-written store of immudb_fixtures.json: its tx log, the cLog of its
    records, vLog 1 rebuilt from each entry's (voff, value).  Asserts that the
    values tile vLog 1 without gaps."""
    raw = bytes.fromhex(fx["txlog"])
    spans = record_spans(raw, len(fx["txs"]))
    pieces = {}
    for t in fx["txs"]:
        for e in t["entries"]:
            vid, at = decode_offset(e["voff"])
            val = bytes.fromhex(e["value"])
            assert len(val) == e["vlen"]
            if not val:
                continue
            assert vid == 1
            assert pieces.setdefault(at, val) == val
    v1, pos = bytearray(), 0
    for at in sorted(pieces):
        assert at == pos, "a gap in vLog 1"
        v1 += pieces[at]
        pos += len(pieces[at])
    return ExpStore(raw, clog_for(raw, spans, es), [(0, bytes(v1))], es)


def _record(orc, txid, prev, tree, ver, txmd, ents, ts):
    """One record of a consistent chain (BlTxID = txid - 1) -> (bytes, alh);
    ents: (md, key, vlen, voff, hval), metadata canonical"""
    digs, eb = [], bytearray()
    for md, key, vlen, voff, hv in ents:
        st, d = orc.entry_digest(ver, key, md, hv)
        assert st == 0
        digs.append(bytes(d))
        eb += struct.pack(">H", len(md)) + md + struct.pack(">H", len(key)) + key
        eb += struct.pack(">IQ", vlen, voff) + hv
    ne = len(ents)
    eh = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))[1] if ne \
        else orc.sha256(b"")
    bl = txid - 1
    bl_root = tree.root_at(bl)[1] if bl else R.ZERO32
    st, inner = orc.tx_inner_hash(ts, ver, txmd, ne, eh, bl, bl_root)
    assert st == 0
    alh = orc.tx_alh(txid, prev, inner)
    hdr = struct.pack(">QqQ", txid, ts, bl) + bl_root + prev + struct.pack(">H", ver)
    hdr += struct.pack(">H", ne) if ver == 0 else struct.pack(">H", len(txmd)) + txmd + struct.pack(">I", ne)
    return bytes(hdr + eb + alh), alh


VALUE_LENS = (0, 1, 3, 4, 5, 31, 32, 33, 54, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 1000, 4096,
              70001)
WIDTHS = (0, 1, 2, 3, 5, 64, 65, 1024)
KV_MDS = (b"", b"\x00", b"\x01" + struct.pack(">q", 1234567), b"\x02",
          b"\x00\x01" + struct.pack(">q", 99) + b"\x02")
TX_MDS = (b"", b"\x00" + struct.pack(">Q", 3), b"\x01\x00\x05hello",
          b"\x00" + struct.pack(">Q", 9) + b"\x01\x01\x00" + bytes(range(256)))
V2_FIRST = 5000  # vLog 2 is resident from this byte on


class Synthetic:
    """What synthetic() returns: store (ExpStore), roles (tx numbers by name),
    n_accept (txs 1 .. n_accept replicate onto an empty tree) and n_clean (txs
    1 .. n_clean have every value available)."""


def synthetic(orc, seed=11):
    """A consistent chain (every Alh, BlRoot and Eh real) of about 50 txs:
    both header versions, every tx-metadata and KV-metadata kind, key lengths 1
    to 1024, widths 0, 1, 2, 3, 5, 64, 65 and 1024, the value lengths of
    VALUE_LENS, two value logs -- vLog 2 resident from V2_FIRST on only -- and
    32 one-entry txs that put a short (1 to 3 bytes) and a multi-block (200+
    bytes) value on every (source alignment, destination alignment) pair of the
    whole-store export.  Then the truncation cases: a tx behind vLog 2's window
    (all truncated), values that straddle its start and its end, the last value
    ending exactly at its end, id 0 with vLen > 0, mixed classes in both
    orders, an empty value in a truncated tx, an id above nvlogs."""
    rng = np.random.default_rng(seed)
    rb = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))  # noqa: E731
    v1 = bytearray()
    v2 = bytearray(rb(V2_FIRST))  # vLog 2 from byte 0; the window is cut at the end
    logs = {1: v1, 2: v2}
    tree = orc.AHtree(64)
    prev = orc.sha256(b"")
    raw, spans = bytearray(), []
    S = Synthetic()
    S.roles = {}
    pos = 0  # the whole-store export's bytes so far (every tx of the chain is written)

    def put(vid, val, align=None):
        """the value appended to vLog vid (at an offset = align mod 4) -> vOff"""
        log = logs[vid]
        if align is not None:
            log += rb((align - len(log)) & 3)
        at = len(log)
        log += val
        return encode_offset(at, vid)

    def add(ver, txmd, ents, role=None, written=True):
        """ents: (md, key, value, vOff or None = stored in vLog 1 / nowhere when
        empty); written: the whole-store export writes this tx with its values"""
        nonlocal prev, pos
        txid = len(spans) + 1
        recs = []
        for md, key, val, voff in ents:
            if voff is None:
                voff = put(1, val) if val else 0
            recs.append((md, key, len(val), voff, orc.sha256(val)))
        rec, alh = _record(orc, txid, prev, tree, ver, txmd, recs, 1700000000 + txid)
        spans.append((len(raw), len(raw) + len(rec)))
        raw.extend(rec)
        tree.append(alh)
        prev = alh
        if role:
            S.roles[role] = txid
        if written:
            pos += 4 + (128 + len(txmd) if ver else 124) + 3
            pos += sum(2 + len(key) + 2 + len(md) + 4 + len(val) for md, key, val, _ in ents)
        return txid

    # -- variety: versions, metadata, key lengths, widths, value lengths
    lens = list(VALUE_LENS)
    kls = [1, 2, 3, 7, 16, 100, 255, 1023, 1024]
    k = 0

    def width_tx(w):
        nonlocal k
        ver = 0 if w in (2, 64) else 1
        ents = []
        for e in range(w):
            val = rb(lens[k % len(lens)]) if w < 64 else rb((k * 7) % 40)
            md = b"" if ver == 0 else KV_MDS[k % len(KV_MDS)]
            key = rb(kls[k % len(kls)]) if w < 64 else struct.pack(">I", k) + rb(k % 5)
            ents.append((md, key, val, None))
            k += 1
        add(ver, b"" if ver == 0 else TX_MDS[w % len(TX_MDS)], ents, role="width_%d" % w)

    for w in WIDTHS[1:]:
        width_tx(w)
    for i in range(0, len(lens), 4):  # every value length, four to a tx, through both vLogs
        ents = []
        for L in lens[i:i + 4]:
            val = rb(L)
            voff = put(2, val) if L and (k & 1) else None
            ents.append((KV_MDS[k % len(KV_MDS)], rb(kls[k % len(kls)]), val, voff))
            k += 1
        add(1, TX_MDS[(i // 4) % len(TX_MDS)], ents)
    # -- the alignment grid: src alignment by the value's offset, dst by the key's length
    for sa in range(4):
        for da in range(4):
            for L in (1 + (sa + da) % 3, 200 + 13 * sa + 5 * da):
                val = rb(L)
                vid = 1 + ((sa + da) & 1)
                voff = put(vid, val, align=(sa + (V2_FIRST if vid == 2 else 0)) & 3)
                at_value = pos + 4 + 128 + 2 + 2 + 4  # + the key's length
                kl = 4 + ((da - at_value - 4) & 3)
                add(1, b"", [(b"", rb(kl), val, voff)])
    S.n_accept = len(spans)  # txs 1 .. n_accept replicate onto an empty tree (ReplicateTx takes no empty tx)
    width_tx(0)
    S.n_clean = len(spans)  # txs 1 .. n_clean: every value available, every tx written

    # -- truncation (vLog 2's window: [V2_FIRST, end))
    # a tx wholly behind the window start
    lo = 100
    behind = [(b"", b"behind-%d" % i, bytes(v2[lo + 40 * i:lo + 40 * i + 33]), encode_offset(lo + 40 * i, 2))
              for i in range(3)]
    add(1, b"", behind, role="behind_window", written=None)
    # a value straddling first_off
    sval = bytes(v2[V2_FIRST - 10:V2_FIRST + 20])
    add(1, b"", [(b"", b"straddle-start", sval, encode_offset(V2_FIRST - 10, 2))], role="straddle_start",
        written=None)
    # id 0 with vLen > 0
    add(1, b"", [(b"", b"id-zero", rb(12), 0)], role="id_zero", written=None)
    # mixed classes, both orders; an empty value in a truncated tx; an id above nvlogs
    good = rb(20)
    add(1, b"", [(b"", b"mix-a0", good, None), (b"", b"mix-a1", rb(9), 0)], role="mixed_avail_first",
        written=None)
    add(1, b"", [(b"", b"mix-b0", rb(9), 0), (b"", b"mix-b1", good, None)], role="mixed_trunc_first",
        written=None)
    add(1, b"", [(b"", b"e0", rb(5), 0), (b"", b"e1", b"", None)], role="empty_in_truncated", written=None)
    add(1, b"", [(b"", b"n0", good, None), (b"", b"n1", rb(8), encode_offset(64, 3))], role="no_such_vlog",
        written=None)
    add(1, b"", [(b"", b"n2", rb(8), encode_offset(0, 127)), (b"", b"n3", rb(5), 0)], role="no_such_vlog_first",
        written=None)
    # a value straddling end_off, then the last one ending exactly at end_off
    tail = rb(64)
    at_tail = len(v2)
    v2 += tail
    add(1, b"", [(b"", b"straddle-end", tail + rb(6), encode_offset(at_tail + 30, 2))], role="straddle_end",
        written=None)
    # (its stored hVal is of bytes the window does not hold: never read)
    add(1, b"", [(b"", b"exact-end", bytes(tail[40:]), encode_offset(at_tail + 40, 2))], role="exact_end",
        written=None)
    S.store = ExpStore(bytes(raw), clog_for(bytes(raw), spans), [(0, bytes(v1)), (V2_FIRST, bytes(v2[V2_FIRST:]))])
    return S


def alignment_coverage(store, ex):
    """(src alignment, dst alignment, length) of every available non-empty value
    of the written txs of a whole-store export ex = store.expect(): src as the
    device sees it (the vLog windows start 4-byte aligned), dst in out"""
    cov = []
    for t in range(1, store.ntx + 1):
        if ex["status"][t - 1] != OK:
            continue
        h, ents = store.record(t)
        p = int(ex["off"][t - 1]) + 4 + len(R.header_bytes(h))
        for md, key, vlen, voff, hv in ents:
            cls, val = store.value_class(vlen, voff)
            p += 2 + len(key) + 2 + len(md) + 4
            if cls == AVAIL and vlen:
                vid, at = decode_offset(voff)
                cov.append(((at - store.vlogs[vid - 1][0]) & 3, p & 3, vlen))
            p += vlen if cls == AVAIL else 32
        assert p + 3 == int(ex["off"][t])
    return cov


def wide_store(orc, width=1100):
    """Two txs around one of `width` > 1024 entries (the read path validates it
    on a host copy): empty values and truncated ones would mix, so every value
    is three bytes in vLog 1"""
    tree, prev = orc.AHtree(8), orc.sha256(b"")
    raw, spans, v1 = bytearray(), [], bytearray()
    for txid, w in enumerate((2, width, 3), 1):
        ents = []
        for e in range(w):
            val = bytes([e & 255, txid, e >> 8])
            ents.append((b"", struct.pack(">HI", txid, e), 3, encode_offset(len(v1), 1), orc.sha256(val)))
            v1 += val
        rec, alh = _record(orc, txid, prev, tree, 1, b"", ents, 1700000000 + txid)
        spans.append((len(raw), len(raw) + len(rec)))
        raw += rec
        tree.append(alh)
        prev = alh
    return ExpStore(bytes(raw), clog_for(bytes(raw), spans), [(0, bytes(v1))], max_entries=2048)


def log_store(raw, vlogs=()):
    """a tx log as it is (tx_util.metadata_logs): its cLog from its records"""
    return ExpStore(raw, clog_for(raw, record_spans(raw)), list(vlogs))


def big_store(orc, ntx=17, width=1000):
    """ntx x width >= 16384 entries, the size from which the values are taken in
    length-class order (varlen_kernels.hip's bucketing): ragged lengths 0 to 299
    in vLog 1, one corrupted value in the middle"""
    rng = np.random.default_rng(23)
    tree, prev = orc.AHtree(ntx), orc.sha256(b"")
    raw, spans, v1 = bytearray(), [], bytearray()
    for txid in range(1, ntx + 1):
        ents = []
        for e in range(width):
            L = (e * 37 + txid * 11) % 300
            val = bytes(rng.integers(0, 256, L, dtype=np.uint8))
            ents.append((b"", struct.pack(">HH", txid, e), L, encode_offset(len(v1), 1) if L else 0,
                         orc.sha256(val)))
            v1 += val
        rec, alh = _record(orc, txid, prev, tree, 1, b"", ents, 1700000000 + txid)
        spans.append((len(raw), len(raw) + len(rec)))
        raw += rec
        tree.append(alh)
        prev = alh
    v1[len(v1) // 2] ^= 0x40
    return ExpStore(bytes(raw), clog_for(bytes(raw), spans), [(0, bytes(v1))])


def many_store(orc, ntx=2100):
    """More txs than the offsets kernel has threads (1024): one or two entries
    a tx, every 97th tx truncated (vLog id 0), values of 0 to 40 bytes in vLog 1"""
    rng = np.random.default_rng(29)
    tree, prev = orc.AHtree(ntx), orc.sha256(b"")
    raw, spans, v1 = bytearray(), [], bytearray()
    for txid in range(1, ntx + 1):
        ents = []
        for e in range(1 + txid % 2):
            val = bytes(rng.integers(0, 256, 1 + (txid * 7 + e) % 40, dtype=np.uint8))
            voff = 0 if txid % 97 == 0 else encode_offset(len(v1), 1)
            ents.append((b"", struct.pack(">IH", txid, e), len(val), voff, orc.sha256(val)))
            if voff:
                v1 += val
        rec, alh = _record(orc, txid, prev, tree, txid % 2, b"", ents, 1700000000 + txid)
        spans.append((len(raw), len(raw) + len(rec)))
        raw += rec
        tree.append(alh)
        prev = alh
    return ExpStore(bytes(raw), clog_for(bytes(raw), spans), [(0, bytes(v1))])
