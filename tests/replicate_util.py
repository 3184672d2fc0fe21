"""CPU side of the replication tests (TEST INFRASTRUCTURE ONLY):

* export_tx(): ExportTx's byte layout (immustore.go:2621-2770);
* synthetic_store(): chained txs built with the C oracle (sha256,
  entry_digest, htree_build, tx_header_alh, AHtree), linked like the Go
  stores: BlTxID = id - 1, a fixed older BlTxID (fixture txs 11-20), or 0;
* reference(): mh_replicate_tx_batch's contract (include/immustore_merkle.h)
  restated line by line over the same oracle calls.  Every expectation of
  tests/test_gpu_replicate.py comes from it;
* mutants(): one exported tx per rule of the contract, each derived from a
  valid tx, with the status the contract names.
"""
import struct

import numpy as np

from tx_util import TX_HEADER

OK, ILLEGAL, MD_UNSUPPORTED, CORRUPTED, BUFFER_TOO_SMALL = 0, 2, 6, 14, 19
NEWER_VERSION, TRUNCATION_ARG, NULL_KEY, MAX_KEY, MAX_VALUE, MAX_ENTRIES = 26, 27, 28, 29, 30, 31
ALREADY_COMMITTED, OUT_OF_ORDER, NOT_REACHED = 32, 33, 34
SKIP_INTEGRITY, DRY_RUN = 1, 2
ALL_CODES = {OK, ILLEGAL, MD_UNSUPPORTED, CORRUPTED, NEWER_VERSION, TRUNCATION_ARG, NULL_KEY, MAX_KEY,
             MAX_VALUE, MAX_ENTRIES, ALREADY_COMMITTED, OUT_OF_ORDER, NOT_REACHED}

ENTRY = np.dtype([("key_off", "<u8"), ("md_off", "<u8"), ("val_off", "<u8"), ("key_len", "<u4"),
                  ("md_len", "<u4"), ("val_len", "<u4"), ("flags", "<u4")])
ZERO32 = bytes(32)


class Limits:
    def __init__(self, max_entries=1024, max_key_len=1024, max_value_len=1 << 25):
        self.max_entries, self.max_key_len, self.max_value_len = max_entries, max_key_len, max_value_len

    def kw(self):
        return dict(max_entries=self.max_entries, max_key_len=self.max_key_len,
                    max_value_len=self.max_value_len)


# ------------------------------------------------------------------ the wire
def header_bytes(h):
    """TxHeader.Bytes() (tx.go:103-164); h["md"] as stored"""
    b = struct.pack(">Q", h["id"]) + h["prev_alh"] + struct.pack(">qH", h["ts"], h["version"])
    if h["version"] == 0:
        b += struct.pack(">H", h["nentries"])
    else:
        b += struct.pack(">H", len(h["md"])) + h["md"] + struct.pack(">I", h["nentries"])
    return b + h["eh"] + struct.pack(">Q", h["bl_tx_id"]) + h["bl_root"]


def export_entries(entries):
    out = bytearray()
    for key, md, val in entries:
        out += struct.pack(">H", len(key)) + key + struct.pack(">H", len(md)) + md
        out += struct.pack(">I", len(val)) + val
    return bytes(out)


def export_tx(header, entries, truncated, trailer=True):
    """header: dict (header_bytes); entries: [(key, md, value)], value being
    the 32-byte hash (or whatever stands for it) of a truncated tx"""
    hb = header_bytes(header)
    out = struct.pack(">I", len(hb)) + hb + export_entries(entries)
    if trailer:
        out += struct.pack(">H", 1) + bytes([1 if truncated else 0])
    return out


def kv_md_bytes(deleted, expires, non_indexable):
    """KVMetadata.Bytes() of verifiable_entry_util.MD_KINDS-style triples"""
    b = b"\x00" if deleted else b""
    if expires is not None:
        b += b"\x01" + struct.pack(">q", expires)
    return b + (b"\x02" if non_indexable else b"")


def kv_md_canon(md):
    """KVMetadata.unsafeReadFrom + Bytes() (kv_metadata.go:207-256); None: ErrCorruptedData"""
    if len(md) > 11:
        return None
    at, i = {}, 0
    while i < len(md):
        c = md[i]
        i += 1
        if c == 1:
            if len(md) - i < 8:
                return None
            at[1] = md[i:i + 8]
            i += 8
        elif c in (0, 2):
            at[c] = b""
        else:
            return None
    return b"".join(bytes([c]) + at[c] for c in (0, 1, 2) if c in at)


def tx_md_canon(md):
    """TxMetadata.ReadFrom + Bytes() (tx_metadata.go:145-193); None: ErrCorruptedData"""
    if len(md) > 268:
        return None
    at, i = {}, 0
    while i < len(md):
        c = md[i]
        i += 1
        if c == 0:
            if len(md) - i < 8:
                return None
            at[0] = md[i:i + 8]
            i += 8
        elif c == 1:
            if len(md) - i < 2:
                return None
            el, = struct.unpack_from(">H", md, i)
            if el > 256 or len(md) - i - 2 < el:
                return None
            at[1] = md[i:i + 2 + el]
            i += 2 + el
        else:
            return None
    return b"".join(bytes([c]) + at[c] for c in (0, 1) if c in at)


def digest32(v):
    """digest() immustore.go:3666"""
    return bytes(v[:32]).ljust(32, b"\0")


# ------------------------------------------------------------------ stores
def clone_tree(orc, t):
    c = orc.AHtree(1)
    c.dlog = t.dlog.copy()
    c.size = t.size
    return c


def make_tx(orc, txid, prev_alh, tree, entries, version=1, txmd=b"", bl=None, ts=None,
            truncated=False, txmd_hash=None):
    """One valid tx behind `tree` (txid - 1 leaves).  entries: (key, md, value)
    or (key, md_exported, value, md_hashed).  -> dict(header, entries, truncated, alh, blob)"""
    digs, ex = [], []
    for e in entries:
        key, md, val = e[:3]
        hv = digest32(val) if truncated else orc.sha256(val)
        st, d = orc.entry_digest(version, key, e[3] if len(e) > 3 else md, hv)
        assert st == 0
        digs.append(d)
        ex.append((key, md, val))
    eh = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))[1]
    bl = txid - 1 if bl is None else bl
    bl_root = tree.root_at(bl)[1] if bl else ZERO32
    h = dict(id=txid, prev_alh=prev_alh, ts=1700000000 + txid if ts is None else ts, version=version,
             md=txmd, nentries=len(entries), eh=eh, bl_tx_id=bl, bl_root=bl_root)
    st, inner = orc.tx_inner_hash(h["ts"], version, txmd if txmd_hash is None else txmd_hash,
                                  len(entries), eh, bl, bl_root)
    assert st == 0
    alh = orc.tx_alh(txid, prev_alh, inner)
    return dict(header=h, entries=ex, truncated=truncated, alh=alh,
                blob=export_tx(h, ex, truncated))


def synthetic_store(orc, specs, bl_of=None, keep=None):
    """specs: per tx a dict of make_tx keywords (entries, version, txmd,
    truncated).  bl_of(txid) -> BlTxID (None: txid - 1).  -> (txs, trees):
    trees[k] = the oracle AHtree of the first k Alh values (k in keep; None:
    every k)."""
    tree = orc.AHtree(max(len(specs), 1))
    prev = orc.sha256(b"")
    txs, trees = [], {0: clone_tree(orc, tree)}
    for k, sp in enumerate(specs):
        tx = make_tx(orc, k + 1, prev, tree, bl=bl_of(k + 1) if bl_of else None, **sp)
        tree.append(tx["alh"])
        prev = tx["alh"]
        txs.append(tx)
        if keep is None or k + 1 in keep:
            trees[k + 1] = clone_tree(orc, tree)
    return txs, trees


def prev_alh_of(orc, txs, P):
    """the Alh reached after the first P txs"""
    return txs[P - 1]["alh"] if P else orc.sha256(b"")


def simple_specs(n, seed=1):
    """n two-entry v1 txs without metadata (what mutants() derives from)"""
    rng = np.random.default_rng(seed)
    rb = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))  # noqa: E731
    return [dict(entries=[(b"a" + rb(7), b"", rb(20)), (b"b" + rb(3), b"", rb(70))]) for _ in range(n)]


def fixture_store(fx):
    """The txs of one Go-written store of immudb_fixtures.json, exported from
    its keys, values and headers -> (blobs, stored alh, stored aht dLog)"""
    blobs, alhs = [], []
    for t in fx["txs"]:
        h = t["header"]
        hd = dict(id=h["id"], prev_alh=bytes.fromhex(h["prevalh"]), ts=h["ts"], version=h["version"],
                  md=bytes.fromhex(h["md"]), nentries=h["nentries"], eh=bytes.fromhex(h["eh"]),
                  bl_tx_id=h["bltxid"], bl_root=bytes.fromhex(h["blroot"]))
        ents = [(bytes.fromhex(e["key"]), bytes.fromhex(e["md"]), bytes.fromhex(e["value"]))
                for e in t["entries"]]
        blobs.append(export_tx(hd, ents, False))
        alhs.append(bytes.fromhex(h["alh"]))
    return blobs, alhs, bytes.fromhex(fx["aht_dlog"])


# ------------------------------------------------------------------ reference
def parse(b):
    """ReplicateTx's reads (immustore.go:2773-2881, tx.go:166-247) ->
    (status, header dict or None, entry spans [(koff, klen, mdoff, mdlen,
    voff, vlen)], truncated)"""
    L = len(b)
    if L == 0 or L < 4:
        return ILLEGAL, None, [], False
    hl, = struct.unpack_from(">I", b, 0)
    if L < 4 + hl:
        return ILLEGAL, None, [], False
    h = b[4:4 + hl]
    if hl < 124:
        return ILLEGAL, None, [], False
    txid, = struct.unpack_from(">Q", h, 0)
    if txid < 1:
        return ILLEGAL, None, [], False
    ts, ver = struct.unpack_from(">qH", h, 40)
    j, md = 50, b""
    if ver == 0:
        ne, = struct.unpack_from(">H", h, j)
        j += 2
    elif ver == 1:
        ml, = struct.unpack_from(">H", h, j)
        j += 2
        if hl < j + ml + 4 or ml > 268:
            return CORRUPTED, None, [], False
        if ml:
            md = tx_md_canon(h[j:j + ml])
            if md is None:
                return CORRUPTED, None, [], False
            j += ml
        ne, = struct.unpack_from(">I", h, j)
        j += 4
    else:
        return NEWER_VERSION, None, [], False
    if ne < 1:
        return ILLEGAL, None, [], False
    if hl < j + 72:  # Go zero-fills or panics: documented as illegal arguments
        return ILLEGAL, None, [], False
    bl, = struct.unpack_from(">Q", h, j + 32)
    if bl >= txid:
        return ILLEGAL, None, [], False
    hdr = dict(id=txid, prev_alh=h[8:40], ts=ts, version=ver, md=md, nentries=ne, eh=h[j:j + 32],
               bl_tx_id=bl, bl_root=h[j + 40:j + 72])
    i, spans = 4 + hl, []
    for _ in range(ne):
        if L < i + 8:
            return ILLEGAL, None, [], False
        kl, = struct.unpack_from(">H", b, i)
        i += 2
        if L < i + 6 + kl:
            return ILLEGAL, None, [], False
        kp = i
        i += kl
        ml, = struct.unpack_from(">H", b, i)
        i += 2
        if L < i + ml:
            return ILLEGAL, None, [], False
        mp = i
        if ml:
            if kv_md_canon(b[i:i + ml]) is None:
                return CORRUPTED, None, [], False
            i += ml
        if L < i + 4:  # Go panics
            return ILLEGAL, None, [], False
        vl, = struct.unpack_from(">I", b, i)
        i += 4
        if L < i + vl:
            return ILLEGAL, None, [], False
        spans.append((kp, kl, mp, ml, i, vl))
        i += vl
    trunc = False
    if i < L:
        if L < i + 2:  # Go panics
            return ILLEGAL, None, [], False
        tl, = struct.unpack_from(">H", b, i)
        i += 2
        if L < i + tl:
            return ILLEGAL, None, [], False
        if tl > 0 and b[i] > 1:
            return TRUNCATION_ARG, None, [], False
        if tl == 0:  # Go indexes v[0]
            return ILLEGAL, None, [], False
        trunc = b[i] == 1
        i += tl
    if i != L:
        return ILLEGAL, None, [], False
    return OK, hdr, spans, trunc


def local_verdict(orc, b, lim, flags):
    """Envelope through Eh of one exported tx -> dict(status, hdr, spans,
    trunc, hvals, alh, hashed)"""
    st, hdr, spans, trunc = parse(b)
    r = dict(status=st, hdr=hdr, spans=spans, trunc=trunc, hvals=[ZERO32] * len(spans), alh=ZERO32,
             hashed=False)
    if st != OK:
        return r
    held, st = [], OK
    for kp, kl, mp, ml, vp, vl in spans:  # OngoingTx.set, ongoing_tx.go:242-267
        key = b[kp:kp + kl]
        if kl == 0:
            st = NULL_KEY
        elif kl > lim.max_key_len:
            st = MAX_KEY
        elif not trunc and vl > lim.max_value_len:
            st = MAX_VALUE
        elif key not in held:
            if len(held) > lim.max_entries:
                st = MAX_ENTRIES
            else:
                held.append(key)
        if st != OK:
            break
    if st == OK and len(held) != hdr["nentries"]:  # validateAgainst
        st = ILLEGAL
    if st == OK and len(held) > lim.max_entries:  # validateEntries
        st = MAX_ENTRIES
    if st == OK and hdr["version"] == 0 and any(s[3] for s in spans):
        st = MD_UNSUPPORTED
    if st != OK:
        r["status"] = st
        return r
    digs, hvs = [], []
    for kp, kl, mp, ml, vp, vl in spans:
        val = b[vp:vp + vl]
        hv = digest32(val) if trunc else orc.sha256(val)
        md = kv_md_canon(b[mp:mp + ml]) if hdr["version"] == 1 else b""
        s_, d = orc.entry_digest(hdr["version"], b[kp:kp + kl], md, hv)
        assert s_ == 0
        digs.append(d)
        hvs.append(hv)
    eh = orc.htree_build(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32))[1]
    r["hvals"], r["hashed"] = hvs, True
    if eh != hdr["eh"] and not flags & SKIP_INTEGRITY:
        r["status"] = ILLEGAL
    hdr["eh"] = eh  # the header as precommitted
    if r["status"] == OK:
        rec = header_record(hdr, 0)
        s_, _, alh = orc.tx_header_alh(rec, hdr["md"])
        assert s_ == 0
        r["alh"] = alh
    return r


def header_record(h, md_off):
    rec = np.zeros(1, TX_HEADER)[0]
    rec["id"], rec["ts"], rec["bl_tx_id"] = h["id"], h["ts"], h["bl_tx_id"]
    rec["bl_root"] = np.frombuffer(h["bl_root"], np.uint8)
    rec["prev_alh"] = np.frombuffer(h["prev_alh"], np.uint8)
    rec["eh"] = np.frombuffer(h["eh"], np.uint8)
    rec["version"], rec["nentries"] = h["version"], h["nentries"]
    rec["md_len"], rec["md_off"] = len(h["md"]), md_off
    return rec


def reference(orc, blobs, tree, prev_alh, lim=None, flags=0):
    """mh_replicate_tx_batch over the oracle tree `tree` (left untouched) ->
    dict(status, accepted, hdrs, md_blob, alh, ent_off, ents, hvals, dlog,
    size): the arrays the call returns, and the tree after it."""
    lim = lim or Limits()
    n = len(blobs)
    work = clone_tree(orc, tree)
    P = tree.size
    status = np.zeros(n, np.int32)
    hdrs = np.zeros(n, TX_HEADER)
    md_blob = np.zeros(n * 268, np.uint8)
    alh = np.zeros((n, 32), np.uint8)
    ent_off = np.zeros(n + 1, np.uint64)
    ents, hvals = [], []
    reached, cur, a, base = P, prev_alh, None, 0
    for k, b in enumerate(blobs):
        r = local_verdict(orc, b, lim, flags)
        st = r["status"]
        if r["hdr"] is not None:
            h = r["hdr"]
            hdrs[k] = header_record(h, k * 268)
            md_blob[k * 268:k * 268 + len(h["md"])] = np.frombuffer(h["md"], np.uint8)
            for (kp, kl, mp, ml, vp, vl), hv in zip(r["spans"], r["hvals"]):
                ents.append((base + kp, base + mp, base + vp, kl, ml, vl, 1 if r["trunc"] else 0))
                hvals.append(hv)
        ent_off[k + 1] = len(ents)
        alh[k] = np.frombuffer(r["alh"], np.uint8)
        if a is None:
            if st == OK:
                h = r["hdr"]
                if h["id"] <= reached:
                    st = ALREADY_COMMITTED
                elif h["id"] > reached + 1:
                    st = OUT_OF_ORDER
                else:
                    root = work.root_at(h["bl_tx_id"])[1] if h["bl_tx_id"] else ZERO32
                    if root != h["bl_root"] or h["prev_alh"] != cur:
                        st = ILLEGAL
            if st == OK:
                work.append(r["alh"])
                reached, cur = reached + 1, r["alh"]
            else:
                a = k
        elif st == OK:
            st = NOT_REACHED
        status[k] = st
        base += len(b)
    accepted = n if a is None else a
    final = tree if flags & DRY_RUN else work
    return dict(status=status, accepted=accepted, hdrs=hdrs, md_blob=md_blob, alh=alh,
                ent_off=ent_off, ents=np.array(ents, ENTRY) if ents else np.zeros(0, ENTRY),
                hvals=np.frombuffer(b"".join(hvals), np.uint8).reshape(-1, 32) if hvals
                else np.zeros((0, 32), np.uint8),
                dlog=final.dlog_bytes(), size=final.size)


# ------------------------------------------------------------------ mutants
MUT_LIMITS = Limits(max_entries=6, max_key_len=40, max_value_len=300)


def _hdr_edit(tx, **kw):
    return export_tx(dict(tx["header"], **kw), tx["entries"], tx["truncated"])


def _flip(b):
    return bytes([b[0] ^ 1]) + b[1:]


def _raw(tx, hdr_bytes, body=None, trailer=b"\x00\x01\x00"):
    body = export_entries(tx["entries"]) if body is None else body
    return struct.pack(">I", len(hdr_bytes)) + hdr_bytes + body + trailer


def mutants(orc, tx, prev_alh, tree):
    """tx: a valid v1 tx (make_tx) with id >= 2, no metadata, 2 entries,
    applied behind `tree` with `prev_alh`.  -> [(name, blob, status)] under
    MUT_LIMITS: every rule of mh_replicate_tx_batch's contract."""
    h, ents = tx["header"], tx["entries"]
    assert h["version"] == 1 and h["id"] >= 2 and len(ents) == 2 and not h["md"]
    hb, body = header_bytes(h), export_entries(ents)
    good = tx["blob"]
    hend = 4 + len(hb)
    k0, v0 = ents[0][0], ents[0][2]

    def rebuild(entries, **kw):
        return make_tx(orc, h["id"], prev_alh, tree, entries, bl=h["bl_tx_id"], ts=h["ts"], **kw)["blob"]

    def hdr_with(version=1, md=b"", ne=2, cut=0, pad=b""):
        x = dict(h, version=version, md=md, nentries=ne)
        b = header_bytes(x)
        return b[:len(b) - cut] + pad

    ent1 = lambda key=k0, md=b"", val=v0: export_entries([(key, md, val)])  # noqa: E731
    one = lambda b: _raw(tx, hdr_with(ne=1), b, b"")  # noqa: E731  (one entry, no trailer)
    many = lambda n: [(b"k%d" % i, b"", b"v") for i in range(n)]  # noqa: E731
    rows = [
        ("valid", good, OK),
        # envelope
        ("empty", b"", ILLEGAL),
        ("three_bytes", good[:3], ILLEGAL),
        ("cut_in_header", good[:hend - 1], ILLEGAL),
        # TxHeader.ReadFrom
        ("header_short", struct.pack(">I", 100) + hb[:100], ILLEGAL),
        ("id_zero", _hdr_edit(tx, id=0, bl_tx_id=0, bl_root=ZERO32), ILLEGAL),
        ("txmd_len_over_268", _raw(tx, hb[:50] + struct.pack(">H", 300) + bytes(300) + hb[52:]), CORRUPTED),
        ("txmd_len_over_header", _raw(tx, hb[:50] + struct.pack(">H", 200) + hb[52:]), CORRUPTED),
        ("txmd_unknown_attribute", _raw(tx, hdr_with(md=b"\x05")), CORRUPTED),
        ("txmd_short_attribute", _raw(tx, hdr_with(md=b"\x00" + bytes(5))), CORRUPTED),
        ("version_2", _raw(tx, hb[:48] + struct.pack(">H", 2) + hb[50:]), NEWER_VERSION),
        ("nentries_zero", _raw(tx, hdr_with(ne=0)), ILLEGAL),
        ("bl_not_below_id", _hdr_edit(tx, bl_tx_id=h["id"]), ILLEGAL),
        ("bytes_after_blroot", _raw(tx, hdr_with(pad=b"extra")), OK),
        ("header_ends_in_blroot", _raw(tx, hdr_with(cut=4)), ILLEGAL),
        ("header_ends_in_bltxid", _raw(tx, hdr_with(md=b"\x01\x00\x3c" + bytes(60), cut=36)), ILLEGAL),
        ("header_ends_in_eh", _raw(tx, hdr_with(md=b"\x01\x00\x3c" + bytes(60), cut=60)), ILLEGAL),
        # entries
        ("entry_under_8_bytes", good[:hend + 7], ILLEGAL),
        ("klen_past_blob", _raw(tx, hb, struct.pack(">H", 500) + body[2:], b""), ILLEGAL),
        ("kv_mdlen_past_blob", one(struct.pack(">H", 2) + b"ab" + struct.pack(">H", 9) + bytes(6)), ILLEGAL),
        ("kv_md_unknown_attribute", one(ent1(md=b"\x03")), CORRUPTED),
        ("kv_md_short_expiry", one(ent1(md=b"\x01" + bytes(4))), CORRUPTED),
        ("kv_md_over_11", one(ent1(md=b"\x00" * 12)), CORRUPTED),
        ("vlen_word_past_blob", one(struct.pack(">H", 2) + b"ab" + struct.pack(">H", 4) + b"\x00\x02\x00\x02"),
         ILLEGAL),
        ("vlen_past_blob", one(ent1()[:-1]), ILLEGAL),
        # trailer
        ("no_trailer", export_tx(h, ents, False, trailer=False), OK),
        ("trailer_one_byte", good[:-2], ILLEGAL),
        ("trailer_len_past_blob", good[:-3] + struct.pack(">H", 2) + b"\x00", ILLEGAL),
        ("trailer_len_zero", good[:-3] + struct.pack(">H", 0), ILLEGAL),
        ("trailer_flag_2", good[:-1] + b"\x02", TRUNCATION_ARG),
        ("trailer_two_bytes", good[:-3] + struct.pack(">H", 2) + b"\x00\x09", OK),
        ("bytes_after_trailer", good + b"\x00", ILLEGAL),
        # OngoingTx.set, validateAgainst, validateEntries
        ("null_key", _raw(tx, hb, export_entries([(b"", b"", v0), ents[1]])), NULL_KEY),
        ("key_too_long", _raw(tx, hb, export_entries([ents[0], (b"k" * 41, b"", v0)])), MAX_KEY),
        ("key_at_limit", rebuild([ents[0], (b"k" * 40, b"", v0)]), OK),
        ("value_too_long", _raw(tx, hb, export_entries([ents[0], (b"k", b"", bytes(301))])), MAX_VALUE),
        ("value_at_limit", rebuild([ents[0], (b"k", b"", bytes(300))]), OK),
        ("long_key_before_null_key", _raw(tx, hb, export_entries([(b"k" * 41, b"", v0), (b"", b"", v0)])),
         MAX_KEY),
        ("truncated_long_value", rebuild([ents[0], (b"k", b"", bytes(range(256)) * 2)], truncated=True), OK),
        ("entries_at_limit", rebuild(many(6)), OK),
        ("entries_limit_plus_1", _raw(tx, hdr_with(ne=7), export_entries(many(7))), MAX_ENTRIES),
        ("entries_limit_plus_2", _raw(tx, hdr_with(ne=8), export_entries(many(8))), MAX_ENTRIES),
        ("repeated_key", _raw(tx, hb, export_entries([ents[0], (k0, b"", b"other")])), ILLEGAL),
        ("repeated_key_over_limit", _raw(tx, hdr_with(ne=8), export_entries(many(7) + [(b"k3", b"", b"w")])),
         ILLEGAL),
        ("null_key_behind_limit", _raw(tx, hdr_with(ne=9), export_entries(many(8) + [(b"", b"", b"w")])),
         MAX_ENTRIES),
        # hashing
        ("kv_md_under_v0", _raw(tx, hdr_with(version=0), export_entries([ents[0], (b"k", b"\x00", v0)])),
         MD_UNSUPPORTED),
        ("v0", rebuild(ents, version=0), OK),
        ("kv_md_not_canonical", rebuild([ents[0], (b"k", b"\x02\x00\x00", v0, b"\x00\x02")]), OK),
        ("txmd_not_canonical", rebuild(ents, txmd=b"\x01\x00\x01x\x00" + bytes(8),
                                       txmd_hash=b"\x00" + bytes(8) + b"\x01\x00\x01x"), OK),
        ("kv_md_hashed_as_exported", make_tx(orc, h["id"], prev_alh, tree,
                                             [(b"k", b"\x02\x00", v0)], bl=h["bl_tx_id"])["blob"], ILLEGAL),
        # against the exported header
        ("eh_differs", _hdr_edit(tx, eh=_flip(h["eh"])), ILLEGAL),
        ("already_committed", _hdr_edit(tx, id=h["id"] - 1, bl_tx_id=0, bl_root=ZERO32), ALREADY_COMMITTED),
        ("out_of_order", _hdr_edit(tx, id=h["id"] + 1), OUT_OF_ORDER),
        ("blroot_differs", _hdr_edit(tx, bl_root=_flip(h["bl_root"])), ILLEGAL),
        ("blroot_nonzero_for_bl_0", _hdr_edit(tx, bl_tx_id=0, bl_root=_flip(ZERO32)), ILLEGAL),
        ("prev_alh_differs", _hdr_edit(tx, prev_alh=_flip(h["prev_alh"])), ILLEGAL),
    ]
    return rows
