"""The CPU reference of mh_verify_verifiable_tx_pb_batch
(tests/verifiable_tx_util.reference) against Go-written data and against the
server restatement; the mix of the hostile set."""
import struct
from collections import Counter

import verifiable_tx_util as V
from tx_util import headers_from_fixture


def _txlog_records(raw):
    """the records of a Go-written tx log (tx.go:419-603) -> [(header dict with
    the stored alh and no Eh, [(key, kv metadata bytes, hValue, vLen)])]"""
    out, p = [], 0
    while p + 8 <= len(raw) and struct.unpack_from(">Q", raw, p)[0]:
        h = dict(zip(("id", "ts", "bltxid"), struct.unpack_from(">QqQ", raw, p)))
        h["blroot"], h["prevalh"] = raw[p + 24:p + 56], raw[p + 56:p + 88]
        h["version"], = struct.unpack_from(">H", raw, p + 88)
        if h["version"] == 0:
            h["md"] = b""
            h["nentries"], = struct.unpack_from(">H", raw, p + 90)
            q = p + 92
        else:
            ml, = struct.unpack_from(">H", raw, p + 90)
            h["md"] = raw[p + 92:p + 92 + ml]
            h["nentries"], = struct.unpack_from(">I", raw, p + 92 + ml)
            q = p + 96 + ml
        ents = []
        for _ in range(h["nentries"]):
            ml, = struct.unpack_from(">H", raw, q)
            md = raw[q + 2:q + 2 + ml]
            kl, = struct.unpack_from(">H", raw, q + 2 + ml)
            key = raw[q + 4 + ml:q + 4 + ml + kl]
            q += 4 + ml + kl
            vlen, = struct.unpack_from(">I", raw, q)
            ents.append((key, md, raw[q + 12:q + 44], vlen))
            q += 44
        h["alh"] = raw[q:q + 32]
        out.append((h, ents))
        p = q + 32
    return out


def _kvmd_from_bytes(M, md):
    """the KVMetadata message of stored metadata bytes (kv_metadata.go:221-279)"""
    i = 0
    while i < len(md):
        M.SetInParent()
        if md[i] == 0:
            M.deleted = True
            i += 1
        elif md[i] == 1:
            M.expiration.SetInParent()
            M.expiration.expiresAt, = struct.unpack_from(">q", md, i + 1)
            i += 9
        else:
            assert md[i] == 2
            M.nonIndexable = True
            i += 1


def test_go_written_transactions(orc, fixtures):
    """VerifiableTx messages built from the Go-written tx logs and the fixtures'
    Go-written dual_v1 proofs: the reference accepts them, and the Eh and Alh
    it rebuilds from the entries are the stored ones."""
    import wire
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    seen = Counter()
    for name in ("v110_defaultdb", "long_linear_proof"):
        fx = fixtures[name]
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        log = _txlog_records(bytes.fromhex(fx["txlog"]))
        assert len(log) == len(recs)
        proofs = {(c["src"], c["tgt"]): c for c in fx["dual_v1"]}
        for k, (h, ents) in enumerate(log, 1):
            assert h["alh"] == alhs[k - 1]
            h = dict(h, eh=b"not the stored Eh: TxFromProto overwrites it")
            M = V.messages()["VerifiableTx"]()
            M.tx.header.CopyFrom(wire.tx_header_msg(h)[1])
            for key, md, hv, vlen in ents:
                e = M.tx.entries.add(key=key, hValue=hv, vLen=vlen)
                _kvmd_from_bytes(e.metadata, md)
            seen[(h["version"], len(ents))] += 1
            for S in sorted({0, 1, k - 1, k}):
                c = proofs[(S if S else k, k)]
                M.dualProof.ParseFromString(dual_v1_msg(wire, dual_v1_args(c, recs, blob, alhs)))
                raw = M.SerializeToString()
                salh = alhs[S - 1] if S else V.Z32
                # the request: the tx's own keys, as SET_ALL would have sent them;
                # the values are not in the log, so the entry digests are checked
                # through the Eh alone (a key that is not a plain 0x00 key fails
                # only the spec match, never the rebuilt Eh)
                st, ok, ntx, nalh, eh = V.reference(raw, V.TX_BY_ID, (), k, S, salh)
                assert (st, ok, ntx, nalh) == (0, True, k, alhs[k - 1]), (name, k, S)
                specs = tuple((key[1:], b"") for key, _, _, _ in ents)
                st, _, _, _, eh = V.reference(raw, V.SET_ALL, specs, 0, S, salh)
                assert st == 0 and eh == bytes.fromhex(fx["txs"][k - 1]["header"]["eh"]), (name, k, S)
                rec = recs[k - 1].copy()
                assert bytes(rec["eh"]) == eh
                st, _, alh = orc.tx_header_alh(rec, blob)
                assert st == 0 and alh == alhs[k - 1]
    assert seen[(0, 1)] and seen[(0, 4)] and any(v == 1 for v, _ in seen), seen


def test_reference_accepts_the_server_restatement():
    """all five kinds, from S in {0, tx - 1}; TX_BY_ID also from tx + 1 and the
    last tx; eh is the stored Eh, the new state the tx's (or the state's own)"""
    s = V.store()
    n = 0
    for k in list(range(1, V.N_WIDE + 1, 3)) + V.one_entry_txs():
        kinds = [V.TX_BY_ID]
        if all(e.kind == V.SET for e in s.ents[k]):
            kinds.append(V.SET_ALL)
        if len(s.ents[k]) == 1:
            kinds.append(V.own_kind(k))
        for kind in kinds:
            for S in sorted({0, k - 1} | ({min(k + 1, s.n), s.n} if kind == V.TX_BY_ID else set())):
                name, raw, kd, specs, at, S, salh = V.case("", V.answer(k, S).SerializeToString(), k,
                                                            kind, S)
                st, ok, ntx, nalh, eh = V.reference(raw, kd, specs, at, S, salh)
                deleted = kind == V.SET and s.ents[k][0].md[0]
                assert st == 0 and ok == (not deleted), (k, kind, S)
                if ok:
                    t = max(k, S)
                    assert (ntx, nalh) == (t, s.alhs[t - 1]), (k, kind, S)
                if kind != V.TX_BY_ID:
                    assert eh == s.recs[k - 1]["eh"].tobytes()
                n += 1
    assert n > 200


def test_case_lists_cover_the_status_table():
    """the encoding cases reach every status; the tamper cases refuse and accept"""
    cases, want = V.expectations(V.encoding_cases)
    for kind in range(5):
        got = {w[0] for c, w in zip(cases, want) if c[2] == kind}
        need = {0, 2, 14} | ({21} if kind != V.TX_BY_ID else set())
        assert need <= got, (kind, got)
    for name, ok in (("plain", True), ("reversed", True), ("unknown fields", True),
                     ("dualProof twice", True), ("kvEntries / zEntries / signature", True),
                     ("header in two", True), ("vLen and value of an entry: read by nobody", True)):
        hit = [w for c, w in zip(cases, want) if c[0].startswith(name + " (")]
        assert hit and all(w[0] == 0 and w[1] == ok for w in hit), (name, [w[:2] for w in hit])
    cases, want = V.expectations(V.tamper_cases)
    by = {}
    for c, w in zip(cases, want):
        by.setdefault(c[0].split(" (")[0], []).append(w)
    for name in ("untampered", "wire eH flipped: must not matter", "wire eH empty: must not matter",
                 "ZADD asked with a value: ignored", "empty metadata message",
                 "version 0 with an empty metadata message",
                 "header metadata extra too long: dropped", "TX_BY_ID: its tx is not looked at"):
        assert all(w[:2] == (0, True) for w in by[name]), (name, [w[:2] for w in by[name]])
    for name in ("sent value", "sent key", "referenced key", "at_tx", "ZADD key byte 0",
                 "hValue of leaf 0", "key of leaf 0", "deleted on SET", "expiration added",
                 "nonIndexable", "version 0 with entry metadata", "nentries + 1",
                 "entries 3 / 4 swapped, different metadata",
                 "duplicate keys, only the second matching", "target header eH flipped",
                 "reference asked as SET"):
        assert all(w[:2] == (0, False) for w in by[name]), (name, [w[:2] for w in by[name]])
    # the edits a DualProof alone catches pass without a state (duplicates and
    # swaps come with the target eH of the edited entries)
    for name in ("duplicate keys, the first matching", "entries 0 / 1 swapped, equal metadata",
                 "entries 0 / 6 swapped, version 0","header id", "header ts", "header blTxId", "header blRoot", "header prevAlh",
                 "dual linear term"):
        assert {w[1] for w in by[name]} == {True, False}, (name, [w[:2] for w in by[name]])


def test_hostile_set_shares():
    """corrupt / decoded and refused / accepted each hold at least 5 % of the set"""
    cases, want = V.expectations(V.hostile_set)
    n = len(cases)
    assert 1400 <= n <= 1600
    corrupt = sum(w[0] == 14 for w in want)
    refused = sum(w[0] != 14 and not w[1] for w in want)
    accepted = sum(w[1] for w in want)
    assert min(corrupt, refused, accepted) >= 0.05 * n, (n, corrupt, refused, accepted)
