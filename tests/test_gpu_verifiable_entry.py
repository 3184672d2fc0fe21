"""mh_verify_verifiable_entry_pb_batch / mh_multi_verify_verifiable_entry_pb_batch
/ mh_verifiable_entry_pb_decode_batch: whole VerifiableGet answers verified in
one device pass (pkg/client's verifiedGet, client.go:1119-1234, before the
signature check).  Every expectation comes from the CPU reference of
tests/verifiable_entry_util.py (protobuf runtime + C oracle), never from the
library; the cases -- store, padding edges, metadata, state, tampering,
encodings, hostile set -- are built there too."""
import os

import numpy as np
import pytest

import verifiable_entry_util as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import torch  # noqa: F401
    import immustore_amd as m
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _fused(cases, ctx, **kw):
    from immustore_amd import txlayer
    return txlayer.verify_verifiable_entry_pb_batch(
        [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases],
        [c[5] for c in cases], ctx=ctx, **kw)


def _expected(cases):
    return [V.reference(*c[1:]) for c in cases]


def _check(cases, got, exp=None):
    """status, ok, new_tx and new_alh of every answer == the reference's"""
    exp = exp or _expected(cases)
    st, ok, ntx, nalh = got
    assert len(st) == len(cases)
    for k, c in enumerate(cases):
        g = (int(st[k]), bool(ok[k]), int(ntx[k]), nalh[k].tobytes())
        assert g == exp[k], (k, c[0], g[:3], exp[k][:3])
    return exp


@pytest.fixture(scope="module")
def good(orc):
    cases = V.good_cases()
    return cases, _expected(cases)


@pytest.fixture(scope="module")
def tampered(orc):
    cases = V.tamper_cases()
    return cases, _expected(cases)


@pytest.fixture(scope="module")
def hostile(orc):
    cases = [("hostile %d" % k,) + a for k, a in enumerate(V.hostile_set())]
    return cases, _expected(cases)


# ------------------------------------------------------------------ the store
def test_store_every_asked_entry(ctx, good):
    """48 txs, v0 / v1 headers, widths 1 .. 1024, first / last / promoted /
    middle leaves, the padding edges of the prefixed value (0 .. 4096 bytes), of
    a reference (10 + key = 55, 56, 64, 119) and of the digest message (request
    keys of 0 .. 1023 bytes x 0 / 1 / 9 / 10 / 11 metadata bytes; v0: 0, 22, 23,
    24), all 8 metadata flag combinations, expiresAt 0 / 1 / -1 / 2^63 - 1 (0
    is a present-but-empty Expiration on the wire), metadata on v0 answers:
    everything verifies, and gives the new state."""
    cases, exp = good
    assert 350 <= len(cases) <= 3000
    _check(cases, _fused(cases, ctx), exp)
    assert all(e[:2] == (0, True) for e in exp)
    s = V.store()
    assert {len(sl.value) for sl in s.slots if not sl.is_ref} >= set(V.VALUE_LENS)
    assert {10 + len(sl.ref_key) for sl in s.slots if sl.is_ref} >= {55, 56, 64, 119}


def test_go_written_systemdb_entry(ctx, orc, fixtures):
    """the server-written entry of v110_systemdb tx 2 with its Go-written Eh and
    dual proofs (test_verifiable_entry_cpu.py pins the reference on it)"""
    import wire
    from test_verifiable_entry_cpu import _systemdb_answer
    fx = fixtures["v110_systemdb"]
    pairs = {(c["src"], c["tgt"]): c for c in fx["dual_v1"]}
    cases = []
    for S, pair in ((0, (2, 2)), (1, (1, 2)), (2, (2, 2))):
        for flip in (False, True):
            M, key, alhs = _systemdb_answer(wire, fx, pairs[pair], flip)
            cases.append(("systemdb S %d flip %d" % (S, flip), M.SerializeToString(), key, 0, S,
                          alhs[S - 1] if S else bytes(32)))
    exp = _check(cases, _fused(cases, ctx))
    assert [e[1] for e in exp] == [True, False] * 3
    assert exp[0][2:] == (2, alhs[1])


# -------------------------------------------------------------- state, tampering
def test_state_and_at_tx(ctx, orc):
    """S in {0, vTx - 1, vTx, vTx + 1, last} x at_tx in {0, vTx, vTx + 1}, a
    wrong state_alh and another tx's: at_tx = vTx + 1 fails wherever there is a
    state to prove from, and so does every wrong Alh"""
    cases = V.state_cases()
    exp = _check(cases, _fused(cases, ctx))
    for c, e in zip(cases, exp):
        name, S, at = c[0], c[4], c[3]
        if "alh" in name and S:
            assert not e[1], name
        elif at and S and at != int(name.split()[1]):
            assert not e[1], name
        elif "alh" not in name:
            assert e[1], name


def test_tampered(ctx, tampered):
    """one bit in the value, entry.key of a reference, ref.atTx, a metadata
    flag, the request key, an inclusion term, a header's EH, a dual-proof term;
    leaf / width swapped, leaf -1, width 0, a term too many / too few"""
    cases, exp = tampered
    _check(cases, _fused(cases, ctx), exp)
    ok = [e[1] for e in exp]
    assert any(ok) and ok.count(False) > 200
    # what no check reads stays accepted: Go trusts it too
    assert all(e[:2] == (0, True) for c, e in zip(cases, exp) if c[0].startswith("untampered"))


# -------------------------------------------------------------------- encodings
def test_encodings(ctx, orc):
    """fields reversed, entry / inclusionProof split, verifiableTx and dualProof
    twice (the concatenation path: same verdict as unsplit), unknown fields and
    groups, mistyped fields, the 10-byte varint rule, malformed bytes in
    Tx.entries / kvEntries / zEntries / signature, every nil case, tx header
    versions 2 and -1"""
    cases = V.encoding_cases()
    exp = _check(cases, _fused(cases, ctx))
    by = {}
    for c, e in zip(cases, exp):
        by.setdefault(c[0].split(" (")[0], set()).add(e[:2])
    for name in ("plain", "reversed", "entry in two", "inclusionProof in two", "verifiableTx twice",
                 "dualProof twice", "dualProof three times, the first empty",
                 "dualProof twice, its source header in two", "unknown fields", "unknown group",
                 "mistyped known fields", "10-byte varint, 64 bits",
                 "kvEntries / zEntries / signature"):
        assert by[name] == {(0, True)}, name
    for name in ("10-byte varint overflow", "varint overflow inside Tx.entries",
                 "Tx.entries: key runs past its TxEntry", "Tx.zEntries: score cut short",
                 "signature: length past the end", "sub-message longer than its parent"):
        assert by[name] == {(14, False)}, name
    for name in ("no verifiableTx", "no tx", "no header", "no inclusionProof", "no dualProof",
                 "no source header", "no target header", "no linearProof", "no entry"):
        assert by[name] == {(2, False)}, name
    assert by["tx header version 2"] == by["tx header version -1"] == {(21, False)}


def test_hostile_vs_cpu_reference(ctx, hostile):
    """~1500 single-byte mutations and truncations of good answers: each of
    corrupt / decoded and refused / accepted holds >= 5 % of the set
    (test_verifiable_entry_cpu.py asserts it on the reference alone)"""
    cases, exp = hostile
    assert 1300 <= len(cases) <= 1700
    _check(cases, _fused(cases, ctx), exp)


# ----------------------------------------------------------------- launch edges
def test_launch_edges(ctx, good, tampered):
    """n = 1 .. 1025 (lane, wave, workgroup edges), msg_off[0] != 0, one 4 KiB
    value among 255 tiny ones"""
    cases, exp = good
    mixed = [c for pair in zip(cases, tampered[0]) for c in pair]
    mexp = [e for pair in zip(exp, tampered[1]) for e in pair]
    mixed, mexp = mixed * 2, mexp * 2
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        assert len(mixed) >= n
        _check(mixed[:n], _fused(mixed[:n], ctx), mexp[:n])
    _check(mixed[:300], _fused(mixed[:300], ctx, lead=13), mexp[:300])
    big = next(k for k, c in enumerate(cases)
               if 4096 < len(c[1]) < 8192 and len(V.parse(c[1])[1].entry.value) == 4096)
    small = [k for k, c in enumerate(cases) if len(c[1]) < 1500]
    tiny = (small * (255 // len(small) + 1))[:255]
    idx = tiny[:100] + [big] + tiny[100:]
    _check([cases[k] for k in idx], _fused([cases[k] for k in idx], ctx), [exp[k] for k in idx])


def test_chunks(ctx, good, tampered):
    """MH_PB_CHUNK_MIB=1 with MH_PB_GROUP_RATIO=0 over > 3 MiB of answers: at
    least 3 chunks, each decoded and verified on its own"""
    cases = (good[0] + tampered[0])
    exp = good[1] + tampered[1]
    assert sum(len(c[1]) for c in cases) > 3 << 20 and len(cases) <= 3000
    one = _fused(cases, ctx)
    old = {k: os.environ.get(k) for k in ("MH_PB_CHUNK_MIB", "MH_PB_GROUP_RATIO")}
    os.environ["MH_PB_CHUNK_MIB"] = "1"
    try:
        grouped = _fused(cases, ctx)
        os.environ["MH_PB_GROUP_RATIO"] = "0"
        many = _fused(cases, ctx)
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    _check(cases, one, exp)
    for other in (grouped, many):
        for a, b in zip(one, other):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------ composition
def _compose(msgs, keys, at_tx, S, salh, ctx, orc):
    """decode_verifiable_entry_pb, then the existing inclusion and dual-proof
    calls, glued on the host as a caller of the library had to before"""
    import immustore_amd as m
    from immustore_amd import txlayer
    n = len(msgs)
    st, a = txlayer.decode_verifiable_entry_pb(msgs, ctx=ctx)
    info, buf = a["info"], a["buf"].tobytes()
    duals = [a["dual_bytes"][int(a["dual_off"][k]):int(a["dual_off"][k + 1])].tobytes()
             for k in range(n)]
    dst, dec = txlayer.decode_dual_proof_pb(duals, ctx=ctx)
    vtx = [int(at_tx[k]) or int(info["ref_tx"][k] if info["has_ref"][k] else info["entry_tx"][k])
           for k in range(n)]
    fwd = [int(S[k]) <= vtx[k] for k in range(n)]
    hdrs = [dec["tgt_hdr"][k] if fwd[k] else dec["src_hdr"][k] for k in range(n)]
    digests, roots, alh, hok = [], [], [], []
    for k in range(n):
        i = info[k]
        if st[k]:
            digests.append(bytes(32)), roots.append(bytes(32)), alh.append(bytes(32)), hok.append(False)
            continue
        if i["has_ref"]:
            val = b"\x01" + int(i["ref_at_tx"]).to_bytes(8, "big") + b"\x00" + \
                buf[int(i["key_pos"]):int(i["key_pos"] + i["key_len"])]
        else:
            val = b"\x00" + buf[int(i["value_pos"]):int(i["value_pos"] + i["value_len"])]
        key, hval = b"\x00" + bytes(keys[k]), orc.sha256(val)
        md = i["md"][:int(i["md_len"])].tobytes()
        if i["tx_version"] == 0:
            digests.append(orc.sha256(key + hval))
        else:
            digests.append(orc.sha256(len(md).to_bytes(2, "big") + md +
                                      (len(key) & 0xffff).to_bytes(2, "big") + key + hval))
        h = hdrs[k].copy()
        roots.append(h["eh"].tobytes())
        good_hdr = int(h["version"]) <= 1
        if int(h["version"]) == 0:
            h["md_len"] = 0
        e, _, x = orc.tx_header_alh(h, dec["md_blob"].tobytes()) if good_hdr else (1, None, bytes(32))
        alh.append(x if e == 0 else bytes(32))
        hok.append(good_hdr and e == 0)
    iok = m.verify_inclusion_batch(
        [m.InclusionProof(int(info["leaf"][k]), int(info["width"][k]),
                          [t.tobytes() for t in
                           a["incl_terms"][int(a["incl_off"][k]):int(a["incl_off"][k + 1])]])
         for k in range(n)], digests, roots, ctx=ctx)
    src = [int(S[k]) if fwd[k] else vtx[k] for k in range(n)]
    tgt = [vtx[k] if fwd[k] else int(S[k]) for k in range(n)]
    sa = [bytes(salh[k]) if fwd[k] else alh[k] for k in range(n)]
    ta = [alh[k] if fwd[k] else bytes(salh[k]) for k in range(n)]
    _, dok = txlayer.verify_dual_proof_pb_batch(duals, src, tgt, sa, ta, ctx=ctx)
    ok = [st[k] == 0 and bool(iok[k]) and hok[k] and (int(S[k]) == 0 or bool(dok[k])) for k in range(n)]
    return (st, ok, [tgt[k] if ok[k] else 0 for k in range(n)],
            [ta[k] if ok[k] else bytes(32) for k in range(n)])


def test_decode_vs_protobuf_and_composition(ctx, orc, good, tampered, hostile):
    """the envelope pass alone == the protobuf runtime's view of every message;
    composed with mh_htree_verify_inclusion_batch and
    mh_verify_dual_proof_pb_batch by host glue it gives the fused call's
    results on the good, tampered and hostile sets"""
    from immustore_amd import txlayer
    cases = good[0][::4] + tampered[0][::2] + V.encoding_cases()[::3] + hostile[0][::2]
    assert len(cases) <= 3000
    msgs = [c[1] for c in cases]
    st, a = txlayer.decode_verifiable_entry_pb(msgs, ctx=ctx)
    DP = V.messages()["DualProof"]
    off = np.concatenate([[0], np.cumsum([len(x) for x in msgs])])
    buf = a["buf"].tobytes()
    for k, raw in enumerate(msgs):
        est, e = V.expect_decode(raw)
        assert int(st[k]) == est, (k, cases[k][0])
        i = a["info"][k]
        if est:
            assert i.tobytes() == bytes(96)
            assert a["incl_off"][k] == a["incl_off"][k + 1] and a["dual_off"][k] == a["dual_off"][k + 1]
            continue
        kp, kl, vp, vl = (int(i[f]) for f in ("key_pos", "key_len", "value_pos", "value_len"))
        assert off[k] <= kp and kp + kl <= off[k + 1] and off[k] <= vp and vp + vl <= off[k + 1]
        got = {"entry_tx": int(i["entry_tx"]), "has_ref": bool(i["has_ref"]), "ref_tx": int(i["ref_tx"]),
               "ref_at_tx": int(i["ref_at_tx"]), "key": buf[kp:kp + kl], "value": buf[vp:vp + vl],
               "md": i["md"][:int(i["md_len"])].tobytes(), "version": int(i["tx_version"]),
               "leaf": int(i["leaf"]), "width": int(i["width"]),
               "terms": [t.tobytes() for t in
                         a["incl_terms"][int(a["incl_off"][k]):int(a["incl_off"][k + 1])]]}
        assert got == {f: v for f, v in e.items() if f != "dual"}, (k, cases[k][0])
        d = a["dual_bytes"][int(a["dual_off"][k]):int(a["dual_off"][k + 1])].tobytes()
        assert DP.FromString(d) == e["dual"], (k, cases[k][0])
    fused = _fused(cases, ctx)
    cst, cok, cntx, calh = _compose(msgs, [c[2] for c in cases], [c[3] for c in cases],
                                    [c[4] for c in cases], [c[5] for c in cases], ctx, orc)
    assert list(fused[0]) == list(cst)
    assert list(fused[1]) == list(cok)
    assert [int(x) for x in fused[2]] == cntx
    assert [x.tobytes() for x in fused[3]] == calh


def test_decode_capacity(ctx, good):
    """short capacities: offsets, statuses and info are filled and
    MH_ERR_BUFFER_TOO_SMALL comes back; n == 0 writes the two zero offsets"""
    import ctypes as C
    from immustore_amd import _native as N
    from immustore_amd.txlayer import VERIFIABLE_ENTRY_INFO, _VerifiableEntryDecoded, _addr
    msgs = [c[1] for c in good[0][:40]]
    n = len(msgs)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
    info = np.zeros(n, VERIFIABLE_ENTRY_INFO)
    io, do = np.full(n + 1, 7, np.uint64), np.full(n + 1, 7, np.uint64)
    st = np.full(n, -1, np.int32)
    L = N.load()
    d = _VerifiableEntryDecoded(_addr(info), _addr(io), None, 0, _addr(do), None, 0)
    assert L.mh_verifiable_entry_pb_decode_batch(ctx.handle, n, _addr(buf), _addr(off), C.byref(d),
                                                 _addr(st)) == N.MH_ERR_BUFFER_TOO_SMALL
    assert (st == 0).all() and io[0] == 0 and do[0] == 0 and io[n] > 0 and do[n] > 0
    assert (info["width"] > 0).all()
    terms, dual = np.zeros((int(io[n]), 32), np.uint8), np.zeros(int(do[n]), np.uint8)
    d = _VerifiableEntryDecoded(_addr(info), _addr(io), _addr(terms), int(io[n]) - 1, _addr(do),
                                _addr(dual), int(do[n]))
    assert L.mh_verifiable_entry_pb_decode_batch(ctx.handle, n, _addr(buf), _addr(off), C.byref(d),
                                                 _addr(st)) == N.MH_ERR_BUFFER_TOO_SMALL
    assert not terms.any() and not dual.any()
    d = _VerifiableEntryDecoded(_addr(info), _addr(io), _addr(terms), int(io[n]), _addr(do),
                                _addr(dual), int(do[n]))
    assert L.mh_verifiable_entry_pb_decode_batch(ctx.handle, n, _addr(buf), _addr(off), C.byref(d),
                                                 _addr(st)) == 0
    assert terms.any() and dual.any()
    io[0] = do[0] = 9
    assert L.mh_verifiable_entry_pb_decode_batch(ctx.handle, 0, None, None, C.byref(d), None) == 0
    assert io[0] == 0 and do[0] == 0


# ------------------------------------------------------------------------ multi
def test_multi_equals_single(m, ctx, good, tampered, hostile):
    """contexts on device 0 listed 1, 2 and 4 times == the single-device call"""
    from immustore_amd.multi import MultiDevice
    cases = good[0][::3] + tampered[0][::3] + hostile[0][::3]
    one = _fused(cases, ctx)
    for K in (1, 2, 4):
        mc = MultiDevice([0] * K)
        try:
            got = mc.verify_verifiable_entry_pb_batch(
                [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                [c[4] for c in cases], [c[5] for c in cases])
        finally:
            mc.close()
        for a, b in zip(one, got):
            assert np.array_equal(a, b), K
    assert one[1].any() and not one[1].all()


# -------------------------------------------------------------------- arguments
def test_arguments(m, ctx, good):
    import ctypes as C
    from immustore_amd import _native as N
    from immustore_amd.txlayer import _VerifiedGetBatch, pack_verified_get_batch, _addr
    L = N.load()
    cases = good[0][:50]
    n = len(cases)
    b, keep = pack_verified_get_batch([c[1] for c in cases], [c[2] for c in cases],
                                      [c[3] for c in cases], [c[4] for c in cases],
                                      [c[5] for c in cases])
    st, ok = np.full(n, -1, np.int32), np.full(n, 7, np.uint8)
    ntx, nalh = np.full(n, 7, np.uint64), np.full((n, 32), 7, np.uint8)
    outs = [_addr(st), _addr(ok), _addr(ntx), _addr(nalh)]
    fn = L.mh_verify_verifiable_entry_pb_batch
    # n == 0: nothing read, nothing written
    empty = _VerifiedGetBatch(0, *([None] * 7))
    assert fn(ctx.handle, C.byref(empty), *([None] * 4)) == 0
    # a null context, a null batch, each null pointer of the batch, each null output
    assert fn(None, C.byref(b), *outs) == 2
    assert fn(ctx.handle, None, *outs) == 2
    fields = [f for f, _ in _VerifiedGetBatch._fields_[1:]]
    for f in fields:
        bad = _VerifiedGetBatch(n, *[None if g == f else getattr(b, g) for g in fields])
        assert fn(ctx.handle, C.byref(bad), *outs) == 2, f
    for k in range(4):
        o = list(outs)
        o[k] = None
        assert fn(ctx.handle, C.byref(b), *o) == 2, k
    # offsets running backwards: the messages', the keys'
    for which, arr in (("msg_off", keep[1]), ("key_off", keep[3])):
        x = arr.copy()
        x[5], x[7] = x[7] + 1, x[5]
        bad = _VerifiedGetBatch(n, *[_addr(x) if g == which else getattr(b, g) for g in fields])
        assert fn(ctx.handle, C.byref(bad), *outs) == 2, which
    # more answers than the V2 call takes
    bad = _VerifiedGetBatch(8013009, *[getattr(b, g) for g in fields])
    assert fn(ctx.handle, C.byref(bad), *outs) == 2
    assert (st == -1).all() and (ok == 7).all() and (ntx == 7).all() and (nalh == 7).all()
    # the batch itself
    assert fn(ctx.handle, C.byref(b), *outs) == 0
    assert (st == 0).all() and (ok == 1).all()
    exp = good[1][:n]
    assert [int(x) for x in ntx] == [e[2] for e in exp]
    # a sub-range: every array advanced alike, msg_off[0] and key_off[0] != 0
    lo, cnt = 11, 30
    sub = _VerifiedGetBatch(cnt, b.msgs, b.msg_off + 8 * lo, b.keys, b.key_off + 8 * lo,
                            b.at_tx + 8 * lo, b.state_tx + 8 * lo, b.state_alh + 32 * lo)
    st2, ok2 = np.full(cnt, -1, np.int32), np.zeros(cnt, np.uint8)
    ntx2, nalh2 = np.zeros(cnt, np.uint64), np.zeros((cnt, 32), np.uint8)
    assert fn(ctx.handle, C.byref(sub), _addr(st2), _addr(ok2), _addr(ntx2), _addr(nalh2)) == 0
    assert (st2 == 0).all() and (ok2 == 1).all()
    assert np.array_equal(ntx2, ntx[lo:lo + cnt]) and np.array_equal(nalh2, nalh[lo:lo + cnt])
    del keep
