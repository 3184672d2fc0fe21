"""mh_verify_dual_proof_pb_batch / mh_multi_verify_dual_proof_pb_batch:
DualProof (v1) messages decoded and verified in one device pass
(DualProofFromProto + store.VerifyDualProof, verification.go:127-235) against
the C oracle, the CPU reference of dual_v1_verify_util.py and the composition
of the two existing device calls (mh_dual_proof_pb_decode_batch, then
mh_verify_dual_proof_batch).  Both verify calls run dual_proof_v1_core; the
last section drives the array call on its own (CSR bases, lane and grid edges,
the header rules, its argument checks) and pins the one difference between the
two: a v0 header that carries metadata."""
import ctypes as C
import os

import numpy as np
import pytest

import dual_v1_gen_util as U

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


@pytest.fixture(scope="module")
def wire(orc):
    import wire
    return wire


@pytest.fixture(scope="module")
def go_cases(wire, fixtures):
    """every dual_v1 case of the Go stores x {none, lap, lin, last, tbl}:
    (orc.verify_dual_proof arguments, message)"""
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture
    out = []
    for name, fx in fixtures.items():
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        for c in fx["dual_v1"]:
            for tamper in (None, "lap", "lin", "last", "tbl"):
                a = dual_v1_args(c, recs, blob, alhs, tamper)
                out.append((a, dual_v1_msg(wire, a)))
    return out


@pytest.fixture(scope="module")
def synthetic(m, ctx, orc):
    """the device-generated messages of the synthetic store's pairs ->
    (msgs, S, T, SA, TA)"""
    s = U.synthetic_store()
    pairs = U.synthetic_pairs()
    t = m.AHtree(ctx)
    try:
        t.append_batch(np.stack([np.frombuffer(bytes(p), np.uint8) for p in s.alhs]))
        msgs, st = t.dual_proof_pb_batch(s.recs[[a - 1 for a, _ in pairs]],
                                         s.recs[[b - 1 for _, b in pairs]], s.blob, 1, s.alhs,
                                         s.inners)
    finally:
        t.close()
    assert (np.asarray(st) == 0).all()
    return ([bytes(x) for x in msgs], [a for a, _ in pairs], [b for _, b in pairs],
            [s.alhs[a - 1] for a, _ in pairs], [s.alhs[b - 1] for _, b in pairs])


def _compose(txlayer, msgs, S, T, SA, TA, ctx):
    """the two existing calls, with Go's v0 rule (a v0 header's metadata is not
    hashed) -> (status, ok)"""
    st, dec = txlayer.decode_dual_proof_pb(list(msgs), ctx=ctx)
    for h in (dec["src_hdr"], dec["tgt_hdr"]):
        h["md_len"][h["version"] == 0] = 0
    ok = txlayer.verify_decoded_dual_proof_batch(dec, S, T, SA, TA, ctx=ctx)
    return st, ok & (st == 0)


@pytest.fixture(scope="module")
def hostile(m, ctx, orc, wire, go_cases, synthetic):
    """~1500 messages nobody meant well: single-byte mutations and truncations
    of fixture and synthetic messages, a few of them untouched, and random
    protobuf-built ones; ids and Alh values are the right ones where the
    message still tells them -> (msgs, S, T, SA, TA, fused status, fused ok)"""
    from immustore_amd import txlayer
    from test_gpu_pb_decode import random_dual_v1_msg
    rng = np.random.default_rng(2024)
    base = [(msg, a[9], a[10], a[11], a[12]) for a, msg in go_cases[::10]]  # untampered ones
    sm, sS, sT, sSA, sTA = synthetic
    base += [(sm[k], sS[k], sT[k], sSA[k], sTA[k]) for k in range(0, len(sm), 3)]
    msgs, S, T, SA, TA = [], [], [], [], []

    def add(b, k):
        msgs.append(bytes(b))
        S.append(base[k][1])
        T.append(base[k][2])
        SA.append(base[k][3])
        TA.append(base[k][4])

    for k in range(len(base)):
        raw = base[k][0]
        if k % 12 == 0:
            add(raw, k)  # untouched
        b = bytearray(raw)
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        add(b, k)
        if k % 2 == 0:  # a mutation near the front: headers, the first lengths
            b = bytearray(raw)
            b[int(rng.integers(0, min(len(b), 300)))] ^= 1 << int(rng.integers(0, 8))
            add(b, k)
        else:
            add(raw[:int(rng.integers(0, len(raw)))], k)
    for _ in range(500):
        raw = random_dual_v1_msg(wire, rng)
        msgs.append(raw)
        # the message's own ids, and for every other one its headers' real Alh
        # values, so that the checks past the Alh comparison see random proofs
        s_, t_, sa, ta = int(rng.integers(1, 5)), int(rng.integers(1, 5)), bytes(32), bytes(32)
        try:
            M = wire.MSG["DualProof"].FromString(raw)
            s_, t_ = M.sourceTxHeader.id, M.targetTxHeader.id
            if rng.random() < 0.5:
                from dual_v1_verify_util import _header
                for which, h in ((0, M.sourceTxHeader), (1, M.targetTxHeader)):
                    r, md = _header(h)
                    e, _, alh = orc.tx_header_alh(r, md)
                    if e == 0 and which == 0:
                        sa = bytes(alh)
                    elif e == 0:
                        ta = bytes(alh)
        except Exception:  # noqa: BLE001  (not a message: keep the random ids)
            pass
        S.append(s_)
        T.append(t_)
        SA.append(sa)
        TA.append(ta)
    st, ok = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
    return msgs, S, T, SA, TA, st, ok


# ------------------------------------------------------------------ 1. Go stores
def test_go_stores(ctx, orc, go_cases):
    from immustore_amd import txlayer
    args = [a for a, _ in go_cases]
    assert len(args) == 2390
    st, ok = txlayer.verify_dual_proof_pb_batch([msg for _, msg in go_cases],
                                                [a[9] for a in args], [a[10] for a in args],
                                                [a[11] for a in args], [a[12] for a in args], ctx=ctx)
    assert (st == 0).all()
    exp = [orc.verify_dual_proof(*a) for a in args]
    assert list(ok) == exp
    assert sum(exp) > 400 and not all(exp)


# ------------------------------------------------------------ 2. synthetic store
def test_synthetic_store(ctx, synthetic):
    """458 device-generated messages (1/2/3-byte sub-message lengths, 63 / 64 /
    65 nested proofs, the nil advance proof, tgt.bl == 0, src == tgt) all
    verify; with source and target swapped, tgt + 1 or a zero source Alh none
    with src != tgt does."""
    from immustore_amd import txlayer
    msgs, S, T, SA, TA = synthetic
    assert len(msgs) == 458
    st, ok = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
    assert (st == 0).all()
    assert ok.all(), [(S[k], T[k]) for k in np.nonzero(~ok)[0][:10]]
    diff = np.array([a != b for a, b in zip(S, T)])
    assert diff.sum() > 400
    variants = {"swapped": (T, S, TA, SA), "tgt + 1": (S, [t + 1 for t in T], SA, TA),
                "zero src_alh": (S, T, [bytes(32)] * len(S), TA)}
    for name, (s_, t_, sa, ta) in variants.items():
        st, ok = txlayer.verify_dual_proof_pb_batch(msgs, s_, t_, sa, ta, ctx=ctx)
        assert (st == 0).all(), name
        assert not ok[diff].any(), (name, [(S[k], T[k]) for k in np.nonzero(ok & diff)[0][:10]])


# ---------------------------------------------------------------- 3. hostile input
def test_hostile_vs_composition(ctx, hostile):
    from immustore_amd import txlayer
    msgs, S, T, SA, TA, st, ok = hostile
    assert 1300 <= len(msgs) <= 1700
    cst, cok = _compose(txlayer, msgs, S, T, SA, TA, ctx)
    assert list(st) == list(cst)
    bad = np.nonzero(ok != cok)[0]
    assert bad.size == 0, [(int(k), msgs[k][:64].hex()) for k in bad[:5]]
    assert {0, 2, 14} <= set(st.tolist())
    assert ok[st == 0].any() and not ok[st == 0].all()
    assert not ok[st != 0].any()


def test_hostile_vs_cpu_reference(orc, wire, hostile):
    from dual_v1_verify_util import reference
    msgs, S, T, SA, TA, st, ok = hostile
    for k, raw in enumerate(msgs):
        assert (int(st[k]), bool(ok[k])) == reference(wire, orc, raw, S[k], T[k], SA[k], TA[k]), \
            (k, len(raw), raw[:64].hex())


# --------------------------------------------------------------------- 4. chunks
def test_chunks(ctx, wire, synthetic):
    """17 MB of messages in 1 MiB chunks (MH_PB_CHUNK_MIB=1), decoded chunk by
    chunk (MH_PB_GROUP_RATIO=0) or in the call's own groups of chunks, give
    the arrays of the single default chunk; one message longer than a chunk
    is a chunk of its own."""
    from immustore_amd import txlayer
    from test_gpu_pb_decode import tag
    msgs, S, T, SA, TA = (list(x) for x in synthetic)
    pad = 3 << 19  # 1.5 MiB in an unknown length-delimited field
    ln, v = b"", pad
    while v >= 0x80:
        ln += bytes([v & 0x7f | 0x80])
        v >>= 7
    big = msgs[40] + tag(20, 2) + ln + bytes([v]) + bytes(range(256)) * (pad // 256)
    k = 200
    for arr, x in ((msgs, big), (S, S[40]), (T, T[40]), (SA, SA[40]), (TA, TA[40])):
        arr.insert(k, x)
    total = sum(len(x) for x in msgs)
    assert total >= 10 << 20
    one = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
    old = {k: os.environ.get(k) for k in ("MH_PB_CHUNK_MIB", "MH_PB_GROUP_RATIO")}
    os.environ["MH_PB_CHUNK_MIB"] = "1"
    try:
        # 1 MiB copies, decoded in the groups the call forms by itself
        grouped = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
        # ... and every chunk decoded alone: at least 10 sets of launches
        os.environ["MH_PB_GROUP_RATIO"] = "0"
        many = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
        # a neighbour broken: only its own verdict changes, in its own chunk
        msgs2 = list(msgs)
        msgs2[k + 1] = msgs2[k + 1][:-7]
        cut = txlayer.verify_dual_proof_pb_batch(msgs2, S, T, SA, TA, ctx=ctx)
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    assert (one[0] == 0).all() and one[1].all()
    assert np.array_equal(many[0], one[0]) and np.array_equal(many[1], one[1])
    assert np.array_equal(grouped[0], one[0]) and np.array_equal(grouped[1], one[1])
    assert cut[0][k + 1] == 14 and not cut[1][k + 1]
    assert (np.delete(cut[0], k + 1) == 0).all() and np.delete(cut[1], k + 1).all()


# ------------------------------------------------------------------ 5. arguments
def test_arguments(m, ctx, synthetic):
    from immustore_amd import _native as N
    from immustore_amd import txlayer
    from immustore_amd.txlayer import _Pinned, _addr, _d32
    L = N.load()
    msgs, S, T, SA, TA = (x[:60] for x in synthetic)
    n = len(msgs)
    buf = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
    s_, t_ = np.asarray(S, np.uint64), np.asarray(T, np.uint64)
    sa, ta = _d32(SA, n), _d32(TA, n)
    st, ok = np.full(n, -1, np.int32), np.full(n, 7, np.uint8)
    ptrs = [_addr(buf), _addr(off), _addr(s_), _addr(t_), _addr(sa), _addr(ta), _addr(st), _addr(ok)]
    fn = L.mh_verify_dual_proof_pb_batch
    # n == 0: nothing read, nothing written
    assert fn(ctx.handle, 0, *([None] * 8)) == 0
    assert (st == -1).all() and (ok == 7).all()
    # each null pointer, a null context
    assert fn(None, n, *ptrs) == 2
    for k in range(8):
        p = list(ptrs)
        p[k] = None
        assert fn(ctx.handle, n, *p) == 2, k
    assert (st == -1).all() and (ok == 7).all()
    # offsets running backwards
    bad = off.copy()
    bad[5], bad[6] = bad[6], bad[5]
    assert fn(ctx.handle, n, ptrs[0], _addr(bad), *ptrs[2:]) == 2
    # the whole batch, pageable
    assert fn(ctx.handle, n, *ptrs) == 0
    assert (st == 0).all() and (ok == 1).all()
    # a sub-range: msg_off[0] != 0, every per-message array advanced alike
    lo, cnt = 17, 30
    st2, ok2 = np.full(cnt, -1, np.int32), np.full(cnt, 7, np.uint8)
    assert fn(ctx.handle, cnt, ptrs[0], _addr(off) + 8 * lo, _addr(s_) + 8 * lo, _addr(t_) + 8 * lo,
              _addr(sa) + 32 * lo, _addr(ta) + 32 * lo, _addr(st2), _addr(ok2)) == 0
    assert (st2 == 0).all() and (ok2 == 1).all()
    # ... and the wrong ids for that range are refused
    assert fn(ctx.handle, cnt, ptrs[0], _addr(off) + 8 * lo, _addr(s_), _addr(t_), _addr(sa) + 32 * lo,
              _addr(ta) + 32 * lo, _addr(st2), _addr(ok2)) == 0
    assert (st2 == 0).all() and ok2.sum() < cnt
    # pinned message buffer (and pinned offsets)
    pb, po = _Pinned(buf), _Pinned(off)
    st3, ok3 = np.full(n, -1, np.int32), np.full(n, 7, np.uint8)
    assert fn(ctx.handle, n, _addr(pb.a), _addr(po.a), *ptrs[2:6], _addr(st3), _addr(ok3)) == 0
    assert (st3 == 0).all() and (ok3 == 1).all()
    # a zero-length message among good ones: no headers -> status 2, ok 0
    st4, ok4 = txlayer.verify_dual_proof_pb_batch([msgs[0], b"", msgs[2]], [S[0], 1, S[2]],
                                                  [T[0], 1, T[2]], [SA[0], bytes(32), SA[2]],
                                                  [TA[0], bytes(32), TA[2]], ctx=ctx)
    assert list(st4) == [0, 2, 0] and list(ok4) == [True, False, True]
    st5, ok5 = txlayer.verify_dual_proof_pb_batch([], [], [], [], [], ctx=ctx)
    assert st5.size == 0 and ok5.size == 0


# ---------------------------------------------------------------------- 6. multi
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0, 0]])
def test_multi(devices, hostile):
    """1, 2 and 4 contexts on device 0 (parts of nearly equal message bytes):
    the single-context arrays; fewer messages than contexts go to context 0."""
    from immustore_amd.multi import MultiDevice
    msgs, S, T, SA, TA, st, ok = hostile
    md = MultiDevice(devices)
    try:
        gst, gok = md.verify_dual_proof_pb_batch(msgs, S, T, SA, TA)
        assert np.array_equal(gst, st) and np.array_equal(gok, ok)
        few = max(len(devices) - 1, 1)
        gst, gok = md.verify_dual_proof_pb_batch(msgs[:few], S[:few], T[:few], SA[:few], TA[:few])
        assert np.array_equal(gst, st[:few]) and np.array_equal(gok, ok[:few])
        gst, gok = md.verify_dual_proof_pb_batch([], [], [], [], [])
        assert gst.size == 0 and gok.size == 0
    finally:
        md.close()


# ------------------------------------------- 7. the array call, mh_verify_dual_proof_batch
# bytes per proof of the per-proof arrays of mh_dual_proof_batch
_PER_PROOF = {"src_hdr": 136, "tgt_hdr": 136, "incl_off": 8, "cons_off": 8, "target_bl_tx_alh": 32,
              "last_off": 8, "has_linear": 1, "linear_src": 8, "linear_tgt": 8, "linear_off": 8,
              "has_advance": 1, "advance_off": 8, "advance_incl_first": 8, "src": 8, "tgt": 8,
              "src_alh": 32, "tgt_alh": 32}
MH_MAX_TX_METADATA_LEN = 268


def _arrays(args):
    """orc.verify_dual_proof argument tuples -> the arrays of mh_dual_proof_batch
    (all but md_blob), every offset array from 0"""
    from immustore_amd.txlayer import _d32, _hdrs, _terms_csr
    n = len(args)
    a = {"src_hdr": _hdrs(np.array([x[0] for x in args])),
         "tgt_hdr": _hdrs(np.array([x[1] for x in args]))}
    for name, col in (("incl", 3), ("cons", 4), ("last", 6)):
        a[name + "_off"], a[name + "_terms"] = _terms_csr([x[col] for x in args])
    lin, adv = [x[7] for x in args], [x[8] for x in args]
    a["has_linear"] = np.array([x is not None for x in lin], np.uint8)
    a["linear_src"] = np.array([x[0] if x is not None else 0 for x in lin], np.uint64)
    a["linear_tgt"] = np.array([x[1] if x is not None else 0 for x in lin], np.uint64)
    a["linear_off"], a["linear_terms"] = _terms_csr([x[2] if x is not None else [] for x in lin])
    a["has_advance"] = np.array([x is not None for x in adv], np.uint8)
    a["advance_off"], a["advance_terms"] = _terms_csr([x[0] if x is not None else [] for x in adv])
    nested = [x[1] if x is not None else [] for x in adv]
    a["advance_incl_first"] = np.zeros(n + 1, np.uint64)
    a["advance_incl_first"][1:] = np.cumsum([len(x) for x in nested], dtype=np.uint64)
    a["advance_incl_off"], a["advance_incl_terms"] = _terms_csr([ip for ns in nested for ip in ns])
    a["target_bl_tx_alh"] = _d32([x[5] for x in args], n)
    a["src"] = np.array([x[9] for x in args], np.uint64)
    a["tgt"] = np.array([x[10] for x in args], np.uint64)
    a["src_alh"], a["tgt_alh"] = _d32([x[11] for x in args], n), _d32([x[12] for x in args], n)
    return a


def _call(ctx, a, lo=0, n=None, md_blob=None, md_blob_len=None):
    """mh_verify_dual_proof_batch over proofs [lo, lo + n) of the arrays: every
    per-proof pointer advanced by lo, the term pointers at the arrays' start
    -> (return code, ok[n], 7 where the call wrote nothing)"""
    from immustore_amd import _native as N
    from immustore_amd.txlayer import _DualProofBatch, _addr
    n = a["src"].size - lo if n is None else n
    kw = {name: _addr(a[name]) + lo * _PER_PROOF.get(name, 0)
          for name, _ in _DualProofBatch._fields_ if name not in ("n", "md_blob", "md_blob_len")}
    if md_blob_len is None:
        md_blob_len = 0 if md_blob is None else md_blob.size
    b = _DualProofBatch(n=n, md_blob=_addr(md_blob), md_blob_len=md_blob_len, **kw)
    ok = np.full(n, 7, np.uint8)
    rc = N.load().mh_verify_dual_proof_batch(ctx.handle, C.byref(b), _addr(ok))
    return rc, ok


@pytest.fixture(scope="module")
def mixed(orc, fixtures):
    """the 478 dual_v1 cases of the Go stores, case k with tamper k % 5 of
    (none, lap, lin, last, tbl) -> (arguments, oracle verdicts, arrays)"""
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture
    args = []
    for name, fx in fixtures.items():
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        assert blob == b""
        for c in fx["dual_v1"]:
            tamper = (None, "lap", "lin", "last", "tbl")[len(args) % 5]
            args.append(dual_v1_args(c, recs, blob, alhs, tamper))
    assert len(args) == 478
    return args, [orc.verify_dual_proof(*x) for x in args], _arrays(args)


def _span(x):
    """(start, end) of the linear advance proof of an argument tuple
    (verification.go:191-233)"""
    s, sbl, tbl = int(x[9]), int(x[0]["bl_tx_id"]), int(x[1]["bl_tx_id"])
    return sbl, (s if s < tbl else tbl)


def test_arrays_nonzero_csr_bases(ctx, mixed):
    """100 proofs from case 300 on (the first 284 cases carry no advance terms,
    a window at 200 would start two of the arrays at 0): every offset array
    starts above 0 while the term pointers stay at the arrays' start."""
    args, exp, a = mixed
    lo, n = 300, 100
    first = a["advance_incl_first"]
    for name in ("incl_off", "cons_off", "last_off", "linear_off", "advance_off",
                 "advance_incl_first"):
        assert a[name][lo] != 0, name
    assert a["advance_incl_off"][int(first[lo])] != 0
    assert first[lo + n] > first[lo]  # nested inclusion proofs inside the window
    assert any(exp[lo:lo + n]) and not all(exp[lo:lo + n])
    rc, ok = _call(ctx, a, lo, n)
    assert rc == 0
    assert [bool(x) for x in ok] == exp[lo:lo + n]


@pytest.mark.parametrize("n", [1, 256, 257])
def test_arrays_lane_and_grid_edges(ctx, mixed, n):
    args, exp, _ = mixed
    pick = [(285 + 3 * k) % len(args) for k in range(n)]
    # n = 1: a proof that verifies through its nested inclusion proofs
    assert exp[pick[0]] and args[pick[0]][8] is not None and any(args[pick[0]][8][1])
    rc, ok = _call(ctx, _arrays([args[k] for k in pick]))
    assert rc == 0
    assert [bool(x) for x in ok] == [exp[k] for k in pick]


def test_arrays_no_nested_proofs(ctx, mixed):
    """Q = 0: no proof's chain runs (end <= start + 1 everywhere), the nested
    launches are skipped."""
    args, exp, _ = mixed
    pick = [k for k, x in enumerate(args)
            if _span(x)[1] <= _span(x)[0] + 1 and not (x[8] and x[8][1])][:70]
    assert len(pick) >= 20
    a = _arrays([args[k] for k in pick])
    assert a["advance_incl_first"][len(pick)] == 0
    rc, ok = _call(ctx, a)
    assert rc == 0
    assert [bool(x) for x in ok] == [exp[k] for k in pick]
    assert any(exp[k] for k in pick) and not all(exp[k] for k in pick)


def test_arrays_header_rules_on_device(ctx, mixed):
    """One proof that verifies, one thing changed at a time: false, the call
    itself MH_OK, and the neighbours keep their verdicts."""
    args, exp, _ = mixed
    v = next(k for k, x in enumerate(args)
             if exp[k] and _span(x)[1] > _span(x)[0] + 2 and x[8] and len(x[8][1]) >= 2)
    pick = [v - 2, v - 1, v, v + 1, v + 2]
    want = [exp[k] for k in pick]
    blob = np.arange(64, dtype=np.uint8)

    def run(change=None, swap=None, **kw):
        batch = [args[k] for k in pick]
        if swap:
            batch[2] = batch[2][:8] + (swap(batch[2][8]),) + batch[2][9:]
        a = _arrays(batch)
        if change:
            change(a)
        rc, ok = _call(ctx, a, **kw)
        assert rc == 0
        return [bool(x) for x in ok]

    assert run(md_blob=blob) == want and want[2]

    def hdr(which, **fields):
        def change(a):
            for f, val in fields.items():
                a[which][f][2] = val
        return change

    def flag(name):
        def change(a):
            a[name][2] = 0
        return change

    variants = {
        "v0 source header with metadata": dict(change=hdr("src_hdr", version=0, md_len=5), md_blob=blob),
        "target header version 2": dict(change=hdr("tgt_hdr", version=2), md_blob=blob),
        "metadata past the blob": dict(change=hdr("src_hdr", version=1, md_len=4, md_off=blob.size - 3),
                                       md_blob=blob),
        "metadata without a blob": dict(change=hdr("tgt_hdr", version=1, md_len=4, md_off=0)),
        "metadata too long": dict(change=hdr("src_hdr", version=1, md_len=MH_MAX_TX_METADATA_LEN + 1,
                                             md_off=0),
                                  md_blob=np.zeros(512, np.uint8)),
        "no advance proof": dict(change=flag("has_advance"), md_blob=blob),
        "advance terms one short": dict(swap=lambda lap: (lap[0][:-1], lap[1]), md_blob=blob),
        "nested proofs one short": dict(swap=lambda lap: (lap[0], lap[1][:-1]), md_blob=blob),
        "no linear proof": dict(change=flag("has_linear"), md_blob=blob),
    }
    for name, kw in variants.items():
        assert run(**kw) == want[:2] + [False] + want[3:], name


def test_arrays_nested_offsets_checked(ctx, mixed):
    """advance_incl_off running backwards inside [first[0], first[n]] is
    refused before anything is launched; outside that window it is not read."""
    args, exp, a = mixed
    lo, n = 300, 100
    q0, q1 = int(a["advance_incl_first"][lo]), int(a["advance_incl_first"][lo + n])
    off = a["advance_incl_off"]
    assert q0 >= 1 and q1 + 1 < off.size
    k = next(q for q in range(q0, q1) if off[q + 1] > off[q])
    bad = dict(a, advance_incl_off=off.copy())
    bad["advance_incl_off"][[k, k + 1]] = off[[k + 1, k]]
    rc, ok = _call(ctx, bad, lo, n)
    assert rc == 2 and (ok == 7).all()
    outside = dict(a, advance_incl_off=off.copy())
    outside["advance_incl_off"][0] = 1 << 40  # above entry 1
    outside["advance_incl_off"][-1] = 0       # below the entry before it
    rc, ok = _call(ctx, outside, lo, n)
    assert rc == 0
    assert [bool(x) for x in ok] == exp[lo:lo + n]


def test_v0_metadata_wire_drops_arrays_refuse(ctx, orc, wire, mixed):
    """The one intended difference between the two callers of the verifier: a
    v0 source header that carries metadata on the wire.  The fused call drops
    the metadata as Go's innerHash does (tx.go:258-263): the CPU reference's
    verdict.  The array call on the decoded arrays keeps check_header's rule:
    false.  (_compose above zeroes md_len of decoded v0 headers before the
    array call, which is why the composition test sees no difference.)"""
    from dual_v1_verify_util import reference
    from immustore_amd import txlayer
    from test_gpu_pb_decode import dual_v1_msg
    args, exp, _ = mixed
    pick = [k for k, x in enumerate(args) if exp[k] and int(x[0]["version"]) == 0][:3]
    assert len(pick) == 3
    msgs = [dual_v1_msg(wire, args[k]) for k in pick]
    M = wire.MSG["DualProof"].FromString(msgs[1])
    M.sourceTxHeader.metadata.truncatedTxID = 5
    msgs[1] = M.SerializeToString()
    S, T = [args[k][9] for k in pick], [args[k][10] for k in pick]
    SA, TA = [args[k][11] for k in pick], [args[k][12] for k in pick]
    ref = [reference(wire, orc, msgs[k], S[k], T[k], SA[k], TA[k]) for k in range(3)]
    assert ref == [(0, True)] * 3
    st, ok = txlayer.verify_dual_proof_pb_batch(msgs, S, T, SA, TA, ctx=ctx)
    assert [(int(a), bool(b)) for a, b in zip(st, ok)] == ref
    st, dec = txlayer.decode_dual_proof_pb(msgs, ctx=ctx)
    assert (st == 0).all()
    assert dec["src_hdr"]["version"][1] == 0 and dec["src_hdr"]["md_len"][1] == 9
    ok = txlayer.verify_decoded_dual_proof_batch(dec, S, T, SA, TA, ctx=ctx)
    assert list(ok) == [True, False, True]
