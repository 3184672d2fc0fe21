"""The expectation of the generated-answer tests checked (no GPU): answer_util
reproduces every DualProof the Go stores emitted, every expected answer passes
the restated client checks, the synthetic store holds what it promises, and
the call's host-side argument checks."""
import ctypes as C

import numpy as np
import pytest

import answer_util as A

STORES = ("long_linear_proof", "v110_defaultdb", "v110_systemdb")


@pytest.fixture(scope="module")
def wire(orc):
    import wire
    return wire


def test_dual_proofs_match_go_stores(orc, wire, fixtures):
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture
    n = 0
    assert set(fixtures) == set(STORES)
    for name in STORES:
        fx = fixtures[name]
        s = A.fixture_store(fx)
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        assert s.alhs == alhs and not any(s.rst), name
        for c in fx["dual_v1"]:
            st, raw = s.dual(c["src"], c["tgt"])
            assert st == 0 and raw == dual_v1_msg(wire, dual_v1_args(c, recs, blob, alhs)), \
                (name, c["src"], c["tgt"])
            n += 1
    assert n == 478


def test_go_store_answers_pass_the_client(orc, fixtures):
    import verifiable_tx_util as VT
    for name in STORES:
        s = A.fixture_store(fixtures[name])
        N = s.ntx
        for T in range(1, N + 1):
            for S in sorted({0, 1, max(T - 1, 1), T, min(T + 1, N), N, (T * 5) % N + 1}):
                st, raw = s.expect(A.ANS_TX, T, S)
                assert st == 0, (name, T, S)
                got = VT.reference(raw, VT.TX_BY_ID, [], T, S, s.state_alh(S))
                want_tx = max(T, S)
                assert got[:4] == (0, True, want_tx, s.alhs[want_tx - 1]), (name, T, S)


def test_go_store_entry_answers_pass_the_client(orc, fixtures):
    """The ENTRY answers of the Go-written stores through the restated
    verifiedGet.  The client hashes EncodeKey(key) = 0x00 || key and 0x00 ||
    value, so only entries the database layer wrote as plain key-values (stored
    key and stored value both led by 0x00) can be asked through VerifiableGet;
    the embedded-store keys of long_linear_proof and the SQL catalog keys (0x02)
    cannot, and their expectations are held by the byte comparison with the
    golden DualProofs and the TX answers above."""
    import verifiable_entry_util as VE
    Entry = VE.messages()["Entry"]
    n = 0
    for name in STORES:
        fx = fixtures[name]
        s = A.fixture_store(fx)
        N = s.ntx
        for T in range(1, N + 1):
            for j, (md, key, _, hv) in enumerate(s.txs[T - 1].entries):
                value = bytes.fromhex(fx["txs"][T - 1]["entries"][j]["value"])
                if key[:1] != b"\x00" or value[:1] != b"\x00" or orc.sha256(value) != hv:
                    continue
                E = Entry()
                E.tx, E.key, E.value = T, key[1:], value[1:]
                if md:
                    A._fill_kvmd(E.metadata, md)
                for S in sorted({0, 1, max(T - 1, 1), T, min(T + 1, N), N}):
                    st, raw = s.expect(A.ANS_ENTRY, T, S, key, E.SerializeToString(deterministic=True))
                    assert st == 0, (name, T, j, S)
                    want_tx = max(T, S)
                    got = VE.reference(raw, key[1:], 0, S, s.state_alh(S))
                    assert got[:4] == (0, True, want_tx, s.alhs[want_tx - 1]), (name, T, j, S)
                    n += 1
    assert n >= 2  # v110_systemdb holds the plain key-value the Go stores have


def test_synthetic_answers_pass_the_client(orc):
    import verifiable_entry_util as VE
    import verifiable_tx_util as VT
    s = A.synthetic()
    reqs = A.synthetic_requests(s)
    assert 550 <= len(reqs) <= 900
    seen = set()
    for kind, T, S, key, entry in reqs:
        if (kind, T, S, key) in seen:
            continue
        seen.add((kind, T, S, key))
        st, raw = s.expect(kind, T, S, key, entry)
        assert st == 0, (kind, T, S)
        want_tx = max(T, S)
        if kind == A.ANS_TX:
            got = VT.reference(raw, VT.TX_BY_ID, [], T, S, s.state_alh(S))
        elif entry:
            got = VE.reference(raw, key[1:], 0, S, s.state_alh(S))
        else:
            continue  # (no Entry to check the value against: the client refuses a nil entry)
        assert got[:4] == (0, True, want_tx, s.alhs[want_tx - 1]), (kind, T, S)


def test_synthetic_store_holds_what_it_promises(orc):
    from verifiable_entry_util import messages
    s = A.synthetic()
    assert s.ntx == A.N_TX == 60
    assert {t.width for t in s.txs} == set(A.WIDTHS)
    assert {int(v) for v in s.recs["version"]} == {0, 1}
    assert any(int(r["md_len"]) for r in s.recs) and not all(int(r["md_len"]) for r in s.recs)
    lag = {int(r["id"]) - 1 - int(r["bl_tx_id"]) for r in s.recs[1:]}
    assert lag == {0, 1, 2, 3}
    ents = [e for t in s.txs for e in t.entries]
    klens = {len(e[1]) for e in ents}
    assert min(klens) == 1 and max(klens) == 1024
    assert {e[2] for e in ents} == set(A.VLENS)
    flags = {A.md_flags(e[0]) for e in ents if e[0]}
    assert {(d, e is not None, n) for d, e, n in flags} | {(False, False, False)} == \
        {(d, e, n) for d in (False, True) for e in (False, True) for n in (False, True)}
    assert {e for _, e, _ in flags if e is not None} == set(A.EXPIRES)
    Tx = messages()["Tx"]
    for T, want in A.TX_BODY_TUNED.items():
        assert len(s.tx_proto(T)) == want
    for (T, j), want in A.ENTRY_BODY_TUNED.items():
        assert Tx.FromString(s.tx_proto(T)).entries[j].ByteSize() == want
    dup = s.txs[A.DUP_TX - 1].entries
    assert dup[A.DUP_FIRST][1] == dup[A.DUP_SECOND][1] and \
        s.index_of(A.DUP_TX, dup[A.DUP_SECOND][1]) == A.DUP_FIRST


def _call(L, t, store, batch, out_cap=0, off=True, status=True):
    n = batch.n
    o = np.zeros(n + 1, np.uint64)
    st = np.zeros(max(n, 1), np.int32)
    return L.mh_verifiable_answer_pb_batch(t, C.addressof(store) if store is not None else None,
                                           C.addressof(batch) if batch is not None else None, None,
                                           out_cap, o.ctypes.data if off else None,
                                           st.ctypes.data if status else None)


def test_argument_checks_need_no_device():
    """every refusal below is decided before the tree is touched: the handle is
    never dereferenced"""
    from immustore_amd import _native as N
    from immustore_amd.answers import _Batch, _Store
    L = N.load()
    ILLEGAL = N.MH_ERR_ILLEGAL_ARGUMENTS
    t = C.c_void_p(0x1000)  # a non-null handle that no check may follow
    n = 3
    kind = np.zeros(n, np.uint8)
    tx = np.ones(n, np.uint64)
    ps = np.zeros(n, np.uint64)
    ko = np.zeros(n + 1, np.uint64)
    eo = np.zeros(n + 1, np.uint64)
    keys = np.zeros(8, np.uint8)

    def batch(**kw):
        b = _Batch()
        b.n, b.kind, b.tx, b.prove_since = n, kind.ctypes.data, tx.ctypes.data, ps.ctypes.data
        b.keys, b.key_off, b.entries, b.entry_off = keys.ctypes.data, ko.ctypes.data, None, \
            eo.ctypes.data
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def store(es=12):
        s = _Store()
        s.txlog, s.txlog_len, s.clog, s.ntx = 0x2000, 100, 0x3000, 1
        s.clog_entry_size, s.max_entries, s.max_key_len = es, 1024, 1024
        return s

    assert _call(L, None, store(), batch()) == ILLEGAL
    assert _call(L, t, None, batch()) == ILLEGAL
    assert L.mh_verifiable_answer_pb_batch(t, C.addressof(store()), None, None, 0, None, None) == ILLEGAL
    assert _call(L, t, store(), batch(), off=False) == ILLEGAL
    assert _call(L, t, store(), batch(), status=False) == ILLEGAL
    assert _call(L, t, store(), batch(), out_cap=10) == ILLEGAL  # a capacity without a buffer
    for f in ("kind", "tx", "prove_since", "key_off", "entry_off"):
        assert _call(L, t, store(), batch(**{f: None})) == ILLEGAL, f
    for es in (0, 11, 13, 43, 45):
        assert _call(L, t, store(es), batch()) == ILLEGAL, es
    assert _call(L, t, store(), batch(n=1 << 31)) == ILLEGAL
    # offsets running backwards
    bad = np.array([0, 2, 1, 2], np.uint64)
    kind[:] = 1
    assert _call(L, t, store(), batch(key_off=bad.ctypes.data)) == ILLEGAL
    assert _call(L, t, store(), batch(entry_off=bad.ctypes.data)) == ILLEGAL
    # key / entry bytes without a buffer
    up = np.array([0, 1, 2, 3], np.uint64)
    assert _call(L, t, store(), batch(key_off=up.ctypes.data, keys=None)) == ILLEGAL
    assert _call(L, t, store(), batch(entry_off=up.ctypes.data)) == ILLEGAL
    # a kind outside the enum; a TX request that owns key bytes
    kind[:] = (0, 2, 1)
    assert _call(L, t, store(), batch()) == ILLEGAL
    kind[:] = (1, 0, 1)
    assert _call(L, t, store(), batch(key_off=up.ctypes.data)) == ILLEGAL
    # a store without its logs
    kind[:] = 0
    s = store()
    s.txlog = None
    assert _call(L, t, s, batch()) == ILLEGAL
    s = store()
    s.clog = None
    assert _call(L, t, s, batch()) == ILLEGAL
    # n == 0 is MH_OK and touches nothing
    o = np.full(1, 7, np.uint64)
    b0 = batch(n=0)
    assert L.mh_verifiable_answer_pb_batch(t, C.addressof(store()), C.addressof(b0), None, 0,
                                           o.ctypes.data, None) == 0 and o[0] == 0
