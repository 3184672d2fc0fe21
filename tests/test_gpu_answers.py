"""mh_verifiable_answer_pb_batch: whole VerifiableTx / VerifiableEntry answers
generated on the device from a resident store, against the Go-shaped messages
of answer_util (byte for byte, with off and status), and fed back to the
device's own verifiers."""
import ctypes as C
import struct

import numpy as np
import pytest

import answer_util as A

pytestmark = pytest.mark.gpu

STORES = ("long_linear_proof", "v110_defaultdb", "v110_systemdb")


@pytest.fixture(scope="module")
def m():
    import torch  # noqa: F401  (first: the library binds the HIP runtime torch loaded)
    import immustore_amd as m
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def resident(ctx, s, alhs=None):
    """s on the device: the logs, and the ahtree over alhs (default: s's own)"""
    import immustore_amd as m
    t = m.AHtree(ctx)
    a = alhs if alhs is not None else s.alhs
    if a:
        t.append_batch(np.frombuffer(b"".join(a), np.uint8).reshape(-1, 32))
    return m.ResidentStore(t, s.raw, s.clog, s.es)


def release(d):
    """the device logs and the tree, while their context is still there"""
    d.close()
    d.tree.close()


@pytest.fixture(scope="module")
def syn(ctx):
    s = A.synthetic()
    d = resident(ctx, s)
    yield s, d
    release(d)


def run(d, reqs, **kw):
    import immustore_amd as m
    return m.verifiable_answers(d, *A.columns(reqs), **kw)


def expected(s, reqs):
    exp = [s.expect(*r) for r in reqs]
    off = np.zeros(len(reqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for _, b in exp], dtype=np.uint64)
    return exp, off


def check(s, reqs, got, exp=None):
    msgs, st, off = got
    exp, eoff = exp or expected(s, reqs)
    assert [int(x) for x in st] == [e[0] for e in exp], \
        [(r[:3], int(x), e[0]) for r, x, e in zip(reqs, st, exp) if int(x) != e[0]][:5]
    for p, (r, m_, e) in enumerate(zip(reqs, msgs, exp)):
        assert m_ == e[1], (p, r[:3], len(m_), len(e[1]))
    assert np.array_equal(off, eoff)
    return exp


def _entry_for(T, key):
    from verifiable_entry_util import messages
    E = messages()["Entry"]()
    E.tx, E.key = T, key
    return E.SerializeToString(deterministic=True)


@pytest.mark.parametrize("es", (12, 44))
@pytest.mark.parametrize("name", STORES)
def test_go_written_stores(ctx, fixtures, name, es):
    s = A.fixture_store(fixtures[name], es)
    N = s.ntx
    reqs = [(A.ANS_TX, T, S, b"", b"") for T in range(1, N + 1) for S in range(0, N + 1)]
    for T in range(1, N + 1):
        for j, e in enumerate(s.txs[T - 1].entries):
            for S in sorted({0, 1, T - 1, T, T + 1, N}):
                reqs.append((A.ANS_ENTRY, T, S, e[1], _entry_for(T, e[1]) if (T + j) % 2 else b""))
    d = resident(ctx, s)
    try:
        exp = check(s, reqs, run(d, reqs))
    finally:
        release(d)
    assert sum(1 for e in exp if e[0] == 0) >= len(reqs) - N * 8  # (S = N + 1 is ErrIllegalState)


def _pinned(keep):
    from immustore_amd import _native as N
    L = N.load()

    def place(a):
        p = C.c_void_p()
        N.check(L.mh_host_alloc_pinned(max(a.nbytes, 1), C.byref(p)))
        keep.append(p)
        v = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(a.nbytes, 1),))
        v = v[:a.nbytes].view(a.dtype)
        v[:] = a
        return v
    return place


def test_synthetic_store(syn):
    from immustore_amd import _native as N
    s, d = syn
    reqs = A.synthetic_requests(s)
    assert 550 <= len(reqs) <= 900
    exp = expected(s, reqs)
    assert all(e[0] == 0 for e in exp[0])
    check(s, reqs, run(d, reqs), exp)
    keep = []
    try:
        check(s, reqs, run(d, reqs, arrays=_pinned(keep)), exp)  # request arrays in pinned memory
    finally:
        for p in keep:
            N.load().mh_host_free_pinned(p)
    for r in (reqs[0], reqs[8], reqs[-1]):  # n = 1, both kinds
        check(s, [r], run(d, [r]))
    msgs, st, off = run(d, [])  # n = 0
    assert msgs == [] and len(st) == 0 and int(off[0]) == 0


def test_round_trip(ctx, syn):
    """the device's answers through the device's verifiers"""
    from immustore_amd import txlayer
    s, d = syn
    reqs = [r for r in A.synthetic_requests(s) if r[0] == A.ANS_TX or r[4]]
    msgs, st, _ = run(d, reqs)
    assert not st.any()
    tx = [(m_, r) for m_, r in zip(msgs, reqs) if r[0] == A.ANS_TX]
    en = [(m_, r) for m_, r in zip(msgs, reqs) if r[0] == A.ANS_ENTRY]
    assert len(tx) > 300 and len(en) > 150
    got = txlayer.verify_verifiable_tx_pb_batch(
        [m_ for m_, _ in tx], [txlayer.VTX_TX_BY_ID] * len(tx), [[]] * len(tx),
        [r[1] for _, r in tx], [r[2] for _, r in tx], [s.state_alh(r[2]) for _, r in tx], ctx=ctx)
    for (st1, ok, ntx, nalh), (_, r) in zip(zip(*got[:4]), tx):
        want = max(r[1], r[2])
        assert (int(st1), bool(ok), int(ntx), bytes(nalh)) == (0, True, want, s.alhs[want - 1]), r[:3]
    got = txlayer.verify_verifiable_entry_pb_batch(
        [m_ for m_, _ in en], [r[3][1:] for _, r in en], [0] * len(en), [r[2] for _, r in en],
        [s.state_alh(r[2]) for _, r in en], ctx=ctx)
    for (st1, ok, ntx, nalh), (_, r) in zip(zip(*got), en):
        want = max(r[1], r[2])
        assert (int(st1), bool(ok), int(ntx), bytes(nalh)) == (0, True, want, s.alhs[want - 1]), r[:3]


@pytest.mark.parametrize("w", A.WIDTHS)
def test_inclusion_paths(syn, w):
    s, d = syn
    reqs = []
    for T in range(1, s.ntx + 1):
        if s.txs[T - 1].width != w:
            continue
        for j in A.asked_leaves(w):
            key = s.txs[T - 1].entries[j][1]
            if s.index_of(T, key) == j:
                reqs.append((A.ANS_ENTRY, T, (T + j) % (s.ntx + 1), key, s.entry_msg(T, j)))
    assert len(reqs) >= 2 * len(A.asked_leaves(w)) - 1
    exp = check(s, reqs, run(d, reqs))
    from verifiable_entry_util import messages
    leaves = {messages()["VerifiableEntry"].FromString(e[1]).inclusionProof.leaf for e in exp}
    assert leaves == set(A.asked_leaves(w)) - ({A.DUP_SECOND} if w == 64 else set())


# ------------------------------------------------------------------ the status table
def _broad(s):
    """requests over the whole store, both kinds and both directions"""
    N = s.ntx
    reqs = []
    for T in range(1, N + 1):
        for S in (0, max(T - 3, 1), T, min(T + 5, N), 20, 23):
            reqs.append((A.ANS_TX, T, S, b"", b""))
        reqs.append((A.ANS_ENTRY, T, (T * 3) % N + 1, s.txs[T - 1].entries[-1][1], b"\x08\x01"))
    return reqs


def _hval_pos(s, X, j=0):
    """offset in the log of entry j's hVal in tx X"""
    p = struct.unpack_from(">Q", s.clog, (X - 1) * s.es)[0]
    r = s.recs[X - 1]
    q = p + (96 + int(r["md_len"]) if int(r["version"]) else 92)
    for i in range(j + 1):
        m_, = struct.unpack_from(">H", s.raw, q)
        k_, = struct.unpack_from(">H", s.raw, q + 2 + m_)
        if i == j:
            return q + 4 + m_ + k_ + 12
        q += 48 + m_ + k_


def _mutated(ctx, s, raw=None, clog=None):
    m = A.AnsStore(raw if raw is not None else s.raw, clog if clog is not None else s.clog, s.es,
                   aht=s.aht)
    m.values = s.values
    return m, resident(ctx, m, alhs=s.alhs)


# (tx whose hVal is flipped, the probing request (T, S), why it reads that tx)
FLIPS = [(30, (30, 10), "T"), (10, (30, 10), "S"), (23, (25, 25), "tgt.BlTxID"),
         (25, (27, 20), "a mid-range tx of the linear proof [23, 27]"),
         (22, (40, 23), "a mid-range tx of the advance proof [20, 23]")]


@pytest.mark.parametrize("X,probe,why", FLIPS, ids=[f[2].split()[0] + str(f[0]) for f in FLIPS])
def test_flipped_hval(ctx, syn, X, probe, why):
    s, _ = syn
    raw = bytearray(s.raw)
    raw[_hval_pos(s, X) + 5] ^= 0x10
    m, d = _mutated(ctx, s, raw=bytes(raw))
    try:
        assert [k + 1 for k, v in enumerate(m.rst) if v] == [X] and m.rst[X - 1] == A.CORRUPTED_DATA
        T, S = probe
        if why not in ("T", "S"):  # the proof reads X, the request's own txs are sound
            src, tgt = (S, T) if S <= T else (T, S)
            bl, sbl = int(m.recs[tgt - 1]["bl_tx_id"]), int(m.recs[src - 1]["bl_tx_id"])
            assert X not in (T, S)
            if why.startswith("tgt"):
                assert X == bl
            elif "linear" in why:
                assert max(src, bl) < X < tgt
            else:
                assert sbl + 1 < X < min(src, bl)
        reqs = [(A.ANS_TX, T, S, b"", b"")] + _broad(m)
        exp = check(m, reqs, run(d, reqs))
        assert exp[0][0] == A.CORRUPTED_DATA
        # every request that does not read X answers as the sound store does
        same = [r for r, e in zip(reqs, exp) if e[0] == 0]
        assert len(same) > len(reqs) // 2
        assert [m.expect(*r) for r in same] == [s.expect(*r) for r in same]
    finally:
        release(d)


def test_resealed_prev_alh(ctx, syn, orc):
    """tx X with another PrevAlh and its Alh sealed over it: a sound record, a
    broken chain -- ErrCorruptedTxData for the proofs whose ranges cross it"""
    s, _ = syn
    X = 25
    p, size = struct.unpack_from(">QI", s.clog, (X - 1) * s.es)
    raw = bytearray(s.raw)
    prev = bytes(range(32))
    raw[p + 56:p + 88] = prev
    raw[p + size - 32:p + size] = orc.tx_alh(X, prev, s.inners[X - 1])
    m, d = _mutated(ctx, s, raw=bytes(raw))
    try:
        assert not any(m.rst) and m.alhs[X - 1] != s.alhs[X - 1]
        reqs = [(A.ANS_TX, 27, 20, b"", b""), (A.ANS_TX, 25, 25, b"", b""),
                (A.ANS_TX, 24, 20, b"", b"")] + _broad(m)
        exp = check(m, reqs, run(d, reqs))
        assert [e[0] for e in exp[:3]] == [A.CORRUPTED_TX_DATA, 0, 0]  # [23, 27] crosses it
        bad = {r[1:3] for r, e in zip(reqs, exp) if e[0]}
        assert all(e[0] in (0, A.CORRUPTED_TX_DATA) for e in exp) and len(bad) >= 3
    finally:
        release(d)


def test_clog_entry_past_the_log(ctx, syn):
    s, _ = syn
    X = 31
    clog = bytearray(s.clog)
    struct.pack_into(">Q", clog, (X - 1) * s.es, len(s.raw) + 1000)
    m, d = _mutated(ctx, s, clog=bytes(clog))
    try:
        assert m.rst[X - 1] == A.TRUNCATED and sum(1 for v in m.rst if v) == 1
        reqs = [(A.ANS_TX, X, 0, b"", b""), (A.ANS_TX, 40, X, b"", b"")] + _broad(m)
        exp = check(m, reqs, run(d, reqs))
        assert exp[0][0] == exp[1][0] == A.TRUNCATED
    finally:
        release(d)


def test_status_rows(syn):
    s, d = syn
    N = s.ntx
    e2 = s.txs[1].entries
    long_key = s.txs[6].entries[5][1]
    dup_key = s.txs[A.DUP_TX - 1].entries[A.DUP_SECOND][1]
    rows = [((A.ANS_TX, 5, N + 1, b"", b""), A.ILLEGAL_STATE),
            ((A.ANS_TX, 0, N + 1, b"", b""), A.ILLEGAL_STATE),       # S > N is asked first
            ((A.ANS_TX, 0, 3, b"", b""), A.ILLEGAL_ARGUMENTS),
            ((A.ANS_TX, N + 1, 3, b"", b""), A.TX_NOT_FOUND),
            ((A.ANS_ENTRY, N + 7, 0, b"k", b""), A.TX_NOT_FOUND),
            ((A.ANS_ENTRY, 7, 3, b"\x00no such key", b""), A.KEY_NOT_FOUND),
            ((A.ANS_ENTRY, 7, 3, b"", b""), A.KEY_NOT_FOUND),
            ((A.ANS_ENTRY, 2, 1, b"\x00", b""), A.KEY_NOT_FOUND),     # a proper prefix of both keys
            ((A.ANS_ENTRY, 7, 9, long_key[:-1], b""), A.KEY_NOT_FOUND),
            ((A.ANS_ENTRY, 7, 9, long_key + b"\x00", b""), A.KEY_NOT_FOUND),
            ((A.ANS_ENTRY, 2, 1, e2[0][1], b""), A.OK),              # "\0a" itself: leaf 0
            ((A.ANS_ENTRY, 2, 1, e2[1][1], b""), A.OK),
            ((A.ANS_ENTRY, A.DUP_TX, 9, dup_key, b""), A.OK),        # the first occurrence wins
            ((A.ANS_TX, 9, 9, b"", b""), A.OK)]
    assert len(long_key) == 1024
    reqs = [r for r, _ in rows]
    exp = check(s, reqs, run(d, reqs))
    assert [e[0] for e in exp] == [w for _, w in rows]
    from verifiable_entry_util import messages
    assert messages()["VerifiableEntry"].FromString(exp[12][1]).inclusionProof.leaf == A.DUP_FIRST


def test_out_cap_one_byte_short(syn):
    s, d = syn
    reqs = A.synthetic_requests(s)[:40] + [(A.ANS_TX, 0, 0, b"", b"")] + A.synthetic_requests(s)[40:60]
    exp, off = expected(s, reqs)
    for k in (0, 7, 40, 41, len(reqs) - 1):
        cap = int(off[k + 1]) - 1
        msgs, st, goff = run(d, reqs, out_cap=cap)
        assert np.array_equal(goff, off)  # complete: off[n] sizes the retry
        for p, e in enumerate(exp):
            fits = int(off[p + 1]) <= cap
            want = e[0] if e[0] or fits else A.BUFFER_TOO_SMALL
            assert int(st[p]) == want, (k, p)
            assert msgs[p] == (e[1] if want == 0 else b""), (k, p)
    msgs, st, goff = run(d, reqs, out_cap=int(off[-1]))
    assert msgs == [e[1] for e in exp]


def test_distinct_reads(syn):
    """256 requests over three (T, S) pairs: the same bytes as the three alone"""
    s, d = syn
    three = [(A.ANS_TX, 44, 17, b"", b""), (A.ANS_ENTRY, 39, 52, s.txs[38].entries[999][1], b"\x08\x27"),
             (A.ANS_TX, 12, 0, b"", b"")]
    alone = run(d, three)
    check(s, three, alone)
    reqs = [three[i % 3] for i in range(256)]
    msgs, st, off = run(d, reqs)
    assert not st.any()
    assert msgs == [alone[0][i % 3] for i in range(256)]
    assert int(off[-1]) == sum(len(x) for x in msgs)


def test_size_hint_skips_the_sizing_pass(syn):
    s, d = syn
    reqs = A.synthetic_requests(s)[:50]
    exp, off = expected(s, reqs)
    for hint in (int(off[-1]), int(off[-1]) + 1000, int(off[-1]) - 1, 10):
        check(s, reqs, run(d, reqs, size_hint=hint), (exp, off))


def test_two_trees_of_one_context_answer_from_two_threads(ctx, syn, fixtures):
    """the call's scratch is the context's: two trees of one context answering
    at once must give what each gives alone"""
    import threading
    s, d = syn
    f = A.fixture_store(fixtures["long_linear_proof"])
    fd = resident(ctx, f)
    try:
        jobs = [(s, d, A.synthetic_requests(s)[:200]),
                (f, fd, [(A.ANS_TX, T, S, b"", b"") for T in range(1, f.ntx + 1) for S in (0, 3, 30)])]
        want = [expected(x, r) for x, _, r in jobs]
        errs = []

        def work(k):
            x, dev, reqs = jobs[k]
            try:
                for _ in range(6):
                    check(x, reqs, run(dev, reqs), want[k])
            except BaseException as e:  # noqa: B036 (reported by the main thread)
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
    finally:
        release(fd)
