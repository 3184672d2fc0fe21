"""mh_tx_answer_pb_batch on the device -- db.TxByID / db.TxScan /
db.VerifiableTxByID under an EntriesSpec -- against the CPU restatement of
tests/tx_spec_util.py: off, status and the messages byte for byte, out in host
and device memory, and the VerifiableTx answers fed back to the device's own
verifier.  The export call, whose value stores moved into a shared header, is
checked against its oracle in both MH_EXPORT_ARM arms."""
import ctypes as C
import os

import numpy as np
import pytest

import export_util as X
import tx_spec_util as U

pytestmark = pytest.mark.gpu
CANARY = 0xA5
PAD = 64


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


def on_device(m, ctx, st):
    return m.ExportStore(st.raw, st.clog, [(f, b) for f, b in st.vlogs], st.es, ctx=ctx,
                         max_entries=st.max_entries)


@pytest.fixture(scope="module")
def syn(m, ctx, orc):
    """the synthetic store, its device copy, the ahtree over its Alh values"""
    S = U.synthetic()
    s = S.store
    dev = on_device(m, ctx, s.exp)
    tree = m.AHtree(ctx)
    tree.append_batch(np.frombuffer(b"".join(s.ans.alhs), np.uint8).reshape(-1, 32))
    yield S, s, dev, tree
    dev.close()
    tree.close()


def parity_requests(s):
    """every tx x both kinds x the action triples (and a nil EntriesSpec), the
    VERIFIABLE ones with prove_since in {0, tx - 1, tx, tx + 1, ntx}; then the
    requests that fail ahead of the record"""
    N = s.ntx
    reqs = []
    for T in range(1, N + 1):
        for sp in U.triples() + [None]:
            reqs.append((U.TXA_TX, T, 7, sp))  # (prove_since of a TX request is ignored)
            for S in sorted({0, T - 1, T, min(T + 1, N), N}):
                reqs.append((U.TXA_VERIFIABLE, T, S, sp))
    for sp in (None, U.ALL_RAW):
        reqs += [(U.TXA_TX, 0, 0, sp), (U.TXA_TX, N + 1, 0, sp), (U.TXA_TX, 1, N + 1, sp),
                 (U.TXA_VERIFIABLE, 0, 0, sp), (U.TXA_VERIFIABLE, N + 1, 0, sp),
                 (U.TXA_VERIFIABLE, 1, N + 1, sp), (U.TXA_VERIFIABLE, 0, N + 1, sp)]
    return reqs


@pytest.fixture(scope="module")
def parity(syn):
    """the case list and its expectation, computed once and left unchanged"""
    _, s, _, _ = syn
    reqs = parity_requests(s)
    return reqs, U.expect(s, reqs)


class Out:
    """cap bytes of out between two canary pads, in host or device memory"""

    def __init__(self, m, ctx, mode, cap):
        from immustore_amd import _native as N
        self.L, self.ctx, self.mode, self.cap = N.load(), ctx, mode, cap
        self.size = PAD + cap + PAD
        self.host = np.full(self.size, CANARY, np.uint8)
        self.p = C.c_void_p()
        if mode == "device":
            N.check(self.L.mh_dev_alloc(ctx.handle, self.size, C.byref(self.p)))
            N.check(self.L.mh_memcpy_h2d(ctx.handle, self.p.value, self.host.ctypes.data, self.size))
            ctx.synchronize()
            self.addr = self.p.value + PAD
        else:
            self.addr = self.host.ctypes.data + PAD

    def fetch(self):
        from immustore_amd import _native as N
        if self.mode == "device":
            N.check(self.L.mh_memcpy_d2h(self.ctx.handle, self.host.ctypes.data, self.p.value, self.size))
            self.ctx.synchronize()
            N.check(self.L.mh_dev_free(self.ctx.handle, self.p.value))
        pads = bool((self.host[:PAD] == CANARY).all() and (self.host[PAD + self.cap:] == CANARY).all())
        return self.host[PAD:PAD + self.cap], pads


def call(m, ctx, dev, tree, reqs, cap, mode="host", now=U.NOW):
    """one call into cap bytes -> (off, status, out bytes); asserts the pads"""
    o = Out(m, ctx, mode, cap)
    off, st = m.answers.tx_answers_raw(dev, tree, *U.columns(reqs), now, o.addr, cap)
    buf, pads = o.fetch()
    assert pads, "bytes outside out were written"
    return off, st, buf


def same(reqs, res, exp, what=""):
    """off, status, every MH_OK message; every byte of out that no written
    answer and no answer failing on a digest alone owns still holds the canary"""
    off, st, buf = res
    est, eoff, emsgs = exp
    bad = [(r, int(x), int(e)) for r, x, e in zip(reqs, st, est) if int(x) != int(e)]
    assert not bad, (what, len(bad), bad[:6])
    assert off.tolist() == eoff.tolist(), what
    owned = np.zeros(len(buf), bool)
    for p, msg in enumerate(emsgs):
        lo, hi = int(off[p]), int(off[p + 1])
        if st[p] == U.OK:
            assert bytes(buf[lo:hi]) == msg, (what, p, reqs[p], hi - lo)
            owned[lo:hi] = True
        elif st[p] == U.CORRUPTED_DATA:
            owned[lo:min(hi, len(buf))] = True  # contents unspecified
    assert (buf[~owned] == CANARY).all(), what


# ------------------------------------------------------------------ parity
def test_case_list_covers_the_contract(syn, parity):
    S, s, _, _ = syn
    reqs, (st, off, msgs) = parity
    tx = {int(x) for r, x in zip(reqs, st) if r[0] == U.TXA_TX}
    ver = {int(x) for r, x in zip(reqs, st) if r[0] == U.TXA_VERIFIABLE}
    # TX: T == 0, T > ntx, the record verdict, serializeTx's statuses, MH_OK
    assert {U.ILLEGAL_ARGUMENTS, U.TX_NOT_FOUND, U.CORRUPTED_DATA, U.ILLEGAL_STATE, U.EOF, U.OK} <= tx
    assert {U.ILLEGAL_STATE, U.ILLEGAL_ARGUMENTS, U.TX_NOT_FOUND, U.CORRUPTED_DATA, U.EOF, U.OK} <= ver
    by = lambda kind, T, want: any(r[0] == kind and r[1] == T and int(x) == want  # noqa: E731
                                   for r, x in zip(reqs, st))
    for kind in (U.TXA_TX, U.TXA_VERIFIABLE):
        assert by(kind, S.corrupt, U.CORRUPTED_DATA)                       # the record verdict
        assert by(kind, S.roles["flip_behind_sql"], U.ILLEGAL_ARGUMENTS)   # SQL RESOLVE
        assert by(kind, S.roles["flip_ahead_of_sql"], U.CORRUPTED_DATA)    # a digest ahead of it
        assert by(kind, S.roles["empty_key"], U.ILLEGAL_STATE)
        assert by(kind, S.roles["no_such_vlog"], U.ILLEGAL_STATE)
        assert by(kind, S.roles["id_zero"], U.EOF)
    # a DualProof status ahead of the serialization: the tx behind the corrupt record
    # as the target (the proof then reads the record its BlTxID names)
    assert all(int(x) == U.CORRUPTED_DATA for r, x in zip(reqs, st)
               if r[0] == U.TXA_VERIFIABLE and r[1] == S.corrupt + 1 and r[2] <= r[1])
    assert by(U.TXA_TX, S.corrupt + 1, U.OK)
    # (MH_ERR_BUFFER_TOO_SMALL: test_sizing)
    with_value = 0
    M = U.messages()
    for r, x, msg in zip(reqs, st, msgs):
        if int(x) == U.OK and r[3] is not None:
            t = M["Tx"].FromString(msg) if r[0] == U.TXA_TX else M["VerifiableTx"].FromString(msg).tx
            with_value += any(len(e.value) for e in t.entries)
    assert 3 * with_value >= len(reqs), (with_value, len(reqs))
    for T, want in S.tx_tuned.items():
        assert len(U.serialize_tx(s, T, U.ALL_RAW)[1]) == want
    bodies = {e.ByteSize() for e in M["Tx"].FromString(
        U.serialize_tx(s, S.entry_tuned, U.ALL_RAW)[1]).entries}
    assert set(U.ENTRY_BODIES) <= bodies


def test_parity(m, ctx, syn, parity):
    _, s, dev, tree = syn
    reqs, exp = parity
    res = call(m, ctx, dev, tree, reqs, int(exp[1][-1]))
    same(reqs, res, exp)
    # every destination alignment of a multi-block value is met
    off, st, buf = res
    align = set()
    for p, r in enumerate(reqs):
        if st[p] != U.OK or r[3] != U.ALL_RAW or r[0] != U.TXA_TX:
            continue
        msg = exp[2][p]
        for md, key, vlen, voff, hv in s.entries(r[1]):
            cls, val = s.exp.value_class(vlen, voff)
            if val and len(val) >= 200 and msg.count(val) == 1:
                align.add((int(off[p]) + msg.index(val)) & 3)
    assert align == {0, 1, 2, 3}


def test_tx_requests_without_a_tree(m, ctx, syn, parity):
    _, s, dev, _ = syn
    reqs = [r for r in parity[0] if r[0] == U.TXA_TX]
    exp = U.expect(s, reqs)
    same(reqs, call(m, ctx, dev, None, reqs, int(exp[1][-1])), exp)
    one = [reqs[5]]
    exp1 = U.expect(s, one)
    same(one, call(m, ctx, dev, None, one, int(exp1[1][-1])), exp1)  # n = 1
    off, st = m.answers.tx_answers_raw(dev, None, [], [], [], [], U.NOW, 0, 0)  # n = 0
    assert len(st) == 0 and int(off[0]) == 0


def test_expiry_follows_now(m, ctx, syn):
    _, s, dev, _ = syn
    T = U.synthetic().roles["expirations"]
    for now in (U.NOW - 2, U.NOW - 1, U.NOW, U.NOW + 1, U.NOW + 200, -10):
        reqs = [(U.TXA_TX, T, 0, U.ALL_RAW)]
        exp = U.expect(s, reqs, now=now)
        same(reqs, call(m, ctx, dev, None, reqs, int(exp[1][-1]), now=now), exp, now)


# ------------------------------------------------------------------ the existing call
def test_nil_spec_is_the_verifiable_answer_call(m, ctx, syn):
    """has_spec = 0, VERIFIABLE: byte-equal to mh_verifiable_answer_pb_batch"""
    _, s, dev, tree = syn
    N = s.ntx
    pairs = [(T, S) for T in range(0, N + 2) for S in sorted({0, 1, max(T - 1, 0), T, min(T + 1, N), N, N + 1})]
    reqs = [(U.TXA_VERIFIABLE, T, S, None) for T, S in pairs]
    res = m.ResidentStore(tree, s.exp.raw, s.exp.clog, s.exp.es, max_entries=s.exp.max_entries)
    try:
        msgs0, st0, off0 = m.verifiable_answers(res, [m.answers.MH_ANS_TX] * len(pairs),
                                                [p[0] for p in pairs], [p[1] for p in pairs])
    finally:
        res.close()
    msgs, st, off = m.tx_answers(dev, tree, *U.columns(reqs), U.NOW)
    assert st.tolist() == st0.tolist()
    assert off.tolist() == off0.tolist()
    assert msgs == msgs0
    assert sum(1 for x in st if x == 0) > len(pairs) // 2


# ------------------------------------------------------------------ sizing, memory forms
def test_sizing(m, ctx, syn, parity):
    _, s, dev, tree = syn
    reqs, exp = parity
    reqs, exp = reqs[:700], U.expect(s, parity[0][:700])
    # out_cap = 0: the same off, nothing written, the statuses ahead of the size kept
    zero = U.expect(s, reqs, out_cap=0)
    assert zero[1].tolist() == exp[1].tolist() and U.CORRUPTED_DATA in zero[0] and U.OK not in zero[0]
    same(reqs, call(m, ctx, dev, tree, reqs, 0), zero, "sizing")
    # one byte short of the last MH_OK answer: that one alone does not fit
    last = max(p for p, e in enumerate(exp[0]) if int(e) == U.OK and exp[1][p + 1] > exp[1][p])
    cap = int(exp[1][last + 1]) - 1
    short = U.expect(s, reqs, out_cap=cap)
    assert [p for p, (x, e) in enumerate(zip(short[0], exp[0])) if int(x) != int(e)] == [last]
    same(reqs, call(m, ctx, dev, tree, reqs, cap), short, "short")
    # and in the middle: every answer that ends beyond the capacity, no other
    mid = U.expect(s, reqs, out_cap=int(exp[1][350]) + 1)
    assert (mid[0] == U.BUFFER_TOO_SMALL).sum() > 100
    same(reqs, call(m, ctx, dev, tree, reqs, int(exp[1][350]) + 1), mid, "mid")
    # more room than needed: the bytes behind the answers stay
    same(reqs, call(m, ctx, dev, tree, reqs, int(exp[1][-1]) + 1000), exp, "roomy")


def test_device_out_equals_host_out(m, ctx, syn, parity):
    _, s, dev, tree = syn
    reqs = parity[0][::3]
    exp = U.expect(s, reqs)
    host = call(m, ctx, dev, tree, reqs, int(exp[1][-1]))
    devo = call(m, ctx, dev, tree, reqs, int(exp[1][-1]), mode="device")
    same(reqs, devo, exp, "device")
    assert host[0].tolist() == devo[0].tolist() and host[1].tolist() == devo[1].tolist()
    ok = np.zeros(len(host[2]), bool)
    for p in range(len(reqs)):
        if host[1][p] == U.OK:
            ok[int(host[0][p]):int(host[0][p + 1])] = True
    assert (host[2][ok] == devo[2][ok]).all()
    cap = int(exp[1][len(reqs) // 2])
    same(reqs, call(m, ctx, dev, tree, reqs, cap, mode="device"), U.expect(s, reqs, out_cap=cap), "device, short")


# ------------------------------------------------------------------ shared txs
def test_one_tx_asked_once_and_fifty_times(m, ctx, syn):
    S, s, dev, tree = syn
    for T in (S.roles["width_65"], S.roles["align_1"], S.roles["flip_in_excluded"], S.roles["empty_value"]):
        specs = (U.triples() + [None]) * 3
        many = [((U.TXA_TX, T, 0, sp) if i % 2 else (U.TXA_VERIFIABLE, T, (0, T, s.ntx)[i % 3], sp))
                for i, sp in enumerate(specs[:50])]
        exp = U.expect(s, many)
        off, st, buf = call(m, ctx, dev, tree, many, int(exp[1][-1]))
        same(many, (off, st, buf), exp, T)
        for p, r in enumerate(many):  # and each alone
            e1 = U.expect(s, [r])
            o1, s1, b1 = call(m, ctx, dev, tree, [r], int(e1[1][-1]))
            same([r], (o1, s1, b1), e1, (T, p))
            if s1[0] == U.OK:
                assert bytes(b1) == bytes(buf[int(off[p]):int(off[p + 1])])


# ------------------------------------------------------------------ round trip
def test_round_trip(m, ctx, syn, parity):
    """every MH_OK VerifiableTx answer through the device's verifier"""
    from immustore_amd import txlayer
    _, s, dev, tree = syn
    reqs = [r for r in parity[0] if r[0] == U.TXA_VERIFIABLE]
    msgs, st, _ = m.tx_answers(dev, tree, *U.columns(reqs), U.NOW)
    ok = [(m_, r) for m_, r, x in zip(msgs, reqs, st) if x == U.OK]
    assert len(ok) > len(reqs) // 2
    got = txlayer.verify_verifiable_tx_pb_batch(
        [m_ for m_, _ in ok], [txlayer.VTX_TX_BY_ID] * len(ok), [[]] * len(ok), [r[1] for _, r in ok],
        [r[2] for _, r in ok], [s.ans.state_alh(r[2]) for _, r in ok], ctx=ctx)
    for (st1, good, ntx, nalh), (_, r) in zip(zip(*got[:4]), ok):
        want = max(r[1], r[2])
        assert (int(st1), bool(good), int(ntx), bytes(nalh)) == (0, True, want, s.ans.alhs[want - 1]), r


# ------------------------------------------------------------------ the refactored export call
@pytest.mark.parametrize("arm", ["A", "B"])
def test_export_still_equals_its_oracle(m, ctx, orc, arm):
    st = X.synthetic(orc).store
    ex = st.expect()
    dev = on_device(m, ctx, st)
    old = os.environ.get("MH_EXPORT_ARM")
    os.environ["MH_EXPORT_ARM"] = arm
    try:
        total = int(ex["off"][-1])
        out = np.full(total + 2 * PAD, CANARY, np.uint8)
        off, sts, tr = m.export.export_tx_batch_raw(dev, 1, st.ntx, out.ctypes.data + PAD, total)
    finally:
        if old is None:
            del os.environ["MH_EXPORT_ARM"]
        else:
            os.environ["MH_EXPORT_ARM"] = old
        dev.close()
    assert off.tolist() == ex["off"].tolist()
    assert sts.tolist() == ex["status"].tolist()
    assert tr.tolist() == ex["truncated"].tolist()
    assert (out[:PAD] == CANARY).all() and (out[PAD + total:] == CANARY).all()
    for k, blob in enumerate(ex["blobs"]):
        if sts[k] == X.OK:
            assert bytes(out[PAD + int(off[k]):PAD + int(off[k + 1])]) == blob, k


# ------------------------------------------------------------------ arguments
def test_argument_errors_on_the_device(m, ctx, syn):
    from immustore_amd import _native as N
    _, s, dev, tree = syn
    raw = m.answers.tx_answers_raw
    with pytest.raises(N.MerkleError):  # kv RESOLVE: the whole call
        raw(dev, tree, [U.TXA_TX], [1], [0], [(U.RESOLVE, None, None)], U.NOW, 0, 0)
    with pytest.raises(N.MerkleError):  # z RESOLVE
        raw(dev, tree, [U.TXA_TX, U.TXA_TX], [1, 2], [0, 0], [None, (None, U.RESOLVE, None)], U.NOW, 0, 0)
    with pytest.raises(N.MerkleError):  # VERIFIABLE without a tree
        raw(dev, None, [U.TXA_VERIFIABLE], [1], [0], [None], U.NOW, 0, 0)
    with pytest.raises(N.MerkleError):  # a kind outside the enum
        raw(dev, tree, [2], [1], [0], [None], U.NOW, 0, 0)
    with pytest.raises(N.MerkleError):  # an action outside the enum
        raw(dev, tree, [U.TXA_TX], [1], [0], [(4, None, None)], U.NOW, 0, 0)
    with pytest.raises(N.MerkleError):  # out NULL with a capacity
        raw(dev, tree, [U.TXA_TX], [1], [0], [None], U.NOW, 0, 16)
    other = m.Context(0)
    try:
        t2 = m.AHtree(other)
        with pytest.raises(N.MerkleError):  # a tree of another context
            raw(dev, t2, [U.TXA_VERIFIABLE], [1], [0], [None], U.NOW, 0, 0)
        t2.close()
    finally:
        other.close()
    # the store is still served
    reqs = [(U.TXA_VERIFIABLE, 2, 1, U.ALL_RAW)]
    exp = U.expect(s, reqs)
    same(reqs, call(m, ctx, dev, tree, reqs, int(exp[1][-1])), exp)
