"""DualProof (v1) generated and marshalled on the device
(mh_ahtree_dual_proof_pb_batch / mh_dev_dual_proof_pb_batch: ImmuStore.DualProof
with its LinearProof and LinearAdvanceProof, immustore.go:2394-2562, as the
schema.DualProof message) against the CPU restatement in dual_v1_gen_util.py
(checked against the Go stores by test_dual_v1_gen_cpu.py).  Bit-exact, and
every message decodes and verifies on the device."""
import ctypes as C

import numpy as np
import pytest

import dual_v1_gen_util as U
from gpu_util import DevBuf

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


def _tree(m, ctx, payloads):
    t = m.AHtree(ctx)
    t.append_batch(np.stack([np.frombuffer(bytes(p), np.uint8) for p in payloads]))
    return t


def _round_trip(ctx, msgs, S, T, SA, TA):
    """decode on the device, VerifyDualProof on the device -> ok[n]"""
    from immustore_amd import txlayer
    st, dec = txlayer.decode_dual_proof_pb(list(msgs), ctx=ctx)
    assert (st == 0).all()
    return txlayer.verify_decoded_dual_proof_batch(dec, S, T, SA, TA, ctx=ctx)


@pytest.fixture(scope="module")
def fixture_runs(m, ctx, orc, wire, fixtures):
    """every dual_v1 case of the three Go stores through the device:
    name -> (S, T, alhs, expected messages, messages, status)"""
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture, inner_hashes
    runs = {}
    for name, fx in fixtures.items():
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        inners = inner_hashes(orc, recs, blob)
        t = _tree(m, ctx, [bytes.fromhex(p) for p in fx["aht_payloads"]])
        S = [c["src"] for c in fx["dual_v1"]]
        T = [c["tgt"] for c in fx["dual_v1"]]
        want = [dual_v1_msg(wire, dual_v1_args(c, recs, blob, alhs)) for c in fx["dual_v1"]]
        msgs, st = t.dual_proof_pb_batch(recs[[a - 1 for a in S]], recs[[b - 1 for b in T]], blob, 1,
                                         alhs, inners)
        runs[name] = (S, T, alhs, want, msgs, st)
    return runs


def test_fixture_stores(fixture_runs):
    n = 0
    for name, (S, T, _, want, msgs, st) in fixture_runs.items():
        for k in range(len(S)):
            assert st[k] == 0 and msgs[k] == want[k], (name, S[k], T[k])
        n += len(S)
    assert n == 478


def test_fixture_stores_round_trip(ctx, fixture_runs):
    for name, (S, T, alhs, _, msgs, _) in fixture_runs.items():
        ok = _round_trip(ctx, msgs, S, T, [alhs[a - 1] for a in S], [alhs[b - 1] for b in T])
        assert ok.all(), name


@pytest.fixture(scope="module")
def synthetic_run(m, ctx, orc):
    s = U.synthetic_store()
    pairs = U.synthetic_pairs()
    t = _tree(m, ctx, s.alhs)
    msgs, st = t.dual_proof_pb_batch(s.recs[[a - 1 for a, _ in pairs]], s.recs[[b - 1 for _, b in pairs]],
                                     s.blob, 1, s.alhs, s.inners)
    return t, msgs, st


def test_synthetic_store(synthetic_run):
    """3000 txs whose BlTxID lags (dual_v1_gen_util.bl_of): 1-, 2- and 3-byte
    sub-message lengths, 63 / 64 / 65 nested proofs, the nil advance proof,
    tgt.bl == 0, src == tgt (asserted by test_dual_v1_gen_cpu.py)."""
    _, msgs, st = synthetic_run
    pairs, want = U.synthetic_pairs(), U.synthetic_messages()
    for k, (a, b) in enumerate(pairs):
        assert st[k] == 0, (a, b, int(st[k]))
        assert msgs[k] == want[k], (a, b, len(msgs[k]), len(want[k]))


def test_synthetic_store_round_trip(ctx, synthetic_run):
    s = U.synthetic_store()
    pairs = U.synthetic_pairs()
    _, msgs, _ = synthetic_run
    ok = _round_trip(ctx, msgs, [a for a, _ in pairs], [b for _, b in pairs],
                     [s.alhs[a - 1] for a, _ in pairs], [s.alhs[b - 1] for _, b in pairs])
    assert ok.all(), [pairs[k] for k in np.nonzero(~ok)[0][:10]]


def test_statuses(m, ctx, orc):
    """One pair per rule of ImmuStore.DualProof's order and the pairs where two
    rules hold, over a tree the digest window reaches past."""
    s = U.synthetic_store()
    t = _tree(m, ctx, s.alhs[:U.SMALL])
    cases = U.status_cases()
    w = U.windows()
    seen = set()
    for win in ("full", "sub"):
        sel = [c for c in cases if c[3][3] == win]
        blob = sel[0][3][2]
        msgs, st = t.dual_proof_pb_batch(np.array([c[3][0] for c in sel]),
                                         np.array([c[3][1] for c in sel]), blob, *w[win])
        for k, (name, est, want, (_, _, _, _, raw)) in enumerate(sel):
            assert est == want, name  # the restatement and the rule worked out by hand
            assert st[k] == want and msgs[k] == raw, (name, int(st[k]))
            assert (st[k] == 0) == (len(msgs[k]) > 0), name
            seen.add(int(st[k]))
    assert seen == {0, U.ERR_ILLEGAL_ARGUMENTS, U.ERR_UNEXISTENT_DATA, U.ERR_SOURCE_TX_NEWER,
                    U.ERR_CORRUPTED_DATA, U.ERR_CORRUPTED_TX_DATA, U.ERR_TX_NOT_FOUND}


def test_window(ctx, synthetic_run):
    """A digest window of txs 150 .. 1000 over the synthetic store: pairs it
    covers give the whole-store bytes, pairs that need tx 149 or tx 1001 get
    MH_ERR_TX_NOT_FOUND and an empty message."""
    s = U.synthetic_store()
    t, full_msgs, _ = synthetic_run
    first, alhs, inners = U.windows()["sub"]
    pairs = [(k, p) for k, p in enumerate(U.synthetic_pairs()) if 140 <= p[0] and p[1] <= 1010]
    edge = [(a, b) for a in (149, 150, 151, 152, 153) for b in (150, 154, 160)] + \
        [(a, b) for a in (990, 999, 1000) for b in (1000, 1001)] + [(149, 149), (1001, 1001)]
    edge = [(a, b) for a, b in edge if a <= b]
    P = [p for _, p in pairs] + edge
    msgs, st = t.dual_proof_pb_batch(s.recs[[a - 1 for a, _ in P]], s.recs[[b - 1 for _, b in P]], s.blob,
                                     first, alhs, inners)
    n_in = 0
    for j, (a, b) in enumerate(P):
        est, raw = U.go_dual_proof(s.recs[a - 1], s.recs[b - 1], s.blob, s.aht, first, alhs, inners)
        assert est in (0, U.ERR_TX_NOT_FOUND)
        assert st[j] == est and msgs[j] == raw, (a, b, int(st[j]))
        if j < len(pairs) and est == 0:
            assert msgs[j] == full_msgs[pairs[j][0]], (a, b)
            n_in += 1
    assert n_in > 20
    got = dict(zip(P, st))
    # tx 149 (Alh of the linear start / TargetBlTxAlh / the advance part) and tx 1001
    assert got[(149, 149)] == got[(1001, 1001)] == got[(1000, 1001)] == U.ERR_TX_NOT_FOUND
    assert got[(151, 160)] == U.ERR_TX_NOT_FOUND and got[(1000, 1000)] == 0


def test_device_phases_and_capacity(m, ctx, synthetic_run):
    """phase 1 (sizes / offsets) then phase 2 (write) through the device ABI
    with a capacity of half the messages into a canary-filled buffer; the host
    form's size query and retry; n = 0."""
    from immustore_amd import _native as N
    from immustore_amd.merkle import _addr
    L = N.load()
    s = U.synthetic_store()
    t, full_msgs, _ = synthetic_run
    pairs = U.synthetic_pairs()
    sel = list(range(0, len(pairs), 3)) + list(range(400, len(pairs)))
    n = len(sel)
    src = np.ascontiguousarray(s.recs[[pairs[k][0] - 1 for k in sel]])
    tgt = np.ascontiguousarray(s.recs[[pairs[k][1] - 1 for k in sel]])
    alh = np.frombuffer(b"".join(s.alhs), np.uint8)
    inner = np.frombuffer(b"".join(s.inners), np.uint8)
    blob = np.frombuffer(s.blob, np.uint8)
    dl = C.c_void_p()
    N.check(L.mh_ahtree_dlog_device(t.handle, C.byref(dl)))
    dsrc, dtgt, dblob = (DevBuf.from_host(ctx, x) for x in (src, tgt, blob))
    dalh, dinner = DevBuf.from_host(ctx, alh), DevBuf.from_host(ctx, inner)
    doff, dst = DevBuf(ctx, (n + 1) * 8), DevBuf(ctx, n * 4)
    scr = DevBuf(ctx, L.mh_pb_dual_scratch_size(n))

    def dev(phase, out, cap, nn=n):
        N.check(L.mh_dev_dual_proof_pb_batch(ctx.handle, phase, dl, U.N_TX, nn, C.c_void_p(dsrc.ptr),
                                             C.c_void_p(dtgt.ptr), C.c_void_p(dblob.ptr), 1, U.N_TX,
                                             C.c_void_p(dalh.ptr), C.c_void_p(dinner.ptr), out, cap,
                                             C.c_void_p(doff.ptr), C.c_void_p(dst.ptr),
                                             C.c_void_p(scr.ptr)))
        ctx.synchronize()

    dev(1, None, 0)
    off = doff.to_host(np.uint64)
    assert off[0] == 0 and np.all(np.diff(off.astype(np.int64)) > 0)
    assert [int(x) for x in np.diff(off)] == [len(full_msgs[k]) for k in sel]
    assert (dst.to_host(np.int32) == 0).all()
    cap, total = int(off[n // 2]), int(off[n])
    canary = np.full(total, 0xA5, np.uint8)
    dout = DevBuf.from_host(ctx, canary)
    dev(2, C.c_void_p(dout.ptr), cap)
    st, out = dst.to_host(np.int32), dout.to_host()
    for j, k in enumerate(sel):
        if off[j + 1] <= cap:
            assert st[j] == 0 and out[int(off[j]):int(off[j + 1])].tobytes() == full_msgs[k], pairs[k]
        else:
            assert st[j] == N.MH_ERR_BUFFER_TOO_SMALL, pairs[k]
    assert (out[cap:] == 0xA5).all()
    # host form: the size query, then the retry
    offh, sth = np.zeros(n + 1, np.uint64), np.zeros(n, np.int32)
    small = np.zeros(16, np.uint8)

    def host(out, cap, nn=n):
        return L.mh_ahtree_dual_proof_pb_batch(t.handle, nn, _addr(src), _addr(tgt), _addr(blob),
                                               blob.size, 1, U.N_TX, _addr(alh), _addr(inner),
                                               _addr(out), cap, _addr(offh), _addr(sth))
    assert host(small, 16) == N.MH_ERR_BUFFER_TOO_SMALL
    assert np.array_equal(offh, off) and (sth == 0).all() and not small.any()
    big = np.zeros(total, np.uint8)
    assert host(big, total) == 0 and (sth == 0).all()
    assert big.tobytes() == b"".join(full_msgs[k] for k in sel)
    # n = 0: off[0] = 0 and nothing else is touched
    offh[0] = 7
    assert host(None, 0, 0) == 0 and offh[0] == 0
    dev(3, None, 0, 0)
    assert doff.to_host(np.uint64)[0] == 0 and (dout.to_host()[cap:] == 0xA5).all()
