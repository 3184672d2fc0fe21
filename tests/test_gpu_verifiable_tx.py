"""mh_verify_verifiable_tx_pb_batch / mh_multi_verify_verifiable_tx_pb_batch:
whole VerifiableTx answers -- the verified writes (VerifiedSet, SetAll,
VerifiedSetReferenceAt, VerifiedZAddAt) and VerifiedTxByID of pkg/client --
verified in one device pass.  Every expectation (status, ok, new_tx, new_alh,
eh_out) comes from the CPU reference of tests/verifiable_tx_util.py (protobuf
runtime + C oracle), never from the library; the cases are built there too."""
import os

import numpy as np
import pytest

import verifiable_tx_util as V

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
    return txlayer.verify_verifiable_tx_pb_batch(*V.columns(cases), ctx=ctx, **kw)


@pytest.fixture(scope="module")
def good(orc):
    return V.expectations(V.good_cases)


@pytest.fixture(scope="module")
def tampered(orc):
    return V.expectations(V.tamper_cases)


@pytest.fixture(scope="module")
def hostile(orc):
    return V.expectations(V.hostile_set)


def test_good_answers_in_one_batch(ctx, good):
    """every tx as SET_ALL, every one-entry tx under its kind, TX_BY_ID from
    both sides: width 1 and width 1024 share the launches"""
    cases, exp = good
    widths = {len(c[3]) for c in cases}
    assert {0, 1, 64, 65, 1024} <= widths and {c[2] for c in cases} == set(range(5))
    got = _fused(cases, ctx)
    V.check(got, cases, exp)
    # the SET entries with the deleted attribute alone are refused
    assert all(c[2] == V.SET for c, e in zip(cases, exp) if not e[1])
    # 64 / 65: the two arms of build_many_dev, each alone in its batch
    for w in (64, 65):
        sub = [(c, e) for c, e in zip(cases, exp) if len(c[3]) <= w]
        V.check(_fused([c for c, _ in sub], ctx), [c for c, _ in sub], [e for _, e in sub])


def test_many_small_trees(ctx, good):
    """more than 2048 trees of at most 64 leaves: the packed small-roots arm"""
    sub = [(c, e) for c, e in zip(*good) if 1 <= len(c[3]) <= 64]
    reps = 2048 // len(sub) + 1
    cases, exp = [c for c, _ in sub] * reps, [e for _, e in sub] * reps
    assert len(cases) > 2048
    V.check(_fused(cases, ctx), cases, exp)


def test_state_cases(ctx, orc):
    cases, exp = V.expectations(V.state_cases)
    V.check(_fused(cases, ctx), cases, exp)
    assert {e[1] for e in exp} == {True, False}


def test_tampered(ctx, tampered):
    cases, exp = tampered
    V.check(_fused(cases, ctx), cases, exp)
    assert {e[0] for e in exp} >= {0, 2, 21} and {e[1] for e in exp} == {True, False}


def test_encodings(ctx, orc):
    cases, exp = V.expectations(V.encoding_cases)
    V.check(_fused(cases, ctx), cases, exp)
    assert {e[0] for e in exp} == {0, 2, 14, 21}


def test_hostile_vs_cpu_reference(ctx, hostile):
    cases, exp = hostile
    assert 1400 <= len(cases) <= 1600
    V.check(_fused(cases, ctx), cases, exp)


def test_offsets_need_not_start_at_zero(ctx, tampered):
    cases, exp = tampered[0][:200], tampered[1][:200]
    V.check(_fused(cases, ctx, lead=13), cases, exp)


def test_chunks(ctx, good, tampered, hostile):
    """MH_PB_CHUNK_MIB=1 with MH_PB_GROUP_RATIO=0 over > 3 MiB of answers: at
    least 3 chunks, each decoded and verified on its own, equal the default run"""
    cases = good[0] + tampered[0] + hostile[0]
    exp = good[1] + tampered[1] + hostile[1]
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
    V.check(one, cases, exp)
    for other in (grouped, many):
        for a, b in zip(one, other):
            assert np.array_equal(a, b)


def test_multi_equals_single(m, ctx, good, tampered, hostile):
    """contexts on device 0 listed 1, 2 and 4 times == the single-device call"""
    from immustore_amd.multi import MultiDevice
    cases = good[0][::3] + tampered[0][::3] + hostile[0][::3]
    one = _fused(cases, ctx)
    for K in (1, 2, 4):
        mc = MultiDevice([0] * K)
        try:
            got = mc.verify_verifiable_tx_pb_batch(*V.columns(cases))
        finally:
            mc.close()
        for a, b in zip(one, got):
            assert np.array_equal(a, b), K
    assert one[1].any() and not one[1].all()


def test_arguments(m, ctx, good):
    import ctypes as C
    from immustore_amd import _native as N
    from immustore_amd.txlayer import _VerifiedTxBatch, pack_verified_tx_batch, _addr
    L = N.load()
    fine = [(c, e) for c, e in zip(*good) if len(c[3]) <= 9 and e[1]]
    picked = [x for i in range(12) for kind in range(5)
              for x in [y for y in fine if y[0][2] == kind][i:i + 1]]  # the kinds interleaved
    cases, exp = [c for c, _ in picked], [e for _, e in picked]
    assert {c[2] for c in cases} == set(range(5))
    n = len(cases)
    b, keep = pack_verified_tx_batch(*V.columns(cases))
    st, ok = np.full(n, -1, np.int32), np.full(n, 7, np.uint8)
    ntx, nalh, eh = np.full(n, 7, np.uint64), np.full((n, 32), 7, np.uint8), np.full((n, 32), 7, np.uint8)
    outs = [_addr(st), _addr(ok), _addr(ntx), _addr(nalh), _addr(eh)]
    fn = L.mh_verify_verifiable_tx_pb_batch
    fields = [f for f, _ in _VerifiedTxBatch._fields_[1:]]
    # n == 0: nothing read, nothing written
    empty = _VerifiedTxBatch(0, *([None] * len(fields)))
    assert fn(ctx.handle, C.byref(empty), *([None] * 5)) == 0
    # a null context, a null batch, each null pointer of the batch, each null output
    assert fn(None, C.byref(b), *outs) == 2
    assert fn(ctx.handle, None, *outs) == 2
    for f in fields:
        bad = _VerifiedTxBatch(n, *[None if g == f else getattr(b, g) for g in fields])
        assert fn(ctx.handle, C.byref(bad), *outs) == 2, f
    for k in range(4):
        o = list(outs)
        o[k] = None
        assert fn(ctx.handle, C.byref(b), *o) == 2, k

    def with_(which, arr):
        return _VerifiedTxBatch(n, *[_addr(arr) if g == which else getattr(b, g) for g in fields])

    # offsets running backwards
    for which, arr in (("msg_off", keep[1]), ("spec_off", keep[3]), ("key_off", keep[5]),
                       ("val_off", keep[7])):
        x = arr.copy()
        x[5], x[7] = x[7] + 1, x[5]
        assert fn(ctx.handle, C.byref(with_(which, x)), *outs) == 2, which
    # a kind outside the enum; a K that breaks its kind's rule
    kd, soff = keep[2], keep[3]
    x = kd.copy()
    x[3] = 5
    assert fn(ctx.handle, C.byref(with_("kind", x)), *outs) == 2
    for p in range(n):
        K = int(soff[p + 1] - soff[p])
        for other in range(5):
            fits = {V.SET: K == 1, V.REFERENCE: K == 1, V.ZADD: K == 1, V.SET_ALL: K >= 1,
                    V.TX_BY_ID: K == 0}[other]
            if not fits:
                x = kd.copy()
                x[p] = other
                assert fn(ctx.handle, C.byref(with_("kind", x)), *outs) == 2, (p, other)
        if p > 8:
            break
    # more answers than the VerifiableGet call takes
    bad = _VerifiedTxBatch(8013009, *[getattr(b, g) for g in fields])
    assert fn(ctx.handle, C.byref(bad), *outs) == 2
    assert (st == -1).all() and (ok == 7).all() and (ntx == 7).all() and (nalh == 7).all() and \
        (eh == 7).all()
    # the batch itself; eh_out may be NULL
    assert fn(ctx.handle, C.byref(b), *outs[:4], None) == 0
    assert (st == 0).all() and (ok == 1).all() and (eh == 7).all()
    assert fn(ctx.handle, C.byref(b), *outs) == 0
    V.check((st, ok, ntx, nalh, eh), cases, exp)
    # a sub-range: the per-answer arrays advanced alike, no offset starting at 0
    lo, cnt = 7, 25
    sub = _VerifiedTxBatch(cnt, b.msgs, b.msg_off + 8 * lo, b.kind + lo, b.spec_off + 8 * lo, b.keys,
                           b.key_off, b.vals, b.val_off, b.at_tx + 8 * lo, b.state_tx + 8 * lo,
                           b.state_alh + 32 * lo)
    st2, ok2 = np.full(cnt, -1, np.int32), np.zeros(cnt, np.uint8)
    ntx2, nalh2, eh2 = np.zeros(cnt, np.uint64), np.zeros((cnt, 32), np.uint8), np.zeros((cnt, 32), np.uint8)
    assert fn(ctx.handle, C.byref(sub), _addr(st2), _addr(ok2), _addr(ntx2), _addr(nalh2),
              _addr(eh2)) == 0
    V.check((st2, ok2, ntx2, nalh2, eh2), cases[lo:lo + cnt], exp[lo:lo + cnt])
    del keep
