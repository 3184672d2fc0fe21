"""The resident-store check that mh_verifiable_answer_pb_batch,
mh_export_tx_batch and mh_tx_answer_pb_batch share, over one table of store
defects: every defective store is refused with MH_ERR_ILLEGAL_ARGUMENTS before
anything is launched -- off, status and a guard-banded out keep the bytes they
were filled with -- and the same context then serves the sound store.  The
store is long_linear_proof, written by Go; every call asks for tx 2 alone."""
import ctypes as C
import types

import numpy as np
import pytest

import export_util as X
import tx_spec_util as U
from answer_util import ANS_TX
from gpu_util import FILL, Guarded

pytestmark = pytest.mark.gpu
T, SINCE = 2, 1
PAST = 1 << 20  # bytes past an allocation's end, whatever its 256 bytes of slack
ILLEGAL_ARGUMENTS, TX_NOT_FOUND = 2, 25


@pytest.fixture(scope="module")
def env(fixtures, orc):
    import torch  # noqa: F401  (first: the library binds the HIP runtime torch loaded)
    import immustore_amd as m
    from immustore_amd import _native as N
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    s = U.SpecStore(X.go_store(fixtures["long_linear_proof"]))
    e = s.exp
    ctx = m.Context(0)
    tree = m.AHtree(ctx)
    tree.append_batch(np.frombuffer(b"".join(s.ans.alhs), np.uint8).reshape(-1, 32))
    exp_dev = m.ExportStore(e.raw, e.clog, list(e.vlogs), e.es, ctx=ctx, max_entries=e.max_entries)
    ans_dev = m.answers.ResidentStore(tree, e.raw, e.clog, e.es)
    assert e.vlogs[0][1], "vLog 1 of the fixture holds values"
    host = types.SimpleNamespace(  # the store's bytes in pageable host memory, kept alive here
        txlog=np.frombuffer(e.raw, np.uint8).copy(), clog=np.frombuffer(e.clog, np.uint8).copy(),
        vlog=np.frombuffer(e.vlogs[0][1], np.uint8).copy())
    yield types.SimpleNamespace(m=m, L=N.load(), s=s, ctx=ctx, tree=tree, exp_dev=exp_dev,
                                ans_dev=ans_dev, host=host)
    ans_dev.close()
    exp_dev.close()
    tree.close()
    ctx.close()


# ------------------------------------------------------------------ the three calls, one request each
def _u64(*v):
    return np.array(v, np.uint64)


def call_answer(env, d, out, cap, off, st):
    from immustore_amd.answers import _Batch
    kind, zero, none = np.array([ANS_TX], np.uint8), np.zeros(2, np.uint64), np.zeros(1, np.uint8)
    tx, since = _u64(T), _u64(SINCE)
    b = _Batch()
    b.n, b.kind, b.tx, b.prove_since = 1, kind.ctypes.data, tx.ctypes.data, since.ctypes.data
    b.keys, b.key_off, b.entries, b.entry_off = (none.ctypes.data, zero.ctypes.data, none.ctypes.data,
                                                 zero.ctypes.data)
    return env.L.mh_verifiable_answer_pb_batch(env.tree.handle, C.addressof(d), C.addressof(b), out, cap,
                                               off.ctypes.data, st.ctypes.data)


def call_export(env, d, out, cap, off, st, first_tx=T):
    return env.L.mh_export_tx_batch(env.ctx.handle, C.addressof(d), first_tx, 1, out, cap,
                                    off.ctypes.data, st.ctypes.data, None)


def call_tx_answer(env, d, out, cap, off, st):
    from immustore_amd.answers import _TxBatch
    kind, spec = np.array([U.TXA_VERIFIABLE], np.uint8), np.zeros(1, np.uint8)
    act = np.full(1, env.m.answers.MH_TXA_NO_SPEC, np.uint8)
    tx, since = _u64(T), _u64(SINCE)
    b = _TxBatch()
    b.n, b.kind, b.tx, b.prove_since = 1, kind.ctypes.data, tx.ctypes.data, since.ctypes.data
    b.has_spec, b.kv_action, b.z_action, b.sql_action = (spec.ctypes.data,) + (act.ctypes.data,) * 3
    b.now_unix = U.NOW
    return env.L.mh_tx_answer_pb_batch(env.ctx.handle, env.tree.handle, C.addressof(d), C.addressof(b),
                                       out, cap, off.ctypes.data, st.ctypes.data)


def want_answer(env):
    st, msg = env.s.ans.expect(ANS_TX, T, SINCE)
    return st, msg


def want_export(env):
    ex = env.s.exp.expect(T, 1)
    return int(ex["status"][0]), ex["blobs"][0]


def want_tx_answer(env):
    st, _, msgs = U.expect(env.s, [(U.TXA_VERIFIABLE, T, SINCE, None)])
    return int(st[0]), msgs[0]


CALLS = {"answer": (call_answer, want_answer, lambda env: env.ans_dev),
         "export": (call_export, want_export, lambda env: env.exp_dev),
         "tx_answer": (call_tx_answer, want_tx_answer, lambda env: env.exp_dev)}


# ------------------------------------------------------------------ the defects
def vlog_table(dev):
    """the store's vLog table in 128 slots of the test's own"""
    from immustore_amd.export import _Vlog
    vl = (_Vlog * 128)()
    for k in range(dev.nvlogs):
        vl[k].data, vl[k].first_off, vl[k].end_off = dev._vl[k].data, dev._vl[k].first_off, dev._vl[k].end_off
    return vl


def es_13(d, vl, host):
    d.clog_entry_size = 13


def txlog_on_host(d, vl, host):
    d.txlog = host.txlog.ctypes.data


def clog_on_host(d, vl, host):
    d.clog = host.clog.ctypes.data


def txlog_len_past_slack(d, vl, host):
    d.txlog_len += PAST


def nvlogs_128(d, vl, host):
    d.nvlogs = 128


def vlogs_null(d, vl, host):
    d.vlogs = None


def vlog_end_before_first(d, vl, host):
    vl[0].first_off = vl[0].end_off + 1


def vlog_data_null(d, vl, host):
    vl[0].data = None


def vlog_data_on_host(d, vl, host):
    vl[0].data = host.vlog.ctypes.data


def vlog_data_misaligned(d, vl, host):
    vl[0].data += 2


def vlog_end_past_slack(d, vl, host):
    vl[0].end_off += PAST


STORE_DEFECTS = [es_13, txlog_on_host, clog_on_host, txlog_len_past_slack]
VLOG_DEFECTS = [nvlogs_128, vlogs_null, vlog_end_before_first, vlog_data_null, vlog_data_on_host,
                vlog_data_misaligned, vlog_end_past_slack]
CASES = [(c, f) for c in CALLS for f in STORE_DEFECTS + (VLOG_DEFECTS if c != "answer" else [])]


def defective(env, name, defect):
    """-> (descriptor, what it points to): the sound store's with one defect"""
    dev = CALLS[name][2](env)
    d = dev.descriptor()
    vl = None
    if name != "answer":
        vl = vlog_table(dev)
        d.vlogs = C.addressof(vl)
    defect(d, vl, env.host)
    return d, vl


def serves(env, name):
    """the sound store through call `name`: status, off and the bytes, inside the guards"""
    call, want, dev = CALLS[name]
    est, emsg = want(env)
    assert est == 0 and emsg
    d = dev(env).descriptor()
    out = Guarded(len(emsg), pinned=True)
    off, st = np.zeros(2, np.uint64), np.full(1, -1, np.int32)
    try:
        assert call(env, d, out.ptr, len(emsg), off, st) == 0
        assert (int(st[0]), off.tolist()) == (0, [0, len(emsg)])
        assert bytes(out.payload()) == emsg and out.guards_intact()
    finally:
        out.free()


@pytest.mark.parametrize("name,defect", CASES, ids=["%s-%s" % (c, f.__name__) for c, f in CASES])
def test_defective_store_is_refused_untouched(env, name, defect):
    d, keep = defective(env, name, defect)
    out = Guarded(256, pinned=True)
    off, st = np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(1, 0x5A5A5A5A, np.int32)
    try:
        rc = CALLS[name][0](env, d, out.ptr, 256, off, st)
        assert rc == ILLEGAL_ARGUMENTS
        assert off.tolist() == [0xA5A5A5A5A5A5A5A5] * 2 and st.tolist() == [0x5A5A5A5A]
        assert out.untouched() and (out.payload() == FILL).all()
    finally:
        out.free()
    del keep
    serves(env, name)


def test_export_tx_not_found_comes_before_placement(env):
    """first_tx past the store and the tx log in host memory: ErrTxNotFound, as
    the range is settled by the arguments alone, ahead of where the store lies"""
    d, _ = defective(env, "export", txlog_on_host)
    out = Guarded(256, pinned=True)
    off, st = np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(1, 0x5A5A5A5A, np.int32)
    try:
        assert call_export(env, d, out.ptr, 256, off, st, first_tx=env.s.ntx + 1) == TX_NOT_FOUND
        assert off.tolist() == [0xA5A5A5A5A5A5A5A5] * 2 and st.tolist() == [0x5A5A5A5A]
        assert out.untouched()
    finally:
        out.free()
    serves(env, "export")
