"""mh_tx_answer_pb_batch without a device: the CPU restatement of
tests/tx_spec_util.py against the Go-written fixture stores, the binding of the
call in the header, _native.py, answers.py and the Go shim, and the argument
checks that come ahead of any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import answer_util as A
import export_util as X
import tx_spec_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO_STORES = ["long_linear_proof", "v110_defaultdb", "v110_systemdb"]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", GO_STORES)
def test_restatement_returns_every_stored_value(fixtures, orc, name):
    """RAW_VALUE over a store Go wrote: every entry with the value Go stored"""
    fx = fixtures[name]
    s = U.SpecStore(X.go_store(fx))
    M = U.messages()
    seen = stored = 0
    for T, t in enumerate(fx["txs"], 1):
        st, msg, sized = U.serialize_tx(s, T, U.ALL_RAW, 0)
        assert (st, sized) == (U.OK, True)
        tx = M["Tx"].FromString(msg)
        want = [e for e in t["entries"] if bytes.fromhex(e["key"])[0] <= 2]
        assert len(tx.entries) == len(want)
        stored += sum(1 for e in want if e["vlen"])
        for got, e in zip(tx.entries, want):
            assert got.key == bytes.fromhex(e["key"]) and got.vLen == e["vlen"]
            assert got.value == bytes.fromhex(e["value"])
            seen += len(got.value) > 0
        assert tx.header.SerializeToString(deterministic=True) == \
            M["Tx"].FromString(s.ans.tx_proto(T)).header.SerializeToString(deterministic=True)
        assert U.expect_one(s, U.TXA_TX, T, 0, U.ALL_RAW, 0) == (U.OK, msg, len(msg))
    # (long_linear_proof was written through the embedded store: its keys carry no
    # database prefix, and serializeTx drops every one of them)
    assert seen == stored and (stored > 0 or name == "long_linear_proof")


@pytest.mark.parametrize("name", GO_STORES)
def test_nil_spec_is_tx_to_proto(fixtures, orc, name):
    fx = fixtures[name]
    s = U.SpecStore(X.go_store(fx))
    a = A.fixture_store(fx)
    digest = (U.ONLY_DIGEST,) * 3
    for T in range(1, s.ntx + 1):
        assert U.serialize_tx(s, T, None) == (U.OK, a.tx_proto(T), True)
        if all(e[1][0] <= 2 for e in s.entries(T)):  # every class asked as a digest: the same entries
            assert U.serialize_tx(s, T, digest)[1] == a.tx_proto(T)
        for S in (0, 1, T, s.ntx):
            assert U.expect_one(s, U.TXA_VERIFIABLE, T, S, None)[:2] == a.expect(A.ANS_TX, T, S)


def test_synthetic_store_holds_what_it_promises(orc):
    S = U.synthetic()
    s = S.store
    assert 35 <= s.ntx <= 50 and [t for t in range(1, s.ntx + 1) if s.exp.rst[t - 1]] == [S.corrupt]
    ents = [e for T in range(1, s.ntx + 1) if T != S.corrupt for e in s.entries(T)]
    assert {len(s.entries(S.roles["width_%d" % w])) for w in U.WIDTHS} == set(U.WIDTHS)
    assert set(U.VALUE_LENS) <= {e[2] for e in ents}
    assert {0, 1, 2, 3, 0xff} <= {e[1][0] for e in ents if e[1]}
    assert any(e[2] == 0 and e[4] != orc.sha256(b"") for e in ents)
    exps = {A.md_flags(e[0])[1] for e in ents if e[0]}
    assert set(U.EXPIRES) <= exps
    for T, want in S.tx_tuned.items():
        assert len(U.serialize_tx(s, T, U.ALL_RAW)[1]) == want
    # what the flips and the missing values give, by Go's order
    r = S.roles
    one = lambda role, spec: U.serialize_tx(s, r[role], spec)[0]  # noqa: E731
    raw, none = U.RAW_VALUE, None
    assert one("flip_lowest", U.ALL_RAW) == one("flip_highest", U.ALL_RAW) == U.CORRUPTED_DATA
    assert one("flip_in_excluded", (raw, none, raw)) == U.OK
    assert one("flip_in_excluded", (raw, U.ONLY_DIGEST, raw)) == U.OK
    assert one("flip_in_excluded", U.ALL_RAW) == U.CORRUPTED_DATA
    assert one("flip_behind_excluded", (raw, none, raw)) == U.CORRUPTED_DATA
    assert one("flip_in_expired", U.ALL_RAW) == U.OK
    assert one("flip_behind_expired", U.ALL_RAW) == U.CORRUPTED_DATA
    assert one("flip_ahead_of_sql", (raw, raw, U.RESOLVE)) == U.CORRUPTED_DATA
    assert one("flip_behind_sql", (raw, raw, U.RESOLVE)) == U.ILLEGAL_ARGUMENTS
    assert one("flip_behind_sql", (raw, raw, raw)) == U.CORRUPTED_DATA
    assert one("id_zero", U.ALL_RAW) == one("behind_window", U.ALL_RAW) == one("straddle_end", U.ALL_RAW) == U.EOF
    assert one("id_zero", (raw, U.ONLY_DIGEST, raw)) == U.OK
    assert one("no_such_vlog", U.ALL_RAW) == one("empty_key", (none, none, none)) == U.ILLEGAL_STATE
    assert one("exact_end", U.ALL_RAW) == one("empty_value", U.ALL_RAW) == one("empty_key", None) == U.OK


# ------------------------------------------------------------------ the binding
def _header():
    return open(os.path.join(ROOT, "include", "immustore_merkle.h")).read()


def test_symbol_status_and_layout_are_bound():
    from immustore_amd import _native as N
    from immustore_amd import answers
    hdr = _header()
    assert re.search(r"#define\s+MH_ERR_EOF\s+36\b", hdr) and N.MH_ERR_EOF == 36
    assert re.search(r"MH_TXA_TX = 0,", hdr) and re.search(r"MH_TXA_VERIFIABLE = 1\b", hdr)
    assert re.search(r"#define\s+MH_TXA_NO_SPEC\s+0xff\b", hdr)
    assert (N.MH_TXA_TX, N.MH_TXA_VERIFIABLE, N.MH_TXA_NO_SPEC) == (0, 1, 0xff)
    assert issubclass(N.ErrEOF, N.MerkleError)
    with pytest.raises(N.ErrEOF):
        N.check(N.MH_ERR_EOF)
    # the struct as the header declares it, field for field
    body = re.search(r"typedef struct mh_tx_answer_batch \{(.*?)\} mh_tx_answer_batch;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(f.strip().rsplit(None, 1)[0].replace(" ", ""), f.strip().rsplit(None, 1)[1].lstrip("*"))
              for f in body.split(";") if f.strip()]
    names = [re.sub(r"^\*+", "", n) for _, n in fields]
    assert names == [n for n, _ in answers._TxBatch._fields_]
    assert names == ["n", "kind", "tx", "prove_since", "has_spec", "kv_action", "z_action", "sql_action",
                     "now_unix"]
    assert C.sizeof(answers._TxBatch) == 72 and answers._TxBatch.now_unix.offset == 64
    # the prototype and the ctypes signature
    proto = re.search(r"int mh_tx_answer_pb_batch\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)
    assert proto and proto.group(1).count(",") + 1 == 8
    res, args = N.SIGNATURES["mh_tx_answer_pb_batch"]
    assert res is C.c_int and len(args) == 8
    assert hasattr(N.load(), "mh_tx_answer_pb_batch")
    import immustore_amd as m
    assert m.tx_answers is answers.tx_answers and callable(m.tx_list)


def test_go_shim_binds_the_call():
    src = open(os.path.join(ROOT, "go", "store", "answers_mi355x.go")).read()
    assert "C.mh_tx_answer_pb_batch(" in src and "C.MH_ERR_EOF" in src and "C.MH_TXA_NO_SPEC" in src
    assert re.search(r"if st == C\.MH_ERR_EOF \{\s*return io\.EOF", src)
    assert re.search(r"func TxAnswers\(store \*ExportableStore, tree \*ReplicaTree, reqs \[\]TxAnswerRequest, "
                     r"now time\.Time\)", src)
    assert re.search(r"type TxAnswerRequest struct \{\s*Kind\s+int\s*Tx, ProveSinceTx uint64\s*Spec\s+\*EntriesSpec",
                     src)
    assert "func TxScan(" in src and "0x0a" in src[src.index("func TxScan("):]


def test_tx_list_framing():
    from immustore_amd import answers
    M = U.messages()
    assert answers.tx_list([]) == b""
    msgs = [b"", b"\x0a\x00", bytes(127), bytes(128), bytes(16384)]
    raw = answers.tx_list(msgs)
    want = b"".join(b"\x0a" + A._varint(len(x)) + x for x in msgs)
    assert raw == want
    assert "TxList" not in M or len(M["TxList"].FromString(answers.tx_list([b"", b""])).txs) == 2


# ------------------------------------------------------------------ arguments, no device
def _call(ctx, tree, store, batch, out=None, cap=0, off=None, st=None):
    from immustore_amd import _native as N
    return N.load().mh_tx_answer_pb_batch(ctx, tree, store, batch, out, cap, off, st)


def _batch(n, kind=0, spec=None):
    from immustore_amd import answers
    keep = [np.full(n, kind, np.uint8), np.ones(n, np.uint64), np.zeros(n, np.uint64),
            np.full(n, 0 if spec is None else 1, np.uint8)]
    keep += [np.full(n, 0xff if spec is None or spec[k] is None else spec[k], np.uint8) for k in range(3)]
    b = answers._TxBatch()
    b.n = n
    b.kind, b.tx, b.prove_since, b.has_spec, b.kv_action, b.z_action, b.sql_action = \
        (a.ctypes.data for a in keep)
    b.now_unix = U.NOW
    return b, keep


def test_arguments_without_a_device():
    """every check that comes ahead of the device: a status, nothing touched
    (ctx is never dereferenced by them: a dummy block stands in for it)"""
    from immustore_amd import export
    ILL = U.ILLEGAL_ARGUMENTS
    ctx = C.create_string_buffer(4096)
    store = export._Store()
    store.clog_entry_size = 12
    off, st = np.zeros(4, np.uint64), np.zeros(4, np.int32)
    b, keep = _batch(2)
    sa, ba = C.addressof(store), C.addressof(b)
    assert _call(None, None, sa, ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    assert _call(ctx, None, None, ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    assert _call(ctx, None, sa, None, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    assert _call(ctx, None, sa, ba, None, 0, None, st.ctypes.data) == ILL
    assert _call(ctx, None, sa, ba, None, 0, off.ctypes.data, None) == ILL
    assert _call(ctx, None, sa, ba, None, 16, off.ctypes.data, st.ctypes.data) == ILL  # out NULL, a capacity
    e, _k = _batch(0)
    off[0] = 7
    assert _call(ctx, None, sa, C.addressof(e), None, 0, off.ctypes.data, st.ctypes.data) == 0 and off[0] == 0
    for field in ("kind", "tx", "prove_since", "has_spec", "kv_action", "z_action", "sql_action"):
        b2, k2 = _batch(2)
        setattr(b2, field, None)
        assert _call(ctx, None, sa, C.addressof(b2), None, 0, off.ctypes.data, st.ctypes.data) == ILL, field
    for es in (0, 13, 43):
        s2 = export._Store()
        s2.clog_entry_size = es
        assert _call(ctx, None, C.addressof(s2), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    s3 = export._Store()
    s3.clog_entry_size, s3.nvlogs = 12, 128
    assert _call(ctx, None, C.addressof(s3), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    s3.nvlogs = 1  # a vLog table that is not there
    assert _call(ctx, None, C.addressof(s3), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    vl = (export._Vlog * 1)()
    vl[0].data, vl[0].first_off, vl[0].end_off = 0x1002, 0, 8  # not 4-byte aligned
    s3.vlogs = C.addressof(vl)
    assert _call(ctx, None, C.addressof(s3), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    vl[0].data, vl[0].first_off, vl[0].end_off = 0x1000, 9, 8  # ends ahead of its start
    assert _call(ctx, None, C.addressof(s3), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    s4 = export._Store()
    s4.clog_entry_size, s4.ntx = 12, 3  # txs, but no logs
    assert _call(ctx, None, C.addressof(s4), ba, None, 0, off.ctypes.data, st.ctypes.data) == ILL
    # inconsistent requests
    for kw in (dict(kind=2), dict(kind=1),  # outside the enum; VERIFIABLE without a tree
               dict(spec=(4, None, None)), dict(spec=(None, None, 0xfe)),
               dict(spec=(U.RESOLVE, None, None)), dict(spec=(None, U.RESOLVE, U.RAW_VALUE)),
               dict(spec=(U.RESOLVE, U.RESOLVE, U.RESOLVE))):
        b5, k5 = _batch(2, **kw)
        assert _call(ctx, None, sa, C.addressof(b5), None, 0, off.ctypes.data, st.ctypes.data) == ILL, kw
    # kv RESOLVE on one request of many refuses the whole call
    b6, k6 = _batch(5, spec=(U.RAW_VALUE, U.RAW_VALUE, U.RESOLVE))
    k6[4][3] = U.RESOLVE
    assert _call(ctx, None, sa, C.addressof(b6), None, 0, off.ctypes.data, st.ctypes.data) == ILL
    assert bytes(ctx.raw) == bytes(4096)
