"""mh_replicate_tx_batch without a device: the CPU reference of the GPU tests
(tests/replicate_util.py) pinned against the Go-written stores and against
the directed mutant table, and the argument errors of the C call that need no
device."""
import ctypes as C

import numpy as np
import pytest

import replicate_util as R


@pytest.mark.parametrize("store", ["long_linear_proof", "v110_defaultdb", "v110_systemdb"])
def test_reference_replays_go_stores(fixtures, orc, store):
    """Export the fixture's txs from its keys, values and headers and replay
    them onto an empty tree: all accepted, the stored Alh of every tx, the
    stored aht dLog bytes."""
    blobs, alhs, dlog = R.fixture_store(fixtures[store])
    assert len(blobs) == {"long_linear_proof": 30, "v110_defaultdb": 4, "v110_systemdb": 2}[store]
    r = R.reference(orc, blobs, orc.AHtree(1), orc.sha256(b""))
    assert r["accepted"] == len(blobs) and not r["status"].any()
    assert [bytes(a) for a in r["alh"]] == alhs
    assert r["size"] == len(blobs) and r["dlog"] == dlog
    for k, t in enumerate(fixtures[store]["txs"]):
        lo, hi = int(r["ent_off"][k]), int(r["ent_off"][k + 1])
        assert [bytes(h) for h in r["hvals"][lo:hi]] == [bytes.fromhex(e["hval"]) for e in t["entries"]]
        assert bytes(r["hdrs"][k]["eh"]) == bytes.fromhex(t["header"]["eh"])
    # split in two calls at every position: the same tree
    for cut in range(len(blobs) + 1):
        t = orc.AHtree(1)
        a = R.reference(orc, blobs[:cut], t, orc.sha256(b""))
        t2 = orc.AHtree(1)
        t2.dlog = np.frombuffer(a["dlog"], np.uint8).reshape(-1, 32).copy() if a["size"] else t2.dlog
        t2.size = a["size"]
        b = R.reference(orc, blobs[cut:], t2, alhs[cut - 1] if cut else orc.sha256(b""))
        assert a["accepted"] + b["accepted"] == len(blobs) and b["dlog"] == dlog


@pytest.fixture(scope="module")
def mutant_batches(orc):
    """7 valid txs behind a tree of 3; the mutant table derived from txs 0, 3, 6"""
    txs, trees = R.synthetic_store(orc, R.simple_specs(10))
    P = 3
    rows = {}
    for pos in (0, 3, 6):
        k = P + pos
        rows[pos] = R.mutants(orc, txs[k], R.prev_alh_of(orc, txs, k), trees[k])
    return txs, trees, P, rows


def test_mutant_table(orc, mutant_batches):
    """The reference agrees with the table at the head, in the middle and at
    the end of a batch; every status of the contract occurs."""
    txs, trees, P, rows = mutant_batches
    seen = set()
    names = [r[0] for r in rows[0]]
    assert len(set(names)) == len(names) >= 50
    for pos, table in rows.items():
        for name, blob, want in table:
            blobs = [t["blob"] for t in txs[P:P + 7]]
            blobs[pos] = blob
            r = R.reference(orc, blobs, trees[P], R.prev_alh_of(orc, txs, P), R.MUT_LIMITS)
            st = r["status"].tolist()
            assert st[pos] == want, (name, pos, st)
            assert st[:pos] == [0] * pos, (name, pos, st)
            if want == R.OK:
                # the valid rows re-hash to another Alh: the next tx fails on PrevAlh
                ok_all = blob == txs[P + pos]["blob"] or name in ("no_trailer", "trailer_two_bytes",
                                                                 "bytes_after_blroot")
                assert r["accepted"] == (7 if ok_all or pos == 6 else pos + 1), (name, pos, st)
                if not ok_all and pos < 6:
                    assert st[pos + 1] == R.ILLEGAL
                    assert st[pos + 2:] == [R.NOT_REACHED] * (5 - pos)
            else:
                assert r["accepted"] == pos and r["size"] == P + pos
                assert st[pos + 1:] == [R.NOT_REACHED] * (6 - pos), (name, pos, st)
            seen |= set(st)
    assert seen == R.ALL_CODES


def test_local_verdict_survives_the_break(orc, mutant_batches):
    """Behind the first refused tx a tx keeps its own envelope-through-Eh error"""
    txs, trees, P, rows = mutant_batches
    table = {n: b for n, b, _ in rows[3]}
    blobs = [t["blob"] for t in txs[P:P + 7]]
    blobs[1] = b""
    blobs[3] = table["null_key"]
    blobs[5] = R._hdr_edit(txs[P + 5], eh=bytes(32))
    r = R.reference(orc, blobs, trees[P], R.prev_alh_of(orc, txs, P), R.MUT_LIMITS)
    assert r["status"].tolist() == [0, R.ILLEGAL, R.NOT_REACHED, R.NULL_KEY, R.NOT_REACHED, R.ILLEGAL,
                                    R.NOT_REACHED]
    assert r["accepted"] == 1


def test_argument_errors():
    """NULL handle / batch / status / accepted: MH_ERR_ILLEGAL_ARGUMENTS before
    any device work; n == 0 with a handle-shaped pointer never reaches it"""
    from immustore_amd import _native as N
    from immustore_amd.replicate import _Batch
    L = N.load()
    b = _Batch()
    st = np.zeros(1, np.int32)
    acc = C.c_uint64(7)
    args = (None, None, None, None, 0, None)
    f = L.mh_replicate_tx_batch
    assert f(None, C.addressof(b), st.ctypes.data, C.byref(acc), None, *args) == N.MH_ERR_ILLEGAL_ARGUMENTS
    fake = C.create_string_buffer(8)  # never dereferenced on these paths
    h = C.addressof(fake)
    assert f(h, None, st.ctypes.data, C.byref(acc), None, *args) == N.MH_ERR_ILLEGAL_ARGUMENTS
    assert f(h, C.addressof(b), None, C.byref(acc), None, *args) == N.MH_ERR_ILLEGAL_ARGUMENTS
    assert f(h, C.addressof(b), st.ctypes.data, None, None, *args) == N.MH_ERR_ILLEGAL_ARGUMENTS
    assert acc.value == 7
    eo = np.full(1, 9, np.uint64)
    a2 = (None, None, eo.ctypes.data, None, 0, None)
    assert f(h, C.addressof(b), st.ctypes.data, C.byref(acc), None, *a2) == N.MH_OK  # n == 0
    assert acc.value == 0 and eo[0] == 0


def test_status_strings_and_mirror():
    from immustore_amd import _native as N
    L = N.load()
    for code, word in ((26, b"newer version"), (27, b"truncation"), (28, b"null key"),
                       (29, b"max key length"), (30, b"max value length"), (31, b"max number of entries"),
                       (32, b"already committed"), (33, b"wrong order"), (34, b"not reached")):
        assert word in L.mh_status_string(code)
        assert code in N._ERRORS
    assert L.mh_status_string(35) == b"unknown status"
    assert (N.MH_ERR_NEWER_VERSION_OR_CORRUPTED, N.MH_ERR_TX_NOT_REACHED) == (26, 34)
