"""mh_export_tx_batch without a device: the CPU restatement of the GPU tests
(tests/export_util.py) pinned against the Go-written stores and the
replication reference, the synthetic store's coverage, and the argument errors
of the C call that need no device."""
import collections
import ctypes as C

import numpy as np
import pytest

import export_util as X
import replicate_util as R

GO_STORES = ["long_linear_proof", "v110_defaultdb", "v110_systemdb"]


@pytest.mark.parametrize("store", GO_STORES)
def test_restatement_exports_go_stores(fixtures, orc, store):
    """The restatement's blobs are those the replication tests pin
    (replicate_util.fixture_store), every tx MH_OK and not truncated; the
    replication reference accepts them onto an empty tree and yields the stored
    aht dLog.  go_store() asserts that the values tile vLog 1 without gaps."""
    fx = fixtures[store]
    s = X.go_store(fx)
    blobs, alhs, dlog = R.fixture_store(fx)
    ex = s.expect()
    assert not ex["status"].any() and not ex["truncated"].any()
    assert ex["blobs"] == blobs
    assert ex["off"].tolist() == [0] + np.cumsum([len(b) for b in blobs]).tolist()
    r = R.reference(orc, ex["blobs"], orc.AHtree(1), orc.sha256(b""))
    assert r["accepted"] == len(blobs) and r["dlog"] == dlog
    assert [bytes(a) for a in r["alh"]] == alhs
    # ranges are slices of the whole
    sub = s.expect(2, len(blobs) - 1)
    assert sub["blobs"] == blobs[1:]


def test_defaultdb_holds_empty_values_with_vlog_id_0(fixtures):
    ents = [e for t in fixtures["v110_defaultdb"]["txs"] for e in t["entries"]]
    assert any(e["vlen"] == 0 and X.decode_offset(e["voff"])[0] == 0 for e in ents)


def test_decode_offset_uses_gos_mask():
    """0xff << 55: bit 55 is dropped with the id's low seven bits, bit 63 stays"""
    assert X.decode_offset((1 << 56) | 77) == (1, 77)
    assert X.decode_offset((3 << 56) | (1 << 55) | 5) == (3, 5)
    assert X.decode_offset((0x81 << 56) | 9) == (0x81, (1 << 63) | 9)
    assert X.decode_offset((1 << 54) | 1) == (0, (1 << 54) | 1)


@pytest.fixture(scope="module")
def syn(orc):
    S = X.synthetic(orc)
    S.ex = S.store.expect()
    return S


def test_synthetic_store_coverage(orc, syn):
    """What synthetic() promises: the lengths, widths, versions, metadata kinds
    and key lengths; every (source alignment, destination alignment) pair with a
    short and a multi-block value; the truncation cases with their statuses."""
    st, ex = syn.store, syn.ex
    assert 40 <= st.ntx <= 60 and not any(st.rst)
    assert not ex["status"][:syn.n_clean].any() and not ex["truncated"][:syn.n_clean].any()
    recs = [st.record(t) for t in range(1, st.ntx + 1)]
    assert {h["version"] for h, _ in recs} == {0, 1}
    assert {h["md"] for h, _ in recs} >= set(X.TX_MDS)
    assert {e[0] for _, es in recs for e in es} == set(X.KV_MDS)
    kls = {len(e[1]) for _, es in recs for e in es}
    assert {1, 2, 3, 1023, 1024} <= kls and max(kls) == 1024
    assert {len(es) for _, es in recs} >= set(X.WIDTHS)
    assert {e[2] for _, es in recs for e in es} >= set(X.VALUE_LENS)
    assert {X.decode_offset(e[3])[0] for _, es in recs for e in es if e[2]} >= {0, 1, 2, 3, 127}
    assert len(st.vlogs) == 2 and st.vlogs[0][0] == 0 and st.vlogs[1][0] == X.V2_FIRST > 0
    cov = X.alignment_coverage(st, ex)
    short = collections.Counter((a, b) for a, b, L in cov if L <= 3)
    multi = collections.Counter((a, b) for a, b, L in cov if L > 128)
    pairs = {(a, b) for a in range(4) for b in range(4)}
    assert set(short) == pairs and set(multi) == pairs
    want = dict(behind_window=(X.OK, 1), straddle_start=(X.OK, 1), id_zero=(X.OK, 1),
                mixed_avail_first=(X.CORRUPTED_DATA, 0), mixed_trunc_first=(X.CORRUPTED_DATA, 0),
                empty_in_truncated=(X.CORRUPTED_DATA, 0), no_such_vlog=(X.ILLEGAL_STATE, 0),
                no_such_vlog_first=(X.ILLEGAL_STATE, 0), straddle_end=(X.OK, 1), exact_end=(X.OK, 0))
    for role, (status, trunc) in want.items():
        t = syn.roles[role]
        assert (ex["status"][t - 1], ex["truncated"][t - 1]) == (status, trunc), role
        assert ex["sized"][t - 1] == (status == X.OK), role
    # the last value ends exactly at vLog 2's end_off
    _, ents = st.record(syn.roles["exact_end"])
    vid, at = X.decode_offset(ents[0][3])
    assert vid == 2 and at + ents[0][2] == st.vlogs[1][0] + len(st.vlogs[1][1])
    # a truncated tx carries the stored hVal where the value would be
    h, ents = st.record(syn.roles["id_zero"])
    assert ex["blobs"][syn.roles["id_zero"] - 1] == R.export_tx(h, [(ents[0][1], ents[0][0], ents[0][4])], True)


def test_synthetic_store_replicates(orc, syn):
    """Export -> replicate on the CPU: the reference accepts the store's
    replicable prefix onto an empty tree and refuses the empty tx behind it."""
    r = R.reference(orc, syn.ex["blobs"][:syn.n_clean], orc.AHtree(1), orc.sha256(b""))
    assert r["accepted"] == syn.n_accept == syn.n_clean - 1
    assert r["status"][syn.n_accept] == R.ILLEGAL


def test_digest_failure_keeps_its_range(orc, syn):
    """A flipped value byte: that tx alone is MH_ERR_CORRUPTED_DATA, sized, and
    off[] is the clean run's (off never depends on a hash)"""
    st = syn.store
    t = syn.roles["width_5"]
    _, ents = st.record(t)
    vid, at = X.decode_offset(next(e[3] for e in ents if e[2]))
    v = bytearray(st.vlogs[vid - 1][1])
    v[at - st.vlogs[vid - 1][0]] ^= 1
    vl = list(st.vlogs)
    vl[vid - 1] = (vl[vid - 1][0], bytes(v))
    ex = st.clone(vlogs=vl).expect()
    assert ex["status"][t - 1] == X.CORRUPTED_DATA and ex["sized"][t - 1]
    assert ex["off"].tolist() == syn.ex["off"].tolist()
    assert [k for k in range(st.ntx) if ex["status"][k] != syn.ex["status"][k]] == [t - 1]


# ------------------------------------------------------------------ the C call
def _call(L, ctx, store, first, count, out=None, cap=0, off=True, status=True):
    o = np.full(min(count, 16) + 2, 7, np.uint64)  # (no call here gets as far as writing a result)
    st = np.zeros(min(count, 16) + 1, np.int32)
    rc = L.mh_export_tx_batch(ctx, C.addressof(store) if store is not None else None, first, count, out, cap,
                              o.ctypes.data if off else None, st.ctypes.data if status else None, None)
    return rc, o


def test_argument_errors_without_a_device():
    """Every call-level check of the contract returns its code before any
    device work: the handle is a zeroed buffer (device ordinal 0, never a live
    context), the store's pointers are host memory."""
    from immustore_amd import _native as N
    from immustore_amd.export import _Store, _Vlog
    L = N.load()
    fake = C.create_string_buffer(1 << 16)
    h = C.addressof(fake)
    buf = np.zeros(4096, np.uint8)
    vl = (_Vlog * 128)()
    for v in vl:
        v.data, v.first_off, v.end_off = buf.ctypes.data, 0, 16

    def store(**kw):
        s = _Store()
        s.txlog, s.txlog_len, s.clog, s.ntx = buf.ctypes.data, 1000, buf.ctypes.data, 10
        s.clog_entry_size, s.max_entries, s.max_key_len = 12, 1024, 1024
        s.vlogs, s.nvlogs = C.addressof(vl), 2
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    ILL, NF = N.MH_ERR_ILLEGAL_ARGUMENTS, N.MH_ERR_TX_NOT_FOUND
    good = store()
    rc, o = _call(L, h, good, 3, 0)
    assert rc == N.MH_OK and o[0] == 0 and o[1] == 7  # count == 0
    assert _call(L, None, None, 3, 0)[0] == N.MH_OK
    assert _call(L, None, good, 1, 1)[0] == ILL
    assert _call(L, h, None, 1, 1)[0] == ILL
    assert _call(L, h, good, 1, 1, off=False)[0] == ILL
    assert _call(L, h, good, 1, 1, status=False)[0] == ILL
    assert _call(L, h, good, 1, 1, out=None, cap=8)[0] == ILL
    assert _call(L, h, good, 0, 1)[0] == ILL  # first_tx == 0
    for es in (0, 11, 13, 43, 45):
        assert _call(L, h, store(clog_entry_size=es), 1, 1)[0] == ILL
    assert _call(L, h, store(nvlogs=128), 1, 1)[0] == ILL  # MaxParallelIO
    assert _call(L, h, store(vlogs=None), 1, 1)[0] == ILL
    assert _call(L, h, store(txlog=None), 1, 1)[0] == ILL
    assert _call(L, h, store(clog=None), 1, 1)[0] == ILL
    assert _call(L, h, good, 1, 1 << 31)[0] == ILL  # count >= 2^31
    assert _call(L, h, store(ntx=1 << 40), 1, (1 << 31) - 1)[0] == ILL  # (passes the count: host txlog)
    vl[1].first_off, vl[1].end_off = 9, 8
    assert _call(L, h, good, 1, 1)[0] == ILL  # end_off < first_off
    vl[1].first_off, vl[1].end_off, vl[1].data = 0, 16, None
    assert _call(L, h, good, 1, 1)[0] == ILL  # a non-empty vLog without data
    vl[1].data = buf.ctypes.data + 2
    assert _call(L, h, good, 1, 1)[0] == ILL  # data not 4-byte aligned
    vl[1].data, vl[1].end_off = None, 0  # an empty vLog needs no data
    # the range against ntx: decided before the store is looked at
    assert _call(L, h, good, 11, 1)[0] == NF
    assert _call(L, h, good, 10, 2)[0] == NF
    assert _call(L, h, good, 1, 11)[0] == NF
    assert _call(L, h, store(ntx=0, txlog=None, clog=None), 1, 1)[0] == NF
    assert _call(L, h, good, (1 << 64) - 1, 2)[0] == NF
    # txlog / clog / a vLog not on the context's device (here: host memory)
    assert _call(L, h, good, 1, 10)[0] == ILL
    assert _call(L, h, good, 10, 1)[0] == ILL


def test_symbol_status_strings_and_mirror():
    from immustore_amd import _native as N
    from immustore_amd.export import _Store, _Vlog
    L = N.load()
    assert hasattr(L, "mh_export_tx_batch")
    res, args = N.SIGNATURES["mh_export_tx_batch"]
    assert res is C.c_int and len(args) == 9
    # the header's layout (LP64): three 8-byte fields; 8 8 8 8 4 4 4 (4) 8 4 (4)
    assert C.sizeof(_Vlog) == 24 and C.sizeof(_Store) == 64
    assert (_Store.vlogs.offset, _Store.nvlogs.offset) == (48, 56)
    # no new status code
    assert L.mh_status_string(36) == b"unknown status"
