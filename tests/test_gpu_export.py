"""mh_export_tx_batch on the device against the CPU restatement of
tests/export_util.py: blobs, off, status and truncated byte for byte, out in
pageable, pinned and device memory, and the export fed to
mh_replicate_tx_batch against tests/replicate_util.py's reference."""
import ctypes as C
import threading

import numpy as np
import pytest

import export_util as X
import replicate_util as R
from tx_util import metadata_logs

pytestmark = pytest.mark.gpu
GO_STORES = ["long_linear_proof", "v110_defaultdb", "v110_systemdb"]
CANARY = 0xA5
PAD = 64  # canary bytes on both sides of out


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


def on_device(m, ctx, st):
    return m.ExportStore(st.raw, st.clog, [(f, b) for f, b in st.vlogs], st.es, ctx=ctx,
                         max_entries=st.max_entries)


@pytest.fixture(scope="module")
def stores(m, ctx, orc, fixtures):
    """name -> (ExpStore, its device copy, the whole store's expectation); the
    references are computed once and left unchanged"""
    out = {}
    syn = X.synthetic(orc)
    for name, st in [(n, X.go_store(fixtures[n])) for n in GO_STORES] + [("synthetic", syn.store)]:
        out[name] = (st, on_device(m, ctx, st), st.expect())
    out["_syn"] = syn
    yield out
    for k, v in out.items():
        if k != "_syn":
            v[1].close()


class Out:
    """out of one call: cap bytes between two canary pads, in pageable, pinned
    or device memory, `shift` bytes off the allocation's alignment"""

    def __init__(self, m, ctx, mode, cap, shift=0):
        from immustore_amd import _native as N
        self.L, self.ctx, self.mode, self.cap, self.shift = N.load(), ctx, mode, cap, shift
        self.size = shift + PAD + cap + PAD
        self.host = np.full(self.size, CANARY, np.uint8)
        self.p = C.c_void_p()
        if mode == "pinned":
            N.check(self.L.mh_host_alloc_pinned(self.size, C.byref(self.p)))
            C.memset(self.p.value, CANARY, self.size)
            self.addr = self.p.value + shift + PAD
        elif mode == "device":
            N.check(self.L.mh_dev_alloc(ctx.handle, self.size, C.byref(self.p)))
            N.check(self.L.mh_memcpy_h2d(ctx.handle, self.p.value, self.host.ctypes.data, self.size))
            ctx.synchronize()
            self.addr = self.p.value + shift + PAD
        else:
            self.addr = self.host.ctypes.data + shift + PAD

    def fetch(self):
        """-> (the cap bytes of out, True when both pads still hold the canary)"""
        from immustore_amd import _native as N
        if self.mode == "pinned":
            self.host[:] = np.frombuffer(C.string_at(self.p.value, self.size), np.uint8)
            N.check(self.L.mh_host_free_pinned(self.p.value))
        elif self.mode == "device":
            N.check(self.L.mh_memcpy_d2h(self.ctx.handle, self.host.ctypes.data, self.p.value, self.size))
            self.ctx.synchronize()
            N.check(self.L.mh_dev_free(self.ctx.handle, self.p.value))
        lo = self.shift + PAD
        pads = bool((self.host[:lo] == CANARY).all() and (self.host[lo + self.cap:] == CANARY).all())
        return self.host[lo:lo + self.cap], pads


def export(m, ctx, dev, first, count, mode="pageable", cap=None, shift=0, total=None):
    """one call -> (off, status, truncated, out bytes); asserts the canaries
    around out.  cap None: exactly the run's bytes (total)"""
    o = Out(m, ctx, mode, total if cap is None else cap, shift)
    off, st, tr = m.export.export_tx_batch_raw(dev, first, count, o.addr, o.cap)
    buf, pads = o.fetch()
    assert pads, "bytes outside out were written"
    return off, st, tr, buf


def same(res, ex, what=""):
    """res of export() against the expectation: off, status, truncated, every
    MH_OK blob; every byte of out that no written blob and no tx failing on a
    digest owns still holds the canary"""
    off, st, tr, buf = res
    assert off.tolist() == ex["off"].tolist(), what
    assert st.tolist() == ex["status"].tolist(), what
    assert tr.tolist() == ex["truncated"].tolist(), what
    owned = np.zeros(len(buf), bool)
    for k, blob in enumerate(ex["blobs"]):
        lo, hi = int(off[k]), int(off[k + 1])
        if st[k] == X.OK:
            assert bytes(buf[lo:hi]) == blob, (what, k)
            owned[lo:hi] = True
        elif st[k] == X.CORRUPTED_DATA and ex["sized"][k]:
            owned[lo:min(hi, len(buf))] = True  # contents unspecified
    assert (buf[~owned] == CANARY).all(), what


# ------------------------------------------------------------------ whole stores, ranges
@pytest.mark.parametrize("mode", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("store", GO_STORES + ["synthetic"])
def test_whole_store(m, ctx, stores, store, mode):
    st, dev, ex = stores[store]
    same(export(m, ctx, dev, 1, st.ntx, mode, total=int(ex["off"][-1])), ex, (store, mode))


@pytest.mark.parametrize("store", GO_STORES + ["synthetic"])
def test_ranges(m, ctx, stores, store):
    """first_tx > 1, count == 1 at the head and inside, the last tx alone"""
    st, dev, _ = stores[store]
    n = st.ntx
    for first, count in {(2, n - 1), (1, 1), (max(n // 2, 1), 1), (n, 1), (max(n - 2, 1), min(2, n))}:
        ex = st.expect(first, count)
        same(export(m, ctx, dev, first, count, total=int(ex["off"][-1])), ex, (store, first, count))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_device_out_at_every_alignment(m, ctx, stores, shift):
    """out itself off the dword grid: every destination alignment moves; the
    bytes before out, behind out_cap and between the blobs stay untouched"""
    st, dev, ex = stores["synthetic"]
    same(export(m, ctx, dev, 1, st.ntx, "device", total=int(ex["off"][-1]), shift=shift), ex, shift)


@pytest.fixture
def arm(request, monkeypatch):
    """the value kernels of the calls of this test (MH_EXPORT_ARM is read per call)"""
    monkeypatch.setenv("MH_EXPORT_ARM", request.param)
    return request.param


@pytest.mark.parametrize("arm", ["A", "B"], indirect=True)
@pytest.mark.parametrize("shift", [0, 3])
def test_both_value_arms(m, ctx, stores, arm, shift):
    """The hashing lane's own stores (A) and the hash-only lanes with the copy
    kernel (B): the same bytes, statuses and untouched canaries"""
    st, dev, ex = stores["synthetic"]
    same(export(m, ctx, dev, 1, st.ntx, "device", total=int(ex["off"][-1]), shift=shift), ex, (arm, shift))
    cap = int(ex["off"][11]) - 1
    same(export(m, ctx, dev, 1, st.ntx, "device", cap=cap, shift=shift), st.expect(out_cap=cap), (arm, cap))


@pytest.fixture(scope="module")
def big(orc):
    st = X.big_store(orc)
    return st, st.expect()


@pytest.mark.parametrize("arm", ["A", "B"], indirect=True)
def test_length_class_order(m, ctx, big, arm):
    """16384 entries and more: the lanes take the values bucketed by block
    count, not in input order; one corrupted value in the middle"""
    big, ex = big
    assert sum(len(big.record(t)[1]) for t in range(1, big.ntx + 1)) >= 16384
    assert sorted(set(ex["status"].tolist())) == [X.OK, X.CORRUPTED_DATA]
    dev = on_device(m, ctx, big)
    same(export(m, ctx, dev, 1, big.ntx, "device", total=int(ex["off"][-1]), shift=1), ex, arm)
    dev.close()


def test_more_txs_than_the_offsets_kernel_has_threads(m, ctx, orc):
    """2100 txs: a thread of the one-workgroup offsets kernel owns a run of
    three txs, the last threads none; ranges that start inside a run"""
    st = X.many_store(orc)
    dev = on_device(m, ctx, st)
    for first, count in ((1, st.ntx), (2, 1025), (1000, 1101)):
        ex = st.expect(first, count)
        assert ex["truncated"].any() or count < 97
        same(export(m, ctx, dev, first, count, "device", total=int(ex["off"][-1])), ex, (first, count))
    dev.close()


# ------------------------------------------------------------------ corruption
def _flip_value(st, t, entry, at):
    """a copy of st with byte `at` (negative: from the end) of that value flipped"""
    _, ents = st.record(t)
    vlen, voff = ents[entry][2], ents[entry][3]
    vid, off = X.decode_offset(voff)
    first, data = st.vlogs[vid - 1]
    v = bytearray(data)
    v[off - first + (at if at >= 0 else vlen + at)] ^= 0x10
    vl = list(st.vlogs)
    vl[vid - 1] = (first, bytes(v))
    return st.clone(vlogs=vl)


def _entry_with(st, t, pred):
    return next(i for i, e in enumerate(st.record(t)[1]) if pred(e))


def _against_clean(m, ctx, bad, t, clean_res, want):
    """the mutated store: tx t alone changes to `want`, every other blob is
    byte-equal to the clean run's"""
    dev = on_device(m, ctx, bad)
    ex = bad.expect()
    res = export(m, ctx, dev, 1, bad.ntx, total=int(ex["off"][-1]))
    dev.close()
    same(res, ex, t)
    assert ex["status"][t - 1] == want
    off0, st0, _, buf0 = clean_res
    off, st, _, buf = res
    for k in range(bad.ntx):
        if k != t - 1:
            assert st[k] == st0[k]
            if st[k] == X.OK:
                assert bytes(buf[int(off[k]):int(off[k + 1])]) == bytes(buf0[int(off0[k]):int(off0[k + 1])])


@pytest.fixture(scope="module")
def clean_run(m, ctx, stores):
    st, dev, ex = stores["synthetic"]
    return export(m, ctx, dev, 1, st.ntx, total=int(ex["off"][-1]))


@pytest.mark.parametrize("where", ["first", "last", "block_edge", "second_entry"])
def test_flipped_value_byte(m, ctx, stores, clean_run, where):
    st = stores["synthetic"][0]
    ts = [t for t in range(1, stores["_syn"].n_clean + 1) if any(e[2] >= 129 for e in st.record(t)[1])]
    t = ts[0]
    e = _entry_with(st, t, lambda x: x[2] >= 129)
    if where == "second_entry":  # a value that is not its tx's first: the lowest failing entry
        t = next(t for t in ts if _entry_with(st, t, lambda x: x[2] >= 129) > 0)
        e = _entry_with(st, t, lambda x: x[2] >= 129)
    at = {"first": 0, "last": -1, "block_edge": 64, "second_entry": 63}[where]
    _against_clean(m, ctx, _flip_value(st, t, e, at), t, clean_run, X.CORRUPTED_DATA)


def test_flipped_stored_hval_and_record_byte(m, ctx, stores, clean_run):
    """a flipped hVal (the record then fails its own re-hash) and a flipped key
    byte: the status is what mh_txlog_validate_clog reports for that entry"""
    st = stores["synthetic"][0]
    t = stores["_syn"].roles["width_5"]
    lo, = np.frombuffer(st.clog[(t - 1) * 12:(t - 1) * 12 + 8], ">u8")
    size, = np.frombuffer(st.clog[(t - 1) * 12 + 8:t * 12], ">u4")
    for at in (int(lo) + int(size) - 32 - 1, int(lo) + 100):  # the last entry's hVal; inside the header / first entry
        raw = bytearray(st.raw)
        raw[at] ^= 1
        bad = st.clone(raw=bytes(raw))
        per_tx = m.txlayer.txlog_validate_clog(bad.raw, None, bad.clog, ctx=ctx)[5]
        assert per_tx[t - 1] != X.OK and per_tx.tolist() == bad.rst
        _against_clean(m, ctx, bad, t, clean_run, int(per_tx[t - 1]))


def test_digest_ahead_of_a_missing_vlog_decides(m, ctx, stores, clean_run):
    """entry 0's value corrupted in the tx whose entry 1 names a value log the
    store does not have: Go reads entry 0 first"""
    st = stores["synthetic"][0]
    t = stores["_syn"].roles["no_such_vlog"]
    bad = _flip_value(st, t, 0, 3)
    assert bad.expect()["status"][t - 1] == X.CORRUPTED_DATA and st.expect()["status"][t - 1] == X.ILLEGAL_STATE
    _against_clean(m, ctx, bad, t, clean_run, X.CORRUPTED_DATA)


# ------------------------------------------------------------------ sizing
def test_sizing(m, ctx, stores):
    st, dev, ex = stores["synthetic"]
    n, total = st.ntx, int(ex["off"][-1])
    # out_cap = 0: the same off; what would be written is MH_ERR_BUFFER_TOO_SMALL
    ex0 = st.expect(out_cap=0)
    assert ex0["off"].tolist() == ex["off"].tolist()
    assert set(ex0["status"].tolist()) == {X.BUFFER_TOO_SMALL, X.CORRUPTED_DATA, X.ILLEGAL_STATE}
    same(export(m, ctx, dev, 1, n, cap=0), ex0, "cap 0")
    blobs, status, tr, off = m.export_tx_batch(dev, 1, n)  # the wrapper's two calls
    assert blobs == ex["blobs"] and off[n] == total and status.tolist() == ex["status"].tolist()
    # a cap inside tx j, at its first and at its last byte, and exactly at its end
    for j in (0, 7, stores["_syn"].n_clean - 1, n - 1):
        for cap in (int(ex["off"][j]), int(ex["off"][j + 1]) - 1, int(ex["off"][j + 1])):
            for mode in ("pageable", "device"):
                exc = st.expect(out_cap=cap)
                assert exc["status"][j] == (X.OK if cap == int(ex["off"][j + 1]) else X.BUFFER_TOO_SMALL)
                same(export(m, ctx, dev, 1, n, mode, cap=cap), exc, (j, cap, mode))


# ------------------------------------------------------------------ export -> replicate
def _replicate_same(m, ctx, orc, blobs, P, alhs, what):
    t = m.AHtree(ctx)
    ot = orc.AHtree(max(P, 1))
    for a in alhs[:P]:
        ot.append(a)
    if P:
        t.append_batch(np.frombuffer(b"".join(alhs[:P]), np.uint8).reshape(P, 32))
    prev = alhs[P - 1] if P else orc.sha256(b"")
    ref = R.reference(orc, blobs, ot, prev)
    out = m.replicate_tx_batch(t, blobs, prev)
    assert out["status"].tolist() == ref["status"].tolist(), what
    assert out["accepted"] == ref["accepted"], what
    for name in ("hdrs", "md_blob", "alh", "ents", "hvals"):
        assert out[name].tobytes() == ref[name].tobytes(), (what, name)
    assert t.size() == ref["size"] and t.dlog() == ref["dlog"], what
    t.close()
    return ref


@pytest.mark.parametrize("store", GO_STORES + ["synthetic"])
def test_round_trip(m, ctx, orc, fixtures, stores, store):
    """The device's export into the device's replicate, on an empty tree and on
    one holding a prefix: exactly the reference's outputs; an untruncated store
    is accepted whole and the follower's dLog is the leader's."""
    st, dev, ex = stores[store]
    n = st.ntx
    blobs = m.export_tx_batch(dev, 1, n, size_hint=int(ex["off"][-1]))[0]
    assert blobs == ex["blobs"]
    ref = _replicate_same(m, ctx, orc, blobs, 0, [], store)
    alhs = [bytes(a) for a in ref["alh"]]
    if store in GO_STORES:
        assert ref["accepted"] == n and ref["dlog"] == bytes.fromhex(fixtures[store]["aht_dlog"])
        P = n // 2
    else:
        assert ref["accepted"] == stores["_syn"].n_accept
        P = 9
    ref2 = _replicate_same(m, ctx, orc, blobs[P:], P, alhs, (store, P))
    assert ref2["accepted"] == ref["accepted"] - P and ref2["dlog"] == ref["dlog"]


# ------------------------------------------------------------------ threads, odd records, arguments
def test_two_threads_one_context(m, ctx, stores):
    st, dev, _ = stores["synthetic"]
    half = st.ntx // 2
    jobs = [(1, half), (half + 1, st.ntx - half)]
    exs = [st.expect(f, c) for f, c in jobs]
    res, errs = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                res[i] = export(m, ctx, dev, jobs[i][0], jobs[i][1], total=int(exs[i]["off"][-1]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for i in range(2):
        same(res[i], exs[i], i)


def test_records_the_read_path_takes_to_the_host(m, ctx, orc):
    """A tx of more than 1024 entries, and records whose metadata is valid but
    not canonical: exported like any other, the metadata re-serialised"""
    wide = X.wide_store(orc)
    assert not any(wide.rst)
    dev = on_device(m, ctx, wide)
    ex = wide.expect()
    assert not ex["status"].any()
    same(export(m, ctx, dev, 1, 3, total=int(ex["off"][-1])), ex, "wide")
    dev.close()
    raw = next(r for n, r in metadata_logs(orc) if n == "noncanonical_sealed_canonical")
    nc = X.log_store(raw, [(0, bytes(100))])
    assert not any(nc.rst)
    ex = nc.expect()
    assert not ex["status"].any() and ex["truncated"].all()  # (vOff 77 with id 0: hVal only)
    stored = {bytes(e[0]) for t in range(1, nc.ntx + 1) for e in nc.record(t)[1]}
    assert b"\x00\x02" in stored and b"\x02\x00" not in stored
    dev = on_device(m, ctx, nc)
    same(export(m, ctx, dev, 1, nc.ntx, total=int(ex["off"][-1])), ex, "noncanonical")
    dev.close()


def test_argument_errors_on_the_device(m, ctx, stores):
    from immustore_amd import _native as N
    st, dev, ex = stores["long_linear_proof"]
    L = N.load()
    off = np.zeros(st.ntx + 1, np.uint64)
    status = np.zeros(st.ntx, np.int32)
    out = np.zeros(int(ex["off"][-1]), np.uint8)

    def call(s, first=1, count=st.ntx):
        return L.mh_export_tx_batch(ctx.handle, C.addressof(s), first, count, out.ctypes.data, len(out),
                                    off.ctypes.data, status.ctypes.data, None)

    assert call(dev.descriptor()) == N.MH_OK and status.tolist() == ex["status"].tolist()
    assert call(dev.descriptor(), st.ntx, 2) == N.MH_ERR_TX_NOT_FOUND
    assert call(dev.descriptor(), st.ntx + 1, 1) == N.MH_ERR_TX_NOT_FOUND
    host = np.frombuffer(st.raw, np.uint8).copy()
    s = dev.descriptor()
    s.txlog = host.ctypes.data
    assert call(s) == N.MH_ERR_ILLEGAL_ARGUMENTS  # the tx log in host memory
    s = dev.descriptor()
    s.clog = host.ctypes.data
    assert call(s) == N.MH_ERR_ILLEGAL_ARGUMENTS
    s = dev.descriptor()
    s.txlog_len += 1 << 20  # the slack is not there
    assert call(s) == N.MH_ERR_ILLEGAL_ARGUMENTS
    s = dev.descriptor()
    vl = (m.export._Vlog * 1)()
    vl[0].data, vl[0].first_off, vl[0].end_off = host.ctypes.data, 0, 16
    s.vlogs = C.addressof(vl)
    assert call(s) == N.MH_ERR_ILLEGAL_ARGUMENTS  # a value log in host memory
    vl[0].data, vl[0].end_off = dev._vl[0].data, dev._vl[0].end_off + (1 << 20)
    assert call(s) == N.MH_ERR_ILLEGAL_ARGUMENTS  # its slack is not there
    assert call(dev.descriptor()) == N.MH_OK
