"""What handles and contexts carry from one call to the next: one mh_ahtree
over resets and re-appends, one mh_htree rebuilt wide -> narrow through every
build form, one mh_ctx whose scratch serves many entry points in turn, and
asynchronous chains checked stage by stage after a single sync.

Every expectation is the oracle's on the logical input of that step alone
(tests/call_sequence_util.py); nothing is compared with an earlier result of
the library.  Where a step fails, the message names the step, the call and
what came before it, and says what the same call gives on a fresh handle: a
plain wrong answer fails there too, a carried-over one does not.
"""
import numpy as np
import pytest

import call_sequence_util as U
from call_sequence_util import first_diff as _first_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import torch  # noqa: F401  (load the HIP runtime the way the bench does)
    import immustore_amd as m
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


# ============================================================ A: one mh_ahtree
def _apply(t, step, p):
    """One step on a handle -> (roots bytes or None, plog, clog)."""
    op = step["op"]
    if op == "reset":
        t.reset_size(step["to"])
        return None, None, None
    if op == "append":
        n, h = t.append(p[0].tobytes())
        assert n == step["n0"] + 1, ("append returned n", n, step)
        return h, None, None
    if op == "batch":
        t.append_batch(p)
        return None, None, None
    if op == "batch_roots":
        return t.append_batch(p, with_roots=True).tobytes(), None, None
    plog, clog = t.append_batch_logs(p, step["p_off0"])
    return None, plog, clog


def _fresh_dlog(m, ctx, segs):
    """The same logical tree on a fresh handle, for the messages."""
    t = m.AHtree(ctx)
    for s in segs:
        if s.shape[0]:
            t.append_batch(s)
    d = t.dlog()
    t.close()
    return d


def test_ahtree_life_vs_oracle(m, orc):
    """One handle through the 28 steps of call_sequence_util.ahtree_steps():
    append / append_batch with and without roots / append_batch_logs,
    reset_size to 0, 1, 2^11 - 1, 2^11, 2^11 + 1, size - 1 and size, re-appends
    of other payloads that end before, on and past the old size, one that
    makes aht_reserve move the dLog, payloads of 32, 50, 1 and 0 bytes.  After
    every step: size, the whole dLog, the root, the batch's roots, the
    pLog / cLog records, about 16 proof rows of each kind and three rows with
    j = size + 1, j = the largest size the handle has had and j = the size just
    before the latest reset (status the oracle's; no term a node of the part cut
    off; the context is this test's own, so that what its proof scratch holds
    comes from these calls alone).  Oracle cost: 28 fresh trees of <= 5200
    leaves, 0.15 s."""
    steps = U.ahtree_steps()
    model = U.ahtree_model(orc, steps)
    ctx = m.Context(0)
    t = m.AHtree(ctx)
    segs, before = [], "new handle"
    for k, (s, e) in enumerate(zip(steps, model)):
        p = None if s["op"] == "reset" else U.payloads(orc, s)
        segs = U.truncate(segs, s["to"]) if p is None else segs + [p]
        where = "step %d %r after %s" % (k, {x: s[x] for x in s if x != "seed"}, before)
        roots, plog, clog = _apply(t, s, p)
        assert t.size() == e["size"], where
        got = t.dlog()
        if got != e["dlog"]:
            d = _first_diff(got, e["dlog"])
            fresh = _first_diff(_fresh_dlog(m, ctx, segs), e["dlog"])
            pytest.fail("%s: dLog differs from the oracle's at node %r (nodes_upto(n0) = %d); a "
                        "fresh handle fed the same payloads differs at %r"
                        % (where, d, U.nodes_upto(min(s["n0"], e["size"])), fresh))
        if e["size"]:
            assert t.root() == (e["size"], e["root"]), where
            assert t.root_at(e["size"]) == e["root"], where
        else:
            with pytest.raises(m.ErrEmptyTree):
                t.root()
        if e["roots"] is not None:
            assert roots == e["roots"], (where, "roots_out", _first_diff(roots, e["roots"]))
        if s["op"] == "logs":
            assert plog == e["plog"], (where, "pLog", _first_diff(plog, e["plog"], 4 + s["plen"]))
            assert clog == e["clog"], (where, "cLog", _first_diff(clog, e["clog"], 12))
        I, J = U.proof_rows(e["size"], [e["size"] + 1, s["hi"], s["cut"]], k)
        for kind in (0, 1):
            terms, nt, st = t.proof_batch(kind, I, J, max_terms=64)
            ot, ont, ost = e["oracle"].proof_batch(kind, I, J, cap=64)
            for r in range(len(I)):
                row = (where, "proof_batch kind %d" % kind, int(I[r]), int(J[r]))
                assert st[r] == ost[r], row + ("status", int(st[r]), int(ost[r]))
                if ost[r] == 0:
                    assert nt[r] == ont[r] and terms[r, :nt[r]].tobytes() == \
                        ot[r, :ont[r]].tobytes(), row
                else:
                    assert nt[r] == ont[r] == 0, row + ("terms on a failed row", int(nt[r]))
                # nothing the call hands back, past a row's terms either, is a
                # node that the reset removed
                leaked = [x for x in range(64) if terms[r, x].tobytes() in e["stale"]]
                assert not leaked, row + ("terms that are nodes of the part cut off", leaked)
        before = "%s(%s)" % (s["op"], s.get("m", s.get("to")))
    t.close()
    ctx.close()


@pytest.fixture(scope="module")
def aht_big(orc):
    return U.ahtree_big_model(orc)


def test_ahtree_table_kernels_over_stale_dlog(m, ctx, aht_big):
    """(1 << 19) + 5 appends, reset_size(3), as many other payloads in one
    batch: k_aht_perfect_t and k_aht_spine_pairs over a dLog full of plausible
    nodes of the first run.  The whole dLog and the last root.  Oracle cost:
    one tree of 2^19 + 8 leaves, 1.4 s, made once."""
    a, b, odlog, oroot = aht_big
    t = m.AHtree(ctx)
    t.append_batch(a)
    assert t.size() == U.AHT_BIG
    t.reset_size(3)
    roots = t.append_batch(b, with_roots=True)
    assert t.size() == U.AHT_BIG + 3
    got = t.dlog()
    if got != odlog:
        d = _first_diff(got, odlog)
        t2 = m.AHtree(ctx)
        t2.append_batch(a[:3])
        t2.append_batch(b)
        fresh = _first_diff(t2.dlog(), odlog)
        t2.close()
        pytest.fail("append_batch of 2^19 + 5 after reset_size(3) of a 2^19 + 5 tree: dLog differs "
                    "at node %r; a fresh handle differs at %r" % (d, fresh))
    assert roots[-1].tobytes() == oroot and t.root() == (U.AHT_BIG + 3, oroot)
    t.close()


def _replicate_same(out, ref, t, what):
    assert out["status"].tolist() == ref["status"].tolist(), (what, "verdicts")
    assert out["accepted"] == ref["accepted"], (what, "accepted")
    assert out["ent_off"].tolist() == ref["ent_off"].tolist(), (what, "ent_off")
    for name in ("hdrs", "md_blob", "alh", "ents", "hvals"):
        assert out[name].tobytes() == ref[name].tobytes(), (what, name)
    assert t.size() == ref["size"], (what, "size")
    assert t.dlog() == ref["dlog"], (what, "dLog", _first_diff(t.dlog(), ref["dlog"]))
    if ref["size"]:
        assert t.root()[1] == ref["dlog"][-32:], (what, "root")


def test_replicate_again_after_rollback(m, ctx, orc):
    """The follower's rollback: a run of 40 txs replicated onto one handle,
    reset_size(P) for a P inside the accepted prefix, txs P + 1.. replicated
    again -- the same txs, and those of a second store that shares the first P
    txs and differs after them -- each identical to replicate_util.reference
    on a tree of P leaves: verdicts, accepted count, dLog and root.  Oracle
    cost: two stores of 40 two-entry txs and three reference runs, 0.1 s."""
    import replicate_util as R
    n, P = 40, 13
    specs = R.simple_specs(n, seed=31)
    other = specs[:P] + R.simple_specs(n - P, seed=32)
    txs, trees = R.synthetic_store(orc, specs, bl_of=lambda i: [i - 1, i // 2, 0][i % 3])
    txs2, trees2 = R.synthetic_store(orc, other, bl_of=lambda i: [i - 1, i // 2, 0][i % 3])
    assert [x["alh"] for x in txs[:P]] == [x["alh"] for x in txs2[:P]]
    assert txs[P]["alh"] != txs2[P]["alh"]
    empty = orc.sha256(b"")
    t = m.AHtree(ctx)
    kw = R.Limits().kw()
    out = m.replicate_tx_batch(t, [x["blob"] for x in txs], empty, **kw)
    ref = R.reference(orc, [x["blob"] for x in txs], trees[0], empty)
    assert ref["accepted"] == n
    _replicate_same(out, ref, t, "first run of %d txs on a new handle" % n)
    for name, store, tr in (("the same txs", txs, trees), ("another store's txs", txs2, trees2),
                            ("the first store's txs again", txs, trees)):
        what = "reset_size(%d) then replicate %s, after a run that reached %d" % (P, name, t.size())
        t.reset_size(P)
        blobs = [x["blob"] for x in store[P:]]
        # one tx of the batch is broken: the verdicts behind it too
        blobs[20] = R._hdr_edit(store[P + 20], bl_root=bytes(31) + b"\x01")
        prev = R.prev_alh_of(orc, store, P)
        ref = R.reference(orc, blobs, tr[P], prev)
        assert ref["accepted"] == 20
        out = m.replicate_tx_batch(t, blobs, prev, **kw)
        _replicate_same(out, ref, t, what)
        blobs = [x["blob"] for x in store[P + 20:]]
        ref = R.reference(orc, blobs, tr[P + 20], R.prev_alh_of(orc, store, P + 20))
        out = m.replicate_tx_batch(t, blobs, R.prev_alh_of(orc, store, P + 20), **kw)
        assert ref["accepted"] == n - P - 20
        _replicate_same(out, ref, t, what + ", then the rest")
    t.close()


# ============================================================= B: one mh_htree
def _ht_build(t, inp):
    if inp["form"] == "with":
        t.build_with(inp["digests"])
        return None
    return t.build_entries(inp["version"], inp["keys"], inp["vals_sent"], inp["mds"],
                           inp["overrides"])


def _ht_check(m, orc, wire, t, n, exp, prev_n, seed, where, ctx, inp, gone=frozenset()):
    """gone: the nodes of the build before this one that this one does not have"""
    ohv, olv, oroot = exp
    assert t.width == n, (where, "width", t.width)
    assert t.root() == oroot, (where, "root")
    lv = t.levels()
    assert lv.shape[0] == m.levels_len(n) == olv.shape[0], (where, "levels_len")
    if lv.tobytes() != olv.tobytes():
        f = m.HTree(U.HT_MAX_WIDTH, ctx)
        _ht_build(f, inp)
        fresh = _first_diff(f.levels().tobytes(), olv.tobytes())
        f.close()
        pytest.fail("%s: levels differ at node %r; a fresh handle differs at %r"
                    % (where, _first_diff(lv.tobytes(), olv.tobytes()), fresh))
    leaves = U.htree_leaves(n, prev_n, seed)
    terms, nt, st = t.inclusion_proof_batch(leaves)
    for r, leaf in enumerate(leaves):
        est, et = U.htree_proof_expect(orc, olv, n, int(leaf))
        row = (where, "inclusion_proof_batch leaf", int(leaf))
        assert st[r] == est, row + ("status", int(st[r]), est)
        if est == 0:
            assert terms[r, :nt[r]].tobytes() == et, row
        else:
            assert nt[r] == 0, row + ("terms on a refused row", int(nt[r]))
        leaked = [x for x in range(terms.shape[1]) if terms[r, x].tobytes() in gone]
        assert not leaked, row + ("terms that are nodes of the build before", leaked)
    few = np.array(sorted({0, n // 2, max(n, 1) - 1}) + [n, prev_n], np.uint64)
    msgs, st = t.inclusion_proof_pb_batch(few)
    for r, leaf in enumerate(few):
        est, eb = wire.htree_inclusion_proof_pb(olv, n, int(leaf))
        assert st[r] == est and msgs[r] == (eb if est == 0 else b""), \
            (where, "inclusion_proof_pb_batch leaf", int(leaf), int(st[r]), est)


def _ht_fail(m, t, kind, status):
    from immustore_amd import _native as N
    L = N.load()
    if kind == "max_width":
        with pytest.raises(m.ErrMaxWidthExceeded):
            t.build_with(np.zeros((U.HT_MAX_WIDTH + 1, 32), np.uint8))
        n = U.HT_MAX_WIDTH + 1
        off = np.arange(n + 1, dtype=np.uint64)
        buf = np.zeros(n + 16, np.uint8)
        st = L.mh_htree_build_entries(t.handle, 1, n, buf.ctypes.data, off.ctypes.data, None, None,
                                      buf.ctypes.data, off.ctypes.data, None, None, None)
    elif kind == "v0_metadata":
        keys = np.frombuffer(b"abcdefgh", np.uint8).copy()
        off = np.array([0, 4, 8], np.uint64)
        st = L.mh_htree_build_entries(t.handle, 0, 2, keys.ctypes.data, off.ctypes.data,
                                      keys.ctypes.data, off.ctypes.data, keys.ctypes.data,
                                      off.ctypes.data, None, None, None)
    else:
        keys = np.frombuffer(b"abcdefgh", np.uint8).copy()
        ko = np.array([0, 4, 2, 8], np.uint64)   # entry 1 runs backwards
        vo = np.array([0, 1, 2, 3], np.uint64)
        st = L.mh_htree_build_entries(t.handle, 1, 3, keys.ctypes.data, ko.ctypes.data, None, None,
                                      keys.ctypes.data, vo.ctypes.data, None, None, None)
    assert st == status, (kind, st, status)


def test_htree_life_vs_oracle(m, ctx, orc):
    """One handle of max_width 16391 through the 31 builds of
    call_sequence_util.htree_builds(): build_with, the fused fixed path, the
    CSR path with KV metadata / with hVal overrides / with neither, and v0,
    each form followed by each other, the widths 4096, 3, 0, 1, 257, 2, 4095,
    16391 (sorted), 5, 1000 in turn, other data in every build.  After each:
    root, width, exactly levels_len(width) levels, hvals_out, inclusion proofs
    (all leaves up to 257, else 66) with leaf = width and leaf = the previous
    width (a refused row has no terms, and no row hands back a node of the
    build before), and InclusionProof messages.  Then a call that must fail (n >
    max_width, v0 with metadata, a key offset running backwards), after which
    all of that is still the last good build's.  Oracle cost: 31 builds of
    <= 16391 entries, 0.2 s."""
    import wire
    builds = U.htree_builds()
    t = m.HTree(U.HT_MAX_WIDTH, ctx)
    prev_n, before, prev_nodes = 0, "new handle", set()
    for k, b in enumerate(builds):
        inp = U.htree_inputs(orc, b)
        exp = U.htree_expect(orc, inp)
        nodes = {x.tobytes() for x in exp[1]}
        gone = prev_nodes - nodes
        n = b["n"]
        where = "build %d %s(n=%d) after %s" % (k, b["form"], n, before)
        hv = _ht_build(t, inp)
        if exp[0] is not None:
            assert hv.tobytes() == exp[0].tobytes(), \
                (where, "hvals_out", _first_diff(hv.tobytes(), exp[0].tobytes()))
        _ht_check(m, orc, wire, t, n, exp, prev_n, b["seed"], where, ctx, inp, gone)
        kind, status = U.HT_FAILURES[k % len(U.HT_FAILURES)]
        _ht_fail(m, t, kind, status)
        _ht_check(m, orc, wire, t, n, exp, prev_n, b["seed"] + 1,
                  where + ", then a %s call that failed" % kind, ctx, inp, gone)
        prev_n, before, prev_nodes = n, "%s(n=%d)" % (b["form"], n), nodes
    t.close()


# ================================================== D: asynchronous chains, one sync
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _poison(torch, nbytes):
    return torch.full((max(int(nbytes), 1),), 0xA5, dtype=torch.uint8, device="cuda")


def _host(tensor, dtype=np.uint8):
    return tensor.cpu().numpy().view(dtype)


class _cur_ctx:
    """A context created on torch.cuda.current_stream(), as the bench makes
    its own (chains 1-3 share one), with a non-default stream current for the
    life of it: torch's
    default stream has the handle 0, for which mh_ctx_create makes a stream of
    its own, and the torch copies and gathers inside a chain would then not
    be ordered with the library's launches."""

    def __init__(self, m, torch):
        self.torch = torch
        self.old = torch.cuda.current_stream()
        torch.cuda.set_stream(torch.cuda.Stream())
        handle = torch.cuda.current_stream().cuda_stream
        assert handle != 0
        self.c = m.Context(0, handle)
        assert self.c.stream == handle
        self.handle = self.c.handle

    def __getattr__(self, name):
        return getattr(self.c, name)

    def close(self):
        self.torch.cuda.synchronize()
        self.c.close()
        self.torch.cuda.set_stream(self.old)


@pytest.fixture(scope="module")
def chain_ctx(m):
    """The one context of chains 1-3: its scratch (s_sort, s_offs, s_ctr,
    s_edge) goes from one chain to the next."""
    import torch
    c = _cur_ctx(m, torch)
    yield c
    c.close()


def test_chain_htree_build_verify_prove_no_sync(m, orc, chain_ctx):
    """fill_random -> build_entries_fixed with hvals_out -> verify_values over
    those values and hVals -> inclusion_proof_batch from those levels ->
    verify_inclusion_batch of those proofs, n = 1025 x 128 B, queued on the
    torch stream with no host sync in between; after one sync every buffer of
    every stage equals the oracle's (one stored length and one digest are
    wrong on purpose, so both verifiers have a failing row).  Oracle cost: one
    1025-entry build and 1025 proofs, 10 ms."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    n, vlen, seed = 1025, 128, 77
    c = chain_ctx
    try:
        keys = np.frombuffer(np.arange(n, dtype=">u8").tobytes(), np.uint8).reshape(n, 8)
        ovals = orc.fill_random(n * vlen, seed).reshape(n, vlen)
        ohv, olv, oroot = orc.build_entries_fixed(1, keys, ovals)
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(vlen)
        stored_len = np.full(n, vlen, np.uint64)
        stored_len[5] = vlen - 1
        obad, ovst = orc.verify_values(ovals.reshape(-1), off, ohv, stored_len)
        assert obad == 1 and ovst[5] == 14
        # every leaf: all of 0..1023 have 11 terms, leaf 1024 (kept last) has one,
        # so the strided rows of the proof call are a CSR list as they stand
        leaves = np.arange(n, dtype=np.uint64)
        mt = 11
        oterms = [orc.htree_inclusion_proof(olv, n, int(i))[1] for i in leaves]
        assert [len(x) for x in oterms] == [mt] * (n - 1) + [1]
        term_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(mt)
        term_off[n] = term_off[n - 1] + np.uint64(1)
        digs = np.stack([np.frombuffer(orc.entry_digest(1, keys[i].tobytes(), b"", ohv[i].tobytes())[1],
                                       np.uint8) for i in range(n)])
        digs[700, 3] ^= 1
        widths = np.full(n, n, np.uint64)
        flat = np.zeros((n * mt, 32), np.uint8)
        for i, x in enumerate(oterms):
            flat[i * mt:i * mt + len(x)] = x
        _, ook = orc.htree_verify_csr(leaves, widths, term_off, flat, digs,
                                      np.tile(np.frombuffer(oroot, np.uint8), (n, 1)))
        assert ook.sum() == n - 1 and not ook[700]

        dk, doff, dvl = _dev(torch, keys), _dev(torch, off), _dev(torch, stored_len)
        dleaf, dw, dto, ddig = (_dev(torch, leaves), _dev(torch, widths), _dev(torch, term_off),
                                _dev(torch, digs))
        dv, dhv = _poison(torch, n * vlen), _poison(torch, n * 32)
        dlv, drt = _poison(torch, m.levels_len(n) * 32), _poison(torch, 32)
        dvst = _poison(torch, n * 4)
        dterms, dnt, dpst = _poison(torch, n * mt * 32), _poison(torch, n * 4), _poison(torch, n * 4)
        dok = _poison(torch, n)
        torch.cuda.synchronize()
        h = c.handle
        N.check(L.mh_dev_fill_random(h, dv.data_ptr(), n * vlen, seed))
        N.check(L.mh_dev_htree_build_entries_fixed(h, 1, n, dk.data_ptr(), 8, dv.data_ptr(), vlen,
                                                   dhv.data_ptr(), dlv.data_ptr(), drt.data_ptr()))
        N.check(L.mh_dev_verify_values_batch(h, n, dv.data_ptr(), doff.data_ptr(), dvl.data_ptr(),
                                             dhv.data_ptr(), dvst.data_ptr()))
        N.check(L.mh_dev_htree_inclusion_proof_batch(h, dlv.data_ptr(), n, n, dleaf.data_ptr(),
                                                     dterms.data_ptr(), mt, dnt.data_ptr(),
                                                     dpst.data_ptr()))
        droots = drt.view(1, 32).expand(n, 32).contiguous()   # on the same stream
        N.check(L.mh_dev_htree_verify_inclusion_batch(h, n, dleaf.data_ptr(), dw.data_ptr(),
                                                      dto.data_ptr(), dterms.data_ptr(),
                                                      ddig.data_ptr(), droots.data_ptr(),
                                                      dok.data_ptr()))
        c.synchronize()
        assert _host(dv).tobytes() == ovals.tobytes(), "stage 1 fill_random"
        for name, got, want in (("hvals_out", dhv, ohv), ("levels", dlv, olv)):
            g, w = _host(got).tobytes(), want.tobytes()
            assert g == w, ("stage 2 build_entries_fixed after fill_random", name, _first_diff(g, w))
        assert _host(drt).tobytes() == oroot, "stage 2 root"
        assert _host(dvst, np.int32).tolist() == ovst.tolist(), "stage 3 verify_values after the build"
        nt, pst = _host(dnt, np.uint32), _host(dpst, np.int32)
        assert not pst.any() and nt.tolist() == [mt] * (n - 1) + [1], "stage 4 proof statuses"
        gt = _host(dterms).reshape(n, mt, 32)
        for i in range(n):
            assert gt[i, :nt[i]].tobytes() == oterms[i].tobytes(), \
                ("stage 4 inclusion_proof_batch after verify_values", i)
        assert _host(dok).tolist() == ook.tolist(), "stage 5 verify_inclusion_batch of those proofs"
    finally:
        torch.cuda.synchronize()   # the context lives on for the next chain


def test_chain_ahtree_append_twice_prove_verify_no_sync(m, orc, chain_ctx):
    """mh_dev_ahtree_append_batch at n0 = 0 (m = 300) -> a second one onto the
    same dLog at n0 = 300 (m = 1000; the context's spine counter used twice) ->
    mh_dev_ahtree_proof_batch of both kinds -> mh_dev_ahtree_verify_batch of
    those proofs with eval_out, no host sync in between.  The dLog, both
    batches' roots, every proof and every verdict / evaluation against the
    oracle.  Oracle cost: a 1300-leaf tree and 2 x 64 proofs, 5 ms."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    m1, m2 = 300, 1000
    size = m1 + m2
    c = chain_ctx
    try:
        pay = orc.fill_random(size * 32, 41).reshape(size, 32)
        o = orc.AHtree(size)
        o.append_batch(pay)
        odlog = o.dlog_bytes()
        oroots = b"".join(o.root_at(k)[1] for k in range(1, size + 1))
        rng = np.random.default_rng(42)
        J = np.concatenate([rng.integers(1, size + 1, 60), [1, m1, m1 + 1, size]]).astype(np.uint64)
        I = np.array([int(rng.integers(1, j + 1)) for j in J], np.uint64)
        I[-1] = size
        nrow, mt = len(I), 24
        dp = _dev(torch, pay)
        dI, dJ = _dev(torch, I), _dev(torch, J)
        ddlog = _poison(torch, U.nodes_upto(size) * 32)
        droots = _poison(torch, size * 32)
        h = c.handle
        stages = {}
        for kind in (0, 1):
            ot, ont, ost = o.proof_batch(kind, I, J, cap=mt)
            assert not ost.any()
            toff = np.zeros(nrow + 1, np.uint64)
            toff[1:] = np.cumsum(ont.astype(np.uint64))
            # where term k of row r lies in the strided output: a gather list
            gidx = np.concatenate([r * mt + np.arange(ont[r]) for r in range(nrow)]).astype(np.int64)
            flat = np.concatenate([ot[r, :ont[r]] for r in range(nrow)])
            leaf_idx = np.array([orc.nodes_until(int(i)) for i in I], np.int64)
            a_idx = leaf_idx if kind == 0 else None
            a = np.stack([np.frombuffer(odlog[32 * x:32 * x + 32], np.uint8) for x in leaf_idx]) \
                if kind == 0 else np.stack([np.frombuffer(o.root_at(int(i))[1], np.uint8) for i in I])
            b = np.stack([np.frombuffer(o.root_at(int(j))[1], np.uint8) for j in J])
            _, ook = orc.ahtree_verify_batch(kind, I, J, toff, flat, a, b)
            oev, odef = orc.ahtree_eval_batch(kind, I, J, toff, flat, a)
            assert ook.all() and odef.sum() >= nrow - 2
            stages[kind] = dict(ot=ot, ont=ont, ook=ook, oev=oev, odef=odef, dtoff=_dev(torch, toff),
                                dgidx=torch.from_numpy(gidx).cuda(),
                                da_idx=None if a_idx is None else torch.from_numpy(a_idx).cuda(),
                                dterms=_poison(torch, nrow * mt * 32), dnt=_poison(torch, nrow * 4),
                                dst=_poison(torch, nrow * 4), dok=_poison(torch, nrow),
                                dev=_poison(torch, nrow * (64 if kind else 32)))
        dIm1 = torch.from_numpy((I - 1).astype(np.int64)).cuda()
        dJm1 = torch.from_numpy((J - 1).astype(np.int64)).cuda()
        torch.cuda.synchronize()
        N.check(L.mh_dev_ahtree_append_batch(h, ddlog.data_ptr(), 0, dp.data_ptr(), m1, 32,
                                             droots.data_ptr()))
        N.check(L.mh_dev_ahtree_append_batch(h, ddlog.data_ptr(), m1, dp.data_ptr() + m1 * 32, m2, 32,
                                             droots.data_ptr() + m1 * 32))
        keep = []
        for kind in (0, 1):
            s = stages[kind]
            N.check(L.mh_dev_ahtree_proof_batch(h, kind, ddlog.data_ptr(), size, nrow, dI.data_ptr(),
                                                dJ.data_ptr(), s["dterms"].data_ptr(), mt,
                                                s["dnt"].data_ptr(), s["dst"].data_ptr()))
            # CSR terms, a and b gathered on the same stream from the chain's own outputs
            flat = torch.index_select(s["dterms"].view(-1, 32), 0, s["dgidx"]).contiguous()
            rv = droots.view(-1, 32)
            da = (torch.index_select(ddlog.view(-1, 32), 0, s["da_idx"]) if kind == 0
                  else torch.index_select(rv, 0, dIm1)).contiguous()
            db = torch.index_select(rv, 0, dJm1).contiguous()
            keep += [flat, da, db]
            N.check(L.mh_dev_ahtree_verify_batch(h, kind, nrow, dI.data_ptr(), dJ.data_ptr(),
                                                 s["dtoff"].data_ptr(), flat.data_ptr(),
                                                 da.data_ptr(), db.data_ptr(), s["dok"].data_ptr(),
                                                 s["dev"].data_ptr()))
        c.synchronize()
        g = _host(ddlog).tobytes()
        assert g == odlog, ("append_batch(n0=0, m=300) then append_batch(n0=300, m=1000): dLog node",
                            _first_diff(g, odlog), "nodes_upto(300) = %d" % U.nodes_upto(m1))
        g = _host(droots).tobytes()
        assert g == oroots, ("roots_out of the two appends", _first_diff(g, oroots), "second from", m1)
        for kind in (0, 1):
            s = stages[kind]
            what = "proof_batch kind %d after the two appends" % kind
            assert not _host(s["dst"], np.int32).any(), what
            nt = _host(s["dnt"], np.uint32)
            assert nt.tolist() == s["ont"].tolist(), what
            gt = _host(s["dterms"]).reshape(nrow, mt, 32)
            for r in range(nrow):
                assert gt[r, :nt[r]].tobytes() == s["ot"][r, :nt[r]].tobytes(), \
                    (what, int(I[r]), int(J[r]))
            assert _host(s["dok"]).astype(bool).tolist() == s["ook"].astype(bool).tolist(), \
                "verify_batch kind %d of those proofs" % kind
            # rows where Go's Eval* is defined (not an empty consistency proof)
            ev = _host(s["dev"]).reshape(nrow, -1)[s["odef"]].tobytes()
            want = s["oev"][s["odef"]].tobytes()
            assert ev == want, ("eval_out kind %d" % kind, _first_diff(ev, want))
    finally:
        torch.cuda.synchronize()   # the context lives on for the next chain


@pytest.fixture(scope="module")
def queued_cases(orc):
    """Per n of QUEUED_BUILD_NS: CSR inputs (ragged keys and values) and the
    oracle's hVals, levels and root."""
    out = []
    for k, n in enumerate(U.QUEUED_BUILD_NS):
        rng = np.random.default_rng(900 + k)
        ko = np.zeros(n + 1, np.uint64)
        vo = np.zeros(n + 1, np.uint64)
        ko[1:] = np.cumsum(rng.integers(1, 40, n))
        vo[1:] = np.cumsum(rng.integers(0, 300, n))
        kb = orc.fill_random(int(ko[n]) + 16, 2 * k + 1)
        vb = orc.fill_random(int(vo[n]) + 16, 2 * k + 2)
        st, hv, lv, root = orc.build_entries_csr(1, kb, ko, None, None, vb, vo)
        assert st == 0
        out.append((n, kb, ko, vb, vo, hv.tobytes(), lv.tobytes(), root))
    return out


@pytest.mark.parametrize("timing", [False, True])
def test_queued_builds_every_output(m, orc, queued_cases, timing, chain_ctx):
    """Twelve mh_dev_htree_build_entries queued back to back on one context,
    n = 1 -> 20000 -> 3 across the sort threshold both ways, each into its own
    poisoned outputs, once with per-kernel timing on: after one sync every
    root, level array and hvals_out equals the oracle's.  Oracle cost: twelve
    builds of <= 20000 entries, 0.1 s, made once."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    c = chain_ctx
    try:
        c.set_timing(timing)
        jobs = []
        for (n, kb, ko, vb, vo, ohv, olv, oroot) in queued_cases:
            jobs.append((n, _dev(torch, kb), _dev(torch, ko), _dev(torch, vb), _dev(torch, vo),
                         _poison(torch, n * 32), _poison(torch, m.levels_len(n) * 32),
                         _poison(torch, 32)))
        torch.cuda.synchronize()
        for (n, kb, ko, vb, vo, hv, lv, rt) in jobs:
            N.check(L.mh_dev_htree_build_entries(c.handle, 1, n, kb.data_ptr(), ko.data_ptr(), None,
                                                 None, vb.data_ptr(), vo.data_ptr(), None, None,
                                                 hv.data_ptr(), lv.data_ptr(), rt.data_ptr()))
        c.synchronize()
        prev = "nothing"
        for k, ((n, _, _, _, _, hv, lv, rt), case) in enumerate(zip(jobs, queued_cases)):
            where = "queued build %d (n=%d, timing %s) after %s" % (k, n, timing, prev)
            ohv, olv, oroot = case[5:]
            assert _host(rt).tobytes() == oroot, (where, "root")
            g = _host(lv).tobytes()[:len(olv)]
            assert g == olv, (where, "levels", _first_diff(g, olv))
            g = _host(hv).tobytes()[:len(ohv)]
            assert g == ohv, (where, "hvals_out", _first_diff(g, ohv))
            prev = "n=%d" % n
        if timing:
            ms, launches = c.timing()
            assert launches > 0 and ms > 0
    finally:
        c.set_timing(False)
        torch.cuda.synchronize()


def test_three_streams_two_builds_each_then_reduce(m, orc):
    """Three contexts on three non-default torch streams, each queueing two
    fixed builds of different n into the same level buffer and its third of
    one root array; a fourth context on a fourth stream waits on events
    recorded behind each context's second build and reduces the three roots
    (mh_dev_htree_reduce_nodes).  The second builds' levels, the three roots
    and the reduction against the oracle.  Oracle cost: six builds of <= 3000
    entries, 20 ms."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    streams = [torch.cuda.Stream() for _ in range(4)]
    ctxs = [m.Context(0, s.cuda_stream) for s in streams]
    try:
        roots = _poison(torch, 96)
        jobs = []
        for k in range(3):
            pair = []
            for n, seed in ((3000 + k, 70 + k), (1000 + 7 * k, 80 + k)):
                keys = orc.fill_random(n * 8, seed).reshape(n, 8)
                vals = orc.fill_random(n * 128, seed + 100).reshape(n, 128)
                pair.append((n, keys, vals, _dev(torch, keys), _dev(torch, vals),
                             orc.build_entries_fixed(1, keys, vals)))
            jobs.append((pair, _poison(torch, m.levels_len(3000 + k) * 32)))
        top_lv, top_rt = _poison(torch, m.levels_len(3) * 32), _poison(torch, 32)
        torch.cuda.synchronize()
        events = []
        for k, (pair, lv) in enumerate(jobs):
            for (n, _, _, dk, dv, _) in pair:
                N.check(L.mh_dev_htree_build_entries_fixed(ctxs[k].handle, 1, n, dk.data_ptr(), 8,
                                                           dv.data_ptr(), 128, None, lv.data_ptr(),
                                                           roots.data_ptr() + 32 * k))
            ev = torch.cuda.Event()
            ev.record(streams[k])
            events.append(ev)
        for ev in events:
            streams[3].wait_event(ev)
        N.check(L.mh_dev_htree_reduce_nodes(ctxs[3].handle, roots.data_ptr(), 3, top_lv.data_ptr(),
                                            top_rt.data_ptr()))
        torch.cuda.synchronize()
        r = []
        for k, (pair, lv) in enumerate(jobs):
            n, _, _, _, _, (_, olv, oroot) = pair[1]
            where = "stream %d: build n=%d after n=%d into the same levels" % (k, n, pair[0][0])
            g = _host(lv).tobytes()[:olv.nbytes]
            assert g == olv.tobytes(), (where, _first_diff(g, olv.tobytes()))
            assert _host(roots).tobytes()[32 * k:32 * k + 32] == oroot, (where, "root")
            r.append(oroot)
        l1 = orc.sha256(b"\x01" + r[0] + r[1])
        top = orc.sha256(b"\x01" + l1 + r[2])
        assert _host(top_lv).tobytes() == b"".join(r) + l1 + r[2] + top, "reduce_nodes levels"
        assert _host(top_rt).tobytes() == top, "reduce_nodes root on the fourth stream"
    finally:
        for c in ctxs:
            c.close()


# ================================================ C: one context, many entry points
def _c_htree_verify(m, orc, n, seed):
    rng = np.random.default_rng(seed)
    w = 1000 + seed % 50
    d = orc.fill_random(w * 32, seed).reshape(w, 32)
    lv, root = orc.htree_build(d)
    leaves = rng.integers(0, w, n)
    proofs = [m.InclusionProof(int(i), w, [bytes(x) for x in orc.htree_inclusion_proof(lv, w, int(i))[1]])
              for i in leaves]
    digs = d[leaves].copy()
    digs[::9, 0] ^= 1   # every ninth does not verify
    roots = np.tile(np.frombuffer(root, np.uint8), (n, 1))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(p.terms) for p in proofs])
    flat = np.frombuffer(b"".join(t for p in proofs for t in p.terms), np.uint8).reshape(-1, 32)
    _, ook = orc.htree_verify_csr(leaves.astype(np.uint64), np.full(n, w, np.uint64), off, flat,
                                  digs, roots)
    assert 0 < ook.sum() < n
    return (lambda ctx: m.verify_inclusion_batch(proofs, digs, roots, ctx=ctx).tolist(),
            ook.astype(bool).tolist())


def _c_ahtree_verify(m, orc, kind, n, seed):
    rng = np.random.default_rng(seed)
    size = 700 + seed % 40
    o = orc.AHtree(size)
    o.append_batch(orc.fill_random(size * 32, seed).reshape(size, 32))
    J = rng.integers(1, size + 1, n).astype(np.uint64)
    I = J.copy() if kind == 2 else np.array([int(rng.integers(1, j + 1)) for j in J], np.uint64)
    ot, ont, ost = o.proof_batch(1 if kind == 1 else 0, I, J, cap=24)
    assert not ost.any()
    dl = o.dlog_bytes()
    leaf = [dl[32 * orc.nodes_until(int(i)):32 * orc.nodes_until(int(i)) + 32] for i in I]
    a = leaf if kind != 1 else [o.root_at(int(i))[1] for i in I]
    b = [bytearray(o.root_at(int(j))[1]) for j in J]
    for r in range(0, n, 7):
        b[r][5] ^= 0x10
    items = [([bytes(x) for x in ot[r, :ont[r]]], int(I[r]), int(J[r]), a[r], bytes(b[r]))
             for r in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ont.astype(np.uint64))
    flat = np.concatenate([ot[r, :ont[r]] for r in range(n)] + [np.zeros((0, 32), np.uint8)])
    A = np.frombuffer(b"".join(a), np.uint8).reshape(n, 32)
    B = np.frombuffer(b"".join(bytes(x) for x in b), np.uint8).reshape(n, 32)
    _, ook = orc.ahtree_verify_batch(kind, I, J, off, flat, A, B)
    oev, odef = orc.ahtree_eval_batch(kind, I, J, off, flat, A)
    assert 0 < ook.sum() < n

    def run(ctx):
        ok, ev = m.ahtree_verify_batch(kind, items, ctx, want_eval=True)
        return ok.tolist(), ev[odef].tobytes()

    return run, (ook.astype(bool).tolist(), oev[odef].tobytes())


def _c_values(orc, n, seed, max_len):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    buf = orc.fill_random(int(off[n]) + 16, seed)
    st, hv, _, _ = orc.build_entries_csr(1, np.zeros(1, np.uint8), np.zeros(n + 1, np.uint64), None,
                                         None, buf, off, want_levels=False)
    assert st == 0
    return buf, off, hv, lens


def _c_verify_values(m, orc, n, seed, max_len=300):
    buf, off, hv, lens = _c_values(orc, n, seed, max_len)
    hv = hv.copy()
    hv[::11, 31] ^= 1
    vlen = lens.astype(np.uint64)
    vlen[3 % n] += 1
    want = orc.verify_values(buf, off, hv, vlen)
    assert 0 < want[0] < n

    def run(ctx):
        bad, st = m.verify_values(buf, off, hv, vlen, ctx=ctx)
        return bad, st.tolist()

    return run, (want[0], want[1].tolist())


def _c_dev_sha256(m, orc, n, seed, max_len):
    from gpu_util import DevBuf
    from immustore_amd import _native as N
    buf, off, hv, _ = _c_values(orc, n, seed, max_len)

    def run(ctx):
        db, do = DevBuf.from_host(ctx, buf), DevBuf.from_host(ctx, off)
        out = DevBuf.from_host(ctx, np.full(n * 32, 0xA5, np.uint8))
        N.check(N.load().mh_dev_sha256_batch(ctx.handle, db.ptr, do.ptr, n, out.ptr))
        ctx.synchronize()
        got = out.to_host().tobytes()
        for x in (db, do, out):
            x.free()
        return got

    return run, hv.tobytes()


def _c_tx_alh(m, orc, n, seed):
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, m.TX_HEADER)
    recs["id"] = rng.integers(1, 1 << 62, n)
    recs["ts"] = rng.integers(-(1 << 62), 1 << 62, n)
    recs["bl_tx_id"] = rng.integers(0, 1 << 62, n)
    for f in ("bl_root", "prev_alh", "eh"):
        recs[f] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    recs["version"] = np.arange(n) % 2
    recs["nentries"] = rng.integers(0, 1 << 16, n)
    blob = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    v1 = recs["version"] == 1
    recs["md_len"][v1] = rng.integers(0, 30, int(v1.sum()))
    recs["md_off"][v1] = rng.integers(0, 30, int(v1.sum()))
    want = [orc.tx_header_alh(recs[k], blob) for k in range(n)]
    assert all(w[0] == 0 for w in want)

    def run(ctx):
        inner, alh = m.tx_alh_batch(recs, blob, ctx)
        return inner.tobytes(), alh.tobytes()

    return run, (b"".join(w[1] for w in want), b"".join(w[2] for w in want))


def _c_build_many(m, orc, n, seed, hi):
    rng = np.random.default_rng(seed)
    trees = [orc.fill_random(max(int(w), 1) * 32, seed + k).reshape(-1, 32)[:int(w)]
             for k, w in enumerate(rng.integers(0, hi + 1, n))]
    want = b"".join(orc.htree_build(t)[1] for t in trees)
    return (lambda ctx: m.htree_build_many(trees, ctx).tobytes()), want


def _c_call(m, orc, member, n, seed):
    if member == "htree_verify":
        return _c_htree_verify(m, orc, n, seed)
    if member.startswith("ahtree_verify_"):
        return _c_ahtree_verify(m, orc, {"incl": 0, "cons": 1, "last": 2}[member[14:]], n, seed)
    if member == "verify_values":
        # the sort group's third round: fewer length classes than its first
        return _c_verify_values(m, orc, n, seed, 60 if n == U.SORT_MIN else 4096 if n > 10000 else 300)
    if member == "dev_sha256":
        return _c_dev_sha256(m, orc, n, seed, 60 if n == U.SORT_MIN else 4096)
    if member == "tx_alh":
        return _c_tx_alh(m, orc, n, seed)
    if member == "build_many_packed":
        return _c_build_many(m, orc, n, seed, 16)     # > 2048 trees, none wider than 64
    assert member == "build_many_planned"
    return _c_build_many(m, orc, n, seed, 300)         # the host tree plan


def test_one_context_many_entry_points(m, orc):
    """One context of its own through the interleaving CTX_ORDER of
    call_sequence_util: the users of s_msgs (htree and ahtree proof
    verification of all three kinds with eval_out, the value check), of s_sort
    (mh_dev_sha256_batch and the value check at 20001, 100 and 16384 values,
    the last with fewer length classes) and of s_tx (mh_tx_alh_batch,
    mh_htree_build_many packed and planned), each group large -> small ->
    large with other data and the other groups in between; some rows of
    every verifier fail on purpose.  Every result equals the oracle's for that
    call alone; a call that differs is run again on a fresh context for the
    message.  Oracle cost: 21 calls, 0.6 s."""
    ctx = m.Context(0)
    before = "a new context"
    try:
        for k, (group, idx) in enumerate(U.CTX_ORDER):
            g = U.CTX_GROUPS[group]
            member, n = g["members"][idx], g["sizes"][idx]
            run, want = _c_call(m, orc, member, n, 3000 + k)
            got = run(ctx)
            if got != want:
                f = m.Context(0)
                fresh = run(f) == want
                f.close()
                pytest.fail("call %d %s(n=%d) [%s] after %s differs from the oracle; the same call "
                            "on a fresh context is %s" % (k, member, n, group, before,
                                                          "right" if fresh else "wrong too"))
            before = "%s(n=%d) [%s]" % (member, n, group)
    finally:
        ctx.close()


# ---------------------------------------------- C, continued: wire verifiers and stores
class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rot(seq, k, n):
    """n items of seq from position k on, wrapping: other data for every call"""
    assert len(seq) >= n, (len(seq), n)
    k %= len(seq)
    return (list(seq[k:]) + list(seq[:k]))[:n]


class _Corpora:
    """The corpora of the suite's own utilities, each made once, with its CPU
    reference.  Every member(name, n, k) -> (run(ctx) -> got, want)."""

    def __init__(self, m, orc, fixtures):
        self.m, self.orc, self.fx = m, orc, fixtures
        self.cache = {}

    def get(self, name):
        if name not in self.cache:
            self.cache[name] = getattr(self, "_make_" + name)()
        return self.cache[name]

    # -- DualProofV2 messages of the Go stores from the oracle's own proofs
    def _make_dual_v2(self):
        import wire
        from test_gpu_formats import _rec_hdr
        from tx_util import headers_from_fixture
        orc, rows = self.orc, []
        for name in sorted(self.fx):
            fx = self.fx[name]
            pay = np.stack([np.frombuffer(bytes.fromhex(p), np.uint8) for p in fx["aht_payloads"]])
            o = orc.AHtree()
            o.append_batch(pay)
            recs, blob, alhs = headers_from_fixture(fx["txs"])
            n = len(recs)
            for a in range(1, n + 1):
                for b in range(a, n + 1):
                    est, msg = wire.dual_proof_v2_pb(_rec_hdr(recs[a - 1], blob),
                                                     _rec_hdr(recs[b - 1], blob), o)
                    if est:
                        continue
                    sa, ta = alhs[a - 1], alhs[b - 1]
                    if (a + b) % 5 == 0:
                        ta = bytes(31) + b"\x01"      # a wrong target Alh
                    M = wire.MSG["DualProofV2"].FromString(msg)
                    want = orc.verify_dual_proof_v2(recs[a - 1], recs[b - 1], blob,
                                                    list(M.inclusionProof), list(M.consistencyProof),
                                                    a, b, sa, ta)
                    rows.append((msg, a, b, sa, ta, int(want)))
        assert len({r[5] for r in rows}) > 1
        return rows

    def dual_v2_pb(self, n, k):
        from immustore_amd import txlayer
        rows = _rot(self.get("dual_v2"), 37 * k, n)
        return (lambda ctx: txlayer.verify_dual_proof_v2_pb_batch(
            [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
            [r[4] for r in rows], ctx=ctx).tolist()), [r[5] for r in rows]

    # -- DualProof (v1) messages of the Go stores, tampered ones among them
    def _make_dual_v1(self):
        import wire
        from test_gpu_pb_decode import dual_v1_msg
        from test_tx_oracle import dual_v1_args
        from tx_util import headers_from_fixture
        rows = []
        for name in sorted(self.fx):
            fx = self.fx[name]
            recs, blob, alhs = headers_from_fixture(fx["txs"])
            for c in fx["dual_v1"]:
                for tamper in (None, "lap", "lin", "last", "tbl"):
                    a = dual_v1_args(c, recs, blob, alhs, tamper)
                    rows.append((dual_v1_msg(wire, a), a[9], a[10], a[11], a[12],
                                 bool(self.orc.verify_dual_proof(*a))))
        return rows

    def dual_v1_pb(self, n, k):
        from immustore_amd import txlayer
        rows = _rot(self.get("dual_v1"), 101 * k, n)

        def run(ctx):
            st, ok = txlayer.verify_dual_proof_pb_batch(
                [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                [r[3] for r in rows], [r[4] for r in rows], ctx=ctx)
            return st.tolist(), [bool(x) for x in ok]

        return run, ([0] * n, [r[5] for r in rows])

    # -- VerifiableGet answers
    def _make_ventry(self):
        import verifiable_entry_util as V
        cases = V.good_cases() + V.tamper_cases()
        return [(c, V.reference(*c[1:])) for c in cases]

    def ventry_pb(self, n, k):
        from immustore_amd import txlayer
        rows = _rot(self.get("ventry"), 53 * k, n)
        cases = [c for c, _ in rows]

        def run(ctx):
            st, ok, ntx, nalh = txlayer.verify_verifiable_entry_pb_batch(
                [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                [c[4] for c in cases], [c[5] for c in cases], ctx=ctx)
            return [(int(st[p]), bool(ok[p]), int(ntx[p]), nalh[p].tobytes()) for p in range(n)]

        return run, [e for _, e in rows]

    # -- VerifiableTx answers (the checker is the utility's own)
    def _make_vtx(self):
        import verifiable_tx_util as V
        c1, e1 = V.expectations(V.good_cases)
        c2, e2 = V.expectations(V.tamper_cases)
        return list(zip(list(c1) + list(c2), list(e1) + list(e2)))

    def vtx_pb(self, n, k):
        import verifiable_tx_util as V
        from immustore_amd import txlayer
        rows = _rot(self.get("vtx"), 29 * k, n)
        cases, exp = [c for c, _ in rows], [e for _, e in rows]

        def run(ctx):
            V.check(txlayer.verify_verifiable_tx_pb_batch(*V.columns(cases), ctx=ctx), cases, exp)
            return True

        return run, True

    # -- replication onto a tree of P leaves
    def _make_repl(self):
        import replicate_util as R
        return R.synthetic_store(self.orc, R.simple_specs(200, seed=77),
                                 bl_of=lambda i: [i - 1, i // 2, 0][i % 3])

    def replicate(self, n, k):
        import replicate_util as R
        m, orc = self.m, self.orc
        txs, trees = self.get("repl")
        P = 7 * k % 50
        blobs = [x["blob"] for x in txs[P:P + n]]
        if n > 4:
            blobs[n - 2] = R._hdr_edit(txs[P + n - 2], eh=bytes(32))
        prev = R.prev_alh_of(orc, txs, P)
        ref = R.reference(orc, blobs, trees[P], prev)

        def run(ctx):
            t = m.AHtree(ctx)
            if P:
                t.append_batch(np.frombuffer(b"".join(x["alh"] for x in txs[:P]),
                                             np.uint8).reshape(P, 32))
            out = m.replicate_tx_batch(t, blobs, prev, **R.Limits().kw())
            _replicate_same(out, ref, t, "replicate %d txs onto %d" % (n, P))
            t.close()
            return True

        return run, True

    # -- documents
    def _make_docs(self):
        from tx_util import document_cases
        docs, blob = document_cases(self.fx, self.orc)
        return [(d, self.orc.verify_document(d, blob)) for d in docs], blob

    def documents(self, n, k):
        from immustore_amd import txlayer
        rows, blob = self.get("docs")
        rows = _rot(rows, 61 * k, n)
        docs = [dict(d) for d, _ in rows]
        docs[0]["md_blob"] = blob

        def run(ctx):
            st, alh = txlayer.verify_document_batch(docs, ctx=ctx)
            return [(int(st[p]), alh[p].tobytes()) for p in range(n)]

        return run, [(s, a if s == 0 else bytes(32)) for _, (s, a) in rows]

    # -- answers generated on the device: VerifiableGet answers / tx answers
    def _make_vans(self):
        import answer_util as A
        s = A.synthetic()
        return s, A.synthetic_requests(s), {}

    def verifiable_answers(self, n, k, hint=False):
        import test_gpu_answers as TA
        s, reqs, res = self.get("vans")
        reqs = _rot(reqs, 41 * k, n)
        exp = TA.expected(s, reqs)

        def run(ctx):
            if ctx not in res:
                res[ctx] = TA.resident(ctx, s)
            kw = dict(size_hint=int(exp[1][-1])) if hint else {}
            TA.check(s, reqs, TA.run(res[ctx], reqs, **kw), exp)
            return True

        return run, True

    def _make_txans(self):
        import test_gpu_tx_spec as TT
        import tx_spec_util as TU
        S = TU.synthetic()
        return S.store, TT.parity_requests(S.store), {}

    def tx_answers(self, n, k, hint=False):
        import test_gpu_tx_spec as TT
        import tx_spec_util as TU
        m = self.m
        s, reqs, res = self.get("txans")
        reqs = _rot(reqs, 97 * k, n)
        exp = TU.expect(s, reqs)

        def run(ctx):
            if ctx not in res:
                tree = m.AHtree(ctx)
                tree.append_batch(np.frombuffer(b"".join(s.ans.alhs), np.uint8).reshape(-1, 32))
                res[ctx] = (TT.on_device(m, ctx, s.exp), tree)
            dev, tree = res[ctx]
            TT.same(reqs, TT.call(m, ctx, dev, tree, reqs, int(exp[1][-1])), exp, "tx_answers")
            return True

        return run, True

    # -- export with host out
    def _make_export(self):
        import export_util as X
        return X.synthetic(self.orc), {}

    def export(self, n, k, first=1, arm="A"):
        import test_gpu_export as TE
        m = self.m
        syn, res = self.get("export")
        st = syn.store
        ex = st.expect(first, n)

        def run(ctx):
            if ctx not in res:
                res[ctx] = TE.on_device(m, ctx, st)
            with _Env(MH_EXPORT_ARM=arm):
                TE.same(TE.export(m, ctx, res[ctx], first, n, "pageable", total=int(ex["off"][-1])),
                        ex, ("export", first, n, arm))
            return True

        return run, True

    # -- tx logs
    def _make_bulk(self):
        from tx_util import _bulk_txlog
        return _bulk_txlog(np.random.default_rng(5), 9000)

    def txlog_chunks(self, n, k, weights="1:1:1"):
        m, orc = self.m, self.orc
        raw, starts = self.get("bulk")
        assert len(raw) >= (16 << 20) and n == len(starts)
        bad = bytearray(raw)
        bad[starts[1000 + 777 * k % 7000] - 33] ^= 1    # another record's last hVal every call
        bad = bytes(bad)
        want = orc.txlog_validate(bad)

        def run(ctx):
            with _Env(MH_TXLOG_WEIGHTS=weights):
                a = m.txlog_validate(bad, ctx=ctx)
            return (a[0], a[1], a[2], a[4].tobytes(), list(a[5]))

        return run, (want[0], want[1], want[2], want[3].tobytes(), list(want[4]))

    def clog(self, n, k, mode="host", width=40):
        import test_gpu_clog as TC
        from tx_util import _synthetic_txlog, clog_for, record_spans
        orc = self.orc
        raw = _synthetic_txlog(np.random.default_rng(600 + k), n, orc, max_entries=width)
        spans = record_spans(raw)
        cl = clog_for(raw, spans, 12)

        def run(ctx):
            d = TC._dev(raw)
            TC._same_as_oracle(orc, raw, cl, 12, TC._clog(ctx, raw, d, cl, 12, mode=mode))
            return True

        return run, True

    def close(self):
        for name in ("vans", "txans", "export"):
            if name in self.cache:
                for v in self.cache[name][-1].values():
                    for x in (v if isinstance(v, tuple) else (v,)):
                        tree = getattr(x, "tree", None)
                        x.close()
                        if tree is not None:
                            tree.close()


def test_one_context_wire_verifiers_and_stores(m, orc, fixtures):
    """One context of its own through CTX2_ORDER of call_sequence_util: the
    wire verifiers and mh_replicate_tx_batch on s_tx (DualProofV2, DualProof,
    VerifiableEntry and VerifiableTx messages), VerifiableGet verification
    against replication on s_ventry, mh_verify_document_batch with the other
    users of s_msgs, generated VerifiableGet answers against tx answers on
    s_ans* (with a size hint and without, fewer requests than the call
    before), mh_export_tx_batch with host out in both MH_EXPORT_ARM arms (a
    long clean range, one tx, a range with unavailable values), and tx logs
    validated in 3, 1 and 2 chunk groups, then by their commit log from host
    and resident bytes, wide then narrow then wide.  Each group goes large ->
    small -> large with other data, the others in between; every result is the
    CPU reference's of that call alone (the corpora and references of the
    suite's own utilities).  A call that differs is run again on a fresh
    context for the message.  Oracle cost: 4 s, most of it the VerifiableTx
    and DualProof corpora, each made once."""
    corp = _Corpora(m, orc, fixtures)
    ctx = m.Context(0)
    before = "a new context"
    try:
        for k, (group, idx) in enumerate(U.CTX2_ORDER):
            member, n, kw = U.CTX2_GROUPS[group]["calls"][idx]
            run, want = getattr(corp, member)(n, k, **kw)
            what = "call %d %s(n=%d, %r) [%s] after %s" % (k, member, n, kw, group, before)
            try:
                good = run(ctx) == want
                err = None
            except AssertionError as e:
                good, err = False, e
            if not good:
                f = m.Context(0)
                try:
                    fresh = run(f) == want
                except AssertionError:
                    fresh = False
                pytest.fail("%s differs from the reference%s; the same call on a fresh context is %s"
                            % (what, "" if err is None else " (%s)" % (str(err)[:300],),
                               "right" if fresh else "wrong too"))
            before = "%s(n=%d) [%s]" % (member, n, group)
    finally:
        corp.close()
        ctx.close()
