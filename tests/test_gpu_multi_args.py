"""The nine mh_multi_* batch calls that cut a batch over the devices, against
the promise of the header: "byte-equal to one single-context call over the
whole batch".  On a clique of three contexts on device 0 (an odd K cuts
unevenly):

  * a defective argument -- a required pointer NULL, an offset array running
    backwards at an interior or at its last index, bytes present behind a NULL
    byte pointer -- returns what the single-context call returns for the same
    arguments, with no output byte written;
  * MultiDevice.verify_values takes vlen=None as merkle.verify_values does;
  * batches of 2 (forwarded whole), 3 (one item per part) and 4 items, and a
    7-item batch whose bytes lie almost all in item 2 (parts without items),
    give the outputs of the single call and of the oracle; no offset array
    starts at 0.

Every output of a clique call lies in pinned memory between guard bands
(gpu_util.Guarded), filled with 0xA5."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import FILL, Guarded

pytestmark = pytest.mark.gpu

K = 3       # contexts of the clique
LEAD = 3    # unused bytes / terms / entries ahead of every array's first item
U64 = np.uint64
CALLS = ("htree_verify_inclusion_batch", "verify_dual_proof_v2_batch", "verify_values_batch",
         "verify_dual_proof_v2_pb_batch", "verify_dual_proof_pb_batch",
         "verify_verifiable_entry_pb_batch", "verify_verifiable_tx_pb_batch", "precommit_batch",
         "verify_document_batch")


@pytest.fixture(scope="module")
def m():
    import torch  # noqa: F401
    import immustore_amd as m
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def handles(m):
    """call name -> (single-context handle, clique handle)"""
    from immustore_amd.commit import CommitPipe
    from immustore_amd.multi import MultiDevice
    ctx = m.Context(0)
    pipe = CommitPipe(ctx)
    md = MultiDevice([0] * K)
    yield {c: (pipe.handle if c == "precommit_batch" else ctx.handle, md.handle) for c in CALLS}
    md.close()
    pipe.close()
    ctx.close()


# --------------------------------------------------------------------- a batch
class Case:
    """One batch for one call.  args: every C argument after the handle, by
    name and in order -- an array, an int or None; an output's name holds
    None.  A struct batch (struct: its ctypes class) takes its fields from
    args, the rest follows the struct.  outs: output -> (dtype, shape); want:
    output -> what the oracle says.  required: the pointers the single call
    refuses as NULL; offsets: offset array -> (first, last) index the call
    reads; byte_ptrs: the byte pointers it refuses as NULL when bytes are
    present.  cut: where item i starts, for the calls cut by bytes."""

    def __init__(self, call, args, outs, want, required, offsets, byte_ptrs, struct=None, cut=None):
        self.call, self.args, self.outs, self.want = call, args, outs, want
        self.required, self.offsets, self.byte_ptrs = required, offsets, byte_ptrs
        self.struct, self.cut = struct, cut


def invoke(case, multi, handle, outptr, over=()):
    from immustore_amd import _native as N
    a = dict(case.args)
    a.update(outptr)
    a.update(over)
    v = {k: (x.ctypes.data if isinstance(x, np.ndarray) else x) for k, x in a.items()}
    if v.get("ncorrupted") is not None:  # declared as a pointer to uint64, not as an address
        v["ncorrupted"] = C.cast(v["ncorrupted"], C.POINTER(C.c_uint64))
    fn =getattr(N.load(), ("mh_multi_" if multi else "mh_") + case.call)
    if case.struct is None:
        return fn(handle, *v.values())
    fields = [f for f, _ in case.struct._fields_]
    b = case.struct(*[v[f] for f in fields])
    return fn(handle, C.byref(b), *[x for k, x in v.items() if k not in fields])


def _nbytes(spec):
    dt, shape = spec
    return int(np.dtype(dt).itemsize * np.prod(shape, dtype=np.int64))


def run_guarded(case, multi, handle, over=()):
    """-> (return code, output -> array, every guard intact, nothing written)"""
    g = {k: Guarded(_nbytes(s), pinned=True) for k, s in case.outs.items()}
    try:
        rc = invoke(case, multi, handle, {k: x.ptr for k, x in g.items()}, over)
        out = {k: g[k].view(case.outs[k][0]).reshape(case.outs[k][1]).copy() for k in g}
        return rc, out, all(x.guards_intact() for x in g.values()), \
            all(x.untouched() for x in g.values())
    finally:
        for x in g.values():
            x.free()


def run_plain(case, handle, over=()):
    out = {k: np.full(s[1], FILL, s[0]) for k, s in case.outs.items()}
    return invoke(case, False, handle, out, over)


def defects(case):
    """(what, the arguments replaced)"""
    for name in case.required:
        yield name + " NULL", {name: None}
    for name, (lo, hi) in case.offsets.items():
        assert hi - lo >= 4, (name, lo, hi)
        mid = (lo + hi) // 2
        x = case.args[name].copy()
        x[mid] = x[mid + 1] + U64(1)
        yield "%s backwards at %d of [%d, %d]" % (name, mid, lo, hi), {name: x}
        x = case.args[name].copy()
        assert x[hi - 1] > 0
        x[hi] = x[hi - 1] - U64(1)
        yield "%s backwards at its last index" % name, {name: x}
    for name in case.byte_ptrs:
        yield name + " NULL with bytes present", {name: None}


def cut_by_bytes(start, k=K):
    """the part bounds of items starting at start[i] (n + 1 of them) cut into
    k parts of nearly equal bytes: part d begins with the first item starting
    at or after d / k of the bytes"""
    n = len(start) - 1
    t = [0] * k + [n]
    for d in range(1, k):
        want = start[0] + (start[n] - start[0]) * d // k
        t[d] = next((i for i in range(t[d - 1], n) if start[i] >= want), n)
    return t


# ------------------------------------------------------------------ the inputs
def _csr(items, lead=LEAD, unit=1):
    """items laid end to end behind `lead` unused units, 64 spare bytes behind
    -> (bytes, offsets in units; offsets[0] = lead)"""
    off = np.full(len(items) + 1, lead, U64)
    if items:
        off[1:] += np.cumsum([len(x) // unit for x in items], dtype=U64)
    buf = np.frombuffer(b"\xff" * (lead * unit) + b"".join(bytes(x) for x in items) + bytes(64),
                        np.uint8).copy()
    return buf, off


def _terms(lists):
    return _csr([b"".join(t) for t in lists], unit=32)


def _d32(xs):
    return np.frombuffer(b"".join(bytes(x) for x in xs), np.uint8).reshape(-1, 32).copy()


def _u64(xs):
    return np.array([int(x) for x in xs], U64)


def build_inclusion(items):
    """items: (leaf, width, terms, digest, root, verifies)"""
    n = len(items)
    terms, off = _terms([t[2] for t in items])
    args = dict(n=n, leaf=_u64(t[0] for t in items), width=_u64(t[1] for t in items), term_off=off,
                terms=terms, digests=_d32(t[3] for t in items), roots=_d32(t[4] for t in items),
                ok=None)
    return Case("htree_verify_inclusion_batch", args, {"ok": (np.uint8, (n,))},
                {"ok": np.array([t[5] for t in items], np.uint8)},
                ("leaf", "width", "term_off", "digests", "roots", "ok"), {"term_off": (0, n)}, ())


def _dual_v2_common(items):
    n = len(items)
    return dict(src=_u64(t[4] for t in items), tgt=_u64(t[5] for t in items),
                src_alh=_d32(t[6] for t in items), tgt_alh=_d32(t[7] for t in items),
                status=None), {"status": (np.int32, (n,))}, \
        {"status": np.array([t[8] for t in items], np.int32)}


def build_dual_v2(items, blob):
    """items: (src header, target header, inclusion terms, consistency terms,
    src, tgt, src Alh, tgt Alh, status)"""
    from immustore_amd.txlayer import _hdrs
    n = len(items)
    it, io = _terms([t[2] for t in items])
    ct, co = _terms([t[3] for t in items])
    rest, outs, want = _dual_v2_common(items)
    mb = np.frombuffer(blob, np.uint8).copy() if blob else None
    args = dict(n=n, src_hdr=_hdrs([t[0] for t in items]), tgt_hdr=_hdrs([t[1] for t in items]),
                md_blob=mb, md_blob_len=len(blob), incl_off=io, incl_terms=it, cons_off=co,
                cons_terms=ct, **rest)
    return Case("verify_dual_proof_v2_batch", args, outs, want,
                ("src_hdr", "tgt_hdr", "incl_off", "cons_off", "src", "tgt", "src_alh", "tgt_alh",
                 "status"), {"incl_off": (0, n), "cons_off": (0, n)}, ("incl_terms", "cons_terms"))


def _wire_case(call, msgs, rest, outs, want):
    n = len(msgs)
    buf, off = _csr(msgs)
    return Case(call, dict(n=n, msgs=buf, msg_off=off, **rest), outs, want,
                ("msg_off", "src", "tgt", "src_alh", "tgt_alh") + tuple(outs), {"msg_off": (0, n)},
                ("msgs",), cut=[int(x) for x in off])


def build_dual_v2_pb(items, blob):
    """the same items as DualProofV2 messages (DualProofV2ToProto)"""
    import wire
    from test_gpu_formats import _rec_hdr
    msgs = []
    for t in items:
        M = wire.MSG["DualProofV2"](inclusionProof=t[2], consistencyProof=t[3])
        M.sourceTxHeader.CopyFrom(wire.tx_header_msg(_rec_hdr(t[0], blob))[1])
        M.targetTxHeader.CopyFrom(wire.tx_header_msg(_rec_hdr(t[1], blob))[1])
        msgs.append(M.SerializeToString())
    return _wire_case("verify_dual_proof_v2_pb_batch", msgs, *_dual_v2_common(items))


def build_dual_v1_pb(items):
    """items: (orc.verify_dual_proof arguments, message, verifies)"""
    n = len(items)
    a = [t[0] for t in items]
    rest = dict(src=_u64(x[9] for x in a), tgt=_u64(x[10] for x in a),
                src_alh=_d32(x[11] for x in a), tgt_alh=_d32(x[12] for x in a), status=None, ok=None)
    return _wire_case("verify_dual_proof_pb_batch", [t[1] for t in items], rest,
                      {"status": (np.int32, (n,)), "ok": (np.uint8, (n,))},
                      {"status": np.zeros(n, np.int32), "ok": np.array([t[2] for t in items], np.uint8)})


def _answer_outs(n, exp, eh):
    outs = {"status": (np.int32, (n,)), "ok": (np.uint8, (n,)), "new_tx": (U64, (n,)),
            "new_alh": (np.uint8, (n, 32))}
    want = {"status": np.array([e[0] for e in exp], np.int32),
            "ok": np.array([e[1] for e in exp], np.uint8), "new_tx": _u64(e[2] for e in exp),
            "new_alh": _d32(e[3] for e in exp)}
    if eh:
        outs["eh_out"] = (np.uint8, (n, 32))
        want["eh_out"] = _d32(e[4] for e in exp)
    return outs, want


def _struct_args(struct, b, keep, outs):
    """the arrays a pack_* function made, by the struct's field names"""
    fields = [f for f, _ in struct._fields_]
    assert len(fields) == 1 + len(keep)
    args = dict(zip(fields, (int(b.n),) + tuple(keep)))
    args.update({k: None for k in outs})
    return args


def build_entry(items):
    """items: (verifiable_entry_util case, its reference)"""
    from immustore_amd.txlayer import _VerifiedGetBatch, pack_verified_get_batch
    cases = [c for c, _ in items]
    n = len(cases)
    b, keep = pack_verified_get_batch([c[1] for c in cases], [c[2] for c in cases],
                                      [c[3] for c in cases], [c[4] for c in cases],
                                      [c[5] for c in cases], lead=LEAD)
    outs, want = _answer_outs(n, [e for _, e in items], False)
    return Case("verify_verifiable_entry_pb_batch", _struct_args(_VerifiedGetBatch, b, keep, outs),
                outs, want, ("msg_off", "key_off", "at_tx", "state_tx", "state_alh") + tuple(outs),
                {"msg_off": (0, n), "key_off": (0, n)}, ("msgs", "keys"), _VerifiedGetBatch,
                [int(x) for x in keep[1]])


def build_tx(items):
    """items: (verifiable_tx_util case, its reference)"""
    import verifiable_tx_util as VT
    from immustore_amd.txlayer import _VerifiedTxBatch, pack_verified_tx_batch
    cases = [c for c, _ in items]
    n = len(cases)
    b, keep = pack_verified_tx_batch(*VT.columns(cases), lead=LEAD)
    outs, want = _answer_outs(n, [e for _, e in items], True)
    soff = keep[3]
    span = (int(soff[0]), int(soff[n]))
    return Case("verify_verifiable_tx_pb_batch", _struct_args(_VerifiedTxBatch, b, keep, outs),
                outs, want, ("msg_off", "kind", "spec_off", "key_off", "val_off", "at_tx", "state_tx",
                             "state_alh", "status", "ok", "new_tx", "new_alh"),
                {"msg_off": (0, n), "spec_off": (0, n), "key_off": span, "val_off": span},
                ("msgs", "keys", "vals"), _VerifiedTxBatch, [int(x) for x in keep[1]])


def build_values(items, lengths=True):
    """items: (the bytes read, stored hVal, stored length, status with the
    length checked, status without)"""
    n = len(items)
    vals, off = _csr([t[0] for t in items])
    st = np.array([t[3 if lengths else 4] for t in items], np.int32)
    args = dict(n=n, vals=vals, off=off, vlen=_u64(t[2] for t in items) if lengths else None,
                hvals=_d32(t[1] for t in items), status=None, ncorrupted=None)
    return Case("verify_values_batch", args, {"status": (np.int32, (n,)), "ncorrupted": (U64, (1,))},
                {"status": st, "ncorrupted": _u64([(st != 0).sum()])}, ("off", "hvals", "status"),
                {"off": (0, n)}, ("vals",), cut=[int(x) for x in off])


def build_precommit(items, orc):
    """items: transactions, each a list of (key, KV metadata, value, hVal
    override or None); v1, one expected Eh wrong.  LEAD unused entries lie
    ahead of the first transaction's."""
    from commit_util import pack
    n = len(items)
    ents = [e for tx in items for e in tx]
    E = len(ents)
    tx_off = np.full(n + 1, LEAD, U64)
    tx_off[1:] += np.cumsum([len(tx) for tx in items], dtype=U64)
    ahead = [b""] * LEAD
    keys, key_off = _csr(ahead + [e[0] for e in ents])
    md, md_off = _csr(ahead + [e[1] for e in ents])
    vals, val_off = _csr(ahead + [e[2] for e in ents])
    ov, use = np.zeros((LEAD + E, 32), np.uint8), np.zeros(LEAD + E, np.uint8)
    for k, e in enumerate(ents):
        if e[3] is not None:
            ov[LEAD + k], use[LEAD + k] = np.frombuffer(e[3], np.uint8), 1
    b = pack(items)
    _, eh, _ = orc.precommit_batch(1, **b)
    exp = eh.copy()
    exp[1, 0] ^= 0x40
    hv, eh, st = orc.precommit_batch(1, expect_eh=exp, **b)
    assert st[1] != 0 and not st[[0] + list(range(2, n))].any()
    args = dict(version=1, max_width=0, ntx=n, tx_off=tx_off, keys=keys, key_off=key_off, md=md,
                md_off=md_off, vals=vals, val_off=val_off, hval_override=ov, use_override=use,
                expect_eh=exp, hvals_out=None, eh_out=None, status=None)
    span = (LEAD, LEAD + E)
    return Case("precommit_batch", args,
                {"hvals_out": (np.uint8, (E, 32)), "eh_out": (np.uint8, (n, 32)),
                 "status": (np.int32, (n,))},
                {"hvals_out": hv[:E], "eh_out": eh[:n], "status": st[:n]},
                ("tx_off", "key_off", "val_off", "status", "md", "md_off", "hval_override",
                 "use_override"),
                {"tx_off": (0, n), "key_off": span, "val_off": span, "md_off": span},
                ("keys", "vals"), cut=[int(val_off[int(t)]) for t in tx_off])


def build_document(items, blob):
    """items: (txlayer.verify_document_batch document, (status, new Alh) of
    the oracle).  LEAD unused entries lie ahead of the first document's."""
    from immustore_amd.txlayer import _DocumentBatch, _hdrs
    docs = [d for d, _ in items]
    n = len(docs)
    ents = [e for d in docs for e in d["entries"]]
    E = len(ents)
    ent_off = np.full(n + 1, LEAD, U64)
    ent_off[1:] += np.cumsum([len(d["entries"]) for d in docs], dtype=U64)
    ahead = [b""] * LEAD
    doc, doc_off = _csr([d["encoded_document"] for d in docs])
    dkey, dkey_off = _csr([d["doc_key"] for d in docs])
    ekeys, ekey_off = _csr(ahead + [e[0] for e in ents])
    emd, emd_off = _csr(ahead + [e[1] for e in ents])
    it, io = _terms([d["incl"] for d in docs])
    ct, co = _terms([d["cons"] for d in docs])
    args = dict(n=n, doc=doc, doc_off=doc_off, doc_key=dkey, doc_key_off=dkey_off,
                tx_hdr=_hdrs([d["tx_hdr"] for d in docs]), ent_off=ent_off, ekeys=ekeys,
                ekey_off=ekey_off, emd=emd, emd_off=emd_off,
                ehval=_d32([bytes(32)] * LEAD + [e[2] for e in ents]),
                src_hdr=_hdrs([d["src_hdr"] for d in docs]), tgt_hdr=_hdrs([d["tgt_hdr"] for d in docs]),
                md_blob=np.frombuffer(blob, np.uint8).copy() if blob else None, md_blob_len=len(blob),
                incl_off=io, incl_terms=it, cons_off=co, cons_terms=ct,
                known_tx_id=_u64(d["known_tx_id"] for d in docs),
                known_alh=_d32(d["known_alh"] for d in docs), status=None, target_alh_out=None)
    assert list(args)[:-2] == [f for f, _ in _DocumentBatch._fields_]
    span = (LEAD, LEAD + E)
    return Case("verify_document_batch", args,
                {"status": (np.int32, (n,)), "target_alh_out": (np.uint8, (n, 32))},
                {"status": np.array([o[0] for _, o in items], np.int32),
                 "target_alh_out": _d32(o[1] if o[0] == 0 else bytes(32) for _, o in items)},
                ("doc_off", "doc_key_off", "tx_hdr", "ent_off", "ekey_off", "ehval", "src_hdr",
                 "tgt_hdr", "incl_off", "cons_off", "known_tx_id", "known_alh", "status"),
                {"doc_off": (0, n), "doc_key_off": (0, n), "ent_off": (0, n), "incl_off": (0, n),
                 "cons_off": (0, n), "ekey_off": span, "emd_off": span},
                ("doc", "doc_key", "ekeys", "incl_terms", "cons_terms") +
                (("emd",) if emd_off[-1] > emd_off[0] else ()), _DocumentBatch,
                [(int(ent_off[i]) - LEAD) * 64 + int(doc_off[i]) - LEAD for i in range(n + 1)])


@pytest.fixture(scope="module")
def batches(m, orc, fixtures):
    """call -> (build(items) -> Case, seven items two of which fail, a heavy
    item for the calls cut by bytes or None)"""
    import hashlib

    import verifiable_entry_util as VE
    import verifiable_tx_util as VT
    import wire
    from test_gpu_pb_decode import dual_v1_msg
    from test_oracle import _values_case
    from test_tx_oracle import dual_v1_args
    from tx_util import document_cases, headers_from_fixture
    out = {}
    rng = np.random.default_rng(77)

    # htree inclusion proofs over a 50-leaf tree
    W = 50
    dig = orc.fill_random(W * 32, 41).reshape(W, 32)
    lv, root = orc.htree_build(dig)
    items = []
    for k, leaf in enumerate((0, 7, 31, 49, 16, 33, 2)):
        terms = [bytes(t) for t in orc.htree_inclusion_proof(lv, W, leaf)[1]]
        d = bytes(dig[(leaf + 1) % W if k in (1, 5) else leaf])
        items.append((leaf, W, terms, d, root, orc.htree_verify_inclusion(leaf, W, terms, d, root)))
    assert [t[5] for t in items] == [True, False, True, True, True, False, True]
    out["htree_verify_inclusion_batch"] = (build_inclusion, items, None)

    # DualProofV2: cases of the first Go-written store, as arrays and as messages
    fx = next(iter(fixtures.values()))
    recs, blob, alhs = headers_from_fixture(fx["txs"])
    items = []
    for k, c in enumerate([c for c in fx["dual_v2"] if c["src"] < c["tgt"] and c["incl"]][:7]):
        ii, cc = [bytes.fromhex(x) for x in c["incl"]], [bytes.fromhex(x) for x in c["cons"]]
        sa, ta = alhs[c["src"] - 1], alhs[c["tgt"] - 1]
        if k == 1:
            ii[0] = bytes([ii[0][0] ^ 1]) + ii[0][1:]
        if k == 5:
            ta = bytes([ta[0] ^ 1]) + ta[1:]
        a = (recs[c["src"] - 1], recs[c["tgt"] - 1], ii, cc, c["src"], c["tgt"], sa, ta)
        items.append(a + (orc.verify_dual_proof_v2(a[0], a[1], blob, *a[2:]),))
    assert len(items) == 7 and [t[8] != 0 for t in items] == [k in (1, 5) for k in range(7)]
    t = items[2]
    long_proof = (t[0], t[1], t[2] * 600, t[3], t[4], t[5], t[6], t[7])
    heavy = long_proof + (orc.verify_dual_proof_v2(t[0], t[1], blob, *long_proof[2:]),)
    out["verify_dual_proof_v2_batch"] = (lambda it: build_dual_v2(it, blob), items, None)
    out["verify_dual_proof_v2_pb_batch"] = (lambda it: build_dual_v2_pb(it, blob), items, heavy)

    # DualProof (v1) messages of the same store
    items = []
    for k, c in enumerate(fx["dual_v1"][:7]):
        a = dual_v1_args(c, recs, blob, alhs, "tbl" if k in (1, 5) else None)
        items.append((a, dual_v1_msg(wire, a), orc.verify_dual_proof(*a)))
    assert any(t[2] for t in items) and not all(t[2] for t in items)
    a = items[2][0]
    a = a[:3] + (a[3] * 600,) + a[4:]
    out["verify_dual_proof_pb_batch"] = (build_dual_v1_pb, items,
                                         (a, dual_v1_msg(wire, a), orc.verify_dual_proof(*a)))

    # whole answers: the smallest good ones, two tampered, the largest good one
    for call, mod, build in (("verify_verifiable_entry_pb_batch", VE, build_entry),
                             ("verify_verifiable_tx_pb_batch", VT, build_tx)):
        good = sorted(mod.good_cases(), key=lambda c: len(c[1]))
        if mod is VT:  # every answer owns a spec, so that offsets past the last stay in the arrays
            good = [c for c in good if len(c[3]) >= 1]
        bad = sorted(mod.tamper_cases(), key=lambda c: len(c[1]))
        if mod is VT:
            bad = [c for c in bad if len(c[3]) >= 1]
        picked = [good[0], bad[0], good[1], good[2], good[3], bad[1], good[4]]
        items = [(c, mod.reference(*c[1:])) for c in picked]
        assert [bool(e[1]) for _, e in items].count(False) >= 1
        out[call] = (build, items, (good[-1], mod.reference(*good[-1][1:])))

    # values: five intact and two corrupted of tests/test_oracle._values_case
    vb, off, hv, vlen, _ = _values_case(11, 64)
    _, st_len = orc.verify_values(vb, off, hv, vlen)
    _, st_no = orc.verify_values(vb, off, hv, None)
    full = [(bytes(vb[int(off[i]):int(off[i + 1])]), bytes(hv[i]), int(vlen[i]), int(st_len[i]),
             int(st_no[i])) for i in range(64) if off[i + 1] > off[i]]
    fine, corrupt = [t for t in full if t[3] == 0 and t[4] == 0], [t for t in full if t[3] and t[4]]
    items = [fine[0], corrupt[0], fine[1], fine[2], fine[3], corrupt[1], fine[4]]
    big = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    out["verify_values_batch"] = (build_values, items,
                                  (big, hashlib.sha256(big).digest(), len(big), 0, 0))

    # precommit: 7 transactions of 1-3 entries, KV metadata and truncated values among them
    def entry(vlen_):
        rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
        return (rb(int(rng.integers(1, 40))), rb(int(rng.integers(0, 12))), rb(vlen_),
                rb(32) if rng.random() < 0.2 else None)
    items = [[entry(int(rng.integers(0, 300))) for _ in range(1 + k % 3)] for k in range(7)]
    out["precommit_batch"] = (lambda it: build_precommit(it, orc), items,
                              [entry(200_000), entry(5)])

    # documents of the first store: one untampered and its first six tampered variants
    docs, dblob = document_cases(fixtures, orc, per_store=1)
    items = [(d, orc.verify_document(d, dblob)) for d in docs[:7]]
    assert items[0][1][0] == 0 and any(o[0] for _, o in items)
    d = dict(docs[0], encoded_document=docs[0]["encoded_document"] + b"x" * 200_000)
    out["verify_document_batch"] = (lambda it: build_document(it, dblob), items,
                                    (d, orc.verify_document(d, dblob)))
    return out


# -------------------------------------------------------------------- defects
@pytest.mark.parametrize("call", CALLS)
def test_defect_is_refused_before_any_part_writes(handles, batches, call):
    """every defect of a 7-item batch: the clique's return code is the single
    call's, non-zero, and every output byte is still 0xA5"""
    build, items, _ = batches[call]
    case = build(items)
    single, clique = handles[call]
    bad, seen = [], 0
    for what, over in defects(case):
        want = run_plain(case, single, over)
        rc, _, intact, untouched = run_guarded(case, True, clique, over)
        seen += 1
        print("%s: %s: single %d, clique %d, outputs %s" %
              (call, what, want, rc, "untouched" if untouched else "WRITTEN"))
        if rc != want or not intact or (want != 0 and not untouched):
            bad.append((what, want, rc, intact, untouched))
    assert seen >= len(case.required) + 2 * len(case.offsets) + len(case.byte_ptrs)
    assert not bad, bad
    # and the batch itself is a good one
    rc, out, intact, _ = run_guarded(case, True, clique)
    assert rc == 0 and intact
    for k, w in case.want.items():
        assert np.array_equal(out[k], w), k


# ------------------------------------------------------------------ vlen=None
def test_values_without_lengths(m, orc, batches):
    """MultiDevice.verify_values(vlen=None) == merkle.verify_values(vlen=None)
    == the oracle, 7 ragged values, two corrupted"""
    from immustore_amd.multi import MultiDevice
    _, items, _ = batches["verify_values_batch"]
    case = build_values(items, lengths=False)
    a = case.args
    ost = orc.verify_values(a["vals"], a["off"], a["hvals"], None)
    assert ost[0] == 2 and np.array_equal(ost[1], case.want["status"])
    ctx, md = m.Context(0), MultiDevice([0] * K)
    try:
        one = m.verify_values(a["vals"], a["off"], a["hvals"], None, ctx=ctx)
        got = md.verify_values(a["vals"], a["off"], a["hvals"], None)
    finally:
        md.close()
        ctx.close()
    for r in (one, got):
        assert r[0] == ost[0] and np.array_equal(r[1], ost[1])


# ------------------------------------------------------------------ cut edges
def _same_as_single_and_oracle(case, single, clique, what):
    rc1, one, _, _ = run_guarded(case, False, single)
    rc, got, intact, _ = run_guarded(case, True, clique)
    assert rc1 == 0 and rc == 0 and intact, (what, rc1, rc, intact)
    for k in case.outs:
        assert np.array_equal(got[k], one[k]), (what, k, "single")
        assert np.array_equal(got[k], case.want[k]), (what, k, "oracle")


@pytest.mark.parametrize("call", CALLS)
def test_cut_edges(handles, batches, call):
    """2 items (forwarded whole), 3 (one per part), 4; and, where the cut is
    by bytes, 7 items with nearly all bytes in item 2: a part without items"""
    build, items, heavy = batches[call]
    single, clique = handles[call]
    for n in (2, 3, 4):
        case = build(items[:n])
        assert all(int(case.args[o][0]) == LEAD for o in case.offsets)  # no offset starts at 0
        _same_as_single_and_oracle(case, single, clique, n)
    if heavy is not None:
        case = build(items[:2] + [heavy] + items[3:])
        t = cut_by_bytes(case.cut)
        assert any(t[d] == t[d + 1] for d in range(K)) and t[1] == 3, t
        _same_as_single_and_oracle(case, single, clique, "heavy")
