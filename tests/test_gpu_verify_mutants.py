"""The four proof verifiers -- k_htree_verify, k_ahtree_verify<INCLUSION |
CONSISTENCY | LAST_INCLUSION>, k_linear_verify and the DualProofV2 status logic
over them -- on the corpus of verify_mutants_util.py, through the raw C ABI,
row by row against the oracle (which test_verify_mutants_cpu.py holds to a
restatement of the Go source on the same rows):

  verdicts      real proofs and their structural forgeries (terms dropped,
                appended, swapped; i, j, leaf, width off by one, swapped, 0,
                bit 63; one verifier's proof offered to another), none
                assumed false
  eval_out      Go's Eval* bit for bit on every row that walks, the header's
                promise on every row that is refused before the walk, and on
                synthetic walks with i, j up to 2^64 - 1
  device twin   mh_dev_ahtree_verify_batch with eval_out on the device
  second stride batches longer than resident_grid's launch, so that the
                grid-stride loops of both kernels go round again

No input can fault or hang a kernel: every offset array is monotonic, every
term a kernel can reach lies inside the terms array passed, and huge i / j /
leaf / width only steer selects and shifts.  Outputs are poisoned before a call.
"""
import os

import numpy as np
import pytest

import verify_mutants_util as U
from gpu_util import DevBuf
from verify_mutants_util import KIND_CONSISTENCY, KIND_INCLUSION, KIND_LAST

pytestmark = pytest.mark.gpu

KINDS = [KIND_INCLUSION, KIND_CONSISTENCY, KIND_LAST]
THREADS = min(16, os.cpu_count() or 1)


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


def _aht(m, ctx, kind, c, want_eval=True):
    """mh_ahtree_verify_batch over a corpus -> (ok uint8[n], eval_out or None)"""
    N = m._native
    ok = np.full(c.n, 0xA5, np.uint8)
    ev = np.full((c.n, 64 if kind == KIND_CONSISTENCY else 32), 0xA5, np.uint8) if want_eval else None
    N.check(N.load().mh_ahtree_verify_batch(
        ctx.handle, kind, c.n, c.i.ctypes.data, c.j.ctypes.data, c.term_off.ctypes.data,
        c.terms.ctypes.data, c.a.ctypes.data, c.b.ctypes.data, ok.ctypes.data,
        None if ev is None else ev.ctypes.data))
    return ok, ev


def _same(c, got, want, what, rows=None):
    """got == want row by row (of the rows `rows` of c, when given); the
    message names the first row that differs"""
    got, want = np.asarray(got), np.asarray(want)
    bad = (got != want) if got.ndim == 1 else (got != want).any(axis=1)
    if bad.any():
        p = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d rows differ, first row %d (%s): got %s, want %s" % (
            what, int(bad.sum()), len(bad), p, c.label[p if rows is None else int(rows[p])],
            got[p].tobytes().hex() if got.ndim > 1 else got[p],
            want[p].tobytes().hex() if want.ndim > 1 else want[p]))


# ------------------------------------------------------------------- ahtree
@pytest.mark.parametrize("kind", KINDS)
def test_ahtree_verdicts(m, ctx, kind):
    """(a) + (b) as one batch, eval_out NULL as the DualProof callers pass it."""
    c = U.ahtree_rows(kind)
    ok, _ = _aht(m, ctx, kind, c, want_eval=False)
    _same(c, ok, U.oracle_ahtree_ok(kind).astype(np.uint8), "verdict, kind %d" % kind)


@pytest.mark.parametrize("kind", KINDS)
def test_ahtree_eval_real_proofs(m, ctx, kind):
    """The same batch with eval_out: Go's Eval* wherever the verifier walks;
    on the rows it refuses before the walk (i > j, i == 0, i < j without
    terms; consistency: also i == j without terms) what
    include/immustore_merkle.h promises -- the leaf a[p] unchanged
    (INCLUSION), 64 zero bytes (CONSISTENCY).  LAST_INCLUSION always walks."""
    c = U.ahtree_rows(kind)
    want, refused = U.oracle_ahtree_rows_eval(kind)
    ok, ev = _aht(m, ctx, kind, c)
    _same(c, ok, U.oracle_ahtree_ok(kind).astype(np.uint8), "verdict with eval_out, kind %d" % kind)
    _same(c, ev[~refused], want[~refused], "eval_out of a walked row, kind %d" % kind,
          np.nonzero(~refused)[0])
    if kind == KIND_LAST:
        assert not refused.any()
        assert (c.i == 0).any()  # walked all the same
        return
    assert refused.sum() > 4000
    pinned = c.a[refused] if kind == KIND_INCLUSION else np.zeros((refused.sum(), 64), np.uint8)
    _same(c, ev[refused], pinned, "eval_out of a refused row, kind %d" % kind,
          np.nonzero(refused)[0])
    assert not ok[refused & ~((c.i == c.j) & (c.i != 0))].any()


@pytest.mark.parametrize("kind", KINDS)
def test_ahtree_eval_synthetic_walks(m, ctx, kind):
    """(c): walks at i, j that no tree reaches, every evaluated root bit for
    bit; ok with a / b = the oracle's roots on even rows, a complement on odd."""
    w, want, want_ok = U.oracle_walks(kind)
    assert (w.j >= 2**63).sum() >= 20
    ok, ev = _aht(m, ctx, kind, w)
    _same(w, ev, want, "eval_out of a synthetic walk, kind %d" % kind)
    _same(w, ok, want_ok.astype(np.uint8), "verdict of a synthetic walk, kind %d" % kind)
    assert ok[::2].all() and not ok[1::2].any()


def test_ahtree_eval_last_inclusion_wrapper(m, ctx, orc):
    """immustore_amd.ahtree_eval_last_inclusion, next to its two siblings."""
    real = U.ahtree_rows(KIND_LAST)
    p3 = int(np.nonzero((real.cls == "real") & (np.diff(real.term_off) >= 3))[0][0])
    for c, p in ((real, p3), (U.ahtree_walks(KIND_LAST), U.WALKS_PER_KIND + 2)):
        t = [x.tobytes() for x in c.terms_of(p)]
        assert len(t) > 0
        got = m.ahtree_eval_last_inclusion(t, int(c.i[p]), c.a[p].tobytes(), ctx)
        assert got == orc.ahtree_eval_last_inclusion(t, int(c.i[p]), c.a[p].tobytes()), c.label[p]
    c, p = U.ahtree_walks(KIND_INCLUSION), U.WALKS_PER_KIND  # (1, 2^64 - 1)
    t = [x.tobytes() for x in c.terms_of(p)]
    assert m.ahtree_eval_inclusion(t, int(c.i[p]), int(c.j[p]), c.a[p].tobytes(), ctx) == \
        orc.ahtree_eval_inclusion(t, int(c.i[p]), int(c.j[p]), c.a[p].tobytes())
    c, p = U.ahtree_walks(KIND_CONSISTENCY), U.WALKS_PER_KIND + 1  # (2^64 - 1, 2^64 - 1)
    t = [x.tobytes() for x in c.terms_of(p)]
    assert m.ahtree_eval_consistency(t, int(c.i[p]), int(c.j[p]), ctx) == \
        orc.ahtree_eval_consistency(t, int(c.i[p]), int(c.j[p]))[1:]


@pytest.mark.parametrize("kind", KINDS)
def test_ahtree_device_pointer_twin(m, ctx, kind):
    """mh_dev_ahtree_verify_batch, every pointer device memory, eval_out
    included: 1000 rows across (b) and 1000 of (c), equal to the host call on
    the same rows and to the oracle."""
    N = m._native
    rows, walks = U.ahtree_rows(kind), U.oracle_walks(kind)[0]
    a = rows.take(np.linspace(0, rows.n - 1, 1000).astype(np.int64))
    b = walks.take(np.linspace(0, walks.n - 1, 1000).astype(np.int64))
    c = U.Corpus()
    c.n = a.n + b.n
    c.i, c.j = np.concatenate([a.i, b.i]), np.concatenate([a.j, b.j])
    c.a, c.b = np.concatenate([a.a, b.a]), np.concatenate([a.b, b.b])
    c.term_off = np.concatenate([a.term_off, b.term_off[1:] + a.term_off[-1]])
    c.terms = np.ascontiguousarray(np.concatenate([a.terms[:int(a.term_off[-1])], b.terms]))
    c.label = a.label + b.label
    assert len(set(a.cls)) >= 10 and (np.diff(c.term_off.astype(np.int64)) >= 0).all()
    assert int(c.term_off[-1]) < len(c.terms)
    host_ok, host_ev = _aht(m, ctx, kind, c)
    w = host_ev.shape[1]
    d = {k: DevBuf.from_host(ctx, getattr(c, k)) for k in ("i", "j", "term_off", "terms", "a", "b")}
    d_ok = DevBuf.from_host(ctx, np.full(c.n, 0xA5, np.uint8))
    d_ev = DevBuf.from_host(ctx, np.full(c.n * w, 0xA5, np.uint8))
    N.check(N.load().mh_dev_ahtree_verify_batch(
        ctx.handle, kind, c.n, d["i"].ptr, d["j"].ptr, d["term_off"].ptr, d["terms"].ptr,
        d["a"].ptr, d["b"].ptr, d_ok.ptr, d_ev.ptr))
    ctx.synchronize()
    _same(c, d_ok.to_host(), host_ok, "device-pointer verdict, kind %d" % kind)
    _same(c, d_ev.to_host().reshape(c.n, w), host_ev, "device-pointer eval_out, kind %d" % kind)
    import oracle as orc
    want = orc.ahtree_verify_batch(kind, c.i, c.j, c.term_off, c.terms, c.a, c.b)[1]
    _same(c, host_ok, want, "verdict of the slice, kind %d" % kind)
    _same(c, host_ev, U.ahtree_eval_expected(c, kind)[0], "eval_out of the slice, kind %d" % kind)
    for x in list(d.values()) + [d_ok, d_ev]:
        x.free()


# -------------------------------------------------------------------- htree
def _htree(m, ctx, c):
    N = m._native
    ok = np.full(c.n, 0xA5, np.uint8)
    N.check(N.load().mh_htree_verify_inclusion_batch(
        ctx.handle, c.n, c.i.ctypes.data, c.j.ctypes.data, c.term_off.ctypes.data,
        c.terms.ctypes.data, c.a.ctypes.data, c.b.ctypes.data, ok.ctypes.data))
    return ok


def test_htree_verdicts(m, ctx):
    """(d): every leaf of 39 widths and their forgeries, leaf / width at 0, -1
    and with bit 63 set (Go's signed % and /)."""
    c = U.htree_rows()
    _same(c, _htree(m, ctx, c), U.oracle_htree_ok().astype(np.uint8), "htree verdict")


# ------------------------------------------------------------ linear proofs
def test_linear_verdicts(m, ctx):
    """(e): the length rule t - s + 1 from both sides, ids across 2^32 and at
    2^63, inner terms reordered."""
    N = m._native
    c = U.linear_rows()
    ok = np.full(c.n, 0xA5, np.uint8)
    N.check(N.load().mh_verify_linear_proof_batch(
        ctx.handle, c.n, c.ps.ctypes.data, c.pt.ctypes.data, c.term_off.ctypes.data,
        c.terms.ctypes.data, c.s.ctypes.data, c.t.ctypes.data, c.sa.ctypes.data, c.ta.ctypes.data,
        ok.ctypes.data))
    _same(c, ok, U.oracle_linear_ok().astype(np.uint8), "linear verdict")


# -------------------------------------------------------------- DualProofV2
# every status VerifyDualProofV2 can return (verification.go:304-372)
DUAL_V2_STATUSES = {U.ST_OK, U.ST_ILLEGAL, U.ST_NEWER, U.ST_LINKING, U.ST_INCLUSION,
                    U.ST_CONSISTENCY}


def _dual_v2(m, ctx, c, k=0, blob=None, blob_len=None):
    """mh_verify_dual_proof_v2_batch over c -> status int32[n - k].  k > 0:
    rows [k, n) addressed as a slice of the batch -- incl_off + k, cons_off +
    k, the term arrays whole.  blob: the bytes passed instead of c.blob (False:
    a null pointer), blob_len: the length given for them."""
    N = m._native
    if blob is None:
        blob = np.frombuffer(c.blob, np.uint8)
    st = np.full(c.n - k, -1, np.int32)
    N.check(N.load().mh_verify_dual_proof_v2_batch(
        ctx.handle, c.n - k, c.sh[k:].ctypes.data, c.th[k:].ctypes.data,
        None if blob is False else blob.ctypes.data, blob.size if blob_len is None else blob_len,
        c.incl_off[k:].ctypes.data, c.incl.ctypes.data, c.cons_off[k:].ctypes.data,
        c.cons.ctypes.data, c.s[k:].ctypes.data, c.t[k:].ctypes.data, c.sa[k:].ctypes.data,
        c.ta[k:].ctypes.data, st.ctypes.data))
    return st


def _dual_v2_take(c, idx):
    """the rows idx of a DualCorpus as a corpus of their own (copies)"""
    d = U.DualCorpus()
    d.n, d.blob, d.label = len(idx), c.blob, [c.label[p] for p in idx]
    for f in ("sh", "th", "s", "t", "sa", "ta"):
        setattr(d, f, getattr(c, f)[idx].copy())
    for name in ("incl", "cons"):
        off, terms = getattr(c, name + "_off"), getattr(c, name)
        parts = [terms[int(off[p]):int(off[p + 1])] for p in idx]
        o = np.zeros(d.n + 1, np.uint64)
        o[1:] = np.cumsum([len(x) for x in parts], dtype=np.uint64)
        setattr(d, name + "_off", o)
        setattr(d, name, np.ascontiguousarray(np.concatenate(parts + [np.zeros((1, 32), np.uint8)])))
    return d


@pytest.fixture(scope="module")
def dual_v2_full(m, ctx):
    """the whole corpus through the array call, once"""
    return _dual_v2(m, ctx, U.dual_v2_rows())


def test_dual_v2_status_order(m, ctx, dual_v2_full):
    """(f): one fault per rule of VerifyDualProofV2 and two at once, the
    status of the earlier rule; every status appears.  The rules run on the
    device, behind dual_proof_v2_core: the argument and header checks in
    k_dpv2_prep, the Alh check and dpv2_ladder in k_dpv2_verdict."""
    c = U.dual_v2_rows()
    want = U.oracle_dual_v2_status()
    assert set(want.tolist()) == DUAL_V2_STATUSES
    st = dual_v2_full
    _same(c, st, want, "DualProofV2 status")
    assert set(st.tolist()) == DUAL_V2_STATUSES


def test_dual_v2_header_rules(m, ctx):
    """The header rule of the array call -- check_header, each nonzero result
    MH_ERR_ILLEGAL_ARGUMENTS -- on linked pairs that verify, every other row
    left as it is (status 0): a version above 1 in either header, a v0 header
    with metadata, metadata longer than MH_MAX_TX_METADATA_LEN, metadata
    ending one byte past the blob and, in a call of its own, metadata without
    a blob.  The rule comes after src > tgt and after the id rules.  The blob
    passed has 1 KiB behind the length given for it, so that no row could read
    outside it even without the rule.  Not compared with the oracle, which
    takes no blob length."""
    c = U.dual_v2_rows()
    MAX_MD = 268  # MH_MAX_TX_METADATA_LEN
    good = np.array([x.startswith("linked") for x in c.label]) & (c.s < c.t) & \
        (c.sh["md_len"] == 0) & (c.th["md_len"] == 0) & (U.oracle_dual_v2_status() == 0)
    idx = np.nonzero(good)[0][:16]
    assert len(idx) == 16
    L = len(c.blob)
    blob = np.frombuffer(c.blob + bytes(1024), np.uint8)
    d = _dual_v2_take(c, idx)
    assert not _dual_v2(m, ctx, d, blob=blob, blob_len=L).any()
    faults = {1: ("sh", dict(version=2)), 3: ("th", dict(version=2)),
              5: ("sh", dict(version=0, md_len=5)), 7: ("th", dict(version=1, md_len=MAX_MD + 1)),
              9: ("sh", dict(version=1, md_off=L - 3, md_len=4)),
              # two at once: with src > tgt, with a wrong header id
              11: ("th", dict(version=2)), 13: ("sh", dict(version=1, md_len=MAX_MD + 1))}
    want = np.zeros(d.n, np.int32)
    for p, (which, kw) in faults.items():
        for f, v in kw.items():
            getattr(d, which)[f][p] = v
        want[p] = U.ST_ILLEGAL
    for a, b in ((d.sh, d.th), (d.s, d.t), (d.sa, d.ta)):  # row 11: src > tgt, ids in step
        a[11], b[11] = b[11].copy(), a[11].copy()
    want[11] = U.ST_NEWER
    d.th["id"][13] += 1
    _same(d, _dual_v2(m, ctx, d, blob=blob, blob_len=L), want, "DualProofV2 header rules")
    # metadata without a blob
    d = _dual_v2_take(c, idx)
    for h, p in ((d.sh, 2), (d.th, 6)):
        h["version"][p], h["md_len"][p] = 1, 4
    want = np.zeros(d.n, np.int32)
    want[[2, 6]] = U.ST_ILLEGAL
    _same(d, _dual_v2(m, ctx, d, blob=False, blob_len=L), want,
          "DualProofV2 metadata without a blob")


@pytest.mark.parametrize("k", [1, 257])
def test_dual_v2_offsets_not_from_zero(m, ctx, dual_v2_full, k):
    """Rows [k, n) as a slice of the whole batch: incl_off + k and cons_off + k
    (first entries above 0), the term arrays whole, the per-proof arrays
    advanced.  k = 257 starts the slice past a 256-lane workgroup edge."""
    c = U.dual_v2_rows()
    assert c.n > 257 + 256 and c.incl_off[k] > 0 and c.cons_off[k] > 0
    st = _dual_v2(m, ctx, c, k=k)
    _same(c, st, dual_v2_full[k:], "DualProofV2 status of rows [%d, n)" % k, np.arange(k, c.n))


def test_dual_v2_array_vs_wire(m, ctx, orc, dual_v2_full):
    """The corpus as DualProofV2 messages (DualProofV2ToProto through the
    protobuf runtime) into mh_verify_dual_proof_v2_pb_batch: the array call's
    status on every row, as test_gpu_pb_decode._compose composes them -- the
    decode status where it is not 0, a v0 header's metadata dropped (no row
    of the corpus has any).  Six messages carry 600 KiB of an unknown field,
    so that MH_PB_CHUNK_MIB=1 cuts the batch into at least three chunks of
    different sizes, which reuse one verifier scratch."""
    import wire
    from immustore_amd import txlayer
    from test_gpu_formats import _rec_hdr
    from test_gpu_pb_decode import tag
    c = U.dual_v2_rows()
    assert not ((c.sh["md_len"] > 0) & (c.sh["version"] == 0)).any()
    assert not ((c.th["md_len"] > 0) & (c.th["version"] == 0)).any()
    msgs = []
    for p in range(c.n):
        M = wire.MSG["DualProofV2"]()
        M.sourceTxHeader.CopyFrom(wire.tx_header_msg(_rec_hdr(c.sh[p], c.blob))[1])
        M.targetTxHeader.CopyFrom(wire.tx_header_msg(_rec_hdr(c.th[p], c.blob))[1])
        M.inclusionProof.extend(x.tobytes() for x in c.incl[int(c.incl_off[p]):int(c.incl_off[p + 1])])
        M.consistencyProof.extend(x.tobytes() for x in c.cons[int(c.cons_off[p]):int(c.cons_off[p + 1])])
        msgs.append(M.SerializeToString())
    pad = 600 << 10
    ln, v = b"", pad
    while v >= 0x80:
        ln += bytes([v & 0x7f | 0x80])
        v >>= 7
    for p in np.linspace(0, c.n - 1, 6).astype(int):
        msgs[p] += tag(20, 2) + ln + bytes([v]) + bytes(pad)
    dst = txlayer.decode_dual_proof_v2_pb(msgs, ctx=ctx)[0]
    want = np.where(dst != 0, dst, dual_v2_full)
    assert set(want.tolist()) == DUAL_V2_STATUSES
    args = (msgs, c.s, c.t, list(c.sa), list(c.ta))
    _same(c, txlayer.verify_dual_proof_v2_pb_batch(*args, ctx=ctx), want, "wire vs array, one chunk")
    assert sum(len(x) for x in msgs) > 3 << 20 and max(len(x) for x in msgs) < 1 << 20
    old = os.environ.get("MH_PB_CHUNK_MIB")
    os.environ["MH_PB_CHUNK_MIB"] = "1"
    try:
        st = txlayer.verify_dual_proof_v2_pb_batch(*args, ctx=ctx)
    finally:
        if old is None:
            del os.environ["MH_PB_CHUNK_MIB"]
        else:
            os.environ["MH_PB_CHUNK_MIB"] = old
    _same(c, st, want, "wire vs array, 1 MiB chunks")


# ------------------------------------------------------------ second stride
TAIL = 1537


@pytest.fixture(scope="module")
def stride(m):
    """The term-less rows that fill resident_grid's first stride whatever the
    occupancy query answers (a CU holds at most 4 workgroups of 512, the
    launch is capped at 4 rounds of them): a (random 32-byte rows), half (the
    seeded half on which the row verifies), other (a different random row)
    and leaf_hash(a) for the htree."""
    import hashlib
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 4 * 4 * 512
    print("second stride: %d CUs, %d term-less rows + %d" % (cus, n, TAIL))
    rng = np.random.default_rng(4500)
    block = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    lh = np.stack([np.frombuffer(hashlib.sha256(b"\0" + x.tobytes()).digest(), np.uint8)
                   for x in block])
    r = rng.integers(0, 4096, n)
    half = rng.random(n) < 0.5
    return n, block[r], half, block[(r + 1) % 4096], lh[r]


def _with_prefix(n, tail, i, j, a, b):
    c = U.Corpus()
    c.n = n + tail.n
    c.i = np.concatenate([np.full(n, i, np.uint64), tail.i])
    c.j = np.concatenate([np.full(n, j, np.uint64), tail.j])
    c.term_off = np.concatenate([np.zeros(n, np.uint64), tail.term_off])
    c.terms = tail.terms
    c.a = np.ascontiguousarray(np.concatenate([a, tail.a]))
    c.b = np.ascontiguousarray(np.concatenate([b, tail.b]))
    c.label = None
    assert len(c.term_off) == c.n + 1 and int(c.term_off[-1]) < len(c.terms)
    return c


def _check_stride(c, n, tail, got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d rows differ, first row %d of %d (%s)" % (
        what, len(bad), bad[0], c.n, "term-less" if bad[0] < n else tail.label[bad[0] - n])
    # the second stride hashed, and both verdicts occur on either side of it
    assert want[n:].any() and not want[n:].all() and want[:n].any() and not want[:n].all()


@pytest.mark.parametrize("kind", KINDS)
def test_ahtree_second_stride(m, ctx, orc, stride, kind):
    """CUs * 4 * 4 * 512 + 1537 proofs in one call: more than resident_grid
    launches lanes for, so the rows past the first stride are reached by the
    loop's second pass, which ends on a partial workgroup.  All rows but the
    last 1537 are i == j == 1 without terms (a == b decides, for every kind);
    the last 1537 are real proofs and forgeries of (a) / (b)."""
    n, a, half, other, _ = stride
    rows = U.ahtree_rows(kind)
    tail = rows.take(np.linspace(0, rows.n - 1, TAIL).astype(np.int64))
    c = _with_prefix(n, tail, 1, 1, a, np.where(half[:, None], a, other))
    got, _ = _aht(m, ctx, kind, c, want_eval=False)
    want = orc.ahtree_verify_batch(kind, c.i, c.j, c.term_off, c.terms, c.a, c.b, THREADS)[1]
    _check_stride(c, n, tail, got, want, "second stride, ahtree kind %d" % kind)
    assert (want[:n] == half).all()


def test_htree_second_stride(m, ctx, orc, stride):
    """The same for k_htree_verify: leaf 0 of width 1 without terms (the root
    is the leaf hash of the digest on the seeded half), then 1537 rows of (d)."""
    n, a, half, other, lh = stride
    rows = U.htree_rows()
    tail = rows.take(np.linspace(0, rows.n - 1, TAIL).astype(np.int64))
    c = _with_prefix(n, tail, 0, 1, a, np.where(half[:, None], lh, other))
    got = _htree(m, ctx, c)
    want = orc.htree_verify_csr(c.i, c.j, c.term_off, c.terms, c.a, c.b, THREADS)[1]
    _check_stride(c, n, tail, got, want, "second stride, htree")
    assert (want[:n] == half).all()
