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


def test_dual_v2_status_order(m, ctx):
    """(f): one fault per branch of dual_proof_v2_core and two at once, the
    status of the earlier rule; every status appears."""
    N = m._native
    c = U.dual_v2_rows()
    want = U.oracle_dual_v2_status()
    assert set(want.tolist()) == DUAL_V2_STATUSES
    blob = np.frombuffer(c.blob, np.uint8)
    st = np.full(c.n, -1, np.int32)
    N.check(N.load().mh_verify_dual_proof_v2_batch(
        ctx.handle, c.n, c.sh.ctypes.data, c.th.ctypes.data, blob.ctypes.data, blob.size,
        c.incl_off.ctypes.data, c.incl.ctypes.data, c.cons_off.ctypes.data, c.cons.ctypes.data,
        c.s.ctypes.data, c.t.ctypes.data, c.sa.ctypes.data, c.ta.ctypes.data, st.ctypes.data))
    _same(c, st, want, "DualProofV2 status")
    assert set(st.tolist()) == DUAL_V2_STATUSES


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
