"""The C oracle's proof verifiers against an independent restatement of the Go
source, on exactly the corpus test_gpu_verify_mutants.py gives the kernels
(verify_mutants_util.py): the oracle and the kernels were written by the same
hand, so a shared misreading of the reference would otherwise be pinned by the
GPU tests instead of caught.  The restatement below is plain Python over
hashlib and Python ints, transliterated line for line from

  embedded/ahtree/verification.go:21-137   Verify / Eval Inclusion, Consistency,
                                           LastInclusion
  embedded/htree/htree.go:166-195          VerifyInclusion (Go's signed int)
  embedded/store/verification.go:40-61     VerifyLinearProof
  embedded/store/verification.go:304-372   VerifyDualProofV2's order (header
                                           Alh taken from the oracle)

and calls nothing of the oracle's verifiers.  Also asserted: the shape of the
corpus (every mutation class rejects somewhere, the classes that can
legitimately verify do so somewhere, the synthetic walks reach j >= 2^63).
"""
import hashlib

import numpy as np
import pytest

import verify_mutants_util as U
from verify_mutants_util import KIND_CONSISTENCY, KIND_INCLUSION, KIND_LAST, M64, go_verify_inclusion

NODE = b"\x01"


def H(b):
    return hashlib.sha256(b).digest()


# ---------------------------------------------- ahtree/verification.go:21-137
def go_eval_inclusion(iproof, i, j, ileaf):  # :31-56
    i1 = (i - 1) & M64  # Go's uint64 wraps
    j1 = (j - 1) & M64
    ci = ileaf
    for h in iproof:
        if i1 % 2 == 0 and i1 != j1:
            ci = H(NODE + ci + h)
        else:
            ci = H(NODE + h + ci)
        i1 >>= 1
        j1 >>= 1
    return ci


def go_verify_inclusion_aht(iproof, i, j, ileaf, jroot):  # :21-29
    if i > j or i == 0 or (i < j and len(iproof) == 0):
        return False, None
    ci = go_eval_inclusion(iproof, i, j, ileaf)
    return jroot == ci, ci


def go_eval_consistency(cproof, i, j):  # :72-109
    fn = (i - 1) & M64
    sn = (j - 1) & M64
    while fn % 2 == 1:
        fn >>= 1
        sn >>= 1
    ci = cj = cproof[0]
    for h in cproof[1:]:
        if fn % 2 == 1 or fn == sn:
            ci = H(NODE + h + ci)
            cj = H(NODE + h + cj)
            while fn % 2 == 0 and fn != 0:
                fn >>= 1
                sn >>= 1
        else:
            cj = H(NODE + cj + h)
        fn >>= 1
        sn >>= 1
    return ci, cj


def go_verify_consistency(cproof, i, j, iroot, jroot):  # :58-70
    if i > j or i == 0 or (i < j and len(cproof) == 0):
        return False, None
    if i == j and len(cproof) == 0:
        return iroot == jroot, None
    ci, cj = go_eval_consistency(cproof, i, j)
    return iroot == ci and jroot == cj, ci + cj


def go_eval_last_inclusion(iproof, i, leaf):  # :119-137
    root = leaf
    for h in iproof:
        root = H(NODE + h + root)
    return root


def go_verify_last_inclusion(iproof, i, leaf, root):  # :111-117
    if i == 0:
        return False, go_eval_last_inclusion(iproof, i, leaf)  # the library still walks
    r = go_eval_last_inclusion(iproof, i, leaf)
    return root == r, r


GO_AHTREE = {
    KIND_INCLUSION: go_verify_inclusion_aht,
    KIND_CONSISTENCY: go_verify_consistency,
    KIND_LAST: lambda p, i, j, a, b: go_verify_last_inclusion(p, i, a, b),
}


# ------------------------------------------- store/verification.go:32-61
def go_verify_linear_proof(p_src, p_tgt, terms, src, tgt, src_alh, tgt_alh):
    if p_src != src or p_tgt != tgt:  # :41-43 (the proof is never nil here)
        return False
    if p_src == 0 or p_src > p_tgt or len(terms) == 0 or src_alh != terms[0]:  # :45-48
        return False
    if len(terms) != ((tgt - src + 1) & M64):  # :50-52
        return False
    calc = terms[0]
    for k in range(1, len(terms)):  # advanceLinearHash, :32-38
        calc = H(((p_src + k) & M64).to_bytes(8, "big") + calc + terms[k])
    return tgt_alh == calc


# ------------------------------------------ store/verification.go:304-372
def go_verify_dual_proof_v2(orc, sh, th, blob, incl, cons, src, tgt, src_alh, tgt_alh):
    if int(sh["id"]) == 0 or int(sh["id"]) != src or int(th["id"]) != tgt:
        return U.ST_ILLEGAL
    if src > tgt:
        return U.ST_NEWER
    st, _, alh = orc.tx_header_alh(sh, blob)
    if st or src_alh != alh:
        return U.ST_ILLEGAL
    st, _, alh = orc.tx_header_alh(th, blob)
    if st or tgt_alh != alh:
        return U.ST_ILLEGAL
    if int(sh["id"]) - 1 != int(sh["bl_tx_id"]) or int(th["id"]) - 1 != int(th["bl_tx_id"]):
        return U.ST_LINKING
    if src == tgt:
        return U.ST_OK
    leaf = H(b"\x00" + src_alh)  # leafFor
    tbl, troot = int(th["bl_tx_id"]), th["bl_root"].tobytes()
    if not go_verify_inclusion_aht(incl, src, tbl, leaf, troot)[0]:
        return U.ST_INCLUSION
    if src == 1:
        ok = go_verify_consistency(cons, src, tbl, leaf, troot)[0]
    else:
        ok = go_verify_consistency(cons, int(sh["bl_tx_id"]), tbl, sh["bl_root"].tobytes(), troot)[0]
    return U.ST_OK if ok else U.ST_CONSISTENCY


# ------------------------------------------------------------------- helpers
def _rows(c):
    """-> per row (i, j, [terms], a, b) in Python ints and bytes"""
    tb = c.terms.tobytes()
    off = c.term_off.tolist()
    ii, jj = c.i.tolist(), c.j.tolist()
    ab, bb = c.a.tobytes(), c.b.tobytes()
    for p in range(c.n):
        t = [tb[32 * k:32 * k + 32] for k in range(off[p], off[p + 1])]
        yield ii[p], jj[p], t, ab[32 * p:32 * p + 32], bb[32 * p:32 * p + 32]


def _shape(c, ok, may_verify, never_rejects=()):
    """Every class but "real" (and never_rejects) rejects somewhere; exactly
    the classes of may_verify verify somewhere; every real proof verifies."""
    seen_true, seen_false = set(), set()
    for cls in set(c.cls):
        m = c.cls == cls
        if ok[m].any():
            seen_true.add(cls)
        if (~ok[m]).any():
            seen_false.add(cls)
    assert ok[c.cls == "real"].all()
    assert seen_false == set(c.cls) - {"real"} - set(never_rejects)
    assert seen_true == set(may_verify) | {"real"}, seen_true ^ (set(may_verify) | {"real"})


def _first_bad(c, got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if len(bad) == 0 else (int(bad[0]), c.label[int(bad[0])], len(bad))


# the mutation classes in which some row verifies all the same, e.g. an
# i -> i - 1 that takes the same branches, a width + 1 that leaves every
# left/right choice of the leaf's path alone, (1, 1) where leaf == root
MAY_VERIFY = {
    KIND_INCLUSION: {"no_terms", "i-1", "j-1", "j+1", "swap_ij", "swap_ab", "cons_as_incl"},
    KIND_CONSISTENCY: {"no_terms", "i-1", "i+1", "j-1", "j+1", "swap_ij", "swap_ab"},
    # VerifyLastInclusion reads i only for i != 0
    KIND_LAST: {"i-1", "i+1", "swap_ab"},
}
# width_0: r = -1 never equals i on the way and ends at -1 / 2 == 0 like i
HTREE_MAY_VERIFY = {"leaf+1", "width-1", "width+1", "leaf_eq_width", "width_0", "both_bit63"}


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("kind", [KIND_INCLUSION, KIND_CONSISTENCY, KIND_LAST])
def test_ahtree_real_and_mutants(orc, kind):
    """(a) + (b): every verdict, and the evaluated roots of every row that walks."""
    c = U.ahtree_rows(kind)
    ok = U.oracle_ahtree_ok(kind)
    ev, refused = U.oracle_ahtree_rows_eval(kind)
    go = GO_AHTREE[kind]
    got_ok = np.zeros(c.n, bool)
    evb = ev.tobytes()
    w = ev.shape[1]
    bad_eval = []
    for p, (i, j, t, a, b) in enumerate(_rows(c)):
        got_ok[p], e = go(t, i, j, a, b)
        if (e is None) != bool(refused[p]):
            bad_eval.append((p, "walk / no walk"))
        elif e is not None and e != evb[w * p:w * p + w]:
            bad_eval.append((p, "roots"))
    assert _first_bad(c, got_ok, ok) is None
    assert not bad_eval, (bad_eval[0], c.label[bad_eval[0][0]], len(bad_eval))
    # VerifyLastInclusion reads i only for i != 0: i + 1 changes nothing
    _shape(c, ok, MAY_VERIFY[kind], {"i+1"} if kind == KIND_LAST else ())
    assert refused.any() == (kind != KIND_LAST)
    big = np.array(["big tree" in x for x in c.label])
    assert big.sum() >= 300 and (c.j[big] > 65536).any()


@pytest.mark.parametrize("kind", [KIND_INCLUSION, KIND_CONSISTENCY, KIND_LAST])
def test_ahtree_walks(orc, kind):
    """(c): every evaluated root bit for bit, at i, j that no tree reaches."""
    c = U.ahtree_walks(kind)
    w, ev, ok = U.oracle_walks(kind)
    assert c.n == U.WALKS_PER_KIND + len(U.FIXED_WALKS)
    assert (c.j >= 2**63).sum() >= 20 and (c.j >= 2**60).sum() >= c.n // 20
    assert (c.i == c.j).sum() >= c.n // 3 and (c.i < c.j).sum() >= c.n // 3
    evb = ev.tobytes()
    width = ev.shape[1]
    for p, (i, j, t, a, b) in enumerate(_rows(c)):
        if kind == KIND_INCLUSION:
            e = go_eval_inclusion(t, i, j, a)
        elif kind == KIND_LAST:
            e = go_eval_last_inclusion(t, i, a)
        else:
            e = b"".join(go_eval_consistency(t, i, j))
        assert e == evb[width * p:width * p + width], (p, c.label[p])
    # and the verdicts on the rows the GPU test uses (even: the evaluated
    # roots, odd: a complemented one)
    go = GO_AHTREE[kind]
    got = [go(t, i, j, a, b)[0] for i, j, t, a, b in _rows(w)]
    assert _first_bad(w, got, ok) is None
    assert ok[::2].all() and not ok[1::2].any()


def test_htree_real_and_mutants(orc):
    """(d), with Go's truncating signed arithmetic for leaf / width >= 2^63."""
    c = U.htree_rows()
    ok = U.oracle_htree_ok()

    def signed(x):
        return x - (1 << 64) if x >> 63 else x

    got = [go_verify_inclusion(signed(i), signed(j), t, a, b) for i, j, t, a, b in _rows(c)]
    assert _first_bad(c, got, ok) is None
    _shape(c, ok, HTREE_MAY_VERIFY)
    assert set(U.HTREE_WIDTHS) == set(c.j[c.cls == "real"].tolist())


def test_linear_real_and_mutants(orc):
    """(e)"""
    c = U.linear_rows()
    ok = U.oracle_linear_ok()
    tb, off = c.terms.tobytes(), c.term_off.tolist()
    got = []
    for p in range(c.n):
        t = [tb[32 * k:32 * k + 32] for k in range(off[p], off[p + 1])]
        got.append(go_verify_linear_proof(int(c.ps[p]), int(c.pt[p]), t, int(c.s[p]), int(c.t[p]),
                                          c.sa[p].tobytes(), c.ta[p].tobytes()))
    assert _first_bad(c, got, ok) is None
    _shape(c, ok, set())  # nothing but the real chains verifies
    real = c.cls == "real"
    assert sorted(set(np.diff(c.term_off)[real].tolist())) == list(U.LINEAR_LENGTHS)
    assert (c.s[real] > 2**32).any() and (c.s[real] >= 2**63).any()
    # a chain that crosses 2^32
    assert ((c.s[real] < 2**32) & (c.t[real] > 2**32)).any()


def test_dual_v2_status_order(orc):
    """(f): the oracle's status of every row against the restated order of
    checks; every status the verifier can return appears."""
    c = U.dual_v2_rows()
    st = U.oracle_dual_v2_status()
    it, ct = c.incl.tobytes(), c.cons.tobytes()
    io, co = c.incl_off.tolist(), c.cons_off.tolist()
    got = []
    for p in range(c.n):
        incl = [it[32 * k:32 * k + 32] for k in range(io[p], io[p + 1])]
        cons = [ct[32 * k:32 * k + 32] for k in range(co[p], co[p + 1])]
        got.append(go_verify_dual_proof_v2(orc, c.sh[p], c.th[p], c.blob, incl, cons, int(c.s[p]),
                                           int(c.t[p]), c.sa[p].tobytes(), c.ta[p].tobytes()))
    assert _first_bad(c, got, st) is None
    assert set(st.tolist()) == {U.ST_OK, U.ST_ILLEGAL, U.ST_NEWER, U.ST_LINKING, U.ST_INCLUSION,
                                U.ST_CONSISTENCY}
    # two faults at once: the earlier rule's status
    for label, want in (("src_gt_tgt and wrong_src_alh", U.ST_NEWER),
                        ("wrong_src_alh and src_unlinked", U.ST_ILLEGAL),
                        ("src_unlinked and drop_incl_term", U.ST_LINKING),
                        ("drop_incl_term and drop_cons_term", U.ST_INCLUSION)):
        rows = [p for p in range(c.n) if c.label[p].startswith(label)]
        assert rows and (st[rows] == want).sum() >= len(rows) * 3 // 4, label
    # src == 1 takes the consistency check against the leaf
    assert any(c.label[p].startswith("linked DualProofV2(1, ") and st[p] == 0 for p in range(c.n))
    assert any(c.label[p].startswith("drop_cons_term of DualProofV2(1, ") and
               st[p] == U.ST_CONSISTENCY for p in range(c.n))
