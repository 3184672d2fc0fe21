"""The corpus of test_verify_mutants_cpu.py and test_gpu_verify_mutants.py: real
proofs, structural forgeries of them and synthetic walks for the four proof
verifiers (k_htree_verify, k_ahtree_verify<kind>, k_linear_verify and the
DualProofV2 status logic over them), built once per process with the C oracle
and handed out as flat arrays in the C ABI's CSR shape.

  ahtree_rows(kind)       (a) real proofs + (b) their structural mutants
  ahtree_walks(kind)      (c) synthetic walks with i, j up to 2^64 - 1
  htree_rows()            (d) every leaf of many widths + mutants
  linear_rows()           (e) chains at the length rule's edge, ids above 2^32
  dual_v2_rows()          (f) one variant per status branch, and pairs of them

Every builder is pure, seeded and cached; nobody writes into what it returns.
No row is assumed false: the verdict of each comes from the oracle
(oracle_*), and test_verify_mutants_cpu.py holds the oracle to a from-scratch
restatement of the Go source on exactly these rows.

No row can make a kernel read outside the arrays passed: offsets are
monotonic, a verifier reads only terms [term_off[p], term_off[p + 1]), and
huge i / j / leaf / width only steer selects and shifts.
"""
import functools

import numpy as np

KIND_INCLUSION, KIND_CONSISTENCY, KIND_LAST = 0, 1, 2
M64 = (1 << 64) - 1
ZERO32 = bytes(32)


def H(b):
    import hashlib
    return hashlib.sha256(b).digest()


def go_verify_inclusion(leaf, width, terms, digest, root):
    """htree.VerifyInclusion (htree.go:166-195) with Go's int arithmetic
    (truncating / and %), in Python: the checker for negative leaf / width."""
    calc = H(b"\0" + digest)
    i, r = leaf, width - 1
    tdiv = lambda x: -((-x) // 2) if x < 0 else x // 2  # noqa: E731
    for t in terms:
        # Go's % keeps the dividend's sign: -3 % 2 == -1, so "== 0" is parity
        if i % 2 == 0 and i != r:
            calc = H(b"\1" + calc + t)
        else:
            calc = H(b"\1" + t + calc)
        i, r = tdiv(i), tdiv(r)
    return i == r and calc == root


class Corpus:
    """n rows: i, j (uint64; leaf, width for the htree), term_off (n + 1),
    terms (T, 32), a, b (n, 32), label (what the row is, for messages), cls
    (its mutation class).  kinds: the verifier of each row where one corpus
    mixes them (unused otherwise)."""

    def terms_of(self, p):
        return self.terms[int(self.term_off[p]):int(self.term_off[p + 1])]

    def take(self, idx):
        """The rows idx (in that order) as a corpus of their own."""
        idx = np.asarray(idx, np.int64)
        c = Corpus()
        c.n = len(idx)
        c.i, c.j = self.i[idx].copy(), self.j[idx].copy()
        c.a, c.b = self.a[idx].copy(), self.b[idx].copy()
        nt = (self.term_off[idx + 1] - self.term_off[idx]).astype(np.uint64)
        c.term_off = np.zeros(c.n + 1, np.uint64)
        c.term_off[1:] = np.cumsum(nt)
        parts = [self.terms[int(self.term_off[p]):int(self.term_off[p + 1])] for p in idx]
        c.terms = np.ascontiguousarray(np.concatenate(parts + [np.zeros((1, 32), np.uint8)]))
        c.label = [self.label[p] for p in idx]
        c.cls = self.cls[idx]
        return c


class _Rows:
    def __init__(self):
        self.i, self.j, self.t, self.a, self.b, self.label, self.cls = [], [], [], [], [], [], []

    def add(self, cls, label, i, j, terms, a, b):
        """terms: the concatenated 32-byte terms"""
        assert len(terms) % 32 == 0 and len(a) == 32 and len(b) == 32
        self.i.append(i & M64)
        self.j.append(j & M64)
        self.t.append(terms)
        self.a.append(a)
        self.b.append(b)
        self.label.append("%s of %s" % (cls, label))
        self.cls.append(cls)

    def done(self):
        c = Corpus()
        c.n = len(self.i)
        c.i = np.array(self.i, np.uint64)
        c.j = np.array(self.j, np.uint64)
        c.term_off = np.zeros(c.n + 1, np.uint64)
        c.term_off[1:] = np.cumsum([len(t) // 32 for t in self.t], dtype=np.uint64)
        # one spare term: the array is never empty
        c.terms = np.frombuffer(b"".join(self.t) + ZERO32, np.uint8).reshape(-1, 32).copy()
        c.a = np.frombuffer(b"".join(self.a), np.uint8).reshape(-1, 32).copy()
        c.b = np.frombuffer(b"".join(self.b), np.uint8).reshape(-1, 32).copy()
        c.label = self.label
        c.cls = np.array(self.cls, dtype=object)
        return c


def _flip(b, bit=0):
    return bytes([b[0] ^ (1 << bit)]) + b[1:]


def _term_mutants(R, label, i, j, t, a, b):
    """The mutations of a proof's term list (shared by the ahtree kinds and the
    htree): t is the concatenated terms."""
    k = len(t) // 32
    if k:
        R.add("drop_first", label, i, j, t[32:], a, b)
        R.add("drop_last", label, i, j, t[:-32], a, b)
        R.add("append_copy", label, i, j, t + t[-32:], a, b)
        R.add("no_terms", label, i, j, b"", a, b)
    if k >= 3:
        m = k // 2
        R.add("drop_middle", label, i, j, t[:32 * m] + t[32 * m + 32:], a, b)
    R.add("append_zero", label, i, j, t + ZERO32, a, b)
    if k >= 2:
        for m in sorted({0, k - 2}):  # the first two and the last two
            s = t[:32 * m] + t[32 * m + 32:32 * m + 64] + t[32 * m:32 * m + 32] + t[32 * m + 64:]
            R.add("swap_adjacent", label, i, j, s, a, b)
    R.add("flip_a", label, i, j, t, _flip(a), b)
    R.add("flip_b", label, i, j, t, a, _flip(b, 7))
    for m in range(k):  # each term position in turn
        R.add("flip_term", label, i, j, t[:32 * m] + _flip(t[32 * m:32 * m + 32], m % 8) +
              t[32 * m + 32:], a, b)


# ------------------------------------------------------------------ ahtree
SMALL_N, PAIR_BOUND, TOP_J = 130, 66, (127, 128, 129, 130)
BIG_N = 70000
BIG_EDGES = (1, 2, 32767, 32768, 65535, 65536, 65537, 69999, 70000)


class _Tree:
    """An oracle AHtree over random payloads with its leaves and roots."""

    def __init__(self, n, seed, root_sizes):
        import oracle as orc
        pay = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
        self.o = orc.AHtree(n)
        self.o.append_batch(pay)
        self.pay = pay
        self._roots = {}
        for k in root_sizes:
            st, r = self.o.root_at(k)
            assert st == 0
            self._roots[k] = r

    def leaf(self, i):
        return H(b"\0" + self.pay[i - 1].tobytes())

    def root(self, n):
        return self._roots[n]

    def proofs(self, kind, pairs):
        """kind 0 / 1 -> the concatenated terms of every pair's proof"""
        I = np.array([p[0] for p in pairs], np.uint64)
        J = np.array([p[1] for p in pairs], np.uint64)
        t, nt, st = self.o.proof_batch(kind, I, J, cap=64)
        assert not st.any()
        return [t[k, :nt[k]].tobytes() for k in range(len(pairs))]


@functools.lru_cache(maxsize=None)
def small_tree():
    return _Tree(SMALL_N, 4101, range(1, SMALL_N + 1))


@functools.lru_cache(maxsize=None)
def big_pairs():
    rng = np.random.default_rng(4103)
    pairs = [(i, j) for i in BIG_EDGES for j in BIG_EDGES if i <= j]
    jj = rng.integers(1, BIG_N + 1, 300)
    return tuple(pairs + [(int(rng.integers(1, j + 1)), int(j)) for j in jj])


@functools.lru_cache(maxsize=None)
def big_tree():
    sizes = sorted({x for p in big_pairs() for x in p})
    return _Tree(BIG_N, 4102, sizes)


def small_pairs():
    return [(i, j) for j in range(1, PAIR_BOUND + 1) for i in range(1, j + 1)] + \
        [(i, j) for j in TOP_J for i in range(1, j + 1)]


@functools.lru_cache(maxsize=None)
def ahtree_rows(kind):
    """(a) + (b) for one verifier kind.  Classes: "real" (a proof as the tree
    gives it, small and big tree), the term mutations of _term_mutants, the
    index mutations i-1 / i+1 / j-1 / j+1 / swap_ij / swap_ab, "no_terms",
    "no_terms_ne" (consistency, i == j, no terms, a != b), "neighbour_terms"
    (i == j with the terms of a neighbouring pair), and the proofs of one
    verifier offered to another: "incl_as_last" / "last_as_incl" /
    "cons_as_incl"."""
    T, B = small_tree(), big_tree()
    R = _Rows()
    pairs = small_pairs()
    incl = dict(zip(pairs, T.proofs(0, pairs)))
    cons = dict(zip(pairs, T.proofs(1, pairs)))
    if kind == KIND_LAST:
        # VerifyLastInclusion(InclusionProof(j, j), j, leaf j, root j)
        for j in list(range(1, PAIR_BOUND + 1)) + list(TOP_J):
            label = "last inclusion of %d" % j
            t, a, b = incl[(j, j)], T.leaf(j), T.root(j)
            R.add("real", label, j, j, t, a, b)
            if j > PAIR_BOUND:
                continue
            _term_mutants(R, label, j, j, t, a, b)
            R.add("i-1", label, j - 1, j - 1, t, a, b)  # reaches i == 0
            R.add("i+1", label, j + 1, j + 1, t, a, b)
            R.add("swap_ab", label, j, j, t, b, a)
        # an inclusion proof of (i, j), i < j, offered as the last inclusion
        # of i and of j
        for (i, j) in pairs:
            if i < j <= PAIR_BOUND:
                label = "inclusion (%d, %d)" % (i, j)
                R.add("incl_as_last", label, i, i, incl[(i, j)], T.leaf(i), T.root(j))
                R.add("incl_as_last", label, j, j, incl[(i, j)], T.leaf(i), T.root(j))
        for (i, j), t in zip(big_pairs(), B.proofs(0, [(j, j) for _, j in big_pairs()])):
            R.add("real", "last inclusion of %d (big tree)" % j, j, j, t, B.leaf(j), B.root(j))
        return R.done()
    own = incl if kind == KIND_INCLUSION else cons
    name = "inclusion" if kind == KIND_INCLUSION else "consistency"
    for (i, j) in pairs:
        label = "%s (%d, %d)" % (name, i, j)
        t = own[(i, j)]
        a = T.leaf(i) if kind == KIND_INCLUSION else T.root(i)
        b = T.root(j)
        R.add("real", label, i, j, t, a, b)
        if j > PAIR_BOUND:
            continue
        _term_mutants(R, label, i, j, t, a, b)
        if not t:  # _term_mutants adds it only for a proof with terms
            R.add("no_terms", label, i, j, b"", a, b)
        R.add("i-1", label, i - 1, j, t, a, b)  # reaches i == 0
        R.add("i+1", label, i + 1, j, t, a, b)  # reaches i > j
        R.add("j-1", label, i, j - 1, t, a, b)  # reaches i > j, and j == 0 at (1, 1)
        R.add("j+1", label, i, j + 1, t, a, b)
        R.add("swap_ij", label, j, i, t, a, b)
        R.add("swap_ab", label, i, j, t, b, a)
        if i == j:
            nb = (j - 1, j) if j > 1 else (j, j + 1)
            R.add("neighbour_terms", label, i, j, own[nb], a, b)
            if kind == KIND_CONSISTENCY:
                # verification.go:63-65: no terms, i == j -> iRoot == jRoot
                R.add("no_terms_ne", label, i, j, b"", a, _flip(b, 3))
        if kind == KIND_INCLUSION:
            R.add("cons_as_incl", label, i, j, cons[(i, j)], a, b)
            if i < j:
                R.add("last_as_incl", label, i, j, incl[(j, j)], a, b)
    for (i, j), t in zip(big_pairs(), B.proofs(kind, list(big_pairs()))):
        a = B.leaf(i) if kind == KIND_INCLUSION else B.root(i)
        R.add("real", "%s (%d, %d) (big tree)" % (name, i, j), i, j, t, a, B.root(j))
    return R.done()


WALKS_PER_KIND = 4000
FIXED_WALKS = ((1, M64), (M64, M64), (1 << 63, 1 << 63), (1 << 32, (1 << 32) + 1),
               ((1 << 32) - 1, 1 << 32))


@functools.lru_cache(maxsize=None)
def ahtree_walks(kind):
    """(c): random terms (1..70 of them) under i, j that no tree reaches: j
    uniform in bit length 1..64, i == j / within 2^20 below j / uniform in
    [1, j] in turn, plus FIXED_WALKS.  1 <= i <= j and >= 1 term on every row,
    so Go's Eval* is defined on every row.  a is a random leaf, b is zero:
    the caller sets the roots it wants compared."""
    rng = np.random.default_rng(4200 + kind)
    R = _Rows()

    def u64(lo, hi):  # uniform in [lo, hi], Python ints (numpy stops at 2^63)
        span = hi - lo + 1
        return lo + int.from_bytes(rng.bytes(16), "big") % span

    for r in range(WALKS_PER_KIND + len(FIXED_WALKS)):
        if r < WALKS_PER_KIND:
            bits = 1 + r % 64 if r < 64 else int(rng.integers(1, 65))
            j = u64(1 << (bits - 1), (1 << bits) - 1)
            mode = r % 3
            i = j if mode == 0 else (j - u64(0, min(1 << 20, j - 1)) if mode == 1 else u64(1, j))
        else:
            i, j = FIXED_WALKS[r - WALKS_PER_KIND]
        k = int(rng.integers(1, 71))
        R.add("walk", "(%d, %d) with %d terms" % (i, j, k), i, j, rng.bytes(32 * k),
              rng.bytes(32), ZERO32)
    c = R.done()
    nt = np.diff(c.term_off)
    skipped = int(((c.i < 1) | (c.i > c.j) | (nt < 1)).sum())
    assert skipped == 0, skipped  # the cap on rows left out of the eval comparison is zero
    return c


# ------------------------------------------------------------------- htree
HTREE_WIDTHS = tuple(range(1, 34)) + (63, 64, 65, 1000, 1023, 1025)
BIT63 = 1 << 63


@functools.lru_cache(maxsize=None)
def htree_rows():
    """(d): i = leaf, j = width (the bits of Go ints), a = the entry digest,
    b = the root.  Classes: "real", _term_mutants', leaf-1 / leaf+1 / width-1 /
    width+1 / leaf_eq_width / width_0 (r = -1 in Go's signed arithmetic) /
    leaf_bit63 / width_bit63 / both_bit63."""
    import oracle as orc
    rng = np.random.default_rng(4300)
    R = _Rows()
    for w in HTREE_WIDTHS:
        d = rng.integers(0, 256, (w, 32), dtype=np.uint8)
        lv, root = orc.htree_build(d)
        for leaf in range(w):
            st, terms = orc.htree_inclusion_proof(lv, w, leaf)
            assert st == 0
            t, a = terms.tobytes(), d[leaf].tobytes()
            label = "leaf %d of width %d" % (leaf, w)
            R.add("real", label, leaf, w, t, a, root)
            _term_mutants(R, label, leaf, w, t, a, root)
            R.add("leaf-1", label, leaf - 1, w, t, a, root)  # -1 at leaf 0
            R.add("leaf+1", label, leaf + 1, w, t, a, root)
            R.add("width-1", label, leaf, w - 1, t, a, root)
            R.add("width+1", label, leaf, w + 1, t, a, root)
            R.add("leaf_eq_width", label, w, w, t, a, root)
            R.add("width_0", label, leaf, 0, t, a, root)
            R.add("leaf_bit63", label, leaf | BIT63, w, t, a, root)
            R.add("width_bit63", label, leaf, w | BIT63, t, a, root)
            R.add("both_bit63", label, leaf | BIT63, w | BIT63, t, a, root)
    return R.done()


# ------------------------------------------------------------ linear proofs
LINEAR_LENGTHS = (1, 2, 3, 64, 65, 300)
LINEAR_STARTS = (1, (1 << 32) - 2, 1 << 63)


class LinearCorpus:
    """n rows of mh_verify_linear_proof_batch's arguments: ps, pt (the proof's
    own ids), s, t, term_off, terms, sa, ta, label, cls."""


@functools.lru_cache(maxsize=None)
def linear_rows():
    """(e): chains src .. src + len - 1 of random inner hashes
    (advanceLinearHash, verification.go:32-38, through orc.tx_alh)."""
    import oracle as orc
    rng = np.random.default_rng(4400)
    rows = []

    def add(cls, label, ps, pt, terms, s, t, sa, ta):
        rows.append((cls, "%s of %s" % (cls, label), ps & M64, pt & M64, b"".join(terms), s & M64,
                     t & M64, sa, ta))

    for src in LINEAR_STARTS:
        for ln in LINEAR_LENGTHS:
            tgt = src + ln - 1
            terms = [rng.bytes(32) for _ in range(ln)]  # Alh(src), then the inner hashes
            c = terms[0]
            for k in range(1, ln):
                c = orc.tx_alh(src + k, c, terms[k])
            sa, ta = terms[0], c
            label = "chain %d..+%d" % (src, ln - 1)
            add("real", label, src, tgt, terms, src, tgt, sa, ta)
            add("drop_last", label, src, tgt, terms[:-1], src, tgt, sa, ta)  # t - s terms
            add("append", label, src, tgt, terms + [rng.bytes(32)], src, tgt, sa, ta)  # t - s + 2
            # the length rule alone: the proof that is right for tgt - 1 / tgt + 1
            add("tgt+1", label, src, tgt + 1, terms, src, tgt + 1, sa, ta)
            if ln > 1:
                add("tgt-1", label, src, tgt - 1, terms, src, tgt - 1, sa, ta)
            add("proof_src_ne", label, src + 1, tgt, terms, src, tgt, sa, ta)
            add("proof_tgt_ne", label, src, tgt + 1, terms, src, tgt, sa, ta)
            add("src_0", label, 0, ln - 1, terms, 0, ln - 1, sa, ta)
            add("src_gt_tgt", label, tgt + 1, src, terms, tgt + 1, src, sa, ta)
            if ln >= 3:
                add("swap_inner", label, src, tgt, [terms[0], terms[2], terms[1]] + terms[3:],
                    src, tgt, sa, ta)
                add("swap_inner", label, src, tgt, terms[:-2] + [terms[-1], terms[-2]],
                    src, tgt, sa, ta)
            add("first_term_ne", label, src, tgt, [_flip(terms[0])] + terms[1:], src, tgt, sa, ta)
            add("flip_src_alh", label, src, tgt, terms, src, tgt, _flip(sa), ta)
            add("flip_tgt_alh", label, src, tgt, terms, src, tgt, sa, _flip(ta, 5))
            add("no_terms", label, src, tgt, [], src, tgt, sa, ta)
    c = LinearCorpus()
    c.n = len(rows)
    c.cls = np.array([r[0] for r in rows], dtype=object)
    c.label = [r[1] for r in rows]
    c.ps = np.array([r[2] for r in rows], np.uint64)
    c.pt = np.array([r[3] for r in rows], np.uint64)
    c.term_off = np.zeros(c.n + 1, np.uint64)
    c.term_off[1:] = np.cumsum([len(r[4]) // 32 for r in rows], dtype=np.uint64)
    c.terms = np.frombuffer(b"".join(r[4] for r in rows) + ZERO32, np.uint8).reshape(-1, 32).copy()
    c.s = np.array([r[5] for r in rows], np.uint64)
    c.t = np.array([r[6] for r in rows], np.uint64)
    c.sa = np.frombuffer(b"".join(r[7] for r in rows), np.uint8).reshape(-1, 32).copy()
    c.ta = np.frombuffer(b"".join(r[8] for r in rows), np.uint8).reshape(-1, 32).copy()
    return c


# ------------------------------------------------------------- DualProofV2
DUAL_V2_PAIRS = 300
# every status VerifyDualProofV2 (verification.go:304-372) can return
ST_OK, ST_ILLEGAL, ST_NEWER, ST_LINKING, ST_INCLUSION, ST_CONSISTENCY = 0, 2, 10, 11, 12, 13


class DualCorpus:
    """n rows of mh_verify_dual_proof_v2_batch's arguments: sh, th (TX_HEADER
    records over blob), incl_off / incl, cons_off / cons, s, t, sa, ta, label."""


@functools.lru_cache(maxsize=None)
def dual_v2_rows():
    """(f) over dual_v1_gen_util.synthetic_store(): the first DUAL_V2_PAIRS of
    synthetic_pairs() as they are, and each again moved onto txs whose
    BlTxID is id - 1 (the store's txs 1 and 4k outside its two plateaus: the
    only ones VerifyDualProofV2's linking rule accepts), the proof assembled
    as ImmuStore.DualProofV2 does (immustore.go:2374-2384).  On the linked
    pairs one variant per branch of the verifier, then two at once."""
    from dual_v1_gen_util import bl_of, synthetic_pairs, synthetic_store
    S = synthetic_store()
    aht = S.aht

    def proof(fn, i, j):
        st, t = fn(i, j)
        assert st == 0, (i, j, st)
        return t.tobytes()

    def linked(k):  # the nearest tx at or below k with bl_tx_id == id - 1
        while k > 1 and bl_of(k) != k - 1:
            k -= 1
        return k

    rows = []

    def add(label, sh, th, incl, cons, s, t, sa, ta):
        rows.append((label, sh, th, incl, cons, s, t, sa, ta))

    def base(s, t):
        """DualProofV2(s, t)'s parts, whatever the linking of s and t"""
        sh, th = S.crecs[s - 1].copy(), S.crecs[t - 1].copy()
        incl = cons = b""
        bl = int(th["bl_tx_id"])
        if s < t and 1 <= s <= bl:
            incl = proof(aht.inclusion_proof, s, bl)
            if max(1, int(sh["bl_tx_id"])) <= bl:
                cons = proof(aht.consistency_proof, max(1, int(sh["bl_tx_id"])), bl)
        return sh, th, incl, cons, S.alhs[s - 1], S.alhs[t - 1]

    def hdr(h, **kw):
        h = h.copy()
        for f, v in kw.items():
            h[f] = v
        return h

    # name -> the row (label, sh, th, incl, cons, s, t, sa, ta) changed
    def variants(s, t):
        sh, th, incl, cons, sa, ta = base(s, t)
        junk = bytes(range(32)) * 3
        V = {
            "wrong_src_alh": lambda r: r[:7] + (_flip(r[7]), r[8]),
            "wrong_tgt_alh": lambda r: r[:8] + (_flip(r[8]),),
            # a header whose id - 1 != bl_tx_id, with the Alh that goes with it
            "src_unlinked": lambda r: _rehash(r, 1, bl_tx_id=int(r[1]["bl_tx_id"]) + 1),
            "tgt_unlinked": lambda r: _rehash(r, 2, bl_tx_id=int(r[2]["bl_tx_id"]) + 1),
            "drop_incl_term": lambda r: r[:3] + (r[3][:-32], ) + r[4:],
            "drop_cons_term": lambda r: r[:4] + (r[4][:-32], ) + r[5:],
            "lists_exchanged": lambda r: r[:3] + (r[4], r[3]) + r[5:],
            "src_gt_tgt": lambda r: (r[0], r[2], r[1], r[3], r[4], r[6], r[5], r[8], r[7]),
            "src_hdr_id_ne": lambda r: (r[0], hdr(r[1], id=int(r[1]["id"]) + 1)) + r[2:],
            "tgt_hdr_id_ne": lambda r: (r[0], r[1], hdr(r[2], id=int(r[2]["id"]) + 1)) + r[3:],
            "src_hdr_id_0": lambda r: (r[0], hdr(r[1], id=0)) + r[2:5] + (0,) + r[6:],
            "junk_terms": lambda r: r[:3] + (junk, junk) + r[5:],
        }
        return ("DualProofV2(%d, %d)" % (s, t), sh, th, incl, cons, s, t, sa, ta), V

    def _rehash(r, which, **kw):
        import oracle as orc
        h = hdr(r[which], **kw)
        st, _, alh = orc.tx_header_alh(h, S.cblob)
        assert st == 0
        out = list(r)
        out[which] = h
        out[6 + which] = alh
        return tuple(out)

    pairs = synthetic_pairs()[:DUAL_V2_PAIRS]
    order = ["wrong_src_alh", "wrong_tgt_alh", "src_unlinked", "tgt_unlinked", "drop_incl_term",
             "drop_cons_term", "lists_exchanged", "src_gt_tgt", "src_hdr_id_ne", "tgt_hdr_id_ne",
             "src_hdr_id_0", "junk_terms"]
    # two at once, the rule that must win first: (earlier, later)
    both = [("src_gt_tgt", "wrong_src_alh"), ("src_hdr_id_ne", "src_gt_tgt"),
            ("wrong_src_alh", "src_unlinked"), ("wrong_tgt_alh", "tgt_unlinked"),
            ("wrong_src_alh", "wrong_tgt_alh"), ("src_unlinked", "drop_incl_term"),
            ("tgt_unlinked", "junk_terms"), ("drop_incl_term", "drop_cons_term"),
            ("wrong_tgt_alh", "drop_incl_term"), ("src_unlinked", "tgt_unlinked"),
            ("lists_exchanged", "drop_cons_term"), ("src_hdr_id_0", "wrong_src_alh")]
    k = 0
    for (s0, t0) in pairs:
        r, _ = variants(s0, t0)
        add("as stored " + r[0], *r[1:])
        s, t = linked(s0), linked(t0)
        r, V = variants(s, t)
        add("linked " + r[0], *r[1:])
        name = order[k % len(order)]
        add(name + " of " + r[0], *V[name](r)[1:])
        n1, n2 = both[k % len(both)]
        # a re-hashed header goes in first: it brings its own Alh along
        f1, f2 = sorted((n1, n2), key=lambda x: not x.endswith("_unlinked"))
        add("%s and %s of %s" % (n1, n2, r[0]), *V[f2](V[f1](r))[1:])
        k += 1
    # src == tgt with junk terms, src == 1 (the consistency check against the
    # leaf, verification.go:348-357) and src == tgt == 1, each with variants
    for s, t in ((1, 4), (1, 1000), (1, 1), (8, 8), (1000, 1000), (1, 2996), (4, 8), (196, 1000)):
        r, V = variants(s, t)
        add("linked " + r[0], *r[1:])
        for name in order:
            add(name + " of " + r[0], *V[name](r)[1:])
    c = DualCorpus()
    c.n = len(rows)
    c.label = [r[0] for r in rows]
    c.sh = np.array([r[1] for r in rows], dtype=S.crecs.dtype)
    c.th = np.array([r[2] for r in rows], dtype=S.crecs.dtype)
    c.blob = S.cblob
    for name, col in (("incl", 3), ("cons", 4)):
        off = np.zeros(c.n + 1, np.uint64)
        off[1:] = np.cumsum([len(r[col]) // 32 for r in rows], dtype=np.uint64)
        setattr(c, name + "_off", off)
        setattr(c, name, np.frombuffer(b"".join(r[col] for r in rows) + ZERO32,
                                       np.uint8).reshape(-1, 32).copy())
    c.s = np.array([r[5] for r in rows], np.uint64)
    c.t = np.array([r[6] for r in rows], np.uint64)
    c.sa = np.frombuffer(b"".join(r[7] for r in rows), np.uint8).reshape(-1, 32).copy()
    c.ta = np.frombuffer(b"".join(r[8] for r in rows), np.uint8).reshape(-1, 32).copy()
    return c


# ------------------------------------------------------- the oracle's answers
@functools.lru_cache(maxsize=None)
def oracle_ahtree_ok(kind):
    import oracle as orc
    c = ahtree_rows(kind)
    return orc.ahtree_verify_batch(kind, c.i, c.j, c.term_off, c.terms, c.a, c.b, 4)[1].astype(bool)


def ahtree_refused(c, kind):
    """The rows a verifier answers without a walk (verification.go:22-24,
    :59-65): i > j, i == 0, i < j without terms; for the consistency kind also
    i == j without terms (iRoot == jRoot decides).  VerifyLastInclusion always
    walks."""
    if kind == KIND_LAST:
        return np.zeros(c.n, bool)
    nt = np.diff(c.term_off)
    bad = (c.i > c.j) | (c.i == 0) | ((c.i < c.j) & (nt == 0))
    if kind == KIND_CONSISTENCY:
        bad |= (c.i == c.j) & (nt == 0)
    return bad


def ahtree_eval_expected(c, kind):
    """What eval_out must hold on every row (include/immustore_merkle.h): Go's
    Eval* where the verifier walks (the oracle's, which must be defined
    there), and on a refused row the leaf a[p] unchanged (inclusion) or 64
    zero bytes (consistency)."""
    import oracle as orc
    ev, defined = orc.ahtree_eval_batch(kind, c.i, c.j, c.term_off, c.terms, c.a)
    refused = ahtree_refused(c, kind)
    assert defined[~refused].all()
    ev = ev.copy()
    ev[refused] = c.a[refused] if kind == KIND_INCLUSION else 0
    return ev, refused


@functools.lru_cache(maxsize=None)
def oracle_ahtree_rows_eval(kind):
    return ahtree_eval_expected(ahtree_rows(kind), kind)


@functools.lru_cache(maxsize=None)
def oracle_walks(kind):
    """(c) completed: the oracle's evaluated roots of every walk, and the
    corpus with a / b set so that even rows verify (the evaluated roots) and
    odd rows do not (the complement of one of them) -> (corpus, eval, ok)."""
    import oracle as orc
    c = ahtree_walks(kind)
    ev, defined = orc.ahtree_eval_batch(kind, c.i, c.j, c.term_off, c.terms, c.a)
    assert defined.all()
    w = Corpus()
    w.__dict__.update(c.__dict__)
    odd = (np.arange(c.n) % 2 == 1)
    if kind == KIND_CONSISTENCY:
        w.a, w.b = ev[:, :32].copy(), ev[:, 32:].copy()
        w.a[odd & (np.arange(c.n) % 4 == 1)] ^= 0xFF  # the first root wrong
        w.b[odd & (np.arange(c.n) % 4 == 3)] ^= 0xFF  # the second root wrong
    else:
        w.b = ev.copy()
        w.b[odd] ^= 0xFF
    ok = orc.ahtree_verify_batch(kind, w.i, w.j, w.term_off, w.terms, w.a, w.b, 4)[1].astype(bool)
    assert (ok == ~odd).all()
    return w, ev, ok


@functools.lru_cache(maxsize=None)
def oracle_htree_ok():
    import oracle as orc
    c = htree_rows()
    return orc.htree_verify_csr(c.i, c.j, c.term_off, c.terms, c.a, c.b, 4)[1].astype(bool)


@functools.lru_cache(maxsize=None)
def oracle_linear_ok():
    import oracle as orc
    c = linear_rows()
    return np.array([orc.verify_linear_proof(
        int(c.ps[p]), int(c.pt[p]), c.terms[int(c.term_off[p]):int(c.term_off[p + 1])],
        int(c.s[p]), int(c.t[p]), c.sa[p], c.ta[p]) for p in range(c.n)], bool)


@functools.lru_cache(maxsize=None)
def oracle_dual_v2_status():
    import oracle as orc
    c = dual_v2_rows()
    return np.array([orc.verify_dual_proof_v2(
        c.sh[p], c.th[p], c.blob, c.incl[int(c.incl_off[p]):int(c.incl_off[p + 1])],
        c.cons[int(c.cons_off[p]):int(c.cons_off[p + 1])], int(c.s[p]), int(c.t[p]),
        c.sa[p], c.ta[p]) for p in range(c.n)], np.int32)
