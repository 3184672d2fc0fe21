"""Case lists and oracle models for the call-sequence tests
(test_gpu_call_sequences.py on the device, test_call_sequences_cpu.py for the
lists themselves): what one mh_ahtree, one mh_htree and one mh_ctx carry from
a call to the next.

Every expectation is the oracle's on the LOGICAL input of a step -- for an
ahtree step a fresh oracle.AHtree fed the surviving payloads and then the new
ones, for an htree build the oracle's build of that build's entries alone --
never an earlier result of the library.
"""
import numpy as np

SORT_MIN = 16384            # the length-class sort starts here (varlen_kernels.hip)
HT_MAX_WIDTH = SORT_MIN + 7

MH_OK = 0
MH_ERR_MAX_WIDTH_EXCEEDED = 1
MH_ERR_ILLEGAL_ARGUMENTS = 2
MH_ERR_UNEXISTENT_DATA = 5
MH_ERR_METADATA_UNSUPPORTED = 6


def first_diff(got, want, unit=32):
    """Index of the first `unit`-byte record in which two byte strings differ
    (None when equal), for the assertion messages."""
    if got == want:
        return None
    if len(got) != len(want):
        return ("length", len(got), len(want))
    a = np.frombuffer(got, np.uint8).reshape(-1, unit)
    b = np.frombuffer(want, np.uint8).reshape(-1, unit)
    return int(np.nonzero((a != b).any(axis=1))[0][0])


# ===================================================================== A: ahtree
def nodes_upto(n):
    """ahtree.go:492-511: append k writes 1 + popcount(k - 1) nodes."""
    return n + sum(bin(k).count("1") for k in range(n))


AHT_K = 11  # resets land on 2^11 - 1, 2^11 and 2^11 + 1 once the tree has passed 2^11
AHT_RESET_CLASSES = ("zero", "one", "pow2-1", "pow2", "pow2+1", "size-1", "size")
AHT_MAX_LEAVES = 5200


def ahtree_steps():
    """The life of one mh_ahtree as a list of steps.  Append steps:
    dict(op = append | batch | batch_roots | logs, m, plen, seed, n0, hi,
    ends, grows [, p_off0]); reset steps: dict(op = reset, to, cls, n0, hi).

      n0     the size before the step
      hi     the largest size the handle has had before the step: its dLog
             holds nodes of earlier appends up to there
      cut    the size just before the latest reset (0: none yet); after several
             resets it lies below hi
      ends   where an append that starts below hi ends: "before", "on" or
             "past" hi (None: it starts at or above hi, on untouched memory)
      grows  the append needs more dLog than the handle has (aht_reserve:
             capacity max(need, 2 * capacity), the live part alone copied)
    """
    steps = []
    st = dict(size=0, hi=0, cap=0, seed=100, cut=0)

    def app(op, m, plen=32, **kw):
        n0, hi = st["size"], st["hi"]
        end = n0 + m
        ends = None
        if n0 < hi:
            ends = "before" if end < hi else "on" if end == hi else "past"
        need = nodes_upto(end)
        grows = need > st["cap"]
        if grows:
            st["cap"] = max(need, 2 * st["cap"])
        st["seed"] += 1
        steps.append(dict(op=op, m=m, plen=plen, seed=st["seed"], n0=n0, hi=hi, cut=st["cut"],
                          ends=ends, grows=grows, **kw))
        st["size"] = end
        st["hi"] = max(hi, end)
        assert end <= AHT_MAX_LEAVES

    def reset(to, cls):
        assert to <= st["size"]
        st["cut"] = st["size"]
        steps.append(dict(op="reset", to=to, cls=cls, n0=st["size"], hi=st["hi"], cut=st["cut"]))
        st["size"] = to

    P = 1 << AHT_K
    app("batch_roots", 300)
    app("append", 1)
    app("append", 1)
    app("logs", 700, p_off0=0)
    app("batch", 1100)                      # 2102 > 2^11
    reset(st["size"] - 1, "size-1")
    app("batch_roots", 1)                   # on
    reset(P + 1, "pow2+1")
    app("batch", 20)                        # before
    app("batch_roots", 33)                  # on (2102)
    app("batch", 10)                        # fresh memory
    reset(P, "pow2")
    app("logs", 100, p_off0=36 * 2048)      # past (2148 > 2112)
    reset(P - 1, "pow2-1")
    app("append", 1)                        # before
    app("batch_roots", 64)                  # before
    reset(1, "one")
    app("batch", 500, plen=50)              # a variable-size batch after fixed ones
    app("logs", 40, plen=1, p_off0=7)
    reset(0, "zero")
    app("batch_roots", 2148)                # on
    reset(st["size"], "size")               # a no-op
    app("batch", 5)
    reset(100, "mid")
    app("batch", 5100)                      # past, and the dLog has to move
    reset(4097, "pow2+1")
    app("append", 1)
    app("batch_roots", 3, plen=0)           # empty payloads
    return steps


def payloads(orc, step):
    m, plen = step["m"], step["plen"]
    if plen == 0:
        return np.zeros((m, 0), np.uint8)
    return orc.fill_random(m * plen, step["seed"]).reshape(m, plen)


def oracle_tree(orc, segments, cap=1024):
    """A fresh oracle tree fed the logical payloads (a list of (m, plen)
    arrays) in order."""
    o = orc.AHtree(cap)
    for s in segments:
        if s.shape[0]:
            o.append_batch(s)
    return o


def truncate(segments, size):
    out, left = [], size
    for s in segments:
        if left <= 0:
            break
        out.append(s[:left])
        left -= out[-1].shape[0]
    assert left == 0
    return out


def proof_rows(size, extra_js, seed):
    """About 16 (i, j) with 1 <= i <= j <= size spread over the tree, then one
    row per j of extra_js (size + 1, the largest size the handle has had,
    the size just before the latest reset) -> (i[], j[])."""
    rng = np.random.default_rng(seed)
    I, J = [], []
    if size:
        js = np.unique(np.concatenate([np.linspace(1, size, 8).astype(np.int64),
                                       rng.integers(1, size + 1, 6), [size, size]]))
        for j in js:
            for i in {1, int(j), int(rng.integers(1, j + 1))}:
                I.append(i)
                J.append(int(j))
        I, J = I[-18:], J[-18:]
    for j in extra_js:
        I.append(max(1, min(size, j) // 2))
        J.append(int(j))
    return np.array(I, np.uint64), np.array(J, np.uint64)


def ahtree_model(orc, steps):
    """Per step the oracle's view: dict(size, dlog, root, roots (the batch's,
    (m, 32) bytes or None), plog, clog, stale (the node digests of the part
    the last reset cut off, as a set), prev_size)."""
    segs, out, stale_src = [], [], None
    for s in steps:
        prev_size = sum(x.shape[0] for x in segs)
        e = dict(prev_size=prev_size, roots=None, plog=None, clog=None)
        if s["op"] == "reset":
            before = oracle_tree(orc, segs).dlog_bytes()
            segs = truncate(segs, s["to"])
            stale_src = before
        else:
            p = payloads(orc, s)
            segs = segs + [p]
        o = oracle_tree(orc, segs)
        e["size"] = o.size
        e["dlog"] = o.dlog_bytes()
        e["root"] = o.root_at(o.size)[1] if o.size else None
        if s["op"] in ("batch_roots", "append"):
            e["roots"] = b"".join(o.root_at(n)[1] for n in range(prev_size + 1, o.size + 1))
        if s["op"] == "logs":
            # the records are a function of the batch alone
            e["plog"], e["clog"] = orc.AHtree(1).append_batch_logs(p, s["p_off0"])
        cut = len(e["dlog"])
        tail = stale_src[cut:] if stale_src is not None else b""
        e["stale"] = {tail[k:k + 32] for k in range(0, len(tail), 32)}
        e["oracle"] = o
        out.append(e)
    return out


AHT_BIG = (1 << 19) + 5     # one level of >= 2^18 new perfect nodes: k_aht_perfect_t


def ahtree_big_model(orc):
    """(1 << 19) + 5 payloads, reset to 3, as many different payloads in one
    batch -> (first payloads, second payloads, dLog bytes, last root)."""
    a = orc.fill_random(AHT_BIG * 32, 9001).reshape(AHT_BIG, 32)
    b = orc.fill_random(AHT_BIG * 32, 9002).reshape(AHT_BIG, 32)
    o = orc.AHtree(AHT_BIG + 3)
    o.append_batch(a[:3])
    o.append_batch(b)
    return a, b, o.dlog_bytes(), o.root_at(o.size)[1]


# ====================================================================== B: htree
HT_WIDTHS = (4096, 3, 0, 1, 257, 2, 4095, HT_MAX_WIDTH, 5, 1000)
HT_FORMS = ("with", "fixed", "csr_md", "csr_ov", "csr", "v0")
HT_CSR_FORMS = ("csr_md", "csr_ov", "csr", "v0")   # build_csr: sorted from SORT_MIN entries on


def _euler_forms():
    """Every ordered pair of different forms once: an Euler circuit of the
    complete digraph over HT_FORMS (Hierholzer), 31 builds."""
    k = len(HT_FORMS)
    out_edges = {a: [b for b in range(k) if b != a] for a in range(k)}
    stack, circuit = [2], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop(0))
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return [HT_FORMS[i] for i in circuit]


def htree_builds():
    """dict(form, n, seed) per build: the forms in an order where each is
    followed by each other, the widths of HT_WIDTHS in turn."""
    forms = _euler_forms()
    return [dict(form=f, n=HT_WIDTHS[k % len(HT_WIDTHS)], seed=500 + k)
            for k, f in enumerate(forms)]


# calls that must fail between builds (every status one a well-formed caller
# can provoke) -- after each, the tree is still the last good build's
HT_FAILURES = (("max_width", MH_ERR_MAX_WIDTH_EXCEEDED),
               ("v0_metadata", MH_ERR_METADATA_UNSUPPORTED),
               ("key_off_backwards", MH_ERR_ILLEGAL_ARGUMENTS))


def htree_inputs(orc, b):
    """The inputs of one build -> dict(form, n, version, digests | keys, mds,
    vals, overrides (None or a list), vals_sent)."""
    n, form = b["n"], b["form"]
    rng = np.random.default_rng(b["seed"])
    if form == "with":
        d = orc.fill_random(max(n, 1) * 32, b["seed"]).reshape(-1, 32)[:n]
        return dict(form=form, n=n, digests=d)
    version = 0 if form == "v0" else 1
    if form == "fixed":
        kb = orc.fill_random(max(n, 1) * 8, b["seed"]).reshape(-1, 8)[:n]
        vb = orc.fill_random(max(n, 1) * 128, b["seed"] + 7000).reshape(-1, 128)[:n]
        keys = [x.tobytes() for x in kb]
        vals = [x.tobytes() for x in vb]
        return dict(form=form, n=n, version=1, keys=keys, mds=None, vals=vals, overrides=None,
                    vals_sent=vals)
    kl = rng.integers(1, 40, n)
    vl = rng.integers(0, 200, n)
    kbuf = orc.fill_random(int(kl.sum()) + 1, b["seed"] + 1)
    vbuf = orc.fill_random(int(vl.sum()) + 1, b["seed"] + 2)
    ko = np.concatenate([[0], np.cumsum(kl)])
    vo = np.concatenate([[0], np.cumsum(vl)])
    keys = [kbuf[ko[i]:ko[i + 1]].tobytes() for i in range(n)]
    vals = [vbuf[vo[i]:vo[i + 1]].tobytes() for i in range(n)]
    mds, ov, sent = None, None, vals
    if form == "csr_md":
        ml = rng.integers(0, 12, n)
        if n:
            ml[0] = 3          # never all empty: md_bytes > 0
        mbuf = orc.fill_random(int(ml.sum()) + 1, b["seed"] + 3)
        mo = np.concatenate([[0], np.cumsum(ml)])
        mds = [mbuf[mo[i]:mo[i + 1]].tobytes() for i in range(n)]
    if form == "csr_ov":
        pick = rng.random(n) < 0.2
        if n:
            pick[n // 2] = True  # at least one, so the override arrays are staged
        ov = [orc.sha256(v) if pick[i] else None for i, v in enumerate(vals)]
        sent = [b"" if o is not None else v for o, v in zip(ov, vals)]
    return dict(form=form, n=n, version=version, keys=keys, mds=mds, vals=vals, overrides=ov,
                vals_sent=sent)


def htree_expect(orc, inp):
    """The oracle's build of these inputs alone -> (hvals or None, levels
    (L, 32), root)."""
    n = inp["n"]
    if inp["form"] == "with":
        lv, root = orc.htree_build(inp["digests"])
        return None, lv, root
    st, hv, lv, root = orc.build_entries(inp["version"], inp["keys"], inp["mds"] or [b""] * n,
                                         inp["vals"])
    assert st == 0
    return hv, lv, root


def htree_leaves(n, prev_n, seed):
    """Leaves to prove: all of them up to 257, else 64 sampled plus the first
    and the last; then leaf = width and leaf = the previous width."""
    if n <= 257:
        inside = np.arange(n, dtype=np.uint64)
    else:
        rng = np.random.default_rng(seed)
        inside = np.concatenate([rng.integers(0, n, 64), [0, n - 1]]).astype(np.uint64)
    return np.concatenate([inside, np.array([n, prev_n], np.uint64)])


def htree_proof_expect(orc, lv, n, leaf):
    """(*HTree).InclusionProof (htree.go:121-164): ErrIllegalArguments for a
    leaf outside the tree (:122-124, checked before the oracle's walk), else
    the oracle's terms -> (status, terms bytes)."""
    if leaf >= n:
        return MH_ERR_ILLEGAL_ARGUMENTS, b""
    st, t = orc.htree_inclusion_proof(lv, n, int(leaf))
    return st, t.tobytes()


# =============================================================== C: one context
# Per scratch group the sizes of its calls in order; "members" names the
# entry point of each call.  The CPU companion checks the large -> small ->
# large shape and the sort threshold; the GPU test draws the inputs.
# The groups whose inputs come from the suite's corpora are CTX2_GROUPS below.
CTX_GROUPS = {
    "s_msgs": dict(
        members=("htree_verify", "ahtree_verify_incl", "ahtree_verify_cons", "ahtree_verify_last",
                 "verify_values", "htree_verify", "ahtree_verify_cons", "verify_values",
                 "htree_verify"),
        sizes=(3000, 2000, 40, 2500, 2000, 7, 1800, 5, 3000)),
    "s_sort": dict(
        members=("dev_sha256", "verify_values", "dev_sha256", "verify_values", "dev_sha256",
                 "verify_values"),
        sizes=(20001, 20001, 100, 100, SORT_MIN, SORT_MIN)),
    "s_tx": dict(
        members=("tx_alh", "build_many_packed", "build_many_planned", "tx_alh", "build_many_packed",
                 "tx_alh"),
        sizes=(6000, 2500, 30, 3, 2100, 5000)),
}
# the order the groups' calls are interleaved in: (group, index in the group)
CTX_ORDER = (("s_msgs", 0), ("s_sort", 0), ("s_tx", 0), ("s_msgs", 1), ("s_sort", 1), ("s_tx", 1),
             ("s_msgs", 2), ("s_tx", 2), ("s_sort", 2), ("s_msgs", 3), ("s_tx", 3), ("s_sort", 3),
             ("s_msgs", 4), ("s_sort", 4), ("s_tx", 4), ("s_msgs", 5), ("s_sort", 5), ("s_tx", 5),
             ("s_msgs", 6), ("s_msgs", 7), ("s_msgs", 8))


# The second interleaving: the groups fed from the suite's own corpora.  A call
# is (member, n, keywords); n is what grows the group's scratch (messages,
# txs, requests, records).
TXLOG_BULK = 9000   # tx_util._bulk_txlog records: past 16 MiB, where the log is cut in chunks
CTX2_GROUPS = {
    "s_tx": dict(calls=(
        ("dual_v1_pb", 2000, {}), ("dual_v2_pb", 4, {}), ("ventry_pb", 600, {}),
        ("vtx_pb", 3, {}), ("replicate", 150, {}), ("dual_v1_pb", 5, {}),
        ("vtx_pb", 500, {}), ("ventry_pb", 2, {}), ("dual_v2_pb", 240, {}),
        ("replicate", 3, {}), ("dual_v1_pb", 2000, {}))),
    "s_ventry": dict(calls=(
        ("ventry_pb", 700, {}), ("replicate", 2, {}), ("ventry_pb", 1, {}),
        ("replicate", 140, {}), ("ventry_pb", 650, {}))),
    "s_msgs": dict(calls=(
        ("documents", 900, {}), ("documents", 3, {}), ("documents", 800, {}))),
    "s_ans": dict(calls=(
        ("verifiable_answers", 700, {}), ("tx_answers", 6, {}),
        ("verifiable_answers", 40, dict(hint=True)), ("tx_answers", 1500, {}),
        ("verifiable_answers", 5, {}), ("verifiable_answers", 720, dict(hint=True)))),
    "s_exp": dict(calls=(
        ("export", 46, dict(first=1, arm="A")), ("export", 1, dict(first=5, arm="A")),
        ("export", 16, dict(first=41, arm="A")), ("export", 46, dict(first=1, arm="B")),
        ("export", 1, dict(first=7, arm="B")), ("export", 16, dict(first=41, arm="B")))),
    "s_txg": dict(calls=(
        ("txlog_chunks", TXLOG_BULK, dict(weights="1:1:1")),
        ("clog", 50, dict(mode="host", width=4)),
        ("txlog_chunks", TXLOG_BULK, dict(weights="1")),
        ("clog", 200, dict(mode="dev", width=300)),
        ("txlog_chunks", TXLOG_BULK, dict(weights="1:1")),
        ("clog", 200, dict(mode="host", width=300)),
        ("clog", 200, dict(mode="dev", width=2)),       # narrower: the guess is too wide
        ("clog", 200, dict(mode="dev", width=300)))),   # wider again: the guess is too narrow
}
CTX2_REQUIRED = {
    "s_tx": {"dual_v2_pb", "dual_v1_pb", "ventry_pb", "vtx_pb", "replicate"},
    "s_ventry": {"ventry_pb", "replicate"},
    "s_msgs": {"documents"},
    "s_ans": {"verifiable_answers", "tx_answers"},
    "s_exp": {"export"},
    "s_txg": {"txlog_chunks", "clog"},
}


def _round_robin(groups):
    order, k = [], 0
    while any(k < len(g["calls"]) for g in groups.values()):
        order += [(name, k) for name, g in groups.items() if k < len(g["calls"])]
        k += 1
    return tuple(order)


CTX2_ORDER = _round_robin(CTX2_GROUPS)


# =========================================================== D: asynchronous chains
QUEUED_BUILD_NS = (1, 700, SORT_MIN - 1, SORT_MIN, 20000, 17000, SORT_MIN + 1, SORT_MIN - 1, 2049,
                   64, 5, 3)
