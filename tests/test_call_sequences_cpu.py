"""The case lists of tests/call_sequence_util.py cover what the call-sequence
tests are for, and the oracle model behind them is consistent with itself.
No GPU: the lists and the oracle alone."""
import call_sequence_util as U


# ------------------------------------------------------------------ A: ahtree
def test_ahtree_steps_cover_every_reset_class():
    steps = U.ahtree_steps()
    resets = [s for s in steps if s["op"] == "reset"]
    assert {s["cls"] for s in resets} >= set(U.AHT_RESET_CLASSES)
    P = 1 << U.AHT_K
    for s in resets:
        want = {"zero": 0, "one": 1, "pow2-1": None, "pow2": None, "pow2+1": None,
                "size-1": s["n0"] - 1, "size": s["n0"], "mid": s["to"]}[s["cls"]]
        if want is not None:
            assert s["to"] == want, s
        else:
            k = {"pow2-1": -1, "pow2": 0, "pow2+1": 1}[s["cls"]]
            p = s["to"] - k
            assert p & (p - 1) == 0 and p >= P and s["hi"] > p, s  # a power the tree has passed
        assert s["to"] <= s["n0"]
    assert {s["to"] for s in resets} >= {P - 1, P, P + 1}
    # every reset but the no-op is followed by an append of other payloads
    for k, s in enumerate(steps[:-1]):
        if s["op"] == "reset":
            assert steps[k + 1]["op"] != "reset"
    seeds = [s["seed"] for s in steps if s["op"] != "reset"]
    assert len(set(seeds)) == len(seeds)


def test_ahtree_steps_cover_batch_ends_and_forms():
    steps = U.ahtree_steps()
    apps = [s for s in steps if s["op"] != "reset"]
    assert {s["op"] for s in apps} == {"append", "batch", "batch_roots", "logs"}
    assert {s["ends"] for s in apps} == {None, "before", "on", "past"}
    # one re-append after a reset outgrows the dLog (aht_reserve moves it)
    assert any(s["grows"] and s["ends"] == "past" for s in apps)
    # a variable-size batch after a fixed one, and 32-byte payloads
    plens = [s["plen"] for s in apps]
    assert plens[0] == 32 and any(p not in (0, 32) for p in plens)
    k = next(i for i, p in enumerate(plens) if p != 32)
    assert 32 in plens[k + 1:]
    # logs after a reset, roots after a reset
    assert any(s["op"] == "logs" and s["ends"] for s in apps)
    assert any(s["op"] == "batch_roots" and s["ends"] for s in apps)
    size = 0
    for s in steps:
        assert s["n0"] == size
        size = s["to"] if s["op"] == "reset" else size + s["m"]
        assert size <= U.AHT_MAX_LEAVES


def test_nodes_upto_matches_oracle(orc):
    for n in (0, 1, 2, 3, 100, 2047, 2048, 2049, 5200):
        assert U.nodes_upto(n) == orc.nodes_upto(n)


def test_ahtree_model_consistent_with_stepwise_oracle(orc):
    """The fresh oracle of every step (prefix + suffix in one go) equals an
    oracle that lives through the steps one append at a time, re-made only at
    a reset; roots, records and proof rows hang together."""
    steps = U.ahtree_steps()
    model = U.ahtree_model(orc, steps)
    live, segs = orc.AHtree(), []
    for k, (s, e) in enumerate(zip(steps, model)):
        if s["op"] == "reset":
            segs = U.truncate(segs, s["to"])
            live = U.oracle_tree(orc, segs)
            assert e["size"] == s["to"]
            # what the reset cut off is stale, and none of it is in the tree
            assert len(e["stale"]) > 0 or s["cls"] == "size"
        else:
            p = U.payloads(orc, s)
            segs.append(p)
            if s["op"] == "append":
                assert live.append(p[0].tobytes()) == e["roots"]
            else:
                live.append_batch(p)
        assert live.size == e["size"] == s["n0"] + (s.get("m", 0) if s["op"] != "reset" else
                                                     s["to"] - s["n0"])
        assert live.dlog_bytes() == e["dlog"], k
        if e["size"]:
            assert live.root_at(e["size"])[1] == e["root"]
        if e["roots"] is not None:
            assert e["roots"][-32:] == e["root"] and len(e["roots"]) == 32 * s["m"]
        if s["op"] == "logs":
            assert len(e["plog"]) == s["m"] * (4 + s["plen"]) and len(e["clog"]) == s["m"] * 12
        I, J = U.proof_rows(e["size"], [e["size"] + 1, s["hi"], s["cut"]], k)
        assert len(I) <= 21 and (I >= 1).all() and (I[:-3] <= J[:-3]).all()
        assert e["size"] < 100 or len(I) >= 15  # about 16 rows and the three extra ones
        _, _, st = e["oracle"].proof_batch(0, I, J)
        assert not st[:-3].any() and st[-3] == U.MH_ERR_UNEXISTENT_DATA
        if s["hi"] > e["size"]:  # j = the largest size so far: no longer there
            assert st[-2] == U.MH_ERR_UNEXISTENT_DATA
        if s["cut"] > e["size"]:  # j = the size just before the latest reset
            assert st[-1] == U.MH_ERR_UNEXISTENT_DATA


# ------------------------------------------------------------------- B: htree
def test_htree_builds_cover_every_order():
    builds = U.htree_builds()
    forms = [b["form"] for b in builds]
    pairs = set(zip(forms, forms[1:]))
    assert pairs == {(a, b) for a in U.HT_FORMS for b in U.HT_FORMS if a != b}
    assert any(a == "csr_ov" and b == "csr" for a, b in pairs)     # overrides -> none
    assert any(a == "csr_md" and b == "csr" for a, b in pairs)     # metadata -> none
    assert ("csr", "v0") in pairs and ("csr_md", "v0") in pairs    # v1 -> v0
    ns = [b["n"] for b in builds]
    assert set(ns) == set(U.HT_WIDTHS) and max(ns) == U.HT_MAX_WIDTH == U.SORT_MIN + 7
    assert ns[:len(U.HT_WIDTHS)] == list(U.HT_WIDTHS)
    # the sorted path (a CSR form at >= SORT_MIN entries) and then 5 entries
    sorted_then_small = [(builds[k]["form"], builds[k + 1]["n"]) for k in range(len(builds) - 1)
                         if builds[k]["n"] >= U.SORT_MIN]
    assert sorted_then_small and all(n == 5 for _, n in sorted_then_small)
    assert any(f in U.HT_CSR_FORMS for f, _ in sorted_then_small)
    # wide -> narrow with different entries, on every form
    for f in U.HT_FORMS:
        assert any(builds[k]["form"] == f and builds[k]["n"] < builds[k - 1]["n"]
                   for k in range(1, len(builds))), f
    assert len({b["seed"] for b in builds}) == len(builds)
    assert {name for name, _ in U.HT_FAILURES} == {"max_width", "v0_metadata", "key_off_backwards"}


def test_htree_inputs_take_the_named_path(orc):
    for b in U.htree_builds():
        inp = U.htree_inputs(orc, b)
        n = b["n"]
        if b["form"] == "with":
            assert inp["digests"].shape == (n, 32)
            continue
        assert len(inp["keys"]) == len(inp["vals"]) == n
        if b["form"] == "fixed":
            assert all(len(k) == 8 for k in inp["keys"]) and all(len(v) == 128 for v in inp["vals"])
        if b["form"] == "csr_md" and n:
            assert sum(len(x) for x in inp["mds"]) > 0
        if b["form"] == "csr_ov" and n:
            k = sum(o is not None for o in inp["overrides"])
            assert k >= 1 and (n < 1000 or 0.1 < k / n < 0.3)
            assert all(s == b"" for s, o in zip(inp["vals_sent"], inp["overrides"]) if o is not None)
        if b["form"] in ("csr", "v0", "csr_md", "csr_ov") and n > 2:
            # never a progression: the fused fixed path is not taken
            assert len({len(k) for k in inp["keys"]}) > 1 or len({len(v) for v in inp["vals"]}) > 1
        if b["form"] == "v0":
            assert inp["version"] == 0 and inp["mds"] is None


def test_htree_leaves_and_failures():
    lv = U.htree_leaves(257, 4096, 1)
    assert len(lv) == 259 and lv[-2] == 257 and lv[-1] == 4096
    lv = U.htree_leaves(4096, 3, 1)
    assert len(lv) == 68 and 0 in lv[:-2] and 4095 in lv[:-2] and (lv[:-2] < 4096).all()
    assert len(U.htree_leaves(0, 3, 1)) == 2


# ------------------------------------------------------------- C: one context
def test_context_groups_go_large_small_large():
    for name, g in U.CTX_GROUPS.items():
        sizes = g["sizes"]
        assert len(sizes) == len(g["members"])
        # a middle call smaller than both neighbours (calls of one size side by
        # side, one per entry point, count as one)
        runs = [n for k, n in enumerate(sizes) if k == 0 or n != sizes[k - 1]]
        assert any(runs[k - 1] > runs[k] < runs[k + 1] for k in range(1, len(runs) - 1)), name
        order = [i for grp, i in U.CTX_ORDER if grp == name]
        assert order == list(range(len(sizes))), name
    # members of other groups lie between the calls of a group
    groups = [grp for grp, _ in U.CTX_ORDER]
    for name in U.CTX_GROUPS:
        idx = [k for k, grp in enumerate(groups) if grp == name]
        assert any(b - a > 1 for a, b in zip(idx, idx[1:])), name
    s = U.CTX_GROUPS["s_sort"]["sizes"]
    assert s[0] >= U.SORT_MIN > s[2] and s[-1] >= U.SORT_MIN  # crossed both ways
    t = U.CTX_GROUPS["s_tx"]
    packed = [n for mem, n in zip(t["members"], t["sizes"]) if mem == "build_many_packed"]
    assert packed and all(n > 2048 for n in packed)


def test_context_groups_name_every_required_entry_point():
    """The lists cannot shrink quietly: every scratch group and every entry
    point that the two interleavings are there for."""
    first = {g: set(v["members"]) for g, v in U.CTX_GROUPS.items()}
    second = {g: {c[0] for c in v["calls"]} for g, v in U.CTX2_GROUPS.items()}
    groups = set(first) | set(second)
    assert groups >= {"s_tx", "s_msgs", "s_ventry", "s_ans", "s_exp", "s_txg", "s_sort"}
    s_tx = first["s_tx"] | second["s_tx"]
    assert s_tx >= {"dual_v2_pb", "dual_v1_pb", "ventry_pb", "vtx_pb", "tx_alh",
                    "build_many_packed", "build_many_planned", "replicate"}
    s_msgs = first["s_msgs"] | second["s_msgs"]
    assert s_msgs >= {"htree_verify", "ahtree_verify_incl", "ahtree_verify_cons",
                      "ahtree_verify_last", "documents", "verify_values"}
    for g, need in U.CTX2_REQUIRED.items():
        assert second[g] >= need, g
    assert first["s_sort"] >= {"dev_sha256", "verify_values"}


def test_second_interleaving_goes_large_small_large():
    for name, g in U.CTX2_GROUPS.items():
        calls = g["calls"]
        # per entry point and over the whole group: a middle call smaller than
        # the calls on both sides of it
        sizes = [c[1] for c in calls]
        runs = [n for k, n in enumerate(sizes) if k == 0 or n != sizes[k - 1]]
        assert any(runs[k - 1] > runs[k] < runs[k + 1] for k in range(1, len(runs) - 1)), name
        assert [i for grp, i in U.CTX2_ORDER if grp == name] == list(range(len(calls))), name
    groups = [grp for grp, _ in U.CTX2_ORDER]
    for name in U.CTX2_GROUPS:
        idx = [k for k, grp in enumerate(groups) if grp == name]
        assert any(b - a > 1 for a, b in zip(idx, idx[1:])), name   # others in between
    ans = U.CTX2_GROUPS["s_ans"]["calls"]
    va = [c for c in ans if c[0] == "verifiable_answers"]
    assert {bool(c[2].get("hint")) for c in va} == {True, False}
    assert any(b[1] < a[1] for a, b in zip(ans, ans[1:]))            # fewer requests than before
    exp = U.CTX2_GROUPS["s_exp"]["calls"]
    assert {c[2]["arm"] for c in exp} == {"A", "B"}
    for arm in "AB":
        ns = [c[1] for c in exp if c[2]["arm"] == arm]
        assert ns[0] > ns[1] == 1 < ns[2]       # a long range, one tx, the unavailable values
    txg = U.CTX2_GROUPS["s_txg"]["calls"]
    assert [len(c[2]["weights"].split(":")) for c in txg if c[0] == "txlog_chunks"] == [3, 1, 2]
    cl = [c[2] for c in txg if c[0] == "clog"]
    assert {c["mode"] for c in cl} == {"host", "dev"}
    dev = [c["width"] for c in cl if c["mode"] == "dev"]
    assert any(a > b for a, b in zip(dev, dev[1:])) and any(a < b for a, b in zip(dev, dev[1:]))


# ------------------------------------------------------- D: queued builds
def test_queued_builds_cross_the_sort_threshold_both_ways():
    ns = U.QUEUED_BUILD_NS
    assert len(ns) == 12 and ns[0] == 1 and ns[-1] == 3 and max(ns) == 20000
    side = [n >= U.SORT_MIN for n in ns]
    assert (False, True) in set(zip(side, side[1:])) and (True, False) in set(zip(side, side[1:]))
    assert U.SORT_MIN - 1 in ns and U.SORT_MIN in ns
