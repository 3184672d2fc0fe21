"""mh_replicate_tx_batch on the device against the CPU reference of
tests/replicate_util.py: every output array, and the tree after the call
through mh_ahtree_dlog / mh_ahtree_size."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import replicate_util as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def gpu_tree(m, ctx, txs, P):
    """the follower's tree: the Alh of the first P txs"""
    t = m.AHtree(ctx)
    if P:
        t.append_batch(np.frombuffer(b"".join(x["alh"] for x in txs[:P]), np.uint8).reshape(P, 32))
    return t


def run(m, t, blobs, prev, lim=None, flags=0, **kw):
    return m.replicate_tx_batch(t, blobs, prev, flags=flags, **(lim or R.Limits()).kw(), **kw)


def same(out, ref, t, what=""):
    assert out["status"].tolist() == ref["status"].tolist(), what
    assert out["accepted"] == ref["accepted"], what
    assert out["ent_off"].tolist() == ref["ent_off"].tolist(), what
    for name in ("hdrs", "md_blob", "alh", "ents", "hvals"):
        assert out[name].tobytes() == ref[name].tobytes(), (what, name)
    assert t.size() == ref["size"], what
    assert t.dlog() == ref["dlog"], what


def replay(m, ctx, orc, txs, trees, P, blobs, lim=None, flags=0, what=""):
    t = gpu_tree(m, ctx, txs, P)
    prev = R.prev_alh_of(orc, txs, P)
    ref = R.reference(orc, blobs, trees[P], prev, lim, flags)
    same(run(m, t, blobs, prev, lim, flags), ref, t, what)
    t.close()
    return ref


# ------------------------------------------------------------------ Go stores
@pytest.mark.parametrize("store", ["long_linear_proof", "v110_defaultdb", "v110_systemdb"])
def test_go_stores(m, ctx, orc, fixtures, store):
    blobs, alhs, dlog = R.fixture_store(fixtures[store])
    empty = orc.sha256(b"")
    t = m.AHtree(ctx)
    ref = R.reference(orc, blobs, orc.AHtree(1), empty)
    assert ref["accepted"] == len(blobs) and ref["dlog"] == dlog
    same(run(m, t, blobs, empty), ref, t, store)
    t.close()
    for cut in range(len(blobs) + 1):  # two calls, split at every position
        t = m.AHtree(ctx)
        a = run(m, t, blobs[:cut], empty)
        b = run(m, t, blobs[cut:], alhs[cut - 1] if cut else empty)
        assert a["accepted"] == cut and b["accepted"] == len(blobs) - cut, cut
        assert np.concatenate([a["alh"], b["alh"]]).tobytes() == b"".join(alhs), cut
        assert t.size() == len(blobs) and t.dlog() == dlog, cut
        t.close()


# ------------------------------------------------------------------ block edges
VAL_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 4096)
KEY_LENS = (1, 19, 20, 83, 84, 1024)
WIDTHS = (1, 2, 3, 5, 8, 9, 64, 65, 1024)
MD_KINDS = {0: (False, None, False), 1: (True, None, False), 9: (False, 7, False),
            10: (True, 7, False), 11: (True, 7, True)}  # verifiable_entry_util.MD_KINDS


def _key(i, kl):
    """distinct for distinct i within a tx (kl == 1: i < 256)"""
    return bytes([i % 256]) if kl == 1 else (struct.pack(">I", i) + bytes([i % 251]) * kl)[:kl]


def edge_specs():
    rng = np.random.default_rng(5)
    rb = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    mds = [R.kv_md_bytes(*v) for v in MD_KINDS.values()]
    assert sorted(len(x) for x in mds) == sorted(MD_KINDS)
    extra = b"\x01" + struct.pack(">H", 5) + b"extra"
    specs = []
    for ver in (1, 0):  # every value length x key length, no metadata
        ents = [(_key(i, kl), b"", rb(vl)) for i, (vl, kl) in
                enumerate((v, k) for v in VAL_LENS for k in KEY_LENS)]
        specs.append(dict(entries=ents, version=ver))
    # every KV-metadata kind at the digest's block edges, with tx metadata
    ents = [(_key(i, kl), md, rb(vl)) for i, (md, kl, vl) in
            enumerate((md, k, v) for md in mds for k in (1, 19, 20, 83, 84) for v in (0, 56, 65))]
    specs.append(dict(entries=ents, version=1, txmd=b"\x00" + struct.pack(">Q", 3) + extra))
    specs.append(dict(entries=ents[:7], version=1, txmd=extra))
    for k, w in enumerate(WIDTHS):  # tree widths; six entries of 1024 have one-byte keys
        ents = [(_key(i // 6 if i % 6 == 0 else i, KEY_LENS[i % 6]), mds[i % 5] if k % 2 == 0 else b"",
                 rb(VAL_LENS[i % 9])) for i in range(w)]
        specs.append(dict(entries=ents, version=1 if k % 2 == 0 else 0))
    return specs


@pytest.fixture(scope="module")
def edge_store(orc):
    return R.synthetic_store(orc, edge_specs(), bl_of=lambda i: [i - 1, 0, i // 2][i % 3])


def test_block_edges(m, ctx, orc, edge_store):
    txs, trees = edge_store
    assert {len(t["entries"]) for t in txs} >= set(WIDTHS)
    ref = replay(m, ctx, orc, txs, trees, 0, [t["blob"] for t in txs])
    assert ref["accepted"] == len(txs)
    ref = replay(m, ctx, orc, txs, trees, 4, [t["blob"] for t in txs[4:]])
    assert ref["accepted"] == len(txs) - 4


# ------------------------------------------------------------------ linking
@pytest.fixture(scope="module")
def linked_store(orc):
    """1008 one-entry txs: BlTxID = id - 1, id / 2, a fixed old tx (1), 0 in turn"""
    specs = [dict(entries=[(b"key%d" % k, b"", b"value%d" % k)]) for k in range(1008)]
    return R.synthetic_store(orc, specs, keep={1, 7, 8, 1000},
                             bl_of=lambda i: [i - 1, i // 2, min(1, i - 1), 0][i % 4])


@pytest.mark.parametrize("P", [0, 1, 7, 8, 1000])
def test_linking(m, ctx, orc, linked_store, P):
    txs, trees = linked_store
    bl = [t["header"]["bl_tx_id"] for t in txs[P:P + 8]]
    if P:
        assert any(0 < b <= P for b in bl)  # inside the resident part
    assert any(b > P for b in bl) and 0 in bl  # inside the batch's own part; none
    ref = replay(m, ctx, orc, txs, trees, P, [t["blob"] for t in txs[P:P + 8]], what="P=%d" % P)
    assert ref["accepted"] == 8
    # a BlRoot of the batch's own part that is wrong breaks the chain there
    k = next(i for i, b in enumerate(bl) if b > P)
    blobs = [t["blob"] for t in txs[P:P + 8]]
    blobs[k] = R._hdr_edit(txs[P + k], bl_root=bytes(31) + b"\x01")
    ref = replay(m, ctx, orc, txs, trees, P, blobs, what="P=%d broken" % P)
    assert ref["accepted"] == k and ref["status"][k] == R.ILLEGAL


# ------------------------------------------------------------------ mutants
@pytest.fixture(scope="module")
def mutant_store(orc):
    return R.synthetic_store(orc, R.simple_specs(10))


@pytest.mark.parametrize("pos", [0, 3, 6])
def test_mutant_rows(m, ctx, orc, mutant_store, pos):
    """Every row of the table at the head, in the middle and at the end of a
    7-tx batch behind 3 resident leaves: statuses (MH_ERR_TX_NOT_REACHED
    against the local verdicts behind the break), accepted, P + a leaves."""
    txs, trees = mutant_store
    P = 3
    prev = R.prev_alh_of(orc, txs, P)
    rows = R.mutants(orc, txs[P + pos], R.prev_alh_of(orc, txs, P + pos), trees[P + pos])
    seen = set()
    for name, blob, want in rows:
        blobs = [t["blob"] for t in txs[P:P + 7]]
        blobs[pos] = blob
        if pos < 5:  # a local error behind the break keeps its verdict
            blobs[pos + 2] = blobs[pos + 2][:-1] + b"\x07"
        ref = R.reference(orc, blobs, trees[P], prev, R.MUT_LIMITS)
        assert ref["status"][pos] == want, name
        t = gpu_tree(m, ctx, txs, P)
        same(run(m, t, blobs, prev, R.MUT_LIMITS), ref, t, name)
        assert t.size() == P + ref["accepted"]
        t.close()
        seen |= set(ref["status"].tolist())
    assert seen >= R.ALL_CODES - ({R.NOT_REACHED} if pos == 6 else set())


# ------------------------------------------------------------------ flags
def test_skip_integrity(m, ctx, orc, mutant_store):
    """A wrong exported Eh is accepted, the Alh is the one over the built Eh
    (the valid tx's own), and with a tampered entry the next tx fails on PrevAlh"""
    txs, trees = mutant_store
    P = 2
    blobs = [t["blob"] for t in txs[P:P + 5]]
    blobs[1] = R._hdr_edit(txs[P + 1], eh=bytes(32))
    ref = replay(m, ctx, orc, txs, trees, P, blobs, flags=R.SKIP_INTEGRITY)
    assert ref["accepted"] == 5 and bytes(ref["alh"][1]) == txs[P + 1]["alh"]
    assert bytes(ref["hdrs"][1]["eh"]) == txs[P + 1]["header"]["eh"]
    ref = replay(m, ctx, orc, txs, trees, P, blobs)
    assert ref["accepted"] == 1 and ref["status"][1] == R.ILLEGAL
    e = txs[P + 1]["entries"]
    blobs[1] = R.export_tx(txs[P + 1]["header"], [e[0], (e[1][0], b"", b"tampered")], False)
    ref = replay(m, ctx, orc, txs, trees, P, blobs, flags=R.SKIP_INTEGRITY)
    assert ref["accepted"] == 2 and ref["status"].tolist() == [0, 0, R.ILLEGAL, R.NOT_REACHED,
                                                               R.NOT_REACHED]
    assert bytes(ref["alh"][1]) != txs[P + 1]["alh"]


def test_dry_run(m, ctx, orc, mutant_store):
    txs, trees = mutant_store
    for P in (0, 4):
        t = gpu_tree(m, ctx, txs, P)
        before = t.dlog()
        prev = R.prev_alh_of(orc, txs, P)
        blobs = [x["blob"] for x in txs[P:]]
        ref = R.reference(orc, blobs, trees[P], prev, flags=R.DRY_RUN)
        assert ref["accepted"] == len(blobs) and ref["size"] == P
        same(run(m, t, blobs, prev, flags=R.DRY_RUN), ref, t)
        assert t.size() == P and t.dlog() == before
        same(run(m, t, blobs, prev), R.reference(orc, blobs, trees[P], prev), t)  # and for real
        t.close()


# ------------------------------------------------------------------ truncated
def test_truncated(m, ctx, orc):
    rng = np.random.default_rng(9)
    rb = lambda n: bytes(rng.integers(1, 256, n, dtype=np.uint8))  # noqa: E731
    specs = [dict(entries=[(b"k%d" % i, b"\x00" if i % 2 else b"", rb(vl))
                           for i, vl in enumerate(lens)], truncated=tr, version=ver)
             for lens, tr, ver in (((32, 32, 32), True, 1), ((0, 5, 31, 33, 100), True, 1),
                                   ((32, 7), False, 1), ((32, 40), True, 1))]
    specs.append(dict(entries=[(b"a", b"", rb(32)), (b"b", b"", rb(3))], truncated=True, version=0))
    txs, trees = R.synthetic_store(orc, specs)
    ref = replay(m, ctx, orc, txs, trees, 0, [t["blob"] for t in txs])
    assert ref["accepted"] == len(txs)
    assert ref["ents"]["flags"].tolist() == [1] * 3 + [1] * 5 + [0] * 2 + [1] * 2 + [1] * 2
    assert bytes(ref["hvals"][4]) == txs[1]["entries"][1][2] + bytes(27)


# ------------------------------------------------------------------ chunks
CHUNK_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "oracle"), os.path.join(%(root)r, "tests")]
import torch  # noqa: F401
import immustore_amd as m
import oracle as orc
import replicate_util as R
import test_gpu_replicate as T
rng = np.random.default_rng(3)
specs = [dict(entries=[(b"k%%d" %% e, b"", bytes(rng.integers(0, 256, 20000 + 64 * (k %% 7), dtype=np.uint8)))
                       for e in range(3)]) for k in range(54)]
txs, trees = R.synthetic_store(orc, specs, keep={2}, bl_of=lambda i: [i - 1, i // 2, 0][i %% 3])
P = 2
blobs = [t["blob"] for t in txs[P:]]
assert sum(len(b) for b in blobs) > 3 << 20
ctx = m.Context(0)
for br in (None, 30):  # a break in the second chunk (1 MiB = ~17 txs)
    bl = list(blobs)
    if br is not None:
        bl[br] = R._hdr_edit(txs[P + br], prev_alh=bytes(32))
        bl[br + 3] = b"\x00\x00"
    T.replay(m, ctx, orc, txs, trees, P, bl, what="break %%r" %% br)
ctx.close()
print("chunks ok")
"""


def test_chunks():
    """MH_PB_CHUNK_MIB=1 (and MH_PB_GROUP_RATIO=0: every chunk a group) over 3
    MiB of blobs in a fresh process: several chunks and groups, the chain
    across them, a break in the second chunk."""
    for ratio in ("0", None):
        env = dict(os.environ, MH_PB_CHUNK_MIB="1")
        env.pop("MH_PB_GROUP_RATIO", None)
        if ratio is not None:
            env["MH_PB_GROUP_RATIO"] = ratio
        r = subprocess.run([sys.executable, "-c", CHUNK_CHILD % dict(root=ROOT)], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "chunks ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------ independent cross-check
def test_outputs_make_a_valid_tx_log(m, ctx, orc, edge_store):
    """The tx-log record of every accepted tx assembled from hdrs / ents /
    hvals / alh alone (tx_util's record layout, vOff 0) validates under the
    tx-log oracle with the same Alh: independent of replicate_util.reference."""
    txs, _ = edge_store
    blobs = [t["blob"] for t in txs]
    flat = b"".join(blobs)
    t = m.AHtree(ctx)
    out = run(m, t, blobs, orc.sha256(b""))
    t.close()
    assert out["accepted"] == len(txs)
    log = bytearray()
    for k, h in enumerate(out["hdrs"]):
        md = out["md_blob"][int(h["md_off"]):int(h["md_off"]) + int(h["md_len"])].tobytes()
        rec = struct.pack(">QqQ", int(h["id"]), int(h["ts"]), int(h["bl_tx_id"])) + h["bl_root"].tobytes()
        rec += h["prev_alh"].tobytes() + struct.pack(">H", int(h["version"]))
        rec += struct.pack(">H", int(h["nentries"])) if h["version"] == 0 else \
            struct.pack(">H", len(md)) + md + struct.pack(">I", int(h["nentries"]))
        for e in range(int(out["ent_off"][k]), int(out["ent_off"][k + 1])):
            r = out["ents"][e]
            kv = flat[int(r["md_off"]):int(r["md_off"]) + int(r["md_len"])]
            key = flat[int(r["key_off"]):int(r["key_off"]) + int(r["key_len"])]
            rec += struct.pack(">H", len(kv)) + kv + struct.pack(">H", len(key)) + key
            rec += struct.pack(">IQ", int(r["val_len"]), 0) + out["hvals"][e].tobytes()
        log += rec + out["alh"][k].tobytes()
    st, ntx, used, alh, sts = orc.txlog_validate(bytes(log), max_entries=1024, max_key_len=1024)
    assert st == 0 and ntx == len(txs) and used == len(log) and not sts.any()
    assert alh.tobytes() == out["alh"].tobytes() == b"".join(x["alh"] for x in txs)


# ------------------------------------------------------------------ ents_cap
def test_ents_cap(m, ctx, orc, mutant_store):
    txs, trees = mutant_store
    P = 3
    t = gpu_tree(m, ctx, txs, P)
    before = t.dlog()
    blobs = [x["blob"] for x in txs[P:]]
    prev = R.prev_alh_of(orc, txs, P)
    for cap in (0, 13):
        with pytest.raises(m._native.ErrBufferTooSmall) as e:
            run(m, t, blobs, prev, ents_cap=cap)
        assert e.value.needed == 14
        assert t.size() == P and t.dlog() == before
    ref = R.reference(orc, blobs, trees[P], prev)
    same(run(m, t, blobs, prev, ents_cap=14), ref, t)
    t.close()
