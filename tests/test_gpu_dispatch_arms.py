"""Every kernel arm that the launchers pick by batch size or by an environment
knob, at its own edges, byte for byte against the oracle:

  A  k_leaves_from_digests<1|2|4> under MH_DIGEST_LPL (choose_digest_lpl):
     the LaneReducer group edges (a lane holding 1, 2 or 3 of its 4 digests,
     level-1 / level-2 promotion at the end of the row), whole and partial last
     workgroups, through HTree.build_with and mh_dev_htree_build_digests with
     and without a root pointer.
  B  k_reduce4<256> (launch_reduce: width >= 2^18 and >= 3 levels left): 1, 2,
     3 or 4 nodes on its last lane, the promoted node of an odd width[l0 + 1],
     started at level 0 and at level 1, with a root pointer and without one
     (top = -1: root = NULL, mh_dev_htree_reduce_nodes).
  C  k_small_roots_pack (more than 2048 trees) at every lgp 1..6, the last
     workgroup short, width-0 trees, leaf_off[0] != 0.
  D  The length-class sort (nb_sort, n >= 16384) on both sides of its
     threshold and with a short last sort chunk, under k_sha_varlen (hashing and
     the read-side value check) and k_entries_varlen with overrides; the
     context's "varlen_sort" timer pins each case to its side of the dispatch.
  E  k_aht_perfect_t (a level with >= 2^18 new perfect nodes) appended onto a
     tree that already has nodes.

Outputs are poisoned with 0xA5 before a call, inputs are exactly the bytes
used.  The oracle work of every case is made once (module fixtures) or stays
well under a second.
"""
import os

import numpy as np
import pytest

from gpu_util import DevBuf

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


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Timed:
    """The context's launch timer on for the block, empty at its start."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_timing(True)
        self.ctx.timing_reset()

    def __exit__(self, *a):
        self.ctx.set_timing(False)


def _poison(ctx, nbytes):
    return DevBuf.from_host(ctx, np.full(nbytes, 0xA5, np.uint8))


POISON32 = bytes([0xA5]) * 32


def _first_diff(got, want, unit=32):
    """Index of the first `unit`-byte record in which two byte strings differ
    (None when equal), for the assertion messages."""
    if got == want:
        return None
    if len(got) != len(want):
        return ("length", len(got), len(want))
    a = np.frombuffer(got, np.uint8).reshape(-1, unit)
    b = np.frombuffer(want, np.uint8).reshape(-1, unit)
    return int(np.nonzero((a != b).any(axis=1))[0][0])


def _orc_sha_batch(orc, buf, off):
    """The oracle's SHA-256 of every range buf[off[i]:off[i+1]] (offsets in
    order) in one call: the hVals of entries with empty keys -> (n, 32)."""
    n = len(off) - 1
    b = np.ascontiguousarray(buf, np.uint8)
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    st, hv, _, _ = orc.build_entries_csr(1, np.zeros(1, np.uint8), np.zeros(n + 1, np.uint64), None,
                                         None, b, np.ascontiguousarray(off, np.uint64),
                                         want_levels=False)
    assert st == 0
    return hv


# ------------------------------------------------- A: digest leaves, MH_DIGEST_LPL
# every count c in {1, 2, 3, 4} on the last lane of LPL 4 (and {1, 2} of LPL 2),
# rows that end in a promoted level-1 / level-2 node, whole and partial last
# workgroups (256 lanes = 256 / 512 / 1024 digests)
DIGEST_WIDTHS = (list(range(1, 10)) + [15, 16, 17] + list(range(255, 262)) +
                 list(range(1021, 1030)) + [4095, 4097])


@pytest.fixture(scope="module")
def digest_sets(orc):
    """width -> two different digest sets, each (digests, levels bytes, root)."""
    out = {}
    for w in DIGEST_WIDTHS:
        sets = []
        for seed in (7000, 9000):
            d = orc.fill_random(w * 32, seed + w).reshape(w, 32)
            lv, root = orc.htree_build(d)
            sets.append((d, lv.tobytes(), root))
        out[w] = sets
    return out


@pytest.mark.parametrize("lpl", ["1", "2", "4"])
def test_digest_leaves_every_lpl_vs_oracle(m, ctx, orc, digest_sets, lpl):
    """Both digest sets of a width built alternately into the SAME level
    buffer (a node read before this build stored it would be the other
    set's): HTree.build_with -> root and all levels; the device entry point ->
    levels and root with a root pointer, levels alone (root buffer untouched)
    with root = NULL."""
    from immustore_amd import _native as N
    L = N.load()
    with _Env(MH_DIGEST_LPL=lpl):
        for w in DIGEST_WIDTHS:
            sets = digest_sets[w]
            t = m.HTree(w, ctx)
            for k in (0, 1, 0, 1):
                d, olv, oroot = sets[k]
                assert d.nbytes == w * 32
                t.build_with(d)
                assert t.root() == oroot, ("build_with", lpl, w, k)
                assert t.levels().tobytes() == olv, \
                    ("build_with", lpl, w, k, _first_diff(t.levels().tobytes(), olv))
            t.close()
            dds = [DevBuf.from_host(ctx, s[0]) for s in sets]   # exactly w * 32 bytes
            dl = _poison(ctx, m.levels_len(w) * 32)
            for k, want_root in ((0, True), (1, False), (0, False), (1, True)):
                _, olv, oroot = sets[k]
                dr = _poison(ctx, 32)
                N.check(L.mh_dev_htree_build_digests(ctx.handle, dds[k].ptr, w, dl.ptr,
                                                     dr.ptr if want_root else None))
                ctx.synchronize()
                lv = dl.to_host().tobytes()
                case = ("dev", lpl, w, k, want_root)
                assert lv == olv, case + (_first_diff(lv, olv),)
                assert dr.to_host().tobytes() == (oroot if want_root else POISON32), case
                dr.free()
            dl.free()
            for b in dds:
                b.free()


# ------------------------------------------------------------ B: k_reduce4 residues
# launch_reduce() (htree_kernels.hip) takes k_reduce4<256> only while the level
# the reduction starts from has width[cur] >= 4 * 256 * 256 = 2^18 nodes and at
# least 3 levels remain; below that it is k_reduce.  With MH_DIGEST_LPL=1 the
# reduction starts at level 0 (width[cur] = n), with MH_DIGEST_LPL=2 at level 1
# (width[cur] = ceil(n / 2)): every n below must stay >= 2^18 (LPL 1) or
# > 2^19 - 1 (LPL 2), or the case silently moves to k_reduce.
# n mod 4 walks the 1 / 2 / 3 / 4 nodes of the last lane; an odd width[cur + 1]
# (n mod 4 in {1, 2} at LPL 1) takes the promoted-node store; + 1024 / + 512
# put odd widths at the top of the workgroup's in-LDS levels as well.
# k_reduce4's own root store (l == top) is out of reach at these sizes: a level
# of >= 2^18 nodes has >= 18 levels above it and a launch takes 10, so the top
# launch is k_reduce<512> below 2^28 leaves; the rooted runs here check that
# k_reduce4 stores no root early, the rootless ones its top = -1 use.
_W18 = 1 << 18
REDUCE4_CASES = ([("1", _W18 + r) for r in range(9)] +
                 [("1", _W18 + 1024 + r) for r in (1, 2, 3)] +
                 [("1", _W18 + 512 + 1), ("1", 3 * (1 << 17) + 5)] +
                 [("2", (1 << 19) + r) for r in (1, 2, 3, 5)])
REDUCE4_ROOTLESS = (_W18 + 1, _W18 + 1024 + 3)   # also run with root = NULL (top = -1)


def _level_of(n, node):
    """(level, index in level) of flat node `node` of an n-leaf tree (levels
    back to back, each half the one below rounded up; htree.go:85-110)."""
    lvl, first, w = 0, 0, n
    while w > 1 and node >= first + w:
        first += w
        w = (w + 1) // 2
        lvl += 1
    return lvl, node - first


@pytest.mark.parametrize("lpl,n", REDUCE4_CASES)
def test_reduce4_residues_vs_oracle(m, ctx, orc, lpl, n):
    from immustore_amd import _native as N
    L = N.load()
    assert (n if lpl == "1" else (n + 1) // 2) >= 4 * 256 * 256
    d = orc.fill_random(n * 32, 600 + n).reshape(n, 32)
    olv, oroot = orc.htree_build(d)
    olv = olv.tobytes()
    dd = DevBuf.from_host(ctx, d)                     # exactly n * 32 bytes
    for want_root in (True, False) if n in REDUCE4_ROOTLESS else (True,):
        dl = _poison(ctx, m.levels_len(n) * 32)
        dr = _poison(ctx, 32)
        with _Env(MH_DIGEST_LPL=lpl):
            N.check(L.mh_dev_htree_build_digests(ctx.handle, dd.ptr, n, dl.ptr,
                                                 dr.ptr if want_root else None))
        ctx.synchronize()
        lv = dl.to_host().tobytes()
        bad = _first_diff(lv, olv)
        assert bad is None, (lpl, n, want_root, "first wrong node (level, index)",
                             _level_of(n, bad))
        assert dr.to_host().tobytes() == (oroot if want_root else POISON32), (lpl, n, want_root)
        dl.free()
        dr.free()
    dd.free()


def _reduce_levels_host(orc, row):
    """The levels above a row of nodes and the root, htree.go:85-110 without
    the leaf step (pairs hashed as SHA256(0x01 || l || r), an odd last node
    promoted unchanged): the host restatement of
    test_reduce_nodes_levels_every_small_width, each level's node hashes made
    by one call of the oracle's SHA-256 -> (levels (L, 32), root bytes)."""
    lvl = np.ascontiguousarray(row, np.uint8).reshape(-1, 32)
    out = [lvl]
    while lvl.shape[0] > 1:
        h = lvl.shape[0] // 2
        msg = np.empty((h, 65), np.uint8)
        msg[:, 0] = 1
        msg[:, 1:] = lvl[:2 * h].reshape(h, 64)
        nxt = _orc_sha_batch(orc, msg.reshape(-1), np.arange(h + 1, dtype=np.uint64) * 65)
        if lvl.shape[0] % 2:
            nxt = np.concatenate([nxt, lvl[-1:]])
        out.append(nxt)
        lvl = nxt
    return np.concatenate(out), lvl[0].tobytes()


@pytest.mark.parametrize("w", [_W18 + 1, _W18 + 3, _W18 + 6])
def test_reduce4_reduce_nodes_vs_host_restatement(m, ctx, orc, w):
    """mh_dev_htree_reduce_nodes over a row wide enough for k_reduce4 (the
    launcher's top = -1 use: the root is copied after the last launch)."""
    from immustore_amd import _native as N
    assert w >= 4 * 256 * 256
    row = orc.fill_random(w * 32, 900 + w).reshape(w, 32)
    want, root = _reduce_levels_host(orc, row)
    assert want.shape[0] == m.levels_len(w)
    # the restatement against itself on a row the oracle's htree also covers:
    # leaf hashes of 5 digests, reduced, are htree_build's levels
    d5 = orc.fill_random(5 * 32, 1).reshape(5, 32)
    olv5, oroot5 = orc.htree_build(d5)
    assert _reduce_levels_host(orc, olv5[:5])[0].tobytes() == olv5.tobytes()
    assert _reduce_levels_host(orc, olv5[:5])[1] == oroot5
    dn = DevBuf.from_host(ctx, row)                   # exactly w * 32 bytes
    dl = _poison(ctx, m.levels_len(w) * 32)
    dr = _poison(ctx, 32)
    N.check(N.load().mh_dev_htree_reduce_nodes(ctx.handle, dn.ptr, w, dl.ptr, dr.ptr))
    ctx.synchronize()
    lv = dl.to_host().tobytes()
    bad = _first_diff(lv, want.tobytes())
    assert bad is None, (w, "first wrong node (level, index)", _level_of(w, bad))
    assert dr.to_host().tobytes() == root, w
    for b in (dn, dl, dr):
        b.free()


# ------------------------------------------------- C: k_small_roots_pack, every lgp
# launch_small_roots() runs the packed kernel for more than 2048 trees with
# lgp = ceil(log2(wmax)) clamped to 1..6: wmax 1, 2 -> 1; 3, 4 -> 2; 5, 8 -> 3;
# 9, 16 -> 4; 17, 32 -> 5; 33, 64 -> 6.  A workgroup takes 512 >> lgp trees, so
# 2049 and 2500 trees leave the last workgroup short at every lgp.
PACK_WMAX = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
PACK_COUNTS = (2049, 2500)


def _trees(orc, widths, seed):
    """-> (list of (w, 32) digest arrays, expected roots (n, 32))."""
    tot = int(np.sum(widths))
    flat = orc.fill_random(max(tot, 1) * 32, seed).reshape(-1, 32)
    cut = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    trees = [flat[cut[k]:cut[k + 1]] for k in range(len(widths))]
    roots = np.frombuffer(b"".join(orc.htree_build(t)[1] for t in trees), np.uint8)
    return trees, roots.reshape(-1, 32)


@pytest.mark.parametrize("wmax", PACK_WMAX)
def test_small_roots_pack_every_lgp_vs_oracle(m, ctx, orc, wmax):
    rng = np.random.default_rng(100 + wmax)
    for count in PACK_COUNTS:
        assert count > 2048
        ragged = rng.integers(0, wmax + 1, count)
        assert (ragged == 0).any() and (ragged == wmax).any() and ragged.max() == wmax
        for kind, widths in (("ragged", ragged), ("full", np.full(count, wmax))):
            trees, want = _trees(orc, widths, 3000 + 7 * wmax + count + len(kind))
            got = m.htree_build_many(trees, ctx)
            bad = _first_diff(got.tobytes(), want.tobytes())
            assert bad is None, (wmax, count, kind, "first wrong tree, its width", bad,
                                 int(widths[bad]))


def test_small_roots_pack_leaf_off_not_from_zero(m, ctx, orc):
    """mh_htree_build_many with leaf_off[0] != 0: the digests before
    leaf_off[0] belong to no tree (k_small_roots_pack rebases by leaf_off[0])."""
    from immustore_amd import _native as N
    rng = np.random.default_rng(55)
    count, skip = 2049, 5
    widths = rng.integers(0, 6, count)               # wmax 5: lgp 3
    assert widths.max() == 5 and (widths == 0).any()
    trees, want = _trees(orc, widths, 77)
    flat = np.concatenate([np.full((skip, 32), 0xA5, np.uint8)] + trees)
    off = (np.concatenate([[0], np.cumsum(widths)]) + skip).astype(np.uint64)
    assert flat.shape[0] == int(off[-1])             # exactly the digests used
    roots = np.full((count, 32), 0xA5, np.uint8)
    N.check(N.load().mh_htree_build_many(ctx.handle, count, off.ctypes.data, flat.ctypes.data,
                                         roots.ctypes.data))
    bad = _first_diff(roots.tobytes(), want.tobytes())
    assert bad is None, ("first wrong tree, its width", bad, int(widths[bad]))


# ------------------------------------------------------- D: the length-class sort
SORT_MIN = 16384    # nb_sort() (varlen_kernels.hip): sorted from this many messages
SORT_CHUNK = 4096   # kNbChunk: entries per workgroup of the sort passes
LAST_CLASS = (65472 - 9, 65472 - 8, 70000)   # >= 1023 blocks: the shared last class


def _sort_launches(ctx):
    return ctx.timing("varlen_sort")[1]


def _sha_lens(rng, n):
    """Every length 0..200, the block edges around 256 / 320 bytes, three
    messages of the last length class, the rest short; shuffled."""
    fixed = list(range(201)) + [247, 248, 311, 312] + list(LAST_CLASS)
    lens = np.concatenate([fixed, rng.integers(0, 64, n - len(fixed))]).astype(np.int64)
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("n", [SORT_MIN - 1, SORT_MIN, SORT_MIN + 1, 20001])
def test_sha256_batch_sort_boundary_vs_oracle(m, ctx, orc, n):
    """mh_dev_sha256_batch just below, on and above the sort threshold and at
    a count whose last sort chunk is short; the whole batch at start
    alignments 0, 1 and 3; under 1 MiB of input."""
    from immustore_amd import _native as N
    L = N.load()
    assert 20001 % SORT_CHUNK != 0
    rng = np.random.default_rng(n)
    lens = _sha_lens(rng, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    assert total + 3 < (1 << 20)
    msgs = orc.fill_random(total, 40 + n)
    want = _orc_sha_batch(orc, msgs, off).tobytes()
    assert want[32 * 5:32 * 6] == orc.sha256(msgs[int(off[5]):int(off[6])].tobytes())
    for shift in (0, 1, 3):
        buf = np.concatenate([np.zeros(shift, np.uint8), msgs])   # exactly shift + total bytes
        d_buf = DevBuf.from_host(ctx, buf)
        d_off = DevBuf.from_host(ctx, off + np.uint64(shift))
        d_out = _poison(ctx, 32 * n)
        with _Timed(ctx):
            N.check(L.mh_dev_sha256_batch(ctx.handle, d_buf.ptr, d_off.ptr, n, d_out.ptr))
            ctx.synchronize()
            sorts = _sort_launches(ctx)
        assert (sorts >= 1) if n >= SORT_MIN else (sorts == 0), (n, shift, sorts)
        got = d_out.to_host().tobytes()
        bad = _first_diff(got, want)
        assert bad is None, (n, shift, "first wrong message, its length", bad, int(lens[bad]))
        for b in (d_buf, d_off, d_out):
            b.free()


def test_sha256_batch_sorted_backward_offsets(m, ctx, orc):
    """A sorted batch in which a few device offsets run backwards: those
    ranges hash as the empty message (as in test_csr_offsets_running_backwards),
    their neighbours as the bytes their own offsets name."""
    from immustore_amd import _native as N
    n = SORT_MIN + 100
    rng = np.random.default_rng(66)
    lens = _sha_lens(rng, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    msgs = orc.fill_random(int(off[-1]), 67)
    want = _orc_sha_batch(orc, msgs, off).copy()
    bb = msgs.tobytes()
    # off[j] pulled below off[j - 1]: message j - 1 runs backwards, message j
    # starts early (inside the buffer)
    for j in (1000, 5000, SORT_MIN - 1, n - 1):
        assert off[j - 1] >= 7 and off[j] >= off[j - 1]
        off[j] = off[j - 1] - np.uint64(7)
        want[j - 1] = np.frombuffer(orc.sha256(b""), np.uint8)
        want[j] = np.frombuffer(orc.sha256(bb[int(off[j]):int(off[j + 1])]), np.uint8)
    d_buf = DevBuf.from_host(ctx, msgs)               # exactly the bytes used
    d_off = DevBuf.from_host(ctx, off)
    d_out = _poison(ctx, 32 * n)
    with _Timed(ctx):
        N.check(N.load().mh_dev_sha256_batch(ctx.handle, d_buf.ptr, d_off.ptr, n, d_out.ptr))
        ctx.synchronize()
        assert _sort_launches(ctx) >= 1
    bad = _first_diff(d_out.to_host().tobytes(), want.tobytes())
    assert bad is None, ("first wrong message", bad)
    for b in (d_buf, d_off, d_out):
        b.free()


def _ragged(rng, n, lo, hi):
    """n random byte strings of lo <= length < hi."""
    lens = rng.integers(lo, hi, n)
    cut = np.concatenate([[0], np.cumsum(lens)])
    b = rng.integers(0, 256, int(cut[-1]), dtype=np.uint8).tobytes()
    return [b[cut[i]:cut[i + 1]] for i in range(n)]


def test_entries_sorted_with_overrides_vs_oracle(m, ctx, orc):
    """m.build_hash_tree over SORT_MIN + 7 ragged entries (keys, metadata,
    values of 0..600 bytes), about a fifth of them IsValueTruncated: the sorted
    k_entries_varlen with use_override (nb_key's class 0)."""
    n = SORT_MIN + 7
    rng = np.random.default_rng(14)
    keys = _ragged(rng, n, 1, 130)
    mds = _ragged(rng, n, 0, 12)
    vals = _ragged(rng, n, 0, 601)
    pick = rng.random(n) < 0.2
    assert 0.15 * n < pick.sum() < 0.25 * n
    ov = [orc.sha256(v) if p else None for v, p in zip(vals, pick)]
    vals2 = [b"" if p else v for v, p in zip(vals, pick)]
    with _Timed(ctx):
        eh, hv, lv = m.build_hash_tree(1, keys, vals2, mds, hval_overrides=ov, ctx=ctx)
        sorts = _sort_launches(ctx)
    assert sorts >= 1
    st, ohv, olv, oroot = orc.build_entries(1, keys, mds, vals)
    assert st == 0
    bad = _first_diff(hv.tobytes(), ohv.tobytes())
    assert bad is None, ("first wrong hVal, overridden", bad, bool(pick[bad]))
    bad = _first_diff(lv.tobytes(), olv.tobytes())
    assert bad is None, ("first wrong node", bad)
    assert eh == oroot


def _values_inputs(orc, seed, n, max_len, nbad):
    """Values, stored hVals (the oracle's) and stored lengths with the
    corruptions readValueAt rejects (immustore.go:3235), made the way
    test_oracle._values_case makes them: a flipped byte, a short read, a
    stored length above the bytes read, a wrong hVal; empty values."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    lens[:20] = 0
    off0 = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off0[1:])
    clean = orc.fill_random(int(off0[-1]), seed)
    hv = _orc_sha_batch(orc, clean, off0).copy()
    cb = clean.tobytes()
    vals = [cb[int(off0[i]):int(off0[i + 1])] for i in range(n)]
    vlen = lens.astype(np.uint64).copy()
    bad = np.zeros(n, bool)
    for i in rng.choice(n, nbad, replace=False):
        kind = int(rng.integers(0, 4))
        if kind == 0 and len(vals[i]):
            b = bytearray(vals[i])
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            vals[i] = bytes(b)
        elif kind == 1 and len(vals[i]):
            vals[i] = vals[i][:-1]           # short read: n < len(b)
        elif kind == 2:
            vlen[i] += np.uint64(1)          # stored length above the bytes read
        else:
            hv[i, int(rng.integers(0, 32))] ^= 0x80
        bad[i] = True
    off = np.zeros(n + 1, np.uint64)
    np.cumsum([len(v) for v in vals], out=off[1:])
    return np.frombuffer(b"".join(vals), np.uint8).copy(), off, hv, vlen, bad


def test_verify_values_sorted_vs_oracle(m, ctx, orc):
    """m.verify_values and mh_dev_verify_values_batch over SORT_MIN + 7 values
    of 0..300 bytes: the sorted k_sha_varlen with the read-side comparison."""
    from immustore_amd import _native as N
    n = SORT_MIN + 7
    vb, off, hv, vlen, bad = _values_inputs(orc, 31, n, 300, 700)
    assert vb.nbytes == int(off[-1])                  # exactly the bytes used
    oc, ost = orc.verify_values(vb, off, hv, vlen)
    assert oc == int(bad.sum()) and np.array_equal(ost != 0, bad)
    with _Timed(ctx):
        c, st = m.verify_values(vb, off, hv, vlen, ctx)
        sorts = _sort_launches(ctx)
    assert sorts >= 1
    assert c == oc and np.array_equal(st, ost), np.nonzero(st != ost)[0][:5]
    oc2, ost2 = orc.verify_values(vb, off, hv, None)
    c2, st2 = m.verify_values(vb, off, hv, None, ctx)
    assert c2 == oc2 and np.array_equal(st2, ost2)
    dv, do = DevBuf.from_host(ctx, vb), DevBuf.from_host(ctx, off)
    dlen, dh = DevBuf.from_host(ctx, vlen), DevBuf.from_host(ctx, hv)
    ds = _poison(ctx, 4 * n)
    with _Timed(ctx):
        N.check(N.load().mh_dev_verify_values_batch(ctx.handle, n, dv.ptr, do.ptr, dlen.ptr,
                                                    dh.ptr, ds.ptr))
        ctx.synchronize()
        sorts = _sort_launches(ctx)
    assert sorts >= 1
    got = ds.to_host(np.int32)
    assert np.array_equal(got, ost), np.nonzero(got != ost)[0][:5]
    for b in (dv, do, dlen, dh, ds):
        b.free()


# ------------------------------------- E: k_aht_perfect_t onto a tree with nodes
AHT_M = (1 << 19) + 5      # second batch: level 1 gets >= 2^18 new perfect nodes
AHT_N0 = (1, (1 << 18) - 1, (1 << 18) + 3)


@pytest.fixture(scope="module")
def aht_oracle(orc):
    """One payload stream and its oracle dLog, long enough for every case: a
    dLog does not depend on how the appends were batched, and the dLog of the
    first n appends is a prefix of it."""
    total = max(AHT_N0) + AHT_M
    pay = orc.fill_random(32 * total, 23).reshape(total, 32)
    o = orc.AHtree(total)
    o.append_batch(pay)
    return pay, o


@pytest.mark.parametrize("n0", AHT_N0)
def test_ahtree_perfect_table_onto_nonempty_tree(m, ctx, orc, aht_oracle, n0):
    """n0 appends, then AHT_M more in one batch (launch_ahtree_perfect: levels
    with >= 2^18 new perfect nodes take the grid-stride table kernel, here
    from a first node index past the tree's own): the whole dLog and the last
    root against the oracle."""
    pay, o = aht_oracle
    total = n0 + AHT_M
    assert (total >> 1) - (n0 >> 1) >= 1 << 18        # level 1 of the second batch
    t = m.AHtree(ctx)
    t.append_batch(pay[:n0])
    roots = t.append_batch(pay[n0:total], with_roots=True)
    assert t.size() == total
    want = o.dlog[:orc.nodes_upto(total)].tobytes()
    got = t.dlog()
    bad = _first_diff(got, want)
    assert bad is None, (n0, "first wrong dLog node", bad)
    st, oroot = o.root_at(total)
    assert st == 0 and t.root_at(total) == oroot and roots[-1].tobytes() == oroot
    st, oroot0 = o.root_at(n0)
    assert st == 0 and t.root_at(n0) == oroot0
    t.close()
