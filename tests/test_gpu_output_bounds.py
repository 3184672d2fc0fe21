"""A call writes only the bytes its contract names.

Every output that a kernel stores into sits in a gpu_util.Guarded buffer of
exactly the size include/immustore_merkle.h gives for it: 0xA5 everywhere,
4096 guard bytes before and after the payload inside one allocation.  Each case
asserts parity of the payload with the oracle (or with the host twin that an
existing test ties to the oracle) AND that every guard of every output is
intact; rows or bytes inside a payload that the header says are not written
must still hold 0xA5.  The shapes are the smallest on both sides of each
kernel's tile.

call                                   outputs guarded                  tile edges used
-------------------------------------  -------------------------------  ---------------------------------
mh_dev_fill_random, _fill_keys_be64    dptr                             8-byte words, 256-lane workgroups
mh_dev_sha256_batch                    out                              256-lane workgroup: n 1, 255, 256,
mh_dev_verify_values_batch             status                            257; the length-class sort (n >=
                                                                         16384): 16385, 0..3 blocks
mh_dev_htree_build_digests             levels, root                     DIGEST_WIDTHS x MH_DIGEST_LPL 1/2/4
mh_dev_htree_reduce_nodes              levels, root                     DIGEST_WIDTHS (kSmallTreeMax arms)
mh_dev_htree_build_entries_fixed       hvals_out, levels, root          DIGEST_WIDTHS x MH_LPL 1/2/4 x
                                                                         MH_WG_LEVELS 0/1/8 x MH_FIXED_FAST
mh_dev_htree_build_entries             hvals_out, levels, root          DIGEST_WIDTHS (one lane per entry)
mh_dev_htree_inclusion_proof_batch     terms, nterms, status            256-lane workgroup, one row per
mh_dev_ahtree_proof_batch              terms, nterms, status             lane: n 1, 63, 64, 65; max_terms =
                                                                         longest proof and one less
mh_dev_htree_verify_inclusion_batch    ok                               ok is n BYTES: n 1, 3, 5, 63, 65,
mh_dev_ahtree_verify_batch             ok, eval_out                      257 (a packed dword would overrun)
mh_dev_ahtree_append_batch             dlog, roots_out                  n0 0, 1, 2^8 - 1, 2^8; m 1, 300
mh_dev_ahtree_append_batch_logs        dlog, plog, clog, roots_out      same n0; records at offsets 0, 4, 1
mh_dev_ahtree_log_records              plog, clog                       m 1, 255, 256, 257, 1000
mh_dev_ahtree_append_local /           dlog (per rank)                  shards of 2^k: 2 ranks x 2^11,
  _put_shard_roots / _append_spine     roots_out                         3 ranks x 2^10 with a short last
mh_dev_ahtree_peaks                    peaks_out (host)                 n 1, 255, 256, 300
mh_dev_tx_alh_batch                    scratch, inner_out, alh_out      256-lane workgroup: n 1, 255, 256,
                                                                         257; md lengths 0..268
mh_dev_htree_inclusion_proof_pb_batch  out, off, status, scratch        64 messages per wave: n 1, 63, 64,
mh_dev_dual_proof_v2_pb_batch          out, off, status, scratch         65, 257; phases 1, 2, 3; out_cap
                                                                         exact, one short, 0
mh_verifiable_answer_pb_batch          out (device)                     out_cap exact and one short
mh_txlog_validate / _resident /        hdrs, alh, status (pinned;       4R records per workgroup, R = 64 /
  _clog                                 _clog: device too)               lanes: ntx 1, 4R - 1, 4R, 4R + 1 for
                                                                         1, 2, 4, 8, 16 lanes; both
                                                                         MH_TXLOG_KERNEL values; the last
                                                                         chunk of a 16 MiB pinned log
mh_multi_dev_htree_build_entries_fixed hvals_out, levels, top_levels,   2 contexts on device 0, n_per_dev
                                        root (per device)                1, 256
mh_multi_dev_ahtree_append_batch       dlog, roots_out (per range)      2 ranges on device 0, n0 = 0

Guarded elsewhere, each with the kernel it guards: mh_dev_ahtree_append_range,
mh_dev_ahtree_range_local / _finish (test_gpu_ahtree_wide.py),
mh_export_tx_batch, mh_tx_answer_pb_batch (test_gpu_tx_spec.py,
test_gpu_export.py), mh_dev_dual_proof_pb_batch (test_gpu_dual_v1_gen.py).

The alignment cases follow the header: a device digest array that the kernels
move with 16-byte vector accesses is refused 4 bytes off a 16-byte boundary
with MH_ERR_ILLEGAL_ARGUMENTS and nothing written; an argument stated as "any
alignment" gets one parity + guard case at an odd offset.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from gpu_util import FILL, GUARD, Guarded
from test_gpu_dispatch_arms import DIGEST_WIDTHS

pytestmark = pytest.mark.gpu

ILLEGAL = 2  # MH_ERR_ILLEGAL_ARGUMENTS


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


@pytest.fixture(scope="module")
def L():
    from immustore_amd import _native as N
    assert N.MH_ERR_ILLEGAL_ARGUMENTS == ILLEGAL
    return N.load()


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


def _dev(a):
    """A host array on the device, exactly its bytes."""
    import torch
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if b.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(b.copy()).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()  # fills and copies ran on torch's stream, the calls run on ctx's


def ok(rc):
    from immustore_amd import _native as N
    N.check(rc)


class Outs:
    """The Guarded outputs of one call."""

    def __init__(self):
        self.all = []

    def new(self, nbytes, **kw):
        g = Guarded(nbytes, **kw)
        self.all.append(g)
        return g

    def intact(self):
        return all(g.guards_intact() for g in self.all)

    def untouched(self):
        return all(g.untouched() for g in self.all)


def _fill_rows(n, width=32):
    return np.full((n, width), FILL, np.uint8)


def _sha_all(orc, buf, off):
    """The oracle's SHA-256 of every range buf[off[i]:off[i+1]] -> (n, 32)."""
    n = len(off) - 1
    b = np.ascontiguousarray(buf, np.uint8)
    if b.size == 0:
        b = np.zeros(1, np.uint8)
    st, hv, _, _ = orc.build_entries_csr(1, np.zeros(1, np.uint8), np.zeros(n + 1, np.uint64), None,
                                         None, b, np.ascontiguousarray(off, np.uint64),
                                         want_levels=False)
    assert st == 0
    return hv


# ------------------------------------------------------------------ the helper itself
def test_guarded_reports_one_byte_in_either_band(m, ctx, L):
    """One byte copied into the last byte of the front band, and in a second
    buffer into the first byte of the back band: guards_intact() reports each,
    for an aligned and an offset payload; the payload itself is not blamed."""
    one = np.array([0x5A], np.uint8)
    for offset in (0, 4):
        a, b, c = Guarded(96, offset), Guarded(96, offset), Guarded(96, offset)
        _sync()
        assert a.ptr % 16 == offset and a.payload().size == 96
        assert a.guards_intact() and b.guards_intact() and a.untouched() and b.untouched()
        ok(L.mh_memcpy_h2d(ctx.handle, a.ptr - 1, one.ctypes.data, 1))
        ok(L.mh_memcpy_h2d(ctx.handle, b.ptr + b.n, one.ctypes.data, 1))
        ok(L.mh_memcpy_h2d(ctx.handle, c.ptr + c.n - 1, one.ctypes.data, 1))
        ctx.synchronize()
        assert not a.guards_intact() and not a.front_intact() and a.back_intact()
        assert not b.guards_intact() and b.front_intact() and not b.back_intact()
        assert c.guards_intact() and not c.untouched()           # the payload's last byte
        assert (a.payload() == FILL).all() and (b.payload() == FILL).all()
        assert c.payload()[-1] == 0x5A
    # the pinned flavour, poked from the host
    p, q = Guarded(40, 4, pinned=True), Guarded(40, pinned=True)
    assert p.guards_intact() and q.guards_intact() and p.ptr % 16 == 4
    p.t[p.lo - 1] = 0
    q.t[q.lo + q.n] = 0
    assert not p.front_intact() and p.back_intact() and not p.guards_intact()
    assert q.front_intact() and not q.back_intact() and not q.guards_intact()
    p.free()
    q.free()


# ------------------------------------------------ mh_dev_fill_random, _fill_keys_be64
def test_fill_outputs(m, ctx, L, orc):
    """The synthetic-data fills: nbytes on both sides of the 8-byte word and of
    a 256-lane workgroup's 2048 bytes, n keys on both sides of 256."""
    for nbytes in (1, 7, 8, 9, 2047, 2048, 2049, 100003):
        g = Guarded(nbytes)
        _sync()
        ok(L.mh_dev_fill_random(ctx.handle, g.ptr, nbytes, 5 + nbytes))
        ctx.synchronize()
        assert np.array_equal(g.payload(), orc.fill_random(nbytes, 5 + nbytes)), nbytes
        assert g.guards_intact(), nbytes
    first = (1 << 40) - 3
    for n in (1, 255, 256, 257):
        g = Guarded(n * 8)
        _sync()
        ok(L.mh_dev_fill_keys_be64(ctx.handle, g.ptr, n, first))
        ctx.synchronize()
        assert g.payload().tobytes() == np.arange(first, first + n, dtype=">u8").tobytes(), n
        assert g.guards_intact(), n


# ------------------------------------------------ mh_dev_sha256_batch, _verify_values_batch
def _values_case(orc, n, seed, max_len):
    """n messages of 0..max_len bytes, their digests with a few damaged, the
    stored lengths with a few wrong -> (buf, off, sha, hv, vlen, status)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    lens[:min(n, 4)] = (0, 55, 56, 64)[:min(n, 4)]
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    buf = orc.fill_random(max(int(off[-1]), 1), seed)[:int(off[-1])]
    sha = _sha_all(orc, buf, off)
    hv = sha.copy()
    vlen = lens.astype(np.uint64)
    for i in rng.choice(n, max(1, n // 9), replace=False):
        if i % 2:
            hv[i, int(rng.integers(0, 32))] ^= 0x10
        else:
            vlen[i] += np.uint64(1)
    _, st = orc.verify_values(buf, off, hv, vlen)
    assert st.any()
    return buf, off, sha, hv, vlen, st


@pytest.mark.parametrize("n", [1, 255, 256, 257, 16385])
def test_sha256_and_verify_values_outputs(m, ctx, L, orc, n):
    """out is n * 32 bytes and status n * 4, at the workgroup edges and once
    sorted (n = 16385, messages of 0 to 3 blocks); the message bytes start at
    offsets 0 and 1 of their allocation (buf: any alignment)."""
    buf, off, sha, hv, vlen, st = _values_case(orc, n, 300 + n, 3 * 64 - 9)
    for shift in (0, 1):
        d_buf = _dev(np.concatenate([np.zeros(shift, np.uint8), buf]))
        d_off = _dev(off + np.uint64(shift))
        d_hv, d_vl = _dev(hv), _dev(vlen)
        o = Outs()
        out, status = o.new(n * 32), o.new(n * 4)
        _sync()
        ok(L.mh_dev_sha256_batch(ctx.handle, d_buf.data_ptr(), d_off.data_ptr(), n, out.ptr))
        ok(L.mh_dev_verify_values_batch(ctx.handle, n, d_buf.data_ptr(), d_off.data_ptr(),
                                        d_vl.data_ptr(), d_hv.data_ptr(), status.ptr))
        ctx.synchronize()
        assert np.array_equal(out.rows(), sha), (n, shift)
        assert np.array_equal(status.view(np.int32), st), (n, shift)
        assert o.intact(), (n, shift)


def test_sha256_and_verify_values_refuse_misaligned_digests(m, ctx, L, orc):
    buf, off, sha, hv, vlen, st = _values_case(orc, 5, 9, 100)
    d_buf, d_off, d_vl = _dev(buf), _dev(off), _dev(vlen)
    g_hv = Guarded(5 * 32 + 16)
    g_hv.put(np.concatenate([np.zeros(4, np.uint8), hv.reshape(-1)]))
    o = Outs()
    out, status = o.new(5 * 32 + 16), o.new(5 * 4)
    _sync()
    assert L.mh_dev_sha256_batch(ctx.handle, d_buf.data_ptr(), d_off.data_ptr(), 5,
                                 out.ptr + 4) == ILLEGAL
    assert L.mh_dev_verify_values_batch(ctx.handle, 5, d_buf.data_ptr(), d_off.data_ptr(),
                                        d_vl.data_ptr(), g_hv.ptr + 4, status.ptr) == ILLEGAL
    ctx.synchronize()
    assert o.untouched()


# ------------------------------------------------------------------ htree builds
@pytest.fixture(scope="module")
def digest_sets(orc):
    """width -> (digests, levels (L, 32), root)"""
    out = {}
    for w in DIGEST_WIDTHS:
        d = orc.fill_random(w * 32, 7100 + w).reshape(w, 32)
        lv, root = orc.htree_build(d)
        out[w] = (d, lv, root)
    return out


def _root_rows(root):
    return np.frombuffer(root, np.uint8).reshape(1, 32)


@pytest.mark.parametrize("lpl", ["1", "2", "4"])
def test_build_digests_outputs(m, ctx, L, digest_sets, lpl):
    """levels is exactly mh_htree_levels_len(n) * 32 bytes, root 32, with and
    without a root pointer, under every MH_DIGEST_LPL."""
    with _Env(MH_DIGEST_LPL=lpl):
        for w in DIGEST_WIDTHS:
            d, olv, oroot = digest_sets[w]
            dd = _dev(d)
            for want_root in (True, False):
                o = Outs()
                lv, rt = o.new(L.mh_htree_levels_len(w) * 32), o.new(32)
                _sync()
                ok(L.mh_dev_htree_build_digests(ctx.handle, dd.data_ptr(), w, lv.ptr,
                                                rt.ptr if want_root else None))
                ctx.synchronize()
                case = (lpl, w, want_root)
                assert np.array_equal(lv.rows(), olv), case
                assert np.array_equal(rt.rows(), _root_rows(oroot) if want_root else _fill_rows(1)), case
                assert o.intact(), case


def test_reduce_nodes_outputs(m, ctx, L, digest_sets):
    """The leaf level of the oracle's tree as the nodes: the levels are the
    oracle's, at every width of DIGEST_WIDTHS (the one-launch arm up to
    kSmallTreeMax and the copy + reduce arm above it)."""
    for w in DIGEST_WIDTHS:
        _, olv, oroot = digest_sets[w]
        dn = _dev(olv[:w])
        for want_root in (True, False):
            o = Outs()
            lv, rt = o.new(L.mh_htree_levels_len(w) * 32), o.new(32)
            _sync()
            ok(L.mh_dev_htree_reduce_nodes(ctx.handle, dn.data_ptr(), w, lv.ptr,
                                           rt.ptr if want_root else None))
            ctx.synchronize()
            assert np.array_equal(lv.rows(), olv), (w, want_root)
            assert np.array_equal(rt.rows(), _root_rows(oroot) if want_root else _fill_rows(1)), w
            assert o.intact(), (w, want_root)


@pytest.fixture(scope="module")
def fixed_sets(orc):
    """width -> keys (w, 8), vals (w, 128) and the oracle's (hvals, levels, root)"""
    out = {}
    for w in DIGEST_WIDTHS:
        keys = orc.fill_random(w * 8, 8200 + w).reshape(w, 8)
        vals = orc.fill_random(w * 128, 7200 + w).reshape(w, 128)
        out[w] = (keys, vals) + orc.build_entries_fixed(1, keys, vals)
    return out


@pytest.mark.parametrize("wgl", ["0", "1", "8"])
@pytest.mark.parametrize("lpl", ["1", "2", "4"])
def test_build_entries_fixed_outputs(m, ctx, L, fixed_sets, lpl, wgl):
    """hvals_out n * 32, levels mh_htree_levels_len(n) * 32, root 32: with all
    three and with levels alone, the fast and the general kernel, under every
    MH_LPL / MH_WG_LEVELS."""
    for w in DIGEST_WIDTHS:
        keys, vals, ohv, olv, oroot = fixed_sets[w]
        dk, dv = _dev(keys), _dev(vals)
        for fast in (None, "0"):
            for extra in (True, False):
                o = Outs()
                hv, lv, rt = o.new(w * 32), o.new(L.mh_htree_levels_len(w) * 32), o.new(32)
                _sync()
                with _Env(MH_LPL=lpl, MH_WG_LEVELS=wgl, MH_FIXED_FAST=fast):
                    ok(L.mh_dev_htree_build_entries_fixed(
                        ctx.handle, 1, w, dk.data_ptr(), 8, dv.data_ptr(), 128,
                        hv.ptr if extra else None, lv.ptr, rt.ptr if extra else None))
                ctx.synchronize()
                case = (lpl, wgl, w, fast, extra)
                assert np.array_equal(lv.rows(), olv), case
                assert np.array_equal(hv.rows(), ohv if extra else _fill_rows(w)), case
                assert np.array_equal(rt.rows(), _root_rows(oroot) if extra else _fill_rows(1)), case
                assert o.intact(), case


def test_build_entries_csr_outputs(m, ctx, L, orc):
    """The general CSR build: ragged keys, metadata and values, a fifth of the
    hVals overridden; with hvals_out and root, and with levels alone."""
    for w in DIGEST_WIDTHS:
        rng = np.random.default_rng(600 + w)
        ko, mo, vo = (np.zeros(w + 1, np.uint64) for _ in range(3))
        ko[1:] = np.cumsum(rng.integers(1, 40, w))
        mo[1:] = np.cumsum(rng.integers(0, 12, w))
        vo[1:] = np.cumsum(rng.integers(0, 300, w))
        kb, mb, vb = (orc.fill_random(int(x[w]) + 1, 11 * w + k) for k, x in enumerate((ko, mo, vo)))
        use = (rng.random(w) < 0.2).astype(np.uint8)
        ov = orc.fill_random(w * 32, 5 + w).reshape(w, 32)
        st, ohv, olv, oroot = orc.build_entries_csr(1, kb, ko, mb, mo, vb, vo, ov=ov, use=use)
        assert st == 0
        dev = [_dev(x) for x in (kb[:int(ko[w])], ko, mb[:int(mo[w])], mo, vb[:int(vo[w])], vo, ov, use)]
        p = [t.data_ptr() for t in dev]
        for extra in (True, False):
            o = Outs()
            hv, lv, rt = o.new(w * 32), o.new(L.mh_htree_levels_len(w) * 32), o.new(32)
            _sync()
            ok(L.mh_dev_htree_build_entries(ctx.handle, 1, w, p[0], p[1], p[2], p[3], p[4], p[5], p[6],
                                            p[7], hv.ptr if extra else None, lv.ptr,
                                            rt.ptr if extra else None))
            ctx.synchronize()
            assert np.array_equal(lv.rows(), olv), (w, extra)
            assert np.array_equal(hv.rows(), ohv if extra else _fill_rows(w)), (w, extra)
            assert np.array_equal(rt.rows(), _root_rows(oroot) if extra else _fill_rows(1)), (w, extra)
            assert o.intact(), (w, extra)


def test_htree_builds_refuse_misaligned_digest_arrays(m, ctx, L, digest_sets, fixed_sets):
    """levels, hvals_out, root, digests / nodes and hval_override 4 bytes off a
    16-byte boundary: MH_ERR_ILLEGAL_ARGUMENTS, nothing launched or written."""
    w = 5
    d, olv, _ = digest_sets[w]
    keys, vals = fixed_sets[w][:2]
    g_in = Guarded(w * 32 + 16)
    g_in.put(np.concatenate([np.zeros(4, np.uint8), d.reshape(-1)]))
    dd, dk, dv = _dev(d), _dev(keys), _dev(vals)
    off8 = _dev(np.arange(w + 1, dtype=np.uint64) * 8)
    off128 = _dev(np.arange(w + 1, dtype=np.uint64) * 128)
    use = _dev(np.zeros(w, np.uint8))
    o = Outs()
    nl = L.mh_htree_levels_len(w)
    lv, hv, rt = o.new(nl * 32 + 16), o.new(w * 32 + 16), o.new(48)
    _sync()
    h = ctx.handle
    for bad in ("levels", "root", "in"):
        a = dict(levels=lv.ptr, root=rt.ptr, inp=dd.data_ptr())
        if bad == "in":
            a["inp"] = g_in.ptr + 4
        else:
            a[bad] += 4
        assert L.mh_dev_htree_build_digests(h, a["inp"], w, a["levels"], a["root"]) == ILLEGAL, bad
        assert L.mh_dev_htree_reduce_nodes(h, a["inp"], w, a["levels"], a["root"]) == ILLEGAL, bad
    for bad in ("levels", "root", "hvals", "override"):
        a = dict(levels=lv.ptr, root=rt.ptr, hvals=hv.ptr, override=dd.data_ptr())
        if bad == "override":
            a["override"] = g_in.ptr + 4
        else:
            a[bad] += 4
        if bad != "override":
            assert L.mh_dev_htree_build_entries_fixed(h, 1, w, dk.data_ptr(), 8, dv.data_ptr(), 128,
                                                      a["hvals"], a["levels"], a["root"]) == ILLEGAL, bad
        assert L.mh_dev_htree_build_entries(h, 1, w, dk.data_ptr(), off8.data_ptr(), None, None,
                                            dv.data_ptr(), off128.data_ptr(), a["override"],
                                            use.data_ptr(), a["hvals"], a["levels"],
                                            a["root"]) == ILLEGAL, bad
    ctx.synchronize()
    assert o.untouched()


# ------------------------------------------------------------------ proof generators
PROOF_N = (1, 63, 64, 65)
HT_W = 37          # proofs of 6, 4 and 2 terms; the last leaf's is the shortest


@pytest.fixture(scope="module")
def htree37(orc):
    d = orc.fill_random(HT_W * 32, 37).reshape(HT_W, 32)
    lv, root = orc.htree_build(d)
    proofs = [orc.htree_inclusion_proof(lv, HT_W, i)[1] for i in range(HT_W)]
    return d, lv, root, proofs


def _check_proof_rows(terms, nterms, status, mt, want, what):
    """want[p] = (status, nterms, terms or None).  Of a good row the proof's
    terms, the rest of it and every refused row still 0xA5."""
    n = len(want)
    got = terms.payload().reshape(n, mt, 32)
    nt, st = nterms.view(np.uint32), status.view(np.int32)
    for p, (est, ent, et) in enumerate(want):
        assert (int(st[p]), int(nt[p])) == (est, ent), what + (p,)
        k = ent if est == 0 else 0
        if k:
            assert np.array_equal(got[p, :k], et), what + (p,)
        assert (got[p, k:] == FILL).all(), what + (p, "kept bytes")


@pytest.mark.parametrize("n", PROOF_N)
def test_htree_proof_batch_outputs(m, ctx, L, orc, htree37, n):
    """terms n * max_terms * 32, nterms and status n * 4 each; max_terms the
    longest proof and one less (the longest rows are then refused), leaves past
    the width mixed in."""
    _, lv, _, proofs = htree37
    rng = np.random.default_rng(n)
    leaf = np.concatenate([[HT_W - 1], rng.integers(0, HT_W + 3, n)])[:n].astype(np.uint64)
    if n > 1:
        leaf[1], leaf[-1] = 0, HT_W
    longest = max(len(p) for p in proofs)
    assert longest == 6 and len(proofs[HT_W - 1]) < longest
    dlv, dleaf = _dev(lv), _dev(leaf)
    for mt in (longest, longest - 1):
        want = []
        for i in leaf:
            if i >= HT_W:
                want.append((ILLEGAL, 0, None))
            elif len(proofs[int(i)]) > mt:
                want.append((ILLEGAL, len(proofs[int(i)]), None))
            else:
                want.append((0, len(proofs[int(i)]), proofs[int(i)]))
        o = Outs()
        terms, nterms, status = o.new(n * mt * 32), o.new(n * 4), o.new(n * 4)
        _sync()
        ok(L.mh_dev_htree_inclusion_proof_batch(ctx.handle, dlv.data_ptr(), HT_W, n, dleaf.data_ptr(),
                                                terms.ptr, mt, nterms.ptr, status.ptr))
        ctx.synchronize()
        _check_proof_rows(terms, nterms, status, mt, want, ("htree", n, mt))
        assert o.intact(), (n, mt)


AHT_SIZE = 300


@pytest.fixture(scope="module")
def aht300(orc):
    """An oracle ahtree of 556 appends (the append cases use all of it, the
    proof cases its first 300) -> (payloads, tree, roots[k] = RootAt(k + 1))."""
    total = 256 + 300
    pay = orc.fill_random(total * 32, 77).reshape(total, 32)
    o = orc.AHtree(total)
    o.append_batch(pay)
    roots = np.stack([np.frombuffer(o.root_at(k)[1], np.uint8) for k in range(1, total + 1)])
    return pay, o, roots


def _aht_pairs(rng, n):
    j = rng.integers(1, AHT_SIZE + 1, n).astype(np.uint64)
    i = np.array([int(rng.integers(1, int(x) + 1)) for x in j], np.uint64)
    j[0], i[0] = AHT_SIZE, 1                      # a longest proof
    if n > 3:
        i[1], j[1] = 9, 5                         # i > j
        i[2], j[2] = 1, AHT_SIZE + 1              # j > size
        i[3], j[3] = 0, 0                         # j == 0
    return i, j


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", PROOF_N)
def test_ahtree_proof_batch_outputs(m, ctx, L, orc, aht300, n, kind):
    from immustore_amd import _native as N
    _, o, _ = aht300
    i, j = _aht_pairs(np.random.default_rng(10 * n + kind), n)
    # the oracle reads the first 300 appends of its tree: a dLog is a prefix
    view = orc.AHtree.__new__(orc.AHtree)
    view.size, view.dlog = AHT_SIZE, o.dlog
    # j == 0 is MH_ERR_UNEXISTENT_DATA by the header (Go fails the read, the
    # oracle would read node -1): asked of the oracle as j > size, the same status
    zero = j == 0
    ot, ont, ost = view.proof_batch(kind, np.where(zero, 1, i), np.where(zero, AHT_SIZE + 1, j), cap=64)
    assert n < 4 or (ost[1] == ILLEGAL and ost[2] == ost[3] == N.MH_ERR_UNEXISTENT_DATA)
    longest = int(ont.max())
    assert longest >= 6
    ddlog = _dev(o.dlog[:orc.nodes_upto(AHT_SIZE)])
    di, dj = _dev(i), _dev(j)
    for mt in (longest, longest - 1):
        want = []
        for p in range(n):
            if ost[p]:
                want.append((int(ost[p]), 0, None))
            elif ont[p] > mt:
                want.append((ILLEGAL, int(ont[p]), None))
            else:
                want.append((0, int(ont[p]), ot[p, :ont[p]]))
        assert any(w[0] == ILLEGAL and w[1] for w in want) == (mt < longest)
        outs = Outs()
        terms, nterms, status = outs.new(n * mt * 32), outs.new(n * 4), outs.new(n * 4)
        _sync()
        ok(L.mh_dev_ahtree_proof_batch(ctx.handle, kind, ddlog.data_ptr(), AHT_SIZE, n, di.data_ptr(),
                                       dj.data_ptr(), terms.ptr, mt, nterms.ptr, status.ptr))
        ctx.synchronize()
        _check_proof_rows(terms, nterms, status, mt, want, ("ahtree", kind, n, mt))
        assert outs.intact(), (kind, n, mt)


def test_proof_batches_refuse_misaligned_terms(m, ctx, L, orc, htree37, aht300):
    _, lv, _, _ = htree37
    _, o, _ = aht300
    n, mt = 3, 8
    dlv, ddlog = _dev(lv), _dev(o.dlog[:orc.nodes_upto(AHT_SIZE)])
    idx = _dev(np.array([1, 2, 3], np.uint64))
    outs = Outs()
    terms, nterms, status = outs.new(n * mt * 32 + 16), outs.new(n * 4), outs.new(n * 4)
    _sync()
    assert L.mh_dev_htree_inclusion_proof_batch(ctx.handle, dlv.data_ptr(), HT_W, n, idx.data_ptr(),
                                                terms.ptr + 4, mt, nterms.ptr, status.ptr) == ILLEGAL
    for kind in (0, 1):
        assert L.mh_dev_ahtree_proof_batch(ctx.handle, kind, ddlog.data_ptr(), AHT_SIZE, n,
                                           idx.data_ptr(), idx.data_ptr(), terms.ptr + 4, mt,
                                           nterms.ptr, status.ptr) == ILLEGAL
    ctx.synchronize()
    assert outs.untouched()


# ------------------------------------------------------------------ proof verifiers
VERIFY_N = (1, 3, 5, 63, 65, 257)


@pytest.mark.parametrize("n", VERIFY_N)
def test_htree_verify_ok_bytes(m, ctx, L, orc, htree37, n):
    """ok is n BYTES; every fourth proof is damaged."""
    d, lv, root, proofs = htree37
    rng = np.random.default_rng(n)
    leaf = rng.integers(0, HT_W, n).astype(np.uint64)
    leaf[0] = HT_W - 1
    toff = np.zeros(n + 1, np.uint64)
    toff[1:] = np.cumsum([len(proofs[int(i)]) for i in leaf])
    terms = np.concatenate([proofs[int(i)] for i in leaf]).copy()
    digs = d[leaf.astype(np.int64)].copy()
    roots = np.tile(np.frombuffer(root, np.uint8), (n, 1))
    width = np.full(n, HT_W, np.uint64)
    for p in range(0, n, 4):
        (digs if p % 8 else roots)[p, 7] ^= 1
    _, want = orc.htree_verify_csr(leaf, width, toff, terms, digs, roots)
    assert want.any() or n < 3
    dev = [_dev(x) for x in (leaf, width, toff, terms, digs, roots)]
    o = Outs()
    okb = o.new(n)
    _sync()
    ok(L.mh_dev_htree_verify_inclusion_batch(ctx.handle, n, *[t.data_ptr() for t in dev], okb.ptr))
    ctx.synchronize()
    assert np.array_equal(okb.payload(), want), n
    assert o.intact(), n


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", VERIFY_N)
def test_ahtree_verify_ok_bytes_and_eval(m, ctx, L, orc, aht300, n, kind):
    """ok is n bytes, eval_out n * 32 (n * 64 for CONSISTENCY) or NULL."""
    _, o, roots = aht300
    rng = np.random.default_rng(100 * kind + n)
    j = rng.integers(1, AHT_SIZE + 1, n).astype(np.uint64)
    i = np.array([int(rng.integers(1, int(x) + 1)) for x in j], np.uint64)
    if n > 1:
        i[1] = j[1]
    if kind == 2:
        i = j.copy()   # VerifyLastInclusion: the proof of the last leaf of a tree of size i
    ot, ont, ost = o.proof_batch(1 if kind == 1 else 0, i, j, cap=64)
    assert not ost.any()
    toff = np.zeros(n + 1, np.uint64)
    toff[1:] = np.cumsum(ont.astype(np.uint64))
    terms = np.concatenate([ot[p, :ont[p]] for p in range(n)] + [np.zeros((1, 32), np.uint8)])
    leaf = np.stack([o.dlog[orc.nodes_until(int(x))] for x in i])
    a = roots[i.astype(np.int64) - 1].copy() if kind == 1 else leaf.copy()
    b = roots[j.astype(np.int64) - 1].copy()
    for p in range(2, n, 4):
        (a if p % 8 == 2 else b)[p, 3] ^= 0x20
    _, want = orc.ahtree_verify_batch(kind, i, j, toff, terms, a, b)
    oev, odef = orc.ahtree_eval_batch(kind, i, j, toff, terms, a)
    assert want[0] and (n < 3 or not want.all())
    w = 64 if kind == 1 else 32
    want_ev = oev.copy()
    want_ev[~odef] = 0          # CONSISTENCY with no walk: 64 zero bytes (the header)
    assert odef.all() or kind == 1
    dev = [_dev(x) for x in (i, j, toff, terms, a, b)]
    for with_eval in (True, False):
        outs = Outs()
        okb, ev = outs.new(n), outs.new(n * w)
        _sync()
        ok(L.mh_dev_ahtree_verify_batch(ctx.handle, kind, n, *[t.data_ptr() for t in dev], okb.ptr,
                                        ev.ptr if with_eval else None))
        ctx.synchronize()
        assert np.array_equal(okb.payload(), want), (kind, n)
        assert np.array_equal(ev.payload().reshape(n, w), want_ev if with_eval else _fill_rows(n, w)), \
            (kind, n, with_eval)
        assert outs.intact(), (kind, n, with_eval)


def test_verifiers_refuse_misaligned_digest_arrays(m, ctx, L, orc, htree37, aht300):
    """terms, digests, roots / a, b and eval_out 4 bytes off: refused, ok and
    eval_out untouched."""
    d, lv, root, proofs = htree37
    n = 3
    src = Guarded(64 * 32)
    src.put(np.concatenate([np.zeros(4, np.uint8), orc.fill_random(63 * 32, 1)]))
    good = _dev(orc.fill_random(64 * 32, 2))
    u = _dev(np.array([1, 2, 3, 4], np.uint64))
    toff = _dev(np.array([0, 2, 4, 6], np.uint64))
    outs = Outs()
    okb, ev = outs.new(n), outs.new(n * 64 + 16)
    _sync()
    h, g, bad = ctx.handle, good.data_ptr(), src.ptr + 4
    for k in range(3):
        arrs = [g, g, g]
        arrs[k] = bad
        assert L.mh_dev_htree_verify_inclusion_batch(h, n, u.data_ptr(), u.data_ptr(), toff.data_ptr(),
                                                     arrs[0], arrs[1], arrs[2], okb.ptr) == ILLEGAL, k
        for kind in (0, 1, 2):
            assert L.mh_dev_ahtree_verify_batch(h, kind, n, u.data_ptr(), u.data_ptr(), toff.data_ptr(),
                                                arrs[0], arrs[1], arrs[2], okb.ptr, ev.ptr) == ILLEGAL
    for kind in (0, 1, 2):
        assert L.mh_dev_ahtree_verify_batch(h, kind, n, u.data_ptr(), u.data_ptr(), toff.data_ptr(),
                                            g, g, g, okb.ptr, ev.ptr + 4) == ILLEGAL
    ctx.synchronize()
    assert outs.untouched()


# ------------------------------------------------------------------ ahtree appends
APPEND_N0 = (0, 1, 255, 256)
APPEND_M = (1, 300)


def _expected_logs(orc, pay, p_off0):
    """The oracle's pLog / cLog record streams of a batch (ahtree.go:266-282,
    341-351); they do not depend on the tree the batch is appended to."""
    pl, cl = orc.AHtree(len(pay)).append_batch_logs(pay, p_off0)
    assert pl[:4] == struct.pack(">I", pay.shape[1]) and cl[:8] == struct.pack(">Q", p_off0)
    return np.frombuffer(pl, np.uint8), np.frombuffer(cl, np.uint8)


@pytest.mark.parametrize("logs", [False, True])
@pytest.mark.parametrize("n0", APPEND_N0)
def test_ahtree_append_outputs(m, ctx, L, orc, aht300, n0, logs):
    """dlog is exactly nodes_upto(n0 + m) * 32 bytes and holds the oracle's
    first nodes_upto(n0) nodes, which stay as they are; roots_out m * 32; plog
    m * (4 + plen) and clog m * 12, at offsets 0, 4 and 1 of a 16-byte
    boundary (records: any alignment)."""
    pay, o, roots = aht300
    for m_ in APPEND_M:
        lo, hi = orc.nodes_upto(n0), orc.nodes_upto(n0 + m_)
        dp = _dev(pay[n0:n0 + m_])
        epl, ecl = _expected_logs(orc, pay[n0:n0 + m_], 777)
        for with_roots, shift in ((True, 0), (False, 4), (True, 1)) if logs else ((True, 0), (False, 0)):
            outs = Outs()
            dl, ro = outs.new(hi * 32), outs.new(m_ * 32)
            dl.put(o.dlog[:lo])
            case = (n0, m_, logs, with_roots, shift)
            if logs:
                pl, cl = outs.new(m_ * 36, offset=shift), outs.new(m_ * 12, offset=shift)
                _sync()
                ok(L.mh_dev_ahtree_append_batch_logs(ctx.handle, dl.ptr, n0, dp.data_ptr(), m_, 32, 777,
                                                     pl.ptr, cl.ptr, ro.ptr if with_roots else None))
                ctx.synchronize()
                assert np.array_equal(pl.payload(), epl) and np.array_equal(cl.payload(), ecl), case
            else:
                _sync()
                ok(L.mh_dev_ahtree_append_batch(ctx.handle, dl.ptr, n0, dp.data_ptr(), m_, 32,
                                                ro.ptr if with_roots else None))
                ctx.synchronize()
            assert np.array_equal(dl.rows(), o.dlog[:hi]), case
            assert np.array_equal(ro.rows(), roots[n0:n0 + m_] if with_roots else _fill_rows(m_)), case
            assert outs.intact(), case


def test_ahtree_appends_refuse_misaligned_digest_arrays(m, ctx, L, orc, aht300):
    """dlog or roots_out 4 bytes off a 16-byte boundary: refused, nothing written."""
    pay, _, _ = aht300
    m_ = 5
    dp = _dev(pay[:m_])
    outs = Outs()
    dl, ro = outs.new(orc.nodes_upto(m_) * 32 + 16), outs.new(m_ * 32 + 16)
    pl, cl = outs.new(m_ * 36), outs.new(m_ * 12)
    _sync()
    h = ctx.handle
    for a, b in ((4, 0), (0, 4)):
        assert L.mh_dev_ahtree_append_batch(h, dl.ptr + a, 0, dp.data_ptr(), m_, 32, ro.ptr + b) == ILLEGAL
        assert L.mh_dev_ahtree_append_batch_logs(h, dl.ptr + a, 0, dp.data_ptr(), m_, 32, 0, pl.ptr,
                                                 cl.ptr, ro.ptr + b) == ILLEGAL
        assert L.mh_dev_ahtree_append_spine(h, dl.ptr + a, 0, m_, ro.ptr + b) == ILLEGAL
        assert L.mh_dev_ahtree_append_range(h, dl.ptr + a, 0, None, dp.data_ptr(), m_, 32,
                                            ro.ptr + b) == ILLEGAL
    assert L.mh_dev_ahtree_append_local(h, dl.ptr + 4, 0, dp.data_ptr(), m_, 32, 2) == ILLEGAL
    assert L.mh_dev_ahtree_put_shard_roots(h, dl.ptr + 4, 2, 1, dp.data_ptr()) == ILLEGAL
    ctx.synchronize()
    assert outs.untouched()


@pytest.mark.parametrize("shift", [0, 4, 1])
def test_ahtree_log_records_outputs(m, ctx, L, orc, shift):
    for m_, plen in ((1, 32), (255, 32), (256, 32), (257, 32), (1000, 32), (257, 40), (65, 7)):
        pay = orc.fill_random(m_ * plen, m_ + plen).reshape(m_, plen)
        epl, ecl = _expected_logs(orc, pay, (1 << 32) + 5)
        dp = _dev(pay)
        for which in ("both", "plog", "clog"):
            outs = Outs()
            pl = outs.new(m_ * (4 + plen), offset=shift)
            cl = outs.new(m_ * 12, offset=shift)
            _sync()
            ok(L.mh_dev_ahtree_log_records(ctx.handle, dp.data_ptr(), m_, plen, (1 << 32) + 5,
                                           pl.ptr if which != "clog" else None,
                                           cl.ptr if which != "plog" else None))
            ctx.synchronize()
            case = (shift, m_, plen, which)
            assert np.array_equal(pl.payload(), epl if which != "clog" else np.full(epl.size, FILL)), case
            assert np.array_equal(cl.payload(), ecl if which != "plog" else np.full(ecl.size, FILL)), case
            assert outs.intact(), case


@pytest.mark.parametrize("world,m_total", [(2, 1 << 12), (3, 3000)])
def test_sharded_append_outputs(m, ctx, L, orc, world, m_total):
    """append_local, put_shard_roots and append_spine of every rank into a dLog
    of exactly nodes_upto(m_total) * 32 bytes: the rank's own range is the
    oracle's, every other node is the oracle's or still 0xA5, roots_out is
    RootAt after each of the rank's appends."""
    from immustore_amd import sharding
    k = sharding.ahtree_shard_bits(world, m_total)
    S = 1 << k
    pay = orc.fill_random(32 * m_total, 17).reshape(m_total, 32)
    o = orc.AHtree(m_total)
    o.append_batch(pay)
    nd = orc.nodes_upto(m_total)
    full = o.dlog[:nd]
    spans = [(min(r * S, m_total), min(S, max(m_total - r * S, 0))) for r in range(world)]
    assert sum(mm for _, mm in spans) == m_total
    dps = [_dev(pay[n0:n0 + mm]) for n0, mm in spans]
    dls = [Guarded(nd * 32) for _ in spans]
    ros = [Guarded(max(mm, 1) * 32) for _, mm in spans]
    _sync()
    for r, (n0, mm) in enumerate(spans):
        if mm:
            ok(L.mh_dev_ahtree_append_local(ctx.handle, dls[r].ptr, n0, dps[r].data_ptr(), mm, 32, k))
    ctx.synchronize()
    sroots = np.zeros((world, 32), np.uint8)
    for r, (n0, mm) in enumerate(spans):
        assert dls[r].guards_intact(), ("append_local", r)
        if mm == S:
            sroots[r] = dls[r].rows()[L.mh_ahtree_node_index(n0 + S, k)]
    groots = _dev(sroots)
    complete = min(m_total // S, world)
    _sync()
    for r, (n0, mm) in enumerate(spans):
        if not mm:
            continue
        ok(L.mh_dev_ahtree_put_shard_roots(ctx.handle, dls[r].ptr, k, complete, groots.data_ptr()))
        ctx.synchronize()
        assert dls[r].guards_intact(), ("put_shard_roots", r)
        ok(L.mh_dev_ahtree_append_spine(ctx.handle, dls[r].ptr, n0, mm, ros[r].ptr))
        ctx.synchronize()
        got = dls[r].rows()
        lo, hi = L.mh_ahtree_node_index(n0 + 1, 0), orc.nodes_upto(n0 + mm)
        assert np.array_equal(got[lo:hi], full[lo:hi]), r
        same = (got == full).all(axis=1)
        kept = (got == FILL).all(axis=1)
        assert (same | kept).all(), (r, np.nonzero(~(same | kept))[0][:5])
        want = np.stack([np.frombuffer(o.root_at(x)[1], np.uint8) for x in range(n0 + 1, n0 + mm + 1)])
        assert np.array_equal(ros[r].rows(), want), r
        assert dls[r].guards_intact() and ros[r].guards_intact(), r


def test_ahtree_peaks_output(m, ctx, L, orc, aht300):
    """peaks_out is popcount(n) * 32 bytes of host memory."""
    _, o, _ = aht300
    ddlog = _dev(o.dlog[:orc.nodes_upto(AHT_SIZE)])
    _sync()
    for n in (1, 255, 256, 300):
        bits = [l for l in range(64) if (n >> l) & 1]
        want = np.stack([o.dlog[L.mh_ahtree_node_index(n & ~((1 << l) - 1), l)] for l in bits])
        for pinned in (True, False):
            if pinned:
                g = Guarded(len(bits) * 32, pinned=True)
                ok(L.mh_dev_ahtree_peaks(ctx.handle, ddlog.data_ptr(), n, g.ptr))
                assert np.array_equal(g.rows(), want) and g.guards_intact(), n
                g.free()
            else:
                h = np.full(GUARD + len(bits) * 32 + GUARD, FILL, np.uint8)
                ok(L.mh_dev_ahtree_peaks(ctx.handle, ddlog.data_ptr(), n, h.ctypes.data + GUARD))
                assert np.array_equal(h[GUARD:-GUARD].reshape(-1, 32), want), n
                assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), n


# ------------------------------------------------------------------ mh_dev_tx_alh_batch
def _alh_headers(orc, fixtures):
    """The Go-written headers of the fixture stores (their stored Alh values
    are the expectation), then one v1 header per metadata length 0..268 and a
    few v0 headers -> (recs, blob, inner (n, 32), alh (n, 32), n_go)."""
    from tx_util import TX_HEADER, headers_from_fixture
    parts, blob, go_alh = [], bytearray(), []
    for name in sorted(fixtures):
        recs, b, alhs = headers_from_fixture(fixtures[name]["txs"])
        recs = recs.copy()
        recs["md_off"] += len(blob)
        blob += b
        parts.append(recs)
        go_alh += alhs
    n_go = len(go_alh)
    rng = np.random.default_rng(268)
    rnd = np.zeros(269 + 6, TX_HEADER)
    for k in range(len(rnd)):
        r = rnd[k]
        r["id"] = int(rng.integers(1, 1 << 62))
        r["ts"] = int(rng.integers(-2 ** 40, 2 ** 40))
        r["bl_tx_id"] = int(rng.integers(0, 1 << 62))
        for f in ("bl_root", "prev_alh", "eh"):
            r[f] = rng.integers(0, 256, 32, dtype=np.uint8)
        r["nentries"] = int(rng.integers(0, 1 << 16))
        if k < 269:
            r["version"] = 1
            md = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
            r["md_len"], r["md_off"] = k, len(blob)
            blob += md
    recs = np.concatenate(parts + [rnd])
    blob = bytes(blob)
    inner, alh = [], []
    for k in range(len(recs)):
        st, i_, a_ = orc.tx_header_alh(recs[k], blob)
        assert st == 0, (k, st)
        inner.append(np.frombuffer(i_, np.uint8))
        alh.append(np.frombuffer(a_, np.uint8))
    alh = np.stack(alh)
    assert alh[:n_go].tobytes() == b"".join(go_alh)
    return recs, blob, np.stack(inner), alh, n_go


def test_tx_alh_batch_parity_and_outputs(m, ctx, L, orc, fixtures):
    """mh_dev_tx_alh_batch against the 36 Alh values Go wrote and the oracle's
    for every metadata length 0..268: scratch exactly n * 384 bytes, inner_out
    and alh_out n * 32, at the 256-lane edges; eh passed separately from an
    address 4 bytes off a 16-byte boundary (eh: any alignment); inner_out NULL."""
    recs, blob, inner, alh, n_go = _alh_headers(orc, fixtures)
    assert n_go == 36 and set(recs["md_len"][n_go:n_go + 269]) == set(range(269))
    d_blob = _dev(np.frombuffer(blob, np.uint8))
    N_ALL = len(recs)
    for n, first in ((N_ALL, 0), (n_go, 0), (1, 0), (255, 40), (256, 40), (257, 40)):
        sel = recs[first:first + n]
        d_h = _dev(sel.view(np.uint8))
        # the same headers with eh zeroed: Eh comes from the eh argument
        blank = sel.copy()
        blank["eh"] = 0
        d_blank = _dev(blank.view(np.uint8))
        g_eh = Guarded(n * 32, offset=4)
        g_eh.put(sel["eh"])
        for mode in ("hdr", "eh", "no-inner"):
            o = Outs()
            scr, io, ao = o.new(n * 384), o.new(n * 32), o.new(n * 32)
            _sync()
            ok(L.mh_dev_tx_alh_batch(ctx.handle, n, (d_blank if mode == "eh" else d_h).data_ptr(),
                                     d_blob.data_ptr(), g_eh.ptr if mode == "eh" else None, scr.ptr,
                                     None if mode == "no-inner" else io.ptr, ao.ptr))
            ctx.synchronize()
            case = (n, first, mode)
            assert np.array_equal(ao.rows(), alh[first:first + n]), case
            assert np.array_equal(io.rows(), _fill_rows(n) if mode == "no-inner"
                                  else inner[first:first + n]), case
            assert o.intact() and g_eh.guards_intact(), case


def test_tx_alh_batch_refuses_misaligned_outputs(m, ctx, L, orc, fixtures):
    recs, blob, _, _, _ = _alh_headers(orc, fixtures)
    n = 3
    d_h, d_blob = _dev(recs[:n].view(np.uint8)), _dev(np.frombuffer(blob, np.uint8))
    o = Outs()
    scr, io, ao = o.new(n * 384), o.new(n * 32 + 16), o.new(n * 32 + 16)
    _sync()
    for di, da in ((4, 0), (0, 4)):
        assert L.mh_dev_tx_alh_batch(ctx.handle, n, d_h.data_ptr(), d_blob.data_ptr(), None, scr.ptr,
                                     io.ptr + di, ao.ptr + da) == ILLEGAL
    ctx.synchronize()
    assert o.untouched()


# ------------------------------------------------------------------ protobuf proofs
PB_N = (1, 63, 64, 65, 257)


def _pb_check(n, want, off, status, out, cap, what):
    """want[p] = (status, bytes).  off is complete whatever the capacity; a
    message ending past cap is MH_ERR_BUFFER_TOO_SMALL; every byte of out that
    no written message owns is still 0xA5."""
    from immustore_amd import _native as N
    eoff = np.zeros(n + 1, np.uint64)
    eoff[1:] = np.cumsum([len(b) for _, b in want])
    assert np.array_equal(off.view(np.uint64), eoff), what
    est = [N.MH_ERR_BUFFER_TOO_SMALL if s == 0 and int(eoff[p + 1]) > cap else s
           for p, (s, _) in enumerate(want)]
    assert status.view(np.int32).tolist() == est, what
    if out is None:
        return
    exp = np.full(out.n, FILL, np.uint8)
    for p, (_, b) in enumerate(want):
        if est[p] == 0:
            exp[int(eoff[p]):int(eoff[p + 1])] = np.frombuffer(b, np.uint8)
    assert np.array_equal(out.payload(), exp), what


def _pb_phases(ctx, L, n, want, call, what):
    """Phase 1, then phase 2 into an exact out; phase 3 into an exact out, one
    a byte short and one of capacity 0.  call(phase, out_ptr, cap, off, status,
    scratch) makes the C call."""
    total = sum(len(b) for _, b in want)
    o = Outs()
    off, status, scr = o.new((n + 1) * 8), o.new(n * 4), o.new(L.mh_pb_scratch_size(n))
    _sync()
    ok(call(1, None, 0, off, status, scr))
    ctx.synchronize()
    _pb_check(n, want, off, status, None, 1 << 62, what + ("phase 1",))
    out = o.new(total)
    _sync()
    ok(call(2, out.ptr, total, off, status, scr))
    ctx.synchronize()
    _pb_check(n, want, off, status, out, total, what + ("phase 2",))
    assert o.intact(), what + ("phases 1, 2",)
    for cap in (total, total - 1, 0):
        if cap < 0:
            continue
        o = Outs()
        off, status, scr = o.new((n + 1) * 8), o.new(n * 4), o.new(L.mh_pb_scratch_size(n))
        out = o.new(cap)
        _sync()
        ok(call(3, out.ptr, cap, off, status, scr))
        ctx.synchronize()
        _pb_check(n, want, off, status, out, cap, what + ("phase 3", cap))
        assert o.intact(), what + ("phase 3", cap)


@pytest.mark.parametrize("n", PB_N)
def test_htree_inclusion_proof_pb_outputs(m, ctx, L, orc, htree37, n):
    import wire
    _, lv, _, _ = htree37
    rng = np.random.default_rng(n)
    leaf = rng.integers(0, HT_W + 2, n).astype(np.uint64)
    leaf[0] = 0
    leaf[-1] = HT_W - 1          # the last message is a written one
    want = [wire.htree_inclusion_proof_pb(lv, HT_W, int(i)) for i in leaf]
    assert want[-1][0] == 0 and (n < 60 or any(s for s, _ in want))
    dlv, dleaf = _dev(lv), _dev(leaf)

    def call(phase, out, cap, off, status, scr):
        return L.mh_dev_htree_inclusion_proof_pb_batch(ctx.handle, phase, dlv.data_ptr(), HT_W, n,
                                                       dleaf.data_ptr(), out, cap, off.ptr, status.ptr,
                                                       scr.ptr)
    _pb_phases(ctx, L, n, want, call, ("incl", n))


def _dual_headers(rng, n_tx):
    """Linked headers of txs 1..n_tx (BlTxID = id - 1), v0 and v1, with
    canonical tx metadata of every kind."""
    from tx_util import TX_HEADER
    recs = np.zeros(n_tx, TX_HEADER)
    blob = bytearray()
    for k in range(n_tx):
        r = recs[k]
        r["id"], r["bl_tx_id"] = k + 1, k
        r["ts"] = int(rng.integers(-2 ** 40, 2 ** 40)) if k % 7 else 0
        for f in ("bl_root", "prev_alh", "eh"):
            r[f] = rng.integers(0, 256, 32, dtype=np.uint8)
        r["version"] = 1 if k % 5 else 0
        r["nentries"] = [0, 1, 127, 128, 300, 2 ** 31 + 5, 2 ** 32 - 1][k % 7]
        md = b""
        if r["version"] == 1 and k % 3:
            if k % 4 == 0:
                md = bytes([0]) + int(rng.integers(0, 2 ** 63)).to_bytes(8, "big")
            elif k % 4 == 1:
                ln = int(rng.integers(0, 257))
                md = bytes([1]) + ln.to_bytes(2, "big") + rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            else:
                md = bytes([0]) + (200).to_bytes(8, "big") + bytes([1, 0, 3]) + b"abc"
        r["md_len"], r["md_off"] = len(md), len(blob)
        blob += md
    return recs, bytes(blob)


def _rec_hdr(r, blob):
    return {"id": int(r["id"]), "ts": int(r["ts"]), "bltxid": int(r["bl_tx_id"]),
            "blroot": r["bl_root"].tobytes(), "prevalh": r["prev_alh"].tobytes(),
            "eh": r["eh"].tobytes(), "version": int(r["version"]), "nentries": int(r["nentries"]),
            "md": blob[int(r["md_off"]):int(r["md_off"]) + int(r["md_len"])]}


@pytest.mark.parametrize("n", PB_N)
def test_dual_proof_v2_pb_parity_and_outputs(m, ctx, L, orc, aht300, n):
    """mh_dev_dual_proof_v2_pb_batch against the oracle's DualProofV2 messages
    over a tree of 300 appends: every phase, every capacity, with the Go error
    cases (newer source, source id 0, a target beyond the tree, broken linking)
    mixed in."""
    import wire
    _, o, _ = aht300
    view = orc.AHtree.__new__(orc.AHtree)
    view.size, view.dlog = AHT_SIZE, o.dlog
    rng = np.random.default_rng(40 + n)
    recs, blob = _dual_headers(rng, AHT_SIZE + 8)
    tgt = rng.integers(1, AHT_SIZE + 2, n)
    src = np.array([int(rng.integers(1, x + 1)) for x in tgt])
    tgt[-1], src[-1] = AHT_SIZE + 1, 1        # the longest proofs, written last
    if n > 8:
        src[2] = tgt[2]                       # same tx: headers only
        src[3] = tgt[3] + 1                   # newer source
        tgt[5] = AHT_SIZE + 5                 # beyond the tree
    s = recs[src - 1].copy()
    g = recs[tgt - 1].copy()
    if n > 8:
        s[4]["id"] = 0
        g[6]["bl_tx_id"] = 0 if g[6]["id"] != 1 else 5   # linking error
    want = [wire.dual_proof_v2_pb(_rec_hdr(s[k], blob), _rec_hdr(g[k], blob), view) for k in range(n)]
    assert want[-1][0] == 0 and (n < 9 or len({st for st, _ in want}) >= 4)
    ddlog = _dev(o.dlog[:orc.nodes_upto(AHT_SIZE)])
    ds, dg, db = _dev(s.view(np.uint8)), _dev(g.view(np.uint8)), _dev(np.frombuffer(blob, np.uint8))

    def call(phase, out, cap, off, status, scr):
        return L.mh_dev_dual_proof_v2_pb_batch(ctx.handle, phase, ddlog.data_ptr(), AHT_SIZE, n,
                                               ds.data_ptr(), dg.data_ptr(), db.data_ptr(), out, cap,
                                               off.ptr, status.ptr, scr.ptr)
    _pb_phases(ctx, L, n, want, call, ("dual v2", n))


# ------------------------------------------------------------------ whole answers
def test_verifiable_answers_device_out(m, ctx, L):
    """mh_verifiable_answer_pb_batch writing into device memory of exactly
    off[n] bytes, and of one byte less (the last answer is then refused and
    its bytes stay 0xA5)."""
    import answer_util as A
    from immustore_amd import _native as N
    from immustore_amd.answers import _Batch, _csr
    from test_gpu_answers import release, resident
    s = A.synthetic()
    d = resident(ctx, s)
    try:
        reqs = A.synthetic_requests(s)[:130]
        exp = [s.expect(*r) for r in reqs]
        assert all(e[0] == 0 for e in exp)
        n = len(reqs)
        kind, tx, since, keys, entries = A.columns(reqs)
        kd, txa, ps = (np.ascontiguousarray(kind, np.uint8), np.ascontiguousarray(tx, np.uint64),
                       np.ascontiguousarray(since, np.uint64))
        kb, ko = _csr(keys, n)
        eb, eo = _csr(entries, n)
        b = _Batch()
        b.n, b.kind, b.tx, b.prove_since = n, kd.ctypes.data, txa.ctypes.data, ps.ctypes.data
        b.keys, b.key_off, b.entries, b.entry_off = (kb.ctypes.data, ko.ctypes.data, eb.ctypes.data,
                                                     eo.ctypes.data)
        sd = d.descriptor()
        eoff = np.zeros(n + 1, np.uint64)
        eoff[1:] = np.cumsum([len(x) for _, x in exp])
        total = int(eoff[n])
        for cap in (total, total - 1):
            out = Guarded(cap)
            off, st = np.zeros(n + 1, np.uint64), np.zeros(n, np.int32)
            _sync()
            ok(L.mh_verifiable_answer_pb_batch(d.tree.handle, C.addressof(sd), C.addressof(b), out.ptr,
                                               cap, off.ctypes.data, st.ctypes.data))
            ctx.synchronize()
            assert np.array_equal(off, eoff), cap
            est = [N.MH_ERR_BUFFER_TOO_SMALL if int(eoff[p + 1]) > cap else 0 for p in range(n)]
            assert st.tolist() == est and sum(1 for x in est if x) == (cap < total), cap
            want = np.full(cap, FILL, np.uint8)
            for p in range(n):
                if est[p] == 0:
                    want[int(eoff[p]):int(eoff[p + 1])] = np.frombuffer(exp[p][1], np.uint8)
            assert np.array_equal(out.payload(), want), cap
            assert out.guards_intact(), cap
    finally:
        release(d)


# ------------------------------------------------------------------ the tx-log read path
TXLOG_LANES = (1, 2, 4, 8, 16)


def _exact_txlog(orc, ntx, width, seed):
    """ntx sealed records (immustore.go:1812-1924) of at most `width` entries,
    the first of exactly `width`: the lane count of k_txlog_lanes follows the
    widest record.  -> (log bytes, record spans, entries per record)"""
    from tx_util import md_record
    rng = np.random.default_rng(seed)
    out, spans, nes, prev = bytearray(), [], [], orc.sha256(b"")
    for k in range(ntx):
        ne = width if k % 3 == 0 else int(rng.integers(0, width + 1))
        nes.append(ne)
        ents = [(b"", b"", rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes(),
                 rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(ne)]
        rec, prev = md_record(orc, k + 1, prev, 1 if k % 2 else 0, b"", b"", ents)
        spans.append((len(out), len(out) + len(rec)))
        out += rec
    return bytes(out), spans, nes


@pytest.fixture(scope="module")
def lane_logs(orc):
    """lanes -> (log of 4R + 1 records, spans, the oracle's (alh, status) with
    a few records damaged)"""
    out = {}
    for lanes in TXLOG_LANES:
        R = 64 // lanes
        raw, spans, nes = _exact_txlog(orc, 4 * R + 1, lanes, lanes)
        b = bytearray(raw)
        for k in range(2, len(spans), 7):
            if nes[k]:
                b[spans[k][1] - 33] ^= 1      # the last entry's hVal: an Alh mismatch
        out[lanes] = (bytes(b), spans)
    return out


def _txlog_outs(o, cap, pinned):
    from immustore_amd.txlayer import TX_HEADER
    return (o.new(cap * TX_HEADER.itemsize, pinned=pinned), o.new(cap * 32, pinned=pinned),
            o.new(cap * 4, pinned=pinned))


def _check_txlog_outs(outs, ntx, cap, want, what):
    """Rows [0, ntx) against want = (hdrs, alh, status); rows [ntx, cap) keep
    the caller's bytes."""
    from immustore_amd.txlayer import TX_HEADER
    hd, alh, st = outs
    whd, walh, wst = want
    assert np.array_equal(st.view(np.int32)[:ntx], wst), what
    assert np.array_equal(alh.rows()[:ntx], walh), what
    assert np.array_equal(hd.view(TX_HEADER)[:ntx], whd), what
    for g, w in ((hd, TX_HEADER.itemsize), (alh, 32), (st, 4)):
        assert (g.payload()[ntx * w:] == FILL).all(), what + ("rows past ntx",)
        assert g.guards_intact(), what


@pytest.mark.parametrize("kern", ["wave", "lanes"])
@pytest.mark.parametrize("lanes", TXLOG_LANES)
def test_txlog_validate_pinned_outputs(m, ctx, L, orc, lane_logs, monkeypatch, lanes, kern):
    """mh_txlog_validate, _resident and _clog storing into pinned hdrs / alh /
    status of capacity ntx and ntx + 3 (the rows past ntx keep the caller's
    bytes), _clog into device outputs as well; ntx on both sides of the 4R
    records of a workgroup."""
    import torch
    from tx_util import clog_for
    monkeypatch.setenv("MH_TXLOG_KERNEL", kern)
    raw_all, spans = lane_logs[lanes]
    R = 64 // lanes
    for ntx in sorted({1, 4 * R - 1, 4 * R, 4 * R + 1}):
        raw = raw_all[:spans[ntx - 1][1]]
        ost = orc.txlog_validate(raw)
        assert (ost[0], ost[1], ost[2]) == (0, ntx, len(raw))
        ref = m.txlog_validate(raw, ctx=ctx)          # pageable outputs: the headers' reference
        assert np.array_equal(ref[4], ost[3]) and list(ref[5]) == list(ost[4])
        want = (ref[3], ost[3], ost[4])
        hb = np.frombuffer(raw, np.uint8)
        dlog = torch.zeros(len(raw) + 256, dtype=torch.uint8, device="cuda")
        dlog[:len(raw)] = torch.from_numpy(hb.copy()).cuda()
        clog = np.frombuffer(clog_for(raw, spans[:ntx]), np.uint8)
        for cap in (ntx, ntx + 3):
            n_, used = C.c_uint64(0), C.c_uint64(0)
            for resident in (False, True):
                o = Outs()
                outs = _txlog_outs(o, cap, True)
                _sync()
                if resident:
                    rc = L.mh_txlog_validate_resident(ctx.handle, hb.ctypes.data, dlog.data_ptr(), len(raw),
                                                      1024, 1024, cap, C.byref(n_), C.byref(used),
                                                      outs[0].ptr, outs[1].ptr, outs[2].ptr)
                else:
                    rc = L.mh_txlog_validate(ctx.handle, hb.ctypes.data, len(raw), 1024, 1024, cap,
                                             C.byref(n_), C.byref(used), outs[0].ptr, outs[1].ptr,
                                             outs[2].ptr)
                ctx.synchronize()
                what = (kern, lanes, ntx, cap, "resident" if resident else "host")
                assert (rc, n_.value, used.value) == (0, ntx, len(raw)), what
                _check_txlog_outs(outs, ntx, cap, want, what)
                for g in o.all:
                    g.free()
            for pinned in (True, False):
                o = Outs()
                outs = _txlog_outs(o, cap, pinned)
                nbad, first = C.c_uint64(0), C.c_uint64(0)
                _sync()
                rc = L.mh_txlog_validate_clog(ctx.handle, dlog.data_ptr(), len(raw), clog.ctypes.data, ntx,
                                              12, 1024, 1024, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                              C.byref(nbad), C.byref(first))
                ctx.synchronize()
                what = (kern, lanes, ntx, cap, "clog", "pinned" if pinned else "device")
                assert rc == 0 and nbad.value == int((ost[4] != 0).sum()), what
                _check_txlog_outs(outs, ntx, cap, want, what)
                for g in o.all:
                    g.free()


def test_txlog_validate_pinned_last_chunk_outputs(m, ctx, L, orc):
    """A pinned log of 16 MiB or more goes up in chunks and the last chunk's
    kernel stores Eh alone into the pinned headers (the host fills the other
    fields): hdrs / alh / status of exactly ntx rows, guarded."""
    import torch
    from tx_util import _bulk_txlog
    raw, starts = _bulk_txlog(np.random.default_rng(8), 9000)
    assert len(raw) >= (16 << 20)
    ntx = len(starts)
    pin = torch.empty(len(raw), dtype=torch.uint8).pin_memory()
    pin.numpy()[:] = np.frombuffer(raw, np.uint8)
    ost = orc.txlog_validate(raw)
    assert (ost[0], ost[1]) == (0, ntx)
    ref = m.txlog_validate(raw, ctx=ctx)
    o = Outs()
    outs = _txlog_outs(o, ntx, True)
    n_, used = C.c_uint64(0), C.c_uint64(0)
    rc = L.mh_txlog_validate(ctx.handle, pin.numpy().ctypes.data, len(raw), 1024, 1024, ntx,
                             C.byref(n_), C.byref(used), outs[0].ptr, outs[1].ptr, outs[2].ptr)
    ctx.synchronize()
    assert (rc, n_.value, used.value) == (0, ntx, len(raw))
    _check_txlog_outs(outs, ntx, ntx, (ref[3], ost[3], ost[4]), ("last chunk",))
    for g in o.all:
        g.free()


# ------------------------------------------------------------------ several contexts
@pytest.mark.parametrize("npd", [1, 256])
def test_multi_dev_build_entries_fixed_outputs(m, L, orc, npd):
    """Two contexts on device 0: each device's hvals_out, levels, top_levels
    (mh_htree_levels_len(2) nodes) and root, all exact-size."""
    from immustore_amd.multi import MultiDevice
    K = 2
    n = K * npd
    keys = orc.fill_random(n * 8, 91 + npd).reshape(n, 8)
    vals = orc.fill_random(n * 128, 92 + npd).reshape(n, 128)
    ohv, _, oroot = orc.build_entries_fixed(1, keys, vals)
    subs = [orc.build_entries_fixed(1, keys[d * npd:(d + 1) * npd], vals[d * npd:(d + 1) * npd])
            for d in range(K)]
    top = np.stack([np.frombuffer(subs[0][2], np.uint8), np.frombuffer(subs[1][2], np.uint8),
                    np.frombuffer(oroot, np.uint8)])
    md = MultiDevice([0] * K)
    try:
        dk = [_dev(keys[d * npd:(d + 1) * npd]) for d in range(K)]
        dv = [_dev(vals[d * npd:(d + 1) * npd]) for d in range(K)]
        o = Outs()
        hv = [o.new(npd * 32) for _ in range(K)]
        lv = [o.new(L.mh_htree_levels_len(npd) * 32) for _ in range(K)]
        tl = [o.new(L.mh_htree_levels_len(K) * 32) for _ in range(K)]
        rt = [o.new(32) for _ in range(K)]
        _sync()
        md.dev_build_entries_fixed(1, npd, [t.data_ptr() for t in dk], 8, [t.data_ptr() for t in dv],
                                   128, [g.ptr for g in lv], [g.ptr for g in tl], [g.ptr for g in rt],
                                   hvals=[g.ptr for g in hv])
        md.synchronize()
        for d in range(K):
            assert np.array_equal(hv[d].rows(), ohv[d * npd:(d + 1) * npd]), d
            assert np.array_equal(lv[d].rows(), subs[d][1]), d
            assert np.array_equal(tl[d].rows(), top), d
            assert np.array_equal(rt[d].rows(), _root_rows(oroot)), d
        assert o.intact()
    finally:
        md.close()


def test_multi_dev_ahtree_append_outputs(m, L, orc, aht300):
    """Two ranges on device 0 onto an empty tree: each range's dlog and
    roots_out exact-size."""
    from immustore_amd.multi import MultiDevice, ahtree_range_plan
    pay, o, roots = aht300
    K, total = 2, 300
    _, b = ahtree_range_plan(0, total, K)
    G = len(b) - 1
    assert G == 2
    cut = [orc.nodes_upto(x) for x in b]
    md = MultiDevice([0] * K)
    try:
        dp = [_dev(pay[b[d]:b[d + 1]]) for d in range(G)]
        outs = Outs()
        dl = [outs.new((cut[d + 1] - cut[d]) * 32) for d in range(G)]
        ro = [outs.new((b[d + 1] - b[d]) * 32) for d in range(G)]
        _sync()
        md.dev_ahtree_append_batch(total, [t.data_ptr() for t in dp], 32, [g.ptr for g in dl],
                                   [g.ptr for g in ro])
        md.synchronize()
        for d in range(G):
            assert np.array_equal(dl[d].rows(), o.dlog[cut[d]:cut[d + 1]]), d
            assert np.array_equal(ro[d].rows(), roots[b[d]:b[d + 1]]), d
        assert outs.intact()
    finally:
        md.close()
