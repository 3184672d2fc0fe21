"""The fast instantiation of k_entries_fixed as straight-line code around
called SHA block routines (value loop, padding block, sha_block() for the
entry digest, the leaf, the in-lane nodes and the workgroup-level nodes)
against the oracle, and against the general kernel of the same build
(MH_FIXED_FAST=0), byte for byte: every level, the root and hvals_out, with
hvals_out present and with None.

The entry counts give lanes with fewer than LPL entries, one busy lane in a
wave, idle waves in a workgroup and promoted odd nodes at the in-lane levels
(MH_LPL 2 / 4) and at the workgroup levels (MH_WG_LEVELS 1 / 8).  Value
buffers are exactly n x val_len bytes.

The tail-row case feeds every possible last byte of a right child to the
node hashes the kernel computes itself (MH_LPL=2, MH_WG_LEVELS=1: the
in-lane nodes of level 1 and the workgroup nodes of level 2): a node's second
block depends on that byte alone.
"""
import os

import numpy as np
import pytest

from gpu_util import DevBuf

pytestmark = pytest.mark.gpu

VAL_LENS = (128, 1024, 4096)
KEYS = ((1, 4), (1, 8), (1, 16), (0, 20))      # (version, key_len)
COUNTS = (1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025, 2049)


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
def cases(orc):
    """(version, key_len, val_len, n) -> keys, vals and the oracle's (hvals,
    levels, root) as bytes; each made once, on first use, for all knob arms."""
    memo = {}

    def get(version, klen, vlen, n):
        k = (version, klen, vlen, n)
        if k not in memo:
            vals = orc.fill_random(n * vlen, 7000 + vlen + n).reshape(n, vlen)
            keys = orc.fill_random(n * klen, 8000 + klen + n).reshape(n, klen)
            ohv, olv, oroot = orc.build_entries_fixed(version, keys, vals)
            memo[k] = (keys, vals, (ohv.tobytes(), olv.tobytes(), oroot))
        return memo[k]
    return get


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


def _build(m, ctx, version, n, klen, vlen, dk, dv, want_hvals):
    """One mh_dev_htree_build_entries_fixed call into freshly poisoned
    outputs -> (hvals or None, levels, root) as bytes."""
    from immustore_amd import _native as N
    nl = m.levels_len(n)
    dl = DevBuf.from_host(ctx, np.full(nl * 32, 0xA5, np.uint8))
    dr = DevBuf.from_host(ctx, np.full(32, 0xA5, np.uint8))
    dh = DevBuf.from_host(ctx, np.full(n * 32, 0xA5, np.uint8)) if want_hvals else None
    N.check(N.load().mh_dev_htree_build_entries_fixed(
        ctx.handle, version, n, dk.ptr, klen, dv.ptr, vlen, dh.ptr if dh else None, dl.ptr,
        dr.ptr))
    ctx.synchronize()
    out = (dh.to_host().tobytes() if dh else None, dl.to_host().tobytes(),
           dr.to_host().tobytes())
    for d in (dl, dr, dh):
        if d is not None:
            d.free()
    return out


def _check(m, ctx, version, klen, vlen, n, keys, vals, want, lpl, wgl):
    """Fast and general kernel under one knob setting, with and without
    hvals_out, against `want` = the oracle's (hvals, levels, root)."""
    assert vals.nbytes == n * vlen
    ohv, olv, oroot = want
    dk = DevBuf.from_host(ctx, keys)
    dv = DevBuf.from_host(ctx, vals)   # exactly n * val_len bytes
    for want_hvals in (True, False):
        got = {}
        for fast in (None, "0"):       # default dispatch (fast) / general kernel forced
            with _Env(MH_LPL=lpl, MH_WG_LEVELS=wgl, MH_FIXED_FAST=fast):
                got[fast] = _build(m, ctx, version, n, klen, vlen, dk, dv, want_hvals)
            hv, lv, root = got[fast]
            case = (lpl, wgl, version, klen, vlen, n, want_hvals, fast)
            assert root == oroot, case
            assert lv == olv, case
            if want_hvals:
                assert hv == ohv, case
        assert got[None] == got["0"], (lpl, wgl, version, klen, vlen, n, want_hvals)
    dk.free()
    dv.free()


@pytest.mark.parametrize("version,klen", KEYS)
@pytest.mark.parametrize("wgl", ["0", "1", "8"])
@pytest.mark.parametrize("lpl", ["1", "2", "4"])
def test_leaf_routines_vs_oracle_and_general(m, ctx, cases, lpl, wgl, version, klen):
    for vlen in VAL_LENS:
        for n in COUNTS:
            keys, vals, want = cases(version, klen, vlen, n)
            _check(m, ctx, version, klen, vlen, n, keys, vals, want, lpl, wgl)


def _tail_bytes(olv, n):
    """Last bytes of the right children of the level-1 and level-2 nodes of
    an n-leaf tree (n a power of two): the odd nodes of levels 0 and 1."""
    lv0 = olv[:n]
    lv1 = olv[n:n + n // 2]
    return np.concatenate([lv0[1::2, 31], lv1[1::2, 31]])


def test_leaf_routines_every_node_tail_byte(m, ctx, orc):
    n, vlen, klen, version = 4096, 128, 8, 1
    keys = orc.fill_random(n * klen, 8100).reshape(n, klen)
    # seed chosen on the CPU: the first whose tree shows all 256 tail bytes
    # (3072 samples: a value is missed with probability ~6e-6 per seed)
    for seed in range(9000, 9016):
        vals = orc.fill_random(n * vlen, seed).reshape(n, vlen)
        ohv, olv, oroot = orc.build_entries_fixed(version, keys, vals)
        tails = _tail_bytes(olv, n)
        if len(set(tails.tolist())) == 256:
            break
    assert tails.size == 3072
    assert len(set(tails.tolist())) == 256, "no seed with every node tail byte"
    _check(m, ctx, version, klen, vlen, n, keys, vals,
           (ohv.tobytes(), olv.tobytes(), oroot), "2", "1")
