"""The fast instantiation of k_entries_fixed (values of whole 128-byte units:
buffer-descriptor LDS-DMA with hoisted lane offsets, both blocks of a unit
read before its two compressions, every lane compressing, host-made padding
table) against the oracle, and against the general kernel of the same build
(MH_FIXED_FAST=0), byte for byte: every level, the root and hvals_out.

val_len 128 / 256 / 1024 take the fast kernel, 64 / 192 / 1040 sit just off
it (the dispatch boundary).  The entry counts give lanes with fewer than LPL
entries, one busy lane in a wave, a clamped last entry and whole idle waves
in a workgroup (n = 129 with MH_LPL=2: all four at once).  Value buffers are
exactly n x val_len bytes, so a lane that read past its clamp would leave
the allocation's used part.
"""
import os

import numpy as np
import pytest

from gpu_util import DevBuf

pytestmark = pytest.mark.gpu

VAL_LENS = (128, 256, 1024, 64, 192, 1040)
COUNTS = (1, 2, 3, 127, 128, 129, 255, 257, 511, 1000)


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
def inputs(orc):
    """(val_len, n, key_len) -> keys, vals; made once for all cases."""
    out = {}
    for vlen in VAL_LENS:
        for n in COUNTS:
            vals = orc.fill_random(n * vlen, 4000 + vlen + n).reshape(n, vlen)
            for klen in (8, 16):
                keys = orc.fill_random(n * klen, 5000 + klen + n).reshape(n, klen)
                out[(vlen, n, klen)] = (keys, vals)
    return out


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
    return (dh.to_host().tobytes() if dh else None, dl.to_host().tobytes(),
            dr.to_host().tobytes())


@pytest.mark.parametrize("version,klen", [(1, 8), (1, 16), (0, 8), (0, 16)])
@pytest.mark.parametrize("lpl", ["1", "2", "4"])
def test_entries_fixed_fast_vs_oracle_and_general(m, ctx, orc, inputs, lpl, version, klen):
    for vlen in VAL_LENS:
        for n in COUNTS:
            keys, vals = inputs[(vlen, n, klen)]
            assert vals.nbytes == n * vlen
            ohv, olv, oroot = orc.build_entries_fixed(version, keys, vals)
            ohv, olv = ohv.tobytes(), olv.tobytes()
            dk = DevBuf.from_host(ctx, keys)
            dv = DevBuf.from_host(ctx, vals)   # exactly n * val_len bytes
            for want_hvals in (True, False):
                got = {}
                for fast in (None, "0"):       # default dispatch / general kernel forced
                    with _Env(MH_LPL=lpl, MH_FIXED_FAST=fast):
                        got[fast] = _build(m, ctx, version, n, klen, vlen, dk, dv, want_hvals)
                    hv, lv, root = got[fast]
                    case = (lpl, version, klen, vlen, n, want_hvals, fast)
                    assert root == oroot, case
                    assert lv == olv, case
                    if want_hvals:
                        assert hv == ohv, case
                assert got[None] == got["0"], (lpl, version, klen, vlen, n, want_hvals)
            dk.free()
            dv.free()
