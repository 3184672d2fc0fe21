"""Ranged ahtree appends onto trees past 2^32 (mh_dev_ahtree_append_range,
mh_dev_ahtree_range_local / _finish, mh_multi_(dev_)ahtree_append_batch):
the replay of syncBinaryLinking resumes at aht.Size()+1 (immustore.go:
1198-1232), and these calls serve it holding only the old tree's peaks, so
n0 is any 64-bit size and every dLog index is 64-bit math behind a biased
base pointer.  The old peaks are fabricated digests; the reference is the
oracle's peaks-only stream (orc_ahtree_stream, ahtree.go:287-322), which does
no dLog index arithmetic.  Every dLog row and every roots_out row is compared
byte for byte; dlog_range and roots_out are filled with 0xA5 and stand between
4096 guard bytes that must still be 0xA5 afterwards."""
import numpy as np
import pytest

from ahtree_wide_util import WIDE_N0, WIDE_TOTALS, nodes_upto, sampled_rows, wide_case
from gpu_util import FILL, GUARD, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import torch  # noqa: F401
    import immustore_amd as m
    if m.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return m


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).cuda()


def _host_peaks(packed):
    """(keep-alive array, address) of the packed peaks, (None, None) for n0 = 0."""
    if not packed:
        return None, None
    a = np.frombuffer(packed, np.uint8)
    return a, a.ctypes.data


class _RangeCall:
    """The buffers of one mh_dev_ahtree_append_range call of case c; run()
    enqueues the call on ctx and returns its status."""

    def __init__(self, c):
        import torch
        self.c = c
        self.dp = _dev(c.pay)
        self.dl = Guarded(len(c.want_rows) * 32)
        self.ro = Guarded(c.total * 32)
        self.pk, self.pkp = _host_peaks(c.packed)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the call runs on ctx's

    def run(self, L, ctx):
        c = self.c
        return L.mh_dev_ahtree_append_range(ctx.handle, self.dl.ptr, c.n0, self.pkp,
                                            self.dp.data_ptr(), c.total, c.plen, self.ro.ptr)

    def check(self, what):
        _check_all(self.c, self.dl, self.ro, what)


def _check_all(c, dl, ro, what):
    """Every dLog row, every root and the guards of a call that ran all of case c."""
    assert np.array_equal(dl.rows(), c.want_rows), what
    assert np.array_equal(ro.rows(), c.want_roots), what
    assert dl.guards_intact() and ro.guards_intact(), what


@pytest.mark.parametrize("n0", WIDE_N0)
def test_append_range_wide(m, orc, n0):
    """mh_dev_ahtree_append_range at every total of WIDE_TOTALS (plen 32).
    Each call is followed on the same context, with no wait between them, by
    one onto another n0 of the table: the context's frontier buffer is reused,
    and neither call may see the other's peaks."""
    from immustore_amd import _native as N
    L = N.load()
    other = WIDE_N0[(WIDE_N0.index(n0) + 4) % len(WIDE_N0)]
    ctx = m.Context(0)
    try:
        for total in WIDE_TOTALS:
            a = wide_case(orc, n0, total)
            b = wide_case(orc, other, total, seed=9)
            ca, cb = _RangeCall(a), _RangeCall(b)
            sa, sb = ca.run(L, ctx), cb.run(L, ctx)
            ctx.synchronize()
            assert sa == 0 and sb == 0
            ca.check((n0, total))
            cb.check((n0, total, "then", other))
    finally:
        ctx.close()


def test_append_range_wide_payload_widths(m, orc):
    """Payloads that are not one SHA block (the leaf kernel's byte path) at
    n0 = 2^40 + 12345, and the argument edges: n0 + total past 2^64 and a
    non-empty tree without peaks are refused with nothing written."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    ctx = m.Context(0)
    try:
        for plen in (8, 40, 1024):
            c = wide_case(orc, 2 ** 40 + 12345, 300, plen=plen)
            call = _RangeCall(c)
            st = call.run(L, ctx)
            ctx.synchronize()
            assert st == 0
            call.check(plen)
        slots = orc.fill_random(64 * 32, 8).reshape(64, 32)
        pay = _dev(orc.fill_random(20 * 32, 7))
        for n0, peaks in ((2 ** 64 - 10, True), (2 ** 32, False)):
            pk = np.ascontiguousarray(slots[[l for l in range(64) if (n0 >> l) & 1]])
            dl, ro = Guarded(64 * 20 * 32), Guarded(20 * 32)
            torch.cuda.synchronize()
            st = L.mh_dev_ahtree_append_range(ctx.handle, dl.ptr, n0,
                                              pk.ctypes.data if peaks else None, pay.data_ptr(),
                                              20, 32, ro.ptr)
            ctx.synchronize()
            assert st == N.MH_ERR_ILLEGAL_ARGUMENTS, n0
            assert dl.untouched() and ro.untouched(), n0
    finally:
        ctx.close()


def _rank_append(m, orc, world, n0, total, ctxs):
    """The `world` ranks of one ranged append played one after the other, rank
    r on ctxs[r % len(ctxs)] with its own buffers, the all-gather by hand in
    rank order; every rank's range compared with its slice of the stream."""
    import torch
    from immustore_amd import _native as N
    from immustore_amd import sharding
    from immustore_amd.multi import ahtree_range_plan
    L = N.load()
    c = wide_case(orc, n0, total)
    _, b = ahtree_range_plan(n0, total, world)
    G = len(b) - 1
    assert b[0] == n0 and b[G] == n0 + total
    send_b, work_b = sharding.ahtree_range_sizes(n0, total, world)
    u0 = nodes_upto(n0)
    cut = [nodes_upto(x) - u0 for x in b]  # range r holds dLog rows [cut[r], cut[r+1])
    pk, pkp = _host_peaks(c.packed)
    ctx = lambda r: ctxs[r % len(ctxs)]  # noqa: E731
    dp = [_dev(c.pay[b[r] - n0:b[r + 1] - n0]) if r < G
          else torch.empty(32, dtype=torch.uint8, device="cuda") for r in range(world)]
    dl = [Guarded((cut[r + 1] - cut[r]) * 32 if r < G else 32) for r in range(world)]
    ro = [Guarded((b[r + 1] - b[r]) * 32 if r < G else 32) for r in range(world)]
    work = [torch.empty(work_b, dtype=torch.uint8, device="cuda") for _ in range(world)]
    send = [torch.zeros(send_b, dtype=torch.uint8, device="cuda") for _ in range(world)]
    recv = [torch.empty(world * send_b, dtype=torch.uint8, device="cuda") for _ in range(world)]
    torch.cuda.synchronize()
    for r in range(world):
        N.check(L.mh_dev_ahtree_range_local(ctx(r).handle, n0, pkp, total, world, r,
                                            dp[r].data_ptr(), 32, dl[r].ptr, work[r].data_ptr(),
                                            send[r].data_ptr()))
    for x in ctxs:
        x.synchronize()
    gathered = torch.cat(send)
    for r in range(world):
        recv[r].copy_(gathered)
    torch.cuda.synchronize()
    for r in range(world):
        N.check(L.mh_dev_ahtree_range_finish(ctx(r).handle, n0, pkp, total, world, r,
                                             recv[r].data_ptr(), dl[r].ptr, work[r].data_ptr(),
                                             ro[r].ptr))
    for x in ctxs:
        x.synchronize()
    for r in range(world):
        what = (world, n0, total, r, b)
        if r >= G:  # a rank past the plan's ranges does nothing
            assert dl[r].untouched() and ro[r].untouched(), what
            continue
        assert np.array_equal(dl[r].rows(), c.want_rows[cut[r]:cut[r + 1]]), what
        assert np.array_equal(ro[r].rows(), c.want_roots[b[r] - n0:b[r + 1] - n0]), what
        assert dl[r].guards_intact() and ro[r].guards_intact(), what
    del pk


@pytest.mark.parametrize("n0", [2 ** 32 - 100, 2 ** 40 + 12345, 2 ** 48 - 129])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_rank_range_append_wide(m, orc, world, n0):
    """mh_dev_ahtree_range_local / _finish, played as
    test_rank_ahtree_range_append_vs_oracle plays them: totals 5 (fewer
    appends than ranks), 300, 2100 (k = 5 over 8 ranks) and 20011."""
    ctxs = [m.Context(0) for _ in range(world)]
    try:
        for total in (5, 300, 2100, 20011):
            _rank_append(m, orc, world, n0, total, ctxs)
    finally:
        for x in ctxs:
            x.close()


def test_rank_range_append_wide_64_ranks(m, orc):
    """64 ranks over 5000 appends onto 2^48 - 129: k = 2 and 64 ranges, the
    range walk (pe0) of the piece-tree kernel at its limit; rank r runs on
    context r % 8."""
    ctxs = [m.Context(0) for _ in range(8)]
    try:
        _rank_append(m, orc, 64, 2 ** 48 - 129, 5000, ctxs)
    finally:
        for x in ctxs:
            x.close()


@pytest.mark.parametrize("K", [1, 3, 8])
def test_multi_append_wide(m, orc, K):
    """mh_multi_dev_ahtree_append_batch (every range's rows and roots) and the
    host form mh_multi_ahtree_append_batch (the whole new dLog and
    RootAt(n0 + total)) at n0 = 2^40 + 12345 over K ranges on one device."""
    import torch
    from immustore_amd import _native as N
    from immustore_amd.multi import MultiDevice, ahtree_range_plan
    L = N.load()
    n0 = 2 ** 40 + 12345
    u0 = nodes_upto(n0)
    md = MultiDevice([0] * K)
    try:
        for total in (300, 20011):
            c = wide_case(orc, n0, total)
            _, b = ahtree_range_plan(n0, total, K)
            G = len(b) - 1
            cut = [nodes_upto(x) - u0 for x in b]
            dp = [_dev(c.pay[b[d] - n0:b[d + 1] - n0]) if d < G else None for d in range(K)]
            dl = [Guarded((cut[d + 1] - cut[d]) * 32) if d < G else None for d in range(K)]
            ro = [Guarded((b[d + 1] - b[d]) * 32) if d < G else None for d in range(K)]
            torch.cuda.synchronize()
            md.dev_ahtree_append_batch(total, [t.data_ptr() if t is not None else None for t in dp],
                                       32, [g.ptr if g else None for g in dl],
                                       [g.ptr if g else None for g in ro], n0=n0, peaks=c.packed)
            md.synchronize()
            for d in range(G):
                what = (K, total, d, b)
                assert np.array_equal(dl[d].rows(), c.want_rows[cut[d]:cut[d + 1]]), what
                assert np.array_equal(ro[d].rows(), c.want_roots[b[d] - n0:b[d + 1] - n0]), what
                assert dl[d].guards_intact() and ro[d].guards_intact(), what
            # the host form, its outputs between guards too
            nb = len(c.want_rows) * 32
            hd = np.full(GUARD + nb + GUARD, FILL, np.uint8)
            hr = np.full(GUARD + 32 + GUARD, FILL, np.uint8)
            pk, pkp = _host_peaks(c.packed)
            N.check(L.mh_multi_ahtree_append_batch(md.handle, n0, pkp, c.pay.ctypes.data, total, 32,
                                                    hd.ctypes.data + GUARD, hr.ctypes.data + GUARD))
            assert np.array_equal(hd[GUARD:GUARD + nb].reshape(-1, 32), c.want_rows), (K, total)
            assert np.array_equal(hr[GUARD:GUARD + 32], c.want_roots[-1]), (K, total)
            for h, n in ((hd, nb), (hr, 32)):
                assert (h[:GUARD] == FILL).all() and (h[GUARD + n:] == FILL).all(), (K, total)
    finally:
        md.close()


def test_append_range_wide_table_arm(m, orc):
    """One call of 2^19 + 300 appends onto n0 = 2^40 + 2^18 + 1: level 1 has
    2^18 or more new nodes, so its perfect nodes go through the table-driven
    kernel with an edge, and n0 is odd, so the first level-1 node's left child
    is the frontier's slot 0.  The context's aht_perfect timer covers both
    perfect kernels and cannot tell them apart: that the table kernel runs
    follows from j1 - j0 >= 2^18 in launch_ahtree_perfect ((n0 + total) >> 1
    minus n0 >> 1 is 2^18 + 150).  The new dLog (about 201 MB) is copied down
    once; the first and last 300 appends, 2000 random ones and every multiple
    of 2^10 are compared in full, with their roots_out rows and the guards."""
    import torch
    from immustore_amd import _native as N
    L = N.load()
    n0, total = 2 ** 40 + 2 ** 18 + 1, 2 ** 19 + 300
    assert ((n0 + total) >> 1) - (n0 >> 1) >= 1 << 18 and n0 & 1
    rng = np.random.default_rng(5)
    smp = set(range(n0 + 1, n0 + 301)) | set(range(n0 + total - 299, n0 + total + 1))
    smp |= set(n0 + 1 + int(x) for x in rng.integers(0, total, 2000))
    smp |= set(range(((n0 >> 10) + 1) << 10, n0 + total + 1, 1 << 10))
    c = wide_case(orc, n0, total, samples=sorted(smp))
    nrows = nodes_upto(n0 + total) - nodes_upto(n0)
    ctx = m.Context(0)
    try:
        dp = _dev(c.pay)
        dl = Guarded(nrows * 32)
        ro = Guarded(total * 32)
        pk, pkp = _host_peaks(c.packed)
        torch.cuda.synchronize()
        N.check(L.mh_dev_ahtree_append_range(ctx.handle, dl.ptr, n0, pkp, dp.data_ptr(), total, 32,
                                             ro.ptr))
        ctx.synchronize()
        got = dl.rows()
        assert np.array_equal(sampled_rows(got, c), c.want_rows)
        roots = ro.rows()
        assert np.array_equal(roots[(c.samples - np.uint64(n0 + 1)).astype(np.int64)], c.want_roots)
        assert dl.guards_intact() and ro.guards_intact()
        del pk
    finally:
        ctx.close()
