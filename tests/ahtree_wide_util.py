"""Shared by the CPU and GPU tests of ranged ahtree appends onto trees past
2^32: the cases, the oracle's digests for them and the dLog index math in
Python integers.

A ranged append needs no old dLog, only the 32-byte peak of every set bit of
n0, and a peak is an opaque digest: the tests fabricate them.  The reference
digests come from orc.ahtree_stream (orc_ahtree_stream, ahtree.go:287-322),
which appends from any 64-bit n_start keeping peaks only and does no dLog
index arithmetic, so it is independent of the index math under test."""
from collections import namedtuple

import numpy as np

# The tree-size domain: nodes_upto(n0 + total) * 32 < 2^63.  The reference
# keeps the dLog size and reads a node as int64 byte offsets (dLogSize =
# int64(nodesUpto(n) * sha256.Size), ahtree.go:232, :369; ReadAt(...,
# int64(i * sha256.Size)), :475), so a tree whose dLog would reach 2^63 bytes
# does not exist there.  nodes_upto(2^53) * 32 is about 2^62.8 (inside),
# nodes_upto(2^54) * 32 = 28 * 2^59 (outside).
WIDE_DOMAIN_BYTES = 1 << 63

WIDE_N0 = (
    2 ** 32 - 100,    # crosses 2^32 inside 300 appends; n = 2^32 builds 32 perfect
                      # levels whose left children all come from the frontier
    2 ** 32 - 1,      # the first append is n = 2^32
    2 ** 32,          # one set bit, at level 32
    2 ** 32 + 1,      # levels 0 and 32
    2 ** 40 + 12345,  # the size test_range_plan_properties plans at
    2 ** 44 + 126,    # two appends short of a spine-pair block edge
    2 ** 48 - 129,    # 40 set bits: spine chains of more than 40 frontier reads
    2 ** 53 - 127,    # the top of the domain, a spine-pair block edge
    2 ** 53 - 1,      # total 1 writes 54 digests, one per level
)
# 127 / 128 / 129: the spine-pair block edges; 2100 over 8 ranges gives k = 5
WIDE_TOTALS = (1, 2, 127, 128, 129, 300, 2100)


def popsum_below(x):
    """sum of popcount(i) for i < x, counted bit position by bit position:
    bit b is set in (x >> (b+1)) whole periods of 2^b numbers, plus the part of
    the last period past its first 2^b numbers."""
    s = 0
    for b in range(x.bit_length()):
        s += (x >> (b + 1)) << b
        s += max(0, (x & ((1 << (b + 1)) - 1)) - (1 << b))
    return s


def nodes_upto(n):
    """dLog digests of a tree of n appends: append i writes 1 + popcount(i-1)
    (ahtree.go:492-511), in Python integers."""
    return n + popsum_below(n)


def node_index(n, l):
    """dLog index of node(n, l): digest l of append n (ahtree.go:460-462)."""
    return nodes_upto(n - 1) + l


def in_domain(n0, total):
    return nodes_upto(n0 + total) * 32 < WIDE_DOMAIN_BYTES


WideCase = namedtuple("WideCase", "n0 total plen pay slots packed samples want_rows want_roots "
                                  "row count")
_CACHE = {}


def wide_case(orc, n0, total, plen=32, seed=7, samples=None):
    """The appends (n0, n0 + total] of fill_random(seed) payloads onto a tree
    of n0 whose peaks are fill_random(seed + 1) digests:
    pay (total, plen); slots (64, 32), slot l the peak of level l; packed, the
    library's `peaks` argument (slots at the set bits of n0, lowest first;
    None for n0 = 0); for the sampled appends (default: all, ascending)
    want_rows (R, 32), their digests concatenated, want_roots (len(samples),
    32), the last digest of each, row[i] / count[i], the range-relative dLog
    row nodes_upto(n-1) - nodes_upto(n0) and the digest count of sample i.
    Cached: the arrays are shared and read-only."""
    key = (n0, total, plen, seed, None if samples is None else tuple(samples))
    if key in _CACHE:
        return _CACHE[key]
    assert total >= 1 and in_domain(n0, total), (n0, total)
    pay = orc.fill_random(total * plen, seed).reshape(total, plen)
    slots = orc.fill_random(64 * 32, seed + 1).reshape(64, 32)
    packed = b"".join(slots[l].tobytes() for l in range(64) if (n0 >> l) & 1) if n0 else None
    if samples is None:
        smp = list(range(n0 + 1, n0 + total + 1))
    else:
        smp = sorted(set(int(n) for n in samples))
    res, _ = orc.ahtree_stream(seed, plen, n0, n0 + total, smp, peaks_in=slots, pay0=0)
    u0 = nodes_upto(n0)
    count = np.array([len(res[n]) for n in smp], np.int64)
    assert all(c == 1 + bin(n - 1).count("1") for c, n in zip(count, smp))
    if samples is None:  # consecutive appends: each starts where the one before ended
        row = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
        assert int(row[-1]) == nodes_upto(n0 + total - 1) - u0
    else:
        row = np.array([nodes_upto(n - 1) - u0 for n in smp], np.int64)
    want_rows = np.frombuffer(b"".join(b"".join(res[n]) for n in smp), np.uint8).reshape(-1, 32)
    want_roots = np.frombuffer(b"".join(res[n][-1] for n in smp), np.uint8).reshape(-1, 32)
    if samples is None:
        assert len(want_rows) == nodes_upto(n0 + total) - u0
    for a in (pay, slots, want_rows, want_roots, row, count):
        a.setflags(write=False)
    c = WideCase(n0, total, plen, pay, slots, packed, np.array(smp, np.uint64), want_rows,
                 want_roots, row, count)
    _CACHE[key] = c
    return c


def sampled_rows(got, case):
    """The rows of the range-relative dLog `got` (R, 32) that the sampled
    appends of `case` wrote, concatenated in sample order (compare with
    case.want_rows)."""
    idx = np.concatenate([np.arange(r, r + c) for r, c in zip(case.row, case.count)])
    return got[idx]
