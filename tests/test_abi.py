"""CPU-side checks of the drop-in boundary (no GPU needed).

- the C-ABI library builds for gfx950 and exports every symbol declared in
  include/immustore_merkle.h
- the ctypes mirror declares exactly that symbol set
- pure host-side index math (levels layout, nodesUpto) agrees with the oracle
- without a device the product fails loudly (no silent CPU fallback)
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immustore_merkle.h")
LIB = os.path.join(ROOT, "immustore_amd", "libimmustore_merkle.so")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "immustore_amd", "csrc"), "-j4"],
                       check=True)
    return LIB


def test_exports_match_header(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (mh_[a-z0-9_]+)", out))
    declared = header_symbols()
    assert declared, "no declarations parsed"
    assert declared - exported == set(), "declared but not exported"
    assert exported - declared == set(), "exported but not declared"


def test_ctypes_mirror_matches_header(lib_built):
    from immustore_amd import _native
    assert set(_native.SIGNATURES) == header_symbols()
    L = _native.load()
    for name in _native.SIGNATURES:
        assert hasattr(L, name)


def test_gfx950_code_object(lib_built):
    blob = open(lib_built, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob


def test_host_index_math(lib_built, orc):
    import immustore_amd as m
    for n in list(range(0, 70)) + [1000, 1023, 1024, 1025, 4097, 1 << 20, (1 << 20) + 3]:
        assert m.levels_len(n) == orc.levels_len(n)
        for lvl in range(0, 22):
            if n and lvl < max(1, (n - 1).bit_length() + 1):
                assert m.level_offset(n, lvl) == orc.level_offset(n, lvl)
    for n in list(range(1, 200)) + [10 ** 7, 2 ** 40 + 12345]:
        assert m.nodes_upto(n) == orc.nodes_upto(n)
    # BASELINE C3: 10^7 appends -> 124,434,624 dLog digests
    assert m.nodes_upto(10 ** 7) == 124434624
    # trees past 2^32 (the ranged appends' sizes): the library's 64-bit index
    # math against the same sums in Python integers
    import ctypes as C
    from immustore_amd import _native as N
    from ahtree_wide_util import WIDE_N0, in_domain, node_index, nodes_upto
    L = N.load()
    for n0 in WIDE_N0:
        for n in (n0 - 1, n0, n0 + 1, n0 + 2100):
            assert in_domain(n, 0)
            assert L.mh_ahtree_nodes_upto(n) == nodes_upto(n), n
            for lvl in (0, (n & -n).bit_length() - 1, 52):
                assert L.mh_ahtree_node_index(n, lvl) == node_index(n, lvl), (n, lvl)
        for total in (1, 300, 2100, 20011):
            for K in (1, 2, 3, 8, 64):
                assert _range_sizes(L, n0, total, K) == _range_sizes_py(L, n0, total, K), \
                    (n0, total, K)
    k, g = C.c_int(), C.c_int()
    b = (C.c_uint64 * 5)()
    assert L.mh_ahtree_range_plan(2 ** 64 - 10, 20, 4, C.byref(k), b, C.byref(g)) == \
        N.MH_ERR_ILLEGAL_ARGUMENTS
    s, w = C.c_uint64(), C.c_uint64()
    assert L.mh_ahtree_range_sizes(2 ** 64 - 10, 20, 4, C.byref(s), C.byref(w)) == \
        N.MH_ERR_ILLEGAL_ARGUMENTS


_AHT_WORK_HEAD = 64 * 32 * 2 + 256  # kAhtWorkHead: peaks | frontier | work counter


def _range_sizes(L, n0, total, K):
    import ctypes as C
    s, w = C.c_uint64(), C.c_uint64()
    assert L.mh_ahtree_range_sizes(n0, total, K, C.byref(s), C.byref(w)) == 0
    return s.value, w.value


def _range_sizes_py(L, n0, total, K):
    """(send_bytes, work_bytes) restated from the plan: Pmax send slots, the
    largest count of pieces ending in one range, and one top-buffer slot per
    piece-tree node of every level l with Pend >> l != 0, slots
    N0 >> l .. Pend >> l."""
    from immustore_amd.multi import ahtree_range_plan
    k, b = ahtree_range_plan(n0, total, K)
    pmax = max([1] + [(y >> k) - (x >> k) for x, y in zip(b, b[1:])])
    N0, Pend = n0 >> k, b[-1] >> k
    slots, lvl = 0, 0
    while lvl < 64 - k and (Pend >> lvl):
        slots += (Pend >> lvl) - (N0 >> lvl) + 1
        lvl += 1
    return pmax * 32, _AHT_WORK_HEAD + 32 * slots


def test_no_silent_cpu_fallback(lib_built):
    import torch  # noqa: F401  (same HIP runtime as the GPU box)
    import immustore_amd as m
    if m.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(m.ErrNoDevice):
        m.Context(0)
