"""The fused DualProof (v1) wire verify without a device: its CPU reference
(dual_v1_verify_util.reference) against the Go stores' proofs and the C
oracle, and the new entry points through every layer of the bindings."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mh_verify_dual_proof_pb_batch", "mh_multi_verify_dual_proof_pb_batch")


@pytest.fixture(scope="module")
def wire(orc):
    import wire
    return wire


@pytest.fixture(scope="module")
def go_cases(fixtures):
    """(orc.verify_dual_proof arguments, tamper) of every dual_v1 case of the
    Go stores, untampered and with each of the four tampers"""
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture
    out = []
    for name, fx in fixtures.items():
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        for c in fx["dual_v1"]:
            for tamper in (None, "lap", "lin", "last", "tbl"):
                out.append((dual_v1_args(c, recs, blob, alhs, tamper), tamper))
    return out


def test_reference_accepts_go_store_proofs(orc, wire, go_cases):
    from dual_v1_verify_util import reference
    from test_gpu_pb_decode import dual_v1_msg
    n = 0
    for a, tamper in go_cases:
        if tamper is None:
            assert reference(wire, orc, dual_v1_msg(wire, a), *a[9:13]) == (0, True), a[9:11]
            n += 1
    assert n == 478


def test_reference_equals_oracle_on_tampers(orc, wire, go_cases):
    from dual_v1_verify_util import reference
    from test_gpu_pb_decode import dual_v1_msg
    seen = {}
    for a, tamper in go_cases:
        if tamper is None:
            continue
        exp = orc.verify_dual_proof(*a)
        assert reference(wire, orc, dual_v1_msg(wire, a), *a[9:13]) == (0, exp), (tamper, a[9:11])
        seen.setdefault(tamper, set()).add(exp)
    assert set(seen) == {"lap", "lin", "last", "tbl"}
    assert all(False in v for v in seen.values())  # every tamper breaks some proof


def test_reference_statuses(orc, wire, go_cases):
    """no linear proof -> 2, a cut message -> 14, wrong ids / Alh -> false"""
    from dual_v1_verify_util import reference
    from test_gpu_pb_decode import dual_v1_msg
    a = next(a for a, t in go_cases if t is None and a[8] is not None)
    raw = dual_v1_msg(wire, a)
    s, t, sa, ta = a[9:13]
    assert reference(wire, orc, raw, s, t, sa, ta) == (0, True)
    assert reference(wire, orc, dual_v1_msg(wire, a[:7] + (None,) + a[8:]), s, t, sa, ta) == (2, False)
    assert reference(wire, orc, raw[:len(raw) - 5], s, t, sa, ta) == (14, False)
    assert reference(wire, orc, b"", s, t, sa, ta) == (2, False)
    assert reference(wire, orc, raw, s, t + 1, sa, ta) == (0, False)
    assert reference(wire, orc, raw, s, t, bytes(32), ta) == (0, False)
    # a nil LinearAdvanceProof where one is needed: verified as it stands
    assert reference(wire, orc, dual_v1_msg(wire, a[:8] + (None,) + a[9:]), s, t, sa, ta) == (0, False)


def test_header_declares_both_functions():
    src = open(os.path.join(ROOT, "include", "immustore_merkle.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        args = [x.strip() for x in m.group(1).split(",")]
        assert len(args) == 10, (name, args)
        assert args[-2].startswith("int32_t *") and args[-1].startswith("uint8_t *"), args


def test_native_mirrors_both_functions():
    import ctypes as C
    from immustore_amd import _native as N
    for name in NAMES:
        assert name in N.SIGNATURES, name
        res, argtypes = N.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == 10
        assert hasattr(N.load(), name)


def test_python_wrappers_exposed():
    import inspect
    from immustore_amd import multi, txlayer
    f = txlayer.verify_dual_proof_pb_batch
    assert list(inspect.signature(f).parameters) == ["msgs", "src", "tgt", "src_alh", "tgt_alh", "ctx"]
    g = multi.MultiDevice.verify_dual_proof_pb_batch
    assert list(inspect.signature(g).parameters) == ["self", "msgs", "src", "tgt", "src_alh", "tgt_alh"]
