"""The checker of the DualProof (v1) generator checked (no GPU): the CPU
restatement in dual_v1_gen_util.py reproduces every v1 proof the Go stores
emitted (tests/golden/immudb_fixtures.json, 478 cases over three stores), part
by part and as the marshalled message; and the synthetic store the GPU tests
use crosses every boundary of the device writer."""
import pytest

import dual_v1_gen_util as U
from tx_util import headers_from_fixture, inner_hashes


@pytest.fixture(scope="module")
def wire(orc):
    import wire
    return wire


def _fixture_tree(orc, fx):
    import numpy as np
    pay = np.stack([np.frombuffer(bytes.fromhex(p), np.uint8) for p in fx["aht_payloads"]])
    o = orc.AHtree(len(pay))
    o.append_batch(pay)
    return o


def test_restatement_matches_go_stores(orc, wire, fixtures):
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    n = 0
    assert len(fixtures) == 3
    for name, fx in fixtures.items():
        recs, blob, alhs = headers_from_fixture(fx["txs"])
        inners = inner_hashes(orc, recs, blob)
        aht = _fixture_tree(orc, fx)
        for c in fx["dual_v1"]:
            s, t = c["src"], c["tgt"]
            want = dual_v1_args(c, recs, blob, alhs)
            st, parts = U.go_dual_proof_parts(recs[s - 1], recs[t - 1], blob, aht, 1, alhs, inners)
            assert st == 0, (name, s, t)
            assert list(parts[3:9]) == list(want[3:9]), (name, s, t)
            st, raw = U.go_dual_proof(recs[s - 1], recs[t - 1], blob, aht, 1, alhs, inners)
            assert st == 0 and raw == dual_v1_msg(wire, want), (name, s, t)
            assert U.dual_v1_marshal(parts) == raw, (name, s, t)
            n += 1
    assert n == 478


def test_synthetic_store_crosses_every_boundary(orc):
    s = U.synthetic_store()
    pairs, exp = U.synthetic_pairs(), U.synthetic_expected()
    assert len(pairs) >= 400 + len(U.BOUNDARY_PAIRS)
    assert all(a <= b for a, b in pairs)
    bls = [U.bl_of(k) for k in range(1, U.N_TX + 1)]
    assert bls == sorted(bls) and all(b < k for k, b in enumerate(bls, 1))
    assert all(st == 0 for st, _ in exp)
    parts = [p for _, p in exp]
    laps = [p[8] for p in parts if p[8] is not None]
    assert len(laps) >= 50
    assert any(p[8] is None for p in parts)                       # the nil advance proof
    assert any(int(p[1]["bl_tx_id"]) == 0 and p[5] == bytes(32) for p in parts)  # tgt.bl == 0
    assert any(int(p[0]["id"]) == int(p[1]["id"]) for p in parts)  # src == tgt
    nested = {len(lap[1]) for lap in laps}
    assert {63, 64, 65, 127, 128, 129} <= nested                  # the wave / round boundaries
    assert {50, 51, 52, 102, 103} <= nested                       # rounds of 51 proofs (bl = 999)
    # nested proofs with 1-byte (<= 3 terms) and 2-byte (>= 4 terms) lengths; none is empty
    # (InclusionProof(k, j) with k < j always has a term)
    nt = {len(ip) for lap in laps for ip in lap[1]}
    assert min(nt) >= 1 and min(nt) <= 3 and max(nt) >= 4
    # sub-message lengths of 1, 2 and 3 bytes
    lin = [U.linear_body_len(p[7]) for p in parts]
    adv = [U.advance_body_len(lap) for lap in laps]
    assert min(lin) < 128
    for lens in (lin, adv):
        assert any(128 <= x <= 16383 for x in lens) and max(lens) > 16383
    assert {481, 482, 483} <= {len(p[7][2]) for p in parts}        # linear: 16 360 / 16 394 bytes
    assert {481, 482, 483} <= {len(lap[0]) for lap in laps}
    # the advance body crosses 16 383 between two neighbouring sources
    edge = sorted(U.advance_body_len(p[8]) for (a, b), p in zip(pairs, parts)
                  if b == 1000 and 232 <= a < 252)
    assert edge[0] <= 16383 < edge[-1]
    assert [U.dual_v1_marshal(p) for p in parts[::5]] == list(U.synthetic_messages()[::5])
    # the chain is consistent: every generated proof verifies
    for (a, b), p in zip(pairs, parts):
        assert orc.verify_dual_proof(s.crecs[a - 1], s.crecs[b - 1], s.cblob, *p[3:], a, b,
                                     s.alhs[a - 1], s.alhs[b - 1]), (a, b)


def test_restatement_status_order(orc):
    """the rules of the issue, one each, on the synthetic store (the GPU test
    runs the same cases through the device)"""
    for name, st, want, _ in U.status_cases():
        assert st == want, name
