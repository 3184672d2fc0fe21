"""CPU checks of the VerifiableGet answer tests' own reference
(tests/verifiable_entry_util.py): its descriptor against the reference's
compiled one, its digest / inclusion / dual-proof composition against a
Go-written store, and the make-up of the hostile set the GPU test runs."""
import collections
import json
import os

import numpy as np

import verifiable_entry_util as V


def test_descriptor_matches_reference_generated_descriptor(orc):
    """the ten messages declared in verifiable_entry_util == the reference's own
    compiled descriptor (schema.pb.go file_schema_proto_rawDesc, decoded by
    tests/golden/make_golden_entry.py): every field's name, number, type,
    label and message type; the other six of the closure are oracle/wire.py's,
    checked by test_wire_oracle.py."""
    from google.protobuf import descriptor_pb2
    import wire
    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "schema_fields_entry.json")))
    assert ref["package"] == "immudb.schema" and ref["syntax"] == "proto3"
    msgs = V.messages()
    assert set(ref["messages"]) == set(V.NEW_MESSAGES)
    for name, fields in ref["messages"].items():
        d = msgs[name].DESCRIPTOR
        assert d.full_name == "immudb.schema." + name
        dp = descriptor_pb2.DescriptorProto()
        d.CopyToProto(dp)
        assert [[f.name, f.number, f.type, f.label, f.type_name] for f in dp.field] == fields, name
    assert len(msgs) == 16
    for name in set(msgs) - set(V.NEW_MESSAGES):
        assert msgs[name] is wire.MSG[name]
    # every message type a field of the closure names is in the closure
    for cls in msgs.values():
        for f in cls.DESCRIPTOR.fields:
            if f.message_type is not None:
                assert f.message_type.name in msgs, (cls.DESCRIPTOR.name, f.name)


def _systemdb_answer(wire, fx, case, flip=False):
    from test_gpu_pb_decode import dual_v1_msg
    from test_tx_oracle import dual_v1_args
    from tx_util import headers_from_fixture
    from test_gpu_formats import _rec_hdr
    recs, blob, alhs = headers_from_fixture(fx["txs"])
    tx = fx["txs"][1]
    e = tx["entries"][0]
    key, value = bytes.fromhex(e["key"]), bytearray(bytes.fromhex(e["value"]))
    assert key == b"\x00\x01immudb" and value[:2] == b"\x00{" and tx["header"]["version"] == 0
    if flip:
        value[10] ^= 0x04
    M = V.messages()["VerifiableEntry"]()
    M.entry.tx, M.entry.key, M.entry.value = 2, key[1:], bytes(value[1:])
    M.inclusionProof.SetInParent()
    M.inclusionProof.leaf, M.inclusionProof.width = 0, 1
    M.verifiableTx.tx.header.CopyFrom(wire.tx_header_msg(_rec_hdr(recs[1], blob))[1])
    t = M.verifiableTx.tx.entries.add()
    t.key, t.hValue, t.vLen = key, bytes.fromhex(e["hval"]), len(value)
    M.verifiableTx.dualProof.ParseFromString(dual_v1_msg(wire, dual_v1_args(case, recs, blob, alhs)))
    return M, key[1:], alhs


def test_go_written_systemdb_entry(orc, fixtures):
    """v110_systemdb tx 2 is a server-written entry (key 00 01 "immudb", value
    00 {json...}, header v0).  With request key 01 "immudb" the helper's digest
    gives a leaf whose width-1 proof verifies against that tx's Go-written Eh,
    and with the fixture's Go-written dual proofs that contain tx 2 the
    reference accepts the answer for S = 0, 1, 2 -- and refuses it after a
    one-bit change to the value."""
    import wire
    fx = fixtures["v110_systemdb"]
    cases = {(c["src"], c["tgt"]): c for c in fx["dual_v1"]}
    eh = bytes.fromhex(fx["txs"][1]["header"]["eh"])
    M, key, alhs = _systemdb_answer(wire, fx, cases[(2, 2)])
    _, digest = V.entry_spec(orc, M, key, 0)
    assert orc.htree_verify_inclusion(0, 1, [], digest, eh)
    assert orc.sha256(b"\x00" + digest) == eh  # a width-1 tree's root is its leaf
    for S, pair in ((0, (2, 2)), (1, (1, 2)), (2, (2, 2))):
        M, key, alhs = _systemdb_answer(wire, fx, cases[pair])
        salh = alhs[S - 1] if S else bytes(32)
        assert V.reference(M.SerializeToString(), key, 0, S, salh) == (0, True, 2, alhs[1]), S
        assert V.reference(M.SerializeToString(), key, 2, S, salh) == (0, True, 2, alhs[1]), S
        bad, _, _ = _systemdb_answer(wire, fx, cases[pair], flip=True)
        assert V.reference(bad.SerializeToString(), key, 0, S, salh) == (0, False, 0, bytes(32)), S
        assert V.reference(M.SerializeToString(), key + b"x", 0, S, salh)[:2] == (0, False), S
    # a wrong state: the dual proof no longer starts from it
    M, key, alhs = _systemdb_answer(wire, fx, cases[(1, 2)])
    assert V.reference(M.SerializeToString(), key, 0, 1, bytes(32))[:2] == (0, False)


def test_reference_accepts_every_server_answer(orc):
    """the server restatement and the client reference agree on the whole
    synthetic store: every asked entry, from no state, the tx before, the tx
    itself, the one after and the last"""
    s = V.store()
    assert len(s.recs) == 48 and {int(v) for v in s.recs["version"]} == {0, 1}
    assert set(V.WIDTHS) == set(s.width.values())
    for sl in s.slots:
        for S in sorted({0, sl.tx - 1, sl.tx, min(sl.tx + 1, V.N_TX), V.N_TX}):
            raw = V.answer(sl, S).SerializeToString()
            want = (0, True, max(S, sl.tx), s.alhs[max(S, sl.tx) - 1])
            assert V.reference(raw, sl.key, 0, S, V.state_alh(S)) == want, (sl.tx, sl.leaf, S)


def test_hostile_set_shares(orc):
    """under the reference alone, each outcome -- not an encoding (status 14),
    decoded and refused (status 0, ok 0), accepted (status 0, ok 1) -- holds at
    least 5 % of the hostile set: the GPU test cannot pass on "everything is
    corrupt" or "everything verifies"."""
    h = V.hostile_set()
    assert 1300 <= len(h) <= 1700
    c = collections.Counter(V.reference(*a)[:2] for a in h)
    for outcome in ((14, False), (0, False), (0, True)):
        assert c[outcome] >= 0.05 * len(h), (outcome, dict(c))
    assert np.sum(list(c.values())) == len(h)
