#!/usr/bin/env python3
"""Generate tests/golden/schema_fields_entry.json: the field tuples of the
messages a VerifiableGet answer (schema.VerifiableEntry) contains beyond the
proof messages of schema_fields.json.

TEST INFRASTRUCTURE ONLY, run once where the reference is available, as
make_golden.py (whose schema_fields() this follows; that script stays as it
is).  Data only: the byte literal of the reference's generated descriptor
(pkg/api/schema/schema.pb.go, file_schema_proto_rawDesc) is parsed and decoded
here, nothing of the Go file is kept but (name, number, type, label, type_name)
per field.
"""
import json
import os
import re
import sys

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

ENTRY_MESSAGES = ("VerifiableEntry", "Entry", "Reference", "KVMetadata", "Expiration",
                  "VerifiableTx", "Tx", "TxEntry", "ZEntry", "Signature")


def schema_fields_entry():
    from google.protobuf import descriptor_pb2
    lines = open(os.path.join(REF, "pkg/api/schema/schema.pb.go")).read().split("\n")
    start = next(k for k, ln in enumerate(lines)
                 if ln.startswith("var file_schema_proto_rawDesc = []byte{"))
    raw = bytearray()
    for ln in lines[start + 1:]:
        if ln.startswith("}"):
            break
        raw += bytes(int(x, 16) for x in re.findall(r"0x([0-9a-f]{2})", ln))
    fdp = descriptor_pb2.FileDescriptorProto.FromString(bytes(raw))
    out = {"package": fdp.package, "syntax": fdp.syntax, "messages": {}}
    for m in fdp.message_type:
        if m.name in ENTRY_MESSAGES:
            assert not m.oneof_decl and not m.nested_type, m.name
            out["messages"][m.name] = [[f.name, f.number, f.type, f.label, f.type_name]
                                       for f in m.field]
    assert set(out["messages"]) == set(ENTRY_MESSAGES)
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (build container only)")
    with open(os.path.join(OUT, "schema_fields_entry.json"), "w") as f:
        json.dump(schema_fields_entry(), f, indent=1, sort_keys=True)
    print("ok")


if __name__ == "__main__":
    main()
