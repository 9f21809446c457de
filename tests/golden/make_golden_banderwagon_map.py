#!/usr/bin/env python3
"""
Re-encode the reference's map-to-scalar-field vectors into a small fixture.

Run in the build container (where /root/reference exists):
    python tests/golden/make_golden_banderwagon_map.py

Source (reference-relative): tests/t_ethereum_verkle_primitives.nim
  expected_scalar_field_elements   batchMapToScalarField of 2G and 4G (test data generated from go-ipa)
  testMapToField                   a serialised point and its scalar (verkle-test-vectors 002_map_to_field_element.json)
      -> banderwagon_map_to_field.json : {"multiples_of_g": [[k, scalar hex], ...], "serialized": [[point hex, scalar hex]]}

The GPU box has no /root/reference: tests read only the file written here.
"""
import json
import os
import re

REF = "/root/reference/tests/t_ethereum_verkle_primitives.nim"
HERE = os.path.dirname(os.path.abspath(__file__))
HEX = re.compile(r'"(0x[0-9a-fA-F]{64})"')


def main():
    text = open(REF).read()
    body = text[text.index("expected_scalar_field_elements"):]
    body = body[body.index("="):]
    two = HEX.findall(body[:body.index("]")])
    body = text[text.index("proc testMapToField() ="):]
    body = body[:body.index("doAssert")]
    scalar, point = HEX.findall(body)[:2]
    assert len(two) == 2 and "expected_field_element" in body[:body.index(scalar)]
    out = {"multiples_of_g": [[2, two[0]], [4, two[1]]], "serialized": [[point, scalar]]}
    with open(os.path.join(HERE, "banderwagon_map_to_field.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
