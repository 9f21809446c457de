#!/usr/bin/env python3
"""
Re-encode the reference's Banderwagon / Verkle vectors into a small fixture.

Run in the build container (where /root/reference exists):
    python tests/golden/make_golden_banderwagon.py

Sources (reference-relative):
  tests/t_ethereum_verkle_primitives.nim         expected_bit_strings (serialisations of G, 2G, 4G, ...), bad_bit_string
                                                 (on the curve, not in the subgroup)
  tests/t_ethereum_verkle_ipa_primitives.nim     the CRS's first and 256th points, the expected vector commitment
  tests/t_ethereum_verkle_ipa_test_helper.nim    testScalarsHex: the 256 commitment scalars
      -> banderwagon_verkle.json : {"doublings": [...], "not_in_subgroup": [...], "crs0": hex, "crs255": hex,
                                    "commit_scalars": [...], "commitment": hex}

The GPU box has no /root/reference: tests read only the file written here.
"""
import json
import os
import re

REF = "/root/reference/tests"
HERE = os.path.dirname(os.path.abspath(__file__))
HEX = re.compile(r'"(0x[0-9a-fA-F]+)"')


def hex_array(path, name):
    text = open(os.path.join(REF, path)).read()
    start = text.index(f"{name}")
    body = text[text.index("[", text.index("=", start)):]
    body = body[:body.index("]") + 1]
    return HEX.findall(body)


def commented_hex(path, what):
    for line in open(os.path.join(REF, path)):
        if what in line:
            return HEX.findall(line)[0]
    raise KeyError(what)


def main():
    prim, ipa = "t_ethereum_verkle_primitives.nim", "t_ethereum_verkle_ipa_primitives.nim"
    out = {
        "doublings": hex_array(prim, "expected_bit_strings"),
        "not_in_subgroup": hex_array(prim, "bad_bit_string"),
        "crs0": commented_hex(ipa, "Failed to generate the 1st point"),
        "crs255": commented_hex(ipa, "Failed to generate the 256th point"),
        "commit_scalars": hex_array("t_ethereum_verkle_ipa_test_helper.nim", "testScalarsHex"),
        "commitment": commented_hex(ipa, "bit string does not match expected"),
    }
    assert len(out["doublings"]) == 16 and len(out["not_in_subgroup"]) == 16 and len(out["commit_scalars"]) == 256
    with open(os.path.join(HERE, "banderwagon_verkle.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
