#!/usr/bin/env python3
"""
Re-encode the reference's EIP-7594 `verify_cell_kzg_proof_batch` and `compute_verify_cell_kzg_proof_batch_challenge` vectors into one
small fixture, and cut the verifier's part out of the ceremony file.  Run where /root/reference exists:

    python tests/golden/make_golden_peerdas_verify.py

Sources (reference-relative):
  tests/protocol_ethereum_eip7594_fulu_peerdas/verify_cell_kzg_proof_batch/kzg-mainnet/*/data.yaml
  tests/protocol_ethereum_eip7594_fulu_peerdas/compute_verify_cell_kzg_proof_batch_challenge/kzg-mainnet/*/data.yaml
      -> peerdas_verify.json : {"blobs": [blob_case, ...],
                                "verify": [[case, [commitment hex], [cell index], [cell], [proof hex], true | false | null], ...],
                                "challenge": [[case, [commitment hex], [commitment index], [cell index], [cell], [proof hex], hex], ...]}
         cell: 128 * blob + position for a cell of a blob of kzg4844_blob_to_commitment.json (matched by its SHA-256 in
         peerdas_cells_and_proofs.json), else zlib+base64 of its bytes (a challenge vector's cosets_evals are the cell's 64 elements)
         proof: 128 * blob + position likewise (the first match), commitment: the blob's number, else the hex string
  constantine/commitments_setups/trusted_setup_ethereum_kzg4844_reference.dat
      -> kzg4844_srs_verify.bin : the first 64 monomial G1 points (64 x 48 bytes), then G2 line 64, [tau^64]_2 (96 bytes)
"""
import base64
import glob
import hashlib
import json
import os
import re
import zlib

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = f"{REF}/tests/protocol_ethereum_eip7594_fulu_peerdas"


def _list(head, key):
    """the flat list of quoted hex strings or of integers under `key:`"""
    m = re.search(r"^  %s:(.*?)(?=^  [a-z_]+:|\Z)" % key, head, re.S | re.M)
    body = m.group(1)
    inline = re.match(r"\s*\[([^\]]*)\]", body)
    if inline and "'" not in inline.group(1):
        return [int(x) for x in inline.group(1).split(",") if x.strip()]
    return re.findall(r"'0x([0-9a-f]*)'", body)


def main():
    where, names, known = {}, [], {}
    for _case, ref, digests, proofs in json.load(open(os.path.join(HERE, "peerdas_cells_and_proofs.json"))):
        if digests is None:
            continue
        if ref not in names:
            names.append(ref)
        for k, d in enumerate(digests):
            where.setdefault(d, 128 * names.index(ref) + k)
            known.setdefault(proofs[k], 128 * names.index(ref) + k)
    for name, _z, com in json.load(open(os.path.join(HERE, "kzg4844_blob_to_commitment.json"))):
        if name in names:
            known.setdefault(com, names.index(name))
    assert not set(where) & set(known)

    def points(hexes):
        return [known.get(h, h) for h in hexes]
    literal = [0]

    def cell(raw):
        at = where.get(hashlib.sha256(raw).hexdigest())
        if at is not None:
            return at
        literal[0] += 1
        return base64.b64encode(zlib.compress(raw, 9)).decode()

    verify = []
    for d in sorted(glob.glob(f"{VECTORS}/verify_cell_kzg_proof_batch/kzg-mainnet/*")):
        name = os.path.basename(d).replace("verify_cell_kzg_proof_batch_case_", "")
        head, out = open(f"{d}/data.yaml").read().split("output:")
        want = {"true": True, "false": False, "null": None}[out.strip()]
        verify.append([name, points(_list(head, "commitments")), _list(head, "cell_indices"), [cell(bytes.fromhex(c)) for c in _list(head, "cells")],
                       points(_list(head, "proofs")), want])
    challenge = []
    for d in sorted(glob.glob(f"{VECTORS}/compute_verify_cell_kzg_proof_batch_challenge/kzg-mainnet/*")):
        name = os.path.basename(d).replace("compute_verify_cell_kzg_proof_batch_challenge_case_", "")
        head, out = open(f"{d}/data.yaml").read().split("output:")
        evals = _list(head, "cosets_evals")
        assert len(evals) % 64 == 0 and all(len(e) == 64 for e in evals), name
        cells = [cell(bytes.fromhex("".join(evals[64 * k:64 * k + 64]))) for k in range(len(evals) // 64)]
        challenge.append([name, points(_list(head, "commitments")), _list(head, "commitment_indices"), _list(head, "cell_indices"), cells,
                          points(_list(head, "proofs")), re.search(r"'0x([0-9a-f]{64})'", out).group(1)])
    assert len(verify) == 32 and len(challenge) == 10
    assert [v[5] for v in verify].count(True) == 12 and [v[5] for v in verify].count(False) == 3
    path = os.path.join(HERE, "peerdas_verify.json")
    json.dump({"blobs": names, "verify": verify, "challenge": challenge}, open(path, "w"), separators=(",", ":"))
    print(len(verify), "+", len(challenge), "cases;", literal[0], "literal cells;", os.path.getsize(path), "bytes")

    lines = open(f"{REF}/constantine/commitments_setups/trusted_setup_ethereum_kzg4844_reference.dat").read().split()
    assert lines[0] == "4096" and lines[1] == "65" and len(lines) == 2 + 4096 + 65 + 4096
    g2 = lines[2 + 4096:2 + 4096 + 65]
    g1m = lines[2 + 4096 + 65:]
    raw = b"".join(bytes.fromhex(x) for x in g1m[:64]) + bytes.fromhex(g2[64])
    assert len(raw) == 64 * 48 + 96
    open(os.path.join(HERE, "kzg4844_srs_verify.bin"), "wb").write(raw)
    print("kzg4844_srs_verify.bin", len(raw), "bytes; G2 generator line:", g2[0][:16], "...")


if __name__ == "__main__":
    main()
