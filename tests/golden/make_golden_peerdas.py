#!/usr/bin/env python3
"""
Re-encode the reference's EIP-7594 (Fulu / PeerDAS) `compute_cells` and `compute_cells_and_kzg_proofs` vectors into one small fixture.
Run where /root/reference exists:

    python tests/golden/make_golden_peerdas.py

Sources (reference-relative):
  tests/protocol_ethereum_eip7594_fulu_peerdas/compute_cells/kzg-mainnet/*/data.yaml
  tests/protocol_ethereum_eip7594_fulu_peerdas/compute_cells_and_kzg_proofs/kzg-mainnet/*/data.yaml
      -> peerdas_cells_and_proofs.json : [[case, blob_case, [128 SHA-256 digests of the cells] | null, [128 proofs, hex] | null], ...]

Every blob of these vectors is one of kzg4844_blob_to_commitment.json (matched by SHA-256; the two wrong-length blobs by their
length, "LEN:n" there): blob_case names it, the blob is not stored again.  A cell is 2048 bytes, so the fixture keeps its digest.  The
two directories must agree on the cells of the same blob.
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


def main():
    by_hash, by_len = {}, {}
    for name, blob, _out in json.load(open(os.path.join(HERE, "kzg4844_blob_to_commitment.json"))):
        if blob.startswith("LEN:"):
            by_len[int(blob[4:])] = name
        else:
            by_hash[hashlib.sha256(zlib.decompress(base64.b64decode(blob))).hexdigest()] = name
    base = f"{REF}/tests/protocol_ethereum_eip7594_fulu_peerdas"
    cells_of = {}     # blob_case -> digests, from compute_cells
    for d in sorted(glob.glob(f"{base}/compute_cells/kzg-mainnet/*")):
        t = open(f"{d}/data.yaml").read()
        blob = bytes.fromhex(re.search(r"blob: '0x([0-9a-f]*)'", t).group(1))
        key = by_hash.get(hashlib.sha256(blob).hexdigest()) or by_len[len(blob)]
        if "output: null" in t:
            cells_of[key] = None
            continue
        cells = re.findall(r"'0x([0-9a-f]{4096})'", t.split("output:")[1])
        assert len(cells) == 128
        cells_of[key] = [hashlib.sha256(bytes.fromhex(c)).hexdigest() for c in cells]
    cases = []
    for d in sorted(glob.glob(f"{base}/compute_cells_and_kzg_proofs/kzg-mainnet/*")):
        t = open(f"{d}/data.yaml").read()
        blob = bytes.fromhex(re.search(r"blob: '0x([0-9a-f]*)'", t).group(1))
        key = by_hash.get(hashlib.sha256(blob).hexdigest()) or by_len[len(blob)]
        name = os.path.basename(d)
        if "output: null" in t:
            assert cells_of[key] is None, name
            cases.append([name, key, None, None])
            continue
        out = t.split("output:")[1]
        cells = re.findall(r"'0x([0-9a-f]{4096})'", out)
        proofs = re.findall(r"'0x([0-9a-f]{96})'", out)
        assert len(cells) == 128 and len(proofs) == 128, name
        digests = [hashlib.sha256(bytes.fromhex(c)).hexdigest() for c in cells]
        assert digests == cells_of[key], (name, "the two directories disagree on the cells")
        cases.append([name, key, digests, proofs])
    path = os.path.join(HERE, "peerdas_cells_and_proofs.json")
    json.dump(cases, open(path, "w"), separators=(",", ":"))
    print(len(cases), "cases;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
