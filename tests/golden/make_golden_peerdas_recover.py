#!/usr/bin/env python3
"""
Re-encode the reference's EIP-7594 `recover_cells_and_kzg_proofs` vectors into one small fixture.  Run where /root/reference exists:

    python tests/golden/make_golden_peerdas_recover.py

Source (reference-relative):
  tests/protocol_ethereum_eip7594_fulu_peerdas/recover_cells_and_kzg_proofs/kzg-mainnet/*/data.yaml
      -> peerdas_recover.json : {"blobs": [blob_case, ...],
                                 "cases": [[case, cell_indices, [128 * blob + position | zlib+base64 of the cell's bytes, ...], blob | null], ...]}
         (blob: an index into "blobs")

Every input cell of these vectors is a cell of a blob of kzg4844_blob_to_commitment.json, matched by its SHA-256 in
peerdas_cells_and_proofs.json and stored as one number, 128 * blob + position; the one altered cell of each invalid_cell_* case is stored as its bytes
(it may be 2047, 2048 or 2049 bytes long).  The output of a valid case is the full set of cells and proofs of one of those blobs: the
last field names it (asserted here), null = the reference rejects the input.
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
    where, full, names = {}, {}, []
    for _case, ref, digests, proofs in json.load(open(os.path.join(HERE, "peerdas_cells_and_proofs.json"))):
        if digests is None:
            continue
        if ref not in names:
            names.append(ref)
        for k, d in enumerate(digests):
            where.setdefault(d, 128 * names.index(ref) + k)
        full.setdefault((tuple(digests), tuple(proofs)), names.index(ref))
    cases, literal = [], 0
    for d in sorted(glob.glob(f"{REF}/tests/protocol_ethereum_eip7594_fulu_peerdas/recover_cells_and_kzg_proofs/kzg-mainnet/*")):
        name = os.path.basename(d)
        head, out = open(f"{d}/data.yaml").read().split("output:")
        indices = [int(x) for x in re.search(r"cell_indices: \[([^\]]*)\]", head).group(1).split(",") if x.strip()]
        cells = []
        for c in re.findall(r"- '0x([0-9a-f]*)'", head):
            raw = bytes.fromhex(c)
            at = where.get(hashlib.sha256(raw).hexdigest())
            if at is None:
                literal += 1
                cells.append(base64.b64encode(zlib.compress(raw, 9)).decode())
            else:
                cells.append(at)
        want = None
        if "null" not in out[:8]:
            oc = re.findall(r"'0x([0-9a-f]{4096})'", out)
            op = re.findall(r"'0x([0-9a-f]{96})'", out)
            assert len(oc) == 128 and len(op) == 128, name
            want = full[(tuple(hashlib.sha256(bytes.fromhex(c)).hexdigest() for c in oc), tuple(op))]
        cases.append([name, indices, cells, want])
    path = os.path.join(HERE, "peerdas_recover.json")
    json.dump({"blobs": names, "cases": cases}, open(path, "w"), separators=(",", ":"))
    print(len(cases), "cases;", literal, "literal cells;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
