"""EIP-7594 recover_cells_and_kzg_proofs restated in Python integers (test infrastructure), by the REFERENCE's steps
(constantine/data_availability_sampling/eth_peerdas.nim, recoverPolynomialCoeff; the validation of eth_eip7594_peerdas.nim): the full
vanishing polynomial Z(X) in coefficient form, two transforms of it over 8192 points and a pointwise division.  The library takes the
shortcut of one constant per cell (constantine_amd/csrc/recover_host.h); this file deliberately does not, so that the shortcut is
checked against an independent formulation.  About 0.3 s per blob."""
import functools
import json
import os
import random

from oracle import kzg_spec as ks
from tests import _golden, _nttref

R = ks.R
N, EXT, CELLS, CELL_ELEMS, CELL_BYTES = 4096, 8192, 128, 64, 2048
W4096 = pow(7, (R - 1) // 4096, R)
W8192 = pow(7, (R - 1) // 8192, R)
SHIFT = 5
SUCCESS, LENGTHS_MISMATCH, SCALAR_TOO_LARGE, NOT_ASCENDING = 0, 2, 4, 9


def validate(cell_indices, cells):
    """the reference's status for one blob's input; cells: len(cell_indices) byte strings of 2048"""
    n = len(cell_indices)
    if n < CELLS // 2 or n > CELLS:
        return LENGTHS_MISMATCH
    if any(i >= CELLS for i in cell_indices):
        return LENGTHS_MISMATCH
    if any(cell_indices[i - 1] >= cell_indices[i] for i in range(1, n)):
        return NOT_ASCENDING
    for c in cells:
        if any(int.from_bytes(c[32 * j:32 * j + 32], "big") >= R for j in range(CELL_ELEMS)):
            return SCALAR_TOO_LARGE
    return SUCCESS


def vanishing_coefficients(missing):
    """Z(X) = prod over the missing cells m of (X^64 - omega_128^brp7(m)): 8192 coefficients, non-zero at multiples of 64 only"""
    short = [1]
    for m in missing:
        root = pow(W8192, 64 * _nttref.brp(m, 7), R)
        short = [((short[i - 1] if i else 0) - root * (short[i] if i < len(short) else 0)) % R for i in range(len(short) + 1)]
    z = [0] * EXT
    for i, c in enumerate(short):
        z[64 * i] = c          # (64 missing cells: the leading 1 sits at 4096)
    return z


def recover_coefficients(cell_indices, cells):
    """-> the 8192 coefficients the reference's recoverPolynomialCoeff leaves (the high half is zero for cells of one blob)"""
    ext = [0] * EXT
    for i, c in zip(cell_indices, cells):
        for j in range(CELL_ELEMS):
            ext[64 * i + j] = int.from_bytes(c[32 * j:32 * j + 32], "big")
    z = vanishing_coefficients([m for m in range(CELLS) if m not in set(cell_indices)])
    z_eval = _nttref.ntt(z, R, W8192, out_brp=True)
    ez = _nttref.ntt([a * b % R for a, b in zip(ext, z_eval)], R, W8192, inverse=True, in_brp=True)
    ez_coset = _nttref.ntt(ez, R, W8192, out_brp=True, shift=SHIFT)
    z_coset = _nttref.ntt(z, R, W8192, out_brp=True, shift=SHIFT)
    p_coset = [a * pow(b, -1, R) % R for a, b in zip(ez_coset, z_coset)]
    return _nttref.ntt(p_coset, R, W8192, inverse=True, in_brp=True, shift=SHIFT)


def blob_of(coefs):
    """the blob of the polynomial truncated to 4096 coefficients (the consensus spec's and c-kzg's reading of inconsistent cells)"""
    ev = _nttref.ntt(coefs[:N], R, W4096, out_brp=True)
    return b"".join(v.to_bytes(32, "big") for v in ev)


@functools.lru_cache(maxsize=None)
def _recover_cached(cell_indices, cells):
    coefs = recover_coefficients(cell_indices, cells)
    return coefs, int(not any(coefs[N:])), blob_of(coefs)


def recover(cell_indices, cells):
    """-> (8192 coefficients, 1 if the high half is zero else 0, the blob's 131072 bytes); computed once per input"""
    return _recover_cached(tuple(cell_indices), tuple(bytes(c) for c in cells))


def coefficient_bytes(coefs):
    return b"".join(v.to_bytes(32, "little") for v in coefs)


# ---- the inputs the CPU harness test and the GPU test share ---------------------------------------------------------------------
def extended_cells(blob):
    """the 128 cells of a blob (tests/_peerdasref.cells without its imports of the MSM oracle)"""
    e = [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(N)]
    p = _nttref.ntt(e, R, W4096, inverse=True, in_brp=True)
    ext = _nttref.ntt(p, R, W4096, out_brp=True, shift=W8192)
    raw = bytes(blob) + b"".join(v.to_bytes(32, "big") for v in ext)
    return [raw[CELL_BYTES * k:CELL_BYTES * (k + 1)] for k in range(CELLS)]


def index_sets():
    rng = random.Random("peerdas-recover")
    return {
        "every_other": list(range(0, CELLS, 2)),
        "first_64": list(range(64)),
        "last_64": list(range(64, CELLS)),
        "random_64": sorted(rng.sample(range(CELLS), 64)),
        "random_65": sorted(rng.sample(range(CELLS), 65)),
        "all_but_0": list(range(1, CELLS)),
        "all_but_127": list(range(CELLS - 1)),
        "all_128": list(range(CELLS)),
    }


@functools.lru_cache(maxsize=None)
def value_cells(kind):
    """the 128 cells of: a fixture blob, the zero blob, a blob of r - 1 throughout, two more fixture-like blobs for batches"""
    if kind == "zero":
        blob = bytes(N * 32)
    elif kind == "r_minus_1":
        blob = (R - 1).to_bytes(32, "big") * N
    elif kind == "fixture":
        blob = next(b for _n, b, com in _golden.kzg4844_raw_cases() if com is not None and len(set(b)) > 16)
    else:
        rng = random.Random("blob-" + kind)
        blob = b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(N))
    return blob, extended_cells(blob)


def altered(cells, which, elem=17):
    """one element of cell `which` of the list changed (+1 mod r): no longer the evaluations of one polynomial of degree < 4096"""
    c = bytearray(cells[which])
    v = (int.from_bytes(c[32 * elem:32 * elem + 32], "big") + 1) % R
    c[32 * elem:32 * elem + 32] = v.to_bytes(32, "big")
    out = list(cells)
    out[which] = bytes(c)
    return out


def fixture_cases():
    """tests/golden/peerdas_recover.json -> [(case, cell_indices, [cell bytes], (128 cell digests, 128 proofs) | None)]"""
    import base64
    import zlib
    blobs = {name: blob for name, blob, _ in _golden.kzg4844_raw_cases()}
    expected = {ref: (dig, [bytes.fromhex(p) for p in proofs])
                for _c, ref, dig, proofs in json.load(open(os.path.join(_golden.HERE, "peerdas_cells_and_proofs.json"))) if dig is not None}
    out = []
    doc = json.load(open(os.path.join(_golden.HERE, "peerdas_recover.json")))
    names = doc["blobs"]
    for case, indices, cells, want in doc["cases"]:
        got = []
        for c in cells:
            if isinstance(c, int):
                got.append(_cells_of_case(names[c // CELLS], blobs[names[c // CELLS]])[c % CELLS])
            else:
                got.append(zlib.decompress(base64.b64decode(c)))
        out.append((case, indices, got, None if want is None else expected[names[want]]))
    return out


@functools.lru_cache(maxsize=None)
def _cells_of_case(name, blob):
    return extended_cells(blob)
