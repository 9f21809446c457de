"""EIP-7594 compute_cells / compute_cells_and_kzg_proofs restated in Python integers (test infrastructure): the four steps of
DESIGN.md section 13 over oracle.kzg_spec (blob parsing, the modulus), tests/_nttref.py (the transforms) and oracle.cref.msm (the
proofs' MSMs over the committed Lagrange SRS).  Pinned to the reference's vectors by tests/test_peerdas.py."""
import functools
import json
import os

import numpy as np

from oracle import cref
from oracle import kzg_spec as ks
from oracle import pyoracle as po
from tests import _golden, _nttref

R = ks.R
N, CELLS, CELL_ELEMS = 4096, 128, 64
W4096 = pow(7, (R - 1) // 4096, R)
W8192 = pow(7, (R - 1) // 8192, R)
CURVE = po.BLS12_381_G1


def fixture_cases():
    """-> [(case, blob bytes, [128 cell digests] | None, [128 proofs bytes] | None)]"""
    blobs = {name: blob for name, blob, _ in _golden.kzg4844_raw_cases()}
    doc = json.load(open(os.path.join(_golden.HERE, "peerdas_cells_and_proofs.json")))
    return [(case, blobs[ref], dig, None if proofs is None else [bytes.fromhex(p) for p in proofs]) for case, ref, dig, proofs in doc]


def coefficients(blob):
    """step 1: the blob holds evaluations at omega_4096^brp12(i) -> the polynomial's coefficients"""
    e = [int(bytes(row[::-1]).hex(), 16) for row in ks.blob_to_bigint_polynomial(blob)]
    return _nttref.ntt(e, R, W4096, inverse=True, in_brp=True)


def cells(blob, p=None):
    """step 2: 128 cells of 2048 bytes -- the blob's own bytes, then the evaluations on the coset omega_8192 * <omega_4096>"""
    p = coefficients(blob) if p is None else p
    ext = _nttref.ntt(p, R, W4096, out_brp=True, shift=W8192)
    raw = bytes(blob) + b"".join(v.to_bytes(32, "big") for v in ext)
    return [raw[2048 * k:2048 * (k + 1)] for k in range(CELLS)]


def c_of(k):
    return pow(W8192, 64 * _nttref.brp(k, 7), R)


def quotient(p, k):
    """step 3: q_k = p div (X^64 - c_k), 4096 coefficients (zero from 4032 on)"""
    c, q = c_of(k), [0] * N
    for j in range(N - 65, -1, -1):
        q[j] = (p[j + 64] + c * q[j + 64]) % R
    return q


@functools.lru_cache(maxsize=1)
def _srs():
    return CURVE.points_to_array(_golden.kzg4844_setup_points())


def proof(q):
    """step 4: the quotient's evaluations in bit-reversed order against the Lagrange SRS (stored in that order), compressed"""
    ev = _nttref.ntt(q, R, W4096, out_brp=True)
    out, _ = cref.msm("bls12_381_g1", CURVE.scalars_to_array(ev), _srs(), nthreads=4)
    return _golden.g1_compress(CURVE.aff_from_bytes(bytes(out)))


def quotients_array(p):
    """all 128 quotients as (128, 4096, 32) uint8 little-endian"""
    out = np.zeros((CELLS, N, 32), dtype=np.uint8)
    for k in range(CELLS):
        out[k] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in quotient(p, k)), dtype=np.uint8).reshape(N, 32)
    return out
