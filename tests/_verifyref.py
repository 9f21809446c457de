"""EIP-7594 verify_cell_kzg_proof_batch restated in Python integers (test infrastructure): the consensus spec's universal verification
equation with the reference's order of checks (constantine/eth_eip7594_peerdas.nim:512-619), its deduplication of the commitments on
their bytes, and its weights r^(k+1).  The interpolation polynomial of every cell is formed by LAGRANGE INTERPOLATION on the cell's
coset, cell by cell; the library sums the cells of a column first and runs one inverse transform per column
(constantine_amd/csrc/verify_host.h), so the two formulations check each other.  Pinned to the reference's 42 vectors by
tests/test_peerdas_verify_cpu.py.

    verify(commitments, cell_indices, cells, proofs, random_bytes=None) -> Result(status, r, LL, RL, verdict)

status: the cttEthKzg value; r, LL and RL (compressed G1) are None unless the input passed every check; verdict True / False / None.
"""
import collections
import functools
import hashlib
import json
import os

from oracle import pyoracle as po
from tests import _golden, _nttref, _pairingref as pr

R = po.BLS12_381_G1.order
P = po.BLS12_381_G1.F.p
G1 = po.BLS12_381_G1
CELLS, CELL_ELEMS, CELL_BYTES, N_BLOB = 128, 64, 2048, 4096
W8192 = pow(7, (R - 1) // 8192, R)
W64 = pow(W8192, 128, R)
DOMAIN = b"RCKZGCBATCH__V1_"
SUCCESS, VERIFICATION_FAILURE, LENGTHS_MISMATCH, SCALAR_TOO_LARGE = 0, 1, 2, 4
ECC_INVALID_ENCODING, ECC_COORDINATE_TOO_LARGE, ECC_NOT_ON_CURVE, ECC_NOT_IN_SUBGROUP = 5, 6, 7, 8

Result = collections.namedtuple("Result", "status r LL RL verdict")


# ---- G1 in Jacobian coordinates (the affine law of oracle.pyoracle inverts at every step: too slow for 900 points) --------------
def _jdbl(T):
    X, Y, Z = T
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    A, B = X * X % P, Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) * (X + B) - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return (X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P)


def _jadd(T, U):
    if T[2] == 0:
        return U
    if U[2] == 0:
        return T
    Z1Z1, Z2Z2 = T[2] * T[2] % P, U[2] * U[2] % P
    U1, U2 = T[0] * Z2Z2 % P, U[0] * Z1Z1 % P
    S1, S2 = T[1] * U[2] * Z2Z2 % P, U[1] * T[2] * Z1Z1 % P
    if U1 == U2:
        return _jdbl(T) if S1 == S2 else (1, 1, 0)
    H, Rr = (U2 - U1) % P, (S2 - S1) % P
    HH = H * H % P
    HHH, V = H * HH % P, U1 * HH % P
    X3 = (Rr * Rr - HHH - 2 * V) % P
    return (X3, (Rr * (V - X3) - S1 * HHH) % P, T[2] * U[2] * H % P)


def _jac(Pt):
    return (1, 1, 0) if Pt is None else (Pt[0], Pt[1], 1)


def _aff(T):
    if T[2] == 0:
        return None
    zi = pow(T[2], -1, P)
    return (T[0] * zi * zi % P, T[1] * zi * zi * zi % P)


def g1_msm(scalars, points, c=8):
    """buckets of c bits, unsigned digits"""
    total = (1, 1, 0)
    for w in range((255 + c - 1) // c - 1, -1, -1):
        for _ in range(c):
            total = _jdbl(total)
        buckets = [(1, 1, 0)] * (1 << c)
        for k, Pt in zip(scalars, points):
            d = ((k % R) >> (w * c)) & ((1 << c) - 1)
            if d and Pt is not None:
                buckets[d] = _jadd(buckets[d], _jac(Pt))
        run = acc = (1, 1, 0)
        for d in range((1 << c) - 1, 0, -1):
            run = _jadd(run, buckets[d])
            acc = _jadd(acc, run)
        total = _jadd(total, acc)
    return _aff(total)


@functools.lru_cache(maxsize=None)
def g1_in_subgroup(Pt):
    return Pt is None or g1_mul(R, Pt) is None


def g1_mul(k, Pt):
    acc, T = (1, 1, 0), _jac(Pt)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd(acc, T)
    return _aff(acc)


def decompress_g1(b48):
    """-> (status, point) without the subgroup check: what one lane of k_vf_decompress decides"""
    b48 = bytes(b48)
    if not b48[0] & 0x80:
        return ECC_INVALID_ENCODING, None
    if b48[0] & 0x40:
        if b48[0] & 0x3f or any(b48[1:]):
            return ECC_INVALID_ENCODING, None
        return SUCCESS, None
    x = int.from_bytes(b48, "big") & ((1 << 381) - 1)
    if x >= P:
        return ECC_COORDINATE_TOO_LARGE, None
    y2 = (pow(x, 3, P) + 4) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return ECC_NOT_ON_CURVE, None
    if bool(b48[0] & 0x20) != (y > (P - 1) // 2):
        y = P - y
    return SUCCESS, (x, y)


@functools.lru_cache(maxsize=None)
def deserialize_g1(b48):
    """-> (status, point): encoding, x < p, on the curve, in the subgroup -- deserialize_g1_compressed; the neutral is accepted"""
    st, pt = decompress_g1(b48)
    if st == SUCCESS and not g1_in_subgroup(pt):
        return ECC_NOT_IN_SUBGROUP, None
    return st, pt


def first_point_outside_the_subgroup():
    """the compressed form of the on-curve point with the smallest x that is not in G1 (the cofactor is not 1: almost every point)"""
    x = 0
    while True:
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80
        st, pt = decompress_g1(bytes(b))
        if st == SUCCESS and not g1_in_subgroup(pt):
            return bytes(b)
        x += 1


def first_x_off_the_curve():
    x = 0
    while decompress_g1(bytes([0x80]) + x.to_bytes(47, "big"))[0] != ECC_NOT_ON_CURVE:
        x += 1
    return bytes([0x80]) + x.to_bytes(47, "big")


# ---- the verifier's part of the trusted setup ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup():
    """-> ([tau^i]_1 for i < 64, [tau^64]_2) from tests/golden/kzg4844_srs_verify.bin"""
    raw = srs_bytes()
    return [_golden.g1_decompress(raw[48 * i:48 * i + 48]) for i in range(64)], pr.g2_decompress(raw[64 * 48:])


def srs_bytes():
    return open(os.path.join(_golden.HERE, "kzg4844_srs_verify.bin"), "rb").read()


# ---- the protocol ----------------------------------------------------------------------------------------------------------------
def coset_shift(j):
    """h_j: cell j holds the values on h_j * <omega_64>, element e at h_j * omega_64^brp6(e)"""
    return pow(W8192, _nttref.brp(j, 7), R)


def challenge(commitments, commitment_indices, cell_indices, cells, proofs):
    """compute_verify_cell_kzg_proof_batch_challenge over the deduplicated commitments"""
    h = hashlib.sha256()
    h.update(DOMAIN + N_BLOB.to_bytes(8, "big") + CELL_ELEMS.to_bytes(8, "big") + len(commitments).to_bytes(8, "big") +
             len(cell_indices).to_bytes(8, "big"))
    for c in commitments:
        h.update(c)
    for k in range(len(cell_indices)):
        h.update(commitment_indices[k].to_bytes(8, "big") + cell_indices[k].to_bytes(8, "big") + cells[k] + proofs[k])
    return int.from_bytes(h.digest(), "big") % R


@functools.lru_cache(maxsize=None)
def interpolation_coefficients(cell_index, cell):
    """the 64 coefficients of I(X), deg < 64, with I(h omega_64^brp6(e)) = cell[e]: Lagrange interpolation over the roots x_e of
    X^64 - h^64, whose basis polynomials are (X^64 - h^64)/(X - x_e) * x_e / (64 h^64) = sum_i x_e^(64 - i) X^i / (64 h^64)"""
    h = coset_shift(cell_index)
    scale = pow(64 * pow(h, 64, R), -1, R)
    coef = [0] * CELL_ELEMS
    for e in range(CELL_ELEMS):
        v = int.from_bytes(cell[32 * e:32 * e + 32], "big") * scale % R
        x = h * pow(W64, _nttref.brp(e, 6), R) % R
        xinv = pow(x, -1, R)
        t = v * pow(x, 64, R) % R
        for i in range(CELL_ELEMS):
            coef[i] = (coef[i] + t) % R
            t = t * xinv % R
    return tuple(coef)


def dedup(commitments):
    unique, index = [], []
    for c in commitments:
        if c not in unique:
            unique.append(c)
        index.append(unique.index(c))
    return unique, index


def blinding(random_bytes):
    """getBatchBlindingFactor: None means: use the Fiat-Shamir challenge"""
    if random_bytes is None or not any(random_bytes):
        return None
    return int.from_bytes(random_bytes, "big") % R or None


def verify(commitments, cell_indices, cells, proofs, random_bytes=None, pairing=True):
    n = len(cell_indices)
    if not (len(commitments) == len(cells) == len(proofs) == n):
        return Result(LENGTHS_MISMATCH, None, None, None, None)
    if n == 0:
        return Result(SUCCESS, None, None, None, True)
    if any(i >= CELLS for i in cell_indices):
        return Result(LENGTHS_MISMATCH, None, None, None, None)
    if any(len(c) != 48 for c in commitments) or any(len(c) != CELL_BYTES for c in cells) or any(len(p) != 48 for p in proofs):
        return Result(LENGTHS_MISMATCH, None, None, None, None)    # (a C caller cannot express these; the wrapper raises ValueError)
    unique, cidx = dedup([bytes(c) for c in commitments])
    C = []
    for c in unique:
        st, pt = deserialize_g1(c)
        if st != SUCCESS:
            return Result(st, None, None, None, None)
        C.append(pt)
    for c in cells:
        if any(int.from_bytes(c[32 * e:32 * e + 32], "big") >= R for e in range(CELL_ELEMS)):
            return Result(SCALAR_TOO_LARGE, None, None, None, None)
    Pi = []
    for p in proofs:
        st, pt = deserialize_g1(bytes(p))
        if st != SUCCESS:
            return Result(st, None, None, None, None)
        Pi.append(pt)
    r = blinding(random_bytes)
    if r is None:
        r = challenge(unique, cidx, cell_indices, [bytes(c) for c in cells], [bytes(p) for p in proofs])
    rho = [pow(r, k + 1, R) for k in range(n)]
    tau, tau64_g2 = setup()
    LL = g1_msm(rho, Pi)
    w = [0] * len(unique)
    coef = [0] * CELL_ELEMS
    for k in range(n):
        w[cidx[k]] = (w[cidx[k]] + rho[k]) % R
        ik = interpolation_coefficients(cell_indices[k], bytes(cells[k]))
        coef = [(a + rho[k] * b) % R for a, b in zip(coef, ik)]
    rlp = [rho[k] * pow(coset_shift(cell_indices[k]), 64, R) % R for k in range(n)]
    RL = g1_msm(w + [(-c) % R for c in coef] + rlp, C + tau + Pi)
    verdict = None
    if pairing:
        verdict = pr.pairing_check([(LL, tau64_g2), (G1.neg(RL), po.BLS12_381_G2.gen)])
    return Result(SUCCESS if verdict in (True, None) else VERIFICATION_FAILURE, r, _golden.g1_compress(LL), _golden.g1_compress(RL), verdict)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _doc():
    return json.load(open(os.path.join(_golden.HERE, "peerdas_verify.json")))


@functools.lru_cache(maxsize=None)
def golden_blobs():
    """-> [(blob name, commitment, [128 cells], [128 proofs])] for the 7 blobs of the PeerDAS fixtures, in fixture order"""
    from tests import _recoverref as rr
    raw = {name: (blob, com) for name, blob, com in _golden.kzg4844_raw_cases()}
    proofs = {ref: [bytes.fromhex(p) for p in pf]
              for _c, ref, dig, pf in json.load(open(os.path.join(_golden.HERE, "peerdas_cells_and_proofs.json"))) if dig is not None}
    return [(name, raw[name][1], rr.extended_cells(raw[name][0]), proofs[name]) for name in _doc()["blobs"]]


def _cell(c):
    import base64
    import zlib
    if isinstance(c, int):
        return golden_blobs()[c // CELLS][2][c % CELLS]
    return zlib.decompress(base64.b64decode(c))


def _com(c):
    return golden_blobs()[c][1] if isinstance(c, int) else bytes.fromhex(c)


def _proof(p):
    return golden_blobs()[p // CELLS][3][p % CELLS] if isinstance(p, int) else bytes.fromhex(p)


def verify_cases():
    """-> [(case, [commitment], [cell index], [cell], [proof], True | False | None)]"""
    return [(name, [_com(c) for c in coms], idx, [_cell(c) for c in cells], [_proof(p) for p in proofs], want)
            for name, coms, idx, cells, proofs, want in _doc()["verify"]]


def challenge_cases():
    """-> [(case, [commitment], [commitment index], [cell index], [cell], [proof], challenge)]"""
    return [(name, [_com(c) for c in coms], cidx, idx, [_cell(c) for c in cells], [_proof(p) for p in proofs], int(want, 16))
            for name, coms, cidx, idx, cells, proofs, want in _doc()["challenge"]]


def batch(blob_ids, cell_ids=range(CELLS)):
    """the cells `cell_ids` of the golden blobs `blob_ids`, blob after blob -> (commitments, cell_indices, cells, proofs)"""
    coms, idx, cells, proofs = [], [], [], []
    for b in blob_ids:
        _name, com, cs, ps = golden_blobs()[b]
        for j in cell_ids:
            coms.append(com)
            idx.append(j)
            cells.append(cs[j])
            proofs.append(ps[j])
    return coms, idx, cells, proofs
