"""EIP-7594 batch verification on the CPU: tests/verify_harness.cpp runs the host logic and the three kernel bodies of
constantine_amd/csrc/verify_host.h lane by lane, the transform of 64 points between them on the bodies of ntt_bodies.h, and the host
pairing of pairing_host.h; everything is compared for equality with Python integers -- tests/_verifyref.py (the spec's equation with
Lagrange interpolation per cell, pinned here to the reference's 42 vectors) and tests/_pairingref.py (Fp12 as polynomials, the final
exponentiation as one pow)."""
import functools
import os
import random
import shutil
import struct
import subprocess

import pytest

from oracle import pyoracle as po
from tests import _pairingref as pr, _verifyref as vr

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")
R, P = vr.R, vr.P
G1, G2 = po.BLS12_381_G1, po.BLS12_381_G2
NEUTRAL = bytes([0xC0]) + bytes(47)
VERIFY_CASES = vr.verify_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_path_factory.mktemp("verify")), "verify_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "verify_harness.cpp"), "-o", exe], check=True)

    def run(cmd, data=b""):
        return subprocess.run([exe, cmd], input=data, check=True, capture_output=True).stdout
    return run


@functools.lru_cache(maxsize=None)
def reference(i, pairing=True):
    _name, coms, idx, cells, proofs, _want = VERIFY_CASES[i]
    return vr.verify(coms, idx, cells, proofs, pairing=pairing)


# ---- the Python reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(VERIFY_CASES)), ids=[c[0] for c in VERIFY_CASES])
def test_python_reference_is_pinned_to_the_verify_vectors(i):
    want = VERIFY_CASES[i][5]
    res = reference(i)
    assert res.verdict is want
    assert (res.status == vr.SUCCESS) == (want is True) and (res.status == vr.VERIFICATION_FAILURE) == (want is False)


@pytest.mark.parametrize("case", vr.challenge_cases(), ids=lambda c: c[0])
def test_challenge_vectors(harness, case):
    _name, coms, cidx, idx, cells, proofs, want = case
    assert vr.challenge(coms, cidx, idx, cells, proofs) == want
    data = struct.pack("<2I", len(coms), len(idx)) + b"".join(coms) + struct.pack("<%dQ" % len(idx), *cidx)
    data += struct.pack("<%dQ" % len(idx), *idx) + b"".join(cells) + b"".join(proofs)
    assert int.from_bytes(harness("challenge", data), "big") == want


# ---- the decompress body -----------------------------------------------------------------------------------------------------------
def _decompress(harness, points, split=None, gap=0, subgroup=False):
    n = len(points)
    split = n if split is None else split
    out = harness("decompress", struct.pack("<4I", n, split, gap, int(subgroup)) + b"".join(points))
    assert len(out) == 4 * n + 96 * (n + gap) + n
    status = list(struct.unpack("<%dI" % n, out[:4 * n]))
    recs = [out[4 * n + 96 * i:4 * n + 96 * (i + 1)] for i in range(n + gap)]
    return status, recs, list(out[-n:])


def test_decompress_golden_points_across_a_gap(harness):
    """the 7 commitments and 7 x 128 proofs of the fixtures in the layout of a call: lane i < 7 -> record i, lane 7 + k -> record
    7 + 64 + k; the 64 records between are not touched"""
    blobs = vr.golden_blobs()
    points = [b[1] for b in blobs] + [p for b in blobs for p in b[3]]
    status, recs, _ = _decompress(harness, points, split=7, gap=64)
    assert status == [0] * len(points)
    assert recs[7:71] == [b"\xab" * 96] * 64
    for i, pt in enumerate(points):
        st, want = vr.decompress_g1(pt)
        assert st == 0 and G1.aff_from_bytes(recs[i + (64 if i >= 7 else 0)]) == want, i


def _with_x(x, flags):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def test_decompress_edge_encodings(harness):
    x = vr.decompress_g1(vr.golden_blobs()[1][1])[1][0]
    points = [
        NEUTRAL, _with_x(x, 0x80), _with_x(x, 0xA0),                                   # the neutral, both signs of one x
        _with_x(P - 1, 0x80), _with_x(P, 0x80), _with_x(P + 5, 0xA0),                  # x = p - 1, x = p, x >= p with the sign flag
        _with_x((1 << 381) - 1, 0x80),                                                 # every bit below the flags
        bytes([0xC0]) + bytes(46) + b"\x01", bytes([0xE0]) + bytes(47),                # infinity with a stray bit, with the sign flag
        _with_x(x, 0x00), _with_x(x, 0x20), bytes(48),                                 # the compression flag clear
        vr.first_x_off_the_curve(), vr.first_point_outside_the_subgroup(),
    ]
    status, recs, sub = _decompress(harness, points, subgroup=True)
    for i, pt in enumerate(points):
        st, want = vr.decompress_g1(pt)
        assert status[i] == st, (i, pt.hex())
        assert G1.aff_from_bytes(recs[i]) == want and (st == 0 or recs[i] == bytes(96)), i
    assert status[:3] == [0, 0, 0] and recs[0] == bytes(96)
    a, b = G1.aff_from_bytes(recs[1]), G1.aff_from_bytes(recs[2])
    assert a == G1.neg(b) and a[1] <= (P - 1) // 2 < b[1]
    assert status[4:9] == [vr.ECC_COORDINATE_TOO_LARGE] * 3 + [vr.ECC_INVALID_ENCODING] * 2
    assert status[9:12] == [vr.ECC_INVALID_ENCODING] * 3 and status[12] == vr.ECC_NOT_ON_CURVE
    # a point of the curve outside G1: the decompress body accepts it, the subgroup check refuses it
    assert status[13] == 0 and sub[13] == 0 and G1.is_on_curve(G1.aff_from_bytes(recs[13]))
    assert sub[:3] == [1, 1, 1] and vr.deserialize_g1(points[13])[0] == vr.ECC_NOT_IN_SUBGROUP


# ---- the colsum and interp bodies around the transform -----------------------------------------------------------------------------
def _colsum(harness, r, idx, cells):
    n = len(idx)
    out = harness("colsum", struct.pack("<I", n) + r.to_bytes(32, "little") + struct.pack("<%dQ" % n, *idx) + b"".join(cells))
    assert len(out) == 4 * n + 64 * 32
    bad = list(struct.unpack("<%dI" % n, out[:4 * n]))
    return bad, [int.from_bytes(out[4 * n + 32 * i:4 * n + 32 * i + 32], "little") for i in range(64)]


def _lagrange_sum(r, idx, cells):
    coef = [0] * 64
    for k, (j, c) in enumerate(zip(idx, cells)):
        ik = vr.interpolation_coefficients(j, c)
        coef = [(a + pow(r, k + 1, R) * b) % R for a, b in zip(coef, ik)]
    return coef


def _edge_cell():
    rng = random.Random("verify-edge-cell")
    vals = [0, 1, R - 1] + [rng.randrange(R) for _ in range(60)] + [R - 1]
    return b"".join(v.to_bytes(32, "big") for v in vals)


def _column_batch():
    """columns with 7 cells (5), 2 cells (9), 1 cell (100 and 127), 3 x the same cell (17), none elsewhere; not sorted"""
    blobs = vr.golden_blobs()
    idx, cells = [], []
    for b in range(7):
        idx.append(5)
        cells.append(blobs[b][2][5])
    for j, b in ((127, 2), (9, 0), (17, 6), (100, 3), (17, 6), (9, 4), (17, 6)):
        idx.append(j)
        cells.append(blobs[b][2][j])
    idx.append(0)
    cells.append(_edge_cell())
    return idx, cells


def test_interpolation_coefficients_match_the_lagrange_sum(harness):
    idx, cells = _column_batch()
    r = random.Random("verify-r").randrange(1, R)
    bad, neg_c = _colsum(harness, r, idx, cells)
    assert bad == [0] * len(idx)
    assert neg_c == [(-c) % R for c in _lagrange_sum(r, idx, cells)]
    bad, neg_c = _colsum(harness, 1, idx[:1], cells[:1])                      # one cell, weight 1: the cell's own interpolant
    assert bad == [0] and neg_c == [(-c) % R for c in vr.interpolation_coefficients(idx[0], cells[0])]


@pytest.mark.parametrize("value", [R, (1 << 256) - 1])
def test_scalar_out_of_range_in_the_last_element_of_the_last_cell(harness, value):
    idx, cells = _column_batch()
    cells[-1] = cells[-1][:-32] + value.to_bytes(32, "big")
    bad, _ = _colsum(harness, 3, idx, cells)
    assert bad == [0] * (len(idx) - 1) + [1]
    cells[-1] = cells[-1][:-32] + (R - 1).to_bytes(32, "big")
    assert _colsum(harness, 3, idx, cells)[0] == [0] * len(idx)


# ---- the checks in the reference's order, and the challenge's two paths --------------------------------------------------------------
def _status(harness, coms, idx, cells, proofs, rnd=None):
    n = len(idx)
    data = struct.pack("<I", n) + (rnd or bytes(32)) + b"".join(coms) + struct.pack("<%dQ" % n, *idx) + b"".join(cells) + b"".join(proofs)
    out = harness("status", data)
    if out[0] != 0 or n == 0:
        assert len(out) == 1
        return out[0], None, None
    return 0, int.from_bytes(out[1:33], "big"), struct.unpack("<I", out[33:37])[0]


@pytest.mark.parametrize("rnd,want", [((1).to_bytes(32, "big"), 1), (R.to_bytes(32, "big"), None), ((R + 1).to_bytes(32, "big"), 1),
                                      (bytes(32), None), (b"\xff" * 32, ((1 << 256) - 1) % R)])
def test_random_bytes_or_fiat_shamir(harness, rnd, want):
    coms, idx, cells, proofs = vr.batch([2, 3], [3, 64])
    ref = vr.verify(coms, idx, cells, proofs, rnd, pairing=False)
    fs = vr.verify(coms, idx, cells, proofs, None, pairing=False).r
    assert ref.r == (fs if want is None else want)
    assert _status(harness, coms, idx, cells, proofs, rnd) == (0, ref.r, 2)


def _offenders():
    """a valid batch of 4 cells of 2 blobs, and for each kind of item a way to spoil item `k`"""
    coms, idx, cells, proofs = vr.batch([2, 3], [7, 120])
    outside = vr.first_point_outside_the_subgroup()
    spoil = {
        "commitment_range": lambda b, k: b[0].__setitem__(k, _with_x(P, 0x80)),
        "commitment_subgroup": lambda b, k: b[0].__setitem__(k, outside),
        "cell": lambda b, k: b[2].__setitem__(k, b[2][k][:-32] + R.to_bytes(32, "big")),
        "proof_curve": lambda b, k: b[3].__setitem__(k, vr.first_x_off_the_curve()),
        "proof_subgroup": lambda b, k: b[3].__setitem__(k, outside),
        "proof_encoding": lambda b, k: b[3].__setitem__(k, bytes(48)),
        "index": lambda b, k: b[1].__setitem__(k, 128),
    }
    return (coms, idx, cells, proofs), spoil


KINDS = ["commitment_range", "commitment_subgroup", "cell", "proof_curve", "proof_subgroup", "proof_encoding"]


@pytest.mark.parametrize("first", KINDS + ["index"])
@pytest.mark.parametrize("second", KINDS + ["index"])
def test_status_of_the_first_offender_in_the_reference_order(harness, first, second):
    """two offenders (one when first == second), the second kind EARLIER in the input than the first: the kind decides, not the place"""
    good, spoil = _offenders()
    b = [list(x) for x in good]
    spoil[first](b, 3)
    spoil[second](b, 0)
    want = vr.verify(*b, pairing=False).status
    assert want != 0 and _status(harness, *b)[0] == want
    if "index" in (first, second):
        assert want == vr.LENGTHS_MISMATCH
    elif first.split("_")[0] != second.split("_")[0]:
        order = {"commitment": 0, "cell": 1, "proof": 2}
        kind = min(first, second, key=lambda s: order[s.split("_")[0]])
        b2 = [list(x) for x in good]
        spoil[kind](b2, 0)
        assert want == vr.verify(*b2, pairing=False).status


def test_valid_batches_pass_every_check(harness):
    good, _ = _offenders()
    ref = vr.verify(*good, pairing=False)
    assert _status(harness, *good) == (0, ref.r, 2)
    assert _status(harness, [], [], [], []) == (0, None, None)
    coms, idx, cells, proofs = good
    assert _status(harness, [NEUTRAL] + coms[1:], idx, cells, [NEUTRAL] + proofs[1:])[0] == 0     # the neutral is accepted


# ---- the pairing -------------------------------------------------------------------------------------------------------------------
def test_frobenius_constants(harness):
    """w^(p^2) = w * xi^((p^2 - 1)/6): each constant against a power of w in Fp[w]/(w^12 - 2 w^6 + 2)"""
    out = harness("frobenius")
    assert len(out) == 5 * 48
    for k in range(1, 6):
        g = int.from_bytes(out[48 * (k - 1):48 * k], "little")
        wk = [0] * 12
        wk[k] = 1
        assert pr.f12_pow(wk, P * P) == [g if i == k else 0 for i in range(12)], k
        assert (g, 0) == _fp2_pow((1, 1), k * (P * P - 1) // 6), k


def _fp2_pow(a, e):
    F2, out = G2.F, (1, 0)
    for bit in bin(e)[2:]:
        out = F2.mul(out, out)
        if bit == "1":
            out = F2.mul(out, a)
    return out


def test_hard_exponent_is_the_cyclotomic_cofactor():
    import re
    text = open(os.path.join(CSRC, "field_params.h")).read()
    limbs = re.search(r"HARD_EXP\[HARD_LIMBS\] = \{([^}]*)\}", text).group(1).split(",")
    hard = sum(int(x.strip().rstrip("ul"), 16) << (64 * i) for i, x in enumerate(limbs))
    assert hard * R == P ** 4 - P ** 2 + 1 and (P ** 6 - 1) * (P ** 2 + 1) * hard == pr.FINAL_EXPONENT


def _g2_bytes(harness, raw):
    out = harness("g2", raw)
    if out[0] != 0:
        return out[0], None
    v = [int.from_bytes(out[1 + 48 * i:49 + 48 * i], "little") for i in range(4)]
    return 0, ((v[0], v[1]), (v[2], v[3]))


def test_g2_decompress(harness):
    raw = vr.srs_bytes()[64 * 48:]
    Q = pr.g2_decompress(raw)
    assert G2.is_on_curve(Q) and G2.scalar_mul(R, Q) is None
    assert _g2_bytes(harness, raw) == (0, Q)
    flipped = bytes([raw[0] ^ 0x20]) + raw[1:]
    assert _g2_bytes(harness, flipped) == (0, G2.neg(Q)) and pr.g2_decompress(flipped) == G2.neg(Q)
    for pt in (G2.gen, G2.neg(G2.gen), G2.double(G2.gen)):
        assert _g2_bytes(harness, pr.g2_compress(pt)) == (0, pt)
    assert _g2_bytes(harness, bytes([0xC0]) + bytes(95)) == (0, ((0, 0), (0, 0)))
    assert _g2_bytes(harness, bytes(96))[0] == vr.ECC_INVALID_ENCODING
    assert _g2_bytes(harness, bytes([0xC0]) + bytes(94) + b"\x01")[0] == vr.ECC_INVALID_ENCODING
    assert _g2_bytes(harness, bytes([0x80]) + bytes(47) + P.to_bytes(48, "big"))[0] == vr.ECC_COORDINATE_TOO_LARGE
    x = 0
    while pr.fp2_sqrt(G2.F.add(G2.F.mul(G2.F.sqr((x, 0)), (x, 0)), G2.b)) is not None:
        x += 1
    assert _g2_bytes(harness, bytes([0x80]) + bytes(47) + x.to_bytes(48, "big"))[0] == vr.ECC_NOT_ON_CURVE


def _gt(harness, pairs):
    data = struct.pack("<I", len(pairs))
    for Pt, Q in pairs:
        for v in (Pt or (0, 0)):
            data += v.to_bytes(48, "little")
        for c in (Q or ((0, 0), (0, 0))):
            for v in c:
                data += v.to_bytes(48, "little")
    out = harness("gt", data)
    assert len(out) == 12 * 48 + 1
    co = [(int.from_bytes(out[96 * k:96 * k + 48], "little"), int.from_bytes(out[96 * k + 48:96 * k + 96], "little")) for k in range(6)]
    return pr.f12_from_tower(co), out[-1]


@functools.lru_cache(maxsize=None)
def _e_g1_g2():
    return tuple(pr.pairing(G1.gen, G2.gen))


@pytest.mark.parametrize("a", [1, 2, R - 1])
@pytest.mark.parametrize("b", [1, 2, R - 1])
def test_pairing_is_bilinear_and_equals_the_integer_pairing(harness, a, b):
    """GT values byte for byte: both sides raise the Miller value to (p^12 - 1)/r, the first power of the pairing"""
    got, one = _gt(harness, [(G1.scalar_mul(a, G1.gen), G2.scalar_mul(b, G2.gen))])
    assert got == pr.f12_pow(list(_e_g1_g2()), a * b % R) and one == 0
    assert got != pr.ONE


def test_pairing_products(harness):
    Pt, Q = G1.scalar_mul(5, G1.gen), G2.scalar_mul(7, G2.gen)
    assert _gt(harness, [(Pt, Q), (G1.neg(Pt), Q)]) == (pr.ONE, 1)
    assert _gt(harness, [(Pt, Q), (Pt, G2.neg(Q))]) == (pr.ONE, 1)
    assert _gt(harness, [(None, Q)]) == (pr.ONE, 1) and _gt(harness, [(Pt, None)]) == (pr.ONE, 1) and _gt(harness, []) == (pr.ONE, 1)
    got, one = _gt(harness, [(G1.gen, G2.gen), (G1.gen, G2.gen)])
    assert one == 0 and got == pr.f12_pow(list(_e_g1_g2()), 2)
    assert pr.pairing_check([(Pt, Q), (G1.neg(Pt), Q)]) and not pr.pairing_check([(G1.gen, G2.gen), (G1.gen, G2.gen)])


DECIDED = [i for i, c in enumerate(VERIFY_CASES) if c[5] is not None and c[2]]


@pytest.mark.parametrize("i", DECIDED, ids=[VERIFY_CASES[i][0] for i in DECIDED])
def test_verdicts_end_to_end_on_the_host(harness, i):
    """LL and RL from Python, the pairing check of the library's host code: the verdicts of the true / false vectors"""
    res = reference(i)
    out = harness("verdict", res.LL + res.RL + vr.srs_bytes()[64 * 48:])
    assert out == bytes([0 if VERIFY_CASES[i][5] else 1])
