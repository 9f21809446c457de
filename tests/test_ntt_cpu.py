"""The bodies of the scalar-field NTT (constantine_amd/csrc/ntt_bodies.h) on the CPU: tests/ntt_harness.cpp runs them pass by pass,
tile by tile and lane by lane, and every output is compared for equality with the Python integers of tests/_nttref.py -- the five
scalar fields, every order and format flag, the coset shift, in place, tile sizes that take one, two and three passes.  The pass
planner (ntt_plan.h) is checked against its brute-force statement: every index bit is covered exactly once.  Above n = 4096 the same
comparison runs up to 2^17 (tests/_nttref.large_cases), and 2^18 is compared through the structured references of tests/_nttlarge.py,
which are themselves compared with the full reference at 2^13."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _nttlarge as big
from tests import _nttref as ref

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_path_factory.mktemp("ntt")), "ntt_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "ntt_harness.cpp"), "-o", exe], check=True)

    def run(*args, data=b""):
        return subprocess.run([exe, *args], input=data, check=True, capture_output=True).stdout
    return run


def _run(harness, field, lg, tile, batch, flags, omega, shift, stored, in_place, lanes=256):
    head = struct.pack("<8I", ref.FIELDS[field][0], lg, tile or ref.DEFAULT_TILE_LOG2, batch, flags, 0 if shift is None else 1,
                       1 if in_place else 0, lanes)
    out = harness("ntt", data=head + ref.to_bytes([omega, shift or 0]) + ref.to_bytes(stored))
    return ref.from_bytes(out)


@pytest.mark.parametrize("field", list(ref.FIELDS))
def test_bodies_match_python(harness, field):
    for case in ref.cases(field):
        name, lg, tile, batch, flags, _sk, in_place = case
        omega, shift, stored, want = ref.case_data(field, case)
        got = _run(harness, field, lg, tile, batch, flags, omega, shift, stored, in_place)
        assert got == want, (field, name)


@pytest.mark.parametrize("field", list(ref.FIELDS))
def test_round_trip(harness, field):
    """inverse(forward(x, g), g) = x, through both orders and both formats"""
    p = ref.FIELDS[field][2]
    lg = min(7, ref.two_adicity(p))
    n = 1 << lg
    omega, g = ref.root_of_unity(p, lg), 0x1234567 % p
    x = ref.stored_inputs(p, 2 * n, "rt" + field)
    for fwd, inv in ((ref.OUT_BRP | ref.OUT_MONT, ref.INVERSE | ref.IN_BRP | ref.IN_MONT), (0, ref.INVERSE),
                     (ref.IN_BRP | ref.OUT_BRP, ref.INVERSE | ref.IN_BRP | ref.OUT_BRP)):
        y = _run(harness, field, lg, 3, 2, fwd, omega, g, x, False)
        assert _run(harness, field, lg, 3, 2, inv, omega, g, y, True) == x, (field, fwd, inv)


def test_lane_count_does_not_matter(harness):
    """the phases share their work among however many lanes there are: 1, 7 and 64 lanes give what 256 give"""
    field = "bls12_381_fr"
    case = ("lanes", 7, 3, 2, ref.OUT_BRP, "rand", False)
    omega, shift, stored, want = ref.case_data(field, case)
    for lanes in (1, 7, 64):
        assert _run(harness, field, 7, 3, 2, ref.OUT_BRP, omega, shift, stored, False, lanes) == want, lanes


def test_planner_covers_every_bit_once(harness):
    for lg in range(1, 25):
        for tile in range(1, 10):
            for dit in (0, 1):
                rows = [tuple(map(int, ln.split())) for ln in harness("plan", str(lg), str(tile), str(dit)).decode().splitlines()]
                assert len(rows) == -(-lg // tile), (lg, tile, dit)
                covered = []
                for lo, t, x, nrows, E, sl in rows:
                    assert 1 <= t <= tile and E == x + nrows and E <= min(tile + 2, lg), (lg, tile, dit)
                    # the image holds the pass's stage bits: local bits sl .. sl + t - 1 are index bits lo .. lo + t - 1
                    assert (sl, nrows >= t, x) == ((0, True, 0) if lo == 0 else (x, True, min(2, lo))), (lg, tile, dit)
                    covered += list(range(lo, lo + t))
                if dit:       # DIT: from bit 0 up
                    assert covered == list(range(lg)), (lg, tile, dit)
                assert sorted(covered) == list(range(lg)), (lg, tile, dit)
                if not dit:   # DIF: from the top bit down, pass by pass
                    assert [r[0] + r[1] for r in rows] == sorted((r[0] + r[1] for r in rows), reverse=True)


# ---- above n = 4096: the width of the index arithmetic (tests/_nttref.large_cases, tests/_nttlarge.py) ---------------------------
@pytest.mark.parametrize("field", [f for f in ref.FIELDS if ref.large_cases(f)])
def test_large_bodies_match_python(harness, field):
    """2^13 .. 2^17 against the full reference: twiddle exponents and power tables past 12 bits, many tile bits, three default passes"""
    for case in ref.large_cases(field):
        name, lg, tile, batch, flags, _sk, in_place = case
        omega, shift, stored, want = ref.large_case_data(field, case)
        got = _run(harness, field, lg, tile, batch, flags, omega, shift, stored, in_place)
        assert got == want, (field, name)


A_VARIANTS = ((0, True), (ref.OUT_BRP, False), (ref.IN_BRP, True), (ref.INVERSE, True), (ref.INVERSE | ref.IN_BRP | ref.OUT_BRP, False),
              (ref.INVERSE | ref.IN_BRP, True))                               # (flags, with a shift) of the sparse reference
B_VARIANTS = ((0, False), (ref.OUT_BRP, True), (ref.IN_BRP, True), (ref.INVERSE, False), (ref.INVERSE | ref.IN_BRP, False),
              (ref.INVERSE | ref.OUT_BRP, False))                             # of the strided one (an inverse takes no shift)
C_VARIANTS = (0, ref.OUT_BRP, ref.IN_BRP, ref.INVERSE, ref.INVERSE | ref.IN_BRP, ref.INVERSE | ref.OUT_BRP)


def _full(field, lg, flags, shift, x):
    p = ref.FIELDS[field][2]
    return ref.ntt(x, p, ref.root_of_unity(p, lg), bool(flags & ref.INVERSE), bool(flags & ref.IN_BRP), bool(flags & ref.OUT_BRP), shift)


@pytest.mark.parametrize("field", ["bls12_381_fr", "pallas_fr"])
def test_structured_references_are_the_transform(field):
    """the three identities of tests/_nttlarge.py against the full reference at 2^13, in every order and direction they are used in"""
    p = ref.FIELDS[field][2]
    lg, n = 13, 1 << 13
    omega, g = ref.root_of_unity(p, lg), random.Random("id" + field).randrange(2, p)
    for flags, shifted in A_VARIANTS:
        shift = g if shifted else None
        pos_in, val, pos_out, want = big.sparse(p, omega, lg, flags, shift, "id", samples=300)
        x = [0] * n
        for i, v in zip(pos_in, val):
            x[i] = v
        full = _full(field, lg, flags, shift, x)
        assert [full[k] for k in pos_out] == want, ("sparse", flags)
    for flags, shifted in B_VARIANTS:
        shift = g if shifted else None
        pos_in, y, tile, (oshape, tshape) = big.strided(p, omega, lg, flags, shift, "id")
        x = [0] * n
        for i, v in zip(pos_in, y):
            x[i] = v
        full = np.frombuffer(ref.to_bytes(_full(field, lg, flags, shift, x)), dtype=np.uint8)
        assert (full.reshape(oshape) == np.frombuffer(ref.to_bytes(tile), dtype=np.uint8).reshape(tshape)).all(), ("strided", flags)
    xb = big.dense_bytes(lg, 13)
    x = ref.from_bytes(xb.tobytes())
    for flags in C_VARIANTS:
        pos_out, want = big.dense(big.fold(xb, p, lg, bool(flags & ref.IN_BRP)), p, omega, lg, flags)
        full = _full(field, lg, flags, None, x)
        assert [full[k] for k in pos_out] == want, ("dense", flags)


def _run_bytes(harness, field, lg, tile, flags, omega, shift, x):
    """one row of n * 32 bytes (numpy uint8) through the harness -> (n, 32) uint8"""
    head = struct.pack("<8I", ref.FIELDS[field][0], lg, tile or ref.DEFAULT_TILE_LOG2, 1, flags, 0 if shift is None else 1, 0, 256)
    out = harness("ntt", data=head + ref.to_bytes([omega, shift or 0]) + x.tobytes())
    return np.frombuffer(out, dtype=np.uint8).reshape(1 << lg, 32)


def _words(rows):
    return ref.from_bytes(np.ascontiguousarray(rows).tobytes())


def test_structured_2p18(harness):
    """2^18, past the recursive reference: sampled outputs of a sparse input, every output of a strided one, 4096 outputs of a dense one"""
    field, lg = "bls12_381_fr", 18
    p = ref.FIELDS[field][2]
    n = 1 << lg
    omega, g = ref.root_of_unity(p, lg), random.Random("2p18").randrange(2, p)
    for flags, shifted in ((ref.OUT_BRP, True), (ref.INVERSE | ref.IN_BRP, True), (0, False)):
        shift = g if shifted else None
        pos_in, val, pos_out, want = big.sparse(p, omega, lg, flags, shift, lg)
        x = np.zeros((n, 32), dtype=np.uint8)
        x[pos_in] = np.frombuffer(ref.to_bytes(val), dtype=np.uint8).reshape(-1, 32)
        got = _run_bytes(harness, field, lg, 0, flags, omega, shift, x)
        assert _words(got[pos_out]) == want, ("sparse", flags)
    for flags, shifted in ((0, False), (ref.OUT_BRP, True), (ref.INVERSE | ref.IN_BRP, False)):
        shift = g if shifted else None
        pos_in, y, tile, (oshape, tshape) = big.strided(p, omega, lg, flags, shift, lg)
        x = np.zeros((n, 32), dtype=np.uint8)
        x[pos_in] = np.frombuffer(ref.to_bytes(y), dtype=np.uint8).reshape(-1, 32)
        got = _run_bytes(harness, field, lg, 0, flags, omega, shift, x)
        assert (got.reshape(oshape) == np.frombuffer(ref.to_bytes(tile), dtype=np.uint8).reshape(tshape)).all(), ("strided", flags)
    xb = big.dense_bytes(lg, lg)
    for flags in (ref.OUT_BRP, ref.INVERSE | ref.IN_BRP):
        pos_out, want = big.dense(big.fold(xb, p, lg, bool(flags & ref.IN_BRP)), p, omega, lg, flags)
        got = _run_bytes(harness, field, lg, 0, flags, omega, None, xb)
        assert _words(got[pos_out]) == want, ("dense", flags)
