"""The bodies of the scalar-field NTT (constantine_amd/csrc/ntt_bodies.h) on the CPU: tests/ntt_harness.cpp runs them pass by pass,
tile by tile and lane by lane, and every output is compared for equality with the Python integers of tests/_nttref.py -- the five
scalar fields, every order and format flag, the coset shift, in place, tile sizes that take one, two and three passes.  The pass
planner (ntt_plan.h) is checked against its brute-force statement: every index bit is covered exactly once."""
import os
import shutil
import struct
import subprocess

import pytest

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
