"""The bodies of the batched fixed-base G1 MSM (csrc/fixed_bodies.h) run lane by lane on the CPU through tests/fixed_harness.cpp, the
way the kernels of csrc/fixed.hip run them: table lanes, lane sums, the tree over a plain array, the chunk partials and the finish.
Every comparison is byte equality of affine Montgomery coordinates with an independent CPU result (tests/_fixedref.py).  No GPU, no
library.  The harness is also the sanitizer target, built by hand with -fsanitize=address,undefined and fed the same inputs."""
import struct

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import _fixedref as fx


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fx.build_harness(tmp_path_factory.mktemp("fixed_harness"))


@pytest.mark.parametrize("c", [3, 5, 6])
def test_t1_every_record_of_the_table(harness, c):
    """BLS12-381 G1, n = 3, one base the neutral: 3 and 5 divide 255 (the extra window exists), 6 does not.  Every record equals
    j * 2^off * P from Python integers; the neutral base's records are (0, 0)."""
    name = "bls12_381_g1"
    curve = po.CURVES[name]
    pts = cref.gen_points(name, 20, 3)
    pts[1] = 0
    lay = fx.layout(255, c)
    assert len(lay) == -(-255 // c) + (1 if 255 % c == 0 else 0)
    rows = sum(1 << (width - 1) for _, width in lay)
    out = harness("table", fx.harness_table_input(name, pts, c))
    W, got_rows = struct.unpack("<2I", out[:8])
    assert (W, got_rows) == (len(lay), rows)
    want = fx.table_bytes(name, [curve.aff_from_bytes(bytes(p)) for p in pts], c)
    assert len(want) == 3 * rows * 96 and want[rows * 96:2 * rows * 96] == bytes(rows * 96)
    assert out[8:] == want


@pytest.mark.parametrize("tag", fx.MSM_CASES)
def test_msm_cases_through_the_bodies(harness, tag):
    """T2 scalar edges, T3 chunk edge, T4 collisions (the doubling branch at every tree level, a neutral sum, an all-zero row), T5
    neutral and opposite bases, T7 BN254 G1, T8 / T8bn the scalar edges and a largest digit in the lowest, a middle and the top window
    at c = 7, 9, 10, 11, 12 (and 2 on 255 bits) against Python integers"""
    case = fx.case(tag)
    for c in case.cs:
        out = harness("msm", fx.harness_msm_input(case.name, case.pts, case.coefs, c))
        got = np.frombuffer(out, dtype=np.uint8).reshape(case.expect.shape)
        for k in range(len(got)):
            assert bytes(got[k]) == bytes(case.expect[k]), (tag, c, k)


# records of one base, from the layout by hand: BITS + 1 bits in ceil((BITS + 1) / c) windows, the first (BITS + 1) mod W one bit wider
A2_TABLES = [("bls12_381_g1", 2, 3, 128 * 2),                  # 256 bits: 128 windows of 2
             ("bls12_381_g1", 7, 3, 34 * 64 + 3 * 32),         # 37 windows: 34 of 7 bits, 3 of 6
             ("bls12_381_g1", 12, 2, 14 * 2048 + 8 * 1024),    # 22 windows: 14 of 12 bits, 8 of 11 -> 36864
             ("bn254_snarks_g1", 2, 3, 127 * 2 + 1),           # 255 bits: 127 windows of 2 and one of 1, a window of one record
             ("bn254_snarks_g1", 8, 3, 31 * 128 + 64),         # 32 windows: 31 of 8 bits, one of 7
             ("bn254_snarks_g1", 12, 2, 13 * 2048 + 9 * 1024)]  # 22 windows: 13 of 12 bits, 9 of 11 -> 35840


@pytest.mark.parametrize("name,c,n,rows", A2_TABLES, ids=[f"{t[0]}-c{t[1]}" for t in A2_TABLES])
def test_every_record_at_the_smallest_and_the_largest_windows(harness, name, c, n, rows):
    """T1's comparison at the window sizes no other table has: c = 2 (on 254 bits with a window of one record), 7 / 8, and the
    maximum 12, whose lanes invert a prefix product over 2048 records; BN254's table record by record.  Base 1 is the neutral."""
    curve = po.CURVES[name]
    assert (14 * 2048 + 8 * 1024, 13 * 2048 + 9 * 1024) == (36864, 35840)
    assert fx.rows_per_base(fx.BITS[name], c) == rows
    pts = cref.gen_points(name, 26, n)
    pts[1] = 0
    out = harness("table", fx.harness_table_input(name, pts, c))
    assert struct.unpack("<2I", out[:8]) == (len(fx.layout(fx.BITS[name], c)), rows)
    want = fx.table_bytes(name, [curve.aff_from_bytes(bytes(p)) for p in pts], c)
    rec = curve.aff_bytes
    assert len(want) == n * rows * rec and want[rows * rec:2 * rows * rec] == bytes(rows * rec)
    assert out[8:] == want


@pytest.mark.parametrize("name", ["bls12_381_g1", "bn254_snarks_g1"])
@pytest.mark.parametrize("chunks", fx.FINISH_CHUNKS)
def test_finish_up_to_256_partials(harness, name, chunks):
    """the finish alone (fx_finish_lane_sum's strides, the tree over 4 x 64 lanes, fx_finish_group) over partials k * G from Python,
    each with a z of its own: m = 6, so the second workgroup has two waves without a row; the rows of _fixedref.FINISH_ROWS"""
    part, expect = fx.finish_case(name, chunks)
    out = harness("finish", fx.harness_finish_input(name, part))
    got = np.frombuffer(out, dtype=np.uint8).reshape(expect.shape)
    for k, what in enumerate(fx.FINISH_ROWS):
        assert bytes(got[k]) == bytes(expect[k]), (chunks, what)


@pytest.mark.parametrize("tag", ["T8", "T8bn"])
def test_t8_montgomery_coefficients_on_both_curves(harness, tag):
    """the `fr` form of T8 at c = 12 and at the case's smallest c: Fr::from_mont of BN254 as well"""
    case = fx.case(tag)
    for c in (case.cs[0], 12):
        out = harness("msm", fx.harness_msm_input(case.name, case.pts, case.coefs_fr, c, fr=True))
        assert out == case.expect.tobytes(), (tag, c)


def test_t6_montgomery_coefficients_give_the_same_bytes(harness):
    """the `fr` form of T3: Montgomery residues of the scalars mod r"""
    case = fx.case("T3")
    out = harness("msm", fx.harness_msm_input(case.name, case.pts, case.coefs_fr, case.cs[0], fr=True))
    assert out == case.expect.tobytes()
