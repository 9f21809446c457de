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
    neutral and opposite bases, T7 BN254 G1"""
    case = fx.case(tag)
    for c in case.cs:
        out = harness("msm", fx.harness_msm_input(case.name, case.pts, case.coefs, c))
        got = np.frombuffer(out, dtype=np.uint8).reshape(case.expect.shape)
        for k in range(len(got)):
            assert bytes(got[k]) == bytes(case.expect[k]), (tag, c, k)


def test_t6_montgomery_coefficients_give_the_same_bytes(harness):
    """the `fr` form of T3: Montgomery residues of the scalars mod r"""
    case = fx.case("T3")
    out = harness("msm", fx.harness_msm_input(case.name, case.pts, case.coefs_fr, case.cs[0], fr=True))
    assert out == case.expect.tobytes()
