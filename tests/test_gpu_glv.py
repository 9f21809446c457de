"""
The endomorphism split of BLS12-381 G1 on the GPU (run with -m gpu on an MI355X): device-resident MSMs with the split forced on
(option "glv" = 1; by default it runs at the curve's measured sizes), byte-exact on the affine result against the big-integer oracle.

The inputs are the synthetic points [s_i]G of known s_i (oracle/cref.py gen_point_scalars), so the expected element is ONE scalar
multiplication of oracle/pyoracle.py: [sum k_i s_i mod r]G -- no elliptic-curve code shared with what is tested.  The CPU twin of this
file is tests/test_glv_split.py; the front kernel alone is held pair by pair in tests/test_glv_front_probe.py and the sort on half
scalars in tests/test_sort_probe.py.  Here also: the sizes at which the split runs by default, cached bases and window tables under the
forcing option, and scalars outside the contract on the split path.
"""
import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NAME = "bls12_381_g1"
CURVE = po.CURVES[NAME]
R = CURVE.order


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def eng(torch_cuda):
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    d.set_option("glv", 1)
    yield d
    d.close()


def _logs(seed, n):
    return [int.from_bytes(bytes(row), "little") for row in cref.gen_point_scalars(seed, n)]


def _case(torch, eng, n, seed, specials=True):
    """(device scalars, device points, canonical scalars, expected affine bytes) of n pairs: synthetic points made on the device, with --
    where n has room -- a neutral point, a pair P / -P under one scalar, one point twice, a zero scalar, r, 2^255 - 1, a scalar just
    above r / 2 and a scalar whose second half is zero"""
    d_pts = torch.empty((n, CURVE.aff_bytes), dtype=torch.uint8, device="cuda")
    eng.gen_points(NAME, seed, n, d_pts)
    sc = cref.synth_scalars(seed + 1, n, 255)
    logs = _logs(seed, n)
    if specials and n >= 65:
        pts = d_pts.cpu().numpy()
        pts[5] = 0
        logs[5] = 0
        pts[7] = CURVE.points_to_array([CURVE.neg(CURVE.aff_from_bytes(bytes(pts[6])))])[0]
        logs[7] = R - logs[6]
        sc[7] = sc[6]
        pts[9] = pts[8]
        logs[9] = logs[8]
        sc[10:16] = CURVE.scalars_to_array([0, R, (1 << 255) - 1, (R + 1) // 2, po.synth_scalar(seed, 3, 120), R - 1])
        d_pts = torch.from_numpy(pts).cuda()
    ks = [int.from_bytes(bytes(row), "little") for row in sc]
    t = sum(k * s for k, s in zip(ks, logs)) % R
    expect = CURVE.aff_to_bytes(CURVE.scalar_mul(t, CURVE.gen))
    return torch.from_numpy(sc).cuda(), d_pts, sc, expect


@pytest.fixture(scope="module")
def cases(torch_cuda, eng):
    return {n: _case(torch_cuda, eng, n, 9100 + n) for n in (1, 65, 4096)}


@pytest.mark.parametrize("n", [1, 65, 4096])
def test_split_msm_vs_big_integer_oracle(n, cases, eng):
    ds, dp, sc, expect = cases[n]
    assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect, eng.last_plan()
    plan = eng.last_plan()
    assert plan["glv"] == 1 and plan["W"] == 2 * plan["bucket_sets"], plan
    # small windows and few entries per lane: several lanes per bucket set, runs that straddle lanes, both merge forms
    for c, K, mc in ((5, 4, 0), (8, 8, 1), (16, 0, 2)):
        for k, v in (("c", c), ("K", K), ("merge_chain", mc)):
            eng.set_option(k, v)
        try:
            assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect, (c, K, mc, eng.last_plan())
        finally:
            for k in ("c", "K", "merge_chain"):
                eng.set_option(k, 0)
    # the same call with the split off: the 16-window path, the same element
    eng.set_option("glv", 2)
    try:
        assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect
        plan = eng.last_plan()
        assert plan["glv"] == 0 and plan["W"] == plan["bucket_sets"], plan
    finally:
        eng.set_option("glv", 1)


@pytest.mark.parametrize("n", [1, 65, 4096])
def test_split_msm_fr_montgomery_coefficients(n, cases, eng, torch_cuda):
    ds, dp, sc, expect = cases[n]
    # the coefficients as Fr elements in Montgomery form: canonical below r first (the entry point takes field elements)
    ks = [int.from_bytes(bytes(row), "little") % R for row in sc]
    d_mont = torch_cuda.from_numpy(CURVE.fr_scalars_to_array(ks)).cuda()
    assert bytes(eng.msm(NAME, d_mont, dp, n, coord="aff", fr_coefs=True)) == expect, eng.last_plan()
    assert eng.last_plan()["glv"] == 1


def test_split_msm_at_sixteen_bit_windows(eng, torch_cuda):
    """2^18 pairs: the default plan of the split has 16-bit windows there -- 2^19 entries in 8 bucket sets of 2^15 buckets, the
    shape of the headline size (its sort runs the partition in several blocks and the accumulation in every lane of the chip)"""
    n = 1 << 18
    ds, dp, sc, expect = _case(torch_cuda, eng, n, 9300, specials=False)
    assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect, eng.last_plan()
    plan = eng.last_plan()
    assert (plan["c"], plan["W"], plan["bucket_sets"], plan["glv"]) == (16, 16, 8, 1), plan


def test_three_in_flight_alternating_inputs(cases, eng, torch_cuda):
    """submit() three deep over two input sets of different sizes: the record array, the half scalars and the canonical scalars are
    shared by the MSMs in flight (stream order keeps them apart), the bucket sets are per slot"""
    a = cases[4096]
    b = _case(torch_cuda, eng, 2500, 9400)
    sets = [(a[0], a[1], 4096, a[3]), (b[0], b[1], 2500, b[3])]
    pend = []
    for i in range(9):
        ds, dp, n, expect = sets[i % 2]
        pend.append((eng.submit(NAME, ds, dp, n), expect, i))
        if len(pend) == 3:
            t, e, j = pend.pop(0)
            assert bytes(eng.finish(t, coord="aff")) == e, j
    for t, e, j in pend:
        assert bytes(eng.finish(t, coord="aff")) == e, j


# the sizes at which a device-resident MSM without cached bases takes the split by default: 2^GLV_LOG2N .. 2^GLV_MAX_LOG2N pairs
# (csrc/msm_bodies.h Bls12381G1::TUNE: glv_log2n, glv_max_log2n)
GLV_LOG2N, GLV_MAX_LOG2N = 17, 21


def test_default_follows_the_curve_sizes(cases, torch_cuda):
    """option "glv" = 0: the split runs at the curve's sizes (msm_bodies.h glv_log2n .. glv_max_log2n; 0 = never) and never on the
    other curves; the result is the same either way"""
    from constantine_amd import DeviceMsm
    ds, dp, sc, expect = cases[4096]
    assert 4096 < 1 << GLV_LOG2N
    d = DeviceMsm(0)
    try:
        assert bytes(d.msm(NAME, ds, dp, 4096, coord="aff")) == expect
        assert d.last_plan()["glv"] == 0
        d.set_option("glv", 1)
        name = "bn254_snarks_g1"
        n = 300
        pts = cref.gen_points(name, 77, n)
        s2 = cref.synth_scalars(78, n, 254)
        want = bytes(cref.msm(name, s2, pts)[0])
        got = d.msm(name, torch_cuda.from_numpy(s2).cuda(), torch_cuda.from_numpy(pts).cuda(), n, coord="aff")
        assert bytes(got) == want and d.last_plan()["glv"] == 0
    finally:
        d.close()


BOUNDS_SEED = 9500


@pytest.fixture(scope="module")
def bounds_inputs(torch_cuda, eng):
    """2^GLV_MAX_LOG2N + 1 synthetic pairs on the device; every size of the test below is a prefix of them"""
    n = (1 << GLV_MAX_LOG2N) + 1
    d_pts = torch_cuda.empty((n, CURVE.aff_bytes), dtype=torch_cuda.uint8, device="cuda")
    eng.gen_points(NAME, BOUNDS_SEED, n, d_pts)
    sc = cref.synth_scalars(BOUNDS_SEED + 1, n, 255)
    return torch_cuda.from_numpy(sc).cuda(), d_pts, sc


@pytest.mark.parametrize("n, glv", [((1 << GLV_LOG2N) - 1, 0), (1 << GLV_LOG2N, 1), (1 << GLV_MAX_LOG2N, 1), ((1 << GLV_MAX_LOG2N) + 1, 0)])
def test_default_split_range_is_exactly_the_curve_sizes(n, glv, bounds_inputs):
    """a fresh context with no option set, one pair below, at both ends of and one pair above GLV_LOG2N .. GLV_MAX_LOG2N: the plan says
    whether the split ran, and the result is [sum k_i s_i mod r]G either way (the dot product over the known discrete logs runs on 16-bit
    limbs in numpy: oracle/cref.py msm_by_discrete_logs)"""
    from constantine_amd import DeviceMsm
    ds, dp, sc = bounds_inputs
    expect = CURVE.aff_to_bytes(cref.msm_by_discrete_logs(NAME, BOUNDS_SEED, sc[:n]))
    d = DeviceMsm(0)
    try:
        assert bytes(d.msm(NAME, ds, dp, n, coord="aff")) == expect, d.last_plan()
        plan = d.last_plan()
        assert plan["glv"] == glv, plan
        assert plan["W"] == (2 if glv else 1) * plan["bucket_sets"], plan
    finally:
        d.close()


@pytest.mark.parametrize("n", [4096, 1 << GLV_LOG2N])
@pytest.mark.parametrize("table", [False, True], ids=["records", "table"])
def test_cached_bases_stay_on_the_plain_path(n, table, bounds_inputs, eng):
    """option "glv" = 1 forces the split for device-resident points only: cached records and a window table have no front stage"""
    from constantine_amd import CachedBases
    ds, dp, sc = bounds_inputs
    expect = CURVE.aff_to_bytes(cref.msm_by_discrete_logs(NAME, BOUNDS_SEED, sc[:n]))
    bases = CachedBases(NAME, dp[:n], ctx=eng.ctx, on_device=True, table=table)
    try:
        assert (bases.window_bits > 0) == table
        assert bytes(bases.msm(ds[:n], coord="aff")) == expect, eng.last_plan()
        plan = eng.last_plan()
        assert plan["glv"] == 0, plan
        if table:
            assert plan["bucket_sets"] == 1, plan
        # and the same pairs without the cache take the split on this context
        assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect and eng.last_plan()["glv"] == 1
    finally:
        bases.close()


def test_scalars_beyond_the_bit_width_on_the_split_path(bounds_inputs, eng, torch_cuda):
    """Scalars of 2^255 and above are outside the contract of the split as of every MSM (its reduction subtracts r once and its quotient
    estimate reads bits 126 .. 253): with bits 254 and 255 set the halves are unspecified and may have bit 127 set.  What holds is what
    tests/test_gpu_parity.py holds for BN254: every call returns, nothing is corrupted, and the next in-contract call on the same
    context is exact."""
    ds, dp, sc = bounds_inputs
    n = 50000
    bad = np.full((n, 32), 0xFF, dtype=np.uint8)
    bad[::3] = sc[:n:3]
    d_bad = torch_cuda.from_numpy(bad).cuda()
    try:
        for c in (0, 16, 13):
            eng.set_option("c", c)
            eng.msm(NAME, d_bad, dp, n, coord="aff")                      # must return
            assert eng.last_plan()["glv"] == 1
    finally:
        eng.set_option("c", 0)
    expect = CURVE.aff_to_bytes(cref.msm_by_discrete_logs(NAME, BOUNDS_SEED, sc[:n]))
    assert bytes(eng.msm(NAME, ds, dp, n, coord="aff")) == expect and eng.last_plan()["glv"] == 1
