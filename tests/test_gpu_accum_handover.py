"""
The priority hand-over of the accumulate kernel on the GPU (run with -m gpu on an MI355X): option "accum_handover" -- 0 off, 1 the curve's
drop distance, n >= 2 that distance -- changes WHEN the waves of k_accum issue, never what they compute.  So every result here is asked
twice: byte-identical under 0, 1 and 8, and equal to the big-integer oracle.

The inputs are the synthetic points [s_i]G of known s_i (oracle/cref.py gen_point_scalars): the expected element is ONE scalar
multiplication of oracle/pyoracle.py, [sum k_i s_i mod r]G.  Only the iteration bookkeeping can go wrong (msm_bodies.h accum_body_xyzz
counts the iterations since the lane's first entry and drops the priority `handover` before K), so the shapes are the small ones that
bend it: n no multiple of 64 or of K; K = 1, 2, the drop distance, one more, and 37 -- a drop point at or before the first iteration,
lanes whose range the end of the set cuts short, whole waves that return at once; one run over many lanes; the INTO form of a sliced
host-pointer call; three MSMs in flight.
"""
import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

BLS, BN = "bls12_381_g1", "bn254_snarks_g1"
HANDOVERS = (0, 1, 8)
DROP = 8                      # the explicit drop distance of HANDOVERS
KS = (1, 2, DROP, DROP + 1, 37)
# (curve, pairs, option "glv": 2 = the split never, 1 = always -- BLS12-381 G1 only)
SHAPES = [(BLS, 1000, 2), (BLS, 4096, 1), (BN, 1000, 0)]
SEED = 9700


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def eng(torch_cuda):
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


def _expect(name, seed, sc):
    curve = po.CURVES[name]
    return curve.aff_to_bytes(cref.msm_by_discrete_logs(name, seed, sc))


@pytest.fixture(scope="module")
def inputs(torch_cuda, eng):
    """per curve: 4096 synthetic points on the device and their scalars; every case is a prefix.  -> name: (d_scalars, d_points, scalars)"""
    out = {}
    for name in (BLS, BN):
        curve = po.CURVES[name]
        d_pts = torch_cuda.empty((4096, curve.aff_bytes), dtype=torch_cuda.uint8, device="cuda")
        eng.gen_points(name, SEED, 4096, d_pts)
        sc = cref.synth_scalars(SEED + 1, 4096, curve.scalar_bits)
        out[name] = (torch_cuda.from_numpy(sc).cuda(), d_pts, sc)
    return out


@pytest.fixture(scope="module")
def expected(inputs):
    """the oracle's element of every shape, computed once"""
    return {(name, n): _expect(name, SEED, inputs[name][2][:n]) for name, n, _ in SHAPES}


def _under_each_handover(eng, call, what):
    """call() under accum_handover 0, 1 and 8 -> the three results (the option is back at its default afterwards)"""
    got = []
    try:
        for h in HANDOVERS:
            eng.set_option("accum_handover", h)
            got.append(bytes(call()))
    finally:
        eng.set_option("accum_handover", 1)
    assert got[1] == got[0] and got[2] == got[0], (what, "the option changed the result")
    return got[0]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name, n, glv", SHAPES, ids=[f"{s[0]}-{s[1]}-glv{s[2]}" for s in SHAPES])
def test_forced_entries_per_lane(name, n, glv, K, inputs, expected, eng):
    ds, dp, _ = inputs[name]
    try:
        eng.set_option("K", K)
        eng.set_option("glv", glv)
        got = _under_each_handover(eng, lambda: eng.msm(name, ds, dp, n, coord="aff"), (name, n, glv, K))
        plan = eng.last_plan()
        # (the planner's floor is four entries per lane, msm_plan.h plan_finish: K = 1 and 2 run as 4 -- still at or below every drop distance here)
        assert plan["K"] == max(K, 4) and plan["glv"] == (1 if glv == 1 else 0), plan
        assert got == expected[(name, n)], (name, n, glv, K, plan)
    finally:
        eng.set_option("K", 0)
        eng.set_option("glv", 0)


@pytest.mark.parametrize("name", [BLS, BN])
def test_default_plan(name, inputs, expected, eng):
    """K as the plan chooses it (no option but the hand-over): what a caller runs"""
    ds, dp, _ = inputs[name]
    assert _under_each_handover(eng, lambda: eng.msm(name, ds, dp, 1000, coord="aff"), name) == expected[(name, 1000)]


@pytest.mark.parametrize("name, log2n", [(BLS, 19), (BN, 20)])
def test_curve_default_at_its_size_bound(name, log2n, eng, torch_cuda):
    """The smallest size at which option 1 switches the hand-over on by itself (msm_bodies.h accum_handover_log2n; every other case of this file
    is below it, where 1 resolves to off): the distance is then max(floor, K / 8) of the plan's own K (msm_place.h place_accum).  Off, the
    default, and the explicit distances K / 8 and K - 1 (the drop point at the first iteration) give the same bytes, the oracle's."""
    n = 1 << log2n
    curve = po.CURVES[name]
    d_pts = torch_cuda.empty((n, curve.aff_bytes), dtype=torch_cuda.uint8, device="cuda")
    eng.gen_points(name, SEED + 10, n, d_pts)
    sc = cref.synth_scalars(SEED + 11, n, curve.scalar_bits)
    ds = torch_cuda.from_numpy(sc).cuda()
    def run(h):
        eng.set_option("accum_handover", h)
        return bytes(eng.msm(name, ds, d_pts, n, coord="aff"))
    try:
        off = run(0)
        K = eng.last_plan()["K"]
        assert K >= 32, eng.last_plan()   # (room for a distance of K / 8 >= 2: below 2 the option's value means something else)
        got = [run(1), run(K // 8), run(K - 1)]
    finally:
        eng.set_option("accum_handover", 1)
    assert got == [off] * 3, (name, "the option changed the result")
    assert off == _expect(name, SEED + 10, sc), (name, eng.last_plan())


@pytest.mark.parametrize("name", [BLS, BN])
@pytest.mark.parametrize("K", [0, DROP + 1])
def test_all_scalars_equal(name, K, inputs, eng, torch_cuda):
    """one scalar 4096 times: every window has ONE run, spanning every lane of the set -- heads only, and the head merge's long chain"""
    curve = po.CURVES[name]
    _, dp, _ = inputs[name]
    sc = np.repeat(cref.synth_scalars(SEED + 2, 1, curve.scalar_bits), 4096, axis=0)
    ds = torch_cuda.from_numpy(sc).cuda()
    try:
        eng.set_option("K", K)
        got = _under_each_handover(eng, lambda: eng.msm(name, ds, dp, 4096, coord="aff"), (name, K))
    finally:
        eng.set_option("K", 0)
    assert got == _expect(name, SEED, sc), (name, K, eng.last_plan())


@pytest.mark.parametrize("name", [BLS, BN])
def test_host_pointer_call_in_two_slices(name, inputs, torch_cuda):
    """a host-pointer MSM uploaded in two slices: the second slice's accumulation continues the stored sums (k_accum<FD, true>)"""
    from constantine_amd import _lib, multiScalarMul_vartime
    curve = po.CURVES[name]
    _, dp, sc = inputs[name]
    pts = dp.cpu().numpy()
    L = _lib.lib()
    got = []
    try:
        assert L.ctt_hip_msm_set_option(None, b"chunks", 2) == 0
        for K in (0, DROP + 1):
            assert L.ctt_hip_msm_set_option(None, b"K", K) == 0
            for h in HANDOVERS:
                assert L.ctt_hip_msm_set_option(None, b"accum_handover", h) == 0
                r = multiScalarMul_vartime(name, sc, pts, coord="jac")
                got.append(curve.aff_to_bytes(curve.jac_from_bytes(bytes(r))))
    finally:
        L.ctt_hip_msm_set_option(None, b"chunks", 0)
        L.ctt_hip_msm_set_option(None, b"K", 0)
        L.ctt_hip_msm_set_option(None, b"accum_handover", 1)
    assert got == [_expect(name, SEED, sc)] * len(got), name


@pytest.mark.parametrize("name", [BLS, BN])
def test_three_in_flight_out_of_order(name, inputs, eng, torch_cuda):
    """three tickets over two input sets (the second: other scalars over the points reversed), finished out of order"""
    curve = po.CURVES[name]
    n = 4096
    ds, dp, sc = inputs[name]
    sc2 = cref.synth_scalars(SEED + 3, n, curve.scalar_bits)
    ds2 = torch_cuda.from_numpy(sc2).cuda()
    dp2 = torch_cuda.flip(dp, dims=[0]).contiguous()
    first = (ds, dp, _expect(name, SEED, sc))
    sets = [first, (ds2, dp2, _expect(name, SEED, sc2[::-1])), first]
    try:
        for h in HANDOVERS:
            eng.set_option("accum_handover", h)
            for order in ((2, 0, 1), (1, 2, 0)):
                t = [eng.submit(name, s[0], s[1], n) for s in sets]
                for i in order:
                    assert bytes(eng.finish(t[i], coord="aff")) == sets[i][2], (name, h, order, i)
    finally:
        eng.set_option("accum_handover", 1)
