"""ctt_hip_fr_ntt on the device through constantine_amd.ntt.NttPlan: the case list of the CPU harness test (tests/_nttref.cases)
compared for equality with the Python integers of tests/_nttref.py, every refusal of the header with guard words around the output,
and two contexts with a plan each."""
import ctypes

import numpy as np
import pytest

from tests import _nttref as ref

pytestmark = pytest.mark.gpu

CURVE_OF = {"bls12_381_fr": "bls12_381_g1", "bn254_snarks_fr": "bn254_snarks_g1", "pallas_fr": "pallas", "vesta_fr": "vesta",
            "banderwagon_fr": "banderwagon"}


def _arr(words):
    return np.frombuffer(ref.to_bytes(words), dtype=np.uint8).copy()


def _flags(fl):
    return dict(inverse=bool(fl & ref.INVERSE), in_brp=bool(fl & ref.IN_BRP), out_brp=bool(fl & ref.OUT_BRP),
                in_mont=bool(fl & ref.IN_MONT), out_mont=bool(fl & ref.OUT_MONT))


@pytest.mark.parametrize("field", list(ref.FIELDS))
def test_device_matches_python(field):
    import torch
    from constantine_amd.ntt import NttPlan
    plans = {}
    try:
        for case in ref.cases(field):
            name, lg, tile, batch, fl, _sk, in_place = case
            omega, shift, stored, want = ref.case_data(field, case)
            if (lg, tile) not in plans:
                plans[(lg, tile)] = NttPlan(CURVE_OF[field], lg, omega, tile_log2=tile)
            plan = plans[(lg, tile)]
            x = _arr(stored)
            if in_place:
                t = torch.from_numpy(x).cuda()
                assert plan.ntt(t, shift=shift, **_flags(fl)) is t
                got = t.cpu().numpy()
            else:
                t = torch.from_numpy(x).cuda()
                out = torch.full_like(t, 0xAB)
                plan.ntt(t, shift=shift, out=out, **_flags(fl))
                assert np.array_equal(t.cpu().numpy(), x), (field, name, "the input changed")
                got = out.cpu().numpy()
            assert ref.from_bytes(got.tobytes()) == want, (field, name)
        # G2 shares G1's field: the same plan parameters under the other curve id give the same transform
        if field == "bls12_381_fr":
            case = ("g2", 7, 3, 1, ref.OUT_BRP, "rand", False)
            omega, shift, stored, want = ref.case_data(field, case)
            p2 = NttPlan("bls12_381_g2", 7, omega, tile_log2=3)
            plans["g2"] = p2
            assert ref.from_bytes(p2.ntt(_arr(stored), out_brp=True, shift=shift).tobytes()) == want
    finally:
        for p in plans.values():
            p.close()


def test_host_arrays_and_info():
    from constantine_amd.ntt import NttPlan
    field = "bls12_381_fr"
    case = ("host", 12, 0, 2, ref.OUT_BRP, "w2n", False)
    omega, shift, stored, want = ref.case_data(field, case)
    plan = NttPlan("bls12_381_g1", 12, omega)
    try:
        assert plan.info() == {"log2n": 12, "tile_log2": 8, "passes": 2, "table_bytes": 2048 * 32}
        x = _arr(stored).reshape(2, 4096, 32)
        y = plan.ntt(x, out_brp=True, shift=shift)
        assert y.shape == x.shape and ref.from_bytes(y.tobytes()) == want
        back = plan.ntt(y, inverse=True, in_brp=True, shift=shift)
        assert np.array_equal(back, x)
    finally:
        plan.close()


def test_refusals_leave_the_output_alone():
    import torch
    from constantine_amd import _lib
    from constantine_amd.msm import DeviceMsm
    from constantine_amd.ntt import NttPlan, NttRefused
    L = _lib.lib()
    p = ref.FIELDS["bls12_381_fr"][2]
    lg, n = 5, 32
    omega = ref.root_of_unity(p, lg)
    dev, other = DeviceMsm(0), DeviceMsm(0)
    plan = None
    try:
        # plan_create: log2n, tile_log2, omega (order n/2, 1, >= r), a NULL omega, the curve id
        for kw in (dict(log2n=0), dict(log2n=25), dict(tile_log2=10), dict(tile_log2=-1), dict(omega=omega * omega % p), dict(omega=1),
                   dict(omega=p), dict(omega=0)):
            args = dict(log2n=lg, omega=omega, tile_log2=0)
            args.update(kw)
            with pytest.raises(NttRefused) as e:
                NttPlan("bls12_381_g1", args["log2n"], args["omega"], device=dev, tile_log2=args["tile_log2"])
            assert e.value.code == -1, kw
        with pytest.raises(NttRefused):   # Banderwagon's scalar field has two-adicity 5
            NttPlan("banderwagon", 6, 1, device=dev)
        assert not L.ctt_hip_fr_ntt_plan_create(dev.ctx, 0, lg, None, 0) and L.ctt_hip_last_error() == -1
        assert not L.ctt_hip_fr_ntt_plan_create(dev.ctx, 7, lg, (ctypes.c_uint8 * 32)(), 0) and L.ctt_hip_last_error() == -1

        plan = NttPlan("bls12_381_g1", lg, omega, device=dev)
        guard = 64
        buf = torch.full((guard + n * 32 + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        src = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        before = buf.cpu().numpy().copy()
        d_out, d_in = buf.data_ptr() + guard, src.data_ptr()
        vp = ctypes.c_void_p

        def refused(rc):
            assert rc == -1 and L.ctt_hip_last_error() == -1
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), before)

        refused(L.ctt_hip_fr_ntt(dev.ctx, None, vp(d_out), vp(d_in), 1, 0, None))                 # NULL plan
        refused(L.ctt_hip_fr_ntt(dev.ctx, plan.plan, None, vp(d_in), 1, 0, None))                 # NULL out
        refused(L.ctt_hip_fr_ntt(dev.ctx, plan.plan, vp(d_out), None, 1, 0, None))                # NULL in
        refused(L.ctt_hip_fr_ntt(other.ctx, plan.plan, vp(d_out), vp(d_in), 1, 0, None))          # another context
        refused(plan.ntt_ptr(d_out, d_in, 1, 0, shift=0))                                         # a shift of zero
        refused(plan.ntt_ptr(d_out, d_in, 1, 0, shift=p))                                         # a shift >= r
        refused(plan.ntt_ptr(d_out, d_in, 1, 32, None))                                           # an unknown flag
        refused(plan.ntt_ptr(d_out + 4, d_in, 1, 0, None))                                        # misaligned
        refused(plan.ntt_ptr(d_out, d_in, (1 << 26 - lg) + 1, 0, None))                           # batch * n > 2^26
        # batch == 0: 0, nothing touched
        assert plan.ntt_ptr(d_out, d_in, 0, 0, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before)
        # and the plan still serves: exactly the n elements between the guards are written
        assert plan.ntt_ptr(d_out, d_in, 1, 0, None) == 0
        after = buf.cpu().numpy()
        assert np.array_equal(after[:guard], before[:guard]) and np.array_equal(after[-guard:], before[-guard:])
        assert not after[guard:-guard].any()    # the transform of zeros
    finally:
        if plan:
            plan.close()
        dev.close()
        other.close()


def test_two_contexts_agree():
    from constantine_amd.msm import DeviceMsm
    from constantine_amd.ntt import NttPlan
    field = "bn254_snarks_fr"
    case = ("two", 9, 0, 3, ref.IN_BRP | ref.IN_MONT, "rand", False)
    omega, shift, stored, want = ref.case_data(field, case)
    devs = [DeviceMsm(0), DeviceMsm(0)]
    plans = [NttPlan("bn254_snarks_g1", 9, omega, device=d) for d in devs]
    try:
        outs = [p.ntt(_arr(stored), in_brp=True, in_mont=True, shift=shift) for p in plans]
        assert np.array_equal(outs[0], outs[1])
        assert ref.from_bytes(outs[0].tobytes()) == want
    finally:
        for p in plans:
            p.close()
        for d in devs:
            d.close()
