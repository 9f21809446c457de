"""The batched fixed-base G1 MSM on the GPU through constantine_amd.fixed.FixedBaseMsm (include/ctt_msm_hip_fixed.h, csrc/fixed.hip):
the cases of the CPU harness with host arrays and with device tensors, the PeerDAS shape against the engine's cached-bases MSM and
the CPU oracle, a batch of one row, and the refusals that come before any launch.  Every comparison is byte equality of affine
Montgomery coordinates."""
import os
import random

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import _fixedref as fx
from tests import _golden

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("tag", fx.MSM_CASES)
def test_cases_with_host_arrays_and_with_device_tensors(tag):
    """T2 scalar edges, T3 chunk edge (and T6: its Montgomery form), T4 collisions, T5 neutral and opposite bases, T7 BN254 G1, T8 /
    T8bn the scalar edges and the largest digits at c = 7, 9 .. 12 (and 2 on 255 bits), in both coefficient forms on both curves"""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    case = fx.case(tag)
    for c in case.cs:
        with FixedBaseMsm(case.name, case.pts, c=c) as f:
            info = f.info()
            assert (info["n"], info["c"], info["windows"]) == (len(case.pts), c, len(fx.layout(fx.BITS[case.name], c)))
            assert info["table_bytes"] == info["n"] * info["records_per_base"] * case.pts.shape[1]
            got = f.msm_batch(case.coefs)
            assert isinstance(got, np.ndarray) and got.tobytes() == case.expect.tobytes(), (tag, c)
            d = f.msm_batch(torch.from_numpy(case.coefs).cuda())
            assert d.is_cuda and d.cpu().numpy().tobytes() == case.expect.tobytes(), (tag, c)
            if case.coefs_fr is not None:
                assert f.msm_batch(case.coefs_fr, fr=True).tobytes() == case.expect.tobytes()
                assert f.msm_batch(torch.from_numpy(case.coefs_fr).cuda(), fr=True).cpu().numpy().tobytes() == case.expect.tobytes()
        with FixedBaseMsm(case.name, torch.from_numpy(case.pts).cuda(), c=c) as f:     # the points as a device tensor
            assert f.msm_batch(case.coefs[:1]).tobytes() == case.expect[:1].tobytes()


@pytest.fixture(scope="module")
def peerdas_shape():
    """the 4096 Lagrange points of the ceremony, 128 rows of seeded scalars below r, and every row through CachedBases.msm -- the
    engine's own path, independent of the table kernel"""
    from constantine_amd import CachedBases, DeviceMsm, kzg
    raw = open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read()
    pts = np.frombuffer(b"".join(kzg.g1_decompress(raw[48 * i:48 * i + 48]) for i in range(4096)), dtype=np.uint8).reshape(4096, 96).copy()
    curve = po.CURVES["bls12_381_g1"]
    rng = random.Random(7594)
    coefs = np.stack([curve.scalars_to_array([rng.randrange(curve.order) for _ in range(4096)]) for _ in range(128)])
    dev = DeviceMsm(0)
    bases = CachedBases("bls12_381_g1", pts, ctx=dev.ctx, table=True)
    want = np.stack([bases.msm(coefs[k], coord="aff") for k in range(128)])
    bases.close()
    dev.close()
    for k in range(0, 128, 16):                                     # 8 of the rows also against the CPU oracle
        assert bytes(want[k]) == bytes(cref.msm("bls12_381_g1", coefs[k], pts, nthreads=8)[0]), k
    return pts, coefs, want


@pytest.mark.parametrize("c", [4, None])
def test_g1_the_peerdas_shape(peerdas_shape, c):
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    pts, coefs, want = peerdas_shape
    with FixedBaseMsm("bls12_381_g1", pts, c=c) as f:
        got = f.msm_batch(torch.from_numpy(coefs).cuda()).cpu().numpy()
        for k in range(128):
            assert bytes(got[k]) == bytes(want[k]), (c, k)
        # G2: a batch of one row
        assert f.msm_batch(coefs[77:78]).tobytes() == want[77:78].tobytes()
        ms = f.last_timings()
        assert ms[0] > 0 and ms[1] > 0


def test_g3_refusals_come_before_any_launch():
    """each case returns -1, leaves the output untouched, and the handle serves the next call"""
    from constantine_amd import FixedBaseMsm, FixedMsmRefused
    case = fx.case("T2")
    g1, g2 = case.pts, np.zeros((1, 192), dtype=np.uint8)
    for kwargs in (dict(curve="bls12_381_g1", points=np.zeros((0, 96), np.uint8)),
                   dict(curve="bls12_381_g1", points=np.zeros((65537, 96), np.uint8)),
                   dict(curve="bls12_381_g1", points=g1, c=1), dict(curve="bls12_381_g1", points=g1, c=13),
                   dict(curve="bls12_381_g2", points=g2)):
        with pytest.raises(FixedMsmRefused) as e:
            FixedBaseMsm(**kwargs)
        assert e.value.code == -1, kwargs
    with FixedBaseMsm("bls12_381_g1", g1, c=5) as f:
        out = np.full((4, 96), 0xA5, dtype=np.uint8)
        with pytest.raises(FixedMsmRefused) as e:
            f.msm_batch(np.zeros((0, 1, 32), np.uint8), out=out[:0])
        assert e.value.code == -1
        huge = np.zeros((1 << 26, 1, 32), dtype=np.uint8)             # m * n * 32 = 2^31; the pages are never touched
        assert f.L.ctt_hip_fixed_msm_batch(f.handle, 0, huge.ctypes.data, 1 << 26, out.ctypes.data, 0) == -1   # (out holds 4 rows only)
        assert f.L.ctt_hip_fixed_last_error() == -1
        del huge
        assert out.tobytes() == b"\xA5" * out.nbytes
        assert f.msm_batch(case.coefs).tobytes() == case.expect.tobytes()
