"""Banderwagon MSM on the GPU (twisted Edwards group law through the pipeline), against the Python oracle tests/_banderwagon.py
and the Verkle vector commitment of tests/golden/banderwagon_verkle.json."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import _banderwagon as bw

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "banderwagon_verkle.json")
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64, 128, 1024, 2048, 16384]
CID = 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def dev(torch_cuda):
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def verkle():
    d = json.load(open(GOLDEN))
    return bw.crs(256), [int(h, 16) for h in d["commit_scalars"]], d["commitment"]


def _pts(points):
    return np.frombuffer(b"".join(bw.aff_bytes(p) for p in points), dtype=np.uint8).reshape(-1, 64).copy()


def _big(scalars):
    return np.frombuffer(b"".join(bw.big_bytes(k) for k in scalars), dtype=np.uint8).reshape(-1, 32).copy()


def _fr(scalars):
    return np.frombuffer(b"".join(bw.fr_bytes(k) for k in scalars), dtype=np.uint8).reshape(-1, 32).copy()


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prj(r):
    r = bytes(r)
    assert bw.fp_from(r[64:96]) == 1, "the canonical representative has Z = 1"
    return bw.aff_from(r[:64])


def _synth(dev, torch, seed, n):
    d = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", seed, n, d)
    return d


def test_verkle_commitment_constantine_symbols(verkle):
    from constantine_amd import multiScalarMul_vartime
    crs, scalars, expect = verkle
    pts = _pts(crs)
    for fr, coefs in ((True, _fr(scalars)), (False, _big(scalars))):
        r = multiScalarMul_vartime("banderwagon", coefs, pts, coord="prj", fr_coefs=fr)
        assert "0x" + bw.serialize(_prj(r)).hex() == expect
        a = multiScalarMul_vartime("banderwagon", coefs, pts, coord="aff", fr_coefs=fr)
        assert "0x" + bw.serialize(bw.aff_from(bytes(a))).hex() == expect


def test_verkle_commitment_cached_bases(dev, torch_cuda, verkle):
    from constantine_amd import CachedBases
    crs, scalars, expect = verkle
    cb = CachedBases("banderwagon", _pts(crs), ctx=dev.ctx)
    try:
        assert "0x" + bw.serialize(_prj(cb.msm(_fr(scalars), coord="prj", fr_coefs=True))).hex() == expect
        other = [random.Random(5).randrange(bw.R) for _ in range(256)]
        t1 = cb.submit(_to_dev(torch_cuda, _fr(scalars)), 256, fr_coefs=True)
        t2 = cb.submit(_to_dev(torch_cuda, _big(other)), 256)
        r2, r1 = cb.finish(t2, coord="aff"), cb.finish(t1, coord="prj")
        assert "0x" + bw.serialize(_prj(r1)).hex() == expect
        assert bw.aff_from(bytes(r2)) == bw.msm_fast(other, crs)
        with pytest.raises(ValueError):
            cb.msm(_fr(scalars), coord="jac", fr_coefs=True)
    finally:
        cb.close()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_device_and_host(dev, torch_cuda, n):
    from constantine_amd import multiScalarMul_vartime
    rng = random.Random(1000 + n)
    d_pts = _synth(dev, torch_cuda, 77 + n, n)
    logs = [bw.synth_log(77 + n, j) for j in range(n)]
    for j in range(min(n, 3)):   # the generator itself against the oracle
        assert bw.aff_from(bytes(d_pts[j].cpu().numpy())) == bw.mul(logs[j], bw.G)
    ks = [rng.randrange(1 << 253) for _ in range(n)]
    expect = bw.mul(sum(k * s for k, s in zip(ks, logs)) % bw.R, bw.G)
    r = dev.msm("banderwagon", _to_dev(torch_cuda, _big(ks)), d_pts, n, coord="aff")
    assert bw.aff_from(bytes(r)) == expect
    r = multiScalarMul_vartime("banderwagon", _big(ks), d_pts.cpu().numpy(), coord="prj")
    assert _prj(r) == expect


def test_edge_cases(dev, torch_cuda):
    from constantine_amd import multiScalarMul_vartime
    P = bw.mul(987654321, bw.G)
    Q = bw.mul(5, bw.G)
    cases = [
        ([0, 0, 0], [P, Q, bw.G]),                                          # zero scalars
        ([bw.R, bw.R + 1, (1 << 253) - 1], [P, Q, bw.G]),                   # scalars >= r
        ([3, 5, 7, 11, 13, 17, 1 << 200, 19], [P] * 8),                     # one point everywhere: doublings inside buckets
        ([9, 9, 123, 123], [P, bw.neg(P), Q, bw.neg(Q)]),                   # P and -P in one bucket
        ([4, 7, 1, 3], [bw.O, bw.T2, bw.T2, bw.O]),                         # the neutral and (0, -1) as inputs
        ([12, 34, 56], [bw.add(P, bw.T2), bw.add(Q, bw.T2), P]),            # coset representatives P + (0, -1)
    ]
    for ks, pts in cases:
        expect = bw.msm(ks, pts)
        r = multiScalarMul_vartime("banderwagon", _big(ks), _pts(pts), coord="prj")
        assert _prj(r) == expect, (ks, pts)
        r = dev.msm("banderwagon", _to_dev(torch_cuda, _big(ks)), _to_dev(torch_cuda, _pts(pts)), len(ks), coord="aff")
        assert bw.aff_from(bytes(r)) == expect, (ks, pts)
    r = multiScalarMul_vartime("banderwagon", np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), coord="prj")
    assert [bw.fp_from(bytes(r)[i:i + 32]) for i in (0, 32, 64)] == [0, 1, 1]


@pytest.mark.parametrize("log2n", [16, 18, 20])
def test_full_size_discrete_log(dev, torch_cuda, log2n):
    n = 1 << log2n
    seed = 900 + log2n
    d_pts = _synth(dev, torch_cuda, seed, n)
    g = torch_cuda.Generator().manual_seed(log2n)
    ks = torch_cuda.randint(0, 256, (n, 32), dtype=torch_cuda.uint8, generator=g)
    ks[:, 31] &= 0x1f   # < 2^253
    kb = ks.numpy()
    kint = [int.from_bytes(kb[j].tobytes(), "little") for j in range(n)]
    total = sum(k * bw.synth_log(seed, j) for j, k in enumerate(kint)) % bw.R
    r = dev.msm("banderwagon", ks.cuda(), d_pts, n, coord="prj")
    assert _prj(r) == bw.mul(total, bw.G)


def test_unknown_logs(dev, torch_cuda):
    n = 1 << 12
    pts = bw.crs(n, skip=256)   # the Verkle CRS generator continued past the 256 points of the commitment
    rng = random.Random(4242)
    ks = [rng.randrange(1 << 128) for _ in range(n)]
    r = dev.msm("banderwagon", _to_dev(torch_cuda, _big(ks)), _to_dev(torch_cuda, _pts(pts)), n, coord="aff")
    assert bw.aff_from(bytes(r)) == bw.msm_fast(ks, pts)


def test_tickets_mixed_with_bls12_381_g1(dev, torch_cuda):
    n = 4096
    bpts = _synth(dev, torch_cuda, 31, n)
    gpts = torch_cuda.empty((n, 96), dtype=torch_cuda.uint8, device="cuda")
    dev.gen_points("bls12_381_g1", 32, n, gpts)
    rng = random.Random(33)
    kb = [[rng.randrange(1 << 253) for _ in range(n)] for _ in range(2)]
    kg = _big([rng.randrange(1 << 255) for _ in range(n)])
    g_expect = dev.msm("bls12_381_g1", _to_dev(torch_cuda, kg), gpts, n, coord="aff")
    t0 = dev.submit("banderwagon", _to_dev(torch_cuda, _big(kb[0])), bpts, n)
    t1 = dev.submit("bls12_381_g1", _to_dev(torch_cuda, kg), gpts, n)
    t2 = dev.submit("banderwagon", _to_dev(torch_cuda, _big(kb[1])), bpts, n)
    r2, r0, r1 = dev.finish(t2, coord="aff"), dev.finish(t0, coord="prj"), dev.finish(t1, coord="aff")
    logs = [bw.synth_log(31, j) for j in range(n)]
    assert _prj(r0) == bw.mul(sum(k * s for k, s in zip(kb[0], logs)) % bw.R, bw.G)
    assert bw.aff_from(bytes(r2)) == bw.mul(sum(k * s for k, s in zip(kb[1], logs)) % bw.R, bw.G)
    assert bytes(r1) == bytes(g_expect)


def test_refusals(dev, torch_cuda):
    from constantine_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    pts = _pts([bw.G, bw.mul(3, bw.G)])
    ks = _big([1, 2])
    sentinel = np.full(96, 0xAB, dtype=np.uint8)

    def untouched(call):
        r = sentinel.copy()
        assert call(r.ctypes.data_as(vp)) == -1
        assert bytes(r) == bytes(sentinel)

    untouched(lambda r: L.ctt_hip_msm_host(CID, 0, 1, r, ks.ctypes.data_as(vp), pts.ctypes.data_as(vp), 2))   # CTT_HIP_OUT_JAC
    untouched(lambda r: L.ctt_hip_ec_sum_affine(CID, 1, r, pts.ctypes.data_as(vp), 2))
    d_pts, d_ks = _to_dev(torch_cuda, pts), _to_dev(torch_cuda, ks)
    untouched(lambda r: L.ctt_hip_msm_device(dev.ctx, CID, 0, 1, r, vp(d_ks.data_ptr()), vp(d_pts.data_ptr()), 2))
    untouched(lambda r: L.ctt_hip_batch_affine(dev.ctx, CID, 2, r, pts.ctypes.data_as(vp), 1, 0))
    untouched(lambda r: L.ctt_hip_subgroup_check(dev.ctx, CID, r, pts.ctypes.data_as(vp), 2, 0))
    untouched(lambda r: L.ctt_hip_field_op(dev.ctx, CID, 0, vp(d_pts.data_ptr()), vp(d_pts.data_ptr()), r, 1))
    untouched(lambda r: L.ctt_hip_fr_quotient(dev.ctx, CID, r, r, vp(d_ks.data_ptr()), vp(d_ks.data_ptr()), ks.ctypes.data_as(vp), 2))
    t = dev.submit("banderwagon", d_ks, d_pts, 2)
    with pytest.raises(ValueError):
        dev.finish(t, coord="jac")
    untouched(lambda r: L.ctt_hip_msm_device_finish(dev.ctx, t[1], 1, r))
    assert bw.aff_from(bytes(dev.finish(t, coord="aff"))) == bw.mul(7, bw.G)
    with pytest.raises(ValueError):
        dev.msm("banderwagon", d_ks, d_pts, 2, coord="jac")
    # sum_reduce and a window table work for the curve, or refuse with -1
    r = np.zeros(64, np.uint8)
    rc = L.ctt_hip_sum_reduce(dev.ctx, CID, 0, r.ctypes.data_as(vp), pts.ctypes.data_as(vp), 2, 0)
    assert rc == 0 and bw.aff_from(bytes(r)) == bw.mul(4, bw.G)
    from constantine_amd import CachedBases
    crs = bw.crs(64)
    cb = CachedBases("banderwagon", _pts(crs), ctx=dev.ctx, table=True)
    try:
        ks = [random.Random(8).randrange(bw.R) for _ in range(64)]
        assert _prj(cb.msm(_big(ks), coord="prj")) == bw.msm_fast(ks, crs)
    finally:
        cb.close()
