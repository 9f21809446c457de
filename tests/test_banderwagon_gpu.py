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


# ----------------------------------------------------------------------------------------------
# The layers the short-Weierstrass curves reach through tests/test_gpu_parity.py: explicit plans, skewed digits, host symbols
# uploading in slices (k_accum<FD, INTO>: a code object of its own), sharding over contexts, window tables, ragged sizes, tickets.
# Expected values: the points of gen_points are [s_i]G with s_i = bw.synth_log(seed, i), so the MSM is [sum k_i s_i mod r]G -- one
# scalar multiplication of the Python oracle that does not depend on plan, slicing or sharding; bw.msm_fast where no logarithm is known.
# ----------------------------------------------------------------------------------------------
_LOGS = {}


def _logs(seed, n):
    have = _LOGS.get(seed, [])
    if len(have) < n:
        have = _LOGS[seed] = have + [bw.synth_log(seed, j) for j in range(len(have), n)]
    return have[:n]


def _rand_scalars(seed, n):
    """(n, 32) bytes of uniform 253-bit scalars (about a quarter of them >= r)"""
    sc = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return sc


def _ints(sc):
    return [int.from_bytes(row.tobytes(), "little") for row in sc]


def _by_logs(sc, logs):
    """[sum k_i s_i mod r]G for scalar bytes or integers"""
    ks = _ints(sc) if isinstance(sc, np.ndarray) else sc
    return bw.mul(sum(k * s for k, s in zip(ks, logs)) % bw.R, bw.G)


def _neg_rows(pts):
    """the affine records of -P for records of P: (x, y) -> (p - x, y), which is the same map on Montgomery residues"""
    out = pts.copy()
    for j in range(pts.shape[0]):
        x = int.from_bytes(pts[j, :32].tobytes(), "little")
        out[j, :32] = np.frombuffer(((bw.P - x) % bw.P).to_bytes(32, "little"), dtype=np.uint8)
    return out


def _set_default(key, value):
    """an option of the default context, the one the host-pointer symbols and CachedBases(ctx=None) use"""
    from constantine_amd import _lib
    assert _lib.lib().ctt_hip_msm_set_option(None, key.encode(), int(value)) == 0


def test_window_sizes_and_lane_spans(dev, torch_cuda):
    """Same element for every plan: window bits (11 divides the scalar width 253: the extra top window), entries per lane, sort
    slices; the first 50 scalars have their top bits on."""
    n, seed = 5000, 91
    d_pts = _synth(dev, torch_cuda, seed, n)
    sc = _rand_scalars(92, n)
    sc[:50, 24:31] = 0xFF
    sc[:50, 31] = 0x1F
    expect = _by_logs(sc, _logs(seed, n))
    ds = _to_dev(torch_cuda, sc)
    try:
        for c, K, S in ((3, 4, 0), (5, 8, 64), (8, 16, 1000), (11, 0, 0), (11, 8, 64), (13, 0, 0), (15, 12, 3000), (16, 0, 0), (0, 0, 0)):
            dev.set_option("c", c)
            dev.set_option("K", K)
            dev.set_option("S", S)
            assert bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff"))) == expect, (c, K, S, dev.last_plan())
    finally:
        dev.set_option("c", 0)
        dev.set_option("K", 0)
        dev.set_option("S", 0)


def test_horner_groups_and_merge_without_host_wait(dev, torch_cuda):
    """The bit Horner of a window cut into groups of hb bits (one quad of lanes each -- for this curve lane 0 of the quad adds alone),
    and the head merge deciding on the device how far its tree goes: same element for every group size, for uniform digits and for
    the inputs whose head chains are far longer than the steps the plan enqueues (all scalars equal; a quarter of them equal)."""
    n, seed = 60000, 191
    d_pts = _synth(dev, torch_cuda, seed, n)
    logs = _logs(seed, n)
    sc = _rand_scalars(192, n)
    sc_eq = np.tile(sc[:1], (n, 1))
    sc_q = sc.copy()
    sc_q[::4] = sc[1]
    try:
        for label, s in (("uniform", sc), ("all equal", sc_eq), ("quarter equal", sc_q)):
            expect = _by_logs(s, logs)
            ds = _to_dev(torch_cuda, s)
            for c, hb, K in ((0, 0, 0), (13, 1, 0), (13, 3, 8), (16, 2, 0), (16, 15, 0), (9, 4, 4), (11, 8, 0), (15, 5, 12)):
                dev.set_option("c", c)
                dev.set_option("K", K)
                dev.set_option("horner_bits", hb)
                got = bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff")))
                assert got == expect, (label, c, hb, K, dev.last_plan())
        # more than 16 groups per window: the groups beyond a workgroup's 16 quads run in further blocks
        expect = _by_logs(sc, logs)
        ds = _to_dev(torch_cuda, sc)
        for c, hb, hws in ((18, 1, 0), (19, 1, 0), (20, 1, 0), (20, 0, 1), (18, 0, 1), (20, 2, 0)):
            dev.set_option("c", c)
            dev.set_option("K", 0)
            dev.set_option("horner_bits", hb)
            dev.set_option("host_window_sums", hws)
            got = bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff")))
            assert got == expect, (c, hb, hws, dev.last_plan())
    finally:
        for k in ("c", "K", "horner_bits", "host_window_sums"):
            dev.set_option(k, 0)


def test_sort_under_skewed_digit_distributions(dev, torch_cuda):
    """The two-pass bucket sort must not depend on the digits being uniform: giant buckets, groups several tiles long, medium
    buckets straddling a tile end -- and the accumulation behind it sees buckets of a hundred thousand points of this law."""
    n, seed = 1 << 18, 311
    d_pts = _synth(dev, torch_cuda, seed, n)
    logs = _logs(seed, n)
    rng = np.random.default_rng(7)
    uni = _rand_scalars(312, n)
    cases = {"uniform": uni}
    cases["five distinct scalars"] = uni[:5][rng.integers(0, 5, n)]
    some = uni[:100]
    cases["hundred distinct scalars"] = some[rng.integers(0, 100, n)]
    low = uni.copy()
    low[:, 1::2] &= 0x1F          # every 16-bit chunk < 2^13: three quarters of the bucket range stay empty
    cases["low quarter of the bucket range"] = low
    mix = uni.copy()
    mix[: n // 2] = some[rng.integers(0, 100, n // 2)]
    cases["half uniform, half repeated"] = mix
    try:
        for label, sc in cases.items():
            sc = np.ascontiguousarray(sc)
            expect = _by_logs(sc, logs)
            ds = _to_dev(torch_cuda, sc)
            for c in (0, 12):
                dev.set_option("c", c)
                assert bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff"))) == expect, (label, c)
            for staged, xcd in ((0, 0), (0, 1), (2, 0), (2, 1)):
                dev.set_option("sort_staged", staged)
                dev.set_option("sort_xcd", xcd)
                for c in (0, 13):
                    dev.set_option("c", c)
                    assert bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff"))) == expect, (label, c, staged, xcd)
            dev.set_option("sort_staged", 1)
            dev.set_option("sort_xcd", 1)
    finally:
        dev.set_option("c", 0)
        dev.set_option("sort_staged", 1)
        dev.set_option("sort_xcd", 1)


def test_host_symbols_upload_in_slices(dev, torch_cuda):
    """The host-pointer symbols upload the pairs in slices underneath the accumulation (MsmEngine::submit_host): ONE bucket set,
    k_accum<FD, INTO> resumes from the stored sums -- for this curve by XYZZ::is_inf() on a record whose neutral, once a bucket has
    cancelled, is (0 : c : c : 0) and not the all-zero one.  Same element for 1, 2, 3, 4, 8 slices and the automatic choice, through
    the big- and the Fr-coefficient Constantine symbols; and an input whose second half cancels every bucket of the first."""
    from constantine_amd import multiScalarMul_vartime
    try:
        for n in ((1 << 18) + 3, 40000):
            seed = 600 + n
            pts = _synth(dev, torch_cuda, seed, n).cpu().numpy()
            logs = _logs(seed, n)
            sc = _rand_scalars(601 + n, n)
            ks = _ints(sc)
            expect = _by_logs(ks, logs)
            fr = _fr([k % bw.R for k in ks])
            for chunks in ((0, 1, 2, 3, 4, 8) if n > 100000 else (0, 2, 3)):
                _set_default("chunks", chunks)
                assert _prj(multiScalarMul_vartime("banderwagon", sc, pts, coord="prj")) == expect, (n, chunks, "big")
                assert _prj(multiScalarMul_vartime("banderwagon", fr, pts, coord="prj", fr_coefs=True)) == expect, (n, chunks, "fr")
        # the second half is the first half with every point negated and the same scalars: whatever the first slices stored, the last
        # ones cancel -- every bucket ends as the law's neutral, and so does the sum
        h = (1 << 17) + 1
        half = _synth(dev, torch_cuda, 77, h).cpu().numpy()
        pts = np.concatenate([half, _neg_rows(half)])
        sc = _rand_scalars(78, h)
        sc = np.concatenate([sc, sc])
        for chunks in (0, 1, 2, 3, 8):
            _set_default("chunks", chunks)
            r = multiScalarMul_vartime("banderwagon", sc, pts, coord="prj")
            assert [bw.fp_from(bytes(r)[i:i + 32]) for i in (0, 32, 64)] == [0, 1, 1], chunks
        # ... and a third part after the cancelled two: the buckets go on from the stored neutral
        t = 50001
        third = _synth(dev, torch_cuda, 79, t).cpu().numpy()
        sc3 = _rand_scalars(80, t)
        for chunks in (0, 3, 5):
            _set_default("chunks", chunks)
            r = multiScalarMul_vartime("banderwagon", np.concatenate([sc, sc3]), np.concatenate([pts, third]), coord="prj")
            assert _prj(r) == _by_logs(sc3, _logs(79, t)), chunks
    finally:
        _set_default("chunks", 0)


def test_host_symbols_shard_over_contexts(dev, torch_cuda):
    """In-library sharding on one device: two (three) contexts on device 0, the symbols cut the call into balanced slices, one host
    thread per context, and the partial results are added on the host (ec_sum_affine: the Edwards law there too)."""
    from constantine_amd import multiScalarMul_vartime, set_devices, set_shard_min
    try:
        set_shard_min(1000)
        for devices, n in (([0, 0], 70001), ([0, 0, 0], 70001), ([0, 0], 1500), ([0, 0, 0], 1500)):   # 1500 < 2 x shard_min: one context
            set_devices(devices)
            seed = 900 + n
            pts = _synth(dev, torch_cuda, seed, n).cpu().numpy()
            sc = _rand_scalars(901 + n, n)
            ks = _ints(sc)
            expect = _by_logs(ks, _logs(seed, n))
            assert _prj(multiScalarMul_vartime("banderwagon", sc, pts, coord="prj")) == expect, (devices, n)
            m = min(n, 4000)
            got = multiScalarMul_vartime("banderwagon", _fr([k % bw.R for k in ks[:m]]), pts[:m], coord="aff", fr_coefs=True)
            assert bw.aff_from(bytes(got)) == _by_logs(ks[:m], _logs(seed, m)), (devices, n, "fr")
    finally:
        set_devices([])
        set_shard_min(1 << 15)


@pytest.mark.parametrize("n", [16385, 40000, 100003, (1 << 20) + 7])
def test_sizes_that_are_not_powers_of_two(dev, torch_cuda, n):
    """Pair counts that are not powers of two (ragged last partition block, groups of uneven size), device-resident and over a
    window table of the same points."""
    from constantine_amd import CachedBases
    seed = 411
    d_pts = _synth(dev, torch_cuda, seed, n)
    sc = _rand_scalars(412 + n, n)
    expect = _by_logs(sc, _logs(seed, n))
    ds = _to_dev(torch_cuda, sc)
    assert bw.aff_from(bytes(dev.msm("banderwagon", ds, d_pts, n, coord="aff"))) == expect
    cb = CachedBases("banderwagon", d_pts, ctx=dev.ctx, on_device=True, table=True)
    try:
        assert cb.window_bits > 0
        assert _prj(cb.msm(ds, coord="prj")) == expect
        assert _prj(cb.msm(sc, coord="prj")) == expect          # host-resident coefficients over the table
    finally:
        cb.close()


def test_window_table_cached_bases(dev, torch_cuda):
    """ctt_hip_msm_bases_create_table over 20000 bases: automatic and explicit window bits (5: many windows and long bucket chains;
    11 divides the scalar width: the extra window), prefixes of the bases, a base (0, 1) -- which table_next_body doubles like any
    point --, a repeated pair, both forms of the merged sort's second sweep, Fr Montgomery coefficients, all-zero scalars."""
    from constantine_amd import CachedBases
    n, seed = 20000, 911
    pts = _synth(dev, torch_cuda, seed, n).cpu().numpy()
    logs = list(_logs(seed, n))
    pts[11], logs[11] = _pts([bw.O])[0], 0
    pts[13], logs[13] = pts[12], logs[12]
    for wb in (0, 5, 11, 15):
        bases = CachedBases("banderwagon", pts, table=True, window_bits=wb)
        try:
            assert bases.window_bits == wb or (wb == 0 and bases.window_bits > 0)
            for s, m in ((1, n), (3, n // 3), (4, 1)):
                sc = _rand_scalars(s, m)
                if m > 13:
                    sc[13] = sc[12]
                expect = _by_logs(sc, logs[:m])
                assert _prj(bases.msm(sc, coord="prj")) == expect, (wb, m)
                try:
                    for staged in (0, 2):
                        _set_default("sort_staged", staged)
                        assert _prj(bases.msm(sc, coord="prj")) == expect, (wb, m, staged)
                finally:
                    _set_default("sort_staged", 1)
            ks = _ints(_rand_scalars(5, n))
            got = bases.msm(_fr([k % bw.R for k in ks]), coord="aff", fr_coefs=True)
            assert bw.aff_from(bytes(got)) == _by_logs(ks, logs), wb
            r = bases.msm(np.zeros((n, 32), np.uint8), coord="prj")
            assert [bw.fp_from(bytes(r)[i:i + 32]) for i in (0, 32, 64)] == [0, 1, 1], wb
        finally:
            bases.close()


def test_all_equal_points_and_all_equal_scalars(dev, torch_cuda):
    """One point everywhere (every addition inside a bucket is P + P or kP + P: the unified law has to be right where the Weierstrass
    one branches to its doubling), then one scalar everywhere too; and one scalar over distinct points (one bucket per window)."""
    n = 22529
    one = _synth(dev, torch_cuda, 51, 1)
    d_pts = one.repeat(n, 1).contiguous()
    log = bw.synth_log(51, 0)
    sc = _rand_scalars(52, n)
    got = dev.msm("banderwagon", _to_dev(torch_cuda, sc), d_pts, n, coord="aff")
    assert bw.aff_from(bytes(got)) == bw.mul(sum(_ints(sc)) * log % bw.R, bw.G)
    sc_eq = np.tile(sc[:1], (n, 1))
    got = dev.msm("banderwagon", _to_dev(torch_cuda, sc_eq), d_pts, n, coord="aff")
    assert bw.aff_from(bytes(got)) == bw.mul(_ints(sc[:1])[0] * n * log % bw.R, bw.G)
    n = 20000
    d_pts = _synth(dev, torch_cuda, 53, n)
    sc_eq = np.tile(_rand_scalars(54, 1), (n, 1))
    got = dev.msm("banderwagon", _to_dev(torch_cuda, sc_eq), d_pts, n, coord="aff")
    assert bw.aff_from(bytes(got)) == _by_logs(sc_eq, _logs(53, n))


def test_unknown_logs_at_size(dev, torch_cuda):
    """Points nobody knows the logarithm of, 2^18 pairs: 1024 points of the Verkle CRS generator (past the 256 of the commitment),
    tiled and permuted, with independent 253-bit scalars (a quarter of them >= r); the pairs of one point collapse to one scalar, so
    the expected element is an MSM of 1024 pairs in the Python oracle.  The collapsed scalars are reduced mod 2r, not mod r: a
    deserialised Banderwagon point is a subgroup point or one plus (0, -1), so its order divides 2r, and the comparison is of curve
    points, not of classes modulo (0, -1).  Oracle side alone, measured on one CPU core:
    9.2 s (bw.crs 5.8 s, bw.msm_fast 3.4 s)."""
    from constantine_amd import multiScalarMul_vartime
    m, n = 1024, 1 << 18
    crs = bw.crs(m, skip=256)
    owner = np.random.default_rng(4242).permutation(np.arange(n) % m)     # pair j carries point owner[j]
    pts = _pts(crs)[owner]
    sc = _rand_scalars(4243, n)
    sums = [0] * m
    for k, i in zip(_ints(sc), owner.tolist()):
        sums[i] += k
    expect = bw.msm_fast([s % (2 * bw.R) for s in sums], crs)
    got = dev.msm("banderwagon", _to_dev(torch_cuda, sc), _to_dev(torch_cuda, pts), n, coord="aff")
    assert bw.aff_from(bytes(got)) == expect
    assert _prj(multiScalarMul_vartime("banderwagon", sc, pts, coord="prj")) == expect


def test_three_banderwagon_tickets_in_flight(dev, torch_cuda):
    """Three tickets of the curve outstanding together, finished out of order, sizes 3000, 70000 and 1: on plain device inputs and
    on cached bases (a prefix of them per ticket)."""
    from constantine_amd import CachedBases
    sizes, seed = (3000, 70000, 1), 195
    nmax = max(sizes)
    d_pts = _synth(dev, torch_cuda, seed, nmax)
    scs = [_rand_scalars(196 + i, m) for i, m in enumerate(sizes)]
    dss = [_to_dev(torch_cuda, s) for s in scs]
    expect = [_by_logs(s, _logs(seed, m)) for s, m in zip(scs, sizes)]
    t = [dev.submit("banderwagon", dss[i], d_pts, sizes[i]) for i in range(3)]
    assert bw.aff_from(bytes(dev.finish(t[2], coord="aff"))) == expect[2]
    assert _prj(dev.finish(t[0], coord="prj")) == expect[0]
    assert bw.aff_from(bytes(dev.finish(t[1], coord="aff"))) == expect[1]
    cb = CachedBases("banderwagon", d_pts, ctx=dev.ctx, on_device=True)
    try:
        t = [cb.submit(dss[i], sizes[i]) for i in range(3)]
        assert _prj(cb.finish(t[1], coord="prj")) == expect[1]
        assert bw.aff_from(bytes(cb.finish(t[2], coord="aff"))) == expect[2]
        assert _prj(cb.finish(t[0], coord="prj")) == expect[0]
    finally:
        cb.close()


# ----------------------------------------------------------------------------------------------
# the forms the defaults never take (tests/test_gpu_parity.py has the short Weierstrass curves)
# ----------------------------------------------------------------------------------------------
MERGE_OPTION_DEFAULTS = {"c": 0, "K": 0, "merge_chain": 0, "merge_queue_quad": 0, "merge_lmax": 0}


def test_forced_merge_forms(dev, torch_cuda):
    """Both forms of the head merge by option -- merge_chain 1 (queue) / 2 (tree) x merge_queue_quad 0 / 2 (one lane per chain) x
    merge_lmax 0 (= 8), 1, 2, 64 -- under the automatic plan, a plan with few buckets and few entries per lane (chains of hundreds of
    heads) and c = 16; uniform scalars, all equal, a quarter equal, all points equal, all points and scalars equal.  In the four-lane
    kernels lane 0 of a quad runs the unified law alone for this curve; the one-lane queue kernel and k_merge_long run nowhere else."""
    n, seed = 60000, 2300
    d_pts = _synth(dev, torch_cuda, seed, n)
    logs = _logs(seed, n)
    d_one = d_pts[:1].repeat(n, 1).contiguous()
    sc = _rand_scalars(2301, n)
    sc_eq = np.tile(sc[:1], (n, 1))
    sc_q = sc.copy()
    sc_q[::4] = sc[1]
    inputs = [("uniform", sc, d_pts, _by_logs(sc, logs)), ("all scalars equal", sc_eq, d_pts, _by_logs(sc_eq, logs)),
              ("a quarter equal", sc_q, d_pts, _by_logs(sc_q, logs)),
              ("all points equal", sc, d_one, bw.mul(sum(_ints(sc)) * logs[0] % bw.R, bw.G)),
              ("all points and scalars equal", sc_eq, d_one, bw.mul(_ints(sc[:1])[0] * n * logs[0] % bw.R, bw.G))]
    try:
        for label, s, dp, expect in inputs:
            ds = _to_dev(torch_cuda, s)
            for k, v in MERGE_OPTION_DEFAULTS.items():
                dev.set_option(k, v)
            default = bytes(dev.msm("banderwagon", ds, dp, n, coord="aff"))
            assert bw.aff_from(default) == expect, (label, dev.last_plan())
            for c, K in ((0, 0), (6, 4), (16, 0)):
                dev.set_option("c", c)
                dev.set_option("K", K)
                for mc in (1, 2):
                    for mq in (0, 2):
                        for ml in (0, 1, 2, 64):
                            dev.set_option("merge_chain", mc)
                            dev.set_option("merge_queue_quad", mq)
                            dev.set_option("merge_lmax", ml)
                            got = bytes(dev.msm("banderwagon", ds, dp, n, coord="aff"))
                            assert bw.aff_from(got) == expect and got == default, (label, c, K, mc, mq, ml, dev.last_plan())
    finally:
        for k, v in MERGE_OPTION_DEFAULTS.items():
            dev.set_option(k, v)


@pytest.mark.parametrize("quad", ["0", "2000000000"])
def test_reduction_all_wide_or_all_narrow(quad, torch_cuda):
    """Contexts created under $CTT_HIP_MSM_QUAD = 0 (every reduction pass through k_pyr) and above any pass (every pass through
    k_pyr_quad, where lane 0 of a quad adds alone for this curve): 2^16 pairs, uniform inputs and all points equal."""
    from constantine_amd import DeviceMsm
    n, seed = 1 << 16, 2400
    old = os.environ.get("CTT_HIP_MSM_QUAD")
    os.environ["CTT_HIP_MSM_QUAD"] = quad
    try:
        eng = DeviceMsm(0)
    finally:
        if old is None:
            os.environ.pop("CTT_HIP_MSM_QUAD", None)
        else:
            os.environ["CTT_HIP_MSM_QUAD"] = old
    try:
        d_pts = _synth(eng, torch_cuda, seed, n)
        logs = _logs(seed, n)
        sc = _rand_scalars(2401, n)
        ds = _to_dev(torch_cuda, sc)
        for label, dp, expect in (("uniform", d_pts, _by_logs(sc, logs)),
                                  ("all points equal", d_pts[:1].repeat(n, 1).contiguous(), bw.mul(sum(_ints(sc)) * logs[0] % bw.R, bw.G))):
            for _ in range(2):
                assert bw.aff_from(bytes(eng.msm("banderwagon", ds, dp, n, coord="aff"))) == expect, (label, quad, eng.last_plan())
    finally:
        eng.close()
