"""Batched Verkle commitments on the GPU (include/ctt_msm_hip.h part 4; csrc/verkle.hip): the fixed-base table, the commit kernel and the
finish kernel against the Python-integer oracle tests/_banderwagon.py, the reference's vectors, and the MSM pipeline's own result.

Expected values never come from the code under test.  Scalars are reduced mod 2r for arbitrary Banderwagon elements (the curve group
the law runs in holds the point (0, -1) of order two beside the subgroup of order r) and mod r for the synthetic multiples of G."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests import _verkle
from tests._verkle import check_outputs as _check, crafted_triples, expected_finish, fr_from, log_point as _log_point, map_fr
from tests._verkle import prj_bytes as _prj_bytes, pts_array as _pts

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOP = (1 << 253) - 1
NEUTRAL_PRJ = bw.fp_bytes(0) + bw.fp_bytes(1) + bw.fp_bytes(1)
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def torch_cuda():
    return _verkle.torch_with_gpu()


@pytest.fixture(scope="module")
def dev(torch_cuda):
    yield from _verkle.device_msm()


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(os.path.join(GOLDEN, "banderwagon_verkle.json")))
    return [int(h, 16) for h in d["commit_scalars"]], d["commitment"]


@pytest.fixture(scope="module")
def verkle_crs(dev):
    from constantine_amd import VerkleCrs
    pts = bw.crs(256)
    crs = VerkleCrs(_pts(pts), ctx=dev.ctx)
    yield pts, crs
    crs.close()


@pytest.fixture(scope="module")
def synth_crs(dev, torch_cuda):
    """256 synthetic points [s_j]G of known s_j, the table made from the device tensor"""
    yield from _verkle.synth_crs(dev, torch_cuda, 4242)


def _rows(rows, fr=False):
    enc = bw.fr_bytes if fr else bw.big_bytes
    return np.frombuffer(b"".join(enc(k) for row in rows for k in row), dtype=np.uint8).reshape(len(rows), len(rows[0]), 32).copy()


# --- 1. golden commitment -------------------------------------------------------------------------------------------------------------
def test_golden_commitment(verkle_crs, golden):
    from constantine_amd import multiScalarMul_vartime
    pts, crs = verkle_crs
    scalars, commitment = golden
    assert crs.window_bits in range(2, 11)
    expect = bw.msm_fast(scalars, pts)
    for fr in (False, True):
        coefs = _rows([scalars], fr)
        out = crs.commit(coefs, fr_coefs=fr)
        assert "0x" + bytes(out["ser"][0]).hex() == commitment
        assert bytes(out["prj"][0]) == bytes(multiScalarMul_vartime("banderwagon", coefs[0], _pts(pts), coord="prj", fr_coefs=fr))
        _check(out, 0, expect)
    rng = random.Random(1)
    other = [[rng.randrange(1 << 253) for _ in range(256)] for _ in range(2)]
    batch = [scalars, scalars, other[0], other[1], scalars]
    out = crs.commit(_rows(batch))
    for i in (0, 1, 4):
        _check(out, i, expect)
    _check(out, 2, bw.msm_fast(other[0], pts))


# --- 2. digits and windows ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def digit_cases():
    rng = random.Random(2)
    pts = [bw.msm_fast([rng.randrange(1, bw.R)], [bw.G]) for _ in range(15)] + [bw.add(bw.mul(rng.randrange(1, bw.R), bw.G), bw.T2)]
    rows = [[0] * 16]
    rows += [[1 if j == i else 0 for j in range(16)] for i in range(16)]
    rows += [[k if j == 5 else 0 for j in range(16)] for k in (bw.R - 1, bw.R, bw.R + 1, TOP)]
    rows += [[int.from_bytes(b"\x80" * 32, "little") & TOP] * 16, [TOP] * 16, [rng.randrange(1 << 253) for _ in range(16)]]
    expect = [bw.msm_fast([k % (2 * bw.R) for k in row], pts) for row in rows]
    assert expect[0] == bw.O and expect[1:17] == pts
    return pts, rows, expect


@pytest.mark.parametrize("c", [0, 2, 4, 5, 8, 10])
def test_digits_and_windows(dev, digit_cases, c):
    from constantine_amd import VerkleCrs
    pts, rows, expect = digit_cases
    with VerkleCrs(_pts(pts), ctx=dev.ctx, window_bits=c) as crs:
        assert crs.window_bits == (c or crs.window_bits) and 2 <= crs.window_bits <= 10
        out = crs.commit(_rows(rows))
        for i, pt in enumerate(expect):
            _check(out, i, pt)
        assert bytes(out["prj"][0]) == NEUTRAL_PRJ and bytes(out["ser"][0]) == bytes(32) and bytes(out["fr"][0]) == bytes(32)
        frrows = [[k % bw.R for k in row] for row in rows[17:]]
        out = crs.commit(_rows(frrows, fr=True), fr_coefs=True, want=("prj",))
        assert list(out) == ["prj"]
        for i, row in enumerate(frrows):
            assert bytes(out["prj"][i]) == _prj_bytes(bw.msm_fast(row, pts)), i


# --- 3. lane edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 255, 256])
def test_lane_edges(dev, synth_crs, n):
    from constantine_amd import VerkleCrs
    d_pts, logs, full = synth_crs
    rng = random.Random(30 + n)
    rows = [[rng.randrange(1 << 253) for _ in range(n)] for _ in range(3)]
    expect = [_log_point(sum(k * s for k, s in zip(row, logs))) for row in rows]
    crs = full if n == 256 else VerkleCrs(d_pts[:n].cpu().numpy(), ctx=dev.ctx)
    try:
        out = crs.commit(_rows(rows))
        for i, pt in enumerate(expect):
            _check(out, i, pt)
    finally:
        if crs is not full:
            crs.close()


def test_cancellation_and_special_points(dev):
    from constantine_amd import VerkleCrs
    P = bw.mul(987654321, bw.G)
    Q = bw.add(P, bw.T2)
    pts = [P, bw.neg(P), bw.O, bw.T2, Q]
    rows = [[9, 9, 0, 0, 0], [TOP - 5, TOP - 5, 0, 0, 0], [9, 9, 4, 0, 0], [9, 9, 0, 1, 0], [9, 9, 0, 0, 12], [3, 5, 7, 11, 13],
            [0, 0, 6, 2, 0], [0, 0, 1, 3, 0]]
    with VerkleCrs(_pts(pts), ctx=dev.ctx) as crs:
        out = crs.commit(_rows(rows))
    for i, row in enumerate(rows):
        _check(out, i, bw.msm(row, pts))
    for i in (0, 1, 2, 6):
        assert bytes(out["prj"][i]) == NEUTRAL_PRJ, i
    assert bytes(out["prj"][3]) == _prj_bytes(bw.T2) and bytes(out["ser"][3]) == bytes(32)


def test_refused_sizes_and_arguments(dev, verkle_crs):
    from constantine_amd import _lib
    L = _lib.lib()
    pts = _pts(bw.crs(2) * 129)[:257].copy()
    for n, c in ((257, 0), (0, 0), (2, 1), (2, 11)):
        assert L.ctt_hip_verkle_crs_create(dev.ctx, pts.ctypes.data_as(VP), n, c, 0) is None
        assert L.ctt_hip_last_error() == -1
    _, crs = verkle_crs
    coefs = np.zeros((1, 256, 32), np.uint8)
    out = np.full(96, 0xAB, np.uint8)
    o, cp = out.ctypes.data_as(VP), coefs.ctypes.data_as(VP)
    other = L.ctt_hip_msm_ctx_create(0)
    try:
        assert L.ctt_hip_verkle_commit_batch(other, crs.handle, 0, o, None, None, cp, 1, 0) == -1     # a crs of another context
    finally:
        L.ctt_hip_msm_ctx_destroy(other)
    assert L.ctt_hip_verkle_commit_batch(dev.ctx, None, 0, o, None, None, cp, 1, 0) == -1
    assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 0, None, None, None, cp, 1, 0) == -1
    assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 2, o, None, None, cp, 1, 0) == -1
    assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 0, o, None, None, cp, 1 << 18, 0) == -1    # 2^31 bytes of coefficients
    assert L.ctt_hip_last_error() == -1
    assert L.ctt_hip_banderwagon_map_to_fr_batch(dev.ctx, o, cp, (1 << 31) // 96 + 1, 0) == -1
    assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 0, o, None, None, cp, 0, 0) == 0           # m = 0 writes nothing
    assert bytes(out) == bytes([0xAB]) * 96


# --- 4. batch edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 257])
def test_batch_edges_host_and_device(torch_cuda, synth_crs, m):
    _, logs, crs = synth_crs
    rng = random.Random(400 + m)
    rows = [[rng.randrange(1 << 253) for _ in range(256)] for _ in range(m)]
    expect = [_log_point(sum(k * s for k, s in zip(row, logs))) for row in rows]
    coefs = _rows(rows)
    host = crs.commit(coefs)
    for i, pt in enumerate(expect):
        _check(host, i, pt)
    d_out = crs.commit(torch_cuda.from_numpy(coefs).cuda())
    for key in ("prj", "ser", "fr"):
        assert d_out[key].is_cuda and bytes(d_out[key].cpu().numpy()) == bytes(host[key]), key


def test_output_subsets_leave_the_rest_untouched(torch_cuda, dev, synth_crs):
    from constantine_amd import _lib
    L = _lib.lib()
    _, logs, crs = synth_crs
    rng = random.Random(44)
    m = 9
    rows = [[rng.randrange(1 << 253) for _ in range(256)] for _ in range(m)]
    coefs = _rows(rows)
    full = crs.commit(coefs)
    _check(full, m - 1, _log_point(sum(k * s for k, s in zip(rows[m - 1], logs))))
    d_coefs = torch_cuda.from_numpy(coefs).cuda()
    widths = (96, 32, 32)
    for mask in range(1, 8):
        host = [np.full((m, w), 0xC3, np.uint8) for w in widths]
        devb = [torch_cuda.full((m, w), 0xC3, dtype=torch_cuda.uint8, device="cuda") for w in widths]
        torch_cuda.cuda.synchronize()
        hp = [a.ctypes.data_as(VP) if mask >> i & 1 else None for i, a in enumerate(host)]
        dp = [VP(t.data_ptr()) if mask >> i & 1 else None for i, t in enumerate(devb)]
        assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 0, hp[0], hp[1], hp[2], coefs.ctypes.data_as(VP), m, 0) == 0
        assert L.ctt_hip_verkle_commit_batch(dev.ctx, crs.handle, 0, dp[0], dp[1], dp[2], VP(d_coefs.data_ptr()), m, 1) == 0
        for i, key in enumerate(("prj", "ser", "fr")):
            want = bytes(full[key]) if mask >> i & 1 else bytes([0xC3]) * (m * widths[i])
            assert bytes(host[i]) == want and bytes(devb[i].cpu().numpy()) == want, (mask, key)


# --- 5. the standalone map and serialise symbols --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finish_cases():
    """crafted triples (tests/_verkle.py), zero Y / zero Z entries, and 1000 points of a walk R + iQ in extended coordinates (any Z)"""
    rng = random.Random(5)
    triples = crafted_triples()
    lam = rng.randrange(1, bw.P)
    triples[3] = (5 * lam % bw.P, 0, lam)
    triples[12] = (7, 9, 0)
    triples[16] = (0, 0, 0)
    q = bw.mul(rng.randrange(1, bw.R), bw.G)
    q = (q[0], q[1], 1, q[0] * q[1] % bw.P)
    r = (0, 1, 1, 0)
    for _ in range(1000):
        r = bw._xadd(r, q)
        lam = rng.randrange(1, bw.P)
        triples.append((r[0] * lam % bw.P, r[1] * lam % bw.P, r[2] * lam % bw.P))
    return triples, [expected_finish(t) for t in triples]


def _triples(ts):
    return np.frombuffer(b"".join(bw.fp_bytes(v) for t in ts for v in t), dtype=np.uint8).reshape(-1, 96).copy()


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 1000, 1055])
def test_map_and_serialize_batches(torch_cuda, finish_cases, m):
    from constantine_amd import batchMapToScalarField, serializeBatch_vartime
    triples, expect = finish_cases
    lo = 0 if m in (63, 64, 65, 1055) else 55          # the crafted ones in front, or random points only
    src = _triples(triples[lo:lo + m])
    fr, ser = batchMapToScalarField(src), serializeBatch_vartime(src)
    for i in range(m):
        assert bytes(ser[i]) == expect[lo + i][1] and fr_from(bytes(fr[i])) == expect[lo + i][2], (m, i)
    d_src = torch_cuda.from_numpy(src).cuda()
    assert bytes(batchMapToScalarField(d_src).cpu().numpy()) == bytes(fr)
    assert bytes(serializeBatch_vartime(d_src).cpu().numpy()) == bytes(ser)


def test_serialisation_identifies_the_two_representatives():
    from constantine_amd import batchMapToScalarField, serializeBatch_vartime
    rng = random.Random(6)
    pts = [bw.mul(rng.randrange(1, bw.R), bw.G) for _ in range(4)]
    ts = []
    for x, y in pts:
        z1, z2, z3 = (rng.randrange(1, bw.P) for _ in range(3))
        ts += [(x * z1 % bw.P, y * z1 % bw.P, z1), (-x * z2 % bw.P, -y * z2 % bw.P, z2), (-x * z3 % bw.P, y * z3 % bw.P, z3)]
    ser, fr = serializeBatch_vartime(_triples(ts)), batchMapToScalarField(_triples(ts))
    for i, p in enumerate(pts):
        assert bytes(ser[3 * i]) == bytes(ser[3 * i + 1]) == bw.serialize(p)       # (x, y) and (-x, -y): one element
        assert bytes(ser[3 * i + 2]) == bw.serialize(bw.neg(p)) != bytes(ser[3 * i])  # -P is another
        assert fr_from(bytes(fr[3 * i])) == fr_from(bytes(fr[3 * i + 1])) == map_fr(p)


def test_reference_map_vectors():
    from constantine_amd import batchMapToScalarField, serializeBatch_vartime
    d = json.load(open(os.path.join(GOLDEN, "banderwagon_map_to_field.json")))
    pts = [bw.mul(k, bw.G) for k, _ in d["multiples_of_g"]] + [bw.deserialize(bytes.fromhex(p[2:])) for p, _ in d["serialized"]]
    want = [int(h, 16) for _, h in d["multiples_of_g"]] + [int(h, 16) for _, h in d["serialized"]]
    src = _triples([(x * 3 % bw.P, y * 3 % bw.P, 3) for x, y in pts])
    assert [fr_from(bytes(b)) for b in batchMapToScalarField(src)] == want
    assert "0x" + bytes(serializeBatch_vartime(src)[2]).hex() == d["serialized"][0][0]


# --- 6. coexistence with MSM tickets --------------------------------------------------------------------------------------------------
def test_commit_between_outstanding_msm_tickets(torch_cuda, dev, synth_crs):
    d_pts, logs, crs = synth_crs
    rng = random.Random(66)
    ks = [[rng.randrange(1 << 253) for _ in range(256)] for _ in range(3)]
    big = [torch_cuda.from_numpy(_rows([k])[0]).cuda() for k in ks]
    expect = [_log_point(sum(k * s for k, s in zip(row, logs))) for row in ks]
    t0 = dev.submit("banderwagon", big[0], d_pts, 256)
    t1 = dev.submit("banderwagon", big[1], d_pts, 256)
    out = crs.commit(_rows([ks[2], ks[0]]))
    r1, r0 = dev.finish(t1, coord="prj"), dev.finish(t0, coord="prj")
    assert bytes(r0) == _prj_bytes(expect[0]) and bytes(r1) == _prj_bytes(expect[1])
    _check(out, 0, expect[2])
    _check(out, 1, expect[0])
