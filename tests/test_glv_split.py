"""
The endomorphism split of BLS12-381 G1 on the CPU: the split body of msm_bodies.h (bls12_381_glv_split) against Python integers, and
the whole emulated pipeline with the split on (tests/emu/glv_emu.cpp: the emulator's backend plus the front body and 4-word scalars,
under the same host orchestration as the GPU engine) against the big-integer oracle oracle/pyoracle.py.

phi(x, y) = (beta x, y) = [mu](x, y) with mu = -x^2 mod r (x the curve parameter): every scalar k becomes s1 k1 + s2 k2 mu (mod r)
with k1, k2 < 2^127, and an MSM over n pairs one over the 2n points s1 P, s2 phi(P) with 127-bit scalars -- half the bucket sets.
"""
import ctypes
import fcntl
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.emu import emu

NAME = "bls12_381_g1"
CURVE = po.CURVES[NAME]
R = CURVE.order
X = 0xd201000000010000          # |x| of BLS12-381
X2 = X * X
MU = (-X2) % R


_glv = None


def glv_lib():
    """tests/emu/glv_emu.cpp as a library of its own, built once (one builder at a time, as tests/emu/emu.py does)"""
    global _glv
    if _glv is None:
        src = os.path.join(emu.HERE, "glv_emu.cpp")
        bdir = os.path.join(emu.HERE, "build")
        out = os.path.join(bdir, "libglv_emu.so")
        os.makedirs(bdir, exist_ok=True)
        csrc = os.path.join(emu.ROOT, "constantine_amd", "csrc")
        deps = [src, os.path.join(emu.HERE, "msm_emu.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(bdir, ".glv.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, src, "-o", out + ".tmp"])
                os.replace(out + ".tmp", out)
        L = ctypes.CDLL(out)
        vp, sz, i32, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
        L.emu_glv_msm.argtypes = [i32, i32, vp, vp, vp, sz, i32, i32, i32, i32, vp]
        L.emu_glv_msm_slots.argtypes = [vp, vp, vp, sz, vp, vp, sz, i32]
        L.emu_glv_split.argtypes = [vp, u32, vp]
        _glv = L
    return _glv


def glv_msm(sc, pts, glv, coef_is_fr=False, c=0, K=0, S=0):
    sc = np.ascontiguousarray(sc, dtype=np.uint8)
    pts = np.ascontiguousarray(pts, dtype=np.uint8)
    out = np.zeros(emu.AFF_BYTES[NAME], dtype=np.uint8)
    plan = np.zeros(8, dtype=np.int32)
    assert glv_lib().emu_glv_msm(int(coef_is_fr), 0, emu._p(out), emu._p(sc), emu._p(pts), sc.shape[0], c, K, S, glv, emu._p(plan)) == 0
    return out, plan


def test_constants():
    assert R == X2 * X2 - X2 + 1
    assert (MU * MU + MU + 1) % R == 0          # a primitive cube root of unity mod r: the eigenvalue of phi


def _split(ks):
    """bls12_381_glv_split of every k (any value below 2^255): [(s1, k1, s2, k2)] with signs +1 / -1"""
    L = glv_lib()
    buf = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint32).reshape(len(ks), 8).copy()
    out = np.full((len(ks), 10), 0xA5A5A5A5, dtype=np.uint32)
    assert L.emu_glv_split(emu._p(buf), len(ks), emu._p(out)) == 0
    res = []
    for row in out:
        k1 = sum(int(w) << (32 * i) for i, w in enumerate(row[0:4]))
        k2 = sum(int(w) << (32 * i) for i, w in enumerate(row[4:8]))
        assert int(row[8]) in (0, 1) and int(row[9]) in (0, 1)
        res.append((-1 if row[8] else 1, k1, -1 if row[9] else 1, k2))
    return res


EDGE = [0, 1, 2, R - 1, R, R + 1, (R - 1) // 2, (R + 1) // 2, X2, X2 - 1, X2 + 1, 1 << 127, (1 << 128) - 1, (1 << 255) - 1]


def test_split_body_vs_python_integers():
    rng = random.Random(0x61F5)
    ks = EDGE + [rng.getrandbits(255) for _ in range(2000)]
    largest = 0
    for k, (s1, k1, s2, k2) in zip(ks, _split(ks)):
        assert (s1 * k1 + s2 * k2 * MU - k) % R == 0, hex(k)
        assert k1 < (1 << 127) and k2 < (1 << 127), hex(k)
        # what the body's comment proves: both halves are at most x^2 / 2
        assert 2 * k1 <= X2 and 2 * k2 <= X2, hex(k)
        largest = max(largest, k1, k2)
    assert largest.bit_length() == 127       # ~2^126.4: the 128-bit digit windows have their spare top bit


def _ints(sc):
    return [int.from_bytes(bytes(row), "little") for row in sc]


def _points(pts):
    return [CURVE.aff_from_bytes(bytes(row)) for row in pts]


def _expect(sc, pts):
    return CURVE.msm_pippenger(_ints(sc), _points(pts))


def _emu(monkeypatch, sc, pts, **kw):
    out, plan = glv_msm(sc, pts, 1, **kw)
    assert plan[5] == 1 or len(sc) == 0, "the split did not run"
    return CURVE.aff_from_bytes(bytes(out)), plan


def _inputs(n, seed):
    """n pairs with what the split has to get right, as far as n has room for it: scalars on both sides of r / 2 (a 255-bit
    seeded value is above it more often than not), a neutral point, a pair P / -P under one scalar, the same point twice under
    different scalars, a zero scalar and scalars whose k2 half is zero (k < x^2 / 2)"""
    pts = emu.gen_points(NAME, seed, n)
    ks = [po.synth_scalar(seed + 1, i, 255) for i in range(n)]
    if n >= 2:
        ks[1] = (R - 1) // 2 + (seed & 1)
    if n >= 3:
        ks[2] = po.synth_scalar(seed + 2, 2, 120)            # k2 = 0
    if n >= 64:
        pts[5] = 0                                           # the neutral (0, 0)
        pts[7] = CURVE.points_to_array([CURVE.neg(CURVE.aff_from_bytes(bytes(pts[6])))])[0]
        ks[7] = ks[6]
        pts[9] = pts[8]
        ks[10] = 0
        ks[11] = R                                           # == 0 mod r
        ks[12] = (1 << 255) - 1
    return CURVE.scalars_to_array(ks), pts


@pytest.fixture(scope="module")
def cases():
    out = {}
    for n in (1, 2, 3, 64, 65, 257):
        sc, pts = _inputs(n, 700 + n)
        out[n] = (sc, pts, _expect(sc, pts))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_emulated_pipeline_with_split_vs_oracle(n, cases, monkeypatch):
    sc, pts, expect = cases[n]
    # the default plan, and small windows / few entries per lane: more than one lane per bucket set, runs that straddle lanes
    for kw in (dict(), dict(c=5, K=4), dict(c=7, K=8, S=1)):
        got, plan = _emu(monkeypatch, sc, pts, **kw)
        assert got == expect, (n, kw, list(plan))
    # the same call with the split off is the path of every other curve: same element
    out, plan = glv_msm(sc, pts, 2)
    assert plan[5] == 0 and CURVE.aff_from_bytes(bytes(out)) == expect
    # and the emulator of the other tests, whose backend has no front stage, takes the plain path whatever the size
    out, _ = emu.msm(NAME, sc, pts)
    assert CURVE.aff_from_bytes(bytes(out)) == expect


def test_plan_of_the_split(cases, monkeypatch):
    """2n entries of 127 bits: windows over 128 bits, half as many bucket sets as the 256-bit plan at the same width"""
    sc, pts, expect = cases[257]
    got, plan = _emu(monkeypatch, sc, pts, c=16, K=8)
    assert got == expect
    assert (plan[0], plan[1], plan[6]) == (16, 8, 8), list(plan)      # c, bucket sets, digit windows of a half
    _, plan = glv_msm(sc, pts, 2, c=16, K=8)
    assert (plan[0], plan[1], plan[5]) == (16, 16, 0), list(plan)


def test_small_specials(monkeypatch):
    G = CURVE.gen
    # P and -P under one scalar cancel, in both halves
    k = po.synth_scalar(5, 0, 255)
    pts = CURVE.points_to_array([G, CURVE.neg(G)])
    got, _ = _emu(monkeypatch, CURVE.scalars_to_array([k, k]), pts)
    assert got is None
    # neutral points only; zero scalars only
    got, _ = _emu(monkeypatch, CURVE.scalars_to_array([k, 3]), CURVE.points_to_array([None, None]))
    assert got is None
    got, _ = _emu(monkeypatch, CURVE.scalars_to_array([0, R]), CURVE.points_to_array([G, G]))
    assert got is None
    # the same point twice under different scalars
    k2 = po.synth_scalar(5, 1, 255)
    got, _ = _emu(monkeypatch, CURVE.scalars_to_array([k, k2]), CURVE.points_to_array([G, G]), c=4, K=4)
    assert got == CURVE.scalar_mul((k + k2) % R, G)
    # every edge scalar on its own point
    pts = emu.gen_points(NAME, 88, len(EDGE))
    sc = CURVE.scalars_to_array(EDGE)
    got, _ = _emu(monkeypatch, sc, pts, c=6, K=4)
    assert got == _expect(sc, pts)


def test_all_equal_scalars_long_chains(monkeypatch):
    """every entry of a window in one bucket -- now 2n entries in two buckets per window (one per half): head chains over all lanes,
    through the tree and through the queue form of the merge"""
    n = 257
    pts = emu.gen_points(NAME, 41, n)
    k = po.synth_scalar(42, 0, 255)
    sc = CURVE.scalars_to_array([k] * n)
    total = None
    for P in _points(pts):
        total = CURVE.add(total, P)
    expect = CURVE.scalar_mul(k % R, total)
    for kw in (dict(c=6, K=4), dict(c=6, K=28), dict()):
        got, plan = _emu(monkeypatch, sc, pts, **kw)
        assert got == expect, (kw, list(plan))
    monkeypatch.setenv("EMU_MERGE_CHAIN", "1")
    got, plan = _emu(monkeypatch, sc, pts, c=6, K=4)
    assert got == expect


def test_fr_montgomery_coefficients(monkeypatch):
    n = 65
    pts = emu.gen_points(NAME, 61, n)
    ks = [po.synth_scalar(62, i, 256) % R for i in range(n)]
    expect = CURVE.msm_pippenger(ks, _points(pts))
    got, _ = _emu(monkeypatch, CURVE.fr_scalars_to_array(ks), pts, coef_is_fr=True, c=5, K=4)
    assert got == expect


def test_three_in_flight_over_two_input_sets(cases):
    """submit A, B, A before any finish: the slots share the record array, the half scalars and the canonical scalars"""
    sa, pa, ea = cases[257]
    sb, pb, eb = cases[65]
    out = np.zeros((3, emu.AFF_BYTES[NAME]), dtype=np.uint8)
    assert glv_lib().emu_glv_msm_slots(emu._p(out), emu._p(sa), emu._p(pa), 257, emu._p(sb), emu._p(pb), 65, 0) == 0
    assert [CURVE.aff_from_bytes(bytes(o)) for o in out] == [ea, eb, ea]
