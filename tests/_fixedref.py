"""Inputs and expected values of the batched fixed-base MSM tests (test infrastructure): the window layout and the records of the
table in Python integers, the cases the CPU harness (tests/fixed_harness.cpp) and the GPU path share, each with its expected affine
Montgomery bytes from an independent CPU result -- oracle.pyoracle integers for small counts, oracle.cref.msm per row otherwise --
computed once per process, and the build of the harness."""
import functools
import os
import random
import shutil
import struct
import subprocess

import numpy as np

from oracle import cref
from oracle import pyoracle as po

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")
CURVE_ID = {"bls12_381_g1": 0, "bn254_snarks_g1": 2}
BITS = {"bls12_381_g1": 255, "bn254_snarks_g1": 254}


def build_harness(tmp_dir):
    """compile tests/fixed_harness.cpp into tmp_dir -> run(mode, stdin bytes) -> stdout bytes"""
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_dir), "fixed_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "fixed_harness.cpp"), "-o", exe], check=True)

    def run(mode, data):
        return subprocess.run([exe, mode], input=data, check=True, capture_output=True).stdout
    return run


def layout(bits, c):
    """msm_bodies.h window_layout(bits, c): [(offset, width)] of every window"""
    t = bits + 1
    nw = (t + c - 1) // c
    cb = t // nw
    r = t - cb * nw
    out, off = [], 0
    for w in range(nw):
        width = cb + (1 if w < r else 0)
        out.append((off, width))
        off += width
    assert off == t
    return out


def table_bytes(name, points, c):
    """every record of the table of `points` (affine integer points, None the neutral) in table order, from Python integers"""
    curve = po.CURVES[name]
    out = []
    for P in points:
        for off, width in layout(BITS[name], c):
            Q = curve.scalar_mul(1 << off, P) if P is not None else None
            R = None
            for _ in range(1 << (width - 1)):
                R = curve.add(R, Q)
                out.append(curve.aff_to_bytes(R))
    return b"".join(out)


def harness_table_input(name, pts, c):
    return struct.pack("<3I", CURVE_ID[name], len(pts), c) + pts.tobytes()


def harness_msm_input(name, pts, coefs, c, fr=False):
    m, n = coefs.shape[:2]
    return struct.pack("<5I", CURVE_ID[name], n, c, 1 if fr else 0, m) + pts.tobytes() + coefs.tobytes()


def rows_per_base(bits, c):
    """records of one base: 2^(width - 1) per window"""
    return sum(1 << (width - 1) for _, width in layout(bits, c))


def booth_digits(k, lay):
    """the signed digit of every window of `lay` for the scalar k (bigints.nim signedWindowEncoding over windows of their own width)"""
    out = []
    for off, width in lay:
        d = ((k << 1) >> off) & ((1 << (width + 1)) - 1)
        e = (d + 1) >> 1
        out.append(e - (1 << width) if d >> width else e)
    assert sum(dg << off for dg, (off, _) in zip(out, lay)) == k
    return out


def largest_digit_scalars(bits, c):
    """three scalars below 2^bits with a digit of the largest magnitude 2^(width - 1) in the lowest window, in a middle window and in
    the top window: -2^(width - 1), the top bit of the window alone (the window above takes the carry, +1), in the lowest and the
    middle window; the top window has bit `bits` as its top bit, which no scalar sets, so its largest digit is +2^(width - 1): all its
    other bits and the bit below it (the top bit of the window below, which so holds -2^(width - 1) too).  Each such digit reads the
    last record of its window."""
    lay = layout(bits, c)
    W = len(lay)
    out = []
    for w in (0, W // 2):
        off, width = lay[w]
        k = 1 << (off + width - 1)
        assert booth_digits(k, lay)[w] == -(1 << (width - 1))
        out.append(k)
    off, width = lay[W - 1]
    k = ((1 << (width - 1)) - 1) << off | 1 << (off - 1)
    assert k < 1 << bits and booth_digits(k, lay)[W - 1] == 1 << (width - 1)
    out.append(k)
    return out


def harness_finish_input(name, part):
    m, chunks = part.shape[:2]
    return struct.pack("<3I", CURVE_ID[name], m, chunks) + part.tobytes()


FINISH_CHUNKS = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
FINISH_ROWS = ("dense", "last only", "from 64 on", "all zero", "equal at s and s + 64", "opposite at s and s + 64")


@functools.lru_cache(maxsize=None)
def _finish_pool(name):
    """(k_j, k_j * G) for 320 known k_j = k_0 + j * d, by running additions: two scalar multiplications in all"""
    curve = po.CURVES[name]
    rng = random.Random("finish pool " + name)
    k0, d = rng.randrange(1, curve.order), rng.randrange(1, curve.order)
    P, D = curve.scalar_mul(k0, curve.gen), curve.scalar_mul(d, curve.gen)
    pool = []
    for j in range(320):
        pool.append(((k0 + j * d) % curve.order, P))
        P = curve.add(P, D)
    return pool


def _xyzz_bytes(curve, P, z):
    """(x z^2, y z^3, z^2, z^3) in Montgomery words; None: the in-memory neutral, all zero"""
    F = curve.F
    if P is None:
        return bytes(4 * F.nbytes)
    zz = F.sqr(z)
    zzz = F.mul(zz, z)
    return b"".join(F.to_mont_bytes(v) for v in (F.mul(P[0], zz), F.mul(P[1], zzz), zz, zzz))


@functools.lru_cache(maxsize=None)
def finish_case(name, chunks):
    """-> (part (6, chunks, 4 * coordinate bytes) uint8, expect (6, aff) uint8): the six rows of FINISH_ROWS as XYZZ partials k * G
    with known k, each with a random non-zero z of its own, and (sum of the row's k mod r) * G.  s, the lane of the last two rows, is
    chunks - 65 where the row has a partial s + 64 (so at 256 chunks the pair is the third and fourth stride of lane 63), and the
    pair is (0, chunks - 1) below 65 chunks."""
    curve = po.CURVES[name]
    pool = _finish_pool(name)
    rng = random.Random(f"finish {name} {chunks}")
    s0, s1 = (chunks - 65, chunks - 1) if chunks > 64 else (0, chunks - 1)
    rows = []
    for what in FINISH_ROWS:
        row = [None] * chunks                                   # (k, point) per partial
        if what == "dense":
            row = [pool[rng.randrange(320)] for _ in range(chunks)]
        elif what == "last only":
            row[chunks - 1] = pool[rng.randrange(320)]
        elif what == "from 64 on":
            row = [pool[rng.randrange(320)] if s >= 64 else None for s in range(chunks)]
        elif what == "equal at s and s + 64":                   # the rest of that lane's partials neutral: its sum so far is the point
            row = [pool[rng.randrange(320)] if s % 64 != s0 % 64 else None for s in range(chunks)]
            row[s0] = row[s1] = pool[rng.randrange(320)]
        elif what == "opposite at s and s + 64":
            k, P = pool[rng.randrange(320)]
            row[s0] = (k, P)
            if s1 != s0:
                row[s1] = (curve.order - k, curve.neg(P))
        rows.append(row)
    part = b"".join(_xyzz_bytes(curve, e[1] if e else None, rng.randrange(1, curve.F.p)) for row in rows for e in row)
    expect = [curve.scalar_mul(sum(e[0] for e in row if e) % curve.order, curve.gen) for row in rows]
    if chunks > 1:
        assert expect[3] is None and expect[5] is None
    return (np.frombuffer(part, dtype=np.uint8).reshape(6, chunks, 4 * curve.F.nbytes).copy(), curve.points_to_array(expect))


class Case:
    """name: the curve; pts (n, aff) uint8; coefs (m, n, 32) uint8 canonical; cs: the window sizes to run; expect (m, aff) uint8;
    coefs_fr: the same scalars mod r as Montgomery residues, where the case has that form"""

    def __init__(self, name, pts, coefs, cs, expect, coefs_fr=None):
        self.name, self.pts, self.coefs, self.cs, self.expect, self.coefs_fr = name, pts, coefs, cs, expect, coefs_fr


def _rows_by_cref(name, pts, coefs, keep=None):
    """cref.msm per row; keep: the indices of the bases handed to the oracle (the others are neutral)"""
    rows = []
    for k in range(coefs.shape[0]):
        sc, p = (coefs[k], pts) if keep is None else (coefs[k][keep], pts[keep])
        rows.append(cref.msm(name, np.ascontiguousarray(sc), np.ascontiguousarray(p), nthreads=4)[0])
    return np.stack(rows)


def _scalars(curve, rows):
    return np.stack([curve.scalars_to_array(r) for r in rows])


@functools.lru_cache(maxsize=None)
def case(tag):
    bls, bn = "bls12_381_g1", "bn254_snarks_g1"
    if tag == "T2":      # scalar edges, n = 1
        curve = po.CURVES[bls]
        r = curve.order
        pts = cref.gen_points(bls, 21, 1)
        P = curve.aff_from_bytes(bytes(pts[0]))
        ks = [0, 1, 2, r - 1, r, r + 1, 2**255 - 1]
        expect = curve.points_to_array([curve.scalar_mul(k, P) for k in ks])
        assert bytes(expect[0]) == bytes(96) and bytes(expect[4]) == bytes(96) and bytes(expect[1]) == bytes(pts[0])
        return Case(bls, pts, _scalars(curve, [[k] for k in ks]), (5, 6), expect)
    if tag == "T3":      # chunk edge: the second chunk holds one base; uniform unreduced 255-bit scalars
        curve = po.CURVES[bls]
        rng = random.Random(33)
        pts = cref.gen_points(bls, 22, 257)
        ks = [[rng.getrandbits(255) for _ in range(257)] for _ in range(3)]
        coefs = _scalars(curve, ks)
        fr = np.stack([curve.fr_scalars_to_array(row) for row in ks])
        return Case(bls, pts, coefs, (5,), _rows_by_cref(bls, pts, coefs), fr)
    if tag == "T4":      # collisions: every base is G
        curve = po.CURVES[bls]
        r = curve.order
        pts = curve.points_to_array([curve.gen] * 256)
        k = 0x1234567_89abcdef_0fedcba9_87654321_13579bdf_2468ace0_0badc0de_5ca1ab1e % r
        ks = [[k] * 256, [k if i % 2 == 0 else r - k for i in range(256)], [0] * 256]
        expect = curve.points_to_array([curve.scalar_mul(256 * k % r, curve.gen), None, None])
        return Case(bls, pts, _scalars(curve, ks), (6,), expect)
    if tag == "T5":      # neutral bases at both ends of the chunk, P and -P next to each other
        curve = po.CURVES[bls]
        rng = random.Random(55)
        pts = cref.gen_points(bls, 23, 256)
        P = curve.aff_from_bytes(bytes(pts[1]))
        pts[2] = np.frombuffer(curve.aff_to_bytes(curve.neg(P)), dtype=np.uint8)
        pts[0] = 0
        pts[255] = 0
        ks = [[rng.getrandbits(255) for _ in range(256)] for _ in range(2)]
        ks[1][2] = ks[1][1]                                  # the two cancel
        coefs = _scalars(curve, ks)
        return Case(bls, pts, coefs, (6,), _rows_by_cref(bls, pts, coefs, keep=np.arange(1, 255)))
    if tag == "T7":      # BN254 G1; 2 divides 254
        curve = po.CURVES[bn]
        rng = random.Random(77)
        pts = cref.gen_points(bn, 24, 70)
        coefs = _scalars(curve, [[rng.getrandbits(254) for _ in range(70)] for _ in range(2)])
        return Case(bn, pts, coefs, (2, 8), _rows_by_cref(bn, pts, coefs))
    if tag in ("T8", "T8bn"):   # the window sizes 7 and 9 .. 12 (and 2 on 255 bits): n = 5, six rows that hold every scalar edge once
        name = bls if tag == "T8" else bn
        curve = po.CURVES[name]
        r, bits = curve.order, BITS[name]
        cs = (2, 7, 9, 10, 11, 12) if tag == "T8" else (7, 9, 10, 11, 12)
        rng = random.Random(tag)
        pts = cref.gen_points(name, 25, 5)
        edges = [0, 1, 2, r - 1, r, r + 1, 2**bits - 1] + [k for c in cs for k in largest_digit_scalars(bits, c)]
        ks = edges + [rng.getrandbits(bits) for _ in range(-len(edges) % 5 + 5)]
        rows = [ks[j:j + 5] for j in range(0, len(ks), 5)]
        P = [curve.aff_from_bytes(bytes(p)) for p in pts]
        expect = curve.points_to_array([curve.msm_naive(row, P) for row in rows])
        fr = np.stack([curve.fr_scalars_to_array(row) for row in rows])
        return Case(name, pts, _scalars(curve, rows), cs, expect, fr)
    raise KeyError(tag)


MSM_CASES = ("T2", "T3", "T4", "T5", "T7", "T8", "T8bn")
