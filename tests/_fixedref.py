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
    raise KeyError(tag)


MSM_CASES = ("T2", "T3", "T4", "T5", "T7")
