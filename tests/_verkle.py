"""Expected values of the batched Verkle commitment and update tests in Python integers (test infrastructure, over
tests/_banderwagon.py): the window layout of the table, its records, the crafted inputs of the finish kernel and what it must make of
them, the encodings and the three-output check the GPU test files share, and the build of the CPU harness (tests/verkle_harness.cpp)."""
import os
import random
import shutil
import subprocess

import numpy as np

from tests import _banderwagon as bw

HALF = (bw.P - 1) // 2
TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")


def build_harness(tmp_dir):
    """compile tests/verkle_harness.cpp into tmp_dir -> run(mode, stdin bytes) -> stdout bytes"""
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_dir), "verkle_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "verkle_harness.cpp"), "-o", exe], check=True)

    def run(mode, data):
        return subprocess.run([exe, mode], input=data, check=True, capture_output=True).stdout
    return run


def torch_with_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def device_msm():
    """(generator, for a fixture) one DeviceMsm on device 0, closed afterwards"""
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


def synth_crs(dev, torch, seed):
    """(generator, for a fixture) 256 synthetic points [s_j]G of known s_j, the table made from the device tensor"""
    from constantine_amd import VerkleCrs
    d = torch.empty((256, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", seed, 256, d)
    dev.sync()
    logs = [bw.synth_log(seed, j) for j in range(256)]
    crs = VerkleCrs(d, ctx=dev.ctx, on_device=True)
    yield d, logs, crs
    crs.close()


def pts_array(points):
    """affine points -> (n, 64) uint8, C-API layout"""
    return np.frombuffer(b"".join(bw.aff_bytes(p) for p in points), dtype=np.uint8).reshape(-1, 64).copy()


def prj_bytes(pt, z=1):
    """(X, Y, Z) bytes of the affine point scaled by z"""
    return bw.fp_bytes(pt[0] * z % bw.P) + bw.fp_bytes(pt[1] * z % bw.P) + bw.fp_bytes(z % bw.P)


def ser_bytes(pt):
    x = pt[0] if pt[1] >= HALF else (-pt[0]) % bw.P
    return x.to_bytes(32, "big")


def log_point(t):
    return bw.msm_fast([t % bw.R], [bw.G])


def check_outputs(out, i, pt):
    """row i of the outputs prj, ser, fr of a commit or update call is the point pt"""
    assert bytes(out["prj"][i]) == prj_bytes(pt), i
    assert bytes(out["ser"][i]) == ser_bytes(pt), i
    assert fr_from(bytes(out["fr"][i])) == map_fr(pt), i


def layout(c):
    """msm_bodies.h window_layout(253, c): [(offset, width)] of every window"""
    t = 254
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


def rec_bytes(pt):
    return bw.fp_bytes(pt[0]) + bw.fp_bytes(pt[1]) + bw.fp_bytes(bw.D * pt[0] * pt[1] % bw.P)


def map_fr(pt):
    return pt[0] * bw.inv(pt[1]) % bw.P % bw.R


def fr_from(b):
    return int.from_bytes(b, "little") * pow(bw.MONT, -1, bw.R) % bw.R


def crafted_triples():
    """(X, Y, Z) with X = t*Y*lambda, Y = y*lambda, Z = lambda: the map gives t mod r, the affine point is (t*y*lambda, y)"""
    rng = random.Random(5)
    r, p = bw.R, bw.P
    ts = [0, 1, r - 1, r, r + 1, 2 * r, 3 * r, 4 * r - 1, 4 * r, 4 * r + 1, p - 1]
    ys = [1, HALF - 1, HALF, HALF + 1, p - 1]
    out = []
    for t in ts:
        for y in ys:
            lam = rng.randrange(1, p)
            out.append((t * y * lam * lam % p, y * lam % p, lam))
    return out


def expected_finish(tr):
    X, Y, Z = tr
    p = bw.P
    iz = bw.inv(Z) if Z else 0
    iy = bw.inv(Y) if Y else 0
    x, y = X * iz % p, Y * iz % p
    sx = x if y >= HALF else (-x) % p
    return bw.fp_bytes(x) + bw.fp_bytes(y) + bw.fp_bytes(1), sx.to_bytes(32, "big"), X * iy % p % bw.R
