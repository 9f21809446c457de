"""Expected values of the batched Verkle commitment tests in Python integers (test infrastructure, over tests/_banderwagon.py): the
window layout of the table, its records, the crafted inputs of the finish kernel and what it must make of them."""
import random

from tests import _banderwagon as bw

HALF = (bw.P - 1) // 2


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
