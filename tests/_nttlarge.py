"""References for transforms too large for the recursive transform of tests/_nttref.py (test infrastructure, Python integers and
numpy, never the code under test).  Write w for the plan's root, n = 2^L, m = 2^12, s = n / m, g for the coset shift; forward
X_k = sum_i g^i x_i w^(ik), inverse x_i = g^-i / n * sum_k X_k w^(-ik), a bit-reversed side holds natural element i at position brp(i).

  sparse    x is zero but for a few c_j at natural indices i_j: X_k = sum_j c_j g^(i_j) w^(i_j k mod n), and the inverse likewise with
            w^-1 and the factor g^-k / n -- a few products per output, so outputs are sampled
  strided   x_(q s) = y_q, zero elsewhere: X_k = Y_(k mod m), Y the transform of y with root w^s and shift g^s; the inverse (no shift)
            is the inverse transform of y over s -- every output is known
  dense     x dense, f_r = sum_q x_(r + q m): X_(j s) = F_j, F the transform of f with root w^s; the inverse is the inverse transform
            of f over s -- every input counts, m outputs are known

Each of the three is compared with the full transform at 2^13 in tests/test_ntt_cpu.py before anything relies on it."""
import random

import numpy as np

from tests import _nttref as ref

M_LOG2 = 12
M = 1 << M_LOG2


class _Powers:
    """base^e mod p for e < 2^bits as one product of two table entries"""

    def __init__(self, base, p, bits):
        self.p, self.h = p, (bits + 1) // 2
        self.lo = self._run(base, 1 << self.h)
        self.hi = self._run(pow(base, 1 << self.h, p), 1 << (bits - self.h))

    def _run(self, b, count):
        out, v = [], 1
        for _ in range(count):
            out.append(v)
            v = v * b % self.p
        return out

    def __call__(self, e):
        return self.lo[e & ((1 << self.h) - 1)] * self.hi[e >> self.h] % self.p


def sparse(p, omega, lg, flags, shift, seed, terms=24, samples=2000):
    """-> (input positions, their canonical values, output positions, the canonical values expected there).  The indices hold 0, 1,
    n - 1, n / 2 and n / 2 + 1, so every index bit is set in one and clear in another; the outputs are 0, 1, n - 1, 2^b and 2^b - 1
    for every b < L and `samples` seeded ones.  flags: INVERSE, IN_BRP, OUT_BRP."""
    assert not flags & ~(ref.INVERSE | ref.IN_BRP | ref.OUT_BRP)
    n = 1 << lg
    rng = random.Random("sparse%s" % (seed,))
    idx = [0, 1, n - 1, n // 2, n // 2 + 1]
    while len(idx) < terms:
        i = rng.randrange(n)
        if i not in idx:
            idx.append(i)
    for b in range(lg):
        assert any(i >> b & 1 for i in idx) and not all(i >> b & 1 for i in idx)
    val = [rng.randrange(1, p) for _ in idx]
    ks = {0, 1, n - 1} | {1 << b for b in range(lg)} | {(1 << b) - 1 for b in range(lg)} | {rng.randrange(n) for _ in range(samples)}
    ks = sorted(ks)
    g = 1 if shift is None else shift
    if flags & ref.INVERSE:
        w, ginv, ninv = _Powers(pow(omega, -1, p), p, lg), pow(g, -1, p), pow(n, -1, p)
        want = [ninv * pow(ginv, k, p) * sum(c * w(i * k % n) for i, c in zip(idx, val)) % p for k in ks]
    else:
        w = _Powers(omega, p, lg)
        cg = [c * pow(g, i, p) % p for i, c in zip(idx, val)]
        want = [sum(c * w(i * k % n) for i, c in zip(idx, cg)) % p for k in ks]
    pos_in = [ref.brp(i, lg) if flags & ref.IN_BRP else i for i in idx]
    pos_out = [ref.brp(k, lg) if flags & ref.OUT_BRP else k for k in ks]
    return pos_in, val, pos_out, want


def strided(p, omega, lg, flags, shift, seed):
    """-> (input positions of y_0 .. y_(m-1), y, the m values `tile` the output repeats, (shape of the output, shape of the tile)):
    the output bytes viewed in the first shape equal the tile's bytes viewed in the second, broadcast.  Natural order out: s copies
    of Y one after the other; bit-reversed out: position a s + b holds Y_(brp12(a)) for every b < s.  An inverse takes no shift."""
    assert not flags & ~(ref.INVERSE | ref.IN_BRP | ref.OUT_BRP) and lg >= M_LOG2
    s = 1 << (lg - M_LOG2)
    y = ref.stored_inputs(p, M, "strided%s" % (seed,))
    ws = pow(omega, s, p)
    if flags & ref.INVERSE:
        assert shift is None
        sinv = pow(s, -1, p)
        Y = [v * sinv % p for v in ref.ntt(y, p, ws, inverse=True)]
    else:
        Y = ref.ntt(y, p, ws, shift=None if shift is None else pow(shift, s, p))
    pos_in = [ref.brp(q, M_LOG2) if flags & ref.IN_BRP else q * s for q in range(M)]    # brp_L(q s) = brp_12(q)
    if flags & ref.OUT_BRP:
        return pos_in, y, [Y[ref.brp(a, M_LOG2)] for a in range(M)], ((M, s, 32), (M, 1, 32))
    return pos_in, y, Y, ((s, M, 32), (1, M, 32))


def dense_bytes(lg, seed):
    """n * 32 seeded bytes, the top byte of every word below 0x20: words below 2^253, which is below the four 2-adic moduli"""
    x = np.random.default_rng(seed).integers(0, 256, size=(1 << lg, 32), dtype=np.uint8)
    x[:, 31] &= 0x1f
    return x.reshape(-1)


def fold(x, p, lg, in_brp):
    """x: n * 32 bytes (numpy uint8) of words below 2^256 -> f_r = sum_q x_(r + q m) mod p, r < m, by natural index"""
    s = 1 << (lg - M_LOG2)
    w = np.ascontiguousarray(x).view("<u4")
    if in_brp:     # natural index r + q m sits at position brp_12(r) s + brp(q)
        a = w.reshape(M, s, 8).sum(axis=1, dtype=np.uint64)
        a = a[[ref.brp(r, M_LOG2) for r in range(M)]]
    else:
        a = w.reshape(s, M, 8).sum(axis=0, dtype=np.uint64)
    return [sum(int(v) << (32 * j) for j, v in enumerate(row)) % p for row in a]


def dense(f, p, omega, lg, flags):
    """f = fold(x) -> (output positions, the m canonical values expected there): the outputs of natural index j s, j < m"""
    assert not flags & ~(ref.INVERSE | ref.IN_BRP | ref.OUT_BRP)
    s = 1 << (lg - M_LOG2)
    ws = pow(omega, s, p)
    if flags & ref.INVERSE:
        sinv = pow(s, -1, p)
        F = [v * sinv % p for v in ref.ntt(f, p, ws, inverse=True)]
    else:
        F = ref.ntt(f, p, ws)
    return [ref.brp(j, M_LOG2) if flags & ref.OUT_BRP else j * s for j in range(M)], F     # brp_L(j s) = brp_12(j)
