"""A plain restatement of the endomorphism split of BLS12-381 G1 (steps 1 to 4 of the comment above Bls12381Glv in csrc/msm_bodies.h), for
tests/test_glv_front_probe.py and tests/test_sort_probe.py.  Python integers only; nothing of constantine_amd is imported and no code is
shared with what is tested.

k == s1 k1 + s2 k2 mu (mod r) with mu = -x^2 mod r, k1 = |k' - q x^2|, k2 = q = round(k' / x^2) for k' = k mod r folded to at most
(r - 1) / 2; a remainder of exactly x^2 / 2 is NOT rounded up.  Beside the halves and the signs, split() reports the way the body takes
through its branches: whether it folds, how many correction steps its estimate of the quotient needs, whether it rounds up."""
from collections import namedtuple

X = 0xd201000000010000                 # |x| of BLS12-381
X2 = X * X
R = X2 * X2 - X2 + 1                   # the order of G1
MU = (-X2) % R                         # phi(P) = [MU]P
M = (1 << 254) // X2                   # the body's reciprocal: floor(2^254 / x^2)

Split = namedtuple("Split", "k1 k2 s1 s2 fold steps up")


def split(k):
    """the split of any k < 2^255"""
    assert 0 <= k < (1 << 255)
    if k >= R:                          # 2^255 < 2r: once
        k -= R
    fold = k > (R - 1) // 2
    if fold:
        k = R - k
    q = ((k >> 126) * M) >> 128         # an estimate of k / x^2 from below
    rem = k - q * X2
    steps = 0
    while rem >= X2:
        rem, q, steps = rem - X2, q + 1, steps + 1
    up = 2 * rem > X2                   # a tie stays below
    if up:
        rem, q = X2 - rem, q + 1
    return Split(rem, q, -1 if up != fold else 1, 1 if fold else -1, fold, steps, up)


def ties(qs):
    """q x^2 + x^2 / 2 (the remainder is exactly half: not rounded up) and its successor (rounded up), and the same two behind the fold"""
    out = []
    for q in qs:
        assert 0 <= q < X2 // 2 - 1
        t = q * X2 + X2 // 2
        out += [t, t + 1, R - t, R - t - 1]
    return out
