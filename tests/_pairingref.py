"""The BLS12-381 optimal ate pairing in plain Python integers (test infrastructure; the reference the host pairing of
constantine_amd/csrc/pairing_host.h is compared with).  Nothing is shared with that header: Fp12 here is Fp[w]/(w^12 - 2 w^6 + 2), one
list of 12 integers (w^6 = 1 + i, so i = w^6 - 1), the final exponentiation is ONE pow by (p^12 - 1)/r, and the square root of the G2
decompression is the complex method.

The twist is of M type: E'(Fp2): y^2 = x^3 + 4 (1 + i), and (x', y') -> (x'/w^2, y'/w^3) lands on E(Fp12): y^2 = x^3 + 4.  The line through
T with slope s (both on the twist), at P = (xP, yP) of G1 and scaled by w^3 -- an element of Fp4, which the final exponentiation sends
to 1 -- is  (s x_T - y_T) - s xP w^2 + yP w^3.
"""
from oracle import pyoracle as po

P = po.BLS12_381_G1.F.p
R = po.BLS12_381_G1.order
X_ABS = 0xd201000000010000          # |x|; x is negative: the Miller loop's value is conjugated
G1 = po.BLS12_381_G1
G2 = po.BLS12_381_G2
F2 = G2.F
FINAL_EXPONENT = (P ** 12 - 1) // R
ONE = [1] + [0] * 11


def f12_mul(a, b):
    c = [0] * 23
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                c[i + j] += ai * bj
    for k in range(22, 11, -1):         # w^12 = 2 w^6 - 2
        c[k - 6] += 2 * c[k]
        c[k - 12] -= 2 * c[k]
    return [v % P for v in c[:12]]


def f12_pow(a, e):
    r = ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_conj(a):
    """a^(p^6): w -> -w"""
    return [v if k % 2 == 0 else (-v) % P for k, v in enumerate(a)]


def f12_from_fp2_at(a, k):
    """(a0 + a1 i) w^k as a polynomial in w, k < 6"""
    out = [0] * 12
    out[k] = (a[0] - a[1]) % P
    out[k + 6] = a[1] % P
    return out


def f12_from_tower(coeffs):
    """six Fp2 coefficients of w^0 .. w^5 (an element of Fp2[w]/(w^6 - (1 + i))) -> the polynomial form"""
    out = [0] * 12
    for k, a in enumerate(coeffs):
        out[k] = (out[k] + a[0] - a[1]) % P
        out[k + 6] = (out[k + 6] + a[1]) % P
    return out


def _line(s, T, Pt):
    xP, yP = Pt
    l = f12_from_fp2_at(F2.sub(F2.mul(s, T[0]), T[1]), 0)
    m = f12_from_fp2_at(F2.neg(F2.mul(s, (xP, 0))), 2)
    out = [(x + y) % P for x, y in zip(l, m)]
    out[3] = (out[3] + yP) % P
    return out


def miller_loop(Pt, Q):
    """f_{|x|,Q}(P), conjugated; P in G1 (affine or None), Q in G2 on the twist (affine over Fp2 or None).  A neutral argument gives 1."""
    if Pt is None or Q is None:
        return ONE
    f, T = ONE, Q
    for bit in bin(X_ABS)[3:]:
        s = F2.mul(F2.mul((3, 0), F2.sqr(T[0])), F2.inv(F2.add(T[1], T[1])))
        f = f12_mul(f12_mul(f, f), _line(s, T, Pt))
        T = G2.double(T)
        if bit == "1":
            s = F2.mul(F2.sub(Q[1], T[1]), F2.inv(F2.sub(Q[0], T[0])))
            f = f12_mul(f, _line(s, T, Pt))
            T = G2.add(T, Q)
    return f12_conj(f)


def final_exponentiation(f):
    return f12_pow(f, FINAL_EXPONENT)


def pairing(Pt, Q):
    return final_exponentiation(miller_loop(Pt, Q))


def pairing_check(pairs):
    """prod e(P_i, Q_i) == 1: one accumulator, one final exponentiation"""
    f = ONE
    for Pt, Q in pairs:
        f = f12_mul(f, miller_loop(Pt, Q))
    return final_exponentiation(f) == ONE


# ---- G2, the ZCash encoding: 96 bytes, x.c1 then x.c0; flags as for G1; the sign flag says that y is the "larger" root, compared on
# y.c1 unless it is zero, then on y.c0 (serialization/codecs_bls12_381.nim)
def fp_sqrt(a):
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def fp2_sqrt(a):
    """the complex method: for a = a0 + a1 i, with n = sqrt(a0^2 + a1^2): x0^2 = (a0 +- n)/2, x1 = a1 / (2 x0)"""
    a0, a1 = a
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a0 % P)
        return None if s is None else (0, s)
    n = fp_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    half = pow(2, -1, P)
    for cand in ((a0 + n) * half % P, (a0 - n) * half % P):
        x0 = fp_sqrt(cand)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, P) % P)
            if F2.sqr(x) == (a0 % P, a1 % P):
                return x
    return None


def g2_is_larger(y):
    return y[1] > (P - 1) // 2 if y[1] else y[0] > (P - 1) // 2


def g2_decompress(b96):
    assert len(b96) == 96 and b96[0] & 0x80
    if b96[0] & 0x40:
        return None
    x1 = int.from_bytes(b96[:48], "big") & ((1 << 381) - 1)
    x0 = int.from_bytes(b96[48:], "big")
    assert x0 < P and x1 < P
    x = (x0, x1)
    y = fp2_sqrt(F2.add(F2.mul(F2.sqr(x), x), G2.b))
    assert y is not None, "not on the curve"
    if bool(b96[0] & 0x20) != g2_is_larger(y):
        y = F2.neg(y)
    return (x, y)


def g2_compress(Q):
    if Q is None:
        return bytes([0xC0]) + bytes(95)
    (x0, x1), y = Q
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if g2_is_larger(y) else 0)
    return bytes(b)
