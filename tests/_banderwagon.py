"""
Banderwagon oracle in Python integers (test infrastructure): the twisted Edwards curve -5x^2 + y^2 = 1 + d x^2 y^2 over the
BLS12-381 scalar field (constantine/named/config_fields_and_curves.nim:179-195), its affine unified law, scalar multiplication,
the 32-byte serialisation (constantine/serialization/codecs_banderwagon.nim:97-197), the subgroup test
(named/constants/banderwagon_subgroups.nim) and the Verkle CRS (constantine/ethereum_verkle_ipa.nim:23-64), plus the C-API byte
layout of libctt_msm_hip (Montgomery form, R = 2^256, little-endian 64-bit limbs).
"""
import hashlib

P = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R = 0x1cfb69d4ca675f520cce760202687600ff8f87007419047174fd06b52876e7e1   # order of the prime subgroup
A = P - 5
D = 0x6389c12633c267cbc66e3bf86be3b6d8cb66677177e54f92b369f2f5188d58e7
G = (0x29c132cc2c0b34c5743711777bbe42f32b79c022ad998465e1e71866a252ae18,
     0x2a6c669eda123e0f157d8b50badcd586358cad81eee464605e3167b6cc974166)
O = (0, 1)              # neutral
T2 = (0, P - 1)         # the point of order two that Banderwagon identifies with O
MONT = 1 << 256
SEED = b"eth_verkle_oct_2021"


def inv(v):
    return pow(v, P - 2, P)


def on_curve(pt):
    x, y = pt
    return (A * x * x + y * y - 1 - D * x * x * y * y) % P == 0


def add(p1, p2):
    x1, y1 = p1
    x2, y2 = p2
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % P, (y1 * y2 - A * x1 * x2) * inv(1 - t) % P)


def neg(pt):
    return ((-pt[0]) % P, pt[1])


def mul(k, pt):
    r = O
    for bit in bin(k)[2:] if k > 0 else "":
        r = add(r, r)
        if bit == "1":
            r = add(r, pt)
    return r


def msm(scalars, points):
    r = O
    for k, pt in zip(scalars, points):
        r = add(r, mul(k, pt))
    return r


def sqrt(v):
    """Tonelli-Shanks; None when v is not a square"""
    v %= P
    if v == 0:
        return 0
    if pow(v, (P - 1) // 2, P) != 1:
        return None
    q, s = P - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (P - 1) // 2, P) != P - 1:
        z += 1
    m, c, t, r = s, pow(z, q, P), pow(v, q, P), pow(v, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % P, i + 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


def in_subgroup(pt):
    return pow((1 - A * pt[0] * pt[0]) % P, (P - 1) // 2, P) == 1


def serialize(pt):
    if pt == O:
        return bytes(32)
    largest = pt[1] >= (P - 1) // 2
    x = pt[0] if largest else (-pt[0]) % P
    return x.to_bytes(32, "big")


def deserialize(b, check_subgroup=True):
    """the affine point with the lexicographically largest y, or None (codecs_banderwagon.nim deserialize_vartime)"""
    if b == bytes(32):
        return O
    x = int.from_bytes(b, "big")
    if x >= P:
        return None
    y = sqrt((1 - A * x * x) * inv((1 - D * x * x) % P))
    if y is None:
        return None
    if y < (P - 1) // 2:
        y = P - y
    pt = (x, y)
    if check_subgroup and not in_subgroup(pt):
        return None
    return pt


def crs(n, skip=0):
    """the first n points of the Verkle CRS generator (after `skip` of them): hash-to-x from SHA-256(seed || BE u64 counter)"""
    out, i = [], 0
    while len(out) < n + skip:
        h = int.from_bytes(hashlib.sha256(SEED + i.to_bytes(8, "big")).digest(), "big") % P
        i += 1
        pt = deserialize(h.to_bytes(32, "big"))
        if pt is not None:
            out.append(pt)
    return out[skip:]


# --- C-API bytes -------------------------------------------------------------------------------------------------------------
def fp_bytes(v):
    return (v * MONT % P).to_bytes(32, "little")


def fp_from(b):
    return int.from_bytes(b, "little") * pow(MONT, -1, P) % P


def aff_bytes(pt):
    return fp_bytes(pt[0]) + fp_bytes(pt[1])


def aff_from(b):
    return (fp_from(b[:32]), fp_from(b[32:64]))


def prj_from(b):
    x, y, z = fp_from(b[:32]), fp_from(b[32:64]), fp_from(b[64:96])
    iz = inv(z)
    return (x * iz % P, y * iz % P)


def big_bytes(k):
    return k.to_bytes(32, "little")


def fr_bytes(k):
    return (k * MONT % R).to_bytes(32, "little")


# --- the synthetic points of ctt_hip_gen_points (msm_bodies.h gen_point_body) ------------------------------------------------
def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def synth_log(seed, j, first=0):
    """discrete log of point j of ctt_hip_gen_points(seed, first) to the base G"""
    m = (1 << 64) - 1
    sd = (seed ^ 0xA5A5A5A5A5A5A5A5) & m
    j += first
    return (_splitmix64((sd + 4 * j) & m) | 1) | (_splitmix64((sd + 4 * j + 1) & m) << 64)


def _xadd(p, q):   # extended coordinates (X, Y, Z, T), unified law (add-2008-hwcd); no inversions
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b, c, d = x1 * x2 % P, y1 * y2 % P, D * t1 * t2 % P, z1 * z2 % P
    e, f, g, h = ((x1 + y1) * (x2 + y2) - a - b) % P, (d - c) % P, (d + c) % P, (b - A * a) % P
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def msm_fast(scalars, points):
    """sum k_i P_i in extended coordinates (for a few thousand points: one inversion at the end)"""
    r = (0, 1, 1, 0)
    for k, (x, y) in zip(scalars, points):
        q, acc = (x, y, 1, x * y % P), (0, 1, 1, 0)
        while k:
            if k & 1:
                acc = _xadd(acc, q)
            q, k = _xadd(q, q), k >> 1
        r = _xadd(r, acc)
    iz = inv(r[2])
    return (r[0] * iz % P, r[1] * iz % P)
