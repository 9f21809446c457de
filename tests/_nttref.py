"""The scalar-field NTT of ctt_hip_fr_ntt in Python integers (test infrastructure): a recursive transform, every flag, the
fields' moduli and roots of unity, and the case list the CPU harness test and the GPU test share."""
import functools
import random

R = 1 << 256   # the Montgomery radix of the 8-word fields

# name -> (harness field id, a curve id with this scalar field, modulus)
FIELDS = {
    "bls12_381_fr": (0, 0, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001),
    "bn254_snarks_fr": (1, 2, 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001),
    "pallas_fr": (2, 4, 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001),
    "vesta_fr": (3, 5, 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001),
    "banderwagon_fr": (4, 6, 0x1cfb69d4ca675f520cce760202687600ff8f87007419047174fd06b52876e7e1),
}
INVERSE, IN_BRP, OUT_BRP, IN_MONT, OUT_MONT = 1, 2, 4, 8, 16
DEFAULT_TILE_LOG2 = 8


def two_adicity(p):
    return ((p - 1) & -(p - 1)).bit_length() - 1


def root_of_unity(p, log2n):
    """an element of order exactly 2^log2n (BLS12-381: 7^((r-1)/n), the consensus spec's)"""
    for x in (7, 2, 3, 5, 11, 13, 17, 19):
        w = pow(x, (p - 1) >> log2n, p)
        if pow(w, 1 << (log2n - 1), p) == p - 1:
            return w
    raise AssertionError("no generator among the small primes")


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _dft(x, w, p):
    n = len(x)
    if n == 1:
        return list(x)
    ev, od = _dft(x[0::2], w * w % p, p), _dft(x[1::2], w * w % p, p)
    out, t = [0] * n, 1
    for k in range(n // 2):
        o = t * od[k] % p
        out[k], out[k + n // 2] = (ev[k] + o) % p, (ev[k] - o) % p
        t = t * w % p
    return out


def ntt(x, p, omega, inverse=False, in_brp=False, out_brp=False, shift=None):
    """one row of plain integers: forward out[k] = sum_i (g^i x[i]) w^(ik); inverse out[i] = g^-i / n * sum_k x[k] w^(-ik);
    a BRP side holds natural element i at position brp(i)"""
    n = len(x)
    bits = n.bit_length() - 1
    if in_brp:
        x = [x[brp(i, bits)] for i in range(n)]
    g = 1 if shift is None else shift
    if not inverse:
        out = _dft([v * pow(g, i, p) % p for i, v in enumerate(x)], omega, p)
    else:
        ninv, ginv = pow(n, -1, p), pow(g, -1, p)
        out = [v * ninv % p * pow(ginv, i, p) % p for i, v in enumerate(_dft(x, pow(omega, -1, p), p))]
    if out_brp:
        out = [out[brp(i, bits)] for i in range(n)]
    return out


def stored_inputs(p, count, seed):
    """`count` stored 256-bit words below p: seeded uniform values, and 0, 1, p - 1 and the residues of 1 and p - 1 in front"""
    rng = random.Random(seed)
    v = [rng.randrange(p) for _ in range(count)]
    for i, s in enumerate((0, 1, p - 1, R % p, (p - 1) * R % p)):
        if i < count - 1:
            v[i] = s
    return v


def decode(stored, p, mont):
    rinv = pow(R, -1, p)
    return [s * rinv % p for s in stored] if mont else list(stored)


def encode(values, p, mont):
    return [v * R % p for v in values] if mont else list(values)


def to_bytes(words):
    return b"".join(w.to_bytes(32, "little") for w in words)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def cases(field):
    """(id, log2n, tile_log2 (0 = default), batch, flags, shift kind (None | 'w2n' | 'rand'), in_place) for one field; sizes above
    the field's two-adicity are left out (Banderwagon: 5)"""
    p = FIELDS[field][2]
    T = DEFAULT_TILE_LOG2
    out = [
        ("n2", 1, 0, 1, 0, None, False), ("n4", 2, 0, 2, 0, None, False),
        ("t3_n8_one_pass", 3, 3, 1, 0, None, False), ("t3_n16_second_pass_of_one", 4, 3, 1, 0, None, False),
        ("t3_n32", 5, 3, 2, IN_BRP | OUT_MONT, None, False),
        ("t3_n128_three_passes", 7, 3, 1, 0, None, False), ("t3_n128_dit", 7, 3, 1, IN_BRP, None, False),
        ("t3_n128_batch3", 7, 3, 3, OUT_BRP, None, False), ("t3_n128_batch3_dit", 7, 3, 3, IN_BRP, None, False),
        ("default_n_T", T, 0, 1, OUT_BRP, None, False), ("default_n_T1", T + 1, 0, 1, OUT_BRP, None, False),
        ("default_n_T1_dit", T + 1, 0, 2, IN_BRP, None, False),
        ("default_n4096", 12, 0, 1, OUT_BRP, None, False), ("default_n4096_dit_inv", 12, 0, 1, INVERSE | IN_BRP, None, False),
        ("t2_n32_in_place", 5, 2, 2, 0, None, True),
        ("t9_n4096_largest_image", 12, 9, 1, IN_MONT, None, False), ("t9_n4096_dit", 12, 9, 1, IN_BRP | OUT_MONT, "rand", False),
        ("t1_n32_one_stage_per_pass", 5, 1, 1, 0, None, False),
    ]
    for fl in (0, IN_BRP, OUT_BRP, IN_BRP | OUT_BRP):
        for lg, t in ((7, 3), (5, 2)):
            out.append(("order%d_n%d" % (fl, 1 << lg), lg, t, 1, fl, None, False))
            out.append(("order%d_n%d_inverse" % (fl, 1 << lg), lg, t, 1, fl | INVERSE, None, False))
    for lg, t in ((7, 3), (5, 3)):
        for sk in ("w2n", "rand"):
            for fl in (OUT_BRP, INVERSE | IN_BRP, 0, INVERSE, IN_BRP | OUT_BRP, INVERSE | IN_BRP | OUT_BRP):
                out.append(("shift_%s_%d_n%d" % (sk, fl, 1 << lg), lg, t, 2, fl, sk, False))
        for fl in (IN_MONT, OUT_MONT, IN_MONT | OUT_MONT, INVERSE | IN_MONT, INVERSE | OUT_MONT, INVERSE | IN_MONT | OUT_MONT | IN_BRP):
            out.append(("mont%d_n%d" % (fl, 1 << lg), lg, t, 1, fl, None, False))
        out.append(("in_place_n%d" % (1 << lg), lg, t, 2, 0, None, True))
        out.append(("in_place_inv_shift_n%d" % (1 << lg), lg, t, 2, INVERSE | IN_BRP | OUT_BRP | IN_MONT, "rand", True))
    lim = two_adicity(p)
    return [c for c in out if c[1] <= lim and (c[5] != "w2n" or c[1] + 1 <= lim)]


def large_cases(field):
    """cases() continued above n = 4096, where the width of an index shows: twiddle exponents of 12 bits and more, power tables
    longer than 4096, more than a few tile bits on either side of a pass's rows.  2^13 and 2^14 at the default tile in every order,
    direction and with both shift tables, 2^14 at the largest image and in four passes, 2^16 (two full default passes) and 2^17
    (the smallest three-pass default plan) on one field each: the recursive reference costs a second per row there."""
    p = FIELDS[field][2]
    S = INVERSE | IN_BRP
    out = [
        ("n8192_dif", 13, 0, 1, OUT_BRP, None, False), ("n8192_dit", 13, 0, 1, IN_BRP, None, False),
        ("n8192_inverse", 13, 0, 1, INVERSE, None, False), ("n8192_shift", 13, 0, 1, 0, "rand", False),
        ("n8192_inverse_shift_in_place", 13, 0, 1, S, "rand", True), ("n8192_batch2", 13, 0, 2, IN_BRP | OUT_BRP, None, False),
        ("n16384_dif", 14, 0, 1, 0, None, False), ("n16384_dit_batch2", 14, 0, 2, IN_BRP, None, False),
        ("n16384_inverse", 14, 0, 1, S | OUT_BRP, None, False), ("n16384_shift", 14, 0, 1, OUT_BRP, "rand", False),
        ("n16384_inverse_shift", 14, 0, 1, INVERSE, "rand", False), ("n16384_in_place", 14, 0, 1, OUT_BRP, None, True),
        ("t9_n16384_largest_image", 14, 9, 1, OUT_BRP, None, False), ("t9_n16384_dit_inverse_shift", 14, 9, 1, S, "rand", False),
        ("t4_n16384_four_passes", 14, 4, 1, OUT_BRP, "rand", False), ("t4_n16384_dit", 14, 4, 1, IN_BRP, None, False),
    ]
    if field == "bls12_381_fr":
        out.append(("n65536_two_full_passes", 16, 0, 1, OUT_BRP, "rand", False))
    if field == "bn254_snarks_fr":
        out += [("n131072_three_passes", 17, 0, 1, OUT_BRP, None, False), ("n131072_three_passes_dit", 17, 0, 1, IN_BRP, None, False)]
    lim = two_adicity(p)
    return [c for c in out if c[1] <= lim]


@functools.lru_cache(maxsize=None)
def large_case_data(field, case):
    """case_data, computed once for the CPU harness test and the GPU test of one session"""
    return case_data(field, case)


def case_data(field, case):
    """-> (omega, shift or None, stored input words (batch * n), expected stored output words)"""
    name, lg, _t, batch, fl, sk, _ip = case
    p = FIELDS[field][2]
    n = 1 << lg
    omega = root_of_unity(p, lg)
    shift = None if sk is None else root_of_unity(p, lg + 1) if sk == "w2n" else random.Random("g" + name).randrange(1, p)
    stored = stored_inputs(p, batch * n, field + name)
    want = []
    for b in range(batch):
        row = decode(stored[b * n:(b + 1) * n], p, bool(fl & IN_MONT))
        res = ntt(row, p, omega, bool(fl & INVERSE), bool(fl & IN_BRP), bool(fl & OUT_BRP), shift)
        want += encode(res, p, bool(fl & OUT_MONT))
    return omega, shift, stored, want
