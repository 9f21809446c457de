"""
The fields below the group law, one operation at a time, against Python integers: Montgomery arithmetic (fp.h) and the modular
inversion by division steps (modinv.h: signed 30-bit limbs, batches of 30 steps, a sign fix-up, a repack to 32-bit words) -- for
every modulus the library instantiates them with: the coordinate field F and the scalar field C::Fr of all seven curves.

The probe ops of ctt_hip_field_op (msm_bodies.h field_probe; tests/emu runs the same function on the CPU):
    k         0 mul   1 sqr   2 add   3 sub   4 neg   5 inv   6 inv_fermat (Fp2: inv again)   7 from_mont   8 to_mont
    0 + k     coordinate field, k = 0 .. 6, short Weierstrass curves only (refused for Banderwagon)
    64 + k    coordinate field, k = 0 .. 6, every curve
    80 + k    scalar field, k = 0 .. 8, every curve, rows of 32 bytes
(32 .. 51 are the group law, tests/test_ec_probe.py.)  Every other number is refused before anything is launched.

One seeded, fixed case list per (curve, field) drives two legs: the emulator (CPU) and the device (GPU).  Expected values come from
Python integers only (pow(a, -1, m), %, and oracle/pyoracle.py's Fp2 formulas over them); every comparison is exact.

Per (curve, field): inv equals pow(a, -1, m) and inv(0) = 0; the stored result is canonical (< m); op 5 and op 6 agree bytewise;
inv(inv(a)) gives the input bytes back; mul(a, inv(a)) is the Montgomery one; mul / sqr / add / sub / neg equal Python's; the scalar
field's from_mont / to_mont equal a * R^-1 / a * R and undo each other; on the device the numbers 0 + k and 64 + k give the same bytes.
"""
import random
import time

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import _banderwagon as bw

BW = "banderwagon"
ALL = list(po.CURVES) + [BW]
OP_F, OP_F_ALL, OP_FR = 0, 64, 80          # the three number ranges of ctt_hip_field_op
MUL, SQR, ADD, SUB, NEG, INV, INV_FERMAT, FROM_MONT, TO_MONT = range(9)
N_UNIFORM, N_PAIRS, N_FP2_PAIRS = 2048, 2048, 1024
PAIRS = [(name, field) for name in ALL for field in ("F", "Fr")]


def modulus_of(name, field):
    """(modulus, extension degree) of the curve's coordinate field ("F") or scalar field ("Fr")"""
    if name == BW:
        return (bw.P, 1) if field == "F" else (bw.R, 1)
    c = po.CURVES[name]
    if field == "Fr":
        return c.Fr.p, 1
    return (c.F.p, 1) if c.F.degree == 1 else (c.F.base.p, 2)


class Mod:
    """A modulus as fp.h and modinv.h see it: N 32-bit words (whole 64-bit limbs), R = 2^(32 N), L signed 30-bit limbs."""

    def __init__(self, m):
        self.m = m
        self.b = m.bit_length()
        self.N = 2 * ((self.b + 63) // 64)
        self.nbytes = 4 * self.N
        self.R = (1 << (32 * self.N)) % m
        self.Rinv = pow(self.R, -1, m)
        self.L = (self.b + 2 + 29) // 30      # ModInv::L

    def structured(self):
        """the edge values of the issue's list, in [0, m), each once, in a fixed order"""
        m, b, R, Ri = self.m, self.b, self.R, self.Rinv
        M30 = (1 << 30) - 1
        v = [0] + list(range(1, 65)) + [m - i for i in range(1, 65)]
        for k in range(b):
            v += [1 << k, (1 << k) - 1, (1 << k) + 1, m - (1 << k), m - (1 << k) - 1, m - (1 << k) + 1]
        v += [(m + 1) // 2, (m - 1) // 2, R, R * R % m, R * R * R % m, Ri, Ri * Ri % m]
        # limb boundaries of both radices: 30-bit limbs of ModInv, 32-bit words of Fp
        for i in range(self.L):
            v += [(1 << (30 * i)) - 1, M30 << (30 * i)]
        for j in range(self.N):
            v.append(0xffffffff << (32 * j))
        v.append((1 << (b - 1)) - 1)
        even = sum(M30 << (30 * i) for i in range(0, self.L, 2))
        odd = sum(M30 << (30 * i) for i in range(1, self.L, 2))
        v += [even % m, odd % m]
        seen, out = set(), []
        for x in v:
            if 0 <= x < m and x not in seen:
                seen.add(x)
                out.append(x)
        return out


def to_rows(elems, nbytes):
    """elements (tuples of stored integers, one per component) -> (n, deg * nbytes) uint8"""
    buf = b"".join(c.to_bytes(nbytes, "little") for e in elems for c in e)
    return np.frombuffer(buf, dtype=np.uint8).reshape(len(elems), -1).copy()


def from_rows(rows, nbytes):
    out = []
    for row in rows:
        raw = row.tobytes()
        out.append(tuple(int.from_bytes(raw[o:o + nbytes], "little") for o in range(0, len(raw), nbytes)))
    return out


class Cases:
    """Seeded, fixed case lists of one (curve, field).  Elements are tuples of STORED integers (Montgomery residues a * R mod m),
    one per component; the value of a component s is s * R^-1 mod m."""

    def __init__(self, name, field):
        self.name, self.field = name, field
        m, self.deg = modulus_of(name, field)
        M = self.mod = Mod(m)
        rng = random.Random("field-probe-%s-%s" % (name, field))
        S = self.S = M.structured()
        # the list twice: the listed integer as the value a (stored a * R), and as the stored residue itself -- inv_words acts on
        # the stored words -- then the uniform values
        self.edges = [v * M.R % m for v in S] + list(S)
        comps = self.comps = self.edges + [rng.randrange(m) for _ in range(N_UNIFORM)]
        if self.deg == 1:
            self.unary = [(s,) for s in comps]
        else:
            self.unary = []
            for s in comps:
                self.unary += [(s, 0), (0, s), (s, s), (s, (m - s) % m)]
            self.unary += [(rng.choice(comps), rng.choice(comps)) for _ in range(N_FP2_PAIRS)]

        def operand():   # 50/50 from the structured list and uniform values, per component
            return tuple(rng.choice(self.edges) if rng.random() < 0.5 else rng.randrange(m) for _ in range(self.deg))

        self.pa = [operand() for _ in range(N_PAIRS)]
        self.pb = [operand() for _ in range(N_PAIRS)]
        self.unary_rows = to_rows(self.unary, M.nbytes)
        self.pa_rows = to_rows(self.pa, M.nbytes)
        self.pb_rows = to_rows(self.pb, M.nbytes)
        self._want = {}

    # ---- Python-integer references (computed once, shared by both legs) ----------------------------------------------------------
    def value(self, e):
        M = self.mod
        return tuple(s * M.Rinv % M.m for s in e)

    def stored(self, v):
        M = self.mod
        return tuple(c * M.R % M.m for c in v)

    def want_inv(self):
        """values of 1 / a for the unary list (0 for a = 0)"""
        if "inv" not in self._want:
            m = self.mod.m
            F2 = po.Fp2Field(po.FpField(m))
            out = []
            for e in self.unary:
                a = self.value(e)
                if not any(a):
                    out.append((0,) * self.deg)
                elif self.deg == 1:
                    out.append((pow(a[0], -1, m),))
                else:
                    out.append(tuple(F2.inv(a)))
            self._want["inv"] = out
        return self._want["inv"]

    def want_binary(self, k):
        """rows of the stored results of op k over the pair list"""
        if k not in self._want:
            m = self.mod.m
            F = po.FpField(m) if self.deg == 1 else po.Fp2Field(po.FpField(m))
            fn = {MUL: F.mul, SQR: lambda x, y: F.sqr(x), ADD: F.add, SUB: F.sub, NEG: lambda x, y: F.neg(x)}[k]
            out = []
            for ea, eb in zip(self.pa, self.pb):
                a, b = self.value(ea), self.value(eb)
                r = fn(a[0], b[0]) if self.deg == 1 else fn(a, b)
                out.append(self.stored((r,) if self.deg == 1 else tuple(r)))
            self._want[k] = to_rows(out, self.mod.nbytes)
        return self._want[k]


_CASES = {}


def cases_of(name, field):
    if (name, field) not in _CASES:
        _CASES[(name, field)] = Cases(name, field)
    return _CASES[(name, field)]


def same_rows(got, want, ctx):
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError((ctx, "first differing element", i, bytes(got[i]).hex(), "expected", bytes(want[i]).hex()))


def run_all(name, field, run):
    """every op of the field over its case lists; run(k, a, b) -> rows like a (uint8)"""
    cs = cases_of(name, field)
    M, deg = cs.mod, cs.deg
    m, nb = M.m, M.nbytes
    a = cs.unary_rows
    n = a.shape[0]
    ctx = (name, field)
    counts = {}
    # mul, sqr, add, sub, neg against Python
    for k in (MUL, SQR, ADD, SUB, NEG):
        same_rows(run(k, cs.pa_rows, cs.pb_rows), cs.want_binary(k), ctx + ("op", k))
        counts[k] = len(cs.pa)
    # inversion by division steps
    inv = run(INV, a, a)
    assert inv.shape == a.shape, ctx
    want = cs.want_inv()
    for i, (raw, w) in enumerate(zip(from_rows(inv, nb), want)):
        assert all(c < m for c in raw), (ctx, "inv: stored result not canonical", i, cs.unary[i])
        assert cs.value(raw) == w, (ctx, "inv differs from pow(a, -1, m)", i, "stored input", [hex(s) for s in cs.unary[i]])
    zero = [i for i, e in enumerate(cs.unary) if not any(e)]
    assert zero and not inv[zero].any(), (ctx, "inv(0) must be 0")
    # ... equals Fermat's a^(m-2) bytewise (Fp2: the same code twice)
    same_rows(run(INV_FERMAT, a, a), inv, ctx + ("op 6 against op 5",))
    # ... is an involution on the stored bytes
    same_rows(run(INV, inv, inv), a, ctx + ("inv(inv(a)) against a",))
    # ... and a * (1 / a) is the Montgomery one (0 for a = 0), by the probe's own product
    one = to_rows([cs.stored((1,) + (0,) * (deg - 1))], nb)[0]
    ones = np.tile(one, (n, 1))
    ones[zero] = 0
    same_rows(run(MUL, a, inv), ones, ctx + ("a * inv(a) against one",))
    counts[INV] = n
    if field == "Fr":
        # from_mont: a * R in, the words of a out; to_mont the reverse, on every stored integer of the list taken as canonical words
        canon = to_rows([cs.value(e) for e in cs.unary], nb)
        same_rows(run(FROM_MONT, a, a), canon, ctx + ("from_mont",))
        same_rows(run(TO_MONT, canon, canon), a, ctx + ("to_mont",))
        up = run(TO_MONT, a, a)
        same_rows(up, to_rows([cs.stored(e) for e in cs.unary], nb), ctx + ("to_mont of the stored words",))
        same_rows(run(FROM_MONT, up, up), a, ctx + ("from_mont(to_mont(x)) against x",))
        counts[FROM_MONT] = counts[TO_MONT] = n
    print("%s %s: %d bits, %d structured values, cases per op %s" % (name, field, M.b, len(cs.S), counts))
    return counts


# ---- CPU: the emulator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,field", PAIRS)
def test_field_probe_emulator(name, field):
    from tests.emu import emu
    t0 = time.time()
    fn = emu.field_op_n if field == "F" else emu.fr_op

    def run(k, a, b):
        out = fn(name, k, a, b)
        assert out is not None, (name, field, k)
        return out

    counts = run_all(name, field, run)
    assert len(counts) == (6 if field == "F" else 8)
    print("%s %s: %.1f s" % (name, field, time.time() - t0))


@pytest.mark.parametrize("name", ALL)
def test_refusals_emulator(name):
    """ops outside the tables are refused and write nothing (emu._rows_op checks the buffer); Banderwagon's coordinate field is served
    like every other"""
    from tests.emu import emu
    m, deg = modulus_of(name, "F")
    zf = np.zeros((2, Mod(m).nbytes * deg), dtype=np.uint8)
    for op in (-1,) + tuple(range(7, 16)) + (16, 24, 31, 32, 48, 64, 71, 80, 1 << 20):
        assert emu.field_op_n(name, op, zf) is None, (name, op)
    zr = np.zeros((2, 32), dtype=np.uint8)
    for op in (-1,) + tuple(range(9, 16)) + (16, 32, 48, 57, 63, 64, 80, 1 << 20):
        assert emu.fr_op(name, op, zr) is None, (name, op)
    for k in range(7):
        out = emu.field_op_n(name, k, zf)
        assert out is not None and not out.any(), (name, k)
    for k in range(9):
        out = emu.fr_op(name, k, zr)
        assert out is not None and not out.any(), (name, k)


def test_case_lists_are_fixed():
    """the generated lists are seeded: the same cases on every run and every machine, and they hold what they are meant to"""
    for name, field in (("pallas", "F"), ("bn254_snarks_g2", "F"), (BW, "Fr")):
        a, b = Cases(name, field), Cases(name, field)
        for lst in ("S", "unary", "pa", "pb"):
            assert getattr(a, lst) == getattr(b, lst)
            assert len(getattr(a, lst)) > 0
        assert np.array_equal(a.unary_rows, b.unary_rows)
    c = Cases("pallas", "F")
    M = c.mod
    assert (M.b, M.N, M.L) == (255, 8, 9) and Mod(bw.R).b == 253 and Mod(po.CURVES["bls12_381_g1"].F.p).N == 12
    S = set(c.S)
    for v in (0, 1, 64, M.m - 1, M.m - 64, 1 << 254, M.m - (1 << 254) + 1, (M.m + 1) // 2, M.R, M.Rinv, (1 << 30) - 1,
              ((1 << 30) - 1) << 210, 0xffffffff << 192, (1 << 254) - 1):
        assert v in S, hex(v)
    assert len(c.unary) == 2 * len(c.S) + N_UNIFORM
    assert len(Cases("bn254_snarks_g2", "F").unary) == 4 * (2 * len(Mod(po.CURVES["bn254_snarks_g1"].F.p).structured())
                                                            + N_UNIFORM) + N_FP2_PAIRS
    # every stored residue of the structured list is met both ways round
    assert (1,) in c.unary and (M.R,) in c.unary and ((M.m - 1) * M.R % M.m,) in c.unary


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,field", PAIRS)
def test_field_probe_gpu(name, field, dev):
    import torch
    t0 = time.time()
    bases = (OP_FR,) if field == "Fr" else (OP_F_ALL,) if name == BW else (OP_F_ALL, OP_F)

    def run(k, a, b):
        n = a.shape[0]
        da = torch.from_numpy(a).cuda()
        db = torch.from_numpy(b).cuda()
        outs = []
        for base in bases:
            dr = torch.full_like(da, 0xA5)
            dev.field_op(name, base + k, da, db, dr, n)
            outs.append(dr.cpu().numpy())
        for o in outs[1:]:   # the coordinate field under both of its numbers
            same_rows(o, outs[0], (name, field, "op %d against op %d" % (bases[1] + k, bases[0] + k)))
        return outs[0]

    counts = run_all(name, field, run)
    assert len(counts) == (6 if field == "F" else 8)
    print("%s %s: %.1f s" % (name, field, time.time() - t0))


REFUSED = (-1,) + tuple(range(7, 16)) + tuple(range(24, 32)) + tuple(range(43, 48)) + tuple(range(52, 64)) + tuple(range(71, 80)) \
    + tuple(range(89, 100)) + (127, 128, 255, 256, 1 << 16, (1 << 31) - 1)
REFUSED_BW = tuple(range(0, 7)) + tuple(range(16, 24)) + tuple(range(36, 40))   # the ops below 32 and the holder form: not Banderwagon's


@pytest.mark.gpu
def test_refusals_gpu(dev):
    """an op outside the tables is refused before anything is launched: RuntimeError, and the output buffer keeps its sentinel"""
    import torch
    za = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    zr = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    keep = zr.clone()
    for name in ALL:
        for op in REFUSED + (REFUSED_BW if name == BW else ()):
            with pytest.raises(RuntimeError):
                dev.field_op(name, op, za, za, zr, 1)
            dev.sync()
            assert torch.equal(zr, keep), (name, op)
    # Banderwagon: 0 refused (above), 64 + 0 served
    M = Mod(bw.P)
    a = torch.from_numpy(to_rows([(3 * M.R % M.m,), (M.m - 1,)], M.nbytes)).cuda()
    b = torch.from_numpy(to_rows([(5 * M.R % M.m,), (M.m - 1,)], M.nbytes)).cuda()
    r = torch.full_like(a, 0xA5)
    dev.field_op(BW, OP_F_ALL + MUL, a, b, r, 2)
    assert from_rows(r.cpu().numpy(), M.nbytes) == [(15 * M.R % M.m,), ((M.m - 1) * (M.m - 1) * M.Rinv % M.m,)]
