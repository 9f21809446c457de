"""
The group law below the MSM, one formula at a time: ec.h (xyzz_madd_flag, xyzz_madd_core, xyzz_add_inl, xyzz_dbl, xyzz_mdbl and
the twisted Edwards law behind the same names) and the four-lane forms of hip_backend.h (xyzz_add_quad, xyzz_add_quad_reg,
xyzz_dbl_quad_reg), through the probe ops 32 + op of ctt_hip_field_op (msm_bodies.h ec_probe) -- on the CPU through tests/emu for
every op that is host/device code, on the GPU for all of them.

Operands are RAW device records, so the test chooses the representative of every coordinate: the carry-free field (fpu.h) keeps
x*R' mod p only up to a multiple of p, and every formula of ec.h states the multiples it accepts (X < 9p, Y < 4p, ZZ, ZZZ < 2p;
affine x, y < 2p).  Each coordinate is stored as x~ + k*p with k over that whole range, on ordinary sums and on every exceptional
case (a neutral operand, b = a as a different record, b = -a, the mixed forms against the accumulator's own point with both signs).
Expected values come from the Python-integer oracles only (oracle/pyoracle.py, tests/_banderwagon.py).

Per result: limbs normalised; every coordinate inside the contract the consumers state; the decoded affine point equals the
oracle's; the flag word (is_inf() as the code sees it) is set exactly when ZZ == 0 (mod p); the register forms hold four identical
copies; the memory form writes d1 == d2, and the same d1 without d2.
"""
import random
import time

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import _banderwagon as bw

BW = "banderwagon"
# (limb bits, limbs per base-field element, degree, carry-free): fpu.h / field_params.h; the CPU leg holds it against the emulator's
FIELD = {"bls12_381_g1": (28, 14, 1, True), "bls12_381_g2": (28, 14, 2, True), "bn254_snarks_g1": (29, 9, 1, True),
         "bn254_snarks_g2": (32, 8, 2, False), "pallas": (29, 9, 1, True), "vesta": (29, 9, 1, True), BW: (32, 8, 1, False)}
ALL = list(FIELD)
# stated input ranges of ec.h in units of p (exclusive): record X, Y, ZZ, ZZZ and affine x, y -- the widest any producer states
# (xyzz_madd_flag: X < XYZZ_XB = 9; the four-lane forms: X < 4M = 8, Y < 2M = 4; xyzz_dbl: Y < 4)
REC_BOUND = (9, 4, 2, 2)
AFF_BOUND = (2, 2)
OP_MADD_FLAG, OP_MADD_CORE, OP_ADD, OP_DBL, OP_MDBL = 0, 4, 8, 9, 10
OP_QUAD_MEM2, OP_QUAD_MEM1, OP_QUAD_ADD_REG, OP_QUAD_DBL_REG = 16, 17, 18, 19
COPIES = {OP_QUAD_MEM2: 2, OP_QUAD_ADD_REG: 4, OP_QUAD_DBL_REG: 4}


def _sqrt(v, p):
    """a square root of v mod p, or None (Tonelli-Shanks)"""
    v %= p
    if v == 0:
        return 0
    if pow(v, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(v, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(v, q, p), pow(v, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


class Law:
    """One curve: its field representation on the device, its records and its oracle."""

    def __init__(self, name):
        self.name = name
        self.lb, self.nl, self.deg, self.unsat = FIELD[name]
        self.edwards = name == BW
        if self.edwards:
            self.F = po.FpField(bw.P)
            self.neutral = bw.O
        else:
            self.curve = po.CURVES[name]
            self.F = self.curve.F
            self.neutral = None
        self.p = self.F.p
        self.Rr = 1 << (self.lb * self.nl)          # R' of the device representation (2^256 for the Montgomery fields)
        self.Rr_inv = pow(self.Rr, -1, self.p)
        self.cw = self.nl * self.deg                 # words of a coordinate
        self.rw = 4 * self.cw                        # words of a record

    # ---- field representation --------------------------------------------------------------------------------------------
    def comps(self, v):
        return (v,) if self.deg == 1 else tuple(v)

    def elem(self, c):
        return c[0] if self.deg == 1 else tuple(c)

    def enc(self, v, k):
        """limbs of the element v with component j stored as (v_j R' mod p) + k_j p"""
        out = []
        mask = (1 << self.lb) - 1
        for c, kk in zip(self.comps(v), k):
            w = c * self.Rr % self.p + kk * self.p
            for i in range(self.nl - 1):
                out.append(w & mask)
                w >>= self.lb
            assert w < (1 << 32)
            out.append(w)
        return out

    def dec(self, words):
        """-> (element, [stored integer per component]); asserts the limbs are normalised"""
        raw = []
        for j in range(self.deg):
            part = [int(x) for x in words[j * self.nl:(j + 1) * self.nl]]
            assert all(x < (1 << self.lb) for x in part[:-1]), "limbs must come back normalised"
            raw.append(sum(x << (self.lb * i) for i, x in enumerate(part)))
        return self.elem([r * self.Rr_inv % self.p for r in raw]), raw

    def rand_elem(self, rng, nonzero=True):
        while True:
            c = [rng.randrange(self.p) for _ in range(self.deg)]
            if not nonzero or any(c):
                return self.elem(c)

    def embed(self, v):
        return v if self.deg == 1 else (v, 0)

    # ---- oracle ----------------------------------------------------------------------------------------------------------
    def add(self, a, b):
        return bw.add(a, b) if self.edwards else self.curve.add(a, b)

    def neg(self, a):
        return bw.neg(a) if self.edwards else self.curve.neg(a)

    # ---- records ---------------------------------------------------------------------------------------------------------
    def coords(self, pt, z):
        """the record of the affine point pt with the free parameter z"""
        F = self.F
        x, y = pt
        if self.edwards:   # (X : Y : Z : T) = (xz, yz, z, xyz)
            return (F.mul(x, z), F.mul(y, z), z, F.mul(F.mul(x, y), z))
        z2 = F.sqr(z)
        z3 = F.mul(z2, z)
        return (F.mul(x, z2), F.mul(y, z3), z2, z3)

    def record(self, pt, z, ks):
        if pt is None:   # the all-zero record: the neutral element in memory (both laws)
            return [0] * self.rw
        out = []
        for v, k in zip(self.coords(pt, z), ks):
            out += self.enc(v, k)
        return out

    def aff_record(self, pt, ks):
        """second operand of the mixed forms: x, y of an affine point (ZZ, ZZZ are not read; they hold one)"""
        one = self.elem([1] + [0] * (self.deg - 1))
        zk = (0,) * self.deg
        return self.enc(pt[0], ks[0]) + self.enc(pt[1], ks[1]) + self.enc(one, zk) + self.enc(one, zk)

    def z_for_target(self, pt, t, which):
        """z (from the base field) that makes a stored residue equal t: component 0 of X (which = 0) or of ZZ / Z (1); None when
        there is none (t / x is not a square)"""
        p = self.p
        x0 = self.comps(pt[0])[0]
        den = self.Rr if which else x0 * self.Rr
        if den % p == 0:
            return None
        v = t * pow(den, -1, p) % p
        z = v if self.edwards else _sqrt(v, p)
        return self.embed(z) if z else None


# ---- representative multiples ---------------------------------------------------------------------------------------------
def _corner_ks(law, bound, rng, nrandom):
    """tuples (one per coordinate) of per-component multiples: the all-zero and all-maximal corners, every single maximum, and a
    seeded sample of the rest.  The Montgomery fields have one representative."""
    d = law.deg
    zero = tuple((0,) * d for _ in bound)
    if not law.unsat:
        return [zero]
    out = [zero, tuple((b - 1,) * d for b in bound)]
    for i, b in enumerate(bound):
        for j in range(d):
            k = [list(c) for c in zero]
            k[i][j] = b - 1
            out.append(tuple(tuple(c) for c in k))
    for _ in range(nrandom):
        out.append(tuple(tuple(rng.randrange(b) for _ in range(d)) for b in bound))
    return out


def _all_ks(law, bound, rng, nrandom):
    """every combination of the multiples (the same for both components of an extension element), plus a per-component sample"""
    d = law.deg
    if not law.unsat:
        return [tuple((0,) * d for _ in bound)]
    out = [()]
    for b in bound:
        out = [o + ((k,) * d,) for o in out for k in range(b)]
    if d > 1:
        for _ in range(nrandom):
            out.append(tuple(tuple(rng.randrange(b) for _ in range(d)) for b in bound))
    return out


class Cases:
    """Seeded, fixed case lists of one curve.  A case is (label, record a, record b, point a, point b)."""

    def __init__(self, name):
        law = self.law = Law(name)
        rng = self.rng = random.Random("ec-probe-" + name)
        p = law.p
        # points: generator multiples and points of unknown logarithm
        if law.edwards:
            gens = [bw.mul(k, bw.G) for k in (1, 2, 3, 7, bw.R - 1, rng.randrange(bw.R), rng.randrange(bw.R))]
            unknown = bw.crs(6)
            self.specials = [bw.O, (0, p - 1)]
        else:
            c = law.curve
            gens = [c.scalar_mul(k, c.gen) for k in (1, 2, 3, 7, c.order - 1, rng.randrange(c.order), rng.randrange(c.order))]
            raw = cref.gen_points_unknown_log(name, 4242, 6, nthreads=1)
            unknown = [c.aff_from_bytes(bytes(r)) for r in raw]
            self.specials = []
        self.points = gens + unknown
        for pt in self.points:
            assert bw.on_curve(pt) if law.edwards else law.curve.is_on_curve(pt)
        small = 24 if law.deg == 1 else 12
        self.rec_ks = _corner_ks(law, REC_BOUND, rng, small)
        self.aff_ks = _all_ks(law, AFF_BOUND, rng, 4)
        self.pair = self._pair_cases()
        self.mixed = self._mixed_cases()
        self.single = self._single_cases()
        self.affine = [("mdbl", law.aff_record(pt, k), law.aff_record(pt, k), pt, pt) for pt in self.points + self.specials
                       for k in self.aff_ks]

    def _z(self):
        return self.law.rand_elem(self.rng)

    def _rec(self, pt, ks=None, z=None):
        ks = ks if ks is not None else self.rng.choice(self.rec_ks)
        return self.law.record(pt, z if z is not None else self._z(), ks)

    def _targeted(self, pt):
        """records of pt whose stored X or ZZ residue sits on an edge"""
        law, p = self.law, self.law.p
        out = []
        for t in (1, 2, p - 1, p - 2, (p - 1) // 2):
            for which in (0, 1):
                z = law.z_for_target(pt, t, which)
                if z is None:
                    continue
                for ks in self.rec_ks[:2]:
                    rec = law.record(pt, z, ks)
                    _, raw = law.dec(rec[(2 * law.cw if which else 0):][:law.cw])
                    assert raw[0] % p == t   # the residue is where it was aimed
                    out.append(rec)
        return out

    def _pair_cases(self):
        law, rng = self.law, self.rng
        pts = self.points + self.specials
        out = []
        for i in range(160):   # ordinary sums
            a, b = rng.sample(self.points, 2)
            out.append(("a+b", self._rec(a), self._rec(b), a, b))
        for ks in self.rec_ks:   # every corner on either side of an ordinary sum
            a, b = rng.sample(self.points, 2)
            out.append(("a+b corner a", self._rec(a, ks), self._rec(b), a, b))
            out.append(("a+b corner b", self._rec(a), self._rec(b, ks), a, b))
        for a in self.points[:3] + self.points[-2:]:
            b = rng.choice([q for q in self.points if q != a])
            for rec in self._targeted(a):
                out.append(("a+b edge residue a", rec, self._rec(b), a, b))
                out.append(("a+b edge residue b", self._rec(b), rec, b, a))
                out.append(("a+a edge residue", rec, self._rec(a), a, a))
        zero = law.record(None, None, None)
        out.append(("0+0", zero, zero, law.neutral, law.neutral))
        for ks in self.rec_ks:   # a neutral operand
            a = rng.choice(pts)
            out.append(("a+0", self._rec(a, ks), zero, a, law.neutral))
            out.append(("0+b", zero, self._rec(a, ks), law.neutral, a))
        for a in (self.points[0], self.points[-1]):   # b = +-a as a different record (other z, other multiples)
            for ka in self.rec_ks:
                for kb in self.rec_ks:
                    out.append(("a+a", self._rec(a, ka), self._rec(a, kb), a, a))
                    out.append(("a-a", self._rec(a, ka), self._rec(law.neg(a), kb), a, law.neg(a)))
        if law.unsat:
            # the products U1 = X1 ZZ2, U2 = X2 ZZ1 leave the Montgomery reduction above p only with probability ~ k1 k2 p / R':
            # many equal-point sums with the largest multiples, so that P = U2 - U1 + c p meets every multiple of p in its range
            top = tuple((b - 1,) * law.deg for b in REC_BOUND)
            for i in range(1200):
                a = self.points[i % len(self.points)]
                b = a if i & 1 else law.neg(a)
                out.append(("a+-a largest multiples", self._rec(a, top), self._rec(b, top), a, b))
        for s in self.specials:   # twisted Edwards: (0, 1) as (0 : c : c : 0), (0, -1), against points, themselves and the zero record
            for t in pts:
                out.append(("special+b", self._rec(s), self._rec(t), s, t))
                out.append(("a+special", self._rec(t), self._rec(s), t, s))
            out.append(("special+0", self._rec(s), zero, s, law.neutral))
            out.append(("0+special", zero, self._rec(s), law.neutral, s))
        return out

    def _mixed_cases(self):
        law, rng = self.law, self.rng
        pts = self.points + self.specials
        out = []
        for i in range(160):
            a, q = rng.sample(self.points, 2)
            out.append(("acc+-q", self._rec(a), law.aff_record(q, rng.choice(self.aff_ks)), a, q))
        for ks in self.rec_ks:
            for kq in self.aff_ks:
                a, q = rng.sample(self.points, 2)
                out.append(("acc+-q corner", self._rec(a, ks), law.aff_record(q, kq), a, q))
        for a in self.points[:2] + self.points[-2:]:
            q = rng.choice([t for t in self.points if t != a])
            for rec in self._targeted(a):
                out.append(("acc+-q edge residue", rec, law.aff_record(q, rng.choice(self.aff_ks)), a, q))
                out.append(("acc+-acc edge residue", rec, law.aff_record(a, rng.choice(self.aff_ks)), a, a))
        # q = the accumulator's point and its negative (each op applies its own sign of the digit): every combination of multiples
        every = _all_ks(law, REC_BOUND, rng, 64)
        for a in (self.points[1], self.points[-1]):
            for ks in every:
                for kq in self.aff_ks:
                    out.append(("acc+-acc", self._rec(a, ks), law.aff_record(a, kq), a, a))
                    out.append(("acc-+acc", self._rec(a, ks), law.aff_record(law.neg(a), kq), a, law.neg(a)))
        for s in self.specials:
            for t in pts:
                for kq in self.aff_ks:
                    out.append(("special+-q", self._rec(s), law.aff_record(t, kq), s, t))
                    out.append(("acc+-special", self._rec(t), law.aff_record(s, kq), t, s))
        return out

    def _single_cases(self):
        law = self.law
        out = [("2*0", law.record(None, None, None), law.record(None, None, None), law.neutral, law.neutral)]
        for a in self.points + self.specials:
            for ks in self.rec_ks:
                r = self._rec(a, ks)
                out.append(("2a", r, r, a, a))
        for a in self.points[:3]:
            for r in self._targeted(a):
                out.append(("2a edge residue", r, r, a, a))
        return out


_CASES = {}


def cases_of(name):
    if name not in _CASES:
        _CASES[name] = Cases(name)
    return _CASES[name]


def ops_of(law, quad):
    """(op, case list name, expected(a, b) -> point) for every op the curve has"""
    dbl = lambda a, b: law.add(a, a)
    ops = []
    for base in (OP_MADD_FLAG,) if law.edwards else (OP_MADD_FLAG, OP_MADD_CORE):
        ops += [(base + 0, "mixed", lambda a, b: law.add(a, b)), (base + 1, "mixed", lambda a, b: law.add(a, law.neg(b))),
                (base + 2, "mixed", lambda a, b: b), (base + 3, "mixed", lambda a, b: law.neg(b))]   # (+ 2: empty = true)
    ops += [(OP_ADD, "pair", law.add), (OP_DBL, "single", dbl), (OP_MDBL, "affine", dbl)]
    if quad:
        ops += [(OP_QUAD_MEM2, "pair", law.add), (OP_QUAD_MEM1, "pair", law.add), (OP_QUAD_ADD_REG, "pair", law.add),
                (OP_QUAD_DBL_REG, "single", dbl)]
    return ops


def check_result(law, words, want, ctx):
    """one result record + flag word against the oracle's point; returns the decoded affine point"""
    F, p, cw = law.F, law.p, law.cw
    flag = int(words[law.rw])
    assert flag in (0, 1), ctx
    el, raws = [], []
    for i in range(4):
        e, raw = law.dec(words[i * cw:(i + 1) * cw])   # (1) limbs normalised
        el.append(e)
        raws.append(raw)
        bound = REC_BOUND[i] if law.unsat else 1       # (2) inside the contract of every consumer
        assert all(r < bound * p for r in raw), (ctx, "coordinate %d outside its bound" % i, [r // p for r in raw])
    X, Y, ZZ, ZZZ = el
    # (4) the code's own neutral test must agree with ZZ == 0 (mod p)
    assert (flag == 1) == F.is_zero(ZZ), (ctx, "is_inf() %d but ZZ %s 0 (mod p)" % (flag, "==" if F.is_zero(ZZ) else "!="))
    if flag:
        assert not any(int(w) for w in words[:law.rw]), (ctx, "a neutral result is the all-zero record")
        assert want == law.neutral, (ctx, "neutral result, expected", want)
        return law.neutral
    if law.edwards:
        iz = F.inv(ZZ)
        got = (F.mul(X, iz), F.mul(Y, iz))
        assert F.mul(ZZZ, ZZ) == F.mul(X, Y), (ctx, "T Z != X Y")
    else:
        got = (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))
        assert F.mul(F.sqr(ZZ), ZZ) == F.sqr(ZZZ), (ctx, "ZZ^3 != ZZZ^2")
    assert got == want, (ctx, "decoded point differs from the oracle's")   # (3)
    return got


def run_all(name, run, quad):
    """every op of the curve over its case lists; run(op, a, b) -> (n, copies, rw + 1) uint32"""
    cs = cases_of(name)
    law = cs.law
    counts = {}
    points = {}
    raw_out = {}
    for op, lst, fn in ops_of(law, quad):
        cases = getattr(cs, lst)
        a = np.array([c[1] for c in cases], dtype=np.uint32)
        b = np.array([c[2] for c in cases], dtype=np.uint32)
        out = run(op, a, b)
        copies = COPIES.get(op, 1)
        assert out.shape == (len(cases), copies, law.rw + 1), (name, op, out.shape)
        raw_out[op] = out
        got = []
        memo = {}
        for i, c in enumerate(cases):
            ctx = (name, "op", op, c[0], "case", i)
            for k in range(1, copies):   # (5), (6): every copy bit-identical
                assert np.array_equal(out[i, k], out[i, 0]), (ctx, "copy %d differs from copy 0" % k)
            key = (c[3], c[4])
            if key not in memo:
                memo[key] = fn(c[3], c[4])
            got.append(check_result(law, out[i, 0], memo[key], ctx))
        points[op] = got
        counts[op] = len(cases)
    if quad:
        # the memory form without d2 writes the same d1
        assert np.array_equal(raw_out[OP_QUAD_MEM1][:, 0], raw_out[OP_QUAD_MEM2][:, 0]), (name, "d1 differs without d2")
        # the four-lane forms and the one-lane formulas give the same group element on the same inputs
        for q, s in ((OP_QUAD_MEM2, OP_ADD), (OP_QUAD_MEM1, OP_ADD), (OP_QUAD_ADD_REG, OP_ADD), (OP_QUAD_DBL_REG, OP_DBL)):
            assert points[q] == points[s], (name, q, s)
    print("%s: cases per op %s, total %d" % (name, counts, sum(counts.values())))
    return counts


# ---- CPU: the emulator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_group_law_probe_emulator(name):
    from tests.emu import emu
    law = Law(name)
    info = emu.dev_field_info(name)
    assert (info is not None) == law.unsat
    if info:
        assert info == (law.lb, law.nl * law.deg)
    t0 = time.time()

    def run(op, a, b):
        out = emu.ec_op(name, op, a, b, law.rw)
        assert out is not None, (name, op)
        return out.reshape(a.shape[0], 1, law.rw + 1)

    counts = run_all(name, run, quad=False)
    assert len(counts) == (7 if law.edwards else 11)   # every host/device op ran
    # ops the curve does not have, and the four-lane forms, are refused
    z = np.zeros((1, law.rw), dtype=np.uint32)
    for op in (-1, 11, 15, 16, 17, 18, 19, 20) + ((4, 5, 6, 7) if law.edwards else ()):
        assert emu.ec_op(name, op, z, z, law.rw) is None
    print("%s: %.1f s" % (name, time.time() - t0))


def test_case_counts_are_fixed():
    """the generated lists are seeded: the same cases on every run and every machine"""
    a, b = Cases("pallas"), Cases("pallas")
    for lst in ("pair", "mixed", "single", "affine"):
        assert getattr(a, lst) == getattr(b, lst)
        assert len(getattr(a, lst)) > 0


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
@pytest.mark.parametrize("name", ALL)
def test_group_law_probe_gpu(name, dev):
    import torch
    law = Law(name)
    t0 = time.time()

    def run(op, a, b):
        n = a.shape[0]
        copies = COPIES.get(op, 1)
        da = torch.from_numpy(a.astype(np.int32)).cuda()
        db = torch.from_numpy(b.astype(np.int32)).cuda()
        dr = torch.full((n, copies, law.rw + 1), -1, dtype=torch.int32, device="cuda")
        dev.field_op(name, 32 + op, da, db, dr, n)
        return dr.cpu().numpy().astype(np.uint32)

    counts = run_all(name, run, quad=True)
    assert len(counts) == (11 if law.edwards else 15)
    # ops the curve does not have are refused before anything is launched
    z = torch.zeros((1, 4, law.rw + 1), dtype=torch.int32, device="cuda")
    for op in (11, 15, 20) + ((4, 5, 6, 7) if law.edwards else ()):
        with pytest.raises(RuntimeError):
            dev.field_op(name, 32 + op, z, z, z, 1)
    print("%s: %.1f s" % (name, time.time() - t0))
