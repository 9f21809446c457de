"""
Banderwagon through the CPU emulator (tests/emu: the per-thread bodies of csrc/msm_bodies.h and the host orchestration of
msm_pipeline.h, kernel launches replaced by loops), case by case what tests/test_emu_pipeline.py does for the short-Weierstrass
curves, plus the inputs where the twisted Edwards law has conventions of its own: the affine neutral (0, 1), the order-two point
(0, -1), buckets whose sum is the law's neutral (0 : c : c : 0) -- an ordinary record with Z != 0, not the all-zero "neutral in
memory" -- and buckets that go on after that.

The oracle is tests/_banderwagon.py (Python integers; it shares no code with the engine): bw.msm_fast for inputs of a few hundred
points, and for generated points [sum k_i * synth_log(seed, i) mod r]G.  All comparisons are equalities of affine coordinates.
"""
import random

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests.emu import emu

BW = "banderwagon"
BIG = [(1 << 253) - 1, bw.R - 1, bw.R, bw.R + 1]   # large scalars: all window bits on, and the values around the group order


def _pts(points):
    return np.frombuffer(b"".join(bw.aff_bytes(p) for p in points), dtype=np.uint8).reshape(-1, 64).copy()


def _big(scalars):
    return np.frombuffer(b"".join(bw.big_bytes(k) for k in scalars), dtype=np.uint8).reshape(-1, 32).copy()


def _fr(scalars):
    return np.frombuffer(b"".join(bw.fr_bytes(k) for k in scalars), dtype=np.uint8).reshape(-1, 32).copy()


def _aff(out):
    return bw.aff_from(bytes(out))


def _fp(v):
    return np.frombuffer(bw.fp_bytes(v), dtype=np.uint8)


def _scalars(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1 << 253) for _ in range(n)]   # full width: about a quarter of them are >= r


def _gen(seed, n):
    """n generated points (the emulator's gen_point_body; checked against the oracle in test_gen_points_vs_oracle) and their logs"""
    return emu.gen_points(BW, seed, n), [bw.synth_log(seed, j) for j in range(n)]


def _by_logs(ks, logs):
    return bw.mul(sum(k * s for k, s in zip(ks, logs)) % bw.R, bw.G)


def _point(pts, j):
    return bw.aff_from(bytes(pts[j]))


def test_field_ops_vs_python():
    p = bw.P
    rng = random.Random(5)
    edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, 1 << 254, bw.MONT % p, pow(bw.MONT, -1, p)]

    def rnd():
        return rng.choice(edge) if rng.random() < 0.5 else rng.randrange(p)

    def op(o, a, b=None):
        return bw.fp_from(bytes(emu.field_op(BW, o, _fp(a), None if b is None else _fp(b))))

    pairs = [(a, b) for a in edge for b in edge] + [(rnd(), rnd()) for _ in range(60)]
    for a, b in pairs:
        assert op(0, a, b) == a * b % p, (a, b)
        assert op(1, a) == a * a % p, a
        assert op(2, a, b) == (a + b) % p, (a, b)
        assert op(3, a, b) == (a - b) % p, (a, b)
        assert op(4, a) == -a % p, a
    # inversion by division steps (modinv.h) against Python, and against a^(p-2) (op 6); inv(0) = 0
    for v in edge[1:] + [3, (p + 1) // 2] + [rng.randrange(1, p) for _ in range(60)]:
        v %= p
        assert op(5, v) == pow(v, -1, p), v
        assert op(6, v) == pow(v, -1, p), v
    assert op(5, 0) == 0 and op(6, 0) == 0


def test_no_carry_free_device_field():
    """Banderwagon computes in the canonical 32-bit-limb field on the device; the carry-free probe of
    test_carry_free_device_field_vs_python has nothing to probe.  The day the curve gets such a field this fails and the probe
    test has to follow."""
    assert emu.dev_field_info(BW) is None
    assert len(emu.field_op_dev(BW, 0, _fp(3), _fp(5))) == 0


def test_unsupported_operations_are_absent():
    """no Jacobian / projective batch conversion and no KZG quotient for the curve, as in the engine: the emulator answers -1"""
    z = np.zeros(96, np.uint8)
    L = emu.lib()
    assert L.emu_batch_affine(emu.CURVE_ID[BW], 1, emu._p(z), emu._p(z), 1, 8) == -1
    with pytest.raises(AssertionError):
        emu.batch_affine(BW, z)


def test_gen_points_vs_oracle():
    for seed, n, first in ((77, 5, 2), (77, 3, 0), (1, 2, 1 << 40)):
        out = emu.gen_points(BW, seed, n, first=first)
        for j in range(n):
            assert _point(out, j) == bw.mul(bw.synth_log(seed, j, first), bw.G), (seed, j, first)
    assert bw.synth_log(77, 2, 3) == bw.synth_log(77, 5) and bw.synth_log(77, 5, 0) == bw.synth_log(77, 5)
    # the generated points are subgroup elements on the curve
    for j in range(2):
        assert bw.on_curve(_point(out, j)) and bw.in_subgroup(_point(out, j))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 64, 300])
def test_msm_vs_oracle(n):
    pts, logs = _gen(3, n)
    ks = _scalars(4 + n, n)
    expect = bw.msm_fast(ks, [_point(pts, j) for j in range(n)])
    assert expect == _by_logs(ks, logs)          # the two oracle forms agree (and gen_points is what synth_log says)
    sc = _big(ks)
    # K < 0: the emulator harness routes the call through prepare_bases + submit(prepared) (cached-base path)
    for kw in (dict(), dict(c=3, K=4), dict(c=5, K=8), dict(c=7, K=4, S=1), dict(c=6, K=-8)):
        out, plan = emu.msm(BW, sc, pts, **kw)
        assert _aff(out) == expect, (kw, plan)
    prj, _ = emu.msm(BW, sc, pts, out_kind=2)
    assert bw.fp_from(bytes(prj[64:96])) == 1 and bw.prj_from(bytes(prj)) == expect


def test_msm_medium_default_plan():
    n = 5000
    pts, logs = _gen(13, n)
    ks = _scalars(14, n)
    expect = _by_logs(ks, logs)
    out, plan = emu.msm(BW, _big(ks), pts)
    assert _aff(out) == expect, plan
    out, plan = emu.msm(BW, _big(ks), pts, S=3, K=12)
    assert _aff(out) == expect, plan


def test_window_sizes_including_divisors_of_bits():
    """c | bits needs the extra top window; 253 = 11 * 23, so c = 11 is this curve's case.  The plan lays its windows over
    bits + 1 = 254 bits (the Booth carry of the top window): scalars with every bit on, and r - 1, r, r + 1, are among the inputs."""
    n = 200
    pts, logs = _gen(31, n)
    ks = _scalars(32, n)
    ks[:len(BIG)] = BIG
    for j in range(len(BIG), 20):
        ks[j] |= ((1 << 64) - 1) << 189            # force the top bits on for some scalars
    expect = _by_logs(ks, logs)
    assert expect == bw.msm_fast(ks, [_point(pts, j) for j in range(n)])
    for c in (2, 11, 16):
        out, plan = emu.msm(BW, _big(ks), pts, c=c, K=8)
        assert _aff(out) == expect, (c, plan)
        assert plan[0] == c and plan[1] == -(-254 // c), plan
    # one pair, every large scalar on its own (nothing to cancel a wrong top window against)
    P = _point(pts, 0)
    for k in BIG + [1 << 252, (1 << 253) - (1 << 242)]:
        for c in (0, 11):
            out, _ = emu.msm(BW, _big([k]), pts[:1], c=c)
            assert _aff(out) == bw.mul(k % bw.R, P), (k, c)


def test_all_equal_scalars_long_chains():
    """Every point lands in the same bucket per window: exercises tail/head chains and the merge tree."""
    n = 700
    pts, logs = _gen(41, n)
    ks = _scalars(42, 1) * n
    expect = _by_logs(ks, logs)
    for K in (4, 8, 28, 64):
        out, plan = emu.msm(BW, _big(ks), pts, c=6, K=K)
        assert _aff(out) == expect, (K, plan)


def test_all_equal_points_and_scalars_doubling_paths():
    """all points equal -> P == Q additions everywhere (the unified law has no doubling branch: it must simply be right)"""
    n = 257
    pts1, logs1 = _gen(51, 1)
    pts = np.tile(pts1, (n, 1))
    ks = _scalars(52, n)
    out, _ = emu.msm(BW, _big(ks), pts, c=4, K=4)
    assert _aff(out) == _by_logs(ks, logs1 * n)
    ks2 = ks[:1] * n
    out, _ = emu.msm(BW, _big(ks2), pts, c=5, K=8)
    assert _aff(out) == _by_logs(ks2, logs1 * n)


def test_neutral_inputs_cancellation_and_zero_scalars():
    P, Q = bw.mul(987654321, bw.G), bw.mul(5, bw.G)
    far = [bw.mul(1000 + i, bw.G) for i in range(6)]
    k = 0x1b3f5d7f9b1d3f5f7f9b1d3f5f7f9b1d3f5f7f9b1d3f5f7f9b1d3f5f7f9b1d3f
    cases = [
        ([5, 77, 5, 3, 0, 0], [bw.G, bw.O, bw.G, bw.neg(bw.G), bw.G, bw.O]),           # the Weierstrass test's input, (0, 1) for None
        ([4, 7, 1, 3, k, k + 1], [bw.O, bw.T2, bw.T2, bw.O, bw.T2, bw.O]),             # the neutral and (0, -1) alone
        ([k, 7, k, 3], [P, bw.T2, Q, bw.O]),                                           # ... and among ordinary points; odd scalar on (0, -1)
        ([12, 35, 56, k | 1], [bw.add(P, bw.T2), bw.add(Q, bw.T2), P, bw.add(bw.G, bw.T2)]),   # coset representatives P + (0, -1)
        # P next to -P with equal scalars, then further points with that scalar: every bucket of k first sums to the law's neutral
        # (a record with Z != 0) and then goes on
        ([k] * 5, [P, bw.neg(P)] + far[:3]),
        ([k] * 8, [P, bw.neg(P), Q, bw.neg(Q)] + far[:4]),
        ([k, k, 3, k, k, k], [far[0], P, Q, bw.neg(P), bw.neg(far[0]), far[1]]),
        ([0, 0, 0], [P, Q, bw.G]),                                                     # zero scalars
        ([0, k, 0], [P, Q, bw.T2]),
        ([bw.R, bw.R + 1, (1 << 253) - 1, bw.R - 1], [P, Q, bw.G, bw.T2]),             # scalars around and above r
    ]
    for ks, pts in cases:
        expect = bw.msm(ks, pts)
        assert expect == bw.msm_fast(ks, pts)
        for kw in (dict(), dict(c=3, K=4), dict(c=11, K=4), dict(c=5, K=-4), dict(c=4, K=64)):
            out, plan = emu.msm(BW, _big(ks), _pts(pts), **kw)
            assert _aff(out) == expect, (ks, pts, kw)
        out, _ = emu.msm_host(BW, _big(ks), _pts(pts), chunks=2)
        assert _aff(out) == expect, (ks, pts, "slices")
    # complete cancellations: (0, 1) in affine and (0, 1, 1) in projective form, whatever the route to it
    for ks, pts in (([9, 9], [bw.G, bw.neg(bw.G)]), ([k] * 4, [P, bw.neg(P), bw.neg(Q), Q]), ([0, 0, 0], [P, Q, bw.G]),
                    ([2, 4], [bw.T2, bw.T2]), ([bw.R], [P]), ([3, 3], [bw.O, bw.O]), ([], [])):
        sc, pa = (_big(ks), _pts(pts)) if ks else (np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8))
        for kw in (dict(), dict(c=5, K=4)):
            out, _ = emu.msm(BW, sc, pa, out_kind=0, **kw)
            assert _aff(out) == bw.O, (ks, kw)
            prj, _ = emu.msm(BW, sc, pa, out_kind=2, **kw)
            assert [bw.fp_from(bytes(prj[i:i + 32])) for i in (0, 32, 64)] == [0, 1, 1], (ks, kw)


def test_fr_coefs_entry():
    """fr_from_mont_body<Banderwagon_Fr>: coefficients in Montgomery form over the scalar field"""
    n = 50
    pts, logs = _gen(61, n)
    rng = random.Random(62)
    ks = [0, 1, bw.R - 1, 2, bw.R - 2, (bw.R - 1) // 2] + [rng.randrange(bw.R) for _ in range(n - 6)]
    expect = _by_logs(ks, logs)
    for kw in (dict(c=4), dict(), dict(c=11, K=-4)):
        out, _ = emu.msm(BW, _fr(ks), pts, coef_is_fr=True, **kw)
        assert _aff(out) == expect, kw
    for k in (0, 1, bw.R - 1):
        out, _ = emu.msm(BW, _fr([k]), pts[:1], coef_is_fr=True)
        assert _aff(out) == bw.mul(k * logs[0] % bw.R, bw.G), k


def _slices_input(n, seed):
    """the input shape of test_host_pointer_form_uploads_in_slices, with the Edwards cases added; returns (ks, pts, logs)"""
    pts, logs = _gen(seed, n)
    ks = _scalars(seed + 1, n)
    ks[:40] = [ks[0]] * 40                   # one heavy bucket per window that lives in the first slice only
    pts[7], logs[7] = _pts([bw.O])[0], 0     # the neutral (0, 1): an ordinary point to the law

    def put(j, k, src, sign):                # pair j := (k, sign * point src)
        ks[j], logs[j] = k, sign * logs[src]
        pts[j] = pts[src] if sign > 0 else _pts([bw.neg(_point(pts, src))])[0]

    put(n - 4, ks[45], 45, 1)                # the same pair again in the last slice: the stored sum is doubled
    put(n - 3, ks[46], 46, -1)               # the negative in the last slice: the stored sum becomes the law's neutral, Z != 0
    put(n // 2, ks[47], 47, -1)              # the negative in a middle slice ...
    ks[n - 2] = ks[47]                       # ... and a third point for that bucket after it: resumes from the stored neutral
    put(n - 5, ks[48], 48, -1)               # P, then (-P, Q) within the last slice
    ks[n - 1] = ks[48]
    return ks, pts, logs


def test_host_pointer_form_uploads_in_slices():
    """MsmEngine::submit_host: every slice is sorted on its own and accumulated INTO the one bucket set
    (accum_body<F, INTO = true> resumes from the stored bucket by is_inf()) -- same element for any number of slices."""
    n = 1201
    ks, pts, logs = _slices_input(n, 501)
    expect = _by_logs(ks, logs)
    for chunks, c in ((1, 0), (2, 0), (3, 5), (8, 0), (2, 11)):
        out, used = emu.msm_host(BW, _big(ks), pts, c=c, chunks=chunks)
        assert _aff(out) == expect, (chunks, c)
        assert used == chunks
    rng = random.Random(503)
    mont = [rng.randrange(1 << 250) for _ in range(n)]               # Fr elements given by their Montgomery residues
    expect = _by_logs([m * pow(bw.MONT, -1, bw.R) % bw.R for m in mont], logs)
    out, _ = emu.msm_host(BW, _big(mont), pts, coef_is_fr=True, chunks=3)
    assert _aff(out) == expect
    # the second half is the first half negated: every bucket the first slices filled is cancelled by the later ones
    m = 300
    hp, hl = _gen(505, m)
    hk = _scalars(506, m)
    neg = _pts([bw.neg(_point(hp, j)) for j in range(m)])
    for chunks in (1, 2, 4, 5):
        out, _ = emu.msm_host(BW, _big(hk + hk), np.concatenate([hp, neg]), chunks=chunks, c=6)
        assert _aff(out) == bw.O, chunks
        prj, _ = emu.msm_host(BW, _big(hk + hk), np.concatenate([hp, neg]), chunks=chunks, out_kind=2)
        assert [bw.fp_from(bytes(prj[i:i + 32])) for i in (0, 32, 64)] == [0, 1, 1], chunks
    # ... and goes on: a third part after the cancelled two
    tp, tl = _gen(507, m)
    tk = _scalars(508, m)
    for chunks in (3, 6):
        out, _ = emu.msm_host(BW, _big(hk + hk + hk[:m // 2] + tk[m // 2:]), np.concatenate([hp, neg, tp]), chunks=chunks, c=6)
        assert _aff(out) == _by_logs(hk[:m // 2] + tk[m // 2:], tl), chunks


def test_head_chains_of_every_length_class():
    """Buckets that span several accumulate lanes leave a chain of partial sums (heads) that the merge sums: chains of
    3 ... 250 heads next to ordinary buckets."""
    K = 4
    rng = np.random.default_rng(5)
    for n_equal in (9, 130, 255, 258, 262, 1000):       # chains of 3, 33, 64, 65, 66, 250 heads
        n = n_equal + 300
        pts, logs = _gen(700 + n_equal, n)
        ks = _scalars(701 + n_equal, n)
        idx = rng.permutation(n)[:n_equal]
        for j in idx:
            ks[j] = ks[idx[0]]                            # n_equal pairs share every bucket; the rest is spread out
        expect = _by_logs(ks, logs)
        for c in (5, 9):
            out, plan = emu.msm(BW, _big(ks), pts, c=c, K=K)
            assert _aff(out) == expect, (n_equal, c)


def test_head_merge_chain_form_and_tree_agree(monkeypatch):
    """The chain form of the head merge and the launch-per-level tree, every lmax class (every chain long, some long, none long),
    on inputs whose chains hold 1 ... 250 heads, a quarter-equal and an all-equal input, and a chain that starts with P, -P."""
    K = 4
    rng = np.random.default_rng(11)
    cases = []
    for n_equal in (0, 9, 40, 258):
        n = n_equal + 200
        pts, logs = _gen(1700 + n_equal, n)
        ks = _scalars(1701 + n_equal, n)
        if n_equal:
            idx = rng.permutation(n)[:n_equal]
            for j in idx:
                ks[j] = ks[idx[0]]
        cases.append((ks, pts, logs))
    pts, logs = _gen(1801, 300)
    cases.append((_scalars(1802, 1) * 300, pts, logs))                   # all equal: one chain per window
    pts, logs = _gen(1901, 90)
    ks = _scalars(1902, 90)
    ks[:40] = [ks[0]] * 40
    pts[1], logs[1] = _pts([bw.neg(_point(pts, 0))])[0], -logs[0]        # the chain's first piece sums to the law's neutral
    pts[5], logs[5] = _pts([bw.neg(_point(pts, 4))])[0], -logs[4]        # ... and so does its second (K = 4)
    pts[6], logs[6] = pts[7], logs[7]
    cases.append((ks, pts, logs))
    for ks, pts, logs in cases:
        expect = _by_logs(ks, logs)
        sc = _big(ks)
        for mode, lmax in ((2, 0), (1, 1), (1, 2), (1, 3), (1, 8), (1, 1000), (0, 0)):
            monkeypatch.setenv("EMU_MERGE_CHAIN", str(mode))
            monkeypatch.setenv("EMU_MERGE_LMAX", str(lmax))
            for c in (5, 9):
                out, _ = emu.msm(BW, sc, pts, c=c, K=K)
                assert _aff(out) == expect, (len(ks), mode, lmax, c)
            # the host-pointer form merges once per slice, the later slices into the stored sums
            out, _ = emu.msm_host(BW, sc, pts, chunks=3)
            assert _aff(out) == expect, (len(ks), mode, lmax, "slices")


def test_window_table_for_cached_bases():
    """MsmEngine::prepare_table: T[w][j] = 2^(c*w) * P_j by table_next_body, whose Affine::is_inf() shortcut never fires for this
    curve: a base (0, 1) goes through c doublings per row and stays (0, 1), a base (0, -1) doubles to (0, 1)."""
    n = 120
    pts, logs = _gen(801, n)
    ks = _scalars(802, n)
    ks[:len(BIG)] = BIG
    pts[5], logs[5] = _pts([bw.O])[0], 0        # a neutral base
    pts[9], logs[9], ks[9] = pts[8], logs[8], ks[8]   # the same pair twice: the shared bucket doubles
    pts[11], logs[11], ks[11] = _pts([bw.neg(_point(pts, 10))])[0], -logs[10], ks[10]   # P and -P: the shared bucket cancels
    expect = _by_logs(ks, logs)
    for c, K in ((0, 0), (3, 4), (5, 8), (11, 4)):
        out, cu = emu.msm_table(BW, _big(ks), pts, c=c, K=K)
        assert cu == c or c == 0
        assert cu > 0
        assert _aff(out) == expect, (c, cu)
    for c, chunks in ((0, 1), (5, 2), (6, 3), (-1, 1), (-1, 3)):
        out, cu = emu.msm_table(BW, _big(ks), pts, c=c, K=4, chunks=chunks)
        assert _aff(out) == expect, (c, chunks)
        assert (cu == 0) == (c < 0)
    # (0, -1) in the table, with odd and even scalars: its first row is (0, -1), every other row (0, 1)
    tpts, tks = pts.copy(), list(ks)
    tpts[20], tks[20] = _pts([bw.T2])[0], ks[20] | 1
    tpts[21], tks[21] = _pts([bw.T2])[0], ks[21] & ~1
    tl = list(logs)
    tl[20] = tl[21] = 0
    for c, K, chunks in ((0, 0, 0), (3, 4, 0), (11, 4, 0), (5, 4, 2), (-1, 4, 3)):
        out, _ = emu.msm_table(BW, _big(tks), tpts, c=c, K=K, chunks=chunks)
        assert _aff(out) == bw.add(_by_logs(tks, tl), bw.T2), (c, K, chunks)
    # a prefix of the cached bases (table rows stay ntab apart)
    m = n // 3
    expect = _by_logs(ks[:m], logs[:m])
    out, _ = emu.msm_table(BW, _big(ks[:m]), pts, c=6, K=4)
    assert _aff(out) == expect
    out, _ = emu.msm_table(BW, _big(ks[:m]), pts, c=6, K=4, chunks=2)
    assert _aff(out) == expect
    out, _ = emu.msm_table(BW, _big(ks[:1]), pts, c=11)
    assert _aff(out) == _by_logs(ks[:1], logs[:1])
    rng = random.Random(803)
    fr = [0, 1, bw.R - 1] + [rng.randrange(bw.R) for _ in range(n - 3)]
    out, _ = emu.msm_table(BW, _fr(fr), pts, coef_is_fr=True, c=7)
    assert _aff(out) == _by_logs(fr, logs)
    # all-zero scalars -> neutral
    out, _ = emu.msm_table(BW, np.zeros((n, 32), np.uint8), pts, c=4)
    assert _aff(out) == bw.O
    prj, _ = emu.msm_table(BW, np.zeros((n, 32), np.uint8), pts, c=4, out_kind=2)
    assert [bw.fp_from(bytes(prj[i:i + 32])) for i in (0, 32, 64)] == [0, 1, 1]


def test_horner_groups(monkeypatch):
    """The bit Horner cut into groups of 1, 2, 3, 7 bits or a single group per window (the legacy host_window_sums spellings
    included): the same element whatever the group size."""
    n = 400
    pts, logs = _gen(901, n)
    ks = _scalars(902, n)
    ks[:len(BIG)] = BIG
    expect = _by_logs(ks, logs)
    sc = _big(ks)
    for c in (2, 4, 9, 10, 11, 12, 14):
        for hb in (0, 1, 2, 3, 7, 30):
            monkeypatch.setenv("EMU_HORNER_BITS", str(hb))
            out, plan = emu.msm(BW, sc, pts, c=c, K=8)
            assert _aff(out) == expect, (c, hb)
    monkeypatch.delenv("EMU_HORNER_BITS")
    for hws in (1, 2):
        monkeypatch.setenv("EMU_HOST_WINDOW_SUMS", str(hws))
        out, _ = emu.msm(BW, sc, pts, c=11, K=8)
        assert _aff(out) == expect, hws


def test_sum_reduce():
    """MsmEngine::sum_reduce (the plain sum of affine points: the host sum of a sharded MSM has the same cases)"""
    P = bw.mul(0x1234567890abcdef, bw.G)
    pts, logs = _gen(931, 200)
    gen = [_point(pts, j) for j in range(200)]
    cases = [[], [bw.O], [bw.T2], [P], [P, bw.neg(P)], [P, P], [bw.T2, bw.T2], [P, bw.T2], [bw.G, P, bw.T2, bw.O, bw.neg(bw.G)],
             [P, bw.neg(P)] + gen[:3], gen[:7] + [bw.O, bw.T2, P, bw.neg(P)] + gen[7:70], [bw.O] * 9, [bw.T2] * 9,
             gen + [bw.T2, bw.O] + [bw.neg(q) for q in gen[:199]]]
    for pl in cases:
        expect = bw.O
        for q in pl:
            expect = bw.add(expect, q)
        arr = _pts(pl) if pl else np.zeros((0, 64), np.uint8)
        for K in (0, 1, 4, 64):
            assert _aff(emu.sum_reduce(BW, arr, K=K)) == expect, (len(pl), K)
            prj = emu.sum_reduce(BW, arr, out_kind=2, K=K)
            assert bw.fp_from(bytes(prj[64:96])) == 1 and bw.aff_from(bytes(prj[:64])) == expect, (len(pl), K)


def test_tickets_finished_out_of_order():
    n = 90
    pts, logs = _gen(911, n)
    ks = _scalars(912, n)
    expect = _by_logs(ks, logs)
    out, refused = emu.msm_slots(BW, _big(ks), pts)
    assert refused == 0
    for i in range(3):
        assert _aff(out[i]) == expect, i
