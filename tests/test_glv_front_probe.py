"""The front kernel of the endomorphism split alone (csrc/hip_backend.h k_glv_front behind HipBackend::launch_glv_front: the scalar split,
beta * x, the signs in y, two record arrays staged through a swizzled LDS image, the half scalars), through ctt_hip_glv_front_probe, and
its CPU twin (tests/emu/glv_emu.cpp emu_glv_front: msm_bodies.h glv_front_body per pair) under ONE checker.

First half, no GPU: the Python restatement of the split (tests/_glvref.py) against the congruence and the bounds, the shape of the scalar
set from that restatement alone, the CPU twin through the checker, and the refusal of the probe without a device.  Second half, `gpu`:
the same inputs through the probe and the same checker, and every refusal.  Every comparison is integer equality against Python integers
and oracle/pyoracle.py; no elliptic-curve or split code is shared with what is tested.

Sizes: CONVERT_BLOCK = 128 pairs per workgroup and 8 chunks of 16 bytes per record, so n = 1 (one lane), 127, 128, 129 (a block one
short, exact, one over), 257 (two blocks and a lane) and 1000 (eight blocks, the last ragged) put every rec & 7 of the swizzle into both
halves of the image and the staged read-out at the edge of a block.

Correction steps: the body allows two; its estimate q' of Q = k / x^2 is short by less than 2^126 / x^2 (0.3716) + frac(2^254 / x^2) *
floor(k / 2^126) / 2^128 (0.5033 * 0.9057 = 0.4558 for k <= (r - 1) / 2) + 1 (the floor) < 1.83, so floor(Q) - q' is 0 or 1: NO scalar
takes the second step (none among 10^7 directed candidates either -- the largest k / 2^126 with all lower bits set).  The set below holds
scalars of 0 and of 1 step.

Per pair j the checker asserts: half[j] == k1 and half[n + j] == k2 of the restatement; k1, k2 <= x^2 / 2 on their own; both records'
limbs normalised and the stored integers below 2p (tests/test_ec_probe.py Law.dec, R' = 2^392); record j decodes to (P.x, s1 P.y),
record n + j to (b P.x, s2 P.y) with s1, s2 = +-1 read off the records and ONE b for all pairs, b^3 == 1, b != 1;
k == s1 k1 + s2 k2 mu (mod r) with those signs; (b P.x, P.y) == [mu]P by the oracle's scalar_mul for the first 32 non-neutral pairs (which
cube root); the flag word 1 exactly for a neutral input, in both records, whose coordinates are raw zeros; 64 guard words behind each
output untouched.  The bytes behind the flag word are not asserted (the body does not write them).
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import _glvref as gr
from tests import _sortref as sr
from tests.emu import emu
from tests.test_ec_probe import Law
from tests.test_glv_split import EDGE, glv_lib

NAME = "bls12_381_g1"
CURVE = po.CURVES[NAME]
LAW = Law(NAME)
P = LAW.p
SIZES = (1, 127, 128, 129, 257, 1000)
BLOCK = 128                            # hip_backend.h CONVERT_BLOCK
STRIDE, FLAG_OFF = 128, 112            # msm_bodies.h gather_stride<FD>(), gather_flag_offset<FD>() of BLS12-381 G1 (the CPU leg holds them against the code)
NL = LAW.nl                            # 14 limbs of 28 bits per coordinate
FILL_WORD = sr.FILL * 0x01010101
MU_CHECKED = 32
NEUTRAL_FIRST = 5                      # a neutral input in the first block, and one at the last index


# --- inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all_points():
    """1000 distinct synthetic points: (C-API bytes, oracle tuples)"""
    arr = cref.gen_points(NAME, 7301, max(SIZES))
    return arr, [CURVE.aff_from_bytes(bytes(row)) for row in arr]


def _specials():
    rng = random.Random(0x71E5)
    qs = [0, 1, rng.randrange(gr.X2 // 2 - 1), gr.X2 // 2 - 2]
    return EDGE + gr.ties(qs) + [po.synth_scalar(7302, 0, 120)]


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(scalars as integers, points as C-API bytes, points as oracle tuples / None) of n pairs"""
    arr, pts = _all_points()
    arr, pts = arr[:n].copy(), list(pts[:n])
    rng = random.Random(0x5EED00 + n)
    ks = [rng.getrandbits(255) for _ in range(n)]
    if n >= BLOCK - 1:
        sp = _specials()
        ks[:len(sp)] = sp
        ks[n - 1 - len(EDGE):n - 1] = EDGE               # the ragged end of the last block holds the edges as well
        for j in (NEUTRAL_FIRST, n - 1):
            arr[j] = 0
            pts[j] = None
    return ks, arr, pts


@functools.lru_cache(maxsize=None)
def _mu_point(j):
    return CURVE.scalar_mul(gr.MU, _all_points()[1][j])


def _buffers(n):
    """(records, half) with their guards, pre-filled as tests/_sortref.py fills the sort's outputs"""
    return (np.full(2 * n * STRIDE + 4 * sr.GUARD, sr.FILL, dtype=np.uint8), np.full(2 * n * 4 + sr.GUARD, FILL_WORD, dtype=np.uint32))


def _words(ks):
    return sr.to_words(ks)


# --- the checker -----------------------------------------------------------------------------------------------------------------------
def check(n, ks, pts, rec, half):
    assert len(rec) == 2 * n * STRIDE + 4 * sr.GUARD and len(half) == 2 * n * 4 + sr.GUARD
    assert (rec[2 * n * STRIDE:] == sr.FILL).all(), "guard behind the records"
    assert (half[2 * n * 4:] == FILL_WORD).all(), "guard behind the half scalars"
    recw = np.ascontiguousarray(rec[:2 * n * STRIDE]).view(np.uint32).reshape(2 * n, STRIDE // 4)
    hw = half[:2 * n * 4].reshape(2 * n, 4)
    flag = FLAG_OFF // 4
    roots, seen_mu = set(), 0
    for j in range(n):
        k, pt = ks[j], pts[j]
        at = f"pair {j} of {n}, k = {k:#x}"
        want = gr.split(k)
        k1 = sum(int(w) << (32 * i) for i, w in enumerate(hw[j]))
        k2 = sum(int(w) << (32 * i) for i, w in enumerate(hw[n + j]))
        assert (k1, k2) == (want.k1, want.k2), f"{at}: halves {k1:#x}, {k2:#x}; {want.k1:#x}, {want.k2:#x} expected"
        assert 2 * k1 <= gr.X2 and 2 * k2 <= gr.X2, f"{at}: a half above x^2 / 2"
        r1, r2 = recw[j], recw[n + j]
        assert int(r1[flag]) == int(r2[flag]) == (1 if pt is None else 0), f"{at}: flag words {r1[flag]}, {r2[flag]}"
        if pt is None:
            assert not r1[:2 * NL].any() and not r2[:2 * NL].any(), f"{at}: a neutral input with coordinates that are not raw zeros"
            continue
        xs, signs = [], []
        for name, r in (("j", r1), ("n + j", r2)):
            try:
                x, rawx = LAW.dec(r[:NL])
                y, rawy = LAW.dec(r[NL:2 * NL])
            except AssertionError as err:
                raise AssertionError(f"{at}, record {name}: {err}") from None
            assert rawx[0] < 2 * P and rawy[0] < 2 * P, f"{at}, record {name}: a stored integer of 2p or more"
            assert y in (pt[1], P - pt[1]), f"{at}, record {name}: y is neither P.y nor -P.y"
            xs.append(x)
            signs.append(1 if y == pt[1] else -1)
        assert xs[0] == pt[0], f"{at}: record j does not hold P.x"
        assert (signs[0] * k1 + signs[1] * k2 * gr.MU - k) % gr.R == 0, f"{at}: k != s1 k1 + s2 k2 mu with the signs of the records {signs}"
        assert (signs[0], signs[1]) == (want.s1, want.s2), f"{at}: signs {signs}, {(want.s1, want.s2)} expected"
        roots.add(xs[1] * pow(pt[0], -1, P) % P)
        if seen_mu < MU_CHECKED:
            assert (xs[1], pt[1]) == _mu_point(j), f"{at}: (x of record n + j, P.y) is not [mu]P"
            seen_mu += 1
    assert len(roots) == 1, f"x of record n + j is not ONE multiple of P.x: {len(roots)} ratios"
    b = roots.pop()
    assert pow(b, 3, P) == 1 and b != 1
    assert seen_mu == min(MU_CHECKED, sum(pt is not None for pt in pts))


# --- CPU ---------------------------------------------------------------------------------------------------------------------------------
def _emu_front(n, ks, arr):
    L = glv_lib()
    L.emu_glv_front.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rec, half = _buffers(n)
    words = _words(ks)
    shape = np.zeros(4, dtype=np.uint32)
    assert L.emu_glv_front(emu._p(words), emu._p(arr), n, emu._p(rec), emu._p(half), emu._p(shape)) == 0
    return rec, half, [int(x) for x in shape]


def test_restatement_of_the_split_vs_python_integers():
    """tests/_glvref.py split() on its own: the congruence, the bounds the body's comment proves, ties below, at most one correction"""
    rng = random.Random(0x61F6)
    ks = _specials() + [rng.getrandbits(255) for _ in range(20000)] + [rng.randrange(gr.R // 2) for _ in range(20000)]
    for k in ks:
        s = gr.split(k)
        assert (s.s1 * s.k1 + s.s2 * s.k2 * gr.MU - k) % gr.R == 0, hex(k)
        assert 2 * s.k1 <= gr.X2 and 2 * s.k2 <= gr.X2 and s.steps <= 1, hex(k)
        assert s.fold == ((k % gr.R) > (gr.R - 1) // 2), hex(k)
    assert gr.R == CURVE.order and (gr.MU * gr.MU + gr.MU + 1) % gr.R == 0 and gr.M == 0x5f1afb3c7807eab758fdb948bdb3fb8b
    for t in gr.ties([0, 7])[0::4]:
        assert gr.split(t).k1 == gr.X2 // 2 and not gr.split(t).up and gr.split(t + 1).up and gr.split(t + 1).k1 == gr.X2 // 2 - 1


@pytest.mark.parametrize("n", [s for s in SIZES if s > 1])
def test_shape_of_the_inputs(n):
    """from the restatement alone: the set holds scalars with and without the fold, with and without the round-up, of 0 and of 1
    correction step, ties on both sides of the fold, a zero second half; the points are distinct, two of them neutral"""
    ks, arr, pts = _inputs(n)
    sp = [gr.split(k) for k in ks]
    for fold in (False, True):
        assert any(s.fold == fold and s.up for s in sp) and any(s.fold == fold and not s.up for s in sp)
        assert any(s.fold == fold and s.steps == 0 for s in sp) and any(s.fold == fold and s.steps == 1 for s in sp)
        assert any(s.fold == fold and 2 * s.k1 == gr.X2 and not s.up for s in sp)                      # a tie, not rounded up
        assert any(s.fold == fold and 2 * s.k1 == gr.X2 - 2 and s.up for s in sp)                      # its successor, rounded up
    assert all(s.steps <= 1 for s in sp)
    assert any(s.k2 == 0 and s.k1 > 1 for s in sp) and any(s.k1 == 0 for s in sp)
    assert all(k in ks[:64] for k in EDGE) and all(k in ks[n - 1 - len(EDGE):] for k in EDGE) and max(ks) < 1 << 255
    live = [pt for pt in pts if pt is not None]
    assert len(set(live)) == len(live) == n - 2 and pts[NEUTRAL_FIRST] is None and pts[n - 1] is None and NEUTRAL_FIRST < BLOCK
    assert not arr[NEUTRAL_FIRST].any() and not arr[n - 1].any()
    assert {j & 7 for j in range(min(n, BLOCK))} == set(range(8)) and STRIDE // 16 == 8
    assert [(s - 1) // BLOCK + 1 for s in SIZES] == [1, 1, 1, 2, 3, 8] and [s % BLOCK for s in SIZES] == [1, 127, 0, 1, 1, 104]


@pytest.mark.parametrize("n", SIZES)
def test_front_body_on_the_cpu(n):
    ks, arr, pts = _inputs(n)
    rec, half, shape = _emu_front(n, ks, arr)
    assert shape == [STRIDE, FLAG_OFF, NL, LAW.lb]
    check(n, ks, pts, rec, half)


def test_probe_symbol_is_exported_and_the_abi_version_stays():
    from constantine_amd import _lib
    L = _lib.lib()
    assert "ctt_hip_glv_front_probe" in _lib.exported_symbols() and hasattr(L, "ctt_hip_glv_front_probe")
    assert L.ctt_hip_msm_abi_version() == _lib.ABI_VERSION == 11


def test_without_a_device_the_probe_refuses():
    from constantine_amd import _lib
    L = _lib.lib()
    if L.ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    vp = ctypes.c_void_p
    bufs = [np.full(n, 0xAB, np.uint8) for n in (32, 96, 2 * STRIDE, 32)]
    p = [a.ctypes.data_as(vp) for a in bufs]
    L.ctt_hip_clear_last_error()
    assert L.ctt_hip_glv_front_probe(None, 0, p[0], p[1], 1, p[2], p[3]) == -1
    assert L.ctt_hip_last_error() == -3
    assert all(bytes(a) == bytes([0xAB]) * len(a) for a in bufs)


# --- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


def _device_buffers(torch, n):
    rec, half = _buffers(n)
    return torch.from_numpy(rec).cuda(), torch.from_numpy(half.view(np.int32)).cuda()


def _back(torch, d_rec, d_half):
    torch.cuda.synchronize()
    return d_rec.cpu().numpy(), d_half.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_probe_gpu(n, dev):
    import torch
    ks, arr, pts = _inputs(n)
    d_sc = torch.from_numpy(_words(ks).view(np.int32)).cuda()
    d_pts = torch.from_numpy(arr).cuda()
    d_rec, d_half = _device_buffers(torch, n)
    assert dev.glv_front_probe(NAME, d_sc, d_pts, n, d_rec[:2 * n * STRIDE], d_half[:2 * n * 4])
    rec, half = _back(torch, d_rec, d_half)
    check(n, ks, pts, rec, half)


@pytest.mark.gpu
def test_front_probe_refusals_gpu(dev):
    """a curve without a split, n = 0 and every NULL pointer: -1, the last error set, both outputs at their fill; then the same call with
    legal values goes through"""
    import torch
    from constantine_amd import _lib
    from constantine_amd.curves import CURVES
    L = _lib.lib()
    n = 129
    ks, arr, pts = _inputs(n)
    d_sc = torch.from_numpy(_words(ks).view(np.int32)).cuda()
    d_pts = torch.from_numpy(arr).cuda()
    d_rec, d_half = _device_buffers(torch, n)
    keep = _buffers(n)

    def untouched():
        rec, half = _back(torch, d_rec, d_half)
        return (rec == keep[0]).all() and (half == keep[1]).all()

    ok = [d_sc, d_pts, n, d_rec, d_half]
    cases = [(name, ok) for name in CURVES if name != NAME] + [(NAME, [d_sc, d_pts, 0, d_rec, d_half])]
    cases += [(NAME, [None if i == q else a for i, a in enumerate(ok)]) for q in (0, 1, 3, 4)]
    for name, args in cases:
        L.ctt_hip_clear_last_error()
        assert not dev.glv_front_probe(name, *args), (name, args[2])
        assert L.ctt_hip_last_error() != 0 and L.ctt_hip_last_error_message(), (name, args[2])
        assert untouched(), (name, args[2])
    assert len(cases) >= 6 + 4
    assert dev.glv_front_probe(NAME, *ok)
    check(n, ks, pts, *_back(torch, d_rec, d_half))
