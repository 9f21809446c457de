"""Sparse batched Verkle updates without a GPU: the update bodies of csrc/verkle_bodies.h (lane sum, the store that adds the old
commitment, the parent's delta) compiled for the CPU (tests/verkle_harness.cpp) and run the way k_vk_update runs them -- four rows to a
workgroup, the lanes of a row's wave one by one, the kernel's tree through the wave's own slots, the finish, the delta -- against the
Python-integer oracle, and the wiring of ctt_hip_verkle_update_batch and VerkleCrs.update on a box without a device.

Expected values are exact curve points (tests/_banderwagon.py): scalars are taken mod 2r on bases that carry the point of order two,
mod r on points of the prime subgroup."""
import ctypes
import random
import struct

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests._verkle import build_harness, fr_from, layout, map_fr, prj_bytes as _prj, ser_bytes

TOP = (1 << 253) - 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("verkle_update"))


def _update(harness, pts, rows, c, bases=None, fr=False):
    """rows: [[(index, delta), ...], ...]; bases: None or m (X, Y, Z)-byte strings.  -> per row (prj, ser, fr, dfr) bytes"""
    enc = bw.fr_bytes if fr else bw.big_bytes
    m = len(rows)
    row_ptr = [0]
    for row in rows:
        row_ptr.append(row_ptr[-1] + len(row))
    E = row_ptr[-1]
    data = struct.pack("<6I", len(pts), c, 1 if fr else 0, m, 1 if bases is not None else 0, E)
    data += b"".join(bw.aff_bytes(p) for p in pts) + struct.pack(f"<{m + 1}I", *row_ptr)
    data += bytes(i for row in rows for i, _ in row) + b"".join(enc(d) for row in rows for _, d in row)
    if bases is not None:
        data += b"".join(bases)
    out = harness("update", data)
    assert len(out) == 192 * m
    prj, ser, rfr, dfr = out[:96 * m], out[96 * m:128 * m], out[128 * m:160 * m], out[160 * m:]
    return [(prj[96 * i:96 * i + 96], ser[32 * i:32 * i + 32], rfr[32 * i:32 * i + 32], dfr[32 * i:32 * i + 32]) for i in range(m)]


def _expect(pts, row, base_pt=bw.O, mod=None):
    mod = mod or 2 * bw.R
    return bw.add(base_pt, bw.msm_fast([d % mod for _, d in row], [pts[i] for i, _ in row]))


def _check(got, pt, base_pt=bw.O):
    prj, ser, rfr, dfr = got
    assert bw.fp_from(prj[64:]) == 1 and bw.aff_from(prj[:64]) == pt
    assert ser == ser_bytes(pt)
    assert fr_from(rfr) == map_fr(pt)
    assert int.from_bytes(dfr, "little") < bw.R and fr_from(dfr) == (map_fr(pt) - map_fr(base_pt)) % bw.R


def _subgroup_points(rng, n):
    return [bw.msm_fast([rng.randrange(1, bw.R)], [bw.G]) for _ in range(n)]


# --- digits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 7, 10])
def test_digit_parity_one_entry_rows(harness, c):
    rng = random.Random(200 + c)
    pts = _subgroup_points(rng, 4) + [bw.T2]
    scalars = [0, 1, bw.R - 1, bw.R, bw.R + 1, TOP, int.from_bytes(b"\x80" * 32, "little") & TOP, rng.randrange(1 << 253)]
    rows = [[(i, k)] for k in scalars for i in (rng.randrange(4), 4)]
    got = _update(harness, pts, rows, c)
    for g, row in zip(got, rows):
        _check(g, bw.msm_fast([row[0][1] % (2 * bw.R)], [pts[row[0][0]]]))
    frrows = [[(i, k % bw.R)] for row in rows for i, k in row]
    got = _update(harness, pts, frrows, c, fr=True)
    for g, row in zip(got, frrows):
        _check(g, bw.msm_fast([row[0][1]], [pts[row[0][0]]]))


# --- the split of a row's items over the lanes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cnts", [(10, [0, 1, 2, 3, 63, 64, 65]), (7, [0, 1, 2, 7, 12]), (2, [0, 1, 2, 3])])
@pytest.mark.parametrize("fr", [False, True])
def test_item_split(harness, c, cnts, fr):
    """cnt * W below, on and above multiples of the group (W = 26 at c = 10; 37 at 7; 127 at 2, wider than the group)"""
    W = len(layout(c))
    assert W == {10: 26, 7: 37, 2: 127}[c]
    rng = random.Random(300 + c)
    pts = _subgroup_points(rng, 6)
    rows = [[(rng.randrange(6), rng.randrange(bw.R)) for _ in range(cnt)] for cnt in cnts]
    bases = [bw.O if j % 2 else bw.mul(j + 5, bw.G) for j in range(len(rows))]
    got = _update(harness, pts, rows, c, bases=[_prj(b, rng.randrange(1, bw.P)) for b in bases], fr=fr)
    for g, row, b in zip(got, rows, bases):
        _check(g, _expect(pts, row, b, bw.R), b)
    # the rows are independent of their neighbours: the same rows in reverse order, without bases
    got = _update(harness, pts, rows[::-1], c, fr=fr)
    for g, row in zip(got, rows[::-1]):
        _check(g, _expect(pts, row, mod=bw.R))
    assert got[-1][0] == _prj(bw.O) and got[-1][1] == bytes(32) and got[-1][3] == bytes(32)     # the empty row: (0 : 1 : 1 : 0)


def test_duplicates_and_cancellation(harness):
    rng = random.Random(41)
    pts = _subgroup_points(rng, 3)
    d1, d2, d3 = (rng.randrange(1, bw.R) for _ in range(3))
    base = bw.mul(77, bw.G)
    rows = [[(1, d1), (1, d2)], [(2, d1), (0, d3), (2, d2), (2, d1)], [(1, d1), (1, bw.R - d1)], [(0, d2), (2, d3), (0, bw.R - d2), (2, bw.R - d3)]]
    for fr in (False, True):
        got = _update(harness, pts, rows, 10, bases=[_prj(base, 3)] * 4, fr=fr)
        _check(got[0], bw.add(base, bw.mul((d1 + d2) % bw.R, pts[1])), base)
        _check(got[1], bw.add(base, bw.add(bw.mul((2 * d1 + d2) % bw.R, pts[2]), bw.mul(d3, pts[0]))), base)
        for g in got[2:]:
            _check(g, base, base)
            assert g[3] == bytes(32)                        # R = base: the parent's delta is 0


def test_bases(harness):
    rng = random.Random(42)
    pts = _subgroup_points(rng, 4)
    row = [(0, rng.randrange(bw.R)), (3, rng.randrange(bw.R)), (1, 5)]
    total = _expect(pts, row, mod=bw.R)
    Q = bw.mul(rng.randrange(1, bw.R), bw.G)
    z = rng.randrange(2, bw.P)
    cases = [(bw.O, _prj(bw.O)), (bw.O, _prj(bw.O, z)), (Q, _prj(Q, z)), (bw.add(Q, bw.T2), _prj(bw.add(Q, bw.T2), z)),
             (bw.neg(total), _prj(bw.neg(total), z)), (Q, _prj(Q))]
    assert bw.add(Q, bw.T2) == ((-Q[0]) % bw.P, (-Q[1]) % bw.P)
    got = _update(harness, pts, [row] * len(cases), 10, bases=[b for _, b in cases])
    for g, (bp, _) in zip(got, cases):
        _check(g, bw.add(bp, total), bp)
    assert got[4][0] == _prj(bw.O) and got[4][1] == bytes(32)                      # base = -(sum): the neutral
    assert fr_from(got[4][3]) == (-map_fr(bw.neg(total))) % bw.R
    # no bases at all: the neutral, whose map is 0 -- and empty rows with bases: the bases normalised and mapped
    got = _update(harness, pts, [row, []], 10)
    _check(got[0], total)
    assert got[0][3] == got[0][2] and got[1][0] == _prj(bw.O)
    got = _update(harness, pts, [[], []], 10, bases=[_prj(Q, z), _prj(bw.O, z)])
    _check(got[0], Q, Q)
    _check(got[1], bw.O, bw.O)


def test_update_means_what_the_dense_commitment_means(harness):
    rng = random.Random(43)
    pts = _subgroup_points(rng, 16)
    old = [rng.randrange(bw.R) for _ in range(16)]
    new = list(old)
    changed = [2, 3, 11, 15]
    for i in changed:
        new[i] = rng.randrange(bw.R)
    new[11] = 0
    c_old, c_new = bw.msm_fast(old, pts), bw.msm_fast(new, pts)
    row = [(i, (new[i] - old[i]) % bw.R) for i in changed]
    for fr in (False, True):
        got = _update(harness, pts, [row], 10, bases=[_prj(c_old, rng.randrange(1, bw.P))], fr=fr)
        assert got[0][0] == _prj(c_new)
        _check(got[0], c_new, c_old)


# --- ABI wiring ---------------------------------------------------------------------------------------------------------------------
def test_update_symbol_is_exported_and_the_abi_version_stays():
    from constantine_amd import _lib
    L = _lib.lib()
    assert "ctt_hip_verkle_update_batch" in _lib.exported_symbols() and hasattr(L, "ctt_hip_verkle_update_batch")
    assert L.ctt_hip_msm_abi_version() == _lib.ABI_VERSION == 11


def test_without_a_device_the_update_refuses():
    from constantine_amd import _lib
    L = _lib.lib()
    if L.ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    vp = ctypes.c_void_p
    outs = [np.full(n, 0xAB, np.uint8) for n in (96, 32, 32, 32)]
    o = [a.ctypes.data_as(vp) for a in outs]
    row_ptr, idx, deltas = np.array([0, 1], np.uint32), np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8)
    L.ctt_hip_clear_last_error()
    assert L.ctt_hip_verkle_update_batch(None, None, 0, o[0], o[1], o[2], o[3], None, row_ptr.ctypes.data_as(vp), idx.ctypes.data_as(vp),
                                         deltas.ctypes.data_as(vp), 1, 0) == -1
    assert L.ctt_hip_last_error() == -3
    assert all(bytes(a) == bytes([0xAB]) * len(a) for a in outs)


def test_python_argument_errors_come_before_any_call(monkeypatch):
    from constantine_amd import _lib, verkle

    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded for a call that must be refused in Python")
    monkeypatch.setattr(_lib, "lib", no_gpu)
    crs = verkle.VerkleCrs.__new__(verkle.VerkleCrs)
    crs.n, crs.handle = 4, 1
    crs.L = crs.ctx = None
    d = np.zeros((3, 32), np.uint8)
    bad = [dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 2, 1, 3]),                     # not monotone
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 1, 2]),                        # row_ptr[-1] != E
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[1, 3]),                           # does not start at 0
           dict(deltas=d, idx=[0, 256, 2], row_ptr=[0, 3]),                         # an index outside [0, n)
           dict(deltas=d, idx=[0, 4, 2], row_ptr=[0, 3]),
           dict(deltas=d, idx=[0, -1, 2], row_ptr=[0, 3]),
           dict(deltas=d, idx=[0, 1], row_ptr=[0, 3]),                              # one index per entry
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 3], want=()),
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 3], want=("prj", "aff")),
           dict(deltas=np.zeros((3, 31), np.uint8), idx=[0, 1, 2], row_ptr=[0, 3]),  # trailing shapes
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 3], base=np.zeros((1, 64), np.uint8)),
           dict(deltas=d, idx=[0, 1, 2], row_ptr=[0, 3], base=np.zeros((2, 96), np.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            crs.update(**kw)

    class FakeCuda:                                                                # a base of another kind than the deltas
        is_cuda = True

        def data_ptr(self):
            return 0
    with pytest.raises(ValueError):
        crs.update(d, [0, 1, 2], [0, 3], base=FakeCuda())


def test_python_update_without_a_device():
    from constantine_amd import _lib, verkle
    L = _lib.lib()
    if L.ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    crs = verkle.VerkleCrs.__new__(verkle.VerkleCrs)
    crs.n, crs.handle, crs.L, crs.ctx = 4, 1, L, None
    with pytest.raises(_lib.GpuUnavailable):
        crs.update(np.zeros((1, 32), np.uint8), [0], [0, 1], want=("dfr",))
    crs.handle = None
