"""Sparse batched Verkle updates without a GPU: the update bodies of csrc/verkle_bodies.h (lane sum, the store that adds the old
commitment, the parent's delta) compiled for the CPU and run the way k_vk_update runs them -- the lanes of a row's group one by one,
the kernel's tree, the finish, the delta -- against the Python-integer oracle, and the wiring of ctt_hip_verkle_update_batch and
VerkleCrs.update on a box without a device.

Expected values are exact curve points (tests/_banderwagon.py): scalars are taken mod 2r on bases that carry the point of order two,
mod r on points of the prime subgroup."""
import ctypes
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests._verkle import fr_from, layout, map_fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "constantine_amd")
TOP = (1 << 253) - 1
G_LANES = 64          # the kernel's group: one wavefront per row

HARNESS = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "verkle_bodies.h"
using namespace ctt;
using F = Banderwagon::F;
using Fr = Banderwagon::Fr;
template <class T> static bool rd(T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, stdin) == n; }
static void wr(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }
// every body is instantiated once (they inline all of the field arithmetic)
static __attribute__((noinline)) XYZZ<F> lane_sum(const VkUpdateArgs& a, uint32_t k, uint32_t l, uint32_t G) { return vk_update_lane_sum<F, Fr>(a, k, l, G); }
static __attribute__((noinline)) void finish(const VkFinishArgs& f, uint32_t lanes) {
  for (uint32_t lane = 0; lane < lanes; lane++) vk_finish_body<F, Fr>(f, lane);
}
// in: n, c, fr, m, has_base, G, E, n points, row_ptr[m + 1], idx[E] (bytes), deltas[E][8], base[m][24] if has_base
// out: prj m x 96, ser m x 32, fr m x 32, dfr m x 32
int main() {
  uint32_t n, c, fr, m, has_base, G, E;
  if (!rd(&n, 1) || !rd(&c, 1) || !rd(&fr, 1) || !rd(&m, 1) || !rd(&has_base, 1) || !rd(&G, 1) || !rd(&E, 1)) return 1;
  std::vector<uint32_t> pts(n * 16), row_ptr(m + 1), deltas((size_t)E * 8 + 1), base((size_t)m * 24 + 1);
  std::vector<uint8_t> idx(E + 1);
  if (!rd(pts.data(), n * 16) || !rd(row_ptr.data(), m + 1) || !rd(idx.data(), E) || !rd(deltas.data(), (size_t)E * 8)) return 1;
  if (has_base && !rd(base.data(), (size_t)m * 24)) return 1;
  VkTableArgs t;
  int W;
  t.lay = window_layout(Banderwagon::BITS, (int)c, &W);
  t.n = n; t.W = (uint32_t)W; t.rows = vk_row_off(t.lay, t.W); t.stride = VK_REC_WORDS;
  std::vector<uint32_t> tab((size_t)n * t.rows * t.stride), pre((size_t)n * t.rows * 8);
  t.pts = pts.data(); t.tab = tab.data(); t.pre = pre.data();
  for (uint32_t lane = 0; lane < n * t.W; lane++) vk_table_body<F>(t, lane);
  std::vector<uint32_t> ext((size_t)m * VK_EXT_WORDS, 0x5A5A5A5Au);
  VkUpdateArgs a{tab.data(), n, t.W, t.lay, t.rows, t.stride, row_ptr.data(), idx.data(), deltas.data(), (int)fr,
                 has_base ? base.data() : nullptr, m, ext.data()};
  for (uint32_t k = 0; k < m; k++) {
    std::vector<XYZZ<F>> lanes(G);
    for (uint32_t l = 0; l < G; l++) lanes[l] = lane_sum(a, k, l, G);
    for (uint32_t s = G >> 1; s >= 1; s >>= 1)      // the kernel's tree: the upper half of the live lanes hands over to the lower half
      for (uint32_t l = 0; l < s; l++) lanes[l] = ed_add<F>(lanes[l], lanes[l + s]);
    vk_update_store<F>(a, k, lanes[0]);
  }
  for (uint32_t l = 0; l < G; l++)                  // a wave without a row holds neutrals (and reads nothing)
    if (!lane_sum(a, m, l, G).is_inf() || !lane_sum(a, m + 3, l, G).is_inf()) return 3;
  std::vector<uint32_t> prj((size_t)m * 24), ser((size_t)m * 8), rfr((size_t)m * 8), bfr((size_t)m * 8), dfr((size_t)m * 8, 0x5A5A5A5Au);
  const uint32_t K = VK_FINISH_CHUNK, fl = (m + K - 1) / K + 2;
  VkFinishArgs f{ext.data(), VK_EXT_WORDS, m, K, prj.data(), ser.data(), rfr.data()};
  finish(f, fl);
  if (has_base) {
    VkFinishArgs fb{base.data(), 24u, m, K, nullptr, nullptr, bfr.data()};
    finish(fb, fl);
  }
  VkDeltaArgs d{rfr.data(), has_base ? bfr.data() : nullptr, m, dfr.data()};
  for (uint32_t lane = 0; lane < m + 2; lane++) vk_delta_body<Fr>(d, lane);
  wr(prj.data(), prj.size() * 4); wr(ser.data(), ser.size() * 4); wr(rfr.data(), rfr.size() * 4); wr(dfr.data(), dfr.size() * 4);
  return 0;
}
'''


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("verkle_update")
    cxx = shutil.which("g++") or shutil.which("c++")
    (d / "vku.cpp").write_text(HARNESS)
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(PKG, "csrc"), str(d / "vku.cpp"), "-o", str(d / "vku")], check=True)

    def run(data):
        return subprocess.run([str(d / "vku")], input=data, check=True, capture_output=True).stdout
    return run


def _prj(pt, z=1):
    """(X, Y, Z) bytes of the affine point scaled by z"""
    return bw.fp_bytes(pt[0] * z % bw.P) + bw.fp_bytes(pt[1] * z % bw.P) + bw.fp_bytes(z % bw.P)


def _update(harness, pts, rows, c, bases=None, fr=False, G=G_LANES):
    """rows: [[(index, delta), ...], ...]; bases: None or m (X, Y, Z)-byte strings.  -> per row (prj, ser, fr, dfr) bytes"""
    enc = bw.fr_bytes if fr else bw.big_bytes
    m = len(rows)
    row_ptr = [0]
    for row in rows:
        row_ptr.append(row_ptr[-1] + len(row))
    E = row_ptr[-1]
    data = struct.pack("<7I", len(pts), c, 1 if fr else 0, m, 1 if bases is not None else 0, G, E)
    data += b"".join(bw.aff_bytes(p) for p in pts) + struct.pack(f"<{m + 1}I", *row_ptr)
    data += bytes(i for row in rows for i, _ in row) + b"".join(enc(d) for row in rows for _, d in row)
    if bases is not None:
        data += b"".join(bases)
    out = harness(data)
    assert len(out) == 192 * m
    prj, ser, rfr, dfr = out[:96 * m], out[96 * m:128 * m], out[128 * m:160 * m], out[160 * m:]
    return [(prj[96 * i:96 * i + 96], ser[32 * i:32 * i + 32], rfr[32 * i:32 * i + 32], dfr[32 * i:32 * i + 32]) for i in range(m)]


def _expect(pts, row, base_pt=bw.O, mod=None):
    mod = mod or 2 * bw.R
    return bw.add(base_pt, bw.msm_fast([d % mod for _, d in row], [pts[i] for i, _ in row]))


def _check(got, pt, base_pt=bw.O):
    prj, ser, rfr, dfr = got
    assert bw.fp_from(prj[64:]) == 1 and bw.aff_from(prj[:64]) == pt
    x = pt[0] if pt[1] >= (bw.P - 1) // 2 else (-pt[0]) % bw.P
    assert ser == x.to_bytes(32, "big")
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
