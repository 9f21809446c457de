"""The pair walker of the sort's partition kernels (csrc/msm_bodies.h for_each_digit_pair) on the host, no GPU.

A thread of the pair forms (csrc/hip_backend.hip k_part_count<true>, k_part_scatter<false, true>, k_part_scatter_staged<false, true>) holds
PP_NS = 2 pairs of 4-word half scalars as k[NS][8] -- half A in words 0-3, half B in words 4-7.  The harness below, compiled from this
file around the header as tests/emu compiles its sources, walks pairs through for_each_digit_pair<2> (what the kernels instantiate) and
<1> and returns, beside the walker's digits, booth_digit_packed of each half zero-extended to 8 words.  Both are compared, by integer equality, with tests/_sortref.py digits() (Python integers behind a bit matrix).

Every c in 2 .. 20 over 127 bits (windows end at bit 128), whole walks and walks over [w0, w0 + nw).  Halves: 0, 1, 2^127 - 1, all ones
below every window boundary of the layout, the lone bit below and at it, pairs whose half A has its top bits set beside a half B of 0 and
the reverse (a carry or a bit leaking across words 3 / 4 would give the zero half a digit), and seeded values.  A ragged last group is
padded with zero pairs as load_pairs pads it: a padding pair must have no digits.
"""
import ctypes
import fcntl
import os
import random
import subprocess

import numpy as np
import pytest

from tests import _sortref as sr
from tests.emu import emu

BITS = 127
NONE = 0xFFFFFFFF

HARNESS = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "msm_bodies.h"
using namespace ctt;
template <int NS>
static int walk(const WinLayout& L, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t w0, uint32_t nw, uint32_t* out_a, uint32_t* out_b) {
  for (uint32_t jb = 0; jb < n; jb += NS) {
    uint32_t k[NS][8];
    for (uint32_t s = 0; s < (uint32_t)NS; s++)
      for (int q = 0; q < 4; q++) {
        k[s][q] = jb + s < n ? a[4ull * (jb + s) + q] : 0u;
        k[s][4 + q] = jb + s < n ? b[4ull * (jb + s) + q] : 0u;
      }
    uint32_t seen = 0;
    for_each_digit_pair<NS>(k, w0, nw, L, [&](uint32_t w, const uint32_t (&da)[NS], const uint32_t (&db)[NS]) {
      for (uint32_t s = 0; s < (uint32_t)NS; s++) {
        if (jb + s < n) {
          out_a[(size_t)(w - w0) * n + jb + s] = da[s];
          out_b[(size_t)(w - w0) * n + jb + s] = db[s];
        } else if (da[s] != DIGIT_NONE || db[s] != DIGIT_NONE) {
          abort();   // a padding pair has no digits
        }
      }
      seen++;
    });
    if (seen != nw) return -1;
  }
  return 0;
}
extern "C" int pw_walk(int ns, int c, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t w0, uint32_t nw, uint32_t* out_a, uint32_t* out_b) {
  int W;
  const WinLayout L = window_layout(127, c, &W);
  if (w0 + nw > (uint32_t)W) return -1;
  const int rc = ns == 1 ? walk<1>(L, a, b, n, w0, nw, out_a, out_b) : ns == 2 ? walk<2>(L, a, b, n, w0, nw, out_a, out_b) : -1;
  return rc ? rc : W;
}
// booth_digit_packed on the 4-word scalar, the upper four words zero: out[(w - w0) * n + j]
extern "C" int pw_plain(int c, const uint32_t* h, uint32_t n, uint32_t w0, uint32_t nw, uint32_t* out) {
  int W;
  const WinLayout L = window_layout(127, c, &W);
  if (w0 + nw > (uint32_t)W) return -1;
  for (uint32_t j = 0; j < n; j++) {
    uint32_t k[8] = {h[4ull * j], h[4ull * j + 1], h[4ull * j + 2], h[4ull * j + 3], 0u, 0u, 0u, 0u};
    for (uint32_t w = w0; w < w0 + nw; w++) out[(size_t)(w - w0) * n + j] = booth_digit_packed(k, (int)w, L);
  }
  return W;
}
"""

_lib = None


def harness():
    global _lib
    if _lib is None:
        bdir = os.path.join(emu.HERE, "build")
        os.makedirs(bdir, exist_ok=True)
        src, out = os.path.join(bdir, "pair_walk.cpp"), os.path.join(bdir, "libpair_walk.so")
        csrc = os.path.join(emu.ROOT, "constantine_amd", "csrc")
        deps = [__file__] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        with open(os.path.join(bdir, ".pair_walk.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
                with open(src, "w") as f:
                    f.write(HARNESS)
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, src, "-o", out + ".tmp"])
                os.replace(out + ".tmp", out)
        L = ctypes.CDLL(out)
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        L.pw_walk.argtypes = [i32, i32, vp, vp, u32, u32, u32, vp, vp]
        L.pw_plain.argtypes = [i32, vp, u32, u32, u32, vp]
        _lib = L
    return _lib


def _halves(c):
    """(A, B) lists of Python integers below 2^127: the directed pairs first, then seeded ones; an odd count (a ragged group of NS = 2)"""
    lay = sr.window_layout(BITS, c)
    top = (1 << BITS) - 1
    single = [0, 1, top, top - 1, 1 << 126, (1 << 126) - 1]
    for w in range(1, lay.W):
        off = lay.off(w)
        single += [(1 << off) - 1, 1 << (off - 1), 1 << off, ((1 << off) - 1) ^ 1]       # all ones below the boundary, the bit below it, the bit at it
    single = [k for k in single if k <= top]
    cw = lay.width(lay.W - 1)
    high = [top, ((1 << cw) - 1) << lay.off(lay.W - 1) >> 1, 0x7FFFFFFF << 96, 0x7FFFFFFF << 96 | 1 << 95, (1 << 127) - (1 << 96)]
    high = [k & top for k in high]
    a, b = [], []
    for k in single:          # every single value in both seats, beside 0 and beside itself
        a += [k, 0, k]
        b += [0, k, k]
    for k in high:            # top bits of one half beside a zero half, both ways
        a += [k, 0]
        b += [0, k]
    rng = random.Random(0x9A17 + c)
    for _ in range(150):
        a.append(rng.getrandbits(BITS))
        b.append(rng.getrandbits(BITS))
    if len(a) % 2 == 0:
        a.append(rng.getrandbits(BITS))
        b.append(0)
    return a, b


def _words4(ks):
    return np.ascontiguousarray(sr.to_words(ks)[:, :4])


def _want(ks, lay):
    val, neg = sr.digits(sr.to_words(ks), lay)
    return np.where(val > 0, ((val - 1) << 1) | neg, NONE).astype(np.uint32)


@pytest.mark.parametrize("c", range(2, 21))
def test_pair_walker_vs_plain_digits_and_python_integers(c):
    L = harness()
    lay = sr.window_layout(BITS, c)
    assert lay.off(lay.W - 1) + lay.width(lay.W - 1) == 128
    a, b = _halves(c)
    n = len(a)
    assert n % 2 == 1 and all(k < 1 << BITS for k in a + b)
    wa, wb = _words4(a), _words4(b)
    want_a, want_b = _want(a, lay), _want(b, lay)
    # Python integers, digit by digit, for the directed pairs (the bit matrix of _sortref.digits is held against them in test_sort_probe.py)
    for j in range(0, n, 7):
        for w in range(lay.W):
            for k, want in ((a[j], want_a), (b[j], want_b)):
                v, s = sr.booth_digit(k, w, lay)
                assert int(want[w, j]) == (((v - 1) << 1 | s) if v else NONE)
    # a zero half has no digit, whatever sits in the other seat
    assert (want_a[:, [j for j in range(n) if a[j] == 0]] == NONE).all() and (want_b[:, [j for j in range(n) if b[j] == 0]] == NONE).all()
    spans = {(0, lay.W), (1, lay.W - 1), (lay.W // 2, max(1, lay.W // 3)), (lay.W - 1, 1), (min(3, lay.W - 1), 1)}
    for w0, nw in spans:
        if nw < 1 or w0 + nw > lay.W:
            continue
        plain_a, plain_b = np.zeros((nw, n), np.uint32), np.zeros((nw, n), np.uint32)
        assert L.pw_plain(c, emu._p(wa), n, w0, nw, emu._p(plain_a)) == lay.W
        assert L.pw_plain(c, emu._p(wb), n, w0, nw, emu._p(plain_b)) == lay.W
        assert (plain_a == want_a[w0:w0 + nw]).all() and (plain_b == want_b[w0:w0 + nw]).all(), (c, w0, nw)
        for ns in (1, 2):
            got_a, got_b = np.full((nw, n), 0x5A5A5A5A, np.uint32), np.full((nw, n), 0x5A5A5A5A, np.uint32)
            assert L.pw_walk(ns, c, emu._p(wa), emu._p(wb), n, w0, nw, emu._p(got_a), emu._p(got_b)) == lay.W, (c, ns, w0, nw)
            assert (got_a == plain_a).all(), (c, ns, w0, nw, "half A", np.argwhere(got_a != plain_a)[:4])
            assert (got_b == plain_b).all(), (c, ns, w0, nw, "half B", np.argwhere(got_b != plain_b)[:4])


def test_harness_refuses_windows_outside_the_layout():
    L = harness()
    z = np.zeros(4, np.uint32)
    o = np.zeros(64, np.uint32)
    lay = sr.window_layout(BITS, 13)
    assert L.pw_walk(2, 13, emu._p(z), emu._p(z), 1, lay.W, 1, emu._p(o), emu._p(o)) == -1
    assert L.pw_walk(3, 13, emu._p(z), emu._p(z), 1, 0, 1, emu._p(o), emu._p(o)) == -1
