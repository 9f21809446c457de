"""The digit sort alone (csrc/hip_backend.hip: k_part_count, k_part_scan_blocks, k_scan_u32, k_part_scatter, k_part_scatter_staged,
k_group_sort behind HipBackend::launch_digits_sort), through ctt_hip_sort_probe, against the plain reference tests/_sortref.py.

First half, no GPU: the reference against Python integers, the kernels' digit walker at four scalars per thread (for_each_digit<4>,
run on the host by tests/emu) against the reference, the shape of every crafted case from the reference alone, and the refusal of the
probe without a device.  Second half, `gpu`: every case through the probe over both scatter forms, both block-to-slice maps and both
record widths; every comparison is integer equality (tests/_sortref.py check()).

The same for the 4-word half scalars of the endomorphism split (SortArgs::kwords == 4, load_scalar in csrc/hip_backend.hip), through
ctt_hip_sort_probe_words: the device gets the low four words [n][4], the reference the same scalars zero-extended to 8 words with
bits = 127 -- the layouts whose windows end at bit 128 (cases_half below).

The constants the cases lean on are the kernels' own (csrc/hip_backend.hip): GS_RPT * 1024 = 20 * 1024 = 20480 records stay in
registers between the two sweeps of k_group_sort, GS_MAXBG = 1024 buckets per group, GS_LDS_WORDS = 39936 words of LDS at most
(2 * Bg + 1 + cap + big), at most 16384 groups, and the shipped tile sizes cap = 20480, big = 1024 (msm_plan.h SORT_CAP, SORT_BIG)."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import _banderwagon as bw
from tests import _glvref as gr
from tests import _sortref as sr

GS_REGS, GS_MAXBG, GS_LDS_WORDS, MAX_GROUPS = 20 * 1024, 1024, 39936, 16384
VARIANTS = [(staged, xcd) for staged in (0, 1) for xcd in (0, 1)]
ZERO_BYTES = 32


# --- scalars ---------------------------------------------------------------------------------------------------------------------------
def _random_scalars(seed, n, bits):
    rng = random.Random(seed)
    return [rng.randrange(1 << bits) for _ in range(n)]


def _craft(lay, n, windows, seed):
    """n scalars whose digit in window w is given by windows[w] = [(bucket, count, signs)]: `count` scalars get a digit of value
    bucket + 1 there, signs '+', '-' or '*' (random).  Which scalars is a seeded shuffle per window.  A negative digit -v is the
    window's bits 2^width - v: its carry is a digit +1 in the window above, which must be one the case leaves alone."""
    rng = random.Random(seed)
    ks = [0] * n
    for w, recs in windows.items():
        off, cw = lay.off(w), lay.width(w)
        assert w + 1 not in windows and off + cw < lay.bits     # room for the carry below 2^bits
        total = sum(cnt for _, cnt, _ in recs)
        assert total <= n
        idx = rng.sample(range(n), total)
        i = 0
        for bucket, cnt, signs in recs:
            v = bucket + 1
            for _ in range(cnt):
                neg = signs == "-" or (signs == "*" and rng.random() < 0.5)
                assert v <= (1 << (cw - 1)) - (0 if neg else 1)
                ks[idx[i]] += ((1 << cw) - v if neg else v) << off
                i += 1
    assert all(0 <= k < (1 << lay.bits) for k in ks)
    return ks


class Case:
    """One input of the probe: scalars and sizing.  `table`: the case is also run in the window-table form (merged, id_stride = n + 3)."""

    def __init__(self, name, ks, bits, c, log2_ng, slice_=256, cap=0, big=0, table=False, variants=VARIANTS, kwords=8):
        self.name, self.bits, self.c, self.log2_ng, self.slice, self.cap, self.big = name, bits, c, log2_ng, slice_, cap, big
        self.n, self.table, self.variants, self.kwords = len(ks), table, variants, kwords
        self.words = sr.to_words(ks)                       # what the reference reads: 8 words, the upper four zero when kwords == 4
        assert kwords == 8 or (kwords == 4 and not self.words[:, 4:].any())

    def device_words(self):
        """what the device gets: [n][kwords]"""
        return np.ascontiguousarray(self.words[:, :self.kwords])

    def sizing(self, merged=0):
        return dict(bits=self.bits, c=self.c, slice=self.slice, cap=self.cap, big=self.big, merged=merged,
                    id_stride=self.n + 3 if merged else 0, zero_bytes=ZERO_BYTES)

    def used(self, merged=0):
        return sr.derive(self.n, self.bits, self.c, self.log2_ng, self.slice, merged, self.n + 3 if merged else 0)

    @functools.lru_cache(maxsize=None)
    def expected(self, merged=0):
        return sr.expected(self.words, dict(bits=self.bits, c=self.c, merged=merged, id_stride=self.n + 3))

    def __repr__(self):
        return self.name


# 1. the ordinary path, small: bits 255, c = 8 (32 windows of 8 bits, B = 128), 4 groups, slice 256 -> nblk 1 or 12
def cases_small():
    out = [Case(f"small-n{n}", _random_scalars(100 + n, n, 255), 255, 8, 2, table=True) for n in (1, 63, 64, 65, 3001)]
    out.append(Case("small-zero-n3001", [0] * 3001, 255, 8, 2, table=True))
    out.append(Case("small-zero-n1", [0], 255, 8, 2, table=True))
    return out


# 2. the block-to-slice map (part_slice_of_block deals blocks to XCDs in runs: below 8, at 8, above 8, and many blocks), a ragged last
#    slice, an exact multiple, and a slice of 2 * 4096 + 256 scalars with n = 2 * slice + 77: a block's loop over steps of PS_NS * 1024 =
#    4096 scalars (k_part_scatter, k_part_scatter_staged) then runs three times and ends ragged
def cases_map():
    out = []
    for nblk in (1, 7, 8, 9, 23):
        n = (nblk - 1) * 256 + 101
        out.append(Case(f"map-nblk{nblk}", _random_scalars(200 + nblk, n, 255), 255, 8, 2, table=True))
    out.append(Case("map-exact", _random_scalars(231, 9 * 256, 255), 255, 8, 2, table=True))
    s = 2 * 4096 + 256
    out.append(Case("map-long-slice", _random_scalars(232, 2 * s + 77, 255), 255, 8, 2, slice_=s, table=True))
    return out


# 3. narrow windows: c = 13 over 254 .. 256 bits is 20 windows of 12 bits of which the first r are 13 wide; 8 groups of 512 buckets for
#    the wide windows, of 256 for the narrow ones (gshift_narrow = gshift - 1)
def _narrow_scalars(bits, seed):
    lay = sr.window_layout(bits, 13)
    assert lay.cb == 12 and 0 < lay.r < lay.W - 2
    top, nar = lay.W - 1, lay.r          # the top window and the first narrow one
    ks = _random_scalars(seed, 2500, bits)
    ks += [1 << (lay.off(0) + 12)] * 3                             # window 0 (wide): bits 2^12 -> the digit -2^12, bucket B - 1
    ks += [1 << (lay.off(nar) + 11)] * 3                           # a narrow window: bits 2^11 -> the digit -2^11, bucket B/2 - 1
    ks += [((1 << 11) - 1) << lay.off(top) | 1 << (lay.off(top) - 1)] * 3   # the top window: 2^11 - 1 plus the carry from below -> bucket B/2 - 1
    ks += [(1 << bits) - 1, (1 << bits) - 1, 1, 0]
    assert all(k < (1 << bits) for k in ks)
    return ks


def cases_narrow():
    return [Case(f"narrow-bits{bits}", _narrow_scalars(bits, 300 + bits), bits, 13, 3, table=True) for bits in (255, 253, 254)]


# 4. the thresholds of pass B at the shipped sizes: cap = 20480 = GS_RPT * 1024, big = 1024.  c = 13, 4 groups of 1024 buckets, digits
#    in window 0 only (all positive: a negative digit would carry into window 1).
#      group 0: 20 buckets of 1024 = 20480 records: the register path and the single tile at their limit, no big bucket
#      group 1: 20 buckets of 1024 and one record more = 20481: reloaded from memory, two tiles
#      group 2: a bucket of 1025 (bypasses the LDS image) beside one of 1024 and small ones
#      group 3: a few records
def case_thresholds():
    lay = sr.window_layout(255, 13)
    recs = [(b, 1024, "+") for b in range(0, 40, 2)]
    recs += [(1024 + 3 * b, 1024, "+") for b in range(20)] + [(1024 + 1000, 1, "+")]
    recs += [(2048 + 5, 1025, "+"), (2048 + 6, 1024, "+"), (2048 + 7, 3, "+"), (2048 + 1023, 17, "+")]
    recs += [(3072 + 1, 2, "+"), (4094, 5, "+")]
    n = sum(cnt for _, cnt, _ in recs) + 11             # eleven zero scalars between them
    return Case("thresholds", _craft(lay, n, {0: recs}, 41), 255, 13, 2, slice_=2048)


# 5. the tile path with a smaller tile: cap = 4096, big = 256, c = 11 (24 windows, the first 16 of 11 bits: B = 1024), 2 groups of 512
#    buckets.  Windows 0, 2 and 4 are crafted with digits of both signs; 1, 3 and 5 take the carries of the negative ones (bucket 0).
#      window 0, group 0: 16 buckets of 256 = 4096 records: one tile at its limit, buckets at `big`
#      window 0, group 1: 4097 records, all buckets small: two tiles
#      window 2, group 0: a bucket of 257 (bypass) beside one of 256, below cap: the general path from registers
#      window 2, group 1: small buckets that start at offset cap - 1 (and spill into arr[cap .. cap + big)) and exactly at 2 * cap
#      window 4, group 0: a bucket of 3 * cap + 12 records between small ones: tiles 1 and 2 have no small bucket starting in them
#      window 4, group 1: 81 buckets of 256 = 20736 > 20480 records, all small: reloaded from memory and tiled
def case_tiles():
    lay = sr.window_layout(255, 11)
    w0 = [(b, 256, "*") for b in range(16)]
    w0 += [(512 + 2 * b, 256, "*") for b in range(16)] + [(1022, 1, "+")]
    w2 = [(3, 257, "*"), (4, 256, "*"), (9, 100, "*"), (511, 30, "*")]
    w2 += [(512 + b, 256, "*") for b in range(15)] + [(512 + 15, 255, "*"), (512 + 20, 200, "*")]       # 4095 before the 200
    w2 += [(512 + 30 + b, 256, "*") for b in range(15)] + [(512 + 50, 57, "*"), (512 + 60, 100, "-")]   # 8192 before the 100
    w4 = [(3, 10, "*"), (5, 3 * 4096 + 12, "*"), (6, 90, "*"), (500, 7, "*")]
    w4 += [(512 + 6 * b, 256, "*") for b in range(81)]
    n = 34000
    return Case("tiles", _craft(lay, n, {0: w0, 2: w2, 4: w4}, 42), 255, 11, 1, slice_=2048, cap=4096, big=256)


# 6. more than 1024 groups: the carry of k_scan_u32 over several steps of 1024, the direct scatter whatever `staged` says, and window
#    batches of 16384 / NG windows with a short last one (20 windows in batches of 8 / of 4; 18 windows one at a time)
def cases_many_groups():
    return [Case("groups2048", _random_scalars(61, 5003, 255), 255, 13, 11, table=True),
            Case("groups4096", _random_scalars(62, 4999, 255), 255, 13, 12, table=True),
            Case("groups16384", _random_scalars(63, 3001, 255), 255, 15, 14, table=True)]


# 7. the table form: one bucket set of Wd * n candidates, 64-bit records.  Of NG in {1, 2, 256, 1024} x c in {8, 13} the launcher runs
#    NG <= B = 128 at c = 8 and B / NG <= GS_MAXBG at c = 13: {1, 2} at c = 8 (a single group of more than 20480 records; NG = 1 staged
#    puts the 64-bit stage of k_part_scatter_staged at an odd word of LDS) and {256, 1024} at c = 13.  (Run merged only.)
def cases_table():
    return [Case("table-c8-ng1", _random_scalars(71, 701, 255), 255, 8, 0),
            Case("table-c8-ng2", _random_scalars(72, 702, 255), 255, 8, 1),
            Case("table-c13-ng256", _random_scalars(73, 1501, 255), 255, 13, 8),
            Case("table-c13-ng1024", _random_scalars(74, 1499, 255), 255, 13, 10)]


# 8. the half scalars of the endomorphism split: 4 words per scalar, bits = 127, windows over 128 bits.  (c, log2 NG):
#      c = 16   8 windows of 16 bits, B = 2^15, 32 groups: the shipped shape
#      c = 13   10 windows: 8 of 13 bits and 2 narrow ones of 12 (gshift_narrow = gshift - 1 on the top windows), 8 groups
#      c = 8    16 windows;   c = 5   26 windows, the first 24 of 5 bits
#    Scalars: seeded values below 2^127; the real halves of the Python split of seeded scalars (255 bits; below x^2 / 2, whose second
#    half is zero; a few x^2 and a little, whose second half is tiny: few or no records); 2^127 - 1; the largest top-window digit with a
#    carry from below (as _narrow_scalars crafts it); zero.  (Plain form only: a table never has half scalars.)
HALF_BITS = 127
HALF_LAYOUTS = ((16, 5), (13, 3), (8, 2), (5, 2))


def _real_halves(seed, count):
    rng = random.Random(seed)
    ks = [rng.getrandbits(255) for _ in range(count)] + [rng.randrange(gr.X2 // 2) for _ in range(count // 2)]
    ks += [rng.randrange(1, 9) * gr.X2 + rng.randrange(1 << 40) for _ in range(count // 2)]
    out = []
    for k in ks:
        s = gr.split(k)
        out += [s.k1, s.k2]
    return out


def _half_scalars(c, n, seed):
    lay = sr.window_layout(HALF_BITS, c)
    top = lay.W - 1
    off, cw = lay.off(top), lay.width(top)
    assert off + cw == 128
    ks = [(1 << 127) - 1, 0] + [((1 << (cw - 1)) - 1) << off | 1 << (off - 1)] * 3 + [1]
    ks += _real_halves(seed, (n + 7) // 8)
    ks = _random_scalars(seed + 1, 1, HALF_BITS) + ks        # (n = 1: a seeded value)
    ks += _random_scalars(seed + 2, max(0, n - len(ks)), HALF_BITS)
    assert all(k < (1 << HALF_BITS) for k in ks)
    return ks[:n]


def cases_half():
    out = []
    for c, lg in HALF_LAYOUTS:
        out += [Case(f"half-c{c}-n{n}", _half_scalars(c, n, 800 + 10 * c + n), HALF_BITS, c, lg, kwords=4) for n in (1, 65, 3001)]
    out.append(Case("half-zero-n3001", [0] * 3001, HALF_BITS, 16, 5, kwords=4))
    out.append(Case("half-zero-n1", [0], HALF_BITS, 13, 3, kwords=4))
    s = 2 * 4096 + 256
    out.append(Case("half-long-slice", _half_scalars(16, 2 * s + 77, 899), HALF_BITS, 16, 5, slice_=s, kwords=4))
    return out


ORDINARY = cases_small() + cases_map() + cases_narrow() + cases_many_groups()
HALF = cases_half()
CRAFTED = [case_thresholds(), case_tiles()]
TABLE_ONLY = cases_table()


# --- CPU: the reference itself ---------------------------------------------------------------------------------------------------------
def _edge_scalars(bits):
    top = 1 << bits
    ks = [0, 1, 2, top - 1, top - 2, top >> 1, (top >> 1) - 1, int("55" * 32, 16) % top, int("aa" * 32, 16) % top, int("80" * 32, 16) % top,
          int("ff" * 32, 16) % top, int("01" * 32, 16) % top]
    for order in [c.order for c in po.CURVES.values()] + [bw.R]:
        ks += [k for k in (order - 1, order, order + 1) if k < top]
    return ks + _random_scalars(7 * bits, 200, bits)


@pytest.mark.parametrize("bits", [127, 253, 254, 255])
def test_reference_digits_recompose_the_scalar(bits):
    """sum_w +-val_w * 2^off(w) == k for every c, with Python integers; the vectorised digits equal the integer ones; the layout equals
    the engine's wherever its plan takes that c."""
    from tests.emu import emu
    ks = _edge_scalars(bits)
    words = sr.to_words(ks)
    assert sr.from_words(words) == ks
    for c in range(2, 21):
        lay = sr.window_layout(bits, c)
        assert sum(lay.width(w) for w in range(lay.W)) == bits + 1 and lay.off(lay.W - 1) + lay.width(lay.W - 1) == bits + 1
        assert lay.cmax() <= c and all(lay.width(w) in (lay.cb, lay.cb + 1) for w in range(lay.W))
        val, neg = sr.digits(words, lay)
        for j, k in enumerate(ks):
            dg = [sr.booth_digit(k, w, lay) for w in range(lay.W)]
            assert sum((-v if s else v) << lay.off(w) for w, (v, s) in enumerate(dg)) == k, (bits, c, hex(k))
            assert all(v <= 1 << (lay.width(w) - 1) for w, (v, s) in enumerate(dg))
            assert [int(x) for x in val[:, j]] == [v for v, _ in dg] and [bool(x) for x in neg[:, j]] == [s for _, s in dg]
    seen = set()
    for n in (1, 100, 4096, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24):
        for lanes in (65536, 196608):
            p = emu.plan(n, bits, lanes)
            lay = sr.window_layout(bits, p["c"])
            assert (lay.cmax(), lay.W, lay.cb, lay.r, 1 << (lay.cmax() - 1)) == (p["c"], p["W"], p["cb"], p["r"], p["B"])
            u = sr.derive(n, bits, p["c"], p["NG"].bit_length() - 1, p["slice"])
            assert (u["NG"], u["gshift"], u["nblk"], u["nent"]) == (p["NG"], p["gshift"], p["S"], p["nent"])
            seen.add(p["c"])
    assert len(seen) >= 3


@pytest.mark.parametrize("bits", [127, 253, 254, 255])
def test_digit_walker_of_the_kernels_at_four_scalars(bits):
    """for_each_digit<4> (what k_part_count and the scatter kernels instantiate) on the host against the reference: every c, whole
    walks and walks over windows [w0, w0 + nw) with w0 > 0 and nw < Wd, a ragged last group of scalars.  c = 16 at 255 bits starts
    every other window at bit 31 of a word, c = 2 has 128 windows, c = 20 straddles words at every offset.  bits = 127: the layouts over
    128 bits of the half scalars, the upper four words zero -- what load_scalar hands the walker for kwords == 4."""
    from tests.emu import emu
    ks = _edge_scalars(bits)
    while len(ks) % 4 != 3:                        # a ragged last group of three
        ks.pop()
    assert len(ks) % 4 == 3
    words = sr.to_words(ks)
    for c in range(2, 21):
        lay = sr.window_layout(bits, c)
        val, neg = sr.digits(words, lay)
        want = np.where(val > 0, ((val - 1) << 1) | neg, 0xFFFFFFFF).astype(np.uint32)
        got, W = emu.digits(bits, c, words)
        assert W == lay.W and got.shape == want.shape
        assert (got == want).all(), (bits, c, np.argwhere(got != want)[:4])
        for w0, nw in {(1, lay.W - 1), (lay.W // 2, max(1, lay.W // 3)), (lay.W - 1, 1), (min(3, lay.W - 1), 1)}:
            if w0 + nw > lay.W or nw < 1:
                continue
            part, _ = emu.digits(bits, c, words, w0, nw)
            assert (part == want[w0:w0 + nw]).all(), (bits, c, w0, nw)
    assert sr.window_layout(255, 16).off(1) - 1 == 15 and (sr.window_layout(255, 16).off(2) - 1) % 32 == 31
    assert sr.window_layout(255, 2).W == 128


# --- CPU: the crafted cases have the shape they are named for -------------------------------------------------------------------------
def _groups(case, w):
    """(records of every group, counts reshaped (NG, Bg)) of window w's set"""
    u = case.used()
    lay = sr.window_layout(case.bits, case.c)
    gs = u["gshift"] if lay.is_wide(w) else u["gshift_narrow"]
    counts = case.expected()[w]["counts"]
    assert counts[u["NG"] << gs:].sum() == 0
    per = counts[:u["NG"] << gs].reshape(u["NG"], 1 << gs)
    return per.sum(axis=1), per


def test_shape_of_the_ordinary_cases():
    by = {c.name: c for c in ORDINARY}
    assert [by[f"small-n{n}"].used()["nblk"] for n in (1, 63, 64, 65, 3001)] == [1, 1, 1, 1, 12]
    assert all(u["NG"] == 4 and u["B"] == 128 and u["W"] == 32 for u in (c.used() for c in cases_small() + cases_map()))
    for name in ("small-zero-n3001", "small-zero-n1"):
        assert all(s["counts"].sum() == 0 for s in by[name].expected())
    assert [by[f"map-nblk{k}"].used()["nblk"] for k in (1, 7, 8, 9, 23)] == [1, 7, 8, 9, 23]
    assert all(by[f"map-nblk{k}"].n % 256 for k in (1, 7, 8, 9, 23)) and by["map-exact"].n % 256 == 0 and by["map-exact"].used()["nblk"] == 9
    long_ = by["map-long-slice"]
    assert long_.used()["nblk"] == 3 and long_.slice > 2 * 4096 and long_.slice % 4096 and (long_.n - 2 * long_.slice) % 4096 == 77
    # narrow windows: half-width groups, and records in the highest bucket a wide, a narrow and the top window reach
    for bits in (255, 253, 254):
        case = by[f"narrow-bits{bits}"]
        u, lay, exp = case.used(), sr.window_layout(bits, 13), case.expected()
        assert (u["W"], u["B"], u["NG"], u["gshift"], u["gshift_narrow"]) == (20, 4096, 8, 9, 8) and u["r"] == bits - 239
        assert exp[0]["counts"][4095] >= 3 and exp[lay.r]["counts"][2047] >= 3 and exp[19]["counts"][2047] >= 3
        assert all(exp[w]["counts"][2048:].sum() == 0 for w in range(lay.r, 20))
        assert all(_groups(case, w)[0].min() > 0 for w in range(20))       # every group of every window holds records
        assert any(bool((s["entries"] >> 31).any()) and not bool((s["entries"] >> 31).all()) for s in exp)   # both signs
    # more than 1024 groups
    for name, ng, W, wb in (("groups2048", 2048, 20, 8), ("groups4096", 4096, 20, 4), ("groups16384", 16384, 18, 1)):
        u = by[name].used()
        assert (u["NG"], u["W"]) == (ng, W) and ng > 1024 and MAX_GROUPS // ng == wb < W and u["B"] // ng <= 2
        assert by[name].used(1)["NG"] == ng
    assert 20 % 8 == 4                                                     # 2048 groups: two batches of 8 windows and a short one of 4
    assert by["groups16384"].used()["NG"] == MAX_GROUPS == by["groups16384"].used()["B"]


def test_shape_of_the_threshold_case():
    case = case_thresholds()
    u, exp = case.used(), case.expected()
    assert (u["NG"], u["B"], u["gshift"]) == (4, 4096, 10) and case.cap == case.big == 0 and case.n <= 45000
    assert sr.DEFAULT_CAP == GS_REGS == 20480 and sr.DEFAULT_BIG == 1024
    assert all(s["counts"].sum() == 0 for s in exp[1:])                     # window 0 only
    ng, per = _groups(case, 0)
    assert ng[0] == 20480 and per[0].max() == 1024                         # at the register limit and the tile limit, nothing big
    assert ng[1] == 20481 and per[1].max() == 1024                         # one more: reloaded, a second tile
    assert sorted(per[2][per[2] >= 1024]) == [1024, 1025] and ng[2] < 20480  # one bucket at `big`, one above
    assert 0 < ng[3] < 100


def test_shape_of_the_tile_case():
    case = case_tiles()
    u, exp = case.used(), case.expected()
    cap, big = case.cap, case.big
    assert (u["NG"], u["B"], u["gshift"], cap, big) == (2, 1024, 9, 4096, 256) and case.n <= 45000
    assert 2 * (u["B"] // u["NG"]) + 1 + cap + big <= GS_LDS_WORDS
    g0, p0 = _groups(case, 0)
    assert g0[0] == cap and p0[0].max() == big                             # one tile, at its limit
    assert g0[1] == cap + 1 and p0[1].max() == big                         # two tiles
    g2, p2 = _groups(case, 2)
    assert g2[0] < cap and sorted(p2[0][p2[0] >= big]) == [256, 257]
    start = np.concatenate(([0], np.cumsum(p2[1])[:-1]))
    small = (p2[1] > 0) & (p2[1] <= big)
    assert p2[1].max() <= big
    spill = small & (start % cap == cap - 1) & (p2[1] > 1)                 # starts in the last slot of tile 0, ends in arr[cap ..)
    assert spill.any() and (start[spill] // cap == 0).all() and (start[spill] + p2[1][spill] > cap).all()
    assert (small & (start == 2 * cap)).any()
    g4, p4 = _groups(case, 4)
    start = np.concatenate(([0], np.cumsum(p4[0])[:-1]))
    small = (p4[0] > 0) & (p4[0] <= big)
    assert p4[0].max() >= 3 * cap
    tiles = set((start[small] // cap).tolist())
    assert tiles == {0, 3} and g4[0] > 3 * cap                             # tiles 1 and 2 lie inside the big bucket and are skipped
    assert g4[1] == 81 * 256 > GS_REGS and p4[1].max() == big              # beyond the registers, every bucket small
    for w in (0, 2, 4):                                                    # both signs in the crafted windows, the carries above them
        sign = exp[w]["entries"] >> 31
        assert sign.any() and not sign.all()
        assert exp[w + 1]["counts"][0] == int(sign.sum()) and exp[w + 1]["counts"][1:].sum() == 0
    assert all(s["counts"].sum() == 0 for s in exp[6:])


def test_shape_of_the_half_cases():
    """the reference works for the four layouts over 128 bits, and the cases hold what they are named for"""
    shapes = {16: (8, 16, 0), 13: (10, 12, 8), 8: (16, 8, 0), 5: (26, 4, 24)}            # c: (windows, cb, r)
    by = {c.name: c for c in HALF}
    assert len(by) == len(HALF) == 4 * 3 + 3 and all(c.kwords == 4 and c.bits == 127 and not c.table for c in HALF)
    for c, lg in HALF_LAYOUTS:
        lay = sr.window_layout(HALF_BITS, c)
        assert (lay.W, lay.cb, lay.r) == shapes[c] and lay.cmax() == c and lay.off(lay.W - 1) + lay.width(lay.W - 1) == 128
        for n in (1, 65, 3001):
            case = by[f"half-c{c}-n{n}"]
            u, exp = case.used(), case.expected()
            assert case.n == n and case.device_words().shape == (n, 4) and (u["W"], u["NG"], u["B"]) == (lay.W, 1 << lg, 1 << (c - 1))
            assert u["gshift_narrow"] == (u["gshift"] - 1 if lay.r else u["gshift"]) and u["B"] >> u["gshift"] == u["NG"]
            assert len(exp) == lay.W
            ks = sr.from_words(case.words)
            for j, k in enumerate(ks[:40]):                                             # the reference's digits recompose the half
                assert sum((-v if s else v) << lay.off(w) for w, (v, s) in enumerate(sr.booth_digit(k, w, lay) for w in range(lay.W))) == k
            if n > 1:
                top = exp[lay.W - 1]["counts"]
                assert top[(1 << (lay.width(lay.W - 1) - 1)) - 1] >= 3                  # the largest top-window digit, by the carry
                assert (1 << 127) - 1 in ks and 0 in ks and any(0 < k < 1 << 64 for k in ks)
                assert any(bool((s["entries"] >> 31).any()) and not bool((s["entries"] >> 31).all()) for s in exp)   # both signs
            if n == 3001:
                assert all(_groups(case, w)[0].min() > 0 for w in range(lay.W - 1))     # every group of every window but the top holds records
                small = sum(1 for k in ks if k < 1 << 48)
                assert small >= 100                                                     # halves with few or no records
    u13 = by["half-c13-n3001"].used()
    assert (u13["W"], u13["NG"], u13["gshift"], u13["gshift_narrow"], u13["r"]) == (10, 8, 9, 8, 8)
    u16 = by["half-c16-n3001"].used()
    assert (u16["W"], u16["B"], u16["NG"], u16["B"] // u16["NG"]) == (8, 1 << 15, 32, GS_MAXBG)
    for name in ("half-zero-n3001", "half-zero-n1"):
        assert all(s["counts"].sum() == 0 for s in by[name].expected())
    long_ = by["half-long-slice"]
    assert long_.used()["nblk"] == 3 and long_.slice > 2 * 4096 and long_.slice % 4096 and (long_.n - 2 * long_.slice) % 4096 == 77
    s0 = gr.split(_random_scalars(5, 1, 255)[0])
    assert max(s0.k1, s0.k2) < 1 << 127


def test_shape_of_the_table_cases():
    for case, ng, bg in zip(TABLE_ONLY, (1, 2, 256, 1024), (128, 64, 16, 4)):
        u = case.used(1)
        assert (u["W"], u["NG"], u["B"] // u["NG"], u["gshift_narrow"], u["jbits"]) == (1, ng, bg, u["gshift"], 0) and bg <= GS_MAXBG
        assert u["nent"] == u["Wd"] * case.n and case.sizing(1)["id_stride"] > case.n
        exp = case.expected(1)
        assert len(exp) == 1 and exp[0]["counts"].sum() > 0.9 * u["nent"]
        rows = exp[0]["entries"] & 0x7FFFFFFF
        assert int(rows.max()) >= (u["Wd"] - 1) * (case.n + 3)             # rows of the last window
    ng1 = TABLE_ONLY[0]
    assert ng1.expected(1)[0]["counts"].sum() > GS_REGS                   # a single group beyond the registers
    # NG = 1: the stage of 64-bit records of k_part_scatter_staged<true> starts at byte (3 * NG + 16) * 4 + 2 * 4096 of LDS: 4 mod 8
    assert ((3 * 1 + 16) * 4 + 2 * 4096) % 8 == 4


# --- CPU: the wiring -------------------------------------------------------------------------------------------------------------------
def test_probe_symbol_is_exported_and_the_abi_version_stays():
    from constantine_amd import _lib
    L = _lib.lib()
    assert "ctt_hip_sort_probe" in _lib.exported_symbols() and hasattr(L, "ctt_hip_sort_probe")
    assert "ctt_hip_sort_probe_words" in _lib.exported_symbols() and hasattr(L, "ctt_hip_sort_probe_words")
    assert L.ctt_hip_msm_abi_version() == _lib.ABI_VERSION == 11


def test_without_a_device_the_probe_refuses():
    from constantine_amd import _lib
    L = _lib.lib()
    if L.ctt_hip_msm_available() == 1:
        pytest.skip("a HIP device is present: the refusal path of a device-less box cannot be shown here")
    vp = ctypes.c_void_p
    bufs = [np.full(n, 0xAB, np.uint8) for n in (32, 14 * 4, 11 * 4, 64, 64, 16, 64)]
    p = [a.ctypes.data_as(vp) for a in bufs]
    L.ctt_hip_clear_last_error()
    assert L.ctt_hip_sort_probe(None, p[0], 1, p[1], p[2], p[3], p[4], p[5], p[6]) == -1
    assert L.ctt_hip_last_error() == -3
    assert all(bytes(a) == bytes([0xAB]) * len(a) for a in bufs)
    for kwords in (4, 8):
        L.ctt_hip_clear_last_error()
        assert L.ctt_hip_sort_probe_words(None, p[0], kwords, 1, p[1], p[2], p[3], p[4], p[5], p[6]) == -1
        assert L.ctt_hip_last_error() == -3
        assert all(bytes(a) == bytes([0xAB]) * len(a) for a in bufs)


# --- GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


class _Buffers:
    """The probe's four outputs on the device with their guards, pre-filled as tests/_sortref.py new_outputs() fills them."""

    def __init__(self, torch, used, zero_bytes):
        self.torch = torch
        host = sr.new_outputs(used, zero_bytes)
        self.t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
        self.keep = host
        self.used, self.zero_bytes = used, zero_bytes

    def views(self):
        """what the probe is told it may write: the buffers without their guards"""
        u, t = self.used, self.t
        return (t["entries"][:u["W"] * u["nent"]], t["bstart"][:u["W"] * (u["B"] + 1)], t["maxcount"][:4],
                t["buckets"][:u["W"] * u["B"] * self.zero_bytes])

    def host(self):
        self.torch.cuda.synchronize()
        return {k: (v.cpu().numpy().view(np.uint32) if k != "buckets" else v.cpu().numpy()) for k, v in self.t.items()}

    def untouched(self):
        h = self.host()
        return all((h[k] == self.keep[k]).all() for k in h)


def _run(torch, dev, case, merged, staged, xcd, d_words):
    used = case.used(merged)
    buf = _Buffers(torch, used, ZERO_BYTES)
    e, b, m, z = buf.views()
    got = dev.sort_probe(d_words, case.n, e, b, m, z, log2_ng=case.log2_ng, kwords=case.kwords, staged=staged, xcd_map=xcd, **case.sizing(merged))
    assert got == used, (case, merged, staged, xcd, got, used)
    return buf.host(), used


def _run_and_check(dev, case, forms):
    import torch
    d_words = torch.from_numpy(case.device_words().view(np.int32)).cuda()
    for merged in forms:
        exp = case.expected(merged)
        for staged, xcd in case.variants:
            out, used = _run(torch, dev, case, merged, staged, xcd, d_words)
            try:
                sr.check(out, exp, used, ZERO_BYTES)
            except AssertionError as err:
                raise AssertionError(f"{case} merged={merged} staged={staged} xcd_map={xcd}: {err}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("case", ORDINARY, ids=repr)
def test_sort_probe_ordinary_cases_gpu(case, dev):
    """cases 1, 2, 3 and 6 of the module's list, in both record widths"""
    _run_and_check(dev, case, (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CRAFTED, ids=repr)
def test_sort_probe_thresholds_of_pass_b_gpu(case, dev):
    """cases 4 and 5: the shapes are per window, so the table form (one set for all windows) does not apply"""
    _run_and_check(dev, case, (0,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE_ONLY, ids=repr)
def test_sort_probe_table_form_gpu(case, dev):
    _run_and_check(dev, case, (1,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALF, ids=repr)
def test_sort_probe_half_scalars_gpu(case, dev):
    """case 8: 4-word scalars, the plain form over both scatter forms and both block maps"""
    _run_and_check(dev, case, (0,))


@pytest.mark.gpu
@pytest.mark.parametrize("c, lg", [(16, 5), (13, 3)])
def test_sort_probe_half_scalars_outside_the_contract_gpu(c, lg, dev):
    """half scalars with bit 127 set (the plan is made for 127 bits): the same four promises as for 8-word scalars below"""
    import torch
    rng = random.Random(82 + c)
    ks = [rng.randrange(1 << 127) | 1 << 127 for _ in range(1500)] + [(1 << 128) - 1, 1 << 127, (1 << 128) - 1, 1 << 127]
    case = Case("half-outside", ks, HALF_BITS, c, lg, kwords=4)
    lay = sr.window_layout(HALF_BITS, c)
    val, _ = sr.digits(case.words, lay)
    d_words = torch.from_numpy(case.device_words().view(np.int32)).cuda()
    for staged, xcd in VARIANTS:
        out, u = _run(torch, dev, case, 0, staged, xcd, d_words)
        sr.check_guards(out, u, ZERO_BYTES)
        for r in range(u["W"]):
            bs = out["bstart"][r * (u["B"] + 1):(r + 1) * (u["B"] + 1)].astype(np.int64)
            assert bs[0] == 0 and (np.diff(bs) >= 0).all(), (r, staged, xcd)
            assert bs[-1] == int((val[r] > 0).sum()), (r, staged, xcd)
            ent = out["entries"][r * case.n:r * case.n + bs[-1]]
            assert ((ent & 0x7FFFFFFF) < case.n).all(), (r, staged, xcd)
        assert (out["maxcount"][1:4] == 0).all()


@pytest.mark.gpu
def test_sort_probe_scalars_outside_the_contract_gpu(dev):
    """bits = 254, c = 14 with bits 254 and 255 of the scalars set: the digits are unspecified, what the code promises is not -- nothing
    out of bounds, bstart non-decreasing, bstart[B] the number of non-zero digits of the set, every entry a point index below n."""
    import torch
    rng = random.Random(81)
    ks = [rng.randrange(1 << 254) | 3 << 254 for _ in range(1500)] + [(1 << 256) - 1, 3 << 254, 1 << 254, 1 << 255]
    case = Case("outside", ks, 254, 14, 3)
    lay = sr.window_layout(254, 14)
    val, _ = sr.digits(case.words, lay)
    d_words = torch.from_numpy(case.words.view(np.int32)).cuda()
    for staged, xcd in VARIANTS:
        out, u = _run(torch, dev, case, 0, staged, xcd, d_words)
        sr.check_guards(out, u, ZERO_BYTES)
        for r in range(u["W"]):
            bs = out["bstart"][r * (u["B"] + 1):(r + 1) * (u["B"] + 1)].astype(np.int64)
            assert bs[0] == 0 and (np.diff(bs) >= 0).all(), (r, staged, xcd)
            assert bs[-1] == int((val[r] > 0).sum()), (r, staged, xcd)
            ent = out["entries"][r * case.n:r * case.n + bs[-1]]
            assert ((ent & 0x7FFFFFFF) < case.n).all(), (r, staged, xcd)
        assert (out["maxcount"][1:4] == 0).all()


def _refusals(n):
    """(what, n, sizing) of every plan the probe refuses before a launch; the last two are what launch_digits_sort would abort on"""
    ok = dict(bits=255, c=8, log2_ng=2, slice=256, zero_bytes=ZERO_BYTES)
    big_n = (1 << 31) - 1
    return [("n = 0", 0, ok), ("n above 2^31 - 1", 1 << 31, ok), ("c = 1", n, dict(ok, c=1)), ("c = 21", n, dict(ok, c=21)),
            ("bits = 0", n, dict(ok, bits=0)), ("bits = 256", n, dict(ok, bits=256)), ("more groups than buckets", n, dict(ok, log2_ng=8)),
            ("a negative slice", n, dict(ok, slice=-1)), ("a negative cap", n, dict(ok, cap=-5)), ("staged = 2", n, dict(ok, staged=2)),
            ("log2 NG = -2", n, dict(ok, log2_ng=-2)),
            ("merged, id_stride < n", n, dict(ok, merged=1, id_stride=n - 1)), ("zero_bytes = 24", n, dict(ok, zero_bytes=24)),
            ("too many table rows", n, dict(ok, merged=1, id_stride=1 << 27)),
            ("cap + big beyond the LDS", n, dict(ok, cap=GS_LDS_WORDS - 1024, big=1024)),
            ("more than 1024 buckets per group", n, dict(ok, c=13, log2_ng=1)),
            ("more than 16384 groups", n, dict(ok, c=20, log2_ng=15)),
            ("a record above 32 bits", big_n, dict(ok, c=13, log2_ng=10)),
            ("scalars of 5 words", n, dict(ok, kwords=5)), ("scalars of 0 words", n, dict(ok, kwords=0)),
            ("4 words under windows that end above bit 128", n, dict(ok, kwords=4)),
            ("4 words under windows over 129 bits", n, dict(ok, kwords=4, bits=128, c=16, log2_ng=5))]


@pytest.mark.gpu
def test_sort_probe_refusals_gpu(dev):
    """every refusal: -1, the last error set, all four outputs at their fill; then the same call with legal values goes through"""
    import torch
    from constantine_amd import _lib
    L = _lib.lib()
    case = cases_small()[3]
    used = case.used()
    d_words = torch.from_numpy(case.words.view(np.int32)).cuda()
    buf = _Buffers(torch, used, ZERO_BYTES)
    e, b, m, z = buf.views()
    for what, n, sizing in _refusals(case.n):
        L.ctt_hip_clear_last_error()
        assert dev.sort_probe(d_words, n, e, b, m, z, **sizing) is None, what
        assert L.ctt_hip_last_error() != 0 and L.ctt_hip_last_error_message(), what
        if what in ("cap + big beyond the LDS", "more than 1024 buckets per group", "more than 16384 groups", "a record above 32 bits",
                    "4 words under windows that end above bit 128", "4 words under windows over 129 bits"):
            assert b"launcher" in L.ctt_hip_last_error_message(), what      # the predicate of launch_digits_sort, not its abort
        assert buf.untouched(), what
    # a buffer smaller than the derived shape, and NULL pointers
    ok = dict(log2_ng=2, **case.sizing())
    assert dev.sort_probe(d_words, case.n, e[:-1], b, m, z, **ok) is None and buf.untouched()
    assert dev.sort_probe(d_words, case.n, e, b[:-1], m, z, **ok) is None and buf.untouched()
    assert dev.sort_probe(d_words, case.n, e, b, m, z[:-1], **ok) is None and buf.untouched()
    assert dev.sort_probe(d_words, case.n, e, b, m, None, **ok) is None and buf.untouched()
    args = np.array([255, 8, 2, 256, 0, 0, 0, 0, 0, 0, 0, e.numel(), b.numel(), 0], dtype=np.int32)
    out = np.full(11, 0xABABABAB, dtype=np.uint32)
    vp = ctypes.c_void_p
    ptrs = [vp(d_words.data_ptr()), args.ctypes.data_as(vp), out.ctypes.data_as(vp), vp(e.data_ptr()), vp(b.data_ptr()), vp(m.data_ptr())]
    for i in range(len(ptrs)):
        p = list(ptrs)
        p[i] = None
        assert L.ctt_hip_sort_probe(dev.ctx, p[0], case.n, p[1], p[2], p[3], p[4], p[5], None) == -1, i
        assert L.ctt_hip_last_error() != 0 and (out == 0xABABABAB).all() and buf.untouched(), i
    # legal values: the call goes through and the result is the reference's
    got = dev.sort_probe(d_words, case.n, e, b, m, z, **ok)
    assert got == used
    sr.check(buf.host(), case.expected(), used, ZERO_BYTES)


@pytest.mark.gpu
def test_sort_probe_between_outstanding_msm_tickets_gpu(dev):
    """a probe call between two outstanding MSM tickets of the same context leaves both results the oracle's, and its own the reference's"""
    import torch
    from oracle import cref
    name = "bls12_381_g1"
    data = []
    for i, n in enumerate((3000, 4096)):
        pts, sc = cref.gen_points(name, 910 + i, n), cref.synth_scalars(920 + i, n, 255)
        data.append((n, torch.from_numpy(np.ascontiguousarray(sc)).cuda(), torch.from_numpy(np.ascontiguousarray(pts)).cuda(),
                     bytes(cref.msm(name, sc, pts, nthreads=8)[0])))
    case = cases_small()[4]
    d_words = torch.from_numpy(case.words.view(np.int32)).cuda()
    used = case.used()
    buf = _Buffers(torch, used, ZERO_BYTES)
    e, b, m, z = buf.views()
    t0 = dev.submit(name, data[0][1], data[0][2], data[0][0])
    t1 = dev.submit(name, data[1][1], data[1][2], data[1][0])
    got = dev.sort_probe(d_words, case.n, e, b, m, z, log2_ng=case.log2_ng, staged=1, xcd_map=1, **case.sizing())
    r1, r0 = dev.finish(t1), dev.finish(t0)
    assert bytes(r0) == data[0][3] and bytes(r1) == data[1][3]
    assert got == used
    sr.check(buf.host(), case.expected(), used, ZERO_BYTES)
