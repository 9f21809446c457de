"""The pair forms of the sort's partition kernels on the GPU (run with -m gpu on an MI355X): csrc/hip_backend.hip k_part_count<true>,
k_part_scatter<false, true> and k_part_scatter_staged<false, true>, which launch_digits_sort takes for 4-word half scalars whenever n and
the slice are even (csrc/msm_bodies.h sort_by_pairs) -- every split MSM.  Slice blk then holds the PAIRS [blk * slice / 2, (blk + 1) *
slice / 2), the entries j and n / 2 + j of each, and one thread walks both halves of a pair.  Through ctt_hip_sort_probe_words, against
tests/_sortref.py (per-bucket multisets of the entries, bstart, maxcount[0], the cleared empty buckets, every guard): the output contract
is the one of every other form.  The 4-word cases of tests/test_sort_probe.py have odd n and keep the kernels that walk scalar by scalar.

The device gets the half scalars of the split (tests/_glvref.py split()) of p pairs as [2p][4]: half j = k1, half p + j = k2.  Shapes,
with the slice set to 512 half scalars = 256 pairs (SLICE): 1 and 2 pairs; 63, 64, 65 (a wave one short, exact, one over); 255, 256, 257
(a slice one short, exact, and a second block of one pair); 9 slices and an odd remainder of 77 pairs with xcd_map on and off (10 blocks:
part_slice_of_block deals 8 + 2 blocks with a remainder); 6001 pairs (24 blocks; a lane holds two pairs, a block 2048 at a time, so
every block has idle lanes and zero pairs) with c = 13 and 256 groups in the staged form, c = 13 and 8 groups in the direct form, c = 4
and one group (32 windows of 8 buckets, every bucket above `big`); an odd slice with even n, which must take the scalar-by-scalar
kernels and give the same.  Scalars: seeded values below r; 0, 1, r - 1, (r - 1) / 2; x^2 and 2 x^2, where one half comes out 0; and
one case of 300 equal scalars under big = 64, where every non-empty bucket bypasses pass B's LDS image.
"""
import functools
import random

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import _glvref as gr
from tests import _sortref as sr

pytestmark = pytest.mark.gpu

R = po.CURVES["bls12_381_g1"].order
SLICE = 512            # half scalars per partition slice: 256 pairs
ZERO_BYTES = 32
BITS = 127


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from constantine_amd import DeviceMsm
    d = DeviceMsm(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _halves(p, kind="mixed"):
    """the 2p half scalars of p pairs as Python integers: k1 of every pair, then k2 of every pair"""
    rng = random.Random(0xC0DE00 + p)
    special = [0, 1, R - 1, (R - 1) // 2, gr.X2, 2 * gr.X2]
    if kind == "equal":
        ks = [rng.randrange(R)] * p
    else:
        ks = [rng.randrange(R) for _ in range(p)]
        if p >= 63:
            ks[:len(special)] = special
            ks[p - 7:p - 1] = special          # the ragged end of the last slice holds them as well
        elif p == 2:
            ks = [R - 1, gr.X2]
    sp = [gr.split(k) for k in ks]
    assert all(2 * s.k1 <= gr.X2 and 2 * s.k2 <= gr.X2 for s in sp)
    if kind == "mixed" and p >= 2:
        assert any(s.k2 == 0 for s in sp)
    return [s.k1 for s in sp] + [s.k2 for s in sp]


@functools.lru_cache(maxsize=None)
def _expected(p, kind, c):
    return sr.expected(sr.to_words(_halves(p, kind)), dict(bits=BITS, c=c))


def _run(dev, p, kind, c, lg, staged, xcd, big=0, slice_=SLICE):
    import torch
    n = 2 * p
    used = sr.derive(n, BITS, c, lg, slice_)
    host = sr.new_outputs(used, ZERO_BYTES)
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
    words = np.ascontiguousarray(sr.to_words(_halves(p, kind))[:, :4])
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    W, B, nent = used["W"], used["B"], used["nent"]
    got = dev.sort_probe(d_words, n, t["entries"][:W * nent], t["bstart"][:W * (B + 1)], t["maxcount"][:4], t["buckets"][:W * B * ZERO_BYTES],
                         log2_ng=lg, kwords=4, bits=BITS, c=c, slice=slice_, staged=staged, xcd_map=xcd, big=big, zero_bytes=ZERO_BYTES)
    assert got == used, (got, used)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().view(np.uint32) if k != "buckets" else v.cpu().numpy()) for k, v in t.items()}
    sr.check(out, _expected(p, kind, c), used, ZERO_BYTES)
    return used


@pytest.mark.parametrize("p", [1, 2, 63, 64, 65, 255, 256, 257])
def test_pair_sort_small_shapes(p, dev):
    used = _run(dev, p, "mixed", 13, 3, 0, 1)
    assert used["nblk"] == -(-2 * p // SLICE) and used["W"] == 10


@pytest.mark.parametrize("xcd", [0, 1])
def test_pair_sort_nine_slices_and_a_remainder(xcd, dev):
    p = 9 * (SLICE // 2) + 77
    used = _run(dev, p, "mixed", 13, 3, 0, xcd)
    assert used["nblk"] == 10 and p % 2 == 1


@pytest.mark.parametrize("c, lg, staged", [(13, 8, 1), (13, 3, 0), (4, 0, 0)], ids=["c13-256groups-staged", "c13-8groups-direct", "c4-one-group"])
def test_pair_sort_six_thousand_pairs(c, lg, staged, dev):
    used = _run(dev, 6001, "mixed", c, lg, staged, 1)
    assert used["NG"] == 1 << lg and used["nblk"] == 24


def test_pair_sort_equal_scalars_bypass_the_lds_image(dev):
    p = 300
    _run(dev, p, "equal", 13, 3, 0, 1, big=64)
    counts = np.concatenate([s["counts"] for s in _expected(p, "equal", 13)])
    assert counts.max() >= p > 64                # every record of a half's window sits in ONE bucket, above `big`


@pytest.mark.parametrize("staged", [0, 1])
def test_even_n_under_an_odd_slice_keeps_the_scalar_kernels(staged, dev):
    """sort_by_pairs wants an even slice: 511 half scalars per block cannot be cut into pairs, and the result is the same"""
    used = _run(dev, 1000, "mixed", 13, 3, staged, 1, slice_=511)
    assert used["nblk"] == 4
