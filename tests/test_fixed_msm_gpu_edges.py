"""The edges of the batched fixed-base G1 MSM's documented domain on the GPU, through constantine_amd.fixed.FixedBaseMsm: rows of more
than 64 partials up to the 256 of n = 65536 (the strides of the finish), flat grids past 65535 blocks, and a table of more than 2^32
words at the maximum window size c = 12 (64-bit record addresses).  Every comparison is byte equality of affine Montgomery coordinates
with oracle.cref.msm or oracle.pyoracle integers."""
import functools
import random

import numpy as np
import pytest

from oracle import cref
from oracle import pyoracle as po
from tests import _fixedref as fx

pytestmark = pytest.mark.gpu

BLS, BN = "bls12_381_g1", "bn254_snarks_g1"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _cref_row(name, scalars, pts, keep=None):
    if keep is not None:
        scalars, pts = scalars[keep], pts[keep]
    return cref.msm(name, np.ascontiguousarray(scalars), np.ascontiguousarray(pts), nthreads=8)[0]


def _assert_rows(got, want, what):
    """every row; on a mismatch the first differing row index"""
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, the first is row {bad[0]}"


def _scalar(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------
# B1: more than 64 partials per row
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _points_65536(name):
    """once per curve and process; the shapes of a curve share them (n = 16385 takes the first ones)"""
    return cref.gen_points(name, 27, 65536)


@pytest.mark.parametrize("name,n", [(BLS, 16385), (BLS, 65536), (BN, 65536)], ids=["bls-65-chunks", "bls-256-chunks", "bn254-256-chunks"])
def test_rows_of_more_than_64_partials(name, n):
    """c = 2.  n = 16385: 65 chunks, the last of one base, so lane 0 of the finish takes two partials; n = 65536: 256 chunks, four
    strides (BLS12-381: a 1.5 GiB table).  Six rows: two uniform unreduced ones, one-hot (base 256 * 200 + 17, or the last base of
    16385), one that is non-zero only in the chunks of one finish lane ({5, 69, 133, 197}, or {0, 64} of 65), one that is non-zero
    only from chunk 64 on, all zero.  Device tensors and host arrays; BN254's uniform rows also as Montgomery residues."""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    curve = po.CURVES[name]
    bits = fx.BITS[name]
    pts = _points_65536(name)[:n]
    chunks = -(-n // 256)
    assert chunks == (65 if n == 16385 else 256)
    rng = random.Random(f"B1 {name} {n}")
    uni = cref.synth_scalars(rng.getrandbits(32), 6 * n, bits).reshape(6, n, 32)
    chunk_of = np.arange(n) // 256
    coefs = np.zeros((6, n, 32), dtype=np.uint8)
    want = np.zeros((6, curve.aff_bytes), dtype=np.uint8)
    coefs[0:2] = uni[0:2]
    for k in (0, 1):
        want[k] = _cref_row(name, coefs[k], pts)
    hot = n - 1 if n == 16385 else 256 * 200 + 17
    k_hot = rng.getrandbits(bits)
    coefs[2, hot] = _scalar(k_hot)
    want[2] = np.frombuffer(curve.aff_to_bytes(curve.scalar_mul(k_hot, curve.aff_from_bytes(bytes(pts[hot])))), dtype=np.uint8)
    lane = (0, 64) if n == 16385 else (5, 69, 133, 197)
    assert all(s < chunks for s in lane) and len({s % 64 for s in lane}) == 1
    keep = np.flatnonzero(np.isin(chunk_of, lane))
    coefs[3, keep] = uni[3, keep]
    want[3] = _cref_row(name, coefs[3], pts, keep)
    keep = np.flatnonzero(chunk_of >= 64)
    assert keep.size == n - 16384
    coefs[4, keep] = uni[4, keep]
    want[4] = _cref_row(name, coefs[4], pts, keep)
    assert all(want[k].any() for k in range(5)) and not want[5].any()
    with FixedBaseMsm(name, pts, c=2) as f:
        info = f.info()
        assert (info["n"], info["c"], info["records_per_base"]) == (n, 2, 256 if name == BLS else 255)
        assert info["table_bytes"] == n * info["records_per_base"] * curve.aff_bytes
        got = f.msm_batch(torch.from_numpy(coefs).cuda())
        assert got.is_cuda
        _assert_rows(got.cpu().numpy(), want, "device tensors")
        _assert_rows(f.msm_batch(coefs), want, "host arrays")
        if name == BN:
            fr = np.stack([curve.fr_scalars_to_array([int.from_bytes(bytes(s), "little") for s in coefs[k]]) for k in (0, 1)])
            _assert_rows(f.msm_batch(torch.from_numpy(fr).cuda(), fr=True).cpu().numpy(), want[:2], "Montgomery residues")


# ---------------------------------------------------------------------------------------------
# B2: the flat grid past 65535 blocks
# ---------------------------------------------------------------------------------------------
def test_a_grid_of_70001_blocks_of_one_base():
    """n = 1, m = 70001, c = 4: row k holds scalar k mod 7 of seven small ones, the last three rows others.  7 does not divide 65536,
    so a row index cut to 16 bits lands on another element of the pattern."""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    curve = po.CURVES[BLS]
    m, period = 70001, 7
    assert m > 65536 and 65536 % period != 0
    pts = cref.gen_points(BLS, 28, 1)
    P = curve.aff_from_bytes(bytes(pts[0]))
    ks = [3, 5, 8, 13, 21, 34, 55]
    last = [89, 144, 233]
    assert len(set(ks + last)) == period + 3
    assert all(ks[k % period] != ks[(k - 65536) % period] for k in range(65536, m))
    by_k = {k: np.frombuffer(curve.aff_to_bytes(curve.scalar_mul(k, P)), dtype=np.uint8) for k in ks + last}
    row_k = [ks[k % period] for k in range(m - 3)] + last
    coefs = np.zeros((m, 1, 32), dtype=np.uint8)
    coefs[:, 0, 0] = row_k
    want = np.stack([by_k[k] for k in ks + last])[np.array([(ks + last).index(k) for k in row_k])]
    with FixedBaseMsm(BLS, pts, c=4) as f:
        _assert_rows(f.msm_batch(coefs), want, "host arrays")
        _assert_rows(f.msm_batch(torch.from_numpy(coefs).cuda()).cpu().numpy(), want, "device tensors")


def test_a_grid_of_65542_blocks_of_two_chunks():
    """n = 257 (two chunks), m = 32771, c = 4: row k is row k mod 3 of three seeded ones, the last three rows others; the rows are
    repeated on the device.  3 does not divide 32768: a block index cut to 16 bits is a row index off by 32768, another pattern row."""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    m, n, period = 32771, 257, 3
    assert 2 * m > 65536 and 32768 % period != 0
    assert all(k % period != (k - 32768) % period for k in range(32768, m))
    pts = cref.gen_points(BLS, 29, n)
    six = cref.synth_scalars(30, 6 * n, 255).reshape(6, n, 32)
    assert len({six[k].tobytes() for k in range(6)}) == 6
    six_want = np.stack([_cref_row(BLS, six[k], pts) for k in range(6)])
    assert len({six_want[k].tobytes() for k in range(6)}) == 6
    idx = np.concatenate([np.arange(m - 3) % period, [3, 4, 5]])
    coefs = torch.from_numpy(six).cuda()[torch.from_numpy(idx).cuda()]
    assert tuple(coefs.shape) == (m, n, 32)
    with FixedBaseMsm(BLS, pts, c=4) as f:
        got = f.msm_batch(coefs).cpu().numpy()
    _assert_rows(got, six_want[idx], "device tensors")


# ---------------------------------------------------------------------------------------------
# B3: a table of more than 2^32 words at the maximum window size
# ---------------------------------------------------------------------------------------------
def test_record_addresses_past_32_bits_at_c_12():
    """BLS12-381 G1, c = 12, n = 4864: 4864 * 36864 records of 24 words are 2^32 + 2^23 words, a 16.03 GiB table and 40 GiB while it
    is built.  A uniform row, a one-hot row at the last base whose digits are all non-zero and whose top digit is the largest (it reads
    the last record of the table), a one-hot row at base 0."""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    free = torch.cuda.mem_get_info()[0]
    if free < 48 << 30:
        pytest.skip(f"{free / 2**30:.1f} GiB of device memory free, 48 GiB wanted")
    curve = po.CURVES[BLS]
    n, c, rows = 4864, 12, 14 * 2048 + 8 * 1024
    assert rows == 36864 == fx.rows_per_base(255, c) and n * rows * 24 > 2**32
    assert (n - 1) * rows * 24 >= 2**32 > rows * 24            # the last base lies past 2^32 words, base 0 below
    pts = cref.gen_points(BLS, 31, n)
    lay = fx.layout(255, c)
    rng = random.Random("B3")
    off, width = lay[-1]
    k_top = (rng.getrandbits(off - 1) | ((1 << (width - 1)) - 1) << off | 1 << (off - 1))
    digits = fx.booth_digits(k_top, lay)
    assert all(digits) and digits[-1] == 1 << (width - 1)
    k_0 = rng.getrandbits(255)
    coefs = np.zeros((3, n, 32), dtype=np.uint8)
    coefs[0] = cref.synth_scalars(32, n, 255)
    coefs[1, n - 1] = _scalar(k_top)
    coefs[2, 0] = _scalar(k_0)
    want = np.stack([_cref_row(BLS, coefs[0], pts)] +
                    [np.frombuffer(curve.aff_to_bytes(curve.scalar_mul(k, curve.aff_from_bytes(bytes(pts[i])))), dtype=np.uint8)
                     for k, i in ((k_top, n - 1), (k_0, 0))])
    with FixedBaseMsm(BLS, pts, c=c) as f:
        info = f.info()
        assert (info["windows"], info["records_per_base"], info["table_bytes"]) == (22, 36864, 4864 * 36864 * 96)
        print(f"table of {info['table_bytes'] / 2**30:.2f} GiB built in {info['build_us'] / 1e3:.1f} ms")
        _assert_rows(f.msm_batch(torch.from_numpy(coefs).cuda()).cpu().numpy(), want, "device tensors")
        _assert_rows(f.msm_batch(coefs), want, "host arrays")


# ---------------------------------------------------------------------------------------------
# B4: a batch whose grid the runtime would refuse is refused as an argument
# ---------------------------------------------------------------------------------------------
def test_a_launch_of_2_pow_32_work_items_is_refused_as_an_argument():
    """n = 1, m = 2^24: m * n * 32 = 2^29 passes the size check, but 2^24 blocks of 256 lanes are 2^32 work-items in x, which the HIP
    runtime refuses as an invalid configuration (seen once on an MI355X: -3, returned after reserve() had grown the workspace by 4.5 GiB).  The call
    returns -1 before anything is reserved or launched: the coefficients' pages are never touched, the output and the free device
    memory are unchanged, and the handle serves the next call."""
    from constantine_amd import FixedBaseMsm
    torch = _torch()
    case = fx.case("T2")
    m = 1 << 24
    assert m * 1 * 32 < 2**31 and m * 1 * 256 == 2**32 and (m - 1) * 256 < 2**32
    with FixedBaseMsm(BLS, case.pts, c=4) as f:
        assert f.msm_batch(case.coefs).tobytes() == case.expect.tobytes()      # (the workspace exists)
        out = np.full((4, 96), 0xA5, dtype=np.uint8)                           # (out holds 4 rows only)
        huge = np.zeros((m, 1, 32), dtype=np.uint8)
        free = torch.cuda.mem_get_info()[0]
        assert f.L.ctt_hip_fixed_msm_batch(f.handle, 0, huge.ctypes.data, m, out.ctypes.data, 0) == -1
        assert f.L.ctt_hip_fixed_last_error() == -1
        del huge
        assert free - torch.cuda.mem_get_info()[0] < 1 << 30, "the workspace grew (3 GiB of partials, 1.5 GiB of rows)"
        assert out.tobytes() == b"\xA5" * out.nbytes
        assert f.msm_batch(case.coefs).tobytes() == case.expect.tobytes()
