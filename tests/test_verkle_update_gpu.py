"""Sparse batched Verkle updates on the GPU (ctt_hip_verkle_update_batch, VerkleCrs.update; csrc/verkle.hip k_vk_update) against the
Python-integer oracle tests/_banderwagon.py.

Most rows use the 256 synthetic points [s_j]G of known s_j, so that an expected row is one scalar multiplication of G: the logarithm of
base_k + sum delta_e * P_idx[e] is b_k + sum delta_e * s_idx[e].  Expected values never come from the code under test; the comparison
with VerkleCrs.commit at the end is a cross-check only."""
import ctypes
import random

import numpy as np
import pytest

from tests import _banderwagon as bw
from tests import _verkle
from tests._verkle import check_outputs, fr_from, log_point as _log_point, map_fr, prj_bytes as _prj_bytes, pts_array as _pts

pytestmark = pytest.mark.gpu
TOP = (1 << 253) - 1
NEUTRAL_PRJ = bw.fp_bytes(0) + bw.fp_bytes(1) + bw.fp_bytes(1)
VP = ctypes.c_void_p
ALL = ("prj", "ser", "fr", "dfr")
WIDTHS = (96, 32, 32, 32)
SEED = 5151


@pytest.fixture(scope="module")
def torch_cuda():
    return _verkle.torch_with_gpu()


@pytest.fixture(scope="module")
def dev(torch_cuda):
    yield from _verkle.device_msm()


@pytest.fixture(scope="module")
def synth_crs(dev, torch_cuda):
    """256 synthetic points [s_j]G of known s_j, the table made from the device tensor"""
    yield from _verkle.synth_crs(dev, torch_cuda, SEED)


def _csr(rows, fr=False):
    """rows [[(index, delta), ...], ...] -> deltas (E, 32), idx (E,), row_ptr (m + 1,)"""
    enc = bw.fr_bytes if fr else bw.big_bytes
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.array([i for r in rows for i, _ in r], dtype=np.int64)
    deltas = np.frombuffer(b"".join(enc(d) for r in rows for _, d in r), dtype=np.uint8).reshape(-1, 32).copy()
    return deltas, idx, row_ptr


def _bases(points, rng):
    return np.frombuffer(b"".join(_prj_bytes(p, rng.randrange(1, bw.P)) for p in points), dtype=np.uint8).reshape(-1, 96).copy()


def _check(out, i, pt, base_pt=bw.O):
    check_outputs(out, i, pt)
    dfr = bytes(out["dfr"][i])
    assert int.from_bytes(dfr, "little") < bw.R and fr_from(dfr) == (map_fr(pt) - map_fr(base_pt)) % bw.R, i


def _synth_case(logs, cnts, rng):
    """rows of the given lengths over the synthetic CRS with random bases: (rows, base points, expected points)"""
    rows = [[(rng.randrange(256), rng.randrange(bw.R)) for _ in range(cnt)] for cnt in cnts]
    blogs = [rng.randrange(bw.R) for _ in cnts]
    bases = [_log_point(b) for b in blogs]
    expect = [_log_point(b + sum(d * logs[i] for i, d in row)) for b, row in zip(blogs, rows)]
    return rows, bases, expect


def _to_cuda(torch, a):
    return torch.from_numpy(a).cuda()


# --- 1. row lengths -------------------------------------------------------------------------------------------------------------------
def test_row_lengths(synth_crs):
    """cnt * 26 windows below, on and above multiples of the 64 lanes of a row; the longest row is a whole node"""
    _, logs, crs = synth_crs
    rng = random.Random(1)
    rows, bases, expect = _synth_case(logs, [0, 1, 2, 25, 26, 27, 63, 64, 65, 256], rng)
    deltas, idx, row_ptr = _csr(rows)
    out = crs.update(deltas, idx, row_ptr, base=_bases(bases, rng), want=ALL)
    for i, (pt, b) in enumerate(zip(expect, bases)):
        _check(out, i, pt, b)
    assert expect[0] == bases[0]
    frd, _, _ = _csr(rows, fr=True)
    out2 = crs.update(frd, idx, row_ptr, base=_bases(bases, rng), fr_coefs=True, want=ALL)
    for key in ALL:
        assert bytes(out2[key]) == bytes(out[key]), key


# --- 2. rows per workgroup, host and device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 257])
def test_rows_per_workgroup(torch_cuda, synth_crs, m):
    _, logs, crs = synth_crs
    rng = random.Random(20 + m)
    rows, bases, expect = _synth_case(logs, [3] * m, rng)
    deltas, idx, row_ptr = _csr(rows)
    base = _bases(bases, rng)
    out = crs.update(deltas, idx, row_ptr, base=base, want=ALL)
    for i, (pt, b) in enumerate(zip(expect, bases)):
        _check(out, i, pt, b)
    d_out = crs.update(_to_cuda(torch_cuda, deltas), idx, row_ptr, base=_to_cuda(torch_cuda, base), want=ALL)
    for key in ALL:
        assert d_out[key].is_cuda and bytes(d_out[key].cpu().numpy()) == bytes(out[key]), key


def test_host_and_device_calls_agree(torch_cuda, synth_crs):
    _, logs, crs = synth_crs
    rng = random.Random(3)
    rows, bases, expect = _synth_case(logs, [4, 0, 31, 1, 2, 70, 5], rng)
    base = _bases(bases, rng)
    for fr in (False, True):
        deltas, idx, row_ptr = _csr(rows, fr)
        for b_host, b_dev in ((base, _to_cuda(torch_cuda, base)), (None, None)):
            host = crs.update(deltas, idx, row_ptr, base=b_host, fr_coefs=fr, want=ALL)
            devo = crs.update(_to_cuda(torch_cuda, deltas), list(idx), tuple(row_ptr), base=b_dev, fr_coefs=fr, want=ALL)
            for key in ALL:
                assert bytes(devo[key].cpu().numpy()) == bytes(host[key]), (fr, key)
            if b_host is not None:
                for i, (pt, b) in enumerate(zip(expect, bases)):
                    _check(host, i, pt, b)


# --- 3. window widths and digit edges -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def digit_cases():
    rng = random.Random(4)
    pts = [bw.msm_fast([rng.randrange(1, bw.R)], [bw.G]) for _ in range(15)] + [bw.add(bw.mul(rng.randrange(1, bw.R), bw.G), bw.T2)]
    scalars = [0, 1, bw.R - 1, bw.R, bw.R + 1, TOP, int.from_bytes(b"\x80" * 32, "little") & TOP, rng.randrange(1 << 253)]
    rows = [[(i, k)] for k in scalars for i in (5, 15)] + [[(15, scalars[7]), (0, TOP), (15, 1)]]
    expect = [bw.msm_fast([k % (2 * bw.R) for _, k in row], [pts[i] for i, _ in row]) for row in rows]
    frrows = [[(i, k % bw.R) for i, k in row] for row in rows]
    frexpect = [bw.msm_fast([k for _, k in row], [pts[i] for i, _ in row]) for row in frrows]
    return pts, rows, expect, frrows, frexpect


@pytest.mark.parametrize("c", [2, 5, 10])
def test_window_widths(dev, digit_cases, c):
    from constantine_amd import VerkleCrs
    pts, rows, expect, frrows, frexpect = digit_cases
    with VerkleCrs(_pts(pts), ctx=dev.ctx, window_bits=c) as crs:
        assert crs.window_bits == c
        out = crs.update(*_csr(rows), want=ALL)
        for i, pt in enumerate(expect):
            _check(out, i, pt)
        out = crs.update(*_csr(frrows, fr=True), fr_coefs=True, want=ALL)
        for i, pt in enumerate(frexpect):
            _check(out, i, pt)


# --- 4. special cases -----------------------------------------------------------------------------------------------------------------
def test_special_cases(torch_cuda, synth_crs):
    _, logs, crs = synth_crs
    rng = random.Random(5)
    d1, d2, b = (rng.randrange(1, bw.R) for _ in range(3))
    B = _log_point(b)
    rows = [[(7, d1), (7, d2)],                                        # a duplicate index: both count
            [(9, d1), (200, d2), (9, bw.R - d1), (200, bw.R - d2)],    # cancelling entries: the base comes back
            [],
            [(255, d2)]]
    neg_sum = _log_point(-(d2 * logs[255]))
    bases = [B, B, B, neg_sum]
    expect = [_log_point(b + (d1 + d2) * logs[7]), B, B, bw.O]
    deltas, idx, row_ptr = _csr(rows)
    out = crs.update(deltas, idx, row_ptr, base=_bases(bases, rng), want=ALL)
    for i, (pt, bp) in enumerate(zip(expect, bases)):
        _check(out, i, pt, bp)
    assert bytes(out["dfr"][1]) == bytes(32) and bytes(out["dfr"][2]) == bytes(32)
    assert bytes(out["prj"][3]) == NEUTRAL_PRJ and bytes(out["ser"][3]) == bytes(32) and bytes(out["fr"][3]) == bytes(32)
    # no base: the neutral -- and the neutral as a base, (0, z, z)
    none = crs.update(deltas, idx, row_ptr, want=ALL)
    neutral = crs.update(deltas, idx, row_ptr, base=_bases([bw.O] * 4, rng), want=ALL)
    for i, t in enumerate([(d1 + d2) * logs[7], 0, 0, d2 * logs[255]]):
        _check(none, i, _log_point(t))
        _check(neutral, i, _log_point(t))
    assert bytes(none["prj"][1]) == bytes(none["prj"][2]) == NEUTRAL_PRJ and bytes(none["dfr"]) == bytes(none["fr"])
    # all rows empty: with bases they are normalised and mapped, without any the result is the neutral; tensors of no entries too
    empty = np.zeros((0, 32), np.uint8)
    out = crs.update(empty, [], [0, 0, 0, 0], base=_bases([B, bw.O, neg_sum], rng), want=ALL)
    for i, pt in enumerate([B, bw.O, neg_sum]):
        _check(out, i, pt, pt)
    out = crs.update(empty, [], [0, 0, 0], want=ALL)
    assert bytes(out["prj"]) == NEUTRAL_PRJ * 2 and bytes(out["ser"]) == bytes(64) and bytes(out["fr"]) == bytes(out["dfr"]) == bytes(64)
    out = crs.update(_to_cuda(torch_cuda, empty), [], [0, 0, 0], want=("prj",))
    assert list(out) == ["prj"] and bytes(out["prj"].cpu().numpy()) == NEUTRAL_PRJ * 2
    out = crs.update(empty, [], [0])
    assert all(out[k].shape[0] == 0 for k in ("prj", "ser", "fr"))


# --- 5. output subsets ----------------------------------------------------------------------------------------------------------------
def test_output_subsets_leave_the_rest_untouched(torch_cuda, dev, synth_crs):
    from constantine_amd import _lib
    L = _lib.lib()
    _, logs, crs = synth_crs
    rng = random.Random(6)
    m = 9
    rows, bases, expect = _synth_case(logs, [2, 0, 5, 1, 1, 3, 40, 2, 2], rng)
    deltas, idx, row_ptr = _csr(rows)
    base = _bases(bases, rng)
    full = crs.update(deltas, idx, row_ptr, base=base, want=ALL)
    for i, (pt, b) in enumerate(zip(expect, bases)):
        _check(full, i, pt, b)
    nobase = crs.update(deltas, idx, row_ptr, want=ALL)
    idx8, rp32 = idx.astype(np.uint8), row_ptr.astype(np.uint32)
    d_deltas, d_base = _to_cuda(torch_cuda, deltas), _to_cuda(torch_cuda, base)
    for with_base in (True, False):
        ref = full if with_base else nobase
        for mask in range(1, 16):
            host = [np.full((m, w), 0xC3, np.uint8) for w in WIDTHS]
            devb = [torch_cuda.full((m, w), 0xC3, dtype=torch_cuda.uint8, device="cuda") for w in WIDTHS]
            torch_cuda.cuda.synchronize()
            hp = [a.ctypes.data_as(VP) if mask >> i & 1 else None for i, a in enumerate(host)]
            dp = [VP(t.data_ptr()) if mask >> i & 1 else None for i, t in enumerate(devb)]
            assert L.ctt_hip_verkle_update_batch(dev.ctx, crs.handle, 0, hp[0], hp[1], hp[2], hp[3], base.ctypes.data_as(VP) if with_base else None,
                                                 rp32.ctypes.data_as(VP), idx8.ctypes.data_as(VP), deltas.ctypes.data_as(VP), m, 0) == 0
            assert L.ctt_hip_verkle_update_batch(dev.ctx, crs.handle, 0, dp[0], dp[1], dp[2], dp[3], VP(d_base.data_ptr()) if with_base else None,
                                                 rp32.ctypes.data_as(VP), idx8.ctypes.data_as(VP), VP(d_deltas.data_ptr()), m, 1) == 0
            for i, key in enumerate(ALL):
                want = bytes(ref[key]) if mask >> i & 1 else bytes([0xC3]) * (m * WIDTHS[i])
                assert bytes(host[i]) == want and bytes(devb[i].cpu().numpy()) == want, (with_base, mask, key)


# --- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dev, synth_crs):
    from constantine_amd import VerkleCrs, _lib
    L = _lib.lib()
    d_pts, _, crs = synth_crs
    outs = [np.full((2, w), 0xAB, np.uint8) for w in WIDTHS]
    o = [a.ctypes.data_as(VP) for a in outs]
    rp = np.array([0, 1, 2], np.uint32)
    idx = np.array([3, 4], np.uint8)
    deltas = np.full((2, 32), 1, np.uint8)

    def call(ctx, handle, kind, outp, row_ptr, ix, m=2):
        return L.ctt_hip_verkle_update_batch(ctx, handle, kind, outp[0], outp[1], outp[2], outp[3], None, row_ptr.ctypes.data_as(VP),
                                             ix.ctypes.data_as(VP), deltas.ctypes.data_as(VP), m, 0)
    other = L.ctt_hip_msm_ctx_create(0)
    try:
        assert call(other, crs.handle, 0, o, rp, idx) == -1                              # a crs of another context
    finally:
        L.ctt_hip_msm_ctx_destroy(other)
    assert call(dev.ctx, None, 0, o, rp, idx) == -1
    assert call(dev.ctx, crs.handle, 0, [None] * 4, rp, idx) == -1                       # all outputs NULL
    assert call(dev.ctx, crs.handle, 2, o, rp, idx) == -1                                # coef_kind
    assert call(dev.ctx, crs.handle, 0, o, np.array([0, 2, 1], np.uint32), idx) == -1    # a decreasing row_ptr
    assert L.ctt_hip_last_error() == -1
    assert call(dev.ctx, crs.handle, 0, o, np.array([1, 1, 2], np.uint32), idx) == -1    # row_ptr[0] != 0
    with VerkleCrs(d_pts[:7].cpu().numpy(), ctx=dev.ctx) as small:
        assert call(dev.ctx, small.handle, 0, o, rp, np.array([6, 7], np.uint8)) == -1   # idx[e] = n
        assert L.ctt_hip_last_error() == -1
        assert call(dev.ctx, small.handle, 0, o, rp, np.array([6, 7], np.uint8), m=0) == 0   # m = 0 writes nothing
        assert all(bytes(a) == bytes([0xAB]) * a.size for a in outs)
        assert call(dev.ctx, small.handle, 0, o, rp, np.array([6, 0], np.uint8)) == 0    # (the same call with legal indices goes through)
    assert all(bytes(a) != bytes([0xAB]) * a.size for a in outs)


# --- 7. the dense kernel agrees -------------------------------------------------------------------------------------------------------
def test_update_of_a_commitment_equals_the_commitment_of_the_new_row(synth_crs):
    _, logs, crs = synth_crs
    rng = random.Random(7)
    old = [[rng.randrange(bw.R) for _ in range(256)] for _ in range(3)]
    changed = [[5], sorted(rng.sample(range(256), 4)), list(range(256))]
    new = [list(r) for r in old]
    rows = []
    for k in range(3):
        for i in changed[k]:
            new[k][i] = rng.randrange(bw.R)
        rows.append([(i, (new[k][i] - old[k][i]) % bw.R) for i in changed[k]])
    enc = lambda rs: np.frombuffer(b"".join(bw.big_bytes(v) for r in rs for v in r), dtype=np.uint8).reshape(3, 256, 32).copy()
    c_old, c_new = crs.commit(enc(old)), crs.commit(enc(new))
    out = crs.update(*_csr(rows), base=c_old["prj"], want=ALL)
    assert bytes(out["prj"]) == bytes(c_new["prj"]) and bytes(out["ser"]) == bytes(c_new["ser"]) and bytes(out["fr"]) == bytes(c_new["fr"])
    for k in range(3):
        assert fr_from(bytes(out["dfr"][k])) == (fr_from(bytes(c_new["fr"][k])) - fr_from(bytes(c_old["fr"][k]))) % bw.R
    assert bytes(out["prj"][0]) == _prj_bytes(_log_point(sum(v * s for v, s in zip(new[0], logs))))     # (and the oracle, for one row)


# --- 8. two levels of a tree, chained on the device -----------------------------------------------------------------------------------
def test_two_levels_chained_on_the_device(torch_cuda, synth_crs):
    _, logs, crs = synth_crs
    rng = random.Random(8)
    rows, leaf_old, leaf_new = _synth_case(logs, [2, 5, 1, 3], rng)
    deltas, idx, row_ptr = _csr(rows)
    leaves = crs.update(_to_cuda(torch_cuda, deltas), idx, row_ptr, base=_to_cuda(torch_cuda, _bases(leaf_old, rng)), want=("prj", "dfr"))
    assert leaves["dfr"].is_cuda
    slots = [3, 77, 200, 255]
    p_log = rng.randrange(bw.R)
    parent_old = _log_point(p_log)
    parent = crs.update(leaves["dfr"], slots, [0, 4], base=_to_cuda(torch_cuda, _bases([parent_old], rng)), fr_coefs=True, want=ALL)
    dfr = [(map_fr(n) - map_fr(o)) % bw.R for n, o in zip(leaf_new, leaf_old)]
    expect = _log_point(p_log + sum(d * logs[s] for d, s in zip(dfr, slots)))
    host = {k: v.cpu().numpy() for k, v in parent.items()}
    _check(host, 0, expect, parent_old)
    for i, pt in enumerate(leaf_new):
        assert bytes(leaves["prj"][i].cpu().numpy()) == _prj_bytes(pt), i


# --- 9. coexistence with MSM tickets --------------------------------------------------------------------------------------------------
def test_update_between_outstanding_msm_tickets(torch_cuda, dev, synth_crs):
    d_pts, logs, crs = synth_crs
    rng = random.Random(9)
    ks = [[rng.randrange(1 << 253) for _ in range(256)] for _ in range(2)]
    big = [_to_cuda(torch_cuda, np.frombuffer(b"".join(bw.big_bytes(k) for k in row), dtype=np.uint8).reshape(256, 32).copy()) for row in ks]
    expect = [_log_point(sum(k * s for k, s in zip(row, logs))) for row in ks]
    rows, bases, uexpect = _synth_case(logs, [3, 30, 0, 2, 1], rng)
    deltas, idx, row_ptr = _csr(rows)
    base = _bases(bases, rng)
    t0 = dev.submit("banderwagon", big[0], d_pts, 256)
    t1 = dev.submit("banderwagon", big[1], d_pts, 256)
    out = crs.update(deltas, idx, row_ptr, base=base, want=ALL)
    r1, r0 = dev.finish(t1, coord="prj"), dev.finish(t0, coord="prj")
    assert bytes(r0) == _prj_bytes(expect[0]) and bytes(r1) == _prj_bytes(expect[1])
    for i, (pt, b) in enumerate(zip(uexpect, bases)):
        _check(out, i, pt, b)
