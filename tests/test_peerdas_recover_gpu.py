"""EIP-7594 recovery on the GPU (libctt_msm_hip_peerdas.so: constantine_amd/csrc/recover.hip over the scalar-field NTT and the prover of
the main library) against the reference's 18 vectors and the Python restatement of the reference's steps, tests/_recoverref.py.  The
shapes are the protocol's fixed 8192 points, so the batches are what is kept small: B = 1 and B = 3."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import _golden, _recoverref as rr
from tests.test_peerdas_recover import CASES, VALID, _short, expected_status

pytestmark = pytest.mark.gpu

SETS = rr.index_sets()
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from constantine_amd import kzg
    c = kzg.EthereumKZGContext(open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read())
    yield c
    c.delete()


@pytest.fixture(scope="module")
def rec():
    from constantine_amd import peerdas
    r = peerdas.Recovery(0)
    yield r
    r.delete()


def _pick(cells, indices):
    return [cells[i] for i in indices]


def _coef_bytes(arr_row):
    return arr_row.tobytes()


@pytest.mark.parametrize("case", CASES, ids=_short)
def test_reference_vectors_through_the_reference_symbol(ctx, case):
    from constantine_amd import _lib, kzg
    name, idx, cells, want = case
    if len(idx) != len(cells) or any(len(c) != rr.CELL_BYTES for c in cells):
        with pytest.raises(ValueError):                       # the C symbol has one count and fixed-size cells: the wrapper's check
            kzg.recover_cells_and_kzg_proofs(ctx, idx, cells)
        return
    out_c = np.full(128 * 2048, SENTINEL, dtype=np.uint8)
    out_p = np.full(128 * 48, SENTINEL, dtype=np.uint8)
    ind = (ctypes.c_uint64 * max(len(idx), 1))(*idx)
    raw = np.frombuffer(b"".join(cells) or b"\0", dtype=np.uint8)
    rc = _lib.peerdas_lib().ctt_eth_kzg_recover_cells_and_kzg_proofs(ctx.handle, out_c.ctypes.data_as(ctypes.c_void_p),
                                                                   out_p.ctypes.data_as(ctypes.c_void_p), ind,
                                                                   raw.ctypes.data_as(ctypes.c_void_p), len(idx))
    if want is None:
        assert rc == expected_status(name), name
        assert bytes(out_c) == bytes([SENTINEL]) * (128 * 2048) and bytes(out_p) == bytes([SENTINEL]) * (128 * 48)
        with pytest.raises(kzg.KzgError) as e:
            kzg.recover_cells_and_kzg_proofs(ctx, idx, cells)
        assert e.value.status.value == rc
        return
    digests, proofs = want
    assert rc == 0, name
    got_c, got_p = bytes(out_c), bytes(out_p)
    assert [hashlib.sha256(got_c[2048 * k:2048 * (k + 1)]).hexdigest() for k in range(128)] == digests, name
    assert [got_p[48 * k:48 * (k + 1)] for k in range(128)] == proofs, name
    wc, wp = kzg.recover_cells_and_kzg_proofs(ctx, idx, cells)
    assert b"".join(wc) == got_c and wp == proofs
    for i, c in zip(idx, cells):
        assert wc[i] == c                                     # the given cells come back where they were


@pytest.mark.parametrize("kind,name", [("fixture", n) for n in SETS] + [(k, n) for k in ("zero", "r_minus_1") for n in ("random_64", "all_but_0")])
def test_coefficients_and_blobs_match_the_reference_steps(rec, kind, name):
    idx = SETS[name]
    blob, cells = rr.value_cells(kind)
    given = _pick(cells, idx)
    want, ok, want_blob = rr.recover(idx, given)
    coefs, flags = rec.recover_coefficients(idx, given)
    assert _coef_bytes(coefs[0]) == rr.coefficient_bytes(want) and list(flags) == [True] == [bool(ok)]
    assert rec.recover_blobs(idx, given) == (blob, True) and want_blob == blob
    ms = rec.last_timings()
    assert len(ms) == 5 and all(v >= 0 for v in ms) and ms[4] == 0


@pytest.mark.parametrize("name,flag", [("random_65", False), ("all_128", False), ("random_64", True)])
def test_inconsistent_cells(rec, name, flag):
    """one element of one present cell changed: with more than 64 cells the high half equals the reference's, word for word, and the
    flag is 0; the same change at n = 64 only defines another polynomial.  The blob is that of the truncated polynomial."""
    idx = SETS[name]
    given = rr.altered(_pick(rr.value_cells("fixture")[1], idx), 5)
    want, ok, want_blob = rr.recover(idx, given)
    assert bool(ok) == flag and any(want[rr.N:]) != flag
    coefs, flags = rec.recover_coefficients(idx, given)
    assert _coef_bytes(coefs[0]) == rr.coefficient_bytes(want) and list(flags) == [flag]
    assert rec.recover_blobs(idx, given) == (want_blob, flag)


def test_a_batch_of_three_equals_three_single_calls(rec, ctx):
    idx = SETS["random_65"]
    given = [_pick(rr.value_cells(k)[1], idx) for k in ("fixture", "a", "b")]
    given[1] = rr.altered(given[1], 64)                       # the middle row inconsistent, its neighbours not: rows must not mix
    blobs, flags = rec.recover_blobs(idx, given)
    coefs, cflags = rec.recover_coefficients(idx, given)
    assert blobs.shape == (3, 131072) and list(flags) == [True, False, True] == list(cflags)
    for b in range(3):
        one_blob, one_flag = rec.recover_blobs(idx, given[b])
        assert blobs[b].tobytes() == one_blob == rr.recover(idx, given[b])[2] and one_flag == flags[b], b
        assert coefs[b].tobytes() == rec.recover_coefficients(idx, given[b])[0][0].tobytes(), b
    cells3, proofs3 = rec.recover_cells_and_kzg_proofs(ctx, idx, given)
    assert cells3.shape == (3, 128, 2048) and proofs3.shape == (3, 128, 48)
    for b in range(3):
        c1, p1 = rec.recover_cells_and_kzg_proofs(ctx, idx, given[b])
        assert cells3[b].tobytes() == b"".join(c1) and proofs3[b].tobytes() == b"".join(p1), b
    assert rec.last_timings()[4] > 0


def test_one_blob_through_the_batch_symbol(rec, ctx):
    from constantine_amd import kzg
    name, idx, cells, (digests, proofs) = VALID[0]
    got_c, got_p = rec.recover_cells_and_kzg_proofs(ctx, idx, np.frombuffer(b"".join(cells), dtype=np.uint8).reshape(1, len(idx), 2048))
    assert got_c.shape == (1, 128, 2048)
    assert [hashlib.sha256(got_c[0, k].tobytes()).hexdigest() for k in range(128)] == digests
    assert [got_p[0, k].tobytes() for k in range(128)] == proofs
    assert (b"".join(kzg.recover_cells_and_kzg_proofs(ctx, idx, cells)[0])) == got_c.tobytes()


def test_a_call_succeeds_right_after_a_refused_one(rec):
    from constantine_amd import kzg
    idx = SETS["first_64"]
    blob, cells = rr.value_cells("fixture")
    given = _pick(cells, idx)
    bad = given[:63] + [given[63][:-32] + rr.R.to_bytes(32, "big")]
    for wrong_idx, wrong_cells, status in ((idx, bad, rr.SCALAR_TOO_LARGE), ([1, 0] + idx[2:], given, rr.NOT_ASCENDING),
                                           (idx[:63] + [128], given, rr.LENGTHS_MISMATCH)):
        with pytest.raises(kzg.KzgError) as e:
            rec.recover_blobs(wrong_idx, wrong_cells)
        assert e.value.status.value == status
        assert rec.recover_blobs(idx, given) == (blob, True)


def test_batch_bounds(rec, ctx):
    """B = 4097 is refused and B = 0 succeeds, both before anything is read or written"""
    L = rec.L
    idx = (ctypes.c_uint64 * 64)(*range(64))
    cells = np.zeros(64 * 2048, dtype=np.uint8)               # (never read: the bound is checked first, and B = 0 has no cells)
    blobs = np.full(131072, SENTINEL, dtype=np.uint8)
    flags = np.full(8, SENTINEL, dtype=np.uint8)
    out_c = np.full(128 * 2048, SENTINEL, dtype=np.uint8)
    out_p = np.full(128 * 48, SENTINEL, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for B, want in ((4097, rr.LENGTHS_MISMATCH), (0, rr.SUCCESS)):
        assert L.ctt_hip_peerdas_recover_blobs(rec.handle, vp(blobs), vp(flags), idx, vp(cells), 64, B) == want
        assert L.ctt_hip_peerdas_recover_coefficients(rec.handle, vp(blobs), vp(flags), idx, vp(cells), 64, B) == want
        assert L.ctt_hip_eth_kzg_recover_cells_and_kzg_proofs_batch(rec.handle, ctx.handle, vp(out_c), vp(out_p), idx, vp(cells), 64, B) == want
    for a in (blobs, flags, out_c, out_p):
        assert set(a.tolist()) == {SENTINEL}


def test_the_kzg_context_is_left_as_it_was(rec, ctx):
    from constantine_amd import kzg
    name, idx, cells, (digests, proofs) = VALID[1]
    blob = rr.value_cells("fixture")[0]
    before = kzg.compute_cells_and_kzg_proofs(ctx, blob)
    path = kzg.last_cell_proof_path(ctx)[0]
    got = rec.recover_cells_and_kzg_proofs(ctx, idx, cells)
    assert got[1] == proofs
    kzg.recover_cells_and_kzg_proofs(ctx, idx, cells)
    assert kzg.last_cell_proof_path(ctx)[0] == path
    assert kzg.compute_cells_and_kzg_proofs(ctx, blob) == before
    assert kzg.last_cell_proof_path(ctx)[0] == path
    name0, blob0, com = next(c for c in _golden.kzg4844_raw_cases() if c[2] is not None)
    assert kzg.blob_to_kzg_commitment(ctx, blob0) == com
