"""EIP-7594 recover_cells_and_kzg_proofs without a GPU: the reference's 18 vectors (tests/golden/peerdas_recover.json) through the
Python statement of the validation and of the reference's recovery steps (tests/_recoverref.py), and the Python wrapper's argument
checks.  The GPU path runs the same vectors in tests/test_peerdas_recover_gpu.py."""
import hashlib

import pytest

from tests import _recoverref as rr

CASES = rr.fixture_cases()
VALID = [c for c in CASES if c[3] is not None]
COUNT_MISMATCH = [c for c in CASES if len(c[1]) != len(c[2])]
WRONG_LENGTH = [c for c in CASES if len(c[1]) == len(c[2]) and any(len(x) != rr.CELL_BYTES for x in c[2])]
REJECTED = [c for c in CASES if c[3] is None and c not in COUNT_MISMATCH and c not in WRONG_LENGTH]


def _short(case):
    return case[0].replace("recover_cells_and_kzg_proofs_case_", "")


def expected_status(name):
    """the reference's status of a rejected vector, by what the vector's name says is wrong with it"""
    if "shuffled" in name or "duplicate" in name:
        return rr.NOT_ASCENDING
    if "invalid_cell_index" in name or "more_than_half_missing" in name or "all_cells_are_missing" in name or "more_cells_than_cells_per_ext_blob" in name:
        return rr.LENGTHS_MISMATCH
    assert "invalid_cell_" in name
    return rr.SCALAR_TOO_LARGE


def test_the_fixture_is_the_reference_s_18_vectors():
    assert len(CASES) == 18 and len(VALID) == 4 and len(COUNT_MISMATCH) == 2 and len(WRONG_LENGTH) == 2 and len(REJECTED) == 10


@pytest.mark.parametrize("case", REJECTED, ids=_short)
def test_statuses_of_the_rejected_vectors(case):
    name, idx, cells, _want = case
    assert rr.validate(idx, cells) == expected_status(name) != rr.SUCCESS


@pytest.mark.parametrize("case", VALID, ids=_short)
def test_valid_vectors_recover_the_blob(case):
    """the reference's steps give the blob's coefficients with a zero high half, and the blob gives back the expected cells (the proofs
    are the fixture's: they are not recomputed here)"""
    from tests import _peerdasref as pr
    name, idx, cells, (digests, proofs) = case
    assert rr.validate(idx, cells) == rr.SUCCESS
    coefs, ok, blob = rr.recover(idx, cells)
    assert ok == 1 and not any(coefs[rr.N:])
    assert coefs[:rr.N] == pr.coefficients(blob)
    assert [hashlib.sha256(c).hexdigest() for c in rr.extended_cells(blob)] == digests
    assert len(proofs) == 128 and all(len(p) == 48 for p in proofs)


@pytest.mark.parametrize("case", COUNT_MISMATCH + WRONG_LENGTH, ids=_short)
def test_the_wrapper_refuses_what_the_c_signature_cannot_express(case):
    """different counts of cells and indices, a cell of 2047 or 2049 bytes: ValueError before any library call"""
    from constantine_amd import kzg, peerdas
    _name, idx, cells, _want = case
    with pytest.raises(ValueError) as e:
        peerdas.pack_cells(idx, cells)
    assert not isinstance(e.value, kzg.KzgError)
    with pytest.raises(ValueError):
        kzg.recover_cells_and_kzg_proofs(None, idx, cells)


def test_pack_cells_shapes():
    import numpy as np
    from constantine_amd import peerdas
    cells = [bytes([k]) * rr.CELL_BYTES for k in range(64)]
    idx, arr, batched = peerdas.pack_cells(range(64), cells)
    assert idx.dtype == np.uint64 and arr.shape == (1, 64, rr.CELL_BYTES) and not batched and arr[0, 5, 0] == 5
    idx, arr, batched = peerdas.pack_cells(range(64), [cells, cells, cells])
    assert arr.shape == (3, 64, rr.CELL_BYTES) and batched
    idx, arr, batched = peerdas.pack_cells(range(64), np.zeros((2, 64, rr.CELL_BYTES), dtype=np.uint8))
    assert arr.shape == (2, 64, rr.CELL_BYTES) and batched
    with pytest.raises(ValueError):
        peerdas.pack_cells(range(64), np.zeros((2, 65, rr.CELL_BYTES), dtype=np.uint8))
