"""EIP-7594 cells and cell proofs on the GPU (ctt_eth_kzg_compute_cells_and_kzg_proofs, ctt_hip_eth_kzg_compute_cells; csrc/protocols.hip
over the scalar-field NTT) against the reference's vectors and the Python restatement of tests/_peerdasref.py."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import _golden, _peerdasref as pr

pytestmark = pytest.mark.gpu

CASES = pr.fixture_cases()
VALID = [c for c in CASES if c[2] is not None]
REJECTED = [c for c in CASES if c[2] is None]


@pytest.fixture(scope="module")
def ctx():
    from constantine_amd import kzg
    c = kzg.EthereumKZGContext(open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read())
    yield c
    c.delete()


@pytest.mark.parametrize("case", VALID, ids=[c[0] for c in VALID])
def test_cells_and_proofs_match_the_reference(ctx, case):
    from constantine_amd import kzg
    name, blob, dig, proofs = case
    cells, got_proofs = kzg.compute_cells_and_kzg_proofs(ctx, blob)
    assert cells == pr.cells(blob), name                       # byte-equal to the restatement
    assert [hashlib.sha256(c).hexdigest() for c in cells] == dig, name
    assert got_proofs == proofs, name                          # all 128
    assert kzg.compute_cells(ctx, blob) == cells, name         # the cells-only symbol


def test_all_zero_quotients_give_the_neutral(ctx):
    """a constant polynomial: every cell quotient vanishes, every proof is the compressed point at infinity"""
    from constantine_amd import kzg
    blob = (5).to_bytes(32, "big") * 4096
    cells, proofs = kzg.compute_cells_and_kzg_proofs(ctx, blob)
    assert proofs == [bytes([0xC0]) + bytes(47)] * 128
    assert cells == [(5).to_bytes(32, "big") * 64] * 128


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_blobs(ctx, case):
    from constantine_amd import kzg
    name, blob, _dig, _proofs = case
    want = (kzg.cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch if len(blob) != kzg.BYTES_PER_BLOB
            else kzg.cttEthKzgStatus.cttEthKzg_ScalarLargerThanCurveOrder)
    for fn in (kzg.compute_cells, kzg.compute_cells_and_kzg_proofs, kzg.cell_quotients):
        with pytest.raises(kzg.KzgError) as e:
            fn(ctx, blob)
        assert e.value.status == want, name
    if len(blob) == kzg.BYTES_PER_BLOB:     # the C symbols themselves: the status, and sentinel-filled outputs untouched
        cells = (ctypes.c_uint8 * (128 * 2048))(*([0xA5] * (128 * 2048)))
        proofs = (ctypes.c_uint8 * (128 * 48))(*([0xA5] * (128 * 48)))
        b = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
        assert ctx.L.ctt_eth_kzg_compute_cells_and_kzg_proofs(ctx.handle, cells, proofs, b) == want.value
        assert ctx.L.ctt_hip_eth_kzg_compute_cells(ctx.handle, cells, b) == want.value
        assert bytes(cells) == b"\xA5" * (128 * 2048) and bytes(proofs) == b"\xA5" * (128 * 48)


def test_cell_quotients_kernel(ctx):
    """ctt_hip_eth_kzg_cell_quotients on valid_2 against Python, all 128 x 4096 coefficients"""
    from constantine_amd import kzg
    name, blob, _dig, _proofs = next(c for c in VALID if c[0].endswith("valid_2"))
    got = kzg.cell_quotients(ctx, blob)
    assert np.array_equal(got, pr.quotients_array(pr.coefficients(blob)))


def test_commitments_and_openings_are_unchanged_by_a_cells_call(ctx):
    from constantine_amd import kzg
    name, blob, com = next(c for c in _golden.kzg4844_raw_cases() if c[2] is not None)
    case, pblob, zb, res = next(c for c in _golden.kzg4844_proof_cases()["compute_kzg_proof"] if c[3] is not None)
    assert kzg.blob_to_kzg_commitment(ctx, blob) == com
    assert kzg.compute_kzg_proof(ctx, pblob, zb) == res
    kzg.compute_cells_and_kzg_proofs(ctx, blob)
    assert kzg.blob_to_kzg_commitment(ctx, blob) == com
    assert kzg.compute_kzg_proof(ctx, pblob, zb) == res
    assert len(kzg.last_cell_timings(ctx)) == 7
