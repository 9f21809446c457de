"""The EIP-7594 cell proofs through the batched fixed-base MSM (csrc/fixed.hip; kzg_cells in csrc/protocols.hip): the reference's
vectors on the table path, the loop of 128 MSMs (CTT_HIP_CELL_PROOFS=loop at context creation) byte for byte beside it, and what
ctt_hip_eth_kzg_last_cell_timings reports about the path with cap >= 9."""
import os

import pytest

from tests import _golden, _peerdasref as pr

pytestmark = pytest.mark.gpu

VALID = [c for c in pr.fixture_cases() if c[2] is not None]


def _srs():
    return open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read()


@pytest.fixture(scope="module")
def contexts():
    """(table context, loop context, path and build ms of the table context's first and second proof call)"""
    from constantine_amd import kzg
    assert "CTT_HIP_CELL_PROOFS" not in os.environ and "CTT_HIP_CELL_PROOFS_C" not in os.environ
    table = kzg.EthereumKZGContext(_srs())
    os.environ["CTT_HIP_CELL_PROOFS"] = "loop"
    try:
        loop = kzg.EthereumKZGContext(_srs())
    finally:
        del os.environ["CTT_HIP_CELL_PROOFS"]
    blob = VALID[0][1]
    calls = []
    for _ in range(2):
        kzg.compute_cells_and_kzg_proofs(table, blob)
        calls.append(kzg.last_cell_proof_path(table))
    yield table, loop, calls
    table.delete()
    loop.delete()


def test_the_table_is_built_by_the_first_proof_call_only(contexts):
    _table, _loop, calls = contexts
    assert calls[0][0] == "table" and calls[0][1] > 0
    assert calls[1] == ("table", 0.0)


def test_the_valid_vectors_hold_on_the_table_path_and_the_loop_gives_the_same_bytes(contexts):
    from constantine_amd import kzg
    table, loop, _calls = contexts
    assert len(VALID) == 7
    for name, blob, _dig, proofs in VALID:
        cells, got = kzg.compute_cells_and_kzg_proofs(table, blob)
        assert kzg.last_cell_proof_path(table) == ("table", 0.0), name
        assert got == proofs, name
        cells_l, got_l = kzg.compute_cells_and_kzg_proofs(loop, blob)
        assert kzg.last_cell_proof_path(loop) == ("loop", 0.0), name
        assert got_l == got and cells_l == cells, name
        assert len(kzg.last_cell_timings(table)) == 7


def test_all_zero_quotients_give_128_neutral_proofs_on_the_table_path(contexts):
    from constantine_amd import kzg
    table, _loop, _calls = contexts
    _cells, proofs = kzg.compute_cells_and_kzg_proofs(table, (5).to_bytes(32, "big") * 4096)
    assert kzg.last_cell_proof_path(table)[0] == "table"
    assert proofs == [bytes([0xC0]) + bytes(47)] * 128


def test_commitments_and_openings_are_unchanged_after_a_proof_call(contexts):
    from constantine_amd import kzg
    table, _loop, _calls = contexts
    name, blob, com = next(c for c in _golden.kzg4844_raw_cases() if c[2] is not None)
    case, pblob, zb, res = next(c for c in _golden.kzg4844_proof_cases()["compute_kzg_proof"] if c[3] is not None)
    kzg.compute_cells_and_kzg_proofs(table, blob)
    assert kzg.last_cell_proof_path(table)[0] == "table"
    assert kzg.blob_to_kzg_commitment(table, blob) == com
    assert kzg.compute_kzg_proof(table, pblob, zb) == res
    assert kzg.compute_cells(table, blob) == pr.cells(blob)


def test_a_window_size_out_of_range_never_refuses_a_proof_call(contexts):
    """CTT_HIP_CELL_PROOFS_C=13 is no window size: the context takes the default and serves the call on the table path"""
    from constantine_amd import kzg
    os.environ["CTT_HIP_CELL_PROOFS_C"] = "13"
    try:
        ctx = kzg.EthereumKZGContext(_srs())
    finally:
        del os.environ["CTT_HIP_CELL_PROOFS_C"]
    try:
        name, blob, _dig, proofs = VALID[1]
        _cells, got = kzg.compute_cells_and_kzg_proofs(ctx, blob)
        assert got == proofs
        assert kzg.last_cell_proof_path(ctx)[0] == "table"
    finally:
        ctx.delete()
