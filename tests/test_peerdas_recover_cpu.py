"""EIP-7594 recovery on the CPU: tests/recover_harness.cpp runs the host logic and the three kernel bodies of
constantine_amd/csrc/recover_host.h lane by lane, between the transforms of ntt_bodies.h, and every word is compared for equality with
tests/_recoverref.py, which restates the reference's steps (the full vanishing polynomial, no per-cell shortcut)."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import _recoverref as rr

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "constantine_amd", "csrc")
SETS = rr.index_sets()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = os.path.join(str(tmp_path_factory.mktemp("recover")), "recover_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(TESTS, "recover_harness.cpp"), "-o", exe], check=True)

    def run(cmd, indices, blobs_cells=()):
        """blobs_cells: one list of len(indices) cells per blob"""
        data = struct.pack("<2I", len(indices), len(blobs_cells)) + struct.pack("<%dQ" % len(indices), *indices)
        data += b"".join(b"".join(cells) for cells in blobs_cells)
        return subprocess.run([exe, cmd], input=data, check=True, capture_output=True).stdout
    return run


def _parse(out, B):
    assert out[0] == rr.SUCCESS and len(out) == 1 + B * (rr.EXT * 32 + 4 + rr.N * 32)
    coefs = [out[1 + b * rr.EXT * 32:1 + (b + 1) * rr.EXT * 32] for b in range(B)]
    at = 1 + B * rr.EXT * 32
    flags = list(struct.unpack("<%dI" % B, out[at:at + 4 * B]))
    at += 4 * B
    blobs = [out[at + b * rr.N * 32:at + (b + 1) * rr.N * 32] for b in range(B)]
    return coefs, flags, blobs


def _pick(cells, indices):
    return [cells[i] for i in indices]


@pytest.mark.parametrize("name", list(SETS))
def test_constants_match_the_full_vanishing_polynomial(harness, name):
    """zc and izc5 against the evaluations of the reference's Z(X) over the domain and the coset, cell by cell"""
    from tests import _nttref
    idx = SETS[name]
    out = harness("consts", idx)
    got = [int.from_bytes(out[32 * i:32 * i + 32], "little") for i in range(256)]
    z = rr.vanishing_coefficients([m for m in range(rr.CELLS) if m not in set(idx)])
    on_domain = _nttref.ntt(z, rr.R, rr.W8192, out_brp=True)
    on_coset = _nttref.ntt(z, rr.R, rr.W8192, out_brp=True, shift=rr.SHIFT)
    for k in range(rr.CELLS):
        assert set(on_domain[64 * k:64 * k + 64]) == {got[k]}, (name, k)            # Z is constant on every cell
        assert (got[k] == 0) == (k not in idx), (name, k)
        assert {v * got[128 + k] % rr.R for v in on_coset[64 * k:64 * k + 64]} == {1}, (name, k)


@pytest.mark.parametrize("name", list(SETS))
def test_recovery_matches_the_reference_steps(harness, name):
    idx = SETS[name]
    blob, cells = rr.value_cells("fixture")
    coefs, flags, blobs = _parse(harness("recover", idx, [_pick(cells, idx)]), 1)
    want, ok, want_blob = rr.recover(idx, _pick(cells, idx))
    assert ok == 1 and want_blob == blob                  # (the reference steps themselves give the blob back)
    assert coefs[0] == rr.coefficient_bytes(want) and flags == [1] and blobs[0] == blob


@pytest.mark.parametrize("kind", ["zero", "r_minus_1"])
@pytest.mark.parametrize("name", ["random_64", "all_but_0"])
def test_edge_values(harness, kind, name):
    idx = SETS[name]
    blob, cells = rr.value_cells(kind)
    coefs, flags, blobs = _parse(harness("recover", idx, [_pick(cells, idx)]), 1)
    want, ok, _ = rr.recover(idx, _pick(cells, idx))
    assert coefs[0] == rr.coefficient_bytes(want) and flags == [1] == [ok] and blobs[0] == blob


@pytest.mark.parametrize("name", ["random_65", "all_128"])
def test_inconsistent_cells_are_flagged(harness, name):
    """one element of one present cell changed: the high half is no longer zero, and equals the reference's word for word; the blob is
    that of the polynomial truncated to 4096 coefficients"""
    idx = SETS[name]
    _blob, cells = rr.value_cells("fixture")
    given = rr.altered(_pick(cells, idx), 5)
    coefs, flags, blobs = _parse(harness("recover", idx, [given]), 1)
    want, ok, want_blob = rr.recover(idx, given)
    assert ok == 0 and any(want[rr.N:])
    assert coefs[0] == rr.coefficient_bytes(want) and flags == [0] and blobs[0] == want_blob


def test_any_64_cells_define_a_polynomial(harness):
    """the same change at n = 64: another blob, and nothing to flag"""
    idx = SETS["random_64"]
    blob, cells = rr.value_cells("fixture")
    given = rr.altered(_pick(cells, idx), 5)
    coefs, flags, blobs = _parse(harness("recover", idx, [given]), 1)
    want, ok, want_blob = rr.recover(idx, given)
    assert ok == 1 and want_blob != blob
    assert coefs[0] == rr.coefficient_bytes(want) and flags == [1] and blobs[0] == want_blob


def test_rows_of_a_batch_do_not_mix(harness):
    idx = SETS["random_65"]
    kinds = ["fixture", "a", "b"]
    given = [_pick(rr.value_cells(k)[1], idx) for k in kinds]
    given[1] = rr.altered(given[1], 64)                    # the middle row inconsistent, its neighbours not
    coefs, flags, blobs = _parse(harness("recover", idx, given), 3)
    for b in range(3):
        want, ok, want_blob = rr.recover(idx, given[b])
        assert coefs[b] == rr.coefficient_bytes(want) and flags[b] == ok == (0 if b == 1 else 1) and blobs[b] == want_blob, b


@pytest.mark.parametrize("value", [rr.R, (1 << 256) - 1])
def test_scalar_out_of_range_in_the_last_cell(harness, value):
    idx = SETS["first_64"]
    given = _pick(rr.value_cells("fixture")[1], idx)
    last = bytearray(given[-1])
    last[-32:] = value.to_bytes(32, "big")
    given[-1] = bytes(last)
    assert harness("check", idx, [given]) == bytes([rr.SCALAR_TOO_LARGE])
    assert harness("recover", idx, [given]) == bytes([rr.SCALAR_TOO_LARGE])
    last[-32:] = (rr.R - 1).to_bytes(32, "big")
    given[-1] = bytes(last)
    assert harness("check", idx, [given]) == bytes([rr.SUCCESS])


def test_index_checks_in_the_reference_order(harness):
    cells = rr.value_cells("zero")[1]
    for idx, want in (
        (list(range(63)), rr.LENGTHS_MISMATCH), (list(range(128)) + [128], rr.LENGTHS_MISMATCH),
        (list(range(63)) + [128], rr.LENGTHS_MISMATCH),
        ([1, 0] + list(range(2, 63)) + [128], rr.LENGTHS_MISMATCH),          # every index is checked before the order
        ([1, 0] + list(range(2, 64)), rr.NOT_ASCENDING), ([0, 0] + list(range(2, 64)), rr.NOT_ASCENDING),
        (list(range(64)), rr.SUCCESS),
    ):
        given = [cells[i % 128] for i in idx]
        assert harness("check", idx, [given]) == bytes([want]) == bytes([rr.validate(idx, given)]), idx
    bad = [b"\xff" * 2048] + [cells[i] for i in range(2, 64)] + [cells[0]]
    assert harness("check", [1, 0] + list(range(2, 64)), [bad]) == bytes([rr.NOT_ASCENDING])   # the order before the cells' values
