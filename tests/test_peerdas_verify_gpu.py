"""EIP-7594 batch verification on the GPU (libctt_msm_hip_peerdas_verify.so: constantine_amd/csrc/verify.hip over the NTT, the subgroup
check and the MSM pipeline of the main library, the pairing on the host) against the reference's 32 vectors and tests/_verifyref.py.
Every batch goes through lincombs -- the challenge and both sides of the pairing equation byte for byte -- and through verify.  All
inputs are host arrays, assembled from the golden blobs, commitments and proofs (blobs 0, 1 and 5 of the seven are constant polynomials,
with neutral proofs: the batches below are built on the others)."""
import os

import pytest

from tests import _golden, _verifyref as vr

pytestmark = pytest.mark.gpu

CASES = vr.verify_cases()
R, P = vr.R, vr.P


@pytest.fixture(scope="module")
def ver():
    from constantine_amd import peerdas
    raw = vr.srs_bytes()
    v = peerdas.Verifier(0, g1_monomial=raw[:64 * 48], g2_tau64=raw[64 * 48:])
    yield v
    v.delete()


def check(ver, coms, idx, cells, proofs, rnd=None):
    """lincombs and verify against the Python reference; -> the reference's result"""
    from constantine_amd import kzg
    ref = vr.verify(coms, idx, cells, proofs, rnd)
    if ref.verdict is None:
        for call in (ver.lincombs, ver.verify):
            with pytest.raises(kzg.KzgError) as e:
                call(coms, idx, cells, proofs, rnd)
            assert e.value.status.value == ref.status
        return ref
    ll, rl, r = ver.lincombs(coms, idx, cells, proofs, rnd)
    if len(idx) == 0:
        assert (ll, rl, r) == (None, None, None)
    else:
        assert r == ref.r and ll == ref.LL and rl == ref.RL
    assert ver.verify(coms, idx, cells, proofs, rnd) is ref.verdict
    ms = ver.last_timings()
    assert len(ms) == 6 and all(v >= 0 for v in ms)
    return ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_reference_vectors(ver, case):
    name, coms, idx, cells, proofs, want = case
    fits = len(coms) == len(idx) == len(cells) == len(proofs) and all(len(c) == 48 for c in coms + proofs) and all(len(c) == 2048 for c in cells)
    if not fits:
        assert want is None and vr.verify(coms, idx, cells, proofs).status == vr.LENGTHS_MISMATCH
        for call in (ver.lincombs, ver.verify):
            with pytest.raises(ValueError):                   # the C symbol has one count and fixed-size items: the wrapper's check
                call(coms, idx, cells, proofs)
        return
    assert check(ver, coms, idx, cells, proofs).verdict is want


def test_empty_batch_and_one_cell(ver):
    assert check(ver, [], [], [], []).verdict is True
    assert check(ver, *vr.batch([2], [77])).verdict is True


def test_two_cells_of_one_column_from_two_blobs(ver):
    assert check(ver, *vr.batch([2, 3], [64])).verdict is True


def test_one_cell_three_times(ver):
    coms, idx, cells, proofs = vr.batch([4], [9])
    assert check(ver, coms * 3, idx * 3, cells * 3, proofs * 3).verdict is True


def test_not_sorted(ver):
    coms, idx, cells, proofs = vr.batch([4, 6], [127, 3, 64, 0, 3])
    assert check(ver, coms, idx, cells, proofs).verdict is True


def _batch_257():
    """two whole blobs and one repeat: crosses the decompress workgroup (2 + 257 points), column lists of 2 and 3"""
    coms, idx, cells, proofs = vr.batch([2, 3])
    c1, i1, e1, p1 = vr.batch([2], [5])
    return coms + c1, idx + i1, cells + e1, proofs + p1


@pytest.mark.parametrize("rnd", [None, (0x1234567890abcdef << 64 | 7).to_bytes(32, "big"), R.to_bytes(32, "big"), (R + 1).to_bytes(32, "big")],
                         ids=["fiat_shamir", "random", "r_falls_back", "r_plus_1"])
def test_257_cells_and_both_challenge_paths(ver, rnd):
    b = _batch_257()
    ref = check(ver, *b, rnd)
    assert ref.verdict is True
    fs = vr.verify(*b, None, pairing=False).r
    assert (ref.r == fs) == (rnd is None or int.from_bytes(rnd, "big") % R == 0)


def test_896_cells_of_seven_blobs(ver):
    assert check(ver, *vr.batch(range(7))).verdict is True


def _spoiled(kind):
    coms, idx, cells, proofs = [list(x) for x in _batch_257()]
    k = 256
    if kind == "wrong_proof":
        proofs[k] = vr.golden_blobs()[2][3][6]
    elif kind == "swapped_proofs":
        proofs[k], proofs[0] = proofs[0], proofs[k]
    elif kind == "proof_off_curve":
        proofs[k] = vr.first_x_off_the_curve()
    elif kind == "proof_outside_subgroup":
        proofs[k] = vr.first_point_outside_the_subgroup()
    elif kind == "commitment_x_ge_p":
        coms[k] = bytes([0x80 | P.to_bytes(48, "big")[0]]) + P.to_bytes(48, "big")[1:]
    elif kind == "element_ge_r":
        cells[k] = cells[k][:-32] + R.to_bytes(32, "big")
    return coms, idx, cells, proofs


@pytest.mark.parametrize("kind,status", [("wrong_proof", vr.VERIFICATION_FAILURE), ("swapped_proofs", vr.VERIFICATION_FAILURE),
                                         ("proof_off_curve", vr.ECC_NOT_ON_CURVE), ("proof_outside_subgroup", vr.ECC_NOT_IN_SUBGROUP),
                                         ("commitment_x_ge_p", vr.ECC_COORDINATE_TOO_LARGE), ("element_ge_r", vr.SCALAR_TOO_LARGE)])
def test_offender_in_the_last_of_257_cells(ver, kind, status):
    ref = check(ver, *_spoiled(kind))
    assert ref.status == status and ref.verdict is (False if status == vr.VERIFICATION_FAILURE else None)


def test_a_call_answers_correctly_right_after_a_refused_one(ver):
    """the workspace is reused: a refused batch (larger, so the workspace was grown for it) leaves nothing behind"""
    from constantine_amd import kzg
    good = vr.batch([4, 6], [1, 2, 3])
    ref = vr.verify(*good)
    for kind in ("element_ge_r", "proof_off_curve", "wrong_proof"):
        bad = _spoiled(kind)
        if kind == "wrong_proof":
            assert ver.verify(*bad) is False
        else:
            with pytest.raises(kzg.KzgError):
                ver.verify(*bad)
        assert ver.lincombs(*good) == (ref.LL, ref.RL, ref.r) and ver.verify(*good) is True
    coms, idx, cells, proofs = good
    with pytest.raises(kzg.KzgError) as e:
        ver.verify(coms, [128] + idx[1:], cells, proofs)
    assert e.value.status.value == vr.LENGTHS_MISMATCH and ver.verify(*good) is True


def test_verifier_from_a_trusted_setup_file(ver, tmp_path):
    """the c-kzg text format: the verifier reads G2 line 64 and the first 64 monomial G1 lines; the other lines only need their length"""
    from constantine_amd import _lib, peerdas
    raw = vr.srs_bytes()
    lagrange = open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read()
    g2 = raw[64 * 48:].hex()
    lines = ["4096", "65"] + [lagrange[48 * i:48 * i + 48].hex() for i in range(4096)] + [g2] * 65
    lines += [raw[48 * i:48 * i + 48].hex() for i in range(64)] + [raw[:48].hex()] * (4096 - 64)
    path = tmp_path / "trusted_setup.txt"
    path.write_text("\n".join(lines) + "\n")
    v = peerdas.Verifier(0, trusted_setup=str(path))
    try:
        good = vr.batch([2], [0, 127])
        ref = vr.verify(*good, pairing=False)
        assert v.lincombs(*good) == (ref.LL, ref.RL, ref.r) and v.verify(*good) is True
    finally:
        v.delete()
    (tmp_path / "short.txt").write_text("\n".join(lines[:5000]) + "\n")
    with pytest.raises(_lib.GpuUnavailable):
        peerdas.Verifier(0, trusted_setup=str(tmp_path / "short.txt"))
    bad = bytes([raw[0] ^ 0x20]) + raw[1:48]                     # -[tau^0]_1 is a fine point; a neutral is refused
    with pytest.raises(_lib.GpuUnavailable):
        peerdas.Verifier(0, g1_monomial=bytes([0xC0]) + bytes(47) + raw[48:64 * 48], g2_tau64=raw[64 * 48:])
    v2 = peerdas.Verifier(0, g1_monomial=bad + raw[48:64 * 48], g2_tau64=raw[64 * 48:])
    try:
        assert v2.verify(*vr.batch([2], [0])) is False           # a wrong setup: the equation no longer holds
    finally:
        v2.delete()
