"""EIP-7594 cells and cell proofs without a GPU: the Python restatement (tests/_peerdasref.py) pinned to the reference's vectors
(tests/golden/peerdas_cells_and_proofs.json), the identity the quotient step rests on, and the new symbols' export."""
import hashlib
import random

import pytest

from oracle import kzg_spec as ks
from tests import _peerdasref as pr

VALID = [c for c in pr.fixture_cases() if c[2] is not None]


def test_fixture_shape():
    cases = pr.fixture_cases()
    assert len(cases) == 11 and len(VALID) == 7
    for case, blob, dig, proofs in cases:
        if dig is None:
            assert proofs is None
            with pytest.raises(ks.SpecError):
                ks.blob_to_bigint_polynomial(blob)
        else:
            assert len(dig) == 128 and len(proofs) == 128 and all(len(p) == 48 for p in proofs)


@pytest.mark.parametrize("case", VALID, ids=[c[0] for c in VALID])
def test_restatement_reproduces_the_reference_vectors(case):
    name, blob, dig, proofs = case
    p = pr.coefficients(blob)
    got = pr.cells(blob, p)
    assert [hashlib.sha256(c).hexdigest() for c in got] == dig, name
    for k in (0, 1, 64, 127):
        assert pr.proof(pr.quotient(p, k)) == proofs[k], (name, k)


def test_quotient_identity():
    """q_k * (X^64 - c_k) + r_k = p with deg r_k < 64, coefficient by coefficient"""
    rng = random.Random(7594)
    p = [rng.randrange(pr.R) for _ in range(pr.N)]
    for k in (0, 77, 127):
        q, c = pr.quotient(p, k), pr.c_of(k)
        assert not any(q[pr.N - 64:])
        prod = [0] * (pr.N + 64)
        for j, v in enumerate(q):
            prod[j + 64] = (prod[j + 64] + v) % pr.R
            prod[j] = (prod[j] - c * v) % pr.R
        rem = [(a - b) % pr.R for a, b in zip(p, prod)]
        assert not any(rem[64:]) and not any(prod[pr.N:]), k
        # and the remainder is the cell's interpolant: it takes the cell's values on the cell's coset
        h = pow(pr.W8192, pr._nttref.brp(k, 7), pr.R)            # c_k = h^64
        w64 = pow(pr.W4096, 64, pr.R)
        x = h * pow(w64, 5, pr.R) % pr.R
        ev = lambda poly: sum(a * pow(x, i, pr.R) for i, a in enumerate(poly)) % pr.R   # noqa: E731
        assert ev(rem[:64]) == ev(p), k


def test_new_symbols_are_exported():
    from constantine_amd import _lib
    L = _lib.lib()
    for name in ("ctt_hip_fr_ntt_plan_create", "ctt_hip_fr_ntt_plan_destroy", "ctt_hip_fr_ntt", "ctt_hip_fr_ntt_plan_info",
                 "ctt_eth_kzg_compute_cells_and_kzg_proofs", "ctt_hip_eth_kzg_compute_cells", "ctt_hip_eth_kzg_cell_quotients"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    assert L.ctt_hip_msm_abi_version() == _lib.ABI_VERSION == 11
