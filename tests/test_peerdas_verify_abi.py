"""include/ctt_msm_hip_peerdas_verify.h against _lib.VERIFY_PROTOTYPES and libctt_msm_hip_peerdas_verify.so, by the method of
tests/test_peerdas_recover_abi.py: the same names and kinds, the companion library exports those names and nothing else and imports
only names of the main header, the header compiles as C11, the other headers and libraries gain no name -- and what the symbols answer
where there is no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_abi_symbols import ROOT, _ctypes_kind, _declared_prototypes

HEADER = "ctt_msm_hip_peerdas_verify.h"


def test_prototype_table_agrees_with_the_header():
    from constantine_amd import _lib
    main = _declared_prototypes("ctt_msm_hip.h")
    declared = {name: proto for name, proto in _declared_prototypes(HEADER).items() if name not in main}
    assert len(declared) == 8
    assert set(_lib.VERIFY_PROTOTYPES) == set(declared), sorted(set(_lib.VERIFY_PROTOTYPES) ^ set(declared))
    for name, (restype, argtypes) in _lib.VERIFY_PROTOTYPES.items():
        got = (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes])
        assert got == declared[name], (name, got, declared[name])
    others = set(_lib.PROTOTYPES) | set(_lib.FIXED_PROTOTYPES) | set(_lib.BW_PROTOTYPES) | set(_lib.PEERDAS_PROTOTYPES)
    assert not set(_lib.VERIFY_PROTOTYPES) & others
    assert "ctt_eth_kzg_verify_cell_kzg_proof_batch" not in declared       # the reference-named symbol is left out: the header says why


def test_companion_library_exports_its_header_and_nothing_else():
    from constantine_amd import _lib
    assert os.path.exists(_lib.VERIFY_LIB_PATH), f"{_lib.VERIFY_LIB_PATH} not built; run __graft_entry__.build()"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.VERIFY_LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == set(_lib.VERIFY_PROTOTYPES), sorted(names ^ set(_lib.VERIFY_PROTOTYPES))
    L = _lib.verify_lib()
    for name, (restype, argtypes) in _lib.VERIFY_PROTOTYPES.items():
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    # it is built over the main library's public C ABI: every ctt_* name it imports is one the main header declares
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", _lib.VERIFY_LIB_PATH], text=True)
    imported = {line.split()[-1].split("@")[0] for line in undefined.splitlines() if " ctt_" in line}
    assert imported and imported <= set(_lib.PROTOTYPES), sorted(imported - set(_lib.PROTOTYPES))
    for path in (_lib.LIB_PATH, _lib.PEERDAS_LIB_PATH):
        other = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "verif" not in other and "pairing" not in other, path


def test_header_compiles_as_c11():
    src = r'''
    #include "ctt_msm_hip_peerdas_verify.h"
    int main(void) {
      float ms[6];
      unsigned char rnd[32] = {0}, r[32];
      return ctt_hip_peerdas_verify_last_timings(0, ms, 6) + ctt_hip_peerdas_verify_cell_kzg_proof_batch(0, 0, 0, 0, 0, 0, rnd) +
             ctt_hip_peerdas_verify_challenge(r, 0, 0, 0, 0, 0, 0, 0) + ctt_hip_peerdas_pairing_check(0, 0, 0);
    }
    '''
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-fsyntax-only"],
                       input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_challenge_symbol_needs_no_device():
    from constantine_amd import peerdas
    from tests import _verifyref as vr
    for _name, coms, cidx, idx, cells, proofs, want in vr.challenge_cases():
        assert peerdas.verify_challenge(coms, cidx, idx, cells, proofs) == want, _name


def test_pairing_symbol_needs_no_device():
    from constantine_amd import peerdas
    from oracle import pyoracle as po
    G1, G2 = po.BLS12_381_G1, po.BLS12_381_G2
    Pt, Q = G1.scalar_mul(3, G1.gen), G2.scalar_mul(11, G2.gen)
    g1 = lambda p: G1.aff_to_bytes(p)
    g2 = lambda q: G2.aff_to_bytes(q)
    assert peerdas.pairing_check([g1(Pt), g1(G1.neg(Pt))], [g2(Q), g2(Q)]) is True
    # e(3 G1, 11 G2) = e(33 G1, G2)
    assert peerdas.pairing_check([g1(Pt), g1(G1.neg(G1.scalar_mul(33, G1.gen)))], [g2(Q), g2(G2.gen)]) is True
    assert peerdas.pairing_check([g1(G1.gen), g1(G1.gen)], [g2(G2.gen), g2(G2.gen)]) is False
    assert peerdas.pairing_check([g1(None)], [g2(Q)]) is True and peerdas.pairing_check([g1(Pt)], [g2(None)]) is True
    assert peerdas.pairing_check([], []) is True


def test_symbols_without_a_device():
    """No device, no verifier: create answers NULL, and a call without a verifier gets the reference's answer for a nil context,
    cttEthKzg_InputsLengthsMismatch, before anything is read -- there is no object through which 0xF0 could be reached (a verifier that
    loses its device later answers 0xF0: vf_run).  Every check of the input that needs no device is run by tests/verify_harness.cpp."""
    from constantine_amd import _lib, peerdas
    from tests import _verifyref as vr
    if _lib.lib().ctt_hip_msm_available() == 1:
        pytest.skip("a device is present: tests/test_peerdas_verify_gpu.py runs the symbols")
    L = _lib.verify_lib()
    raw = vr.srs_bytes()
    assert L.ctt_hip_peerdas_verifier_create(0, raw[:64 * 48], raw[64 * 48:]) is None
    assert L.ctt_hip_peerdas_verifier_create(0, None, None) is None
    assert L.ctt_hip_peerdas_verifier_create_from_file(0, b"/nonexistent/trusted_setup.txt") is None
    L.ctt_hip_peerdas_verifier_destroy(None)
    with pytest.raises(_lib.GpuUnavailable):
        peerdas.Verifier(0, g1_monomial=raw[:64 * 48], g2_tau64=raw[64 * 48:])
    coms, idx, cells, proofs = vr.batch([0], [0])
    vp = lambda b: np.frombuffer(b, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p)
    ind = (ctypes.c_uint64 * 1)(*idx)
    out = np.full(48 + 48 + 32, 0xA5, dtype=np.uint8)
    o = out.ctypes.data
    rnd = bytes(32)
    for n in (0, 1):
        assert L.ctt_hip_peerdas_verify_cell_kzg_proof_batch(None, vp(coms[0]), ind, vp(cells[0]), vp(proofs[0]), n, vp(rnd)) == vr.LENGTHS_MISMATCH
        assert L.ctt_hip_peerdas_verify_lincombs(None, o, o + 48, o + 96, vp(coms[0]), ind, vp(cells[0]), vp(proofs[0]), n, vp(rnd)) == vr.LENGTHS_MISMATCH
    assert set(out.tolist()) == {0xA5}
    ms = (ctypes.c_float * 6)()
    assert L.ctt_hip_peerdas_verify_last_timings(None, ms, 6) == 0
