"""include/ctt_msm_hip_fixed.h against _lib.FIXED_PROTOTYPES and libctt_msm_hip_fixed.so, by the method of tests/test_abi_symbols.py:
the same names and kinds, the companion library exports those names and nothing else, the header compiles as C11, and the main
header and library gain no name from the feature (no GPU, no compute)."""
import os
import subprocess

from tests.test_abi_symbols import ROOT, _ctypes_kind, _declared_prototypes

HEADER = "ctt_msm_hip_fixed.h"


def _own(declared):
    """the header includes the main one: what it declares itself"""
    main = _declared_prototypes("ctt_msm_hip.h")
    return {name: proto for name, proto in declared.items() if name not in main}


def test_prototype_table_agrees_with_the_header():
    from constantine_amd import _lib
    declared = _own(_declared_prototypes(HEADER))
    assert len(declared) == 6 and all(name.startswith("ctt_hip_fixed_") for name in declared)
    assert set(_lib.FIXED_PROTOTYPES) == set(declared), sorted(set(_lib.FIXED_PROTOTYPES) ^ set(declared))
    for name, (restype, argtypes) in _lib.FIXED_PROTOTYPES.items():
        got = (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes])
        assert got == declared[name], (name, got, declared[name])
    assert not set(_lib.FIXED_PROTOTYPES) & set(_lib.PROTOTYPES)


def test_companion_library_exports_its_header_and_nothing_else():
    from constantine_amd import _lib
    assert os.path.exists(_lib.FIXED_LIB_PATH), f"{_lib.FIXED_LIB_PATH} not built; run __graft_entry__.build()"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.FIXED_LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == set(_lib.FIXED_PROTOTYPES), sorted(names ^ set(_lib.FIXED_PROTOTYPES))
    L = _lib.fixed_lib()
    for name, (restype, argtypes) in _lib.FIXED_PROTOTYPES.items():
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    # the engine's library keeps its names: the kernels it shares with the companion are hidden C++
    main = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "fixed" not in main


def test_header_compiles_as_c11():
    src = r'''
    #include "ctt_msm_hip_fixed.h"
    _Static_assert(CTT_HIP_FIXED_COEFS_ON_DEVICE == 1 && CTT_HIP_FIXED_OUT_ON_DEVICE == 2, "flags");
    int main(void) { size_t info[6]; return ctt_hip_fixed_bases_info(0, info) + ctt_hip_fixed_last_error(); }
    '''
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-fsyntax-only"],
                       input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_refusals_without_a_handle_are_reported_not_fatal():
    """nothing here needs a device: a NULL handle is refused with -1 and the thread's last error says so"""
    from constantine_amd import _lib
    L = _lib.fixed_lib()
    assert L.ctt_hip_fixed_msm_batch(None, 0, None, 1, None, 0) == -1
    assert L.ctt_hip_fixed_last_error() == -1
    assert L.ctt_hip_fixed_bases_info(None, None) == -1
    L.ctt_hip_fixed_bases_destroy(None)
