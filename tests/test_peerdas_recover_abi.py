"""include/ctt_msm_hip_peerdas.h against _lib.PEERDAS_PROTOTYPES and libctt_msm_hip_peerdas.so, by the method of
tests/test_abi_symbols.py: the same names and kinds, the companion library exports those names and nothing else, the header compiles as
C11, the main header and library gain no name -- and what the reference-named symbol answers where there is no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_abi_symbols import ROOT, _ctypes_kind, _declared_prototypes

HEADER = "ctt_msm_hip_peerdas.h"


def test_prototype_table_agrees_with_the_header():
    from constantine_amd import _lib
    main = _declared_prototypes("ctt_msm_hip.h")
    declared = {name: proto for name, proto in _declared_prototypes(HEADER).items() if name not in main}
    assert len(declared) == 8
    assert set(_lib.PEERDAS_PROTOTYPES) == set(declared), sorted(set(_lib.PEERDAS_PROTOTYPES) ^ set(declared))
    for name, (restype, argtypes) in _lib.PEERDAS_PROTOTYPES.items():
        got = (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes])
        assert got == declared[name], (name, got, declared[name])
    assert not set(_lib.PEERDAS_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.FIXED_PROTOTYPES) | set(_lib.BW_PROTOTYPES))


def test_companion_library_exports_its_header_and_nothing_else():
    from constantine_amd import _lib
    assert os.path.exists(_lib.PEERDAS_LIB_PATH), f"{_lib.PEERDAS_LIB_PATH} not built; run __graft_entry__.build()"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.PEERDAS_LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == set(_lib.PEERDAS_PROTOTYPES), sorted(names ^ set(_lib.PEERDAS_PROTOTYPES))
    L = _lib.peerdas_lib()
    for name, (restype, argtypes) in _lib.PEERDAS_PROTOTYPES.items():
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    # it is built over the main library's public C ABI: every ctt_* name it imports is one the main header declares
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", _lib.PEERDAS_LIB_PATH], text=True)
    imported = {line.split()[-1].split("@")[0] for line in undefined.splitlines() if " ctt_" in line}
    assert imported and imported <= set(_lib.PROTOTYPES), sorted(imported - set(_lib.PROTOTYPES))
    main = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "recover" not in main and "peerdas" not in main


def test_header_compiles_as_c11():
    src = r'''
    #include "ctt_msm_hip_peerdas.h"
    _Static_assert(sizeof(ctt_eth_kzg_cell) == 2048 && sizeof(ctt_eth_kzg_proof) == 48 && sizeof(ctt_eth_kzg_status) == 1, "types");
    int main(void) {
      float ms[5];
      return ctt_hip_peerdas_last_timings(0, ms, 5) + (int)ctt_eth_kzg_recover_cells_and_kzg_proofs(0, 0, 0, 0, 0, 64);
    }
    '''
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-fsyntax-only"],
                       input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_constants_symbol_needs_no_device():
    from constantine_amd import peerdas
    from tests import _recoverref as rr
    idx = rr.index_sets()["all_but_127"]
    zc, izc5 = peerdas.recovery_constants(idx)
    c127 = pow(rr.W8192, 64 * 127, rr.R)               # brp7(127) = 127
    for k in (0, 1, 126):
        ck = pow(rr.W8192, 64 * int(format(k, "07b")[::-1], 2), rr.R)
        assert zc[k] == (ck - c127) % rr.R and izc5[k] * (pow(5, 64, rr.R) * ck - c127) % rr.R == 1
    assert zc[127] == 0
    assert peerdas.recovery_constants(range(128)) == ([1] * 128, [1] * 128)     # nothing missing: Z = 1
    with pytest.raises(peerdas.KzgError) as e:
        peerdas.recovery_constants([1, 0] + list(range(2, 64)))
    assert e.value.status == peerdas.cttEthKzgStatus.cttEthKzg_CellIndicesNotAscending


def _call(L, ctx, idx, cells):
    out_c = np.full(128 * 2048, 0xA5, dtype=np.uint8)
    out_p = np.full(128 * 48, 0xA5, dtype=np.uint8)
    ind = (ctypes.c_uint64 * max(len(idx), 1))(*idx)
    raw = np.frombuffer(b"".join(cells) or b"\0", dtype=np.uint8)
    rc = L.ctt_eth_kzg_recover_cells_and_kzg_proofs(ctx, out_c.ctypes.data_as(ctypes.c_void_p), out_p.ctypes.data_as(ctypes.c_void_p), ind,
                                                    raw.ctypes.data_as(ctypes.c_void_p), len(idx))
    assert bytes(out_c) == b"\xA5" * (128 * 2048) and bytes(out_p) == b"\xA5" * (128 * 48)    # untouched on every status but Success
    return rc


def test_reference_symbol_without_a_device():
    """invalid input gets the reference's status first; valid input cannot be served: 0xF0, sentinel-filled outputs untouched"""
    from constantine_amd import _lib
    from tests import _recoverref as rr
    if _lib.lib().ctt_hip_msm_available() == 1:
        pytest.skip("a device is present: tests/test_peerdas_recover_gpu.py runs the symbol")
    L = _lib.peerdas_lib()
    ctx = ctypes.c_void_p(1)       # never dereferenced before the recovery itself succeeded
    cells = rr.value_cells("zero")[1]
    half = list(range(64))
    assert _call(L, None, half, cells[:64]) == rr.LENGTHS_MISMATCH
    assert _call(L, ctx, list(range(63)), cells[:63]) == rr.LENGTHS_MISMATCH
    assert _call(L, ctx, list(range(63)) + [128], cells[:64]) == rr.LENGTHS_MISMATCH
    assert _call(L, ctx, [1, 0] + half[2:], cells[:64]) == rr.NOT_ASCENDING
    assert _call(L, ctx, half, cells[:63] + [b"\xff" * 2048]) == rr.SCALAR_TOO_LARGE
    assert _call(L, ctx, half, cells[:64]) == _lib.GPU_UNAVAILABLE
    assert L.ctt_hip_peerdas_recovery_create(0) is None
    L.ctt_hip_peerdas_recovery_destroy(None)
