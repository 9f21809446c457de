"""ctypes loader for libctt_msm_hip.so. The product path has no fallback: a missing library is an error.

The prototypes of the libraries are the tables below, name -> (restype, argtypes); tests/test_abi_symbols.py,
tests/test_fixed_abi.py, tests/test_peerdas_recover_abi.py and tests/test_peerdas_verify_abi.py derive the same from the C headers and compare."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTT_MSM_HIP_LIB") or os.path.join(HERE, "libctt_msm_hip.so")
BW_LIB_PATH = os.path.join(HERE, "libctt_msm_hip_banderwagon.so")
FIXED_LIB_PATH = os.path.join(HERE, "libctt_msm_hip_fixed.so")
PEERDAS_LIB_PATH = os.path.join(HERE, "libctt_msm_hip_peerdas.so")
VERIFY_LIB_PATH = os.path.join(HERE, "libctt_msm_hip_peerdas_verify.so")

_lib = None
_bw_lib = None
_fixed_lib = None
_peerdas_lib = None
_verify_lib = None
ABI_VERSION = 11  # ctt_hip_msm_abi_version() of the library this package was written against
GPU_UNAVAILABLE = 0xF0   # CTT_HIP_STATUS_GPU_UNAVAILABLE: what a protocol symbol returns when the GPU cannot serve the call


class HipLibraryMissing(RuntimeError):
    pass


vp, sz, i32, u32, u64, cstr = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p
u8 = ctypes.c_uint8                                  # the reference's status enums are __attribute__((__packed__)): one byte
pvp, pi32 = ctypes.POINTER(vp), ctypes.POINTER(i32)  # out-handles and int arrays the callers pass with byref / as ctypes arrays
psz, pf32 = ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_float)
pu64 = ctypes.POINTER(u64)


def _msm_families():
    """include/ctt_msm_hip.h parts 1 and 1c: the per-curve MSMs under Constantine's names, *_batch_affine, the neutral spellings"""
    t = {}
    for stem, par in (("bls12_381_g1", True), ("bls12_381_g2", False), ("bn254_snarks_g1", True),
                      ("bn254_snarks_g2", False), ("pallas_ec", True), ("vesta_ec", True)):
        for coord in ("jac", "prj"):
            for coef in ("big", "fr"):
                t[f"ctt_{stem}_{coord}_multi_scalar_mul_{coef}_coefs_vartime"] = (None, [vp, vp, vp, sz])
                if par:
                    t[f"ctt_{stem}_{coord}_multi_scalar_mul_{coef}_coefs_vartime_parallel"] = (None, [vp, vp, vp, vp, sz])
            t[f"ctt_{stem}_{coord}_batch_affine"] = (None, [vp, vp, sz])
            for coef in ("big", "fr"):
                t[f"ctt_hip_msm_{stem}_{coord}_{coef}"] = (i32, [vp, vp, vp, sz])
    return t


PROTOTYPES = {
    **_msm_families(),
    "ctt_hip_sum_reduce": (i32, [vp, i32, i32, vp, vp, sz, i32]),
    "ctt_hip_batch_affine": (i32, [vp, i32, i32, vp, vp, sz, i32]),
    "ctt_hip_msm_abi_version": (i32, []),
    "ctt_hip_msm_ctx_create": (vp, [i32]),
    "ctt_hip_msm_ctx_destroy": (None, [vp]),
    "ctt_hip_msm_set_option": (i32, [vp, cstr, i32]),
    "ctt_hip_msm_device": (i32, [vp, i32, i32, i32, vp, vp, vp, sz]),
    "ctt_hip_msm_device_submit": (i32, [vp, i32, i32, vp, vp, sz]),
    "ctt_hip_msm_device_finish": (i32, [vp, i32, i32, vp]),
    "ctt_hip_msm_sync": (None, [vp]),
    "ctt_hip_msm_bases_create": (vp, [vp, i32, vp, sz, i32]),
    "ctt_hip_msm_bases_destroy": (None, [vp, vp]),
    "ctt_hip_msm_with_bases": (i32, [vp, vp, i32, i32, vp, vp, sz, i32]),
    "ctt_hip_msm_with_bases_submit": (i32, [vp, vp, i32, vp, sz]),
    "ctt_hip_msm_bases_create_table": (vp, [vp, i32, vp, sz, i32, i32]),
    "ctt_hip_msm_bases_window_bits": (i32, [vp]),
    "ctt_hip_msm_last_timings": (i32, [vp, vp, i32]),
    "ctt_hip_msm_last_plan": (i32, [vp, vp, i32]),
    "ctt_hip_gen_points": (i32, [vp, i32, u64, u64, u32, vp]),
    "ctt_hip_field_op": (i32, [vp, i32, i32, vp, vp, vp, u32]),
    "ctt_hip_sort_probe": (i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp]),
    "ctt_hip_sort_probe_words": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
    "ctt_hip_glv_front_probe": (i32, [vp, i32, vp, vp, u32, vp, vp]),
    "ctt_hip_ec_sum_affine": (i32, [i32, i32, vp, vp, sz]),
    "ctt_hip_msm_stream": (vp, [vp]),
    "ctt_hip_msm_wait_stream": (i32, [vp, vp]),
    "ctt_hip_msm_set_devices": (i32, [pi32, i32]),
    "ctt_hip_msm_set_shard_min": (None, [sz]),
    "ctt_hip_subgroup_check": (i32, [vp, i32, vp, vp, sz, i32]),
    "ctt_hip_fr_quotient": (i32, [vp, i32, vp, vp, vp, vp, vp, u32]),
    "ctt_hip_msm_host": (i32, [i32, i32, i32, vp, vp, vp, sz]),
    "ctt_hip_msm_available": (i32, []),
    "ctt_hip_last_error": (i32, []),
    "ctt_hip_last_error_message": (cstr, []),
    "ctt_hip_clear_last_error": (None, []),
    # part 3: the MSM's callers under the reference's names + their host-only pieces
    "ctt_eth_kzg_context_new": (u8, [pvp, cstr, u8]),
    "ctt_eth_kzg_context_new_with_precompute": (u8, [pvp, cstr, u8, i32, i32]),
    "ctt_eth_kzg_context_delete": (None, [vp]),
    "ctt_eth_kzg_blob_to_kzg_commitment": (u8, [vp, vp, vp]),
    "ctt_eth_kzg_compute_kzg_proof": (u8, [vp, vp, vp, vp, vp]),
    "ctt_eth_kzg_compute_blob_kzg_proof": (u8, [vp, vp, vp, vp]),
    "ctt_eth_kzg_blob_to_kzg_commitment_parallel": (u8, [vp, vp, vp, vp]),       # (tp, ...) -- ethereum_eip4844_kzg_parallel.h
    "ctt_eth_kzg_compute_kzg_proof_parallel": (u8, [vp, vp, vp, vp, vp, vp]),
    "ctt_eth_kzg_compute_blob_kzg_proof_parallel": (u8, [vp, vp, vp, vp, vp]),
    "ctt_eth_evm_bls12381_g1msm": (u8, [vp, sz, vp, sz]),
    "ctt_eth_evm_bls12381_g2msm": (u8, [vp, sz, vp, sz]),
    "ctt_hip_eth_kzg_context_from_srs": (i32, [pvp, vp, sz, i32, i32]),
    "ctt_hip_sha256": (None, [vp, vp, sz]),
    "ctt_hip_bls12_381_g1_decompress": (i32, [vp, vp]),
    "ctt_hip_bls12_381_g1_compress": (None, [vp, vp]),
    "ctt_hip_eth_kzg_blob_to_scalars": (i32, [vp, vp]),
    "ctt_hip_eth_kzg_challenge": (None, [vp, vp, vp]),
    "ctt_hip_eth_kzg_quotient_host": (None, [vp, vp, vp, vp]),
    # part 4: batched Verkle commitments over a fixed Banderwagon basis
    "ctt_hip_verkle_crs_create": (vp, [vp, vp, sz, i32, i32]),
    "ctt_hip_verkle_crs_destroy": (None, [vp, vp]),
    "ctt_hip_verkle_crs_window_bits": (i32, [vp]),
    "ctt_hip_verkle_commit_batch": (i32, [vp, vp, i32, vp, vp, vp, vp, sz, i32]),
    "ctt_hip_banderwagon_map_to_fr_batch": (i32, [vp, vp, vp, sz, i32]),
    "ctt_hip_banderwagon_serialize_batch": (i32, [vp, vp, vp, sz, i32]),
    "ctt_hip_verkle_last_timings": (i32, [vp, vp, i32]),
    "ctt_hip_verkle_update_batch": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, i32]),
    # part 5: the scalar-field NTT; the EIP-7594 cells and cell proofs on top of it (part 3)
    "ctt_hip_fr_ntt_plan_create": (vp, [vp, i32, i32, vp, i32]),
    "ctt_hip_fr_ntt_plan_destroy": (None, [vp, vp]),
    "ctt_hip_fr_ntt_plan_info": (i32, [vp, vp]),
    "ctt_hip_fr_ntt": (i32, [vp, vp, vp, vp, sz, i32, vp]),
    "ctt_eth_kzg_compute_cells_and_kzg_proofs": (u8, [vp, vp, vp, vp]),
    "ctt_hip_eth_kzg_compute_cells": (u8, [vp, vp, vp]),
    "ctt_hip_eth_kzg_cell_quotients": (u8, [vp, vp, vp]),
    "ctt_hip_eth_kzg_last_cell_timings": (i32, [vp, vp, i32]),
}

# include/ctt_msm_hip_banderwagon.h: the Banderwagon symbols under Constantine's names, and their neutral spellings
BW_PROTOTYPES = {}
for _coef in ("big", "fr"):
    BW_PROTOTYPES[f"ctt_banderwagon_ec_prj_multi_scalar_mul_{_coef}_coefs_vartime"] = (None, [vp, vp, vp, sz])
    BW_PROTOTYPES[f"ctt_hip_msm_banderwagon_ec_prj_{_coef}"] = (i32, [vp, vp, vp, sz])


# include/ctt_msm_hip_fixed.h: the batched fixed-base MSM over BLS12-381 G1 and BN254 G1 (a library with kernels of its own)
FIXED_PROTOTYPES = {
    "ctt_hip_fixed_bases_create": (vp, [i32, i32, vp, sz, i32]),
    "ctt_hip_fixed_bases_destroy": (None, [vp]),
    "ctt_hip_fixed_bases_info": (i32, [vp, psz]),
    "ctt_hip_fixed_msm_batch": (i32, [vp, i32, vp, sz, vp, i32]),
    "ctt_hip_fixed_last_timings": (i32, [vp, pf32]),
    "ctt_hip_fixed_last_error": (i32, []),
}


# include/ctt_msm_hip_peerdas.h: EIP-7594 recovery, batched over blobs (a library with kernels of its own over the C ABI of lib())
PEERDAS_PROTOTYPES = {
    "ctt_hip_peerdas_recovery_create": (vp, [i32]),
    "ctt_hip_peerdas_recovery_destroy": (None, [vp]),
    "ctt_hip_peerdas_recover_blobs": (i32, [vp, vp, vp, pu64, vp, sz, sz]),
    "ctt_hip_eth_kzg_recover_cells_and_kzg_proofs_batch": (u8, [vp, vp, vp, vp, pu64, vp, sz, sz]),
    "ctt_eth_kzg_recover_cells_and_kzg_proofs": (u8, [vp, vp, vp, pu64, vp, sz]),
    "ctt_hip_peerdas_recover_coefficients": (i32, [vp, vp, vp, pu64, vp, sz, sz]),
    "ctt_hip_peerdas_recovery_constants": (i32, [vp, vp, pu64, sz]),
    "ctt_hip_peerdas_last_timings": (i32, [vp, pf32, i32]),
}


# include/ctt_msm_hip_peerdas_verify.h: EIP-7594 batch verification (a library with kernels of its own and the host pairing, over the C
# ABI of lib())
VERIFY_PROTOTYPES = {
    "ctt_hip_peerdas_verifier_create": (vp, [i32, vp, vp]),
    "ctt_hip_peerdas_verifier_create_from_file": (vp, [i32, cstr]),
    "ctt_hip_peerdas_verifier_destroy": (None, [vp]),
    "ctt_hip_peerdas_verify_cell_kzg_proof_batch": (i32, [vp, vp, pu64, vp, vp, sz, vp]),
    "ctt_hip_peerdas_verify_challenge": (i32, [vp, vp, sz, pu64, pu64, vp, vp, sz]),
    "ctt_hip_peerdas_verify_lincombs": (i32, [vp, vp, vp, vp, vp, pu64, vp, vp, sz, vp]),
    "ctt_hip_peerdas_pairing_check": (i32, [vp, vp, sz]),
    "ctt_hip_peerdas_verify_last_timings": (i32, [vp, pf32, i32]),
}


def exported_symbols():
    """Every symbol include/ctt_msm_hip.h declares."""
    return list(PROTOTYPES)


class GpuUnavailable(RuntimeError):
    """A call the GPU could not serve (no device, out of device memory, a failed HIP call, both in-flight slots taken): the
    library reports it through the call's return value; `code` / the message are ctt_hip_last_error() / _message() of this thread.
    There is no CPU path inside the library -- what to do instead is the caller's decision."""

    def __init__(self, what=""):
        L = lib()
        self.code = int(L.ctt_hip_last_error())
        msg = L.ctt_hip_last_error_message()
        super().__init__(f"{what}: GPU unavailable ({self.code}): {msg.decode(errors='replace') if msg else ''}")


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 and asks for it by the unversioned name,
    so if this library pulled in /opt/rocm's copy first, torch would load a second runtime that finds no GPU.  When
    torch is installed, load ITS runtime first (same SONAME libamdhip64.so.7 -> our NEEDED entry binds to it)."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def _load(path, prototypes, header, allow_old=False):
    """dlopen `path` and give every symbol of `prototypes` its argtypes and restype.  A symbol the library lacks is an error, except
    with allow_old: then it becomes a stub, so that a call fails loudly instead of running with default prototypes."""
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
        elif allow_old:
            def _absent(*a, _n=name, **k):
                raise AttributeError(f"{path} (old ABI) has no {_n}")
            setattr(L, name, _absent)
        else:
            raise AttributeError(f"{path} does not export {name} (include/{header} declares it); an older build "
                                 "for a comparison needs CTT_MSM_HIP_ALLOW_OLD_ABI=1")
    return L


def banderwagon_lib():
    """libctt_msm_hip_banderwagon.so (include/ctt_msm_hip_banderwagon.h): the Banderwagon symbols under Constantine's names, over lib()."""
    global _bw_lib
    if _bw_lib is None:
        lib()   # the engine first: the companion library resolves against the copy already loaded
        if not os.path.exists(BW_LIB_PATH):
            raise HipLibraryMissing(f"{BW_LIB_PATH} not found: build it with make -C constantine_amd/csrc")
        _bw_lib = _load(BW_LIB_PATH, BW_PROTOTYPES, "ctt_msm_hip_banderwagon.h")
    return _bw_lib


def fixed_lib():
    """libctt_msm_hip_fixed.so (include/ctt_msm_hip_fixed.h): the batched fixed-base MSM.  It does not need lib(), but shares its HIP runtime."""
    global _fixed_lib
    if _fixed_lib is None:
        if not os.path.exists(FIXED_LIB_PATH):
            raise HipLibraryMissing(f"{FIXED_LIB_PATH} not found: build it with make -C constantine_amd/csrc")
        _share_hip_runtime_with_torch()
        _fixed_lib = _load(FIXED_LIB_PATH, FIXED_PROTOTYPES, "ctt_msm_hip_fixed.h")
    return _fixed_lib


def peerdas_lib():
    """libctt_msm_hip_peerdas.so (include/ctt_msm_hip_peerdas.h): EIP-7594 recovery, over lib()."""
    global _peerdas_lib
    if _peerdas_lib is None:
        lib()   # the engine first: the companion library resolves against the copy already loaded
        if not os.path.exists(PEERDAS_LIB_PATH):
            raise HipLibraryMissing(f"{PEERDAS_LIB_PATH} not found: build it with make -C constantine_amd/csrc")
        _peerdas_lib = _load(PEERDAS_LIB_PATH, PEERDAS_PROTOTYPES, "ctt_msm_hip_peerdas.h")
    return _peerdas_lib


def verify_lib():
    """libctt_msm_hip_peerdas_verify.so (include/ctt_msm_hip_peerdas_verify.h): EIP-7594 batch verification, over lib()."""
    global _verify_lib
    if _verify_lib is None:
        lib()   # the engine first: the companion library resolves against the copy already loaded
        if not os.path.exists(VERIFY_LIB_PATH):
            raise HipLibraryMissing(f"{VERIFY_LIB_PATH} not found: build it with make -C constantine_amd/csrc")
        _verify_lib = _load(VERIFY_LIB_PATH, VERIFY_PROTOTYPES, "ctt_msm_hip_peerdas_verify.h")
    return _verify_lib


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C constantine_amd/csrc). There is no CPU fallback.")
        _share_hip_runtime_with_torch()
        # an OLDER build named explicitly for a same-box comparison (tools/ab_prev.sh) may predate a symbol: only with the explicit
        # opt-in CTT_MSM_HIP_ALLOW_OLD_ABI=1 is a missing symbol skipped; any other library must export what the header declares
        allow_old = bool(os.environ.get("CTT_MSM_HIP_LIB")) and os.environ.get("CTT_MSM_HIP_ALLOW_OLD_ABI") == "1"
        _lib = _load(LIB_PATH, PROTOTYPES, "ctt_msm_hip.h", allow_old)
    return _lib
