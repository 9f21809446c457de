"""
EIP-4844 blob -> KZG commitment and opening proofs on top of the MSM engine (the MSM's immediate caller):
ctypes callers of the reference's own C symbols, which libctt_msm_hip.so exports (include/ctt_msm_hip.h part 3,
constantine_amd/csrc/protocols.hip):

    ctt_eth_kzg_blob_to_kzg_commitment    include/constantine/protocols/ethereum_eip4844_kzg.h:106   (ethereum_eip4844_kzg.nim:297-330)
    ctt_eth_kzg_compute_kzg_proof         :126                                                       (:332-375)
    ctt_eth_kzg_compute_blob_kzg_proof    :153                                                       (:409-444)
    ctt_eth_kzg_context_new / _delete     :200, :238

Wire parsing, range checks, the Fiat-Shamir hash and point (de)compression are C++ on the host, every MSM, the subgroup check
and the quotient polynomial run on the GPU.  Nothing is computed in Python here; the only checks this module adds are the byte
LENGTHS, which the C signatures fix by type (ctt_eth_kzg_blob = 131072 bytes ...) and a Python `bytes` does not.  The EIP-4844
verifications (verify_kzg_proof, verify_blob_kzg_proof*) are not provided.

EIP-7594 (PeerDAS) on the same context:

    ctt_eth_kzg_compute_cells_and_kzg_proofs   include/constantine/protocols/ethereum_eip7594_peerdas.h
    ctt_hip_eth_kzg_compute_cells              the cells alone (the reference's Nim API has it, its C header does not)

The blob's coefficients, the coset evaluations of the cells and the evaluations of the 128 cell quotients are transforms of the
scalar-field NTT (ntt.py); the proofs are 128 MSMs over the cached Lagrange SRS.

    ctt_eth_kzg_recover_cells_and_kzg_proofs   the same header, :91 -- in the companion library libctt_msm_hip_peerdas.so
                                               (peerdas.py has the batched form)

verify_cell_kzg_proof_batch is peerdas.Verifier: a companion library of its own, libctt_msm_hip_peerdas_verify.so, whose verifier object
owns the monomial points the check needs; the device does what grows with the batch, the host the one pairing check (DESIGN.md
section 16).  The FK20 form of the proofs is out of scope.
"""
import ctypes
from enum import Enum

import numpy as np

from . import _lib
from ._arrays import ptr

FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_FIELD_ELEMENT = 32
BYTES_PER_BLOB = FIELD_ELEMENTS_PER_BLOB * BYTES_PER_FIELD_ELEMENT
BYTES_PER_COMMITMENT = 48
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = 2048


class cttEthKzgStatus(Enum):  # ethereum_eip4844_kzg.h:29-40
    cttEthKzg_Success = 0
    cttEthKzg_VerificationFailure = 1
    cttEthKzg_InputsLengthsMismatch = 2
    cttEthKzg_ScalarZero = 3
    cttEthKzg_ScalarLargerThanCurveOrder = 4
    cttEthKzg_EccInvalidEncoding = 5
    cttEthKzg_EccCoordinateGreaterThanOrEqualModulus = 6
    cttEthKzg_EccPointNotOnCurve = 7
    cttEthKzg_EccPointNotInSubGroup = 8
    cttEthKzg_CellIndicesNotAscending = 9


class cttEthTrustedSetupStatus(Enum):  # ethereum_eip4844_kzg.h:63-67
    cttEthTS_Success = 0
    cttEthTS_MissingOrInaccessibleFile = 1
    cttEthTS_InvalidFile = 2


class KzgError(ValueError):
    def __init__(self, status):
        super().__init__(status.name)
        self.status = status


def _check(rc):
    if rc == _lib.GPU_UNAVAILABLE:      # CTT_HIP_STATUS_GPU_UNAVAILABLE: outside the reference's enum, nothing was written
        raise _lib.GpuUnavailable("EIP-4844 KZG")
    if rc != 0:
        raise KzgError(cttEthKzgStatus(rc))


def _buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(b)


class EthereumKZGContext:
    """ctt_eth_kzg_context: srs_lagrange_brp_g1 cached on the GPU (constantine/commitments_setups/ethereum_kzg_srs.nim)."""

    def __init__(self, srs_lagrange_g1_compressed: bytes, device=0, table=True):
        """`srs_lagrange_g1_compressed`: 4096 x 48 bytes, the G1 Lagrange points in ceremony (file) order
        (ctt_hip_eth_kzg_context_from_srs).  table=True (what ctt_eth_kzg_context_new does) caches the SRS as a window table."""
        self.L = _lib.lib()
        if len(srs_lagrange_g1_compressed) != FIELD_ELEMENTS_PER_BLOB * 48:
            raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
        h = ctypes.c_void_p()
        rc = self.L.ctt_hip_eth_kzg_context_from_srs(ctypes.byref(h), _buf(srs_lagrange_g1_compressed), FIELD_ELEMENTS_PER_BLOB,
                                                     int(device), 1 if table else 0)
        if rc == _lib.GPU_UNAVAILABLE:
            raise _lib.GpuUnavailable("KZG context")
        if rc != 0:
            raise ValueError(cttEthTrustedSetupStatus(rc).name)
        self.handle = h

    @classmethod
    def from_ckzg_text(cls, path, precompute=None):
        """ctt_eth_kzg_context_new(ctx, filepath, cttEthTSFormat_ckzg4844): the c-kzg text format of the Ethereum ceremony, as
        shipped by the reference in constantine/commitments_setups/trusted_setup_ethereum_kzg4844_reference.dat.
        precompute = (t, b): through ctt_eth_kzg_context_new_with_precompute (the reference's table sizes; the same context here)."""
        self = cls.__new__(cls)
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        if precompute is not None:
            rc = self.L.ctt_eth_kzg_context_new_with_precompute(ctypes.byref(h), str(path).encode(), 0, int(precompute[0]), int(precompute[1]))
        else:
            rc = self.L.ctt_eth_kzg_context_new(ctypes.byref(h), str(path).encode(), 0)
        if rc == _lib.GPU_UNAVAILABLE:
            raise _lib.GpuUnavailable("KZG context")
        if rc != 0:
            raise ValueError(cttEthTrustedSetupStatus(rc).name)
        self.handle = h
        return self

    def delete(self):
        if self.handle:
            self.L.ctt_eth_kzg_context_delete(self.handle)
            self.handle = None


def blob_to_kzg_commitment(ctx: EthereumKZGContext, blob: bytes) -> bytes:
    """commitment = [p(tau)]_1 as 48 compressed bytes; raises KzgError(status) where the reference returns a status."""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    out = (ctypes.c_uint8 * 48)()
    _check(ctx.L.ctt_eth_kzg_blob_to_kzg_commitment(ctx.handle, out, _buf(blob)))
    return bytes(out)


def compute_kzg_proof(ctx: EthereumKZGContext, blob: bytes, z_bytes: bytes):
    """-> (proof 48 B, y 32 B): [proof]_1 = [(p(tau) - p(z)) / (tau - z)]_1 and y = p(z)."""
    if len(blob) != BYTES_PER_BLOB or len(z_bytes) != 32:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    proof, y = (ctypes.c_uint8 * 48)(), (ctypes.c_uint8 * 32)()
    _check(ctx.L.ctt_eth_kzg_compute_kzg_proof(ctx.handle, proof, y, _buf(blob), _buf(z_bytes)))
    return bytes(proof), bytes(y)


def compute_blob_kzg_proof(ctx: EthereumKZGContext, blob: bytes, commitment_bytes: bytes) -> bytes:
    """Proof that the blob matches the commitment, at the Fiat-Shamir challenge."""
    if len(blob) != BYTES_PER_BLOB or len(commitment_bytes) != 48:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    proof = (ctypes.c_uint8 * 48)()
    _check(ctx.L.ctt_eth_kzg_compute_blob_kzg_proof(ctx.handle, proof, _buf(blob), _buf(commitment_bytes)))
    return bytes(proof)


def compute_cells(ctx: EthereumKZGContext, blob: bytes):
    """-> the 128 cells of the extended blob, 2048 bytes each (ctt_hip_eth_kzg_compute_cells)"""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    cells = (ctypes.c_uint8 * (CELLS_PER_EXT_BLOB * BYTES_PER_CELL))()
    _check(ctx.L.ctt_hip_eth_kzg_compute_cells(ctx.handle, cells, _buf(blob)))
    raw = bytes(cells)
    return [raw[BYTES_PER_CELL * k:BYTES_PER_CELL * (k + 1)] for k in range(CELLS_PER_EXT_BLOB)]


def compute_cells_and_kzg_proofs(ctx: EthereumKZGContext, blob: bytes):
    """-> (128 cells of 2048 bytes, 128 proofs of 48 bytes): ctt_eth_kzg_compute_cells_and_kzg_proofs"""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    cells = (ctypes.c_uint8 * (CELLS_PER_EXT_BLOB * BYTES_PER_CELL))()
    proofs = (ctypes.c_uint8 * (CELLS_PER_EXT_BLOB * 48))()
    _check(ctx.L.ctt_eth_kzg_compute_cells_and_kzg_proofs(ctx.handle, cells, proofs, _buf(blob)))
    raw, pr = bytes(cells), bytes(proofs)
    return ([raw[BYTES_PER_CELL * k:BYTES_PER_CELL * (k + 1)] for k in range(CELLS_PER_EXT_BLOB)],
            [pr[48 * k:48 * (k + 1)] for k in range(CELLS_PER_EXT_BLOB)])


def recover_cells_and_kzg_proofs(ctx: EthereumKZGContext, cell_indices, cells):
    """-> (128 cells of 2048 bytes, 128 proofs of 48 bytes) of the blob that at least 64 of its cells determine:
    ctt_eth_kzg_recover_cells_and_kzg_proofs (libctt_msm_hip_peerdas.so).  cells: len(cell_indices) byte strings of 2048; a count or a
    length that does not fit is a ValueError, what the reference rejects a KzgError with its status."""
    from . import peerdas
    idx, arr, batched = peerdas.pack_cells(cell_indices, cells)
    if batched:
        raise ValueError("one blob's cells: a batch goes through peerdas.Recovery")
    out_c = np.zeros((CELLS_PER_EXT_BLOB, BYTES_PER_CELL), dtype=np.uint8)
    out_p = np.zeros((CELLS_PER_EXT_BLOB, 48), dtype=np.uint8)
    _check(_lib.peerdas_lib().ctt_eth_kzg_recover_cells_and_kzg_proofs(ctx.handle, ptr(out_c), ptr(out_p), idx.ctypes.data_as(_lib.pu64),
                                                                       ptr(arr), idx.shape[0]))
    return [out_c[k].tobytes() for k in range(CELLS_PER_EXT_BLOB)], [out_p[k].tobytes() for k in range(CELLS_PER_EXT_BLOB)]


def cell_quotients(ctx: EthereumKZGContext, blob: bytes) -> np.ndarray:
    """ctt_hip_eth_kzg_cell_quotients (test-facing): the coefficients q_k[j] of p / (X^64 - c_k), (128, 4096, 32) uint8 little-endian"""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    q = np.zeros((CELLS_PER_EXT_BLOB, FIELD_ELEMENTS_PER_BLOB, 32), dtype=np.uint8)
    _check(ctx.L.ctt_hip_eth_kzg_cell_quotients(ctx.handle, ptr(q), _buf(blob)))
    return q


def last_cell_timings(ctx: EthereumKZGContext):
    """host-clock ms of the context's last cells call: parse + upload, INTT, coset NTT, quotients, batched NTT, MSM loop, compress + copy back"""
    ms = (ctypes.c_float * 7)()
    ctx.L.ctt_hip_eth_kzg_last_cell_timings(ctx.handle, ms, 7)
    return list(ms)


def last_cell_proof_path(ctx: EthereumKZGContext):
    """-> ("table" | "loop", build_ms) of the context's last cells-and-proofs call: whether the batched fixed-base MSM served the 128
    proofs in one pass or the loop over the cached SRS did (CTT_HIP_CELL_PROOFS=loop at creation, or no memory for the table), and
    the ms that call paid for building the table (the first proof call of a context; 0 afterwards)"""
    ms = (ctypes.c_float * 9)()
    if ctx.L.ctt_hip_eth_kzg_last_cell_timings(ctx.handle, ms, 9) != 9:
        raise RuntimeError("ctt_hip_eth_kzg_last_cell_timings: the library does not report the cell-proof path")
    return ("table" if int(ms[7]) == CELLS_PER_EXT_BLOB else "loop"), float(ms[8])


# the reference's _parallel forms (ethereum_eip4844_kzg_parallel.nim: `tp` first): the same GPU path, the thread pool is not used
def blob_to_kzg_commitment_parallel(tp, ctx: EthereumKZGContext, blob: bytes) -> bytes:
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    out = (ctypes.c_uint8 * 48)()
    _check(ctx.L.ctt_eth_kzg_blob_to_kzg_commitment_parallel(tp, ctx.handle, out, _buf(blob)))
    return bytes(out)


def compute_kzg_proof_parallel(tp, ctx: EthereumKZGContext, blob: bytes, z_bytes: bytes):
    if len(blob) != BYTES_PER_BLOB or len(z_bytes) != 32:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    proof, y = (ctypes.c_uint8 * 48)(), (ctypes.c_uint8 * 32)()
    _check(ctx.L.ctt_eth_kzg_compute_kzg_proof_parallel(tp, ctx.handle, proof, y, _buf(blob), _buf(z_bytes)))
    return bytes(proof), bytes(y)


def compute_blob_kzg_proof_parallel(tp, ctx: EthereumKZGContext, blob: bytes, commitment_bytes: bytes) -> bytes:
    if len(blob) != BYTES_PER_BLOB or len(commitment_bytes) != 48:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    proof = (ctypes.c_uint8 * 48)()
    _check(ctx.L.ctt_eth_kzg_compute_blob_kzg_proof_parallel(tp, ctx.handle, proof, _buf(blob), _buf(commitment_bytes)))
    return bytes(proof)


# ---- the host-only pieces of the library (no GPU), as the tests reach them ----------------------------------------------------
def g1_decompress(b48: bytes) -> bytes:
    """ctt_hip_bls12_381_g1_decompress: 48 compressed bytes -> affine Montgomery {x, y} (96 bytes, (0,0) = neutral)."""
    if len(b48) != 48:
        raise KzgError(cttEthKzgStatus.cttEthKzg_EccInvalidEncoding)
    out = (ctypes.c_uint8 * 96)()
    _check(_lib.lib().ctt_hip_bls12_381_g1_decompress(out, _buf(b48)))
    return bytes(out)


def g1_compress(aff96: bytes) -> bytes:
    out = (ctypes.c_uint8 * 48)()
    _lib.lib().ctt_hip_bls12_381_g1_compress(out, _buf(aff96))
    return bytes(out)


def blob_to_bigint_polynomial(blob: bytes) -> np.ndarray:
    """ctt_hip_eth_kzg_blob_to_scalars: 4096 big-endian scalars -> (4096, 32) little-endian BigInt[255]; each must be < r."""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgError(cttEthKzgStatus.cttEthKzg_InputsLengthsMismatch)
    out = np.zeros((FIELD_ELEMENTS_PER_BLOB, 32), dtype=np.uint8)
    _check(_lib.lib().ctt_hip_eth_kzg_blob_to_scalars(ptr(out), _buf(blob)))
    return out


def compute_challenge(blob: bytes, commitment_bytes: bytes) -> bytes:
    """ctt_hip_eth_kzg_challenge -> 32 big-endian bytes"""
    assert len(blob) == BYTES_PER_BLOB and len(commitment_bytes) == 48
    z = (ctypes.c_uint8 * 32)()
    _lib.lib().ctt_hip_eth_kzg_challenge(z, _buf(blob), _buf(commitment_bytes))
    return bytes(z)


def quotient_polynomial_host(poly_le: np.ndarray, z: int):
    """ctt_hip_eth_kzg_quotient_host -> (q as (4096, 32) uint8 little-endian, y as int)"""
    poly_le = np.ascontiguousarray(poly_le, dtype=np.uint8)
    assert poly_le.shape == (FIELD_ELEMENTS_PER_BLOB, 32)
    q = np.zeros_like(poly_le)
    y = (ctypes.c_uint8 * 32)()
    _lib.lib().ctt_hip_eth_kzg_quotient_host(ptr(q), y, ptr(poly_le), _buf(z.to_bytes(32, "little")))
    return q, int.from_bytes(bytes(y), "little")


def sha256(data: bytes) -> bytes:
    out = (ctypes.c_uint8 * 32)()
    _lib.lib().ctt_hip_sha256(out, _buf(data) if data else None, len(data))
    return bytes(out)
