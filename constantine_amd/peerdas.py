"""
EIP-7594 (PeerDAS) recovery on the GPU, batched over the blobs of a block: ctypes callers of libctt_msm_hip_peerdas.so
(include/ctt_msm_hip_peerdas.h, constantine_amd/csrc/recover.hip; the formulas: DESIGN.md section 15) -- and batch verification of
cells against their commitments, libctt_msm_hip_peerdas_verify.so (include/ctt_msm_hip_peerdas_verify.h,
constantine_amd/csrc/verify.hip).

    Recovery(device).recover_blobs(cell_indices, cells)                        the blobs alone: field arithmetic, no SRS
    Recovery(device).recover_cells_and_kzg_proofs(ctx, cell_indices, cells)    all 128 cells and proofs of every blob
    kzg.recover_cells_and_kzg_proofs(ctx, cell_indices, cells)                 the reference's own symbol, one blob
    Verifier(device, trusted_setup=path).verify(commitments, cell_indices, cells, proofs)    verify_cell_kzg_proof_batch -> bool

`cells` is one blob's cells -- a sequence of len(cell_indices) byte strings of 2048, or an array (n, 2048) -- or a batch with a leading
axis, (B, n, 2048): every blob of a batch comes with the same cell indices, as the columns a node holds do.  Nothing is computed in
Python; the checks this module adds are the counts and byte lengths, which the C signatures fix by type.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._arrays import ptr
from .kzg import BYTES_PER_BLOB, BYTES_PER_CELL, CELLS_PER_EXT_BLOB, KzgError, cttEthKzgStatus

COEFFICIENTS_PER_EXT_BLOB = 8192
MAX_BLOBS = 4096


def _check(rc, what="EIP-7594 recovery"):
    if rc == _lib.GPU_UNAVAILABLE:
        raise _lib.GpuUnavailable(what)
    if rc != 0:
        raise KzgError(cttEthKzgStatus(rc))


def pack_cells(cell_indices, cells):
    """-> (indices as uint64 (n,), cells as uint8 (B, n, 2048), batched?); ValueError when the counts or a cell's length do not fit"""
    idx = np.ascontiguousarray(np.asarray(list(cell_indices), dtype=np.uint64))
    n = int(idx.shape[0])
    if isinstance(cells, np.ndarray):
        arr = np.ascontiguousarray(cells, dtype=np.uint8)
        batched = arr.ndim == 3
        if arr.ndim not in (2, 3) or arr.shape[-1] != BYTES_PER_CELL:
            raise ValueError(f"cells: expected (n, {BYTES_PER_CELL}) or (B, n, {BYTES_PER_CELL}) bytes, got {arr.shape}")
        if not batched:
            arr = arr[None]
    else:
        rows = list(cells)
        batched = bool(rows) and not isinstance(rows[0], (bytes, bytearray, memoryview))
        if not batched:
            rows = [rows]
        rows = [list(r) for r in rows]
        if any(len(c) != BYTES_PER_CELL for r in rows for c in r):
            raise ValueError(f"cells: every cell is {BYTES_PER_CELL} bytes")
        if any(len(r) != n for r in rows):
            raise ValueError(f"cells: {n} cell indices, but {sorted({len(r) for r in rows})} cells")
        arr = np.frombuffer(b"".join(bytes(c) for r in rows for c in r), dtype=np.uint8).reshape(len(rows), n, BYTES_PER_CELL)
    if arr.shape[1] != n:
        raise ValueError(f"cells: {n} cell indices, but {arr.shape[1]} cells")
    return idx, arr, batched


class Recovery:
    """ctt_hip_peerdas_recovery: an MSM context of its own on `device`, two transform plans and a grow-only workspace."""

    def __init__(self, device=0):
        self.L = _lib.peerdas_lib()
        self.handle = self.L.ctt_hip_peerdas_recovery_create(int(device))
        if not self.handle:
            raise _lib.GpuUnavailable("PeerDAS recovery")

    def delete(self):
        if self.handle:
            self.L.ctt_hip_peerdas_recovery_destroy(self.handle)
            self.handle = None

    def _idx(self, idx):
        return idx.ctypes.data_as(_lib.pu64)

    def recover_blobs(self, cell_indices, cells):
        """-> (blobs, consistent): one blob's 131072 bytes and a bool, or for a batch uint8 (B, 131072) and bool (B,).  consistent is
        False when the cells (more than 64 of them) are not evaluations of one polynomial of degree < 4096; the blob is then that of
        the recovered polynomial truncated to 4096 coefficients."""
        idx, arr, batched = pack_cells(cell_indices, cells)
        B = arr.shape[0]
        blobs = np.zeros((B, BYTES_PER_BLOB), dtype=np.uint8)
        ok = np.zeros(max(B, 1), dtype=np.uint8)
        _check(self.L.ctt_hip_peerdas_recover_blobs(self.handle, ptr(blobs), ptr(ok), self._idx(idx), ptr(arr), idx.shape[0], B))
        if batched:
            return blobs, ok[:B].astype(bool)
        return blobs[0].tobytes(), bool(ok[0])

    def recover_coefficients(self, cell_indices, cells):
        """test-facing: -> (uint8 (B, 8192, 32) canonical little-endian coefficients before the truncation, bool (B,))"""
        idx, arr, _batched = pack_cells(cell_indices, cells)
        B = arr.shape[0]
        coefs = np.zeros((B, COEFFICIENTS_PER_EXT_BLOB, 32), dtype=np.uint8)
        ok = np.zeros(max(B, 1), dtype=np.uint8)
        _check(self.L.ctt_hip_peerdas_recover_coefficients(self.handle, ptr(coefs), ptr(ok), self._idx(idx), ptr(arr), idx.shape[0], B))
        return coefs, ok[:B].astype(bool)

    def recover_cells_and_kzg_proofs(self, ctx, cell_indices, cells):
        """-> (128 cells, 128 proofs) as lists of bytes, or for a batch uint8 (B, 128, 2048) and (B, 128, 48)"""
        idx, arr, batched = pack_cells(cell_indices, cells)
        B = arr.shape[0]
        out_c = np.zeros((B, CELLS_PER_EXT_BLOB, BYTES_PER_CELL), dtype=np.uint8)
        out_p = np.zeros((B, CELLS_PER_EXT_BLOB, 48), dtype=np.uint8)
        _check(self.L.ctt_hip_eth_kzg_recover_cells_and_kzg_proofs_batch(self.handle, ctx.handle, ptr(out_c), ptr(out_p), self._idx(idx), ptr(arr),
                                                                          idx.shape[0], B))
        if batched:
            return out_c, out_p
        return [out_c[0, k].tobytes() for k in range(CELLS_PER_EXT_BLOB)], [out_p[0, k].tobytes() for k in range(CELLS_PER_EXT_BLOB)]

    def last_timings(self):
        """host-clock ms of the last call: checks + upload, the three transforms of 8192, the element-wise kernels, the transform of
        4096 + copy back, the prover"""
        ms = (ctypes.c_float * 5)()
        self.L.ctt_hip_peerdas_last_timings(self.handle, ms, 5)
        return list(ms)


def recovery_constants(cell_indices):
    """test-facing, host only: -> (zc, izc5), 128 integers each: the vanishing polynomial of the missing cells on every cell of the domain,
    and the inverse of its value on every cell of the coset 5 * <omega_8192>"""
    idx = np.ascontiguousarray(np.asarray(list(cell_indices), dtype=np.uint64))
    zc = np.zeros((CELLS_PER_EXT_BLOB, 32), dtype=np.uint8)
    iz = np.zeros((CELLS_PER_EXT_BLOB, 32), dtype=np.uint8)
    _check(_lib.peerdas_lib().ctt_hip_peerdas_recovery_constants(ptr(zc), ptr(iz), idx.ctypes.data_as(_lib.pu64), idx.shape[0]))
    return ([int.from_bytes(zc[k].tobytes(), "little") for k in range(CELLS_PER_EXT_BLOB)],
            [int.from_bytes(iz[k].tobytes(), "little") for k in range(CELLS_PER_EXT_BLOB)])


# ---- verify_cell_kzg_proof_batch --------------------------------------------------------------------------------------------------
def _rows(items, width, what):
    """a sequence of byte strings of `width`, or an array (n, width) -> uint8 (n, width); ValueError when a length does not fit"""
    if isinstance(items, np.ndarray):
        arr = np.ascontiguousarray(items, dtype=np.uint8)
        if arr.ndim != 2 or arr.shape[1] != width:
            raise ValueError(f"{what}: expected (n, {width}) bytes, got {arr.shape}")
        return arr
    rows = [bytes(x) for x in items]
    if any(len(x) != width for x in rows):
        raise ValueError(f"{what}: every item is {width} bytes")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width)


def _pack_batch(commitments, cell_indices, cells, proofs):
    idx = np.ascontiguousarray(np.asarray(list(cell_indices), dtype=np.uint64))
    com, cel, prf = _rows(commitments, 48, "commitments"), _rows(cells, BYTES_PER_CELL, "cells"), _rows(proofs, 48, "proofs")
    n = int(idx.shape[0])
    if not (com.shape[0] == cel.shape[0] == prf.shape[0] == n):
        raise ValueError(f"{com.shape[0]} commitments, {n} cell indices, {cel.shape[0]} cells, {prf.shape[0]} proofs")
    return idx, com, cel, prf


def _random_bytes(random_bytes):
    rnd = bytes(32) if random_bytes is None else bytes(random_bytes)
    if len(rnd) != 32:
        raise ValueError("random_bytes: 32 bytes, or None for the Fiat-Shamir challenge")
    return np.frombuffer(rnd, dtype=np.uint8)


class Verifier:
    """ctt_hip_peerdas_verifier: an MSM context of its own on `device`, the verifier's part of the trusted setup (the first 64 monomial G1
    points and [tau^64]_2, from a file in the c-kzg text format or as compressed bytes) and a grow-only workspace."""

    def __init__(self, device=0, trusted_setup=None, g1_monomial=None, g2_tau64=None):
        self.L = _lib.verify_lib()
        if trusted_setup is not None:
            self.handle = self.L.ctt_hip_peerdas_verifier_create_from_file(int(device), os.fsencode(trusted_setup))
        else:
            g1, g2 = bytes(g1_monomial or b""), bytes(g2_tau64 or b"")
            if len(g1) != 64 * 48 or len(g2) != 96:
                raise ValueError("Verifier: trusted_setup=path, or g1_monomial (64 x 48 bytes) and g2_tau64 (96 bytes)")
            self.handle = self.L.ctt_hip_peerdas_verifier_create(int(device), g1, g2)
        if not self.handle:
            raise _lib.GpuUnavailable("PeerDAS verifier (no usable device, or a trusted setup that was refused)")

    def delete(self):
        if self.handle:
            self.L.ctt_hip_peerdas_verifier_destroy(self.handle)
            self.handle = None

    def verify(self, commitments, cell_indices, cells, proofs, random_bytes=None):
        """verify_cell_kzg_proof_batch -> bool.  random_bytes: 32 bytes, the challenge as a big-endian integer mod r; None (or zero): the
        Fiat-Shamir challenge of the consensus spec.  KzgError with the status on invalid input, GpuUnavailable on 0xF0."""
        idx, com, cel, prf = _pack_batch(commitments, cell_indices, cells, proofs)
        rc = self.L.ctt_hip_peerdas_verify_cell_kzg_proof_batch(self.handle, ptr(com), idx.ctypes.data_as(_lib.pu64), ptr(cel), ptr(prf),
                                                                idx.shape[0], ptr(_random_bytes(random_bytes)))
        if rc == cttEthKzgStatus.cttEthKzg_VerificationFailure.value:
            return False
        _check(rc, "EIP-7594 verification")
        return True

    def lincombs(self, commitments, cell_indices, cells, proofs, random_bytes=None):
        """test-facing: -> (LL, RL, r): the two sides of the pairing equation as compressed G1 points and the challenge, after the same
        checks as verify(); (None, None, None) for an empty batch"""
        idx, com, cel, prf = _pack_batch(commitments, cell_indices, cells, proofs)
        ll, rl, r = np.zeros(48, dtype=np.uint8), np.zeros(48, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        _check(self.L.ctt_hip_peerdas_verify_lincombs(self.handle, ptr(ll), ptr(rl), ptr(r), ptr(com), idx.ctypes.data_as(_lib.pu64), ptr(cel),
                                                      ptr(prf), idx.shape[0], ptr(_random_bytes(random_bytes))), "EIP-7594 verification")
        if idx.shape[0] == 0:
            return None, None, None
        return ll.tobytes(), rl.tobytes(), int.from_bytes(r.tobytes(), "big")

    def last_timings(self):
        """host-clock ms of the last call: checks, challenge + upload; decompress; subgroup check; colsum + transform + interp; the two
        MSMs; pairing"""
        ms = (ctypes.c_float * 6)()
        self.L.ctt_hip_peerdas_verify_last_timings(self.handle, ms, 6)
        return list(ms)


def pairing_check(g1_points, g2_points):
    """test-facing, host only: prod e(P_i, Q_i) == 1 for affine Montgomery points in the C-API layout (96 and 192 bytes each)"""
    g1, g2 = _rows(g1_points, 96, "g1_points"), _rows(g2_points, 192, "g2_points")
    if g1.shape[0] != g2.shape[0]:
        raise ValueError("pairing_check: as many G1 as G2 points")
    rc = _lib.verify_lib().ctt_hip_peerdas_pairing_check(ptr(g1), ptr(g2), g1.shape[0])
    if rc < 0:
        raise ValueError("pairing_check: refused")
    return rc == 1


def verify_challenge(commitments, commitment_indices, cell_indices, cells, proofs):
    """test-facing, host only: compute_verify_cell_kzg_proof_batch_challenge over deduplicated commitments -> the integer r"""
    com = _rows(commitments, 48, "commitments")
    cidx = np.ascontiguousarray(np.asarray(list(commitment_indices), dtype=np.uint64))
    idx = np.ascontiguousarray(np.asarray(list(cell_indices), dtype=np.uint64))
    cel, prf = _rows(cells, BYTES_PER_CELL, "cells"), _rows(proofs, 48, "proofs")
    if not (cidx.shape[0] == idx.shape[0] == cel.shape[0] == prf.shape[0]):
        raise ValueError("verify_challenge: one commitment index, cell index, cell and proof per cell")
    r = np.zeros(32, dtype=np.uint8)
    _check(_lib.verify_lib().ctt_hip_peerdas_verify_challenge(ptr(r), ptr(com), com.shape[0], cidx.ctypes.data_as(_lib.pu64),
                                                             idx.ctypes.data_as(_lib.pu64), ptr(cel), ptr(prf), idx.shape[0]))
    return int.from_bytes(r.tobytes(), "big")
