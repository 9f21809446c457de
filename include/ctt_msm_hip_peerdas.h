/* ctt_msm_hip_peerdas.h -- EIP-7594 (PeerDAS) recovery on the GPU, batched over the blobs of a block: libctt_msm_hip_peerdas.so, a
 * companion of libctt_msm_hip.so built over its public C ABI (ctt_hip_msm_ctx_create, ctt_hip_msm_stream, ctt_hip_fr_ntt*,
 * ctt_eth_kzg_compute_cells_and_kzg_proofs) with three element-wise kernels of its own.  Link both; the companion finds the main
 * library next to itself ($ORIGIN).
 *
 * A node that holds at least 64 of the 128 cells (columns) of a blob rebuilds the blob, and from it all cells and cell proofs:
 *   include/constantine/protocols/ethereum_eip7594_peerdas.h:91   ctt_eth_kzg_recover_cells_and_kzg_proofs
 * (constantine/eth_eip7594_peerdas.nim:621-721, constantine/data_availability_sampling/eth_peerdas.nim:132-225).  The vanishing
 * polynomial of the missing cells is a polynomial in X^64 and so one constant per cell, on the domain and on the coset of the division:
 * the device runs three transforms of 8192 points, two element-wise kernels and one transform of 4096 points per blob, for all blobs
 * of a call at once.  The cell proofs are the main library's prover, blob by blob.
 *
 * Input, for B blobs that share one set of n cell indices: cell_indices[n], strictly ascending, each < 128, 64 <= n <= 128; cells:
 * B * n cells of 2048 bytes (64 big-endian scalars), blob after blob.  Checked in the reference's order before anything else happens:
 *   a NULL pointer, n < 64, n > 128, B > 4096       cttEthKzg_InputsLengthsMismatch
 *   an index >= 128 (every index, first)            cttEthKzg_InputsLengthsMismatch
 *   not strictly ascending                          cttEthKzg_CellIndicesNotAscending
 *   an element >= r (cells in input order)          cttEthKzg_ScalarLargerThanCurveOrder
 * B == 0 returns Success and writes nothing.  A call the GPU cannot serve returns CTT_HIP_STATUS_GPU_UNAVAILABLE (0xF0).  Outputs are
 * written only when the whole call succeeded; nothing terminates the process.
 *
 * Inconsistent input -- cells that are not the evaluations of ONE polynomial of degree < 4096, possible only with n > 64: as the
 * consensus spec and c-kzg do, the recovered polynomial is truncated to 4096 coefficients, and blob, cells and proofs are those of the
 * truncated polynomial (so the returned cells need not equal the given ones).  The reference computes the cells from all 8192
 * coefficients and the proofs from the first 4096.  The two agree on every consistent input and on all of the reference's vectors.
 * recover_blobs reports the case: consistent[b] == 0. */
#ifndef CTT_MSM_HIP_PEERDAS_H
#define CTT_MSM_HIP_PEERDAS_H
#include "ctt_msm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One recovery object = an MSM context of its own on `device`, two transform plans (8192 and 4096 points) and a workspace that only
 * grows (B * 384 KiB + the cells) and is freed with the object.  It needs no SRS: recovering blobs is field arithmetic.  Calls on one
 * object serialise.  NULL when the device cannot be used. */
typedef struct ctt_hip_peerdas_recovery ctt_hip_peerdas_recovery;
ctt_hip_peerdas_recovery* ctt_hip_peerdas_recovery_create(int device);
void ctt_hip_peerdas_recovery_destroy(ctt_hip_peerdas_recovery* rec);

/* The data alone: blobs = B x 131072 bytes; consistent (B bytes, or NULL) = 1 when the upper half of the 8192 recovered coefficients
 * is zero -- with more than 64 cells a 0 proves that the cells do not belong to one blob (with exactly 64 it is always 1).
 * Returns a ctt_eth_kzg_status value or CTT_HIP_STATUS_GPU_UNAVAILABLE. */
int ctt_hip_peerdas_recover_blobs(ctt_hip_peerdas_recovery* rec, uint8_t* blobs, uint8_t* consistent, const uint64_t* cell_indices,
                                  const uint8_t* cells, size_t n, size_t B);

/* All 128 cells and proofs of B blobs: recover_blobs, then ctt_eth_kzg_compute_cells_and_kzg_proofs(ctx, ...) per blob.  The blobs are
 * handed over in host memory, so the KZG context may live on any device and serves its other callers unchanged.  cells_out: B x 128,
 * proofs_out: B x 128. */
ctt_eth_kzg_status ctt_hip_eth_kzg_recover_cells_and_kzg_proofs_batch(ctt_hip_peerdas_recovery* rec, const ctt_eth_kzg_context* ctx,
                                                                      ctt_eth_kzg_cell* cells_out, ctt_eth_kzg_proof* proofs_out,
                                                                      const uint64_t* cell_indices, const ctt_eth_kzg_cell* cells,
                                                                      size_t n, size_t B);

/* The reference's name and signature, over a process-wide recovery object on device $CTT_HIP_DEVICE (default 0), created at the
 * first call that passes the input checks. */
ctt_eth_kzg_status ctt_eth_kzg_recover_cells_and_kzg_proofs(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_cell* recovered_cells,
                                                            ctt_eth_kzg_proof* recovered_proofs, const uint64_t* cell_indices,
                                                            const ctt_eth_kzg_cell* cells, size_t num_cells);

/* test-facing.  recover_coefficients: the B x 8192 coefficients of the recovered polynomials before the truncation, canonical
 * little-endian scalars (the transforms of 8192 points and the three kernels alone); consistent as above.  recovery_constants (host
 * only, no object): for a valid index set, the value of the vanishing polynomial on each cell, zc[128] (0 exactly on the missing
 * cells), and the inverse of its value on each cell of the coset 5 * <omega_8192>, izc5[128], canonical little-endian scalars.
 * last_timings: host-clock ms of the object's last call -- [0] checks + upload, [1] the three transforms of 8192, [2] the three
 * element-wise kernels, [3] the transform of 4096 + copy back, [4] the prover (0 for recover_blobs); returns the number written. */
int ctt_hip_peerdas_recover_coefficients(ctt_hip_peerdas_recovery* rec, uint8_t* coefs_le, uint8_t* consistent,
                                         const uint64_t* cell_indices, const uint8_t* cells, size_t n, size_t B);
int ctt_hip_peerdas_recovery_constants(uint8_t* zc_le, uint8_t* izc5_le, const uint64_t* cell_indices, size_t n);
int ctt_hip_peerdas_last_timings(const ctt_hip_peerdas_recovery* rec, float* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* CTT_MSM_HIP_PEERDAS_H */
