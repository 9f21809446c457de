/* ctt_msm_hip_peerdas_verify.h -- EIP-7594 (PeerDAS) verify_cell_kzg_proof_batch on the GPU, with the one pairing check on the host:
 * libctt_msm_hip_peerdas_verify.so, a companion of libctt_msm_hip.so built over its public C ABI (ctt_hip_msm_ctx_create,
 * ctt_hip_msm_stream, ctt_hip_fr_ntt*, ctt_hip_subgroup_check, ctt_hip_msm_device, ctt_hip_sha256) with three kernels of its own.
 * Link both; the companion finds the main library next to itself ($ORIGIN).
 *
 * A node checks that cells belong to their blobs' commitments, for every column sidecar of every slot:
 *   include/constantine/protocols/ethereum_eip7594_peerdas.h:63   ctt_eth_kzg_verify_cell_kzg_proof_batch
 * (constantine/eth_eip7594_peerdas.nim:512-619).  A batch of any size costs two Miller loops and one final exponentiation, done on
 * the host; what grows with the batch runs on the device: the decompression of the M unique commitments and the N proofs (a square
 * root in Fp per lane), their subgroup checks, the validation of the N * 64 scalars, one inverse transform of 64 points per column,
 * and two MSMs of N and M + 64 + N points.
 *
 * The reference-named ctt_eth_kzg_verify_cell_kzg_proof_batch(ctx, ...) is NOT provided: the main library's KZG context keeps only the
 * Lagrange G1 section of the trusted setup, and verification needs the first 64 monomial G1 points and [tau^64]_2, which the
 * verifier object below owns.
 *
 * Input: n cells.  commitments: n * 48 bytes (the commitment of each cell's blob; equal ones are deduplicated on their bytes);
 * cell_indices[n], each < 128; cells: n * 2048 bytes (64 big-endian scalars); proofs: n * 48 bytes; secure_random_bytes[32]: the
 * challenge r as a big-endian integer mod r -- all zero, or zero mod r: r is the Fiat-Shamir challenge of the consensus spec
 * (compute_verify_cell_kzg_proof_batch_challenge).  Cell k is weighted by r^(k+1).  Checked in the reference's order; the device
 * checks all items at once and the answer is the status of the first offender in that order:
 *   a NULL verifier                                               cttEthKzg_InputsLengthsMismatch
 *   n == 0                                                        cttEthKzg_Success
 *   a NULL pointer, n > 2^20, an index >= 128                     cttEthKzg_InputsLengthsMismatch
 *   the unique commitments in first-occurrence order, each:       cttEthKzg_EccInvalidEncoding, _EccCoordinateGreaterThanOrEqualModulus,
 *     encoding, x < p, on the curve, in the subgroup                _EccPointNotOnCurve, _EccPointNotInSubgroup  (the neutral is accepted)
 *   an element >= r, cells in input order                         cttEthKzg_ScalarLargerThanCurveOrder
 *   the proofs in input order, as the commitments
 * then cttEthKzg_Success or cttEthKzg_VerificationFailure.  A call the GPU cannot serve returns CTT_HIP_STATUS_GPU_UNAVAILABLE
 * (0xF0).  Nothing terminates the process. */
#ifndef CTT_MSM_HIP_PEERDAS_VERIFY_H
#define CTT_MSM_HIP_PEERDAS_VERIFY_H
#include "ctt_msm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One verifier = an MSM context of its own on `device`, a transform plan of 64 points, the 64 monomial G1 points and a table of 128 x 64
 * scalars on the device, [tau^64]_2 on the host, and a workspace that only grows (about 2.5 KiB per cell) and is freed with the object.
 * g1_monomial_64: the first 64 monomial G1 points of the trusted setup, 64 x 48 bytes compressed; g2_tau64: its G2 point number 64,
 * 96 bytes compressed.  create_from_file reads both from a file in the c-kzg text format (the reference's
 * trusted_setup_ethereum_kzg4844_reference.dat).  All 65 points are decompressed and subgroup-checked; the neutral is refused.  NULL on
 * any failure -- a NULL argument, an unreadable or malformed file, a bad point, no usable device.  Calls on one object serialise. */
typedef struct ctt_hip_peerdas_verifier ctt_hip_peerdas_verifier;
ctt_hip_peerdas_verifier* ctt_hip_peerdas_verifier_create(int device, const uint8_t* g1_monomial_64, const uint8_t* g2_tau64);
ctt_hip_peerdas_verifier* ctt_hip_peerdas_verifier_create_from_file(int device, const char* path);
void ctt_hip_peerdas_verifier_destroy(ctt_hip_peerdas_verifier* v);

/* Returns a ctt_eth_kzg_status value or CTT_HIP_STATUS_GPU_UNAVAILABLE. */
int ctt_hip_peerdas_verify_cell_kzg_proof_batch(ctt_hip_peerdas_verifier* v, const uint8_t* commitments, const uint64_t* cell_indices,
                                                const uint8_t* cells, const uint8_t* proofs, size_t n,
                                                const uint8_t secure_random_bytes[32]);

/* test-facing.
 * verify_challenge (host only, no object): the Fiat-Shamir challenge over m already deduplicated commitments and the index of each
 *   cell's commitment among them, 32 big-endian bytes; cttEthKzg_Success, or cttEthKzg_InputsLengthsMismatch for a NULL pointer.
 * verify_lincombs: the same inputs and checks as the call above, without the pairing: the two sides of the equation, compressed,
 *   ll = sum r^(k+1) proof_k and rl = sum w_i C_i - [sum r^(k+1) I_k(tau)]_1 + sum r^(k+1) h_k^64 proof_k, and r (32 big-endian
 *   bytes).  Written on cttEthKzg_Success only, and not for n == 0.
 * pairing_check (host only): 1 when the product of e(P_i, Q_i) over n pairs is 1, else 0; -1 for a NULL pointer.  g1_aff: n x 96 bytes,
 *   g2_aff: n x 192 bytes, affine Montgomery coordinates in the C-API layout (the neutral all zero, contributing 1).  The points are
 *   taken as members of G1 and G2.  The final exponentiation raises to (p^12 - 1)/r exactly.
 * last_timings: host-clock ms of the object's last call -- [0] checks, challenge + upload, [1] decompress, [2] subgroup check,
 *   [3] colsum + transform + interp, [4] the two MSMs, [5] pairing (0 for lincombs); returns the number written. */
int ctt_hip_peerdas_verify_challenge(uint8_t r_be[32], const uint8_t* commitments, size_t m, const uint64_t* commitment_indices,
                                     const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n);
int ctt_hip_peerdas_verify_lincombs(ctt_hip_peerdas_verifier* v, uint8_t ll[48], uint8_t rl[48], uint8_t r_be[32],
                                    const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs,
                                    size_t n, const uint8_t secure_random_bytes[32]);
int ctt_hip_peerdas_pairing_check(const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n);
int ctt_hip_peerdas_verify_last_timings(const ctt_hip_peerdas_verifier* v, float* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* CTT_MSM_HIP_PEERDAS_VERIFY_H */
