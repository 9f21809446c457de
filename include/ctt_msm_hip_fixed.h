/* ctt_msm_hip_fixed.h -- batched fixed-base MSM over BLS12-381 G1 and BN254 G1 on the GPU: libctt_msm_hip_fixed.so, a companion of
 * libctt_msm_hip.so with kernels of its own (link both, or this one alone; include/ctt_msm_hip.h has the types and the curve ids).
 *
 * m MSMs over one fixed set of n <= 65536 points in one pass: a table of window multiples of every point is built once
 * (the reference's fixed-base precomputed MSM, ec_multi_scalar_mul_precomp.nim), and every (row, point) pair then costs one mixed
 * addition per window -- no sort, no buckets, no reduction passes, no tickets.  It pays where the engine's MSM is launch-bound: many
 * MSMs of a few thousand pairs over the same points, the cell proofs of EIP-7594 for instance.
 *
 *   table      for base i, window w of the balanced Booth layout of c-bit windows and j = 1 .. 2^(width(w)-1) the affine point
 *              j * 2^off(w) * P_i: n * W * 2^(c-1) records (about) of 96 bytes (BLS12-381) or 64 bytes (BN254), in device memory.
 *   return     0; -1 refused (an argument, checked before anything is launched); -2 the allocation of the table or of the workspace
 *              failed; -3 a HIP call failed or there is no usable device.  ctt_hip_fixed_last_error() is the code of the calling
 *              thread's last refused call (create returns NULL and leaves it there).  Outputs are written only on 0.  Nothing here
 *              terminates the process.
 *   threads    a handle serves one call at a time (it owns one stream and one workspace); different handles are independent. */
#ifndef CTT_MSM_HIP_FIXED_H
#define CTT_MSM_HIP_FIXED_H

#include "ctt_msm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CTT_HIP_FIXED_COEFS_ON_DEVICE = 1, CTT_HIP_FIXED_OUT_ON_DEVICE = 2 };   /* flags of ctt_hip_fixed_msm_batch */

typedef struct ctt_hip_fixed_bases ctt_hip_fixed_bases;

/* curve: CTT_HIP_BLS12_381_G1 or CTT_HIP_BN254_SNARKS_G1.  points_aff: n affine points in the C-API layout (x, y Montgomery; (0, 0) is
 * the neutral), host or device memory, 1 <= n <= 65536; they are not checked to be on the curve.  c: window bits, 2 .. 12, or 0 for the
 * default.  While the table is built 2.5 times its size is allocated. */
ctt_hip_fixed_bases* ctt_hip_fixed_bases_create(int device, int curve, const void* points_aff, size_t n, int c);
void ctt_hip_fixed_bases_destroy(ctt_hip_fixed_bases* bases);
/* info: n, c, the number of windows W, records per base, table bytes, microseconds the build took */
int ctt_hip_fixed_bases_info(const ctt_hip_fixed_bases* bases, size_t info[6]);
/* out_aff[k] = sum_i coefs[k][i] * P_i for k < m.  coefs: m rows of n scalars, row-major, 32 bytes each -- CTT_HIP_COEF_BIG: canonical
 * little-endian, any value below 2^255 (BN254: 2^254), not reduced mod r; CTT_HIP_COEF_FR: Montgomery residues of the scalar field.
 * out_aff: m affine points (x, y Montgomery), the neutral as (0, 0).  m >= 1, m * n * 32 < 2^31 and m * ceil(n / 256) < 2^24 (one
 * launch has fewer than 2^32 work-items; this only excludes n <= 3 with m >= 2^24): anything else is refused with -1.  flags: which of
 * coefs and out_aff are device pointers; the call returns when out_aff is written. */
int ctt_hip_fixed_msm_batch(ctt_hip_fixed_bases* bases, int coef_kind, const void* coefs, size_t m, void* out_aff, int flags);
/* device times (ms) of the handle's last successful batch: the sum kernel, the finish */
int ctt_hip_fixed_last_timings(const ctt_hip_fixed_bases* bases, float ms[2]);
int ctt_hip_fixed_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
