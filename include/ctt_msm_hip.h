/* ctt_msm_hip.h -- C ABI of libctt_msm_hip.so, the MI355X (gfx950) multi-scalar-multiplication engine.
 *
 * Part 1 re-declares, with identical names, argument order and struct layouts, the MSM symbols of the
 * reference's generated C API, so the library can be linked in place of libconstantine for this path:
 *
 *   serial   : bindings/c_curve_decls.nim:418-431           -> include/constantine/curves/bls12_381.h:163-164,184-185,212-213,233-234
 *                                                               include/constantine/curves/bn254_snarks.h:163-164,184-185,212-213,233-234
 *                                                               include/constantine/curves/pallas.h:125-126,146-147
 *                                                               include/constantine/curves/vesta.h:125-126,146-147
 *   parallel : bindings/c_curve_decls_parallel.nim:33-45    -> include/constantine/curves/{bls12_381,bn254_snarks,pallas,vesta}_parallel.h:20-23
 *
 * All pointers are HOST pointers, buffers are caller-owned, `r` is out-only, the functions block until the
 * result is written, return void and never report an error (same contract as the reference); there is no CPU
 * fallback, so a call of these `void` symbols that the GPU cannot serve aborts with a diagnostic.  Every symbol with a
 * return value -- the neutral spellings of the same MSM (Part 1c), Part 2, and the protocol symbols of Part 3 --
 * reports a GPU refusal through it instead and never aborts (round 5; ctt_hip_last_error() says why).  `tp` is accepted and ignored (the GPU
 * replaces the thread pool).  len == 0 yields the neutral element (undefined behaviour upstream).
 * The result is the same group element as the reference's; its (X,Y,Z) representative is the canonical one
 * with Z = 1 (neutral: jac (1,1,0), prj (0,1,0)).
 *
 * Part 2 is the device-resident interface (inputs already in HBM): the hook for Halo2-ZAL style cached bases
 * (constantine-rust/constantine-halo2-zal/src/lib.rs:60-95) and what bench.py times.
 */
#ifndef CTT_MSM_HIP_H
#define CTT_MSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types: layout-compatible with include/constantine/core/datatypes.h:42-50, curves/bigints.h:18-21,
 *      curves/bls12_381.h:19-27, bn254_snarks.h:19-27, pallas.h:19-24, vesta.h:19-24 ---------------------- */
#ifndef CTT_MSM_HIP_NO_TYPES
typedef size_t secret_word;
#define CTT_WORD_BITWIDTH (sizeof(secret_word) * 8)
#define CTT_WORDS_REQUIRED(bits) (((bits) + CTT_WORD_BITWIDTH - 1) / CTT_WORD_BITWIDTH)

typedef struct ctt_threadpool ctt_threadpool; /* opaque, core/threadpool.h:21 */

typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } big255;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(254)]; } big254;

typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } bls12_381_fr;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(381)]; } bls12_381_fp;
typedef struct { bls12_381_fp c[2]; } bls12_381_fp2;
typedef struct { bls12_381_fp x, y; } bls12_381_g1_aff;
typedef struct { bls12_381_fp x, y, z; } bls12_381_g1_jac;
typedef struct { bls12_381_fp x, y, z; } bls12_381_g1_prj;
typedef struct { bls12_381_fp2 x, y; } bls12_381_g2_aff;
typedef struct { bls12_381_fp2 x, y, z; } bls12_381_g2_jac;
typedef struct { bls12_381_fp2 x, y, z; } bls12_381_g2_prj;

typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(254)]; } bn254_snarks_fr;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(254)]; } bn254_snarks_fp;
typedef struct { bn254_snarks_fp c[2]; } bn254_snarks_fp2;
typedef struct { bn254_snarks_fp x, y; } bn254_snarks_g1_aff;
typedef struct { bn254_snarks_fp x, y, z; } bn254_snarks_g1_jac;
typedef struct { bn254_snarks_fp x, y, z; } bn254_snarks_g1_prj;
typedef struct { bn254_snarks_fp2 x, y; } bn254_snarks_g2_aff;
typedef struct { bn254_snarks_fp2 x, y, z; } bn254_snarks_g2_jac;
typedef struct { bn254_snarks_fp2 x, y, z; } bn254_snarks_g2_prj;

typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } pallas_fr;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } pallas_fp;
typedef struct { pallas_fp x, y; } pallas_ec_aff;
typedef struct { pallas_fp x, y, z; } pallas_ec_jac;
typedef struct { pallas_fp x, y, z; } pallas_ec_prj;

typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } vesta_fr;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } vesta_fp;
typedef struct { vesta_fp x, y; } vesta_ec_aff;
typedef struct { vesta_fp x, y, z; } vesta_ec_jac;
typedef struct { vesta_fp x, y, z; } vesta_ec_prj;
#endif /* CTT_MSM_HIP_NO_TYPES */

/* ---- Part 1: Constantine-compatible MSM symbols -------------------------------------------------------- */
#define CTT_MSM_DECL_SERIAL(EC, AFF, BIG, FR)                                                                      \
  void ctt_##EC##_multi_scalar_mul_big_coefs_vartime(EC* r, const BIG coefs[], const AFF points[], size_t len);    \
  void ctt_##EC##_multi_scalar_mul_fr_coefs_vartime(EC* r, const FR coefs[], const AFF points[], size_t len);
#define CTT_MSM_DECL_PARALLEL(EC, AFF, BIG, FR)                                                                    \
  void ctt_##EC##_multi_scalar_mul_big_coefs_vartime_parallel(const ctt_threadpool* tp, EC* r, const BIG coefs[],  \
                                                              const AFF points[], size_t len);                     \
  void ctt_##EC##_multi_scalar_mul_fr_coefs_vartime_parallel(const ctt_threadpool* tp, EC* r, const FR coefs[],    \
                                                             const AFF points[], size_t len);

/* bls12_381.h:163-164,184-185 ; bls12_381_parallel.h:20-23 */
CTT_MSM_DECL_SERIAL(bls12_381_g1_jac, bls12_381_g1_aff, big255, bls12_381_fr)
CTT_MSM_DECL_SERIAL(bls12_381_g1_prj, bls12_381_g1_aff, big255, bls12_381_fr)
CTT_MSM_DECL_PARALLEL(bls12_381_g1_jac, bls12_381_g1_aff, big255, bls12_381_fr)
CTT_MSM_DECL_PARALLEL(bls12_381_g1_prj, bls12_381_g1_aff, big255, bls12_381_fr)
/* bls12_381.h:212-213,233-234 (G2 has no parallel variant upstream) */
CTT_MSM_DECL_SERIAL(bls12_381_g2_jac, bls12_381_g2_aff, big255, bls12_381_fr)
CTT_MSM_DECL_SERIAL(bls12_381_g2_prj, bls12_381_g2_aff, big255, bls12_381_fr)
/* bn254_snarks.h:163-164,184-185,212-213,233-234 ; bn254_snarks_parallel.h:20-23
 * ctt_bn254_snarks_g1_prj_multi_scalar_mul_fr_coefs_vartime_parallel is the Halo2-ZAL entry
 * (constantine-rust/constantine-halo2-zal/src/lib.rs:42-58). */
CTT_MSM_DECL_SERIAL(bn254_snarks_g1_jac, bn254_snarks_g1_aff, big254, bn254_snarks_fr)
CTT_MSM_DECL_SERIAL(bn254_snarks_g1_prj, bn254_snarks_g1_aff, big254, bn254_snarks_fr)
CTT_MSM_DECL_PARALLEL(bn254_snarks_g1_jac, bn254_snarks_g1_aff, big254, bn254_snarks_fr)
CTT_MSM_DECL_PARALLEL(bn254_snarks_g1_prj, bn254_snarks_g1_aff, big254, bn254_snarks_fr)
CTT_MSM_DECL_SERIAL(bn254_snarks_g2_jac, bn254_snarks_g2_aff, big254, bn254_snarks_fr)
CTT_MSM_DECL_SERIAL(bn254_snarks_g2_prj, bn254_snarks_g2_aff, big254, bn254_snarks_fr)
/* pallas.h:125-126,146-147 ; pallas_parallel.h:20-23 */
CTT_MSM_DECL_SERIAL(pallas_ec_jac, pallas_ec_aff, big255, pallas_fr)
CTT_MSM_DECL_SERIAL(pallas_ec_prj, pallas_ec_aff, big255, pallas_fr)
CTT_MSM_DECL_PARALLEL(pallas_ec_jac, pallas_ec_aff, big255, pallas_fr)
CTT_MSM_DECL_PARALLEL(pallas_ec_prj, pallas_ec_aff, big255, pallas_fr)
/* vesta.h:125-126,146-147 ; vesta_parallel.h:20-23 */
CTT_MSM_DECL_SERIAL(vesta_ec_jac, vesta_ec_aff, big255, vesta_fr)
CTT_MSM_DECL_SERIAL(vesta_ec_prj, vesta_ec_aff, big255, vesta_fr)
CTT_MSM_DECL_PARALLEL(vesta_ec_jac, vesta_ec_aff, big255, vesta_fr)
CTT_MSM_DECL_PARALLEL(vesta_ec_prj, vesta_ec_aff, big255, vesta_fr)

/* ---- Part 1b: Constantine-compatible batch conversion to affine (next row) -----------
 * bindings/c_curve_decls.nim:395-396 (`ctt_<EC>_batch_affine`); bls12_381.h:158,179,207,228, bn254_snarks.h:158,179,
 * 207,228, pallas.h:120,141, vesta.h:120,141.  dst[i] = affine(src[i]); a neutral input gives (0,0).  Host pointers. */
#define CTT_BATCH_AFFINE_DECL(EC, AFF) void ctt_##EC##_batch_affine(AFF dst[], const EC src[], size_t n);
CTT_BATCH_AFFINE_DECL(bls12_381_g1_jac, bls12_381_g1_aff)
CTT_BATCH_AFFINE_DECL(bls12_381_g1_prj, bls12_381_g1_aff)
CTT_BATCH_AFFINE_DECL(bls12_381_g2_jac, bls12_381_g2_aff)
CTT_BATCH_AFFINE_DECL(bls12_381_g2_prj, bls12_381_g2_aff)
CTT_BATCH_AFFINE_DECL(bn254_snarks_g1_jac, bn254_snarks_g1_aff)
CTT_BATCH_AFFINE_DECL(bn254_snarks_g1_prj, bn254_snarks_g1_aff)
CTT_BATCH_AFFINE_DECL(bn254_snarks_g2_jac, bn254_snarks_g2_aff)
CTT_BATCH_AFFINE_DECL(bn254_snarks_g2_prj, bn254_snarks_g2_aff)
CTT_BATCH_AFFINE_DECL(pallas_ec_jac, pallas_ec_aff)
CTT_BATCH_AFFINE_DECL(pallas_ec_prj, pallas_ec_aff)
CTT_BATCH_AFFINE_DECL(vesta_ec_jac, vesta_ec_aff)
CTT_BATCH_AFFINE_DECL(vesta_ec_prj, vesta_ec_aff)

/* ---- Part 1c: neutral host-pointer symbols (SURVEY §8b "replacement plan") ----------------------------------------
 * The same host-pointer MSM as Part 1 under names nothing in Constantine exports, for a binding INSIDE libconstantine: the
 * templates of bindings/c_curve_decls.nim:418-431 and bindings/c_curve_decls_parallel.nim:33-45 keep `libExport`ing the
 * ctt_<EC>_multi_scalar_mul_* names and `importc` these (INTEGRATION.md part B), so a static libconstantine.a defines every
 * name once.  Same argument meaning as Part 1 (host pointers, caller-owned, r out-only); the difference is the `int` they
 * return, the error channel the Constantine names lack: 0 = r holds the result; -1 = bad id, len above 2^31-1, or both
 * in-flight slots of the default context taken by tickets of Part 2; -2 = out of device memory.  r is untouched on an error
 * and the binding runs the reference's CPU path instead (also -1, never an abort: no usable HIP device, or a HIP runtime call
 * failed -- ctt_hip_last_error() tells the cases apart).  ctt_hip_msm_available(): 1 when a HIP device is present (the probe
 * a binding makes once), else 0.
 *
 * Why a call was refused -- per thread, set by every symbol of this header that returns an error value (NULL, -1, -2, or Part 3's
 * CTT_HIP_STATUS_GPU_UNAVAILABLE), and cleared when such a symbol is entered (round 6: no stale code of an earlier call):
 *    0 none   -1 refused (bad arguments: curve id, kind, length, ticket, option key, owner)   -2 out of device memory
 *   -5 busy: all in-flight slots of the context are taken -- finish a ticket, or retry (round 6; was -1)
 *   -3 no usable HIP device   -4 a HIP runtime call failed: the context it happened on is LOST -- every later call on it is
 *      refused with -4; destroy it and create a new one (the default context of the host-pointer symbols stays lost) */
int ctt_hip_last_error(void);
const char* ctt_hip_last_error_message(void);   /* the same, in words; valid until the thread's next refused call */
void ctt_hip_clear_last_error(void);
/* CTT_HIP_BANDERWAGON (twisted Edwards; Constantine-named symbols in include/ctt_msm_hip_banderwagon.h): affine and projective
 * output only (CTT_HIP_OUT_JAC is refused with -1), inputs must be valid Banderwagon elements; batch affine, subgroup check, field
 * probe and KZG quotient refuse it with -1 */
enum { CTT_HIP_BLS12_381_G1 = 0, CTT_HIP_BLS12_381_G2 = 1, CTT_HIP_BN254_SNARKS_G1 = 2,
       CTT_HIP_BN254_SNARKS_G2 = 3, CTT_HIP_PALLAS = 4, CTT_HIP_VESTA = 5, CTT_HIP_BANDERWAGON = 6 };
enum { CTT_HIP_COEF_BIG = 0, CTT_HIP_COEF_FR = 1 };
enum { CTT_HIP_OUT_AFF = 0, CTT_HIP_OUT_JAC = 1, CTT_HIP_OUT_PRJ = 2 };
int ctt_hip_msm_available(void);
int ctt_hip_msm_host(int curve, int coef_kind, int out_kind, void* r, const void* coefs, const void* points, size_t len);
#define CTT_HIP_MSM_DECL_NEUTRAL(STEM, AFF, BIG, FR)                                                        \
  int ctt_hip_msm_##STEM##_jac_big(STEM##_jac* r, const BIG coefs[], const AFF points[], size_t len);       \
  int ctt_hip_msm_##STEM##_jac_fr(STEM##_jac* r, const FR coefs[], const AFF points[], size_t len);         \
  int ctt_hip_msm_##STEM##_prj_big(STEM##_prj* r, const BIG coefs[], const AFF points[], size_t len);       \
  int ctt_hip_msm_##STEM##_prj_fr(STEM##_prj* r, const FR coefs[], const AFF points[], size_t len);
CTT_HIP_MSM_DECL_NEUTRAL(bls12_381_g1, bls12_381_g1_aff, big255, bls12_381_fr)
CTT_HIP_MSM_DECL_NEUTRAL(bls12_381_g2, bls12_381_g2_aff, big255, bls12_381_fr)
CTT_HIP_MSM_DECL_NEUTRAL(bn254_snarks_g1, bn254_snarks_g1_aff, big254, bn254_snarks_fr)
CTT_HIP_MSM_DECL_NEUTRAL(bn254_snarks_g2, bn254_snarks_g2_aff, big254, bn254_snarks_fr)
CTT_HIP_MSM_DECL_NEUTRAL(pallas_ec, pallas_ec_aff, big255, pallas_fr)
CTT_HIP_MSM_DECL_NEUTRAL(vesta_ec, vesta_ec_aff, big255, vesta_fr)

/* ---- Part 2: device-resident interface ------------------------------------------------------------------ */
typedef struct ctt_hip_msm_ctx ctt_hip_msm_ctx;


int ctt_hip_msm_abi_version(void);
/* One context = one GPU, its streams, one grow-only workspace. NULL ctx in the calls below = process default
 * context on device $CTT_HIP_DEVICE (default 0). */
ctt_hip_msm_ctx* ctt_hip_msm_ctx_create(int device);
void ctt_hip_msm_ctx_destroy(ctt_hip_msm_ctx* ctx);
/* key: "c" window bits, "K" sorted entries per accumulate lane, "S" scalars per sort-partition workgroup, "chunks" slices a
 * host-pointer call is uploaded in (the upload of slice i+1 runs underneath the accumulation of slice i),
 * "horner_bits" bits per group of the bit Horner the device runs per window (0 = 4; the host joins the groups),
 * "host_window_sums" (legacy spelling: 1 = groups of one bit, 2 = one group per window), "timings" 1 = record the
 * stage events ctt_hip_msm_last_timings reads (2 = the accumulate stage and the total only), "timings_every" k = only every
 * k-th MSM records them (the others report zeros; default 1).  value 0 = automatic / off.  Returns 0, or -1 for an unknown key.
 * Forms the plan otherwise chooses by itself (tests and experiments): "merge_chain" head merge 1 = the queue form always, 2 = the tree
 * always; "merge_lmax" longest chain of heads the queue form walks with one quad (0 = 8; longer chains go to one workgroup per
 * window); "merge_queue_quad" 2 = the queue kernel with one lane per chain instead of four; "early_tail" merge and every reduction
 * pass of a pipelined MSM on the tail stream (0 never, 1 automatic -- the default --, 2 whenever pipelining); "front_side"
 * conversion and sort of a pipelined MSM on the front stream (1 whenever pipelining, 2 never); "pyr0_tail" 1 = the first reduction
 * pass of a small MSM on the tail stream; "glv" the endomorphism split of a device-resident BLS12-381 G1 MSM (0 at the curve's
 * measured sizes, 1 at every size, 2 never; also $CTT_HIP_MSM_GLV); "accum_handover" the priority hand-over between the waves of the
 * accumulate kernel (0 off, 1 the curve's drop distance -- the default --, n >= 2 this many iterations before a wave's end; also
 * $CTT_HIP_MSM_ACCUM_HANDOVER): it moves when the kernel's waves issue, never what they compute.  A context also reads $CTT_HIP_MSM_MERGE_CHAIN, $CTT_HIP_MSM_MERGE_LMAX and
 * $CTT_HIP_MSM_QUAD (reduction passes of at most this many additions run with four lanes per addition) when it is created.
 * A context created with $CTT_HIP_CU_TAIL = r > 0 partitions the chip: its tail stream runs on r compute units of every XCD
 * (hipExtStreamCreateWithCUMask), its main stream on the others -- an experiment of round 6, measured slower than sharing the chip
 * (profiles/cu_mask_r06.txt); such streams are BLOCKING streams: do not order them behind the legacy null stream. */
int ctt_hip_msm_set_option(ctt_hip_msm_ctx* ctx, const char* key, int value);
/* r (HOST memory, `out_kind` layout) = sum coefs[i] * points[i]; d_coefs / d_points are DEVICE pointers
 * (BigInt canonical or Fr Montgomery 32-byte scalars; affine Montgomery points, C-API struct layout).
 * Returns 0; -1 for a bad curve id, len > 2^31-1, or three tickets outstanding on the curve.  Blocks until r is written. */
int ctt_hip_msm_device(ctt_hip_msm_ctx* ctx, int curve, int coef_kind, int out_kind, void* r, const void* d_coefs,
                       const void* d_points, size_t len);
/* Split form: submit enqueues the GPU work of one MSM and returns a ticket (>= 0) at once, or -1 on bad arguments or
 * when three tickets are outstanding on the curve (two in rounds 1-5); finish waits for the ticket, runs the host tail (Horner over
 * windows, affine normalisation) and writes r (0, or -1 for a ticket that is not outstanding).  Submitting MSM i+1 before
 * finishing MSM i overlaps the host tail of i with the GPU work of i+1 (how bench.py keeps the GPU busy); a caller of SMALL MSMs
 * (up to ~2^16 pairs: the host tail and the enqueueing are a third of a step there; above, the third MSM only crowds the second one's tail)
 * keeps three outstanding -- submit i+2, then finish i. */
int ctt_hip_msm_device_submit(ctt_hip_msm_ctx* ctx, int curve, int coef_kind, const void* d_coefs, const void* d_points,
                              size_t len);
int ctt_hip_msm_device_finish(ctt_hip_msm_ctx* ctx, int ticket, int out_kind, void* r);
/* Wait for everything enqueued on the context's streams (the main one and the tail stream that carries the last,
 * latency-bound reduction passes of an MSM underneath the next MSM's conversion and sort). */
void ctt_hip_msm_sync(ctt_hip_msm_ctx* ctx);
/* Stream ordering: the engine's streams are not ordered against the caller's.  When device inputs may still be in
 * flight on `producer` (a hipStream_t), call this first: what the engine enqueues afterwards waits for the work
 * `producer` holds now (a stream of the context's own device).  Device outputs (ctt_hip_batch_affine on device arrays) are
 * complete when their call returns. */
int ctt_hip_msm_wait_stream(ctt_hip_msm_ctx* ctx, void* producer);
/* Multi-GPU: the host-pointer symbols of Part 1 shard a call by points over these devices -- the reference's msm-level
 * split (ec_multi_scalar_mul_parallel.nim:386-431; balanced chunks, threadpool/partitioners.nim:44-77) with GPUs for
 * threads: each slice is uploaded to its own GPU and the partial results are summed on the host.  `n` device ids (an
 * id may repeat: one context each); n < 2 turns sharding off.  Default: $CTT_HIP_DEVICES ("0,1,2,3" or "all"), else
 * off.  Calls below shard_min pairs per device (default 2^15, $CTT_HIP_SHARD_MIN) use fewer devices.
 * Returns 0, or -1 for a device id out of range. */
int ctt_hip_msm_set_devices(const int* devices, int n);
void ctt_hip_msm_set_shard_min(size_t pairs_per_device);
/* Cached bases -- the Halo2-ZAL descriptor hooks (constantine-halo2-zal/src/lib.rs:60-95: get_base_descriptor,
 * msm_with_cached_base): base points are uploaded and converted to the device representation once and stay resident
 * in HBM; later MSMs move only the 32-byte coefficients. `points` / `coefs` are host pointers when the
 * *_on_device flag is 0, device pointers when it is 1. ctt_hip_msm_with_bases uses the first `len` bases and must be
 * called with the context the bases were created on (-1 otherwise: the records live on that context's GPU); destroy the
 * bases before their context. */
typedef struct ctt_hip_msm_bases ctt_hip_msm_bases;
ctt_hip_msm_bases* ctt_hip_msm_bases_create(ctt_hip_msm_ctx* ctx, int curve, const void* points, size_t len,
                                            int points_on_device);
void ctt_hip_msm_bases_destroy(ctt_hip_msm_ctx* ctx, ctt_hip_msm_bases* bases);
int ctt_hip_msm_with_bases(ctt_hip_msm_ctx* ctx, const ctt_hip_msm_bases* bases, int coef_kind, int out_kind, void* r,
                           const void* coefs, size_t len, int coefs_on_device);
/* split form (device-resident coefficients): a ticket for ctt_hip_msm_device_finish, or -1 */
int ctt_hip_msm_with_bases_submit(ctt_hip_msm_ctx* ctx, const ctt_hip_msm_bases* bases, int coef_kind, const void* d_coefs,
                                  size_t len);
/* Cached bases WITH A WINDOW TABLE: besides the bases themselves their multiples 2^(c*w) * P, w = 0 .. bits/c, are computed
 * once and stay resident ((bits/c + 1) x the memory: 1.7 GB for 2^20 BLS12-381 G1 bases at c = 20).  Every Booth digit
 * of every window then selects a table row, all windows share one bucket set, and the window combine (the doublings of
 * ec_multi_scalar_mul.nim:250-254) disappears: a later ctt_hip_msm_with_bases[_submit] call costs bits/c + 1 accumulations
 * per pair with a larger c than the table-less MSM can afford (13 instead of 16 at 2^20 pairs) and ONE bucket reduction.
 * The result is the same group element.  window_bits = 0 chooses c from len; ctt_hip_msm_bases_window_bits returns the c
 * in use (0 = plain records: no c fits the sort's packed records for this len). */
ctt_hip_msm_bases* ctt_hip_msm_bases_create_table(ctt_hip_msm_ctx* ctx, int curve, const void* points, size_t len,
                                                  int points_on_device, int window_bits);
int ctt_hip_msm_bases_window_bits(const ctt_hip_msm_bases* bases);
/* HIP-event stage times (ms) of the last finished MSM: digits, sort, accumulate, merge, reduce, total.  Opt-in: set the
 * option "timings" to 1 first (the events are host time per MSM; without it the call returns zeros). */
int ctt_hip_msm_last_timings(ctt_hip_msm_ctx* ctx, float* ms, int cap);
/* plan of the last call: c, W, K, G, S, resident lanes, bucket sets, split.  W is the accumulations per input pair: the digit windows of
 * the scalar, or -- when the endomorphism split ran (split = 1: BLS12-381 G1, two half scalars per pair) -- twice the bucket sets. */
int ctt_hip_msm_last_plan(ctt_hip_msm_ctx* ctx, int* out, int cap);
/* d_out[i] = [s_i]G, deterministic synthetic subgroup points (bench / test inputs) */
int ctt_hip_gen_points(ctt_hip_msm_ctx* ctx, int curve, uint64_t seed, uint64_t first, uint32_t n, void* d_out);
/* kernel unit tests on device arrays.  op 0 .. 6: element-wise coordinate-field op (0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 inverse by
 * division steps, 6 inverse by Fermat's exponent -- over Fp2 the same as 5; the inverse of 0 is 0), operands and result in the C-API
 * representation; 16 .. 23: the same operands through the device field, raw device limbs out (curves that compute in the carry-free
 * field).  Both refused (-1) for Banderwagon.
 * op 64 + k, k = 0 .. 6: the coordinate-field ops again, every curve (Banderwagon's field is reached here).
 * op 80 + k, k = 0 .. 8: the same table over the curve's scalar field, every curve: rows of 32 bytes, Montgomery residues; 7 from_mont
 * (residue -> canonical words), 8 to_mont (the reverse).
 * Every op outside these tables and the group law's below is refused (-1) and nothing is launched.
 * op 32 + k: the group law, every curve.  d_a, d_b: n raw device records (X, Y, ZZ, ZZZ; for Banderwagon X, Y, Z, T), 32-bit words in
 * the device representation of the coordinate field -- the caller chooses the representative of every coordinate.  d_r: per result
 * record, the record followed by one flag word (1 = the code takes it for the neutral element).  k = 0 .. 3 the mixed addition of the
 * accumulate kernel, a += +-(b.x, b.y) (bit 0: subtract, bit 1: a is empty); 4 .. 7 the same in its X, Y + ZZ/ZZZ-holder form (not
 * Banderwagon); 8 a + b; 9 2a; 10 2(a.x, a.y) -- one result record per element.  Four lanes per element: 16 the memory form with both
 * destinations (two records per element), 17 with one (one record), 18 the register form of a + b, 19 of 2a (four records per
 * element: every lane's copy).  -1 for an op the curve does not have. */
int ctt_hip_field_op(ctt_hip_msm_ctx* ctx, int curve, int op, const void* d_a, const void* d_b, void* d_r, uint32_t n);
/* kernel unit tests of the digit sort (Booth digits + sort by bucket: the six kernels of csrc/hip_backend.hip behind
 * HipBackend::launch_digits_sort) on device arrays, with the sort's sizing given by the caller instead of the engine's plan, so that
 * small inputs reach every path.  d_scalars: n canonical scalars of 8 words below 2^bits.
 * in[14]: 0 bits (1 .. 255), 1 c (2 .. 20; the windows are balanced over bits + 1 bits as in an MSM), 2 log2 of the bucket groups per set
 * (-1: what the engine's plan has for n), 3 scalars per partition block (0: the plan's), 4 cap and 5 big of pass B (0: 20480 / 1024),
 * 6 staged (0 / 1: the scatter form asked for; more than 1024 groups take the direct form), 7 xcd_map (0 / 1), 8 merged (1: the
 * window-table form, one bucket set, entries are table rows w * id_stride + j), 9 id_stride (merged: >= n), 10 zero_bytes (bytes of
 * one bucket of the region whose empty buckets are cleared, a multiple of 16; 0: none), 11 .. 13 what the caller's buffers hold:
 * words of d_entries, words of d_bstart, bytes of d_buckets.
 * used[11], written on success: cb, r (the first r windows have cb + 1 bits, the others cb), W (bucket sets), Wd (digit windows), B
 * (buckets per set), NG, gshift, gshift_narrow, nblk, jbits, nent (entries per set: n, or Wd * n when merged).
 * Outputs, the contract of the sort (csrc/msm_bodies.h, above SortArgs): d_entries [W][nent], d_bstart [W][B + 1], d_maxcount [4],
 * d_buckets [W][B] x zero_bytes (NULL without zero_bytes).  The intermediate arrays are the call's own; it returns when the sort is done.
 * -1 (last error set) and NOTHING launched or written for: n = 0 or above 2^31 - 1, bits, c or a flag out of range, a group count
 * that is no power of two or above B, merged with id_stride < n or more than 2^31 - 1 table rows,
 * zero_bytes no multiple of 16, a buffer smaller than the derived shape, a NULL pointer, and every plan the sort's launcher cannot
 * run (more than 16384 groups or 1024 buckets per group, cap + big beyond the LDS tile, a packed record above 32 bits).
 * ctt_hip_sort_probe_words is the same call on scalars of `kwords` words each, d_scalars [n][kwords]: 8 (what ctt_hip_sort_probe passes), or
 * 4 -- the half scalars of the endomorphism split, which the sort reads with the upper four words taken as zero; their windows must end
 * at bit 128 or below (bits <= 127).  It refuses, as above, every other kwords and 4 words under windows that end above bit 128. */
int ctt_hip_sort_probe(ctt_hip_msm_ctx* ctx, const void* d_scalars, uint32_t n, const int32_t* in, uint32_t* used, void* d_entries,
                       void* d_bstart, void* d_maxcount, void* d_buckets);
int ctt_hip_sort_probe_words(ctt_hip_msm_ctx* ctx, const void* d_scalars, uint32_t kwords, uint32_t n, const int32_t* in, uint32_t* used,
                             void* d_entries, void* d_bstart, void* d_maxcount, void* d_buckets);
/* kernel unit tests of the endomorphism split (BLS12-381 G1): the front kernel of the split path alone on device arrays -- what an MSM
 * of 2^17 .. 2^21 device-resident pairs runs in place of the point conversion.  d_scalars: n canonical scalars of 8 words below 2^255;
 * d_points: n affine points in the C-API layout.  Outputs, as the sort and the accumulation then read them: d_records [2n] records of
 * 128 bytes -- x, y in the device field (14 limbs of 28 bits each, value * 2^392 mod p up to a multiple of p, below 2p) and a flag word
 * at byte 112 (1 = the neutral element, whose coordinates stay zero) --, record j = s1 P_j and record n + j = s2 phi(P_j) with
 * phi(x, y) = (beta x, y) = [mu](x, y), the signs in y; d_half [2n][4] words, half scalar j = k1 and n + j = k2, both at most x^2 / 2
 * < 2^127, with k == s1 k1 + s2 k2 mu (mod r).  d_scalars, d_records and d_half must be 16-byte aligned (the kernel moves all three in
 * 16-byte pieces; hipMalloc's alignment is more than enough).  It returns when the kernel is done.
 * -1 (last error set) and NOTHING launched or written for a curve without a split, n = 0 or above 2^30, and a NULL pointer. */
int ctt_hip_glv_front_probe(ctt_hip_msm_ctx* ctx, int curve, const void* d_scalars, const void* d_points, uint32_t n, void* d_records,
                            void* d_half);
/* host-only: r (`out_kind` layout) = sum of n affine points -- combines the per-GPU partial results of a
 * sharded MSM (the `r ~+= partial` of ec_multi_scalar_mul_parallel.nim:427-429). Needs no GPU. */
int ctt_hip_ec_sum_affine(int curve, int out_kind, void* r, const void* pts_aff, size_t n);
/* r (host, `out_kind` layout) = sum of `len` affine points -- sum_reduce_vartime
 * (ec_shortweierstrass_batch_ops.nim:649-663) on the GPU; points on the host (points_on_device = 0) or in HBM (1). */
int ctt_hip_sum_reduce(ctt_hip_msm_ctx* ctx, int curve, int out_kind, void* r, const void* points, size_t len,
                       int points_on_device);
/* dst[i] = affine(src[i]), src_kind CTT_HIP_OUT_JAC (x = X/Z^2, y = Y/Z^3) or CTT_HIP_OUT_PRJ (x = X/Z, y = Y/Z) --
 * batchAffine(_vartime) (ec_shortweierstrass_batch_ops.nim:44-345).  Both arrays on the host (on_device = 0) or both
 * in HBM (1).  Blocking. */
int ctt_hip_batch_affine(ctt_hip_msm_ctx* ctx, int curve, int src_kind, void* dst, const void* src, size_t n, int on_device);
/* ok[i] = 1 when points[i] has order r (r = the curve order; the neutral passes): the subgroup check that the MSM's callers
 * run on deserialised points (eth_evm_bls12381_g1msm / g2msm, ethereum_evm_precompiles.nim:894-975; KZG commitments), for all n
 * points at once.  BLS12-381: the reference's endomorphism tests (isInSubgroup, named/constants/bls12_381_subgroups.nim:170-207);
 * other curves: [r]P = neutral.  Up to 64 host-resident points (256 for BLS12-381) are checked on host threads, more -- or
 * device-resident ones -- in one launch.  points: affine, host (points_on_device = 0) or device memory; ok: n bytes of host memory. */
int ctt_hip_subgroup_check(ctt_hip_msm_ctx* ctx, int curve, uint8_t* ok, const void* points, size_t n, int points_on_device);
/* Quotient polynomial of a KZG opening over the scalar field of `curve`, in evaluation form: the Fr-side work of kzg_prove
 * (constantine/commitments/kzg.nim:204-223 -> getQuotientPoly).  d_poly: n canonical scalars (the MSM's coefficient format),
 * d_domain: the n roots of unity as Montgomery residues, both in DEVICE memory; z: the opening point, canonical, host.  Writes
 * q_i = (p_i - y) / (w_i - z), canonical, to d_q (device: the coefficients of the proof's MSM) and y = p(z), canonical, to y
 * (host).  Blocking.  Returns 0; -2 when z is one of the roots of unity (the reference's other branch, left to the caller);
 * -1 for bad arguments or when device memory runs out. */
int ctt_hip_fr_quotient(ctt_hip_msm_ctx* ctx, int curve, void* d_q, void* y, const void* d_poly, const void* d_domain,
                        const void* z, uint32_t n);
/* the engine's hipStream_t */
void* ctt_hip_msm_stream(ctt_hip_msm_ctx* ctx);

/* ---- Part 3: the MSM's immediate callers under the reference's own names -----------------------
 * EIP-4844 KZG commitments and opening proofs over a context that caches the Lagrange SRS on the GPU, and the EIP-2537
 * BLS12_G1MSM / BLS12_G2MSM precompiles: same symbols, argument meaning and status enums as
 *   include/constantine/protocols/ethereum_eip4844_kzg.h:106 (blob_to_kzg_commitment), :126 (compute_kzg_proof),
 *       :153 (compute_blob_kzg_proof), :200 (context_new), :238 (context_delete)
 *   include/constantine/protocols/ethereum_evm_precompiles.h:386 (g1msm), :419 (g2msm)
 * (constantine/ethereum_eip4844_kzg.nim:297-444, constantine/ethereum_evm_precompiles.nim:894-1060).  Host side in C++
 * (constantine_amd/csrc/protocols.hip), MSMs / subgroup checks / quotient polynomial on the GPU.  Verification (pairings) and the
 * other precompiles are out of scope and not exported.  EIP-7594 (PeerDAS): compute_cells_and_kzg_proofs of
 *   include/constantine/protocols/ethereum_eip7594_peerdas.h
 * and the cells alone (recover_cells_and_kzg_proofs: ctt_msm_hip_peerdas.h); verify_cell_kzg_proof_batch and the FK20 form are out of scope.  There is no CPU fallback, and none of
 * these symbols terminates the process (round 5; rounds 1-4 aborted): a call the GPU cannot serve -- no device, out of device
 * memory, a failed HIP call -- returns CTT_HIP_STATUS_GPU_UNAVAILABLE, a value outside every status enum below (the reference's
 * *_status_to_string print "InvalidStatusCode" for it), leaves its outputs untouched, and ctt_hip_last_error() of the calling
 * thread says why.  A precompile whose context is momentarily held by another thread's tickets waits for it (up to ~2 s). */
#define CTT_HIP_STATUS_GPU_UNAVAILABLE 0xF0
#ifndef CTT_MSM_HIP_NO_PROTOCOLS
typedef uint8_t ctt_byte;   /* the reference's `byte` (constantine/core/datatypes.h) */
typedef struct ctt_eth_kzg_context_struct ctt_eth_kzg_context;
typedef struct { ctt_byte raw[48]; }        ctt_eth_kzg_commitment;
typedef struct { ctt_byte raw[48]; }        ctt_eth_kzg_proof;
typedef struct { ctt_byte raw[4096 * 32]; } ctt_eth_kzg_blob;
typedef struct { ctt_byte raw[32]; }        ctt_eth_kzg_opening_challenge;
typedef struct { ctt_byte raw[32]; }        ctt_eth_kzg_eval_at_challenge;
typedef enum __attribute__((__packed__)) {
  cttEthKzg_Success, cttEthKzg_VerificationFailure, cttEthKzg_InputsLengthsMismatch, cttEthKzg_ScalarZero,
  cttEthKzg_ScalarLargerThanCurveOrder, cttEthKzg_EccInvalidEncoding, cttEthKzg_EccCoordinateGreaterThanOrEqualModulus,
  cttEthKzg_EccPointNotOnCurve, cttEthKzg_EccPointNotInSubgroup, cttEthKzg_CellIndicesNotAscending,
} ctt_eth_kzg_status;
typedef enum __attribute__((__packed__)) {
  cttEthTS_Success, cttEthTS_MissingOrInaccessibleFile, cttEthTS_InvalidFile
} ctt_eth_trusted_setup_status;
typedef enum __attribute__((__packed__)) { cttEthTSFormat_ckzg4844 } ctt_eth_trusted_setup_format;
typedef enum __attribute__((__packed__)) {
  cttEVM_Success, cttEVM_InvalidInputSize, cttEVM_InvalidOutputSize, cttEVM_IntLargerThanModulus, cttEVM_PointNotOnCurve,
  cttEVM_PointNotInSubgroup, cttEVM_VerificationFailure,
} ctt_evm_status;

/* the c-kzg text format of the Ethereum ceremony; the SRS is cached on $CTT_HIP_DEVICE (default 0) */
ctt_eth_trusted_setup_status ctt_eth_kzg_context_new(ctt_eth_kzg_context** ctx, const char* filepath,
                                                     ctt_eth_trusted_setup_format format);
/* ethereum_eip4844_kzg.h:232 -- t, b size the reference's CPU lookup tables (PeerDAS); accepted, the same context as above.  This
 * library's counterpart of those tables is the table of the batched fixed-base MSM (include/ctt_msm_hip_fixed.h) that serves the 128
 * cell proofs in one pass: every context builds it at its first proof call, whichever constructor made it; $CTT_HIP_CELL_PROOFS_C
 * (window bits) sizes it, and $CTT_HIP_CELL_PROOFS=loop at creation keeps the loop of 128 MSMs over the cached SRS instead. */
ctt_eth_trusted_setup_status ctt_eth_kzg_context_new_with_precompute(ctt_eth_kzg_context** ctx, const char* filepath,
                                                                     ctt_eth_trusted_setup_format format, int t, int b);
void ctt_eth_kzg_context_delete(ctt_eth_kzg_context* ctx);
ctt_eth_kzg_status ctt_eth_kzg_blob_to_kzg_commitment(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_commitment* dst,
                                                      const ctt_eth_kzg_blob* blob);
ctt_eth_kzg_status ctt_eth_kzg_compute_kzg_proof(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_proof* proof,
                                                 ctt_eth_kzg_eval_at_challenge* y, const ctt_eth_kzg_blob* blob,
                                                 const ctt_eth_kzg_opening_challenge* z);
ctt_eth_kzg_status ctt_eth_kzg_compute_blob_kzg_proof(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_proof* proof,
                                                      const ctt_eth_kzg_blob* blob, const ctt_eth_kzg_commitment* commitment);
/* include/constantine/protocols/ethereum_eip4844_kzg_parallel.h:40, :61, :73 -- the thread pool is accepted and not used */
ctt_eth_kzg_status ctt_eth_kzg_blob_to_kzg_commitment_parallel(const ctt_threadpool* tp, const ctt_eth_kzg_context* ctx,
                                                               ctt_eth_kzg_commitment* dst, const ctt_eth_kzg_blob* blob);
ctt_eth_kzg_status ctt_eth_kzg_compute_kzg_proof_parallel(const ctt_threadpool* tp, const ctt_eth_kzg_context* ctx,
                                                          ctt_eth_kzg_proof* proof, ctt_eth_kzg_eval_at_challenge* y,
                                                          const ctt_eth_kzg_blob* blob, const ctt_eth_kzg_opening_challenge* z);
ctt_eth_kzg_status ctt_eth_kzg_compute_blob_kzg_proof_parallel(const ctt_threadpool* tp, const ctt_eth_kzg_context* ctx,
                                                               ctt_eth_kzg_proof* proof, const ctt_eth_kzg_blob* blob,
                                                               const ctt_eth_kzg_commitment* commitment);
/* EIP-7594: cells[128] and proofs[128] of the extended blob.  The cells' second half is the coset transform of the blob's
 * coefficients, proof k the MSM of the evaluations of p / (X^64 - c_k) over the context's cached Lagrange SRS (Part 5's NTT; 16 MiB
 * of device memory from the first call on).  Nothing is written on any status but Success.  The context is not modified as the
 * caller sees it (it serialises its calls). */
typedef struct { ctt_byte raw[2048]; }      ctt_eth_kzg_cell;
ctt_eth_kzg_status ctt_eth_kzg_compute_cells_and_kzg_proofs(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_cell cells[128],
                                                            ctt_eth_kzg_proof proofs[128], const ctt_eth_kzg_blob* blob);
/* not in the reference's C header (its Nim API has compute_cells): the cells alone -- two transforms, no MSM */
ctt_eth_kzg_status ctt_hip_eth_kzg_compute_cells(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_cell cells[128], const ctt_eth_kzg_blob* blob);
/* test-facing: the 128 x 4096 canonical little-endian coefficients of the cell quotients (the quotient kernel alone), and the
 * host-clock times (ms) of the context's last cells call: parse + upload, INTT, coset NTT, quotients, batched NTT, the MSMs,
 * compress + copy back; with cap >= 9 also [7] the rows of the cell proofs the table kernel served in that call (128, or 0: the
 * loop) and [8] the ms that call paid for building the table (returns the number written: 9, or at most 7) */
ctt_eth_kzg_status ctt_hip_eth_kzg_cell_quotients(const ctt_eth_kzg_context* ctx, uint8_t* q_le, const ctt_eth_kzg_blob* blob);
int ctt_hip_eth_kzg_last_cell_timings(const ctt_eth_kzg_context* ctx, float* ms, int cap);
ctt_evm_status ctt_eth_evm_bls12381_g1msm(ctt_byte* r, size_t r_len, const ctt_byte* inputs, size_t inputs_len);
ctt_evm_status ctt_eth_evm_bls12381_g2msm(ctt_byte* r, size_t r_len, const ctt_byte* inputs, size_t inputs_len);

/* Not in the reference: the context from memory -- the 4096 x 48 bytes of the Lagrange-form G1 SRS in ceremony (file) order --
 * on a chosen GPU, optionally cached as a window table (ctt_hip_msm_bases_create_table).  -> ctt_eth_trusted_setup_status */
int ctt_hip_eth_kzg_context_from_srs(ctt_eth_kzg_context** ctx, const uint8_t* g1_lagrange_compressed, size_t n_points,
                                     int device, int table);
/* Host-only pieces of the above (no GPU): SHA-256; BLS12-381 G1 compressed <-> affine Montgomery {x, y} (C-API layout, no
 * subgroup check; -> ctt_eth_kzg_status); blob -> 4096 canonical little-endian scalars (-> ctt_eth_kzg_status); the Fiat-Shamir
 * challenge of compute_blob_kzg_proof (32 big-endian bytes); the quotient polynomial of an opening on the host, both branches
 * (4096 canonical little-endian scalars in and out, z and y 32 little-endian bytes). */
void ctt_hip_sha256(uint8_t out[32], const uint8_t* data, size_t len);
int ctt_hip_bls12_381_g1_decompress(uint8_t aff[96], const uint8_t in[48]);
void ctt_hip_bls12_381_g1_compress(uint8_t out[48], const uint8_t aff[96]);
int ctt_hip_eth_kzg_blob_to_scalars(uint8_t* scalars_le, const uint8_t* blob);
void ctt_hip_eth_kzg_challenge(uint8_t z_be[32], const uint8_t* blob, const uint8_t commitment[48]);
void ctt_hip_eth_kzg_quotient_host(uint8_t* q_le, uint8_t y_le[32], const uint8_t* poly_le, const uint8_t z_le[32]);
#endif /* CTT_MSM_HIP_NO_PROTOCOLS */

/* ---- Part 4: batched Verkle commitments over a fixed Banderwagon basis -----------------------------------------------------
 * A Verkle node commits 256 scalars against the 256 points of a fixed CRS (constantine/ethereum_verkle_ipa.nim), maps the commitment
 * to a scalar for its parent (batchMapToScalarField) and sometimes serialises it (serializeBatch_vartime,
 * serialization/codecs_banderwagon.nim); a tree update does so thousands of times over the same points.  These symbols keep a table
 * of precomputed multiples of the CRS on the GPU and compute many commitments in one dedicated kernel: no sort, no buckets, no
 * tickets.  Return values as in Part 1c: 0; -1 refused (NULL crs, a crs of another context, every output NULL, a coef_kind other
 * than CTT_HIP_COEF_BIG / _FR, an m whose buffers would pass 2^31 - 1 bytes, no device); -2 out of device memory.  Outputs are
 * untouched on error and ctt_hip_last_error() says why.  ctx == NULL is the default context; m == 0 returns 0 and writes nothing;
 * every call blocks, on the context's main stream, and may be made while MSM tickets are outstanding on the context.
 *
 * crs_create: n affine Banderwagon elements, 1 <= n <= 256 ((0, 1) and (0, -1) are legal), on the host or (on_device = 1) in HBM.
 * window_bits 0 = the default (10), else 2 .. 10: the table holds j * 2^off(w) * P_i for every window w of the balanced layout and
 * j = 1 .. 2^(width(w) - 1) as (x, y, d*x*y) -- 276 MiB at 10 bits and 256 points, 93 MiB at 8.  NULL on refusal (last error -1, -2 or -3).
 * $CTT_HIP_VERKLE_PAD=1 pads the 96-byte records to 128 bytes (an experiment knob, read by crs_create).  Destroy a crs before its context. */
typedef struct ctt_hip_verkle_crs ctt_hip_verkle_crs;
ctt_hip_verkle_crs* ctt_hip_verkle_crs_create(ctt_hip_msm_ctx* ctx, const void* points_aff, size_t n, int window_bits, int on_device);
void ctt_hip_verkle_crs_destroy(ctt_hip_msm_ctx* ctx, ctt_hip_verkle_crs* crs);
int ctt_hip_verkle_crs_window_bits(const ctt_hip_verkle_crs* crs);
/* R_k = sum_i coefs[k][i] * P_i for m rows of n scalars, row-major, 32 bytes each: CTT_HIP_COEF_BIG (canonical, any value below 2^253)
 * or CTT_HIP_COEF_FR (Montgomery).  Any of out_prj (m x 96 bytes: (x, y, 1), byte-identical to ctt_hip_msm_banderwagon_ec_prj_* on the
 * same row; the neutral is (0, 1, 1)), out_ser (m x 32 bytes, big-endian: x if y >= (p-1)/2 else p - x) and out_fr (m x 32 bytes:
 * ((x / y) mod p) mod r, Montgomery) may be NULL; at least one is not.  on_device applies to coefs and to all outputs together
 * (device buffers 4-byte aligned). */
int ctt_hip_verkle_commit_batch(ctt_hip_msm_ctx* ctx, const ctt_hip_verkle_crs* crs, int coef_kind, void* out_prj, void* out_ser,
                                void* out_fr, const void* coefs, size_t m, int on_device);
/* batchMapToScalarField / serializeBatch_vartime on caller-supplied projective points (m x 96 bytes, any Z), one inversion per
 * eight points.  The reference's inv(0) = 0: Y = 0 maps to the scalar 0, Z = 0 serialises to 32 zero bytes. */
int ctt_hip_banderwagon_map_to_fr_batch(ctt_hip_msm_ctx* ctx, void* out_fr, const void* points_prj, size_t m, int on_device);
int ctt_hip_banderwagon_serialize_batch(ctt_hip_msm_ctx* ctx, void* out_ser, const void* points_prj, size_t m, int on_device);
/* The sparse update of m commitments: R_k = base_k + sum over e in [row_ptr[k], row_ptr[k+1]) of deltas[e] * P_idx[e] -- what a tree in
 * service does to a node of which a block changed a few slots (deltas = new - old value, mod r), in one pass: one wavefront per row,
 * the row's entries x windows spread over its lanes.  row_ptr (m + 1 values, CSR) and idx (row_ptr[m] bytes) are ALWAYS host memory
 * and are checked before anything is launched: row_ptr[0] == 0, non-decreasing, every idx[e] < n of the crs, row_ptr[m] * 32 and every
 * m-sized buffer below 2^31 - 1 bytes (else -1, outputs untouched).  Two entries of a row may name the same base; a row may be empty.
 * deltas: row_ptr[m] x 32 bytes, CTT_HIP_COEF_BIG or _FR as above.  base_prj: m x 96 bytes (X, Y, Z) Montgomery, any non-zero Z, or NULL
 * for the neutral.  out_prj, out_ser, out_fr as for commit_batch; out_dfr (m x 32 bytes, Montgomery) = map(R_k) - map(base_k) mod r, the
 * delta the parent node takes for this child (map(neutral) = 0).  Any output may be NULL; at least one is not.  on_device applies to
 * deltas, base_prj and all four outputs together.  ctt_hip_verkle_last_timings then reports the update kernel and the finish. */
int ctt_hip_verkle_update_batch(ctt_hip_msm_ctx* ctx, const ctt_hip_verkle_crs* crs, int coef_kind, void* out_prj, void* out_ser,
                                void* out_fr, void* out_dfr, const void* base_prj, const uint32_t* row_ptr, const uint8_t* idx,
                                const void* deltas, size_t m, int on_device);
/* HIP-event times (ms) of the context's last commit or update batch -- recorded while the option "timings" is non-zero -- and of its
 * last table build: commit (update) kernel, finish kernel(s), table build.  Returns 0, or -1 without a usable context. */
int ctt_hip_verkle_last_timings(ctt_hip_msm_ctx* ctx, float* ms, int cap);

/* ---- Part 5: batched number-theoretic transform over a curve's scalar field -------------------------------------------------
 * n = 2^log2n elements of 32 bytes per row, log2n from 1 to min(24, the two-adicity of the field: 32 for BLS12-381, Pallas and
 * Vesta, 28 for BN254-Snarks, 5 for Banderwagon); G1 and G2 of a pairing curve share their field.  A plan holds the table
 * omega^i, i < n/2 (16 * n bytes of device memory) on its context; destroy it before the context.
 *   plan_create  omega: 32 canonical little-endian bytes on the host, checked there: below the modulus and omega^(n/2) == -1.
 *                tile_log2: radix-2 stages per pass, 1 .. 9, 0 = the default (8).  NULL on refusal (last error -1, -2 or -3).
 *   fr_ntt       d_in, d_out: device memory, 16-byte aligned, `batch` rows of n elements; d_out may equal d_in (rows may not
 *                overlap otherwise).  shift: NULL, or a non-zero canonical scalar g on the host (the coset g * <omega>).
 *                  forward   out[k] = sum_i (g^i * in[i]) * omega^(i*k)
 *                  inverse   out[i] = g^(-i) * n^(-1) * sum_k in[k] * omega^(-i*k)          (CTT_HIP_NTT_INVERSE)
 *                i and k are natural indices; CTT_HIP_NTT_IN_BRP / _OUT_BRP say that a side is laid out in bit-reversed order
 *                (element i at position brp(i)).  With _IN_MONT / _OUT_MONT that side holds Montgomery residues, else canonical
 *                little-endian scalars -- the MSM's CTT_HIP_COEF_BIG -- fully reduced on output; the conversion is part of the
 *                first load and the last store.  batch * n <= 2^26; batch == 0 returns 0 and touches nothing.
 * Blocking, on the context's main stream: ordered against the MSM submits of the same context.  Returns 0; -1 refused before any
 * launch (a NULL pointer, misaligned pointers, unknown flag bits, a shift of zero or >= the modulus, a plan of another context,
 * batch * n too large); -2 out of device memory (the n multipliers of a shift, kept with the plan).  ctx == NULL is the default
 * context. */
#define CTT_HIP_NTT_INVERSE 1
#define CTT_HIP_NTT_IN_BRP 2
#define CTT_HIP_NTT_OUT_BRP 4
#define CTT_HIP_NTT_IN_MONT 8
#define CTT_HIP_NTT_OUT_MONT 16
typedef struct ctt_hip_ntt_plan ctt_hip_ntt_plan;
ctt_hip_ntt_plan* ctt_hip_fr_ntt_plan_create(ctt_hip_msm_ctx* ctx, int curve, int log2n, const void* omega, int tile_log2);
void ctt_hip_fr_ntt_plan_destroy(ctt_hip_msm_ctx* ctx, ctt_hip_ntt_plan* plan);
int ctt_hip_fr_ntt(ctt_hip_msm_ctx* ctx, const ctt_hip_ntt_plan* plan, void* d_out, const void* d_in, size_t batch, int flags,
                   const void* shift);
/* info[0..3] = log2n, tile_log2, passes of a natural-order-in transform, bytes of the twiddle table; 0, or -1 for a NULL */
int ctt_hip_fr_ntt_plan_info(const ctt_hip_ntt_plan* plan, size_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* CTT_MSM_HIP_H */
