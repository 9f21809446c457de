/* ctt_msm_hip_banderwagon.h -- C ABI of libctt_msm_hip_banderwagon.so: the Banderwagon MSM symbols of Constantine's
 * include/constantine/curves/banderwagon.h on the MI355X (gfx950) engine of libctt_msm_hip.so.
 *
 * A library of its own so that libctt_msm_hip.so keeps exactly the symbol set of ctt_msm_hip.h.  Link it in front of
 * libctt_msm_hip.so (it names that library as NEEDED and finds it next to itself: $ORIGIN).
 *
 * Input contract, as in the reference: the points are valid Banderwagon elements (on the curve, in the prime-order subgroup or its
 * coset by (0,-1)), affine, Montgomery form; the affine neutral is (0,1).  The twisted Edwards law the engine uses is complete on
 * that group only: for other curve points the result is unspecified.  Variable time: public inputs only.
 * Results: projective (X:Y:Z) with Z = 1; the neutral is (0,1,1).
 *
 * Types are layout-compatible with banderwagon.h:16-20; define CTT_MSM_HIP_NO_TYPES when Constantine's own headers are included. */
#ifndef CTT_MSM_HIP_BANDERWAGON_H
#define CTT_MSM_HIP_BANDERWAGON_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CTT_MSM_HIP_NO_TYPES
#ifndef CTT_WORD_BITWIDTH
typedef size_t secret_word;
#define CTT_WORD_BITWIDTH (sizeof(secret_word) * 8)
#define CTT_WORDS_REQUIRED(bits) (((bits) + CTT_WORD_BITWIDTH - 1) / CTT_WORD_BITWIDTH)
#endif
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(253)]; } big253;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(253)]; } banderwagon_fr;
typedef struct { secret_word limbs[CTT_WORDS_REQUIRED(255)]; } banderwagon_fp;
typedef struct { banderwagon_fp x, y; } banderwagon_ec_aff;
typedef struct { banderwagon_fp x, y, z; } banderwagon_ec_prj;
#endif /* CTT_MSM_HIP_NO_TYPES */

/* banderwagon.h:127-128.  A call the GPU cannot serve aborts with a diagnostic (the reference's symbols cannot fail). */
void ctt_banderwagon_ec_prj_multi_scalar_mul_big_coefs_vartime(banderwagon_ec_prj* r, const big253 coefs[], const banderwagon_ec_aff points[], size_t len);
void ctt_banderwagon_ec_prj_multi_scalar_mul_fr_coefs_vartime(banderwagon_ec_prj* r, const banderwagon_fr coefs[], const banderwagon_ec_aff points[], size_t len);

/* The same with an error channel, for a binding inside libconstantine that keeps its CPU path (ctt_msm_hip.h Part 1c):
 * 0 = r holds the result; -1 refused (no usable GPU, a length above 2^31-1, all in-flight slots busy), -2 out of device
 * memory -- r is then untouched. */
int ctt_hip_msm_banderwagon_ec_prj_big(banderwagon_ec_prj* r, const big253 coefs[], const banderwagon_ec_aff points[], size_t len);
int ctt_hip_msm_banderwagon_ec_prj_fr(banderwagon_ec_prj* r, const banderwagon_fr coefs[], const banderwagon_ec_aff points[], size_t len);

#ifdef __cplusplus
}
#endif
#endif /* CTT_MSM_HIP_BANDERWAGON_H */
