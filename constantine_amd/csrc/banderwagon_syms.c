/* banderwagon_syms.c -- libctt_msm_hip_banderwagon.so: the Banderwagon symbols of include/ctt_msm_hip_banderwagon.h, thin C over
 * ctt_hip_msm_host(CTT_HIP_BANDERWAGON, ...) of libctt_msm_hip.so (exports: banderwagon_exports.map). */
#include <stdio.h>
#include <stdlib.h>
#include "../../include/ctt_msm_hip.h"
#include "../../include/ctt_msm_hip_banderwagon.h"

int ctt_hip_msm_banderwagon_ec_prj_big(banderwagon_ec_prj* r, const big253 coefs[], const banderwagon_ec_aff points[], size_t len) {
  return ctt_hip_msm_host(CTT_HIP_BANDERWAGON, CTT_HIP_COEF_BIG, CTT_HIP_OUT_PRJ, r, coefs, points, len);
}
int ctt_hip_msm_banderwagon_ec_prj_fr(banderwagon_ec_prj* r, const banderwagon_fr coefs[], const banderwagon_ec_aff points[], size_t len) {
  return ctt_hip_msm_host(CTT_HIP_BANDERWAGON, CTT_HIP_COEF_FR, CTT_HIP_OUT_PRJ, r, coefs, points, len);
}

static void served_or_abort(int rc, const char* fn) {
  if (rc == 0) return;
  fprintf(stderr, "[ctt_msm_hip] FATAL %s: the GPU could not serve the call (%d: %s)\n", fn, ctt_hip_last_error(),
          ctt_hip_last_error_message());
  abort();
}
void ctt_banderwagon_ec_prj_multi_scalar_mul_big_coefs_vartime(banderwagon_ec_prj* r, const big253 coefs[], const banderwagon_ec_aff points[], size_t len) {
  served_or_abort(ctt_hip_msm_banderwagon_ec_prj_big(r, coefs, points, len), __func__);
}
void ctt_banderwagon_ec_prj_multi_scalar_mul_fr_coefs_vartime(banderwagon_ec_prj* r, const banderwagon_fr coefs[], const banderwagon_ec_aff points[], size_t len) {
  served_or_abort(ctt_hip_msm_banderwagon_ec_prj_fr(r, coefs, points, len), __func__);
}
