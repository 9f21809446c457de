// fixed_syms.hip -- the C symbols of include/ctt_msm_hip_fixed.h (libctt_msm_hip_fixed.so) over FixedTable (fixed.h): a handle is
// one table with a stream of its own.  The engine (libctt_msm_hip.so) links the same fixed.o and calls the class directly.
#include "fixed.h"

#include "../../include/ctt_msm_hip_fixed.h"

using namespace ctt;

static_assert(FX_CURVE_BLS12_381_G1 == CTT_HIP_BLS12_381_G1 && FX_CURVE_BN254_G1 == CTT_HIP_BN254_SNARKS_G1, "curve ids");
static_assert(FX_COEF_BIG == CTT_HIP_COEF_BIG && FX_COEF_FR == CTT_HIP_COEF_FR, "coefficient kinds");
static_assert(FX_COEFS_ON_DEVICE == CTT_HIP_FIXED_COEFS_ON_DEVICE && FX_OUT_ON_DEVICE == CTT_HIP_FIXED_OUT_ON_DEVICE, "flags");

struct ctt_hip_fixed_bases {
  hipStream_t stream = nullptr;
  FixedTable* table = nullptr;
};

namespace {
thread_local int fx_last_error = 0;
int report(int rc) {
  if (rc != 0) fx_last_error = rc;
  return rc;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

ctt_hip_fixed_bases* ctt_hip_fixed_bases_create(int device, int curve, const void* points_aff, size_t n, int c) {
  int count = 0, prev = -1;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count || hipGetDevice(&prev) != hipSuccess) {
    (void)hipGetLastError();
    report(FX_HIP_ERROR);
    return nullptr;
  }
  ctt_hip_fixed_bases* h = new ctt_hip_fixed_bases();
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipSetDevice(prev);
    delete h;
    report(FX_HIP_ERROR);
    return nullptr;
  }
  (void)hipSetDevice(prev);
  h->table = new FixedTable(device, h->stream);
  const int rc = h->table->build(curve, points_aff, n, c);
  if (rc != FX_OK) {
    ctt_hip_fixed_bases_destroy(h);
    report(rc);
    return nullptr;
  }
  return h;
}

void ctt_hip_fixed_bases_destroy(ctt_hip_fixed_bases* h) {
  if (!h) return;
  const int device = h->table ? h->table->device() : -1;
  delete h->table;   // (waits for the stream)
  if (h->stream) {
    int prev = -1;
    if (hipGetDevice(&prev) == hipSuccess && device >= 0 && hipSetDevice(device) == hipSuccess) {
      (void)hipStreamDestroy(h->stream);
      (void)hipSetDevice(prev);
    }
    (void)hipGetLastError();
  }
  delete h;
}

int ctt_hip_fixed_bases_info(const ctt_hip_fixed_bases* h, size_t info[6]) {
  if (!h || !info) return report(FX_REFUSED);
  const FixedTable& t = *h->table;
  info[0] = t.n();
  info[1] = (size_t)t.c();
  info[2] = t.windows();
  info[3] = t.rows();
  info[4] = t.table_bytes();
  info[5] = (size_t)(t.build_ms() * 1000.0f);
  return 0;
}

int ctt_hip_fixed_msm_batch(ctt_hip_fixed_bases* h, int coef_kind, const void* coefs, size_t m, void* out_aff, int flags) {
  if (!h) return report(FX_REFUSED);
  return report(h->table->msm_batch(coef_kind, coefs, m, out_aff, flags));
}

int ctt_hip_fixed_last_timings(const ctt_hip_fixed_bases* h, float ms[2]) {
  if (!h || !ms) return report(FX_REFUSED);
  ms[0] = h->table->last_kernel_ms();
  ms[1] = h->table->last_finish_ms();
  return 0;
}

int ctt_hip_fixed_last_error(void) { return fx_last_error; }

}  // extern "C"
#pragma GCC visibility pop
