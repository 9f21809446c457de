// recover.hip -- EIP-7594 recover_cells_and_kzg_proofs on the GPU, batched over blobs: the C symbols of include/ctt_msm_hip_peerdas.h
// (libctt_msm_hip_peerdas.so).  A companion of libctt_msm_hip.so over its public C ABI -- ctt_hip_msm_ctx_create / _destroy,
// ctt_hip_msm_stream, ctt_hip_fr_ntt*, ctt_eth_kzg_compute_cells_and_kzg_proofs -- and nothing of its insides.  The host logic and the
// bodies of the three kernels: recover_host.h; the formulas: DESIGN.md section 15.
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ctt_msm_hip_peerdas.h"
#include "recover_host.h"

using namespace ctt;
using namespace ctt::proto;

namespace {

constexpr int GPU_UNAVAILABLE = CTT_HIP_STATUS_GPU_UNAVAILABLE;
constexpr unsigned RC_BLOCK = 256;

// one lane per element of the B rows; B <= 4096: at most 2^25 lanes in 2^17 workgroups
__global__ void __launch_bounds__(RC_BLOCK) k_rc_load(RcLoadArgs a) { rc_load_body(a, blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(RC_BLOCK) k_rc_scale(RcScaleArgs a) { rc_scale_body(a, blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(RC_BLOCK) k_rc_split(RcSplitArgs a) { rc_split_body(a, blockIdx.x * blockDim.x + threadIdx.x); }

// a failed HIP call ends the call with GPU_UNAVAILABLE; the runtime's sticky error is read away
#define RC_HIP(x)                         \
  do {                                    \
    if ((x) != hipSuccess) {              \
      (void)hipGetLastError();            \
      return GPU_UNAVAILABLE;             \
    }                                     \
  } while (0)

// the calling thread's device is the caller's business: selected for the duration of a call, put back afterwards
struct RcDeviceScope {
  int prev = -1;
  bool ok = false;
  explicit RcDeviceScope(int device) {
    ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess;
    if (!ok) (void)hipGetLastError();
  }
  ~RcDeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

using clk = std::chrono::steady_clock;
float ms_since(clk::time_point& t0) {
  const clk::time_point t1 = clk::now();
  const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  t0 = t1;
  return ms;
}

}  // namespace

struct ctt_hip_peerdas_recovery {
  std::mutex mu;
  int device = 0;
  ctt_hip_msm_ctx* hip = nullptr;
  ctt_hip_ntt_plan* plan13 = nullptr;   // 8192 points, omega_8192
  ctt_hip_ntt_plan* plan12 = nullptr;   // 4096 points, omega_4096 = omega_8192^2
  // the workspace, grow-only: the uploaded cells; B rows of 8192; B x 4096 coefficients; B flags; zc * R^2, izc5 (128 elements each)
  // and slot[128]
  void* d_cells = nullptr;
  size_t cells_cap = 0;
  void* d_rows = nullptr;
  void* d_coef = nullptr;
  void* d_high = nullptr;
  size_t blobs_cap = 0;
  void* d_const = nullptr;
  float ms[5] = {0, 0, 0, 0, 0};
};

namespace {

constexpr size_t CONST_BYTES = 2 * (size_t)N_CELLS * 32 + (size_t)N_CELLS * 4;

void rc_release(ctt_hip_peerdas_recovery* r) {
  RcDeviceScope scope(r->device);
  for (void* d : {r->d_cells, r->d_rows, r->d_coef, r->d_high, r->d_const})
    if (d) (void)hipFree(d);
  if (r->plan13) ctt_hip_fr_ntt_plan_destroy(r->hip, r->plan13);
  if (r->plan12) ctt_hip_fr_ntt_plan_destroy(r->hip, r->plan12);
  if (r->hip) ctt_hip_msm_ctx_destroy(r->hip);
  (void)hipGetLastError();
}

// room for B blobs of n cells
int rc_reserve(ctt_hip_peerdas_recovery* r, size_t n, size_t B) {
  const size_t cells_bytes = B * n * 2048;
  if (cells_bytes > r->cells_cap) {
    if (r->d_cells) (void)hipFree(r->d_cells);
    r->d_cells = nullptr;
    r->cells_cap = 0;
    RC_HIP(hipMalloc(&r->d_cells, cells_bytes));
    r->cells_cap = cells_bytes;
  }
  if (B > r->blobs_cap) {
    for (void** d : {&r->d_rows, &r->d_coef, &r->d_high}) {
      if (*d) (void)hipFree(*d);
      *d = nullptr;
    }
    r->blobs_cap = 0;
    RC_HIP(hipMalloc(&r->d_rows, B * (size_t)N_EXT * 32));
    RC_HIP(hipMalloc(&r->d_coef, B * (size_t)N_BLOB * 32));
    RC_HIP(hipMalloc(&r->d_high, B * 4));
    r->blobs_cap = B;
  }
  return KZG_Success;
}

// Steps 1-6 (and 7 unless coefs_le is asked for) for validated input.  Exactly one of blobs / coefs_le is non-NULL; both and
// `consistent` are written at the very end only.
int rc_recover(ctt_hip_peerdas_recovery* r, uint8_t* blobs, uint8_t* coefs_le, uint8_t* consistent, const uint64_t* idx, const uint8_t* cells,
               size_t n, size_t B, float check_ms) {
  std::lock_guard<std::mutex> lock(r->mu);
  RcDeviceScope scope(r->device);
  if (!scope.ok) return GPU_UNAVAILABLE;
  hipStream_t s = (hipStream_t)ctt_hip_msm_stream(r->hip);
  if (!s) return GPU_UNAVAILABLE;   // the context was lost to an earlier HIP failure
  float ms[5] = {0, 0, 0, 0, 0};
  clk::time_point t0 = clk::now();
  // the constants of this index set (host: 2 x 8192 multiplications, one inversion)
  FrH zc[N_CELLS], izc5[N_CELLS];
  struct {
    uint64_t zcr2[N_CELLS][4], izc5[N_CELLS][4];
    int32_t slot[N_CELLS];
  } consts;
  static_assert(sizeof(consts) == CONST_BYTES, "layout of the constants");
  recovery_constants(idx, n, zc, izc5, consts.slot);
  for (int k = 0; k < N_CELLS; k++) {
    const FrH t = to_mont<FrH>(zc[k].l);   // zc * R^2: the load kernel's one multiplication converts and scales
    memcpy(consts.zcr2[k], t.l, 32);
    memcpy(consts.izc5[k], izc5[k].l, 32);
  }
  const int rc = rc_reserve(r, n, B);
  if (rc != KZG_Success) return rc;
  RC_HIP(hipMemcpyAsync(r->d_const, &consts, CONST_BYTES, hipMemcpyHostToDevice, s));
  RC_HIP(hipMemcpyAsync(r->d_cells, cells, B * n * 2048, hipMemcpyHostToDevice, s));
  RC_HIP(hipMemsetAsync(r->d_high, 0, B * 4, s));
  RC_HIP(hipStreamSynchronize(s));
  ms[0] = check_ms + ms_since(t0);

  const uint32_t nb = (uint32_t)B;
  const dim3 grid(nb * (uint32_t)N_EXT / RC_BLOCK), block(RC_BLOCK);
  const uint32_t* d_zcr2 = (const uint32_t*)r->d_const;
  const uint32_t* d_izc5 = d_zcr2 + N_CELLS * 8;
  const int32_t* d_slot = (const int32_t*)(d_izc5 + N_CELLS * 8);
  uint64_t five[4] = {RC_COSET_SHIFT, 0, 0, 0};
  const int mont = CTT_HIP_NTT_IN_MONT | CTT_HIP_NTT_OUT_MONT;
  // 1. rows = the bit-reversed extended evaluations times Z
  hipLaunchKernelGGL(k_rc_load, grid, block, 0, s, RcLoadArgs{(const uint8_t*)r->d_cells, d_zcr2, d_slot, (uint32_t*)r->d_rows, (uint32_t)n, nb});
  RC_HIP(hipGetLastError());
  RC_HIP(hipStreamSynchronize(s));
  ms[2] += ms_since(t0);
  // 2. the coefficients of E Z; 3. its values on the coset 5 <omega_8192>, bit-reversed
  if (ctt_hip_fr_ntt(r->hip, r->plan13, r->d_rows, r->d_rows, B, CTT_HIP_NTT_INVERSE | CTT_HIP_NTT_IN_BRP | mont, nullptr) != 0) return GPU_UNAVAILABLE;
  if (ctt_hip_fr_ntt(r->hip, r->plan13, r->d_rows, r->d_rows, B, CTT_HIP_NTT_OUT_BRP | mont, five) != 0) return GPU_UNAVAILABLE;
  ms[1] += ms_since(t0);
  // 4. divided by Z there: one constant per cell
  hipLaunchKernelGGL(k_rc_scale, grid, block, 0, s, RcScaleArgs{(uint32_t*)r->d_rows, d_izc5, nb});
  RC_HIP(hipGetLastError());
  RC_HIP(hipStreamSynchronize(s));
  ms[2] += ms_since(t0);
  // 5. the 8192 coefficients of the recovered polynomial, natural order
  if (ctt_hip_fr_ntt(r->hip, r->plan13, r->d_rows, r->d_rows, B, CTT_HIP_NTT_INVERSE | CTT_HIP_NTT_IN_BRP | mont, five) != 0) return GPU_UNAVAILABLE;
  ms[1] += ms_since(t0);
  // 6. the low half compacted, the high half tested for zero
  hipLaunchKernelGGL(k_rc_split, grid, block, 0, s, RcSplitArgs{(uint32_t*)r->d_rows, (uint32_t*)r->d_coef, (uint32_t*)r->d_high, nb, coefs_le ? 1u : 0u});
  RC_HIP(hipGetLastError());
  RC_HIP(hipStreamSynchronize(s));
  ms[2] += ms_since(t0);
  std::vector<uint32_t> high(B);
  std::vector<uint8_t> ev;
  if (coefs_le) {
    ev.resize(B * (size_t)N_EXT * 32);
    RC_HIP(hipMemcpyAsync(ev.data(), r->d_rows, ev.size(), hipMemcpyDeviceToHost, s));
    RC_HIP(hipMemcpyAsync(high.data(), r->d_high, B * 4, hipMemcpyDeviceToHost, s));
    RC_HIP(hipStreamSynchronize(s));
    memcpy(coefs_le, ev.data(), ev.size());
  } else {
    // 7. back to evaluations over <omega_4096>, bit-reversed and canonical: the blob, little-endian
    if (ctt_hip_fr_ntt(r->hip, r->plan12, r->d_coef, r->d_coef, B, CTT_HIP_NTT_IN_MONT | CTT_HIP_NTT_OUT_BRP, nullptr) != 0) return GPU_UNAVAILABLE;
    ev.resize(B * (size_t)N_BLOB * 32);
    RC_HIP(hipMemcpyAsync(ev.data(), r->d_coef, ev.size(), hipMemcpyDeviceToHost, s));
    RC_HIP(hipMemcpyAsync(high.data(), r->d_high, B * 4, hipMemcpyDeviceToHost, s));
    RC_HIP(hipStreamSynchronize(s));
    for (size_t e = 0; e < B * (size_t)N_BLOB; e++) {
      uint64_t v[4];
      memcpy(v, &ev[32 * e], 32);
      limbs_to_be<FrH>(v, blobs + 32 * e);
    }
  }
  ms[3] = ms_since(t0);
  if (consistent)
    for (size_t b = 0; b < B; b++) consistent[b] = high[b] ? 0 : 1;
  memcpy(r->ms, ms, sizeof ms);
  return KZG_Success;
}

// the checks every symbol makes first, in the reference's order; -> KZG_Success with *ms = what they took
int rc_check(const void* out, const uint64_t* idx, const uint8_t* cells, size_t n, size_t B, float* ms) {
  clk::time_point t0 = clk::now();
  if (!out || B > RC_MAX_BLOBS) return KZG_InputsLengthsMismatch;
  const int st = recover_validate(idx, cells, n, B);
  *ms = ms_since(t0);
  return st;
}

int rc_entry(ctt_hip_peerdas_recovery* r, uint8_t* blobs, uint8_t* coefs_le, uint8_t* consistent, const uint64_t* idx, const uint8_t* cells,
             size_t n, size_t B) {
  try {
    float check_ms = 0;
    if (!r) return KZG_InputsLengthsMismatch;
    const int st = rc_check(blobs ? blobs : coefs_le, idx, cells, n, B, &check_ms);
    if (st != KZG_Success || B == 0) return st;
    return rc_recover(r, blobs, coefs_le, consistent, idx, cells, n, B, check_ms);
  } catch (...) {   // (host memory: nothing crosses the C ABI)
    return GPU_UNAVAILABLE;
  }
}

// recover_blobs into host memory, then the main library's prover blob by blob; the outputs are written after the last proof
int rc_cells_and_proofs(ctt_hip_peerdas_recovery* r, const ctt_eth_kzg_context* ctx, uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* idx,
                        const uint8_t* cells, size_t n, size_t B, float check_ms) {
  constexpr size_t BLOB = (size_t)N_BLOB * 32, CELLS_OUT = (size_t)N_CELLS * 2048, PROOFS_OUT = (size_t)N_CELLS * 48;
  std::vector<uint8_t> blobs(B * BLOB), c(B * CELLS_OUT), p(B * PROOFS_OUT);
  int st = rc_recover(r, blobs.data(), nullptr, nullptr, idx, cells, n, B, check_ms);
  if (st != KZG_Success) return st;
  clk::time_point t0 = clk::now();
  for (size_t b = 0; b < B && st == KZG_Success; b++)
    st = ctt_eth_kzg_compute_cells_and_kzg_proofs(ctx, (ctt_eth_kzg_cell*)(c.data() + b * CELLS_OUT), (ctt_eth_kzg_proof*)(p.data() + b * PROOFS_OUT),
                                                  (const ctt_eth_kzg_blob*)(blobs.data() + b * BLOB));
  if (st != KZG_Success) return st;
  {
    std::lock_guard<std::mutex> lock(r->mu);
    r->ms[4] = ms_since(t0);
  }
  memcpy(cells_out, c.data(), c.size());
  memcpy(proofs_out, p.data(), p.size());
  return KZG_Success;
}

std::mutex g_default_mu;
ctt_hip_peerdas_recovery* g_default = nullptr;   // lives as long as the process

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

ctt_hip_peerdas_recovery* ctt_hip_peerdas_recovery_create(int device) {
  ctt_hip_peerdas_recovery* r = new (std::nothrow) ctt_hip_peerdas_recovery();
  if (!r) return nullptr;
  r->device = device;
  r->hip = ctt_hip_msm_ctx_create(device);   // NULL without a usable device
  bool ok = r->hip != nullptr;
  if (ok) {
    uint64_t w13[4], w12[4];
    const FrH w = root_of_unity(13);
    from_mont<FrH>(w, w13);
    from_mont<FrH>(FrH::sqr(w), w12);
    r->plan13 = ctt_hip_fr_ntt_plan_create(r->hip, CTT_HIP_BLS12_381_G1, 13, w13, 0);
    r->plan12 = ctt_hip_fr_ntt_plan_create(r->hip, CTT_HIP_BLS12_381_G1, 12, w12, 0);
    RcDeviceScope scope(device);
    ok = r->plan13 && r->plan12 && scope.ok && hipMalloc(&r->d_const, CONST_BYTES) == hipSuccess;
  }
  if (!ok) {
    rc_release(r);
    delete r;
    return nullptr;
  }
  return r;
}

void ctt_hip_peerdas_recovery_destroy(ctt_hip_peerdas_recovery* rec) {
  if (!rec) return;
  rc_release(rec);
  delete rec;
}

int ctt_hip_peerdas_recover_blobs(ctt_hip_peerdas_recovery* rec, uint8_t* blobs, uint8_t* consistent, const uint64_t* cell_indices,
                                  const uint8_t* cells, size_t n, size_t B) {
  return rc_entry(rec, blobs, nullptr, consistent, cell_indices, cells, n, B);
}

int ctt_hip_peerdas_recover_coefficients(ctt_hip_peerdas_recovery* rec, uint8_t* coefs_le, uint8_t* consistent, const uint64_t* cell_indices,
                                         const uint8_t* cells, size_t n, size_t B) {
  return rc_entry(rec, nullptr, coefs_le, consistent, cell_indices, cells, n, B);
}

ctt_eth_kzg_status ctt_hip_eth_kzg_recover_cells_and_kzg_proofs_batch(ctt_hip_peerdas_recovery* rec, const ctt_eth_kzg_context* ctx,
                                                                      ctt_eth_kzg_cell* cells_out, ctt_eth_kzg_proof* proofs_out,
                                                                      const uint64_t* cell_indices, const ctt_eth_kzg_cell* cells, size_t n,
                                                                      size_t B) {
  try {
    float check_ms = 0;
    if (!rec || !ctx || !proofs_out) return (ctt_eth_kzg_status)KZG_InputsLengthsMismatch;
    const int st = rc_check(cells_out, cell_indices, (const uint8_t*)cells, n, B, &check_ms);
    if (st != KZG_Success || B == 0) return (ctt_eth_kzg_status)st;
    return (ctt_eth_kzg_status)rc_cells_and_proofs(rec, ctx, (uint8_t*)cells_out, (uint8_t*)proofs_out, cell_indices, (const uint8_t*)cells, n, B,
                                                   check_ms);
  } catch (...) {
    return (ctt_eth_kzg_status)GPU_UNAVAILABLE;
  }
}

ctt_eth_kzg_status ctt_eth_kzg_recover_cells_and_kzg_proofs(const ctt_eth_kzg_context* ctx, ctt_eth_kzg_cell* recovered_cells,
                                                            ctt_eth_kzg_proof* recovered_proofs, const uint64_t* cell_indices,
                                                            const ctt_eth_kzg_cell* cells, size_t num_cells) {
  try {
    float check_ms = 0;
    if (!ctx || !recovered_proofs) return (ctt_eth_kzg_status)KZG_InputsLengthsMismatch;
    const int st = rc_check(recovered_cells, cell_indices, (const uint8_t*)cells, num_cells, 1, &check_ms);
    if (st != KZG_Success) return (ctt_eth_kzg_status)st;
    ctt_hip_peerdas_recovery* r;
    {
      std::lock_guard<std::mutex> lock(g_default_mu);
      if (!g_default) {
        const char* dev = getenv("CTT_HIP_DEVICE");
        g_default = ctt_hip_peerdas_recovery_create(dev ? atoi(dev) : 0);
      }
      r = g_default;
    }
    if (!r) return (ctt_eth_kzg_status)GPU_UNAVAILABLE;
    return (ctt_eth_kzg_status)rc_cells_and_proofs(r, ctx, (uint8_t*)recovered_cells, (uint8_t*)recovered_proofs, cell_indices, (const uint8_t*)cells,
                                                   num_cells, 1, check_ms);
  } catch (...) {
    return (ctt_eth_kzg_status)GPU_UNAVAILABLE;
  }
}

int ctt_hip_peerdas_recovery_constants(uint8_t* zc_le, uint8_t* izc5_le, const uint64_t* cell_indices, size_t n) {
  try {
    if (!zc_le || !izc5_le) return KZG_InputsLengthsMismatch;
    const int st = recover_validate_indices(cell_indices, n);
    if (st != KZG_Success) return st;
    FrH zc[N_CELLS], izc5[N_CELLS];
    int32_t slot[N_CELLS];
    recovery_constants(cell_indices, n, zc, izc5, slot);
    for (int k = 0; k < N_CELLS; k++) {
      uint64_t v[4];
      from_mont<FrH>(zc[k], v);
      memcpy(zc_le + 32 * k, v, 32);
      from_mont<FrH>(izc5[k], v);
      memcpy(izc5_le + 32 * k, v, 32);
    }
    return KZG_Success;
  } catch (...) {
    return GPU_UNAVAILABLE;
  }
}

int ctt_hip_peerdas_last_timings(const ctt_hip_peerdas_recovery* rec, float* ms, int cap) {
  if (!rec || !ms || cap <= 0) return 0;
  ctt_hip_peerdas_recovery* r = const_cast<ctt_hip_peerdas_recovery*>(rec);
  std::lock_guard<std::mutex> lock(r->mu);
  const int k = cap < 5 ? cap : 5;
  for (int i = 0; i < k; i++) ms[i] = r->ms[i];
  return k;
}

}  // extern "C"
#pragma GCC visibility pop
