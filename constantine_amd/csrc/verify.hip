// verify.hip -- EIP-7594 verify_cell_kzg_proof_batch on the GPU with the pairing check on the host: the C symbols of
// include/ctt_msm_hip_peerdas_verify.h (libctt_msm_hip_peerdas_verify.so).  A companion of libctt_msm_hip.so over its public C ABI --
// ctt_hip_msm_ctx_create / _destroy, ctt_hip_msm_stream, ctt_hip_fr_ntt*, ctt_hip_subgroup_check, ctt_hip_msm_device, ctt_hip_sha256 --
// and nothing of its insides.  The host logic and the bodies of the three kernels: verify_host.h; the pairing: pairing_host.h; the
// formulas: DESIGN.md section 16.
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ctt_msm_hip_peerdas_verify.h"
#include "verify_host.h"

using namespace ctt;
using namespace ctt::proto;

namespace {

constexpr int GPU_UNAVAILABLE = CTT_HIP_STATUS_GPU_UNAVAILABLE;

// one lane per point; one lane per (column, element): 8192; one lane per coefficient: 64
__global__ void __launch_bounds__(VF_BLOCK) k_vf_decompress(VfDecompressArgs a) { vf_decompress_body(a, blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(VF_BLOCK) k_vf_colsum(VfColsumArgs a) { vf_colsum_body(a, blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(CELL_ELEMS) k_vf_interp(VfInterpArgs a) { vf_interp_body(a, blockIdx.x * blockDim.x + threadIdx.x); }

// a failed HIP call ends the call with GPU_UNAVAILABLE; the runtime's sticky error is read away
#define VF_HIP(x)                         \
  do {                                    \
    if ((x) != hipSuccess) {              \
      (void)hipGetLastError();            \
      return GPU_UNAVAILABLE;             \
    }                                     \
  } while (0)

// the calling thread's device is the caller's business: selected for the duration of a call, put back afterwards
struct VfDeviceScope {
  int prev = -1;
  bool ok = false;
  explicit VfDeviceScope(int device) {
    ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess;
    if (!ok) (void)hipGetLastError();
  }
  ~VfDeviceScope() {
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

constexpr size_t AFF = 96, ROWS_BYTES = (size_t)N_CELLS * CELL_ELEMS * 32;
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the parts of the workspace for up to `cap` cells (M <= n unique commitments)
struct VfLayout {
  size_t in, pts, status, cells, rho_r2, order, bad, ll, rl, total;
  explicit VfLayout(size_t cap) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
      const size_t here = at;
      at += align256(bytes);
      return here;
    };
    in = take(2 * cap * 48);                     // the compressed points: M commitments, n proofs
    pts = take((2 * cap + CELL_ELEMS) * AFF);    // C_0 .. C_{M-1} | [tau^0]_1 .. [tau^63]_1 | pi_0 .. pi_{n-1}
    status = take(2 * cap * 4);
    cells = take(cap * 2048);
    rho_r2 = take(cap * 32);
    order = take(cap * 4);
    bad = take(cap * 4);
    ll = take(cap * 32);
    rl = take((2 * cap + CELL_ELEMS) * 32);
    total = at;
  }
};

}  // namespace

struct ctt_hip_peerdas_verifier {
  std::mutex mu;
  int device = 0;
  ctt_hip_msm_ctx* hip = nullptr;
  ctt_hip_ntt_plan* plan6 = nullptr;   // 64 points, omega_64 = omega_8192^128
  G2Aff tau64;                         // [tau^64]_2
  std::vector<FrH> ck;                 // h_j^64
  void* d_tau = nullptr;               // 64 affine points
  void* d_hinv = nullptr;              // h_j^(-i), 128 x 64
  void* d_rows = nullptr;              // S, then a: 128 x 64
  void* d_start = nullptr;             // 129 words
  void* d_work = nullptr;              // VfLayout(cap), grow-only
  size_t cap = 0;
  float ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

void vf_release(ctt_hip_peerdas_verifier* v) {
  VfDeviceScope scope(v->device);
  for (void* d : {v->d_tau, v->d_hinv, v->d_rows, v->d_start, v->d_work})
    if (d) (void)hipFree(d);
  if (v->plan6) ctt_hip_fr_ntt_plan_destroy(v->hip, v->plan6);
  if (v->hip) ctt_hip_msm_ctx_destroy(v->hip);
  (void)hipGetLastError();
}

int vf_reserve(ctt_hip_peerdas_verifier* v, size_t n) {
  if (n <= v->cap) return KZG_Success;
  if (v->d_work) (void)hipFree(v->d_work);
  v->d_work = nullptr;
  v->cap = 0;
  VF_HIP(hipMalloc(&v->d_work, VfLayout(n).total));
  v->cap = n;
  return KZG_Success;
}

// The whole call for arguments that passed verify_check_arguments, n >= 1.  ll, rl, r_be (all three or none): the test-facing outputs,
// written at the very end; with them the pairing is left out.
int vf_run(ctt_hip_peerdas_verifier* v, uint8_t* ll_out, uint8_t* rl_out, uint8_t* r_be, const uint8_t* commitments, const uint64_t* idx,
           const uint8_t* cells, const uint8_t* proofs, size_t n, const uint8_t* rnd, clk::time_point t0) {
  std::lock_guard<std::mutex> lock(v->mu);
  VfDeviceScope scope(v->device);
  if (!scope.ok) return GPU_UNAVAILABLE;
  hipStream_t s = (hipStream_t)ctt_hip_msm_stream(v->hip);
  if (!s) return GPU_UNAVAILABLE;   // the context was lost to an earlier HIP failure
  float ms[6] = {0, 0, 0, 0, 0, 0};

  // the host's share: the unique commitments, the challenge, the scalar vectors, the column lists
  std::vector<uint32_t> cidx, order;
  std::vector<uint8_t> uniq, transcript;
  verify_dedup(commitments, n, cidx, uniq);
  const size_t M = uniq.size() / 48, npts = M + n, nall = M + CELL_ELEMS + n;
  uint64_t r[4];
  if (!verify_blinding(r, rnd)) {
    uint8_t digest[32];
    verify_transcript(transcript, uniq.data(), M, cidx.data(), idx, cells, proofs, n);
    ctt_hip_sha256(digest, transcript.data(), transcript.size());
    reduce_256_mod_r(digest, r);
  }
  std::vector<uint64_t> rho_r2, ll_sc, rl_sc;
  verify_scalars(r, idx, cidx.data(), n, M, v->ck, rho_r2, ll_sc, rl_sc);
  uint32_t start[N_CELLS + 1];
  verify_column_lists(idx, n, start, order);

  const int rc = vf_reserve(v, n);
  if (rc != KZG_Success) return rc;
  const VfLayout L(v->cap);
  uint8_t* w = (uint8_t*)v->d_work;
  uint8_t* d_pts = w + L.pts;
  VF_HIP(hipMemcpyAsync(w + L.in, uniq.data(), M * 48, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.in + M * 48, proofs, n * 48, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(d_pts + M * AFF, v->d_tau, CELL_ELEMS * AFF, hipMemcpyDeviceToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.cells, cells, n * 2048, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.rho_r2, rho_r2.data(), n * 32, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.order, order.data(), n * 4, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(v->d_start, start, sizeof start, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.ll, ll_sc.data(), n * 32, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemcpyAsync(w + L.rl, rl_sc.data(), nall * 32, hipMemcpyHostToDevice, s));
  VF_HIP(hipMemsetAsync(w + L.bad, 0, n * 4, s));
  VF_HIP(hipStreamSynchronize(s));
  ms[0] = ms_since(t0);

  // 1. the M + n points: lane i < M writes record i, lane M + k record M + 64 + k
  hipLaunchKernelGGL(k_vf_decompress, dim3((uint32_t)((npts + VF_BLOCK - 1) / VF_BLOCK)), dim3(VF_BLOCK), 0, s,
                     VfDecompressArgs{w + L.in, (uint32_t*)d_pts, (uint32_t*)(w + L.status), (uint32_t)npts, (uint32_t)M, (uint32_t)CELL_ELEMS});
  VF_HIP(hipGetLastError());
  VF_HIP(hipStreamSynchronize(s));
  ms[1] = ms_since(t0);
  // 2. all of them in the subgroup? (the 64 points of the setup lie between them and are checked again: one call, one launch)
  std::vector<uint8_t> ok_all(nall), ok(npts);
  if (ctt_hip_subgroup_check(v->hip, CTT_HIP_BLS12_381_G1, ok_all.data(), d_pts, nall, 1) != 0) return GPU_UNAVAILABLE;
  memcpy(ok.data(), ok_all.data(), M);
  memcpy(ok.data() + M, ok_all.data() + M + CELL_ELEMS, n);
  ms[2] = ms_since(t0);
  // 3. the scalars: validated, weighted and summed by column
  hipLaunchKernelGGL(k_vf_colsum, dim3(VF_COLSUM_LANES / VF_BLOCK), dim3(VF_BLOCK), 0, s,
                     VfColsumArgs{w + L.cells, (const uint32_t*)(w + L.rho_r2), (const uint32_t*)v->d_start, (const uint32_t*)(w + L.order),
                                  (uint32_t*)v->d_rows, (uint32_t*)(w + L.bad)});
  VF_HIP(hipGetLastError());
  std::vector<uint32_t> status(npts), bad(n);
  VF_HIP(hipMemcpyAsync(status.data(), w + L.status, npts * 4, hipMemcpyDeviceToHost, s));
  VF_HIP(hipMemcpyAsync(bad.data(), w + L.bad, n * 4, hipMemcpyDeviceToHost, s));
  VF_HIP(hipStreamSynchronize(s));
  const int st = verify_first_offender(status.data(), ok.data(), M, bad.data(), n);
  if (st != KZG_Success) {
    ms[3] = ms_since(t0);
    memcpy(v->ms, ms, sizeof ms);
    return st;
  }
  //    one inverse transform per column, then the 64 coefficients, negated, into the scalars of RL
  if (ctt_hip_fr_ntt(v->hip, v->plan6, v->d_rows, v->d_rows, N_CELLS, CTT_HIP_NTT_INVERSE | CTT_HIP_NTT_IN_BRP | CTT_HIP_NTT_IN_MONT | CTT_HIP_NTT_OUT_MONT,
                     nullptr) != 0)
    return GPU_UNAVAILABLE;
  hipLaunchKernelGGL(k_vf_interp, dim3(1), dim3(CELL_ELEMS), 0, s,
                     VfInterpArgs{(const uint32_t*)v->d_rows, (const uint32_t*)v->d_hinv, (uint32_t*)(w + L.rl + M * 32)});
  VF_HIP(hipGetLastError());
  VF_HIP(hipStreamSynchronize(s));
  ms[3] = ms_since(t0);
  // 4. the two sides
  uint8_t ll_aff[AFF], rl_aff[AFF];
  if (ctt_hip_msm_device(v->hip, CTT_HIP_BLS12_381_G1, CTT_HIP_COEF_FR, CTT_HIP_OUT_AFF, ll_aff, w + L.ll, d_pts + (M + CELL_ELEMS) * AFF, n) != 0)
    return GPU_UNAVAILABLE;
  if (ctt_hip_msm_device(v->hip, CTT_HIP_BLS12_381_G1, CTT_HIP_COEF_FR, CTT_HIP_OUT_AFF, rl_aff, w + L.rl, d_pts, nall) != 0) return GPU_UNAVAILABLE;
  ms[4] = ms_since(t0);
  int verdict = KZG_Success;
  if (ll_out) {
    g1_compress(ll_out, ll_aff);
    g1_compress(rl_out, rl_aff);
    limbs_to_be<FrH>(r, r_be);
  } else {
    // 5. e(LL, [tau^64]_2) e(-RL, G_2) == 1
    G1Aff P[2] = {g1_from_bytes(ll_aff), g1_from_bytes(rl_aff)};
    P[1].y = FpH::neg(P[1].y);
    const G2Aff Q[2] = {v->tau64, g2_generator()};
    verdict = pairing_check(P, Q, 2) ? KZG_Success : KZG_VerificationFailure;
    ms[5] = ms_since(t0);
  }
  memcpy(v->ms, ms, sizeof ms);
  return verdict;
}

int vf_entry(ctt_hip_peerdas_verifier* v, uint8_t* ll, uint8_t* rl, uint8_t* r_be, const uint8_t* commitments, const uint64_t* idx,
             const uint8_t* cells, const uint8_t* proofs, size_t n, const uint8_t* rnd) {
  try {
    clk::time_point t0 = clk::now();
    const int st = verify_check_arguments(v != nullptr, commitments, idx, cells, proofs, rnd, n);
    if (st != KZG_Success || n == 0) return st;
    return vf_run(v, ll, rl, r_be, commitments, idx, cells, proofs, n, rnd, t0);
  } catch (...) {   // (host memory: nothing crosses the C ABI)
    return GPU_UNAVAILABLE;
  }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

ctt_hip_peerdas_verifier* ctt_hip_peerdas_verifier_create(int device, const uint8_t* g1_monomial_64, const uint8_t* g2_tau64) {
  try {
    if (!g1_monomial_64 || !g2_tau64) return nullptr;
    // the 65 points: decompressed here, subgroup-checked below by the main library
    std::vector<uint8_t> tau((size_t)CELL_ELEMS * AFF);
    uint8_t g2[192];
    for (int i = 0; i < CELL_ELEMS; i++) {
      if (g1_decompress(&tau[i * AFF], g1_monomial_64 + 48 * i) != KZG_Success) return nullptr;
      if (g1_from_bytes(&tau[i * AFF]).is_inf()) return nullptr;
    }
    if (g2_decompress(g2, g2_tau64) != KZG_Success || g2_from_bytes(g2).is_inf()) return nullptr;
    ctt_hip_peerdas_verifier* v = new (std::nothrow) ctt_hip_peerdas_verifier();
    if (!v) return nullptr;
    v->device = device;
    v->tau64 = g2_from_bytes(g2);
    v->hip = ctt_hip_msm_ctx_create(device);   // NULL without a usable device
    bool ok = v->hip != nullptr;
    if (ok) {
      uint8_t in_g1[CELL_ELEMS], in_g2 = 0;
      ok = ctt_hip_subgroup_check(v->hip, CTT_HIP_BLS12_381_G1, in_g1, tau.data(), CELL_ELEMS, 0) == 0 &&
           ctt_hip_subgroup_check(v->hip, CTT_HIP_BLS12_381_G2, &in_g2, g2, 1, 0) == 0 && in_g2 == 1;
      for (int i = 0; ok && i < CELL_ELEMS; i++) ok = in_g1[i] == 1;
    }
    if (ok) {
      const FrH w13 = root_of_unity(13);
      v->ck = cell_coset_constants(w13);
      uint64_t w6[4];
      from_mont<FrH>(root_of_unity(6), w6);   // 7^((r-1)/64) = omega_8192^128
      v->plan6 = ctt_hip_fr_ntt_plan_create(v->hip, CTT_HIP_BLS12_381_G1, 6, w6, 0);
      std::vector<uint32_t> hinv;
      verify_hinv_table(hinv);
      VfDeviceScope scope(device);
      ok = v->plan6 && scope.ok && hipMalloc(&v->d_tau, tau.size()) == hipSuccess && hipMalloc(&v->d_hinv, ROWS_BYTES) == hipSuccess &&
           hipMalloc(&v->d_rows, ROWS_BYTES) == hipSuccess && hipMalloc(&v->d_start, (N_CELLS + 1) * 4) == hipSuccess &&
           hipMemcpy(v->d_tau, tau.data(), tau.size(), hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(v->d_hinv, hinv.data(), ROWS_BYTES, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
      vf_release(v);
      delete v;
      return nullptr;
    }
    return v;
  } catch (...) {
    return nullptr;
  }
}

ctt_hip_peerdas_verifier* ctt_hip_peerdas_verifier_create_from_file(int device, const char* path) {
  try {
    if (!path) return nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return nullptr;
    // "4096\n65\n", 4096 Lagrange G1 lines, 65 monomial G2 lines, 4096 monomial G1 lines (protocols_host.h: srs_read_ckzg4844)
    unsigned n1 = 0, n2 = 0;
    bool ok = fscanf(f, "%4u\n", &n1) == 1 && n1 == (unsigned)N_BLOB && fscanf(f, "%4u\n", &n2) == 1 && n2 == 65u;
    uint8_t line[96], g2[96], g1[CELL_ELEMS * 48];
    for (int i = 0; ok && i < N_BLOB; i++) ok = srs_hex_line(f, 96, line);
    for (int i = 0; ok && i < 65; i++) {
      ok = srs_hex_line(f, 192, line);
      if (i == CELL_ELEMS) memcpy(g2, line, 96);
    }
    for (int i = 0; ok && i < N_BLOB; i++) {   // (a truncated file is refused, as the main library's reader refuses it)
      ok = srs_hex_line(f, 96, line);
      if (i < CELL_ELEMS) memcpy(g1 + 48 * i, line, 48);
    }
    fclose(f);
    return ok ? ctt_hip_peerdas_verifier_create(device, g1, g2) : nullptr;
  } catch (...) {
    return nullptr;
  }
}

void ctt_hip_peerdas_verifier_destroy(ctt_hip_peerdas_verifier* v) {
  if (!v) return;
  vf_release(v);
  delete v;
}

int ctt_hip_peerdas_verify_cell_kzg_proof_batch(ctt_hip_peerdas_verifier* v, const uint8_t* commitments, const uint64_t* cell_indices,
                                                const uint8_t* cells, const uint8_t* proofs, size_t n,
                                                const uint8_t secure_random_bytes[32]) {
  return vf_entry(v, nullptr, nullptr, nullptr, commitments, cell_indices, cells, proofs, n, secure_random_bytes);
}

int ctt_hip_peerdas_verify_lincombs(ctt_hip_peerdas_verifier* v, uint8_t ll[48], uint8_t rl[48], uint8_t r_be[32], const uint8_t* commitments,
                                    const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n,
                                    const uint8_t secure_random_bytes[32]) {
  if (!ll || !rl || !r_be) return KZG_InputsLengthsMismatch;
  return vf_entry(v, ll, rl, r_be, commitments, cell_indices, cells, proofs, n, secure_random_bytes);
}

int ctt_hip_peerdas_verify_challenge(uint8_t r_be[32], const uint8_t* commitments, size_t m, const uint64_t* commitment_indices,
                                     const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n) {
  try {
    if (!r_be || (m && !commitments) || (n && (!commitment_indices || !cell_indices || !cells || !proofs))) return KZG_InputsLengthsMismatch;
    std::vector<uint8_t> transcript;
    verify_transcript(transcript, commitments, m, commitment_indices, cell_indices, cells, proofs, n);
    uint8_t digest[32];
    ctt_hip_sha256(digest, transcript.data(), transcript.size());
    uint64_t r[4];
    reduce_256_mod_r(digest, r);
    limbs_to_be<FrH>(r, r_be);
    return KZG_Success;
  } catch (...) {
    return GPU_UNAVAILABLE;
  }
}

int ctt_hip_peerdas_pairing_check(const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n) {
  try {
    if (n && (!g1_aff || !g2_aff)) return -1;
    std::vector<G1Aff> P(n);
    std::vector<G2Aff> Q(n);
    for (size_t i = 0; i < n; i++) {
      P[i] = g1_from_bytes(g1_aff + AFF * i);
      Q[i] = g2_from_bytes(g2_aff + 2 * AFF * i);
    }
    return pairing_check(P.data(), Q.data(), n) ? 1 : 0;
  } catch (...) {
    return -1;
  }
}

int ctt_hip_peerdas_verify_last_timings(const ctt_hip_peerdas_verifier* ver, float* ms, int cap) {
  if (!ver || !ms || cap <= 0) return 0;
  ctt_hip_peerdas_verifier* v = const_cast<ctt_hip_peerdas_verifier*>(ver);
  std::lock_guard<std::mutex> lock(v->mu);
  const int k = cap < 6 ? cap : 6;
  for (int i = 0; i < k; i++) ms[i] = v->ms[i];
  return k;
}

}  // extern "C"
#pragma GCC visibility pop
