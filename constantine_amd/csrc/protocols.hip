// protocols.hip -- the MSM's immediate callers behind the reference's own C symbols:
//
//   EIP-4844 KZG    ctt_eth_kzg_blob_to_kzg_commitment / _compute_kzg_proof / _compute_blob_kzg_proof and the context
//                   constructor / destructor   (include/constantine/protocols/ethereum_eip4844_kzg.h:106,126,153,200,238;
//                   constantine/ethereum_eip4844_kzg.nim:297-444, commitments/kzg.nim:186-223)
//   EIP-2537        ctt_eth_evm_bls12381_g1msm / _g2msm   (include/constantine/protocols/ethereum_evm_precompiles.h:386,419;
//                   constantine/ethereum_evm_precompiles.nim:316-389,894-1060)
//
// Host side: protocols_host.h, plain C++ that tests/protocols_harness.cpp runs without a GPU -- wire formats, range / curve checks,
// the Fiat-Shamir hash, point (de)compression, the trusted setup's text reader, the precompiles' parser and encoder; this file reads
// no wire-format byte itself.  GPU side, here: the KZG context, every MSM (cached SRS: ctt_hip_msm_with_bases; precompile inputs:
// ctt_hip_msm_host), the subgroup checks (ctt_hip_subgroup_check) and the quotient polynomial of an opening (ctt_hip_fr_quotient; the
// branch "z is a root of unity" runs the reference's other formula on the host).  The EIP-4844 verifications are not provided; the EIP-7594 batch
// verification, with its one pairing check on the host, is the companion library of verify.hip.
//
//   EIP-7594 PeerDAS ctt_eth_kzg_compute_cells_and_kzg_proofs (include/constantine/protocols/ethereum_eip7594_peerdas.h) and the
//                   cells alone (ctt_hip_eth_kzg_compute_cells): the blob's coefficients, the coset evaluations and the 128 cell
//                   quotients' evaluations are transforms of ctt_hip_fr_ntt (ntt.hip), the quotients one kernel here
//                   (k_cell_quotients), the proofs 128 MSMs over the context's Lagrange points: one pass of the batched fixed-base
//                   MSM (fixed.h; its table is built at the first proof call), or -- CTT_HIP_CELL_PROOFS=loop, or no memory for the
//                   table -- a loop over the cached bases.  Recovery, the batch verification (pairings) and the FK20 form are out
//                   of scope.  DESIGN.md sections 13 and 14.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <system_error>
#include <thread>

#include "fixed.h"
#include "fixed_bodies.h"   // (the range of window sizes)
#include "hip_errors.h"
#include "msm_pipeline.h"   // (OutOfDeviceMemory)
#include "protocols_host.h"

// (part 3 of the header declares this file's symbols with the reference's packed enums and byte-array structs; the definitions
// below spell the same ABI with uint8_t and plain pointers, so the typed declarations stay out of this translation unit)
#define CTT_MSM_HIP_NO_PROTOCOLS 1
#include "../../include/ctt_msm_hip.h"

using namespace ctt;
using namespace ctt::proto;

namespace {

// a failed HIP call inside a protocol symbol: recorded as the thread's last error and thrown to the symbol's boundary, which
// returns CTT_HIP_STATUS_GPU_UNAVAILABLE -- rounds 1-4 aborted here (hip_errors.h)
#define PROT_HIP_CHECK(x)                                                                                          \
  do {                                                                                                             \
    hipError_t e_ = (x);                                                                                           \
    if (e_ != hipSuccess) ::ctt::hip_failed(#x, hipGetErrorString(e_), e_ == hipErrorOutOfMemory, __FILE__, __LINE__); \
  } while (0)

// What a protocol symbol returns when the GPU cannot serve the call: a value outside every status enum of the reference
// (ctt_eth_kzg_status 0..9, ctt_eth_trusted_setup_status 0..2, ctt_evm_status 0..6 -- their *_status_to_string print
// "InvalidStatusCode" for it); ctt_hip_last_error() / _message() of the calling thread say why.  Outputs are untouched.
constexpr uint8_t GPU_UNAVAILABLE = CTT_HIP_STATUS_GPU_UNAVAILABLE;

// the body of a protocol symbol with the GPU's failures turned into that status
template <class Fn>
uint8_t gpu_guarded(Fn&& fn) {
  ErrorGuard guard;
  try {
    return (uint8_t)fn();
  } catch (const HipFailure&) {
    return GPU_UNAVAILABLE;
  } catch (const OutOfDeviceMemory& e) {
    set_last_error(ERR_OUT_OF_MEMORY, "out of device memory (%zu bytes requested)", e.bytes);
    return GPU_UNAVAILABLE;
  }
}

}  // namespace

// ---- the KZG context: the Lagrange SRS in bit-reversal order cached on the GPU, the domain next to it ---------------------
struct ctt_eth_kzg_context_struct {
  std::mutex mu;
  ctt_hip_msm_ctx* hip = nullptr;
  bool own_hip = false;
  int device = 0;
  ctt_hip_msm_bases* bases = nullptr;
  std::vector<FrH> domain;      // bit-reversed roots of unity, Montgomery
  void* d_domain = nullptr;     // the same on the device (ctt_hip_fr_quotient's layout)
  void* d_poly = nullptr;       // 4096 canonical scalars of the blob being opened
  void* d_q = nullptr;          // quotient evaluations (never leave the GPU before the MSM)
  // EIP-7594: one plan of size 4096 serves the inverse transform of the blob, the coset transform of the cells and the batched one
  // of the cell quotients (a plan of ctt_hip_fr_ntt runs both directions); c_k of the 128 cells; the blob's coefficients (Montgomery)
  // and coset evaluations; the 128 x 4096 quotient coefficients / evaluations (16 MiB, allocated at the first proof call)
  ctt_hip_ntt_plan* ntt = nullptr;
  void* d_ck = nullptr;
  void* d_coef = nullptr;
  void* d_coset = nullptr;
  void* d_cellq = nullptr;
  uint8_t coset_shift[32];      // omega_8192, canonical
  float cell_ms[7] = {0, 0, 0, 0, 0, 0, 0};   // the last cells call: parse + upload, INTT, coset NTT, quotients, batched NTT, MSM loop, compress + copy back
  // the cell proofs as one batched fixed-base MSM (fixed.h): the Lagrange points in the order of `bases`, kept on the host until the
  // table is built at the first proof call; $CTT_HIP_CELL_PROOFS=loop at creation keeps the loop over `bases`, and so does a table
  // that could not be allocated.  $CTT_HIP_CELL_PROOFS_C overrides the window bits.
  std::vector<uint8_t> lagrange_aff;
  FixedTable* fixed = nullptr;
  bool proofs_loop = false;
  int proofs_c = 0;
  float cell_path[2] = {0, 0};   // the last cells call: rows the table kernel served (128 or 0), ms it paid for building the table
};

namespace {

// gives back what the context owns on the GPU, with `with_hip` its MSM context too; the struct itself is the caller's to delete
void kzg_context_release(ctt_eth_kzg_context_struct* c, bool with_hip) {
  if (c->bases) ctt_hip_msm_bases_destroy(c->hip, c->bases);
  for (void* d : {c->d_domain, c->d_poly, c->d_q, c->d_ck, c->d_coef, c->d_coset, c->d_cellq})
    if (d) (void)hipFree(d);
  if (c->ntt) ctt_hip_fr_ntt_plan_destroy(c->hip, c->ntt);
  delete c->fixed;   // (before the MSM context: the table works on its stream)
  c->fixed = nullptr;
  if (with_hip && c->hip) ctt_hip_msm_ctx_destroy(c->hip);
}

// the cell quotients of EIP-7594 (the body and its formula: protocols_host.h)
__global__ void __launch_bounds__(256) k_cell_quotients(CellQuotArgs a) { cell_quotient_body(a, blockIdx.x * blockDim.x + threadIdx.x); }

// srs: 4096 x 48 compressed G1 Lagrange points in ceremony (file) order
int kzg_context_build(ctt_eth_kzg_context_struct** out, const uint8_t* srs, int device, int table) {
  std::vector<uint8_t> aff((size_t)N_BLOB * 96);
  std::vector<int> status(N_BLOB, 0);
  // 4096 square roots (380 squarings each): a few host threads
  const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nth; t++)
    th.emplace_back([&, t]() {
      for (int i = (int)t; i < N_BLOB; i += (int)nth)   // the commitment uses the points in bit-reversal order
        status[i] = g1_decompress(aff.data() + (size_t)bit_reverse((uint32_t)i, 12) * 96, srs + (size_t)i * 48);
    });
  for (std::thread& x : th) x.join();
  for (int i = 0; i < N_BLOB; i++)
    if (status[i] != KZG_Success) return TS_InvalidFile;
  ctt_eth_kzg_context_struct* c = new ctt_eth_kzg_context_struct();
  c->device = device;
  auto fail = [&](int st) {
    kzg_context_release(c, true);   // (the MSM context whenever there is one: it was created here)
    delete c;
    return st;
  };
  c->hip = ctt_hip_msm_ctx_create(device);
  if (!c->hip) return fail(GPU_UNAVAILABLE);            // no usable device: ctt_hip_last_error() == -3
  c->own_hip = true;
  std::vector<uint8_t> ok(N_BLOB);
  if (ctt_hip_subgroup_check(c->hip, CTT_HIP_BLS12_381_G1, ok.data(), aff.data(), N_BLOB, 0) != 0) return fail(GPU_UNAVAILABLE);
  for (int i = 0; i < N_BLOB; i++)
    if (!ok[i]) return fail(TS_InvalidFile);
  c->bases = table ? ctt_hip_msm_bases_create_table(c->hip, CTT_HIP_BLS12_381_G1, aff.data(), N_BLOB, 0, 0)
                   : ctt_hip_msm_bases_create(c->hip, CTT_HIP_BLS12_381_G1, aff.data(), N_BLOB, 0);
  if (!c->bases) return fail(GPU_UNAVAILABLE);
  {
    const char* mode = getenv("CTT_HIP_CELL_PROOFS");
    const char* bits = getenv("CTT_HIP_CELL_PROOFS_C");
    c->proofs_loop = mode && !strcmp(mode, "loop");
    c->proofs_c = bits ? atoi(bits) : 0;
    if (c->proofs_c < FX_MIN_WINDOW_BITS || c->proofs_c > FX_MAX_WINDOW_BITS) c->proofs_c = 0;   // not a window size: the default, never a refused call
    if (!c->proofs_loop) c->lagrange_aff = std::move(aff);
  }
  c->domain = domain_brp();
  try {
    DeviceScope device_scope(device);
    PROT_HIP_CHECK(hipMalloc(&c->d_domain, (size_t)N_BLOB * 32));
    PROT_HIP_CHECK(hipMalloc(&c->d_poly, (size_t)N_BLOB * 32));
    PROT_HIP_CHECK(hipMalloc(&c->d_q, (size_t)N_BLOB * 32));
    PROT_HIP_CHECK(hipMemcpy(c->d_domain, c->domain.data(), (size_t)N_BLOB * 32, hipMemcpyHostToDevice));
    // EIP-7594: the c_k of the 128 cells; the coset shift of the second half of the extended evaluations
    const FrH w8192 = root_of_unity(13);
    const std::vector<FrH> ck = cell_coset_constants(w8192);
    uint64_t g[4];
    from_mont<FrH>(w8192, g);
    memcpy(c->coset_shift, g, 32);
    PROT_HIP_CHECK(hipMalloc(&c->d_ck, (size_t)N_CELLS * 32));
    PROT_HIP_CHECK(hipMalloc(&c->d_coef, (size_t)N_BLOB * 32));
    PROT_HIP_CHECK(hipMalloc(&c->d_coset, (size_t)N_BLOB * 32));
    PROT_HIP_CHECK(hipMemcpy(c->d_ck, ck.data(), (size_t)N_CELLS * 32, hipMemcpyHostToDevice));
  } catch (const HipFailure&) {
    return fail(GPU_UNAVAILABLE);
  }
  {
    uint64_t w[4];
    from_mont<FrH>(root_of_unity(12), w);
    c->ntt = ctt_hip_fr_ntt_plan_create(c->hip, CTT_HIP_BLS12_381_G1, 12, w, 0);
    if (!c->ntt) return fail(GPU_UNAVAILABLE);
  }
  *out = c;
  return TS_Success;
}

// [proof]_1 and y = p(z) for a validated polynomial (canonical scalars) and challenge
// -> KZG_Success, or GPU_UNAVAILABLE when the GPU refused (nothing written)
int kzg_prove(ctt_eth_kzg_context_struct* c, uint8_t proof[48], uint64_t y_c[4], const uint8_t* poly_le, const uint64_t z_c[4]) {
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceScope device_scope(c->device);
  hipStream_t s = (hipStream_t)ctt_hip_msm_stream(c->hip);
  if (!s) return GPU_UNAVAILABLE;                       // the context was lost to an earlier HIP failure
  PROT_HIP_CHECK(hipMemcpyAsync(c->d_poly, poly_le, (size_t)N_BLOB * 32, hipMemcpyHostToDevice, s));
  uint8_t r_aff[96];
  uint64_t y_tmp[4];
  const int rc = ctt_hip_fr_quotient(c->hip, CTT_HIP_BLS12_381_G1, c->d_q, y_tmp, c->d_poly, c->d_domain, z_c, N_BLOB);
  int mrc;
  if (rc == 0) {
    mrc = ctt_hip_msm_with_bases(c->hip, c->bases, CTT_HIP_COEF_BIG, CTT_HIP_OUT_AFF, r_aff, c->d_q, N_BLOB, 1);
  } else if (rc == -2) {   // z is one of the roots of unity: the reference's other formula, on the host
    std::vector<uint8_t> q((size_t)N_BLOB * 32);
    quotient_host(c->domain, poly_le, z_c, q.data(), y_tmp);
    mrc = ctt_hip_msm_with_bases(c->hip, c->bases, CTT_HIP_COEF_BIG, CTT_HIP_OUT_AFF, r_aff, q.data(), N_BLOB, 0);
  } else {
    return GPU_UNAVAILABLE;
  }
  if (mrc != 0) return GPU_UNAVAILABLE;
  memcpy(y_c, y_tmp, 32);
  g1_compress(proof, r_aff);
  return KZG_Success;
}

// EIP-7594 compute_cells / compute_cells_and_kzg_proofs (ethereum_eip7594_peerdas.h; the formulas: DESIGN.md section 13) for a
// validated polynomial.  cells: 128 x 2048 bytes or NULL; proofs: 128 x 48 bytes or NULL; q_le: 128 x 4096 canonical quotient
// coefficients or NULL (the probe of the quotient kernel; nothing else is computed then).  Outputs are written at the very end only.
int kzg_cells(ctt_eth_kzg_context_struct* c, uint8_t* cells, uint8_t* proofs, uint8_t* q_le, const uint8_t* blob, const uint8_t* poly_le, float parse_ms) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point& t0) {
    const clk::time_point t1 = clk::now();
    const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  };
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceScope device_scope(c->device);
  hipStream_t s = (hipStream_t)ctt_hip_msm_stream(c->hip);
  if (!s) return GPU_UNAVAILABLE;
  float ms[7] = {0, 0, 0, 0, 0, 0, 0};
  float path[2] = {0, 0};
  clk::time_point t0 = clk::now();
  PROT_HIP_CHECK(hipMemcpyAsync(c->d_poly, poly_le, (size_t)N_BLOB * 32, hipMemcpyHostToDevice, s));
  PROT_HIP_CHECK(hipStreamSynchronize(s));
  ms[0] = parse_ms + ms_since(t0);
  // 1. coefficients: the blob holds evaluations in bit-reversed order
  if (ctt_hip_fr_ntt(c->hip, c->ntt, c->d_coef, c->d_poly, 1, CTT_HIP_NTT_INVERSE | CTT_HIP_NTT_IN_BRP | CTT_HIP_NTT_OUT_MONT, nullptr) != 0)
    return GPU_UNAVAILABLE;
  ms[1] = ms_since(t0);
  std::vector<uint8_t> coset;
  if (cells) {
    // 2. the second half of the extended evaluations: the coset omega_8192 * <omega_4096>, bit-reversed, canonical
    if (ctt_hip_fr_ntt(c->hip, c->ntt, c->d_coset, c->d_coef, 1, CTT_HIP_NTT_IN_MONT | CTT_HIP_NTT_OUT_BRP, c->coset_shift) != 0)
      return GPU_UNAVAILABLE;
    coset.resize((size_t)N_BLOB * 32);
    PROT_HIP_CHECK(hipMemcpyAsync(coset.data(), c->d_coset, coset.size(), hipMemcpyDeviceToHost, s));
    PROT_HIP_CHECK(hipStreamSynchronize(s));
    ms[2] = ms_since(t0);
  }
  std::vector<uint8_t> aff;
  std::vector<uint8_t> q_host;
  if (proofs || q_le) {
    if (!c->d_cellq) {
      const hipError_t e = hipMalloc(&c->d_cellq, (size_t)N_CELLS * N_BLOB * 32);
      if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        c->d_cellq = nullptr;
        throw OutOfDeviceMemory{(size_t)N_CELLS * N_BLOB * 32};
      }
      PROT_HIP_CHECK(e);
    }
    // 3. the 128 quotients by X^64 - c_k
    CellQuotArgs qa{(const uint32_t*)c->d_coef, (const uint32_t*)c->d_ck, (uint32_t*)c->d_cellq, q_le ? 1u : 0u};
    hipLaunchKernelGGL(k_cell_quotients, dim3(N_CELLS * CELL_ELEMS / 256), dim3(256), 0, s, qa);
    PROT_HIP_CHECK(hipGetLastError());
    if (q_le) {
      q_host.resize((size_t)N_CELLS * N_BLOB * 32);
      PROT_HIP_CHECK(hipMemcpyAsync(q_host.data(), c->d_cellq, q_host.size(), hipMemcpyDeviceToHost, s));
    }
    PROT_HIP_CHECK(hipStreamSynchronize(s));
    ms[3] = ms_since(t0);
  }
  if (proofs) {
    // 4. their evaluations over the domain of the Lagrange bases (bit-reversed, canonical: the MSM's coefficients), in place
    if (ctt_hip_fr_ntt(c->hip, c->ntt, c->d_cellq, c->d_cellq, N_CELLS, CTT_HIP_NTT_IN_MONT | CTT_HIP_NTT_OUT_BRP, nullptr) != 0) return GPU_UNAVAILABLE;
    ms[4] = ms_since(t0);
    aff.resize((size_t)N_CELLS * 96);
    // 5. the 128 MSMs in one pass over the table of the Lagrange points (built here the first time).  No memory for the table or its
    // workspace, or a table that refuses its arguments: the loop below serves the call, now and from now on, so that no call is refused
    // that the loop would have served; a failed HIP call is the GPU's.
    bool by_table = false;
    if (!c->proofs_loop) {
      int rc = FX_OK;
      if (!c->fixed) {
        FixedTable* t = new FixedTable(c->device, s);
        rc = t->build(FX_CURVE_BLS12_381_G1, c->lagrange_aff.data(), N_BLOB, c->proofs_c);
        if (rc == FX_OK) {
          c->fixed = t;
          path[1] = t->build_ms();
          std::vector<uint8_t>().swap(c->lagrange_aff);
        } else {
          if (rc == FX_HIP_ERROR) set_last_error(ERR_HIP_FAILURE, "cell proofs: %s", t->error());
          delete t;
        }
      }
      if (rc == FX_OK) {
        rc = c->fixed->msm_batch(FX_COEF_BIG, c->d_cellq, N_CELLS, aff.data(), FX_COEFS_ON_DEVICE);
        if (rc == FX_HIP_ERROR) set_last_error(ERR_HIP_FAILURE, "cell proofs: %s", c->fixed->error());
      }
      if (rc == FX_OUT_OF_MEMORY || rc == FX_REFUSED) {
        c->proofs_loop = true;
        delete c->fixed;
        c->fixed = nullptr;
        std::vector<uint8_t>().swap(c->lagrange_aff);
      } else if (rc != FX_OK) {
        return GPU_UNAVAILABLE;
      } else {
        by_table = true;
        path[0] = (float)N_CELLS;
      }
    }
    // ... or 128 MSMs over the cached bases, three tickets in flight (the header's advice for small MSMs)
    int ticket[N_CELLS];
    int submitted = 0, finished = by_table ? N_CELLS : 0;
    bool failed = false;
    while (!failed && finished < N_CELLS) {
      if (submitted < N_CELLS && submitted - finished < 3) {
        ticket[submitted] = ctt_hip_msm_with_bases_submit(c->hip, c->bases, CTT_HIP_COEF_BIG, (const uint8_t*)c->d_cellq + (size_t)submitted * N_BLOB * 32, N_BLOB);
        if (ticket[submitted] < 0) failed = true;
        else submitted++;
      } else {
        if (ctt_hip_msm_device_finish(c->hip, ticket[finished], CTT_HIP_OUT_AFF, aff.data() + (size_t)finished * 96) != 0) failed = true;
        finished++;
      }
    }
    if (failed) {   // give the outstanding tickets back: their slots would stay taken on this context
      uint8_t dummy[96];
      for (; finished < submitted; finished++) (void)ctt_hip_msm_device_finish(c->hip, ticket[finished], CTT_HIP_OUT_AFF, dummy);
      return GPU_UNAVAILABLE;
    }
    ms[5] = ms_since(t0);
  }
  // 6. the outputs: the first half of the cells is the blob itself, the second the coset evaluations as big-endian bytes
  if (cells) {
    memcpy(cells, blob, (size_t)N_BLOB * 32);
    uint8_t* second = cells + (size_t)N_BLOB * 32;
    for (int i = 0; i < N_BLOB; i++)
      for (int b = 0; b < 32; b++) second[32 * i + b] = coset[32 * i + 31 - b];
  }
  if (proofs)
    for (int k = 0; k < N_CELLS; k++) g1_compress(proofs + 48 * k, aff.data() + (size_t)k * 96);
  if (q_le) memcpy(q_le, q_host.data(), q_host.size());
  ms[6] = ms_since(t0);
  memcpy(c->cell_ms, ms, sizeof ms);
  memcpy(c->cell_path, path, sizeof path);
  return KZG_Success;
}

// ---- EIP-2537 BLS12_G1MSM / BLS12_G2MSM (ethereum_evm_precompiles.h:386,419) -------------------------------------------
// The reference handles the pairs in order, each point fully (coordinates, curve, subgroup) before the next one
// (fromRawCoords, ethereum_evm_precompiles.nim:316-389): the status is that of the FIRST offending pair.  parse[i] is the
// host-side verdict on pair i; the subgroup checks of all points (or of those in front of the first offender) are one call of
// ctt_hip_subgroup_check.
// When every pair parsed, the MSM is issued at once and the subgroup checks run beside it on host threads (up to 256 points; above
// that the check is a launch, and it goes first): the checks of a call of 16-256 pairs take as long as its MSM (profiles/evm_timing_r04.txt),
// and a call that fails them only discards a result.  r_aff is written in every case, the caller looks at it on EVM_Success only.
int evm_validate_and_msm(int curve, void* r_aff, const void* coefs, const uint8_t* pts, const std::vector<int>& parse) {
  const size_t n = parse.size();
  size_t bad = n;
  for (size_t i = 0; i < n; i++)
    if (parse[i] != EVM_Success) {
      bad = i;
      break;
    }
  std::vector<uint8_t> ok(bad ? bad : 1);
  if (bad < n) {   // the call fails anyway: which status -- a point in front of the first malformed pair outside the subgroup?
    if (bad > 0 && ctt_hip_subgroup_check(nullptr, curve, ok.data(), pts, bad, 0) != 0) return GPU_UNAVAILABLE;
    for (size_t i = 0; i < bad; i++)
      if (!ok[i]) return EVM_PointNotInSubgroup;
    return parse[bad];
  }
  int check_rc = 0;
  bool beside = n <= 256;   // (the host side of ctt_hip_subgroup_check; above it the check is a launch on the context the MSM uses:
                                  //  measured slower side by side than one after the other, 512 G2 pairs 9.0 against 4.8 ms)
  std::thread check;
  if (beside) {
    try {
      check = std::thread([&]() { check_rc = ctt_hip_subgroup_check(nullptr, curve, ok.data(), pts, n, 0); });
    } catch (const std::system_error&) {
      beside = false;   // (no thread to be had: one after the other)
    }
  }
  if (!beside) {
    check_rc = ctt_hip_subgroup_check(nullptr, curve, ok.data(), pts, n, 0);
    if (check_rc != 0) return GPU_UNAVAILABLE;
    for (size_t i = 0; i < n; i++)
      if (!ok[i]) return EVM_PointNotInSubgroup;
  }
  // The MSM.  A refusal because all in-flight slots of the context are held by another thread's device-resident tickets (ERR_BUSY)
  // passes: wait for it (up to ~2 s) instead of failing a consensus call; anything else (bad arguments, no device, out of device
  // memory, a HIP failure) comes back as GPU_UNAVAILABLE at once with the thread's last error set -- rounds 1-4 aborted the process here.
  int rc = ctt_hip_msm_host(curve, CTT_HIP_COEF_BIG, CTT_HIP_OUT_AFF, r_aff, coefs, pts, n);
  for (int spin = 0; rc == -1 && ctt_hip_last_error() == ERR_BUSY && spin < 20000; spin++) {
    std::this_thread::sleep_for(std::chrono::microseconds(100));
    rc = ctt_hip_msm_host(curve, CTT_HIP_COEF_BIG, CTT_HIP_OUT_AFF, r_aff, coefs, pts, n);
  }
  if (beside) check.join();
  if (rc != 0 || check_rc != 0) return GPU_UNAVAILABLE;
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return EVM_PointNotInSubgroup;
  return EVM_Success;
}

// a precompile call over the coordinate field F (EvmMsm<F>, protocols_host.h); the input's length is checked before the output's
template <class F>
uint8_t evm_msm(int curve, uint8_t* r, size_t r_len, const uint8_t* inputs, size_t inputs_len) {
  const size_t n = EvmMsm<F>::pairs(inputs_len);
  if (!n) return EVM_InvalidInputSize;
  if (r_len != EvmMsm<F>::OUT) return EVM_InvalidOutputSize;
  std::vector<uint8_t> pts, coefs;
  std::vector<int> parse;
  EvmMsm<F>::parse(inputs, n, pts, coefs, parse);
  uint8_t aff[EvmMsm<F>::AFF];
  const int st = evm_validate_and_msm(curve, aff, coefs.data(), pts.data(), parse);
  if (st != EVM_Success) return (uint8_t)st;
  EvmMsm<F>::encode(r, aff);
  return EVM_Success;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)

// ---- host-only helpers (no GPU): what tests/ check against the spec restatement, and what a binding may reuse -------------
void ctt_hip_sha256(uint8_t out[32], const uint8_t* data, size_t len) {
  Sha256 t;
  t.update(data, len);
  t.finish(out);
}
// -> ctt_eth_kzg_status; aff = affine Montgomery {x, y} (C-API layout), (0,0) for the neutral; no subgroup check
int ctt_hip_bls12_381_g1_decompress(uint8_t aff[96], const uint8_t in[48]) { return g1_decompress(aff, in); }
void ctt_hip_bls12_381_g1_compress(uint8_t out[48], const uint8_t aff[96]) { g1_compress(out, aff); }
// blob (131072 bytes) -> 4096 canonical little-endian scalars; -> ctt_eth_kzg_status
int ctt_hip_eth_kzg_blob_to_scalars(uint8_t* scalars_le, const uint8_t* blob) { return blob_to_scalars(scalars_le, blob); }
// Fiat-Shamir challenge of compute_blob_kzg_proof, 32 big-endian bytes
void ctt_hip_eth_kzg_challenge(uint8_t z_be[32], const uint8_t* blob, const uint8_t commitment[48]) {
  uint64_t z[4];
  fiat_shamir_challenge(z, blob, commitment);
  limbs_to_be<FrH>(z, z_be);
}
// quotient polynomial on the host, both branches: poly / q = 4096 canonical little-endian scalars, z / y = 32 little-endian bytes
void ctt_hip_eth_kzg_quotient_host(uint8_t* q_le, uint8_t y_le[32], const uint8_t* poly_le, const uint8_t z_le[32]) {
  static const std::vector<FrH> dom = domain_brp();
  uint64_t z[4], y[4];
  memcpy(z, z_le, 32);
  quotient_host(dom, poly_le, z, q_le, y);
  memcpy(y_le, y, 32);
}

// ---- context (ethereum_eip4844_kzg.h:200-238) -------------------------------------------------------------------------
// From memory: the 4096 x 48 bytes of the Lagrange-form G1 SRS in ceremony order (what the file's first 4096 lines hold).
// device: the GPU the SRS is cached on; table != 0 caches it as a window table (ctt_hip_msm_bases_create_table).
// -> ctt_eth_trusted_setup_status
int ctt_hip_eth_kzg_context_from_srs(ctt_eth_kzg_context_struct** ctx, const uint8_t* g1_lagrange_compressed, size_t n_points,
                                     int device, int table) {
  if (!ctx || !g1_lagrange_compressed || n_points != (size_t)N_BLOB) return TS_InvalidFile;
  return gpu_guarded([&]() { return kzg_context_build(ctx, g1_lagrange_compressed, device, table); });
}
// From the ceremony's c-kzg text file: format must be cttEthTSFormat_ckzg4844 (0); the reader and its rules are srs_read_ckzg4844
// (protocols_host.h).  Its Lagrange points, the key of commitments and cell proofs, are decompressed and subgroup-checked by the build.
uint8_t ctt_eth_kzg_context_new(ctt_eth_kzg_context_struct** ctx, const char* filepath, uint8_t format) {
  if (!ctx || !filepath || format != 0) return TS_InvalidFile;
  std::vector<uint8_t> srs((size_t)N_BLOB * 48);
  const int st = srs_read_ckzg4844(filepath, srs.data());
  if (st != TS_Success) return (uint8_t)st;
  const char* dv = getenv("CTT_HIP_DEVICE");
  // the SRS as a window table: 10 MB for 4096 points, commitments 0.38 instead of 0.52 ms (profiles/kzg_timing_r04.txt)
  return gpu_guarded([&]() { return kzg_context_build(ctx, srs.data(), dv ? atoi(dv) : 0, 1); });
}
// ethereum_eip4844_kzg.h:232: the reference's constructor with PrecomputedMSM lookup tables (t base groups, b bits per window -- CPU
// tables for the FK20 proofs of PeerDAS).  The same context as above whatever t and b say: the cell proofs here are not FK20 but 128
// plain MSMs over the Lagrange points in one pass of the batched fixed-base MSM (fixed.h), whose precomputed table -- this library's
// counterpart of those lookup tables, sized by $CTT_HIP_CELL_PROOFS_C -- is built at the first proof call.
uint8_t ctt_eth_kzg_context_new_with_precompute(ctt_eth_kzg_context_struct** ctx, const char* filepath, uint8_t format, int /*t*/, int /*b*/) {
  return ctt_eth_kzg_context_new(ctx, filepath, format);
}
void ctt_eth_kzg_context_delete(ctt_eth_kzg_context_struct* c) {
  if (!c) return;
  (void)gpu_guarded([&]() {
    std::lock_guard<std::mutex> lock(c->mu);
    DeviceScope device_scope(c->device);
    ctt_hip_msm_sync(c->hip);
    kzg_context_release(c, c->own_hip);
    return 0;
  });
  delete c;
}

// ---- EIP-4844 (ethereum_eip4844_kzg.h:106,126,153) -----------------------------------------------------------------------
uint8_t ctt_eth_kzg_blob_to_kzg_commitment(const ctt_eth_kzg_context_struct* ctx, uint8_t dst[48], const uint8_t* blob) {
  ctt_eth_kzg_context_struct* c = const_cast<ctt_eth_kzg_context_struct*>(ctx);
  std::vector<uint8_t> poly((size_t)N_BLOB * 32);
  const int st = blob_to_scalars(poly.data(), blob);
  if (st != KZG_Success) return (uint8_t)st;
  uint8_t r_aff[96];
  {
    std::lock_guard<std::mutex> lock(c->mu);
    const int rc = ctt_hip_msm_with_bases(c->hip, c->bases, CTT_HIP_COEF_BIG, CTT_HIP_OUT_AFF, r_aff, poly.data(), N_BLOB, 0);
    if (rc != 0) return GPU_UNAVAILABLE;     // the GPU refused (ctt_hip_last_error says why); dst untouched
  }
  g1_compress(dst, r_aff);
  return KZG_Success;
}

uint8_t ctt_eth_kzg_compute_kzg_proof(const ctt_eth_kzg_context_struct* ctx, uint8_t proof[48], uint8_t y_be[32], const uint8_t* blob,
                                      const uint8_t z_be[32]) {
  ctt_eth_kzg_context_struct* c = const_cast<ctt_eth_kzg_context_struct*>(ctx);
  uint64_t z[4], y[4];
  if (const int zst = bytes_to_bls_field(z, z_be); zst != KZG_Success) return (uint8_t)zst;   // (comes first)
  std::vector<uint8_t> poly((size_t)N_BLOB * 32);
  const int st = blob_to_scalars(poly.data(), blob);
  if (st != KZG_Success) return (uint8_t)st;
  const uint8_t pst = gpu_guarded([&]() { return kzg_prove(c, proof, y, poly.data(), z); });
  if (pst != KZG_Success) return pst;
  limbs_to_be<FrH>(y, y_be);
  return KZG_Success;
}

uint8_t ctt_eth_kzg_compute_blob_kzg_proof(const ctt_eth_kzg_context_struct* ctx, uint8_t proof[48], const uint8_t* blob,
                                           const uint8_t commitment[48]) {
  ctt_eth_kzg_context_struct* c = const_cast<ctt_eth_kzg_context_struct*>(ctx);
  // bytes_to_kzg_commitment: a validated point (encoding, range, on the curve, in the subgroup; the neutral is allowed)
  uint8_t aff[96];
  int st = g1_decompress(aff, commitment);
  if (st != KZG_Success) return (uint8_t)st;
  {
    std::lock_guard<std::mutex> lock(c->mu);
    uint8_t ok = 0;
    if (ctt_hip_subgroup_check(c->hip, CTT_HIP_BLS12_381_G1, &ok, aff, 1, 0) != 0) return GPU_UNAVAILABLE;
    if (!ok) return KZG_EccPointNotInSubgroup;
  }
  std::vector<uint8_t> poly((size_t)N_BLOB * 32);
  st = blob_to_scalars(poly.data(), blob);
  if (st != KZG_Success) return (uint8_t)st;
  uint64_t z[4], y[4];
  fiat_shamir_challenge(z, blob, commitment);
  return gpu_guarded([&]() { return kzg_prove(c, proof, y, poly.data(), z); });
}

// ---- EIP-7594 (ethereum_eip7594_peerdas.h: compute_cells_and_kzg_proofs; the cells alone are the Nim API's compute_cells) --------
// cells: 128 x ctt_eth_kzg_cell {byte raw[2048]}; proofs: 128 x 48 bytes.  Nothing is written on any status but Success.
static uint8_t cells_entry(const ctt_eth_kzg_context_struct* ctx, uint8_t* cells, uint8_t* proofs, uint8_t* q_le, const uint8_t* blob) {
  ctt_eth_kzg_context_struct* c = const_cast<ctt_eth_kzg_context_struct*>(ctx);
  std::vector<uint8_t> poly((size_t)N_BLOB * 32);
  const auto t0 = std::chrono::steady_clock::now();
  const int st = blob_to_scalars(poly.data(), blob);
  if (st != KZG_Success) return (uint8_t)st;
  const float parse_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return gpu_guarded([&]() { return kzg_cells(c, cells, proofs, q_le, blob, poly.data(), parse_ms); });
}
uint8_t ctt_eth_kzg_compute_cells_and_kzg_proofs(const ctt_eth_kzg_context_struct* ctx, uint8_t* cells, uint8_t* proofs, const uint8_t* blob) {
  return cells_entry(ctx, cells, proofs, nullptr, blob);
}
uint8_t ctt_hip_eth_kzg_compute_cells(const ctt_eth_kzg_context_struct* ctx, uint8_t* cells, const uint8_t* blob) {
  return cells_entry(ctx, cells, nullptr, nullptr, blob);
}
// test-facing: the 128 x 4096 canonical little-endian coefficients q_k[j] of the cell quotients (k_cell_quotients alone)
uint8_t ctt_hip_eth_kzg_cell_quotients(const ctt_eth_kzg_context_struct* ctx, uint8_t* q_le, const uint8_t* blob) {
  return cells_entry(ctx, nullptr, nullptr, q_le, blob);
}
// host-clock times (ms) of the context's last cells call, every step waited for: parse + upload, INTT, coset NTT, quotients,
// batched NTT, the MSMs, compress + copy back; with cap >= 9 also [7] the rows of the cell proofs the table kernel served in that call
// (128, or 0: the loop) and [8] the ms that call paid for building the table.  Returns the number written.
int ctt_hip_eth_kzg_last_cell_timings(const ctt_eth_kzg_context_struct* ctx, float* ms, int cap) {
  if (!ctx || !ms) return -1;
  ctt_eth_kzg_context_struct* c = const_cast<ctt_eth_kzg_context_struct*>(ctx);
  std::lock_guard<std::mutex> lock(c->mu);
  const int n = cap < 7 ? cap : 7;
  for (int i = 0; i < n; i++) ms[i] = c->cell_ms[i];
  if (cap < 9) return n;
  ms[7] = c->cell_path[0];
  ms[8] = c->cell_path[1];
  return 9;
}

// the _parallel forms (ethereum_eip4844_kzg_parallel.h:40,61,73): the thread pool is not used, as in the MSM's _parallel symbols
uint8_t ctt_eth_kzg_blob_to_kzg_commitment_parallel(const void* /*tp*/, const ctt_eth_kzg_context_struct* ctx, uint8_t dst[48],
                                                    const uint8_t* blob) {
  return ctt_eth_kzg_blob_to_kzg_commitment(ctx, dst, blob);
}
uint8_t ctt_eth_kzg_compute_kzg_proof_parallel(const void* /*tp*/, const ctt_eth_kzg_context_struct* ctx, uint8_t proof[48],
                                               uint8_t y_be[32], const uint8_t* blob, const uint8_t z_be[32]) {
  return ctt_eth_kzg_compute_kzg_proof(ctx, proof, y_be, blob, z_be);
}
uint8_t ctt_eth_kzg_compute_blob_kzg_proof_parallel(const void* /*tp*/, const ctt_eth_kzg_context_struct* ctx, uint8_t proof[48],
                                                    const uint8_t* blob, const uint8_t commitment[48]) {
  return ctt_eth_kzg_compute_blob_kzg_proof(ctx, proof, blob, commitment);
}
// ---- EIP-2537 (ethereum_evm_precompiles.h:386,419): evm_msm above ----------------------------------------------------------
uint8_t ctt_eth_evm_bls12381_g1msm(uint8_t* r, size_t r_len, const uint8_t* inputs, size_t inputs_len) {
  return evm_msm<FpH>(CTT_HIP_BLS12_381_G1, r, r_len, inputs, inputs_len);
}
uint8_t ctt_eth_evm_bls12381_g2msm(uint8_t* r, size_t r_len, const uint8_t* inputs, size_t inputs_len) {
  return evm_msm<Fp2H>(CTT_HIP_BLS12_381_G2, r, r_len, inputs, inputs_len);
}

#pragma GCC visibility pop
}  // extern "C"
