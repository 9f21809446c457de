// ntt.hip -- kernels and launch path of the batched scalar-field NTT (bodies: ntt_bodies.h, passes: ntt_plan.h, DESIGN.md
// section 13), instantiated for the five scalar fields of the library's curve ids.
#include "ntt.h"

#include <string.h>

#include "hip_errors.h"
#include "ntt_bodies.h"

namespace ctt {

#define NTT_HIP_CHECK(expr)                                                                           \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      ::ctt::hip_failed(#expr, hipGetErrorString(e_), e_ == hipErrorOutOfMemory, __FILE__, __LINE__); \
  } while (0)

static constexpr uint32_t NTT_POW_K = 16;   // table entries per lane of k_ntt_powers

// One workgroup per tile: the image stays in LDS between the tile's one global read and one global write.  Every lane runs the same
// stages, so the barriers are uniform.
template <class Fr>
__global__ void __launch_bounds__(NTT_BLOCK) k_ntt_pass(NttArgs<Fr> a) {
  extern __shared__ uint32_t ntt_img[];
  const uint32_t tile_id = blockIdx.x, lane = threadIdx.x;
  ntt_tile_load<Fr>(a, ntt_img, tile_id, lane, NTT_BLOCK);
  __syncthreads();
  const uint32_t t = a.pass.t;
#pragma unroll 1
  for (uint32_t j = 0; j < t; j++) {
    ntt_tile_stage<Fr>(a, ntt_img, tile_id, (a.flags & NTT_DIT) ? j : t - 1u - j, lane, NTT_BLOCK);
    __syncthreads();
  }
  ntt_tile_store<Fr>(a, ntt_img, tile_id, lane, NTT_BLOCK);
}

template <class Fr>
__global__ void __launch_bounds__(NTT_BLOCK) k_ntt_powers(NttPowArgs<Fr> a) {
  ntt_powers_body<Fr>(a, blockIdx.x * blockDim.x + threadIdx.x);
}

template <class Fr>
__global__ void __launch_bounds__(NTT_BLOCK) k_ntt_brp_swap(uint32_t* buf, uint32_t log2n, uint64_t total) {
  ntt_brp_swap_body<Fr>(buf, log2n, total, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

template <class Fr>
struct NttImpl {
  using PP = typename Fr::Params;
  struct Plan {
    int log2n, tile_log2;
    uint32_t* d_tw = nullptr;
    Fr ninv;                                  // 1/n, Montgomery
    // the multipliers of the last coset shift, forward ([0]: g^i) and inverse ([1]: g^-i / n): a caller's g rarely changes
    uint32_t* d_shift[2] = {nullptr, nullptr};
    Fr shift_g[2];
    bool shift_ok[2] = {false, false};
  };

  static constexpr int two_adicity() {
    int k = 0;
    for (int i = 0; i < PP::N; i++) {
      const uint32_t w = PP::P[i] - (i == 0 ? 1u : 0u);   // (every modulus here is odd and its low word is not 0)
      if (w == 0u) { k += 32; continue; }
      for (int b = 0; b < 32 && !((w >> b) & 1u); b++) k++;
      break;
    }
    return k;
  }
  // canonical little-endian bytes -> Montgomery; false when not below the modulus
  static bool load_canonical(Fr& out, const void* bytes) {
    Fr c;
    memcpy(c.l, bytes, sizeof(c.l));
    for (int i = Fr::N - 1; i >= 0; i--) {
      if (c.l[i] < PP::P[i]) { out = Fr::to_mont(c); return true; }
      if (c.l[i] > PP::P[i]) return false;
    }
    return false;
  }
  // 0, or -2 with *oom_bytes
  static int alloc(uint32_t** p, size_t bytes, size_t* oom_bytes) {
    const hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      *p = nullptr;
      *oom_bytes = bytes;
      return -2;
    }
    NTT_HIP_CHECK(e);
    return 0;
  }
  static void launch_powers(hipStream_t s, uint32_t* out, const Fr& base, const Fr& c0, uint32_t count) {
    NttPowArgs<Fr> a{out, base, c0, count, NTT_POW_K};
    const uint32_t lanes = (count + NTT_POW_K - 1) / NTT_POW_K;
    hipLaunchKernelGGL(k_ntt_powers<Fr>, dim3((lanes + NTT_BLOCK - 1) / NTT_BLOCK), dim3(NTT_BLOCK), 0, s, a);
    NTT_HIP_CHECK(hipGetLastError());
  }

  static int plan_create(hipStream_t s, int log2n, const void* omega, int tile_log2, void** plan, size_t* oom_bytes) {
    Fr w;
    if (!load_canonical(w, omega)) return -1;
    Fr h = w;
    for (int i = 1; i < log2n; i++) h = Fr::sqr(h);        // omega^(n/2)
    if (!Fr::eq(h, Fr::neg(Fr::one()))) return -1;
    Plan* p = new Plan();
    p->log2n = log2n;
    p->tile_log2 = tile_log2;
    Fr nn = Fr::zero();
    nn.l[0] = 1u << log2n;
    p->ninv = Fr::inv(Fr::to_mont(nn));
    const uint32_t half = 1u << (log2n - 1);
    const int rc = alloc(&p->d_tw, (size_t)half * sizeof(Fr), oom_bytes);
    if (rc != 0) {
      delete p;
      return rc;
    }
    launch_powers(s, p->d_tw, w, Fr::one(), half);
    *plan = p;
    return 0;
  }
  static void plan_destroy(void* plan) {
    Plan* p = (Plan*)plan;
    if (p->d_tw) (void)hipFree(p->d_tw);
    for (uint32_t* q : p->d_shift)
      if (q) (void)hipFree(q);
    delete p;
  }
  static void plan_info(const void* plan, size_t info[4]) {
    const Plan* p = (const Plan*)plan;
    NttPass passes[NTT_MAX_PASSES];
    info[0] = (size_t)p->log2n;
    info[1] = (size_t)p->tile_log2;
    info[2] = (size_t)ntt_plan_passes(p->log2n, p->tile_log2, false, passes);
    info[3] = ((size_t)1 << (p->log2n - 1)) * sizeof(Fr);
  }

  static int run(hipStream_t s, void* plan, void* d_out, const void* d_in, size_t batch, int flags, const void* shift, size_t* oom_bytes) {
    Plan* p = (Plan*)plan;
    const uint32_t L = (uint32_t)p->log2n, n = 1u << L;
    const bool inverse = flags & NTT_FLAG_INVERSE;
    const uint32_t* d_mult = nullptr;
    if (shift) {
      Fr g;
      if (!load_canonical(g, shift) || g.is_zero()) return -1;
      const int d = inverse ? 1 : 0;
      if (!p->d_shift[d]) {
        const int rc = alloc(&p->d_shift[d], (size_t)n * sizeof(Fr), oom_bytes);
        if (rc != 0) return rc;
      }
      if (!p->shift_ok[d] || !Fr::eq(p->shift_g[d], g)) {
        p->shift_ok[d] = false;
        if (inverse) launch_powers(s, p->d_shift[d], Fr::inv(g), p->ninv, n);
        else launch_powers(s, p->d_shift[d], g, Fr::one(), n);
        p->shift_g[d] = g;
        p->shift_ok[d] = true;
      }
      d_mult = p->d_shift[d];
    }
    NttCall<Fr> c;
    ntt_setup<Fr>(c, p->log2n, p->tile_log2, flags, p->ninv, p->d_tw, d_mult, d_out, d_in);
    const uint64_t total = (uint64_t)batch << L;
    for (int k = 0; k < c.npass; k++) {
      const NttArgs<Fr> a = ntt_pass_args<Fr>(c, k);
      const uint32_t tiles = (uint32_t)(total >> a.pass.E);
      hipLaunchKernelGGL(k_ntt_pass<Fr>, dim3(tiles), dim3(NTT_BLOCK), (size_t)sizeof(Fr) << a.pass.E, s, a);
      NTT_HIP_CHECK(hipGetLastError());
    }
    if (c.swap) {
      hipLaunchKernelGGL(k_ntt_brp_swap<Fr>, dim3((uint32_t)((total + NTT_BLOCK - 1) / NTT_BLOCK)), dim3(NTT_BLOCK), 0, s, (uint32_t*)d_out, L, total);
      NTT_HIP_CHECK(hipGetLastError());
    }
    return 0;
  }

  static const NttOps* ops() {
    static const NttOps o = {two_adicity(), plan_create, plan_destroy, run, plan_info};
    return &o;
  }
};

template <> const NttOps* ntt_ops_for<BLS12_381_Fr>() { return NttImpl<Fp<BLS12_381_Fr>>::ops(); }
template <> const NttOps* ntt_ops_for<BN254_Fr>() { return NttImpl<Fp<BN254_Fr>>::ops(); }
template <> const NttOps* ntt_ops_for<Vesta_Fp>() { return NttImpl<Fp<Vesta_Fp>>::ops(); }
template <> const NttOps* ntt_ops_for<Pallas_Fp>() { return NttImpl<Fp<Pallas_Fp>>::ops(); }
template <> const NttOps* ntt_ops_for<Banderwagon_Fr>() { return NttImpl<Fp<Banderwagon_Fr>>::ops(); }

}  // namespace ctt
