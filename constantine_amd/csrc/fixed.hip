// fixed.hip -- kernels and host path of the batched fixed-base G1 MSM (bodies: fixed_bodies.h, class: fixed.h).
#include "fixed.h"

#include <stdarg.h>
#include <stdio.h>

#include <chrono>

#include "fixed_bodies.h"

namespace ctt {

static constexpr int FX_TABLE_BLOCK = 64;
static constexpr uint32_t FX_FINISH_BLOCK = FX_WAVE * FX_FINISH_ROWS;

template <class C>
__global__ void __launch_bounds__(FX_TABLE_BLOCK) k_fx_table(FxTableArgs a) {
  fx_table_body<typename C::F>(a, blockIdx.x * blockDim.x + threadIdx.x);
}

// The pairwise sum of a group of lanes through its SLOTS slots of LDS, from level `first` down to 1: afterwards lane 0 holds the sum
// of the lanes below 2 * first.  Every lane of the workgroup runs the same levels, so the barriers are uniform.
template <class F, uint32_t SLOTS>
__device__ __forceinline__ void fx_tree(uint32_t* slots, uint32_t lane, uint32_t first, XYZZ<F>& acc) {
#pragma unroll 1
  for (uint32_t s = first; s >= 1; s >>= 1) {
    vk_tree_put<F, SLOTS>(slots, lane, s, acc);
    __syncthreads();
    fx_tree_take<F, SLOTS>(slots, lane, s, acc);
    __syncthreads();
  }
}

// Workgroup (row k, chunk s) = block k * chunks + s; lane l owns base 256 s + l: W gathers and mixed additions in registers, then the
// tree (eight levels, 128 slots).  A lane without a base or without a non-zero digit holds the in-memory neutral.
template <class C>
__global__ void __launch_bounds__(FX_BLOCK) k_fx_msm(FxMsmArgs a) {
  using F = typename C::F;
  __shared__ uint32_t slots[4 * F::N * FX_TREE_SLOTS];
  const uint32_t k = blockIdx.x / a.chunks, s = blockIdx.x % a.chunks, lane = threadIdx.x;
  XYZZ<F> acc = fx_lane_sum<F, typename C::Fr>(a, k, s * FX_BLOCK + lane);
  fx_tree<F, FX_TREE_SLOTS>(slots, lane, FX_TREE_SLOTS, acc);
  if (lane == 0) fx_store_xyzz<F>(a.part + (uint64_t)blockIdx.x * (4 * F::N), acc);
}

// One wavefront per row, four rows per workgroup: the partials of the row, six levels of the tree through the wave's own 32 slots,
// then lane 0 of the workgroup makes its rows affine with one inversion.  A wave without a row loads nothing and holds neutrals.
template <class C>
__global__ void __launch_bounds__(FX_FINISH_BLOCK) k_fx_finish(FxFinishArgs a) {
  using F = typename C::F;
  __shared__ uint32_t slots[FX_FINISH_ROWS * 4 * F::N * FX_FINISH_SLOTS];
  __shared__ uint32_t grp[FX_FINISH_ROWS * 4 * F::N];
  __shared__ uint32_t pre[FX_FINISH_ROWS * F::N];
  const uint32_t wave = threadIdx.x / FX_WAVE, lane = threadIdx.x % FX_WAVE;
  const uint32_t k0 = blockIdx.x * FX_FINISH_ROWS;
  XYZZ<F> acc = fx_finish_lane_sum<F>(a, k0 + wave, lane);
  fx_tree<F, FX_FINISH_SLOTS>(slots + wave * (4 * F::N * FX_FINISH_SLOTS), lane, FX_FINISH_SLOTS, acc);
  if (lane == 0) fx_store_xyzz<F>(grp + wave * (4 * F::N), acc);
  __syncthreads();
  if (threadIdx.x == 0) fx_finish_group<F>(a, k0, a.m - k0 < FX_FINISH_ROWS ? a.m - k0 : FX_FINISH_ROWS, grp, pre);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
namespace {

// the calling thread's HIP device is the caller's business: selected for the duration of a call, then put back
struct FxDeviceScope {
  int prev = -1;
  bool ok;
  explicit FxDeviceScope(int dev) {
    ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess);
    if (!ok) (void)hipGetLastError();
  }
  ~FxDeviceScope() {
    int now = -1;
    if (ok && prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
  }
};

template <class C>
void launch_table(hipStream_t s, const FxTableArgs& a) {
  const uint32_t lanes = a.n * a.W;
  hipLaunchKernelGGL((k_fx_table<C>), dim3((lanes + FX_TABLE_BLOCK - 1) / FX_TABLE_BLOCK), dim3(FX_TABLE_BLOCK), 0, s, a);
}
template <class C>
void launch_msm(hipStream_t s, const FxMsmArgs& a) {
  hipLaunchKernelGGL((k_fx_msm<C>), dim3(a.m * a.chunks), dim3(FX_BLOCK), 0, s, a);
}
template <class C>
void launch_finish(hipStream_t s, const FxFinishArgs& a) {
  hipLaunchKernelGGL((k_fx_finish<C>), dim3((a.m + FX_FINISH_ROWS - 1) / FX_FINISH_ROWS), dim3(FX_FINISH_BLOCK), 0, s, a);
}

}  // namespace

#define FX_HIP(expr)                                                                   \
  do {                                                                                 \
    const hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) {                                                            \
      (void)hipGetLastError();                                                         \
      return fail(FX_HIP_ERROR, "%s: %s", #expr, hipGetErrorString(e_));               \
    }                                                                                  \
  } while (0)

int FixedTable::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_, sizeof err_, fmt, ap);
  va_end(ap);
  return code;
}

// a workspace buffer of at least `want` bytes (it only grows)
int FixedTable::reserve(void** p, size_t* have, size_t want) {
  if (*have >= want) return FX_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  const hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? FX_OUT_OF_MEMORY : FX_HIP_ERROR, "workspace of %zu bytes: %s", want, hipGetErrorString(e));
  }
  *have = want;
  return FX_OK;
}

void FixedTable::release() {
  for (void** p : {&tab_, &part_, &out_, &coefs_}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  part_bytes_ = out_bytes_ = coefs_bytes_ = 0;
  for (hipEvent_t& e : ev_) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

FixedTable::~FixedTable() {
  FxDeviceScope scope(device_);
  if (scope.ok) {
    (void)hipStreamSynchronize(stream_);
    release();
  }
}

int FixedTable::build(int curve, const void* points_aff, size_t n, int c) {
  if (tab_) return fail(FX_REFUSED, "the table is already built");
  if (curve != FX_CURVE_BLS12_381_G1 && curve != FX_CURVE_BN254_G1) return fail(FX_REFUSED, "curve %d: BLS12-381 G1 (0) or BN254 G1 (2) only", curve);
  if (!points_aff || n < 1 || n > FX_MAX_BASES) return fail(FX_REFUSED, "n = %zu: 1 .. %u points", n, FX_MAX_BASES);
  if (c == 0) c = FX_DEFAULT_WINDOW_BITS;
  if (c < FX_MIN_WINDOW_BITS || c > FX_MAX_WINDOW_BITS) return fail(FX_REFUSED, "c = %d: %d .. %d bits", c, FX_MIN_WINDOW_BITS, FX_MAX_WINDOW_BITS);
  const bool bls = curve == FX_CURVE_BLS12_381_G1;
  const uint32_t fwords = bls ? (uint32_t)Bls12381G1::F::N : (uint32_t)Bn254G1::F::N;
  int W;
  const WinLayout lay = window_layout(bls ? Bls12381G1::BITS : Bn254G1::BITS, c, &W);
  const uint32_t rows = vk_row_off(lay, (uint32_t)W);
  const uint64_t records = (uint64_t)n * rows;                 // below 2^16 * 2^18
  const uint64_t table_bytes = records * 8u * fwords;          // 64-bit: 2^16 points at c = 12 are hundreds of GB (a failed allocation)
  const uint64_t pre_bytes = records * 12u * fwords;

  FxDeviceScope scope(device_);
  if (!scope.ok) return fail(FX_HIP_ERROR, "device %d cannot be selected", device_);
  const auto t0 = std::chrono::steady_clock::now();
  void *tab = nullptr, *pre = nullptr, *pts = nullptr;
  auto give_back = [&]() {
    for (void* p : {tab, pre, pts})
      if (p) (void)hipFree(p);
  };
  void** const want_ptr[3] = {&tab, &pre, &pts};
  const uint64_t want_bytes[3] = {table_bytes, pre_bytes, (uint64_t)n * 8u * fwords};
  for (int b = 0; b < 3; b++) {
    const hipError_t e = hipMalloc(want_ptr[b], (size_t)want_bytes[b]);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      *want_ptr[b] = nullptr;
      give_back();
      return fail(e == hipErrorOutOfMemory ? FX_OUT_OF_MEMORY : FX_HIP_ERROR, "table of %llu bytes (and %llu while it is built): %s",
                  (unsigned long long)table_bytes, (unsigned long long)pre_bytes, hipGetErrorString(e));
    }
  }
  FxTableArgs a;
  a.tab = (uint32_t*)tab;
  a.n = (uint32_t)n;
  a.W = (uint32_t)W;
  a.lay = lay;
  a.rows = rows;
  a.stride = 2 * fwords;
  a.pts = (const uint32_t*)pts;
  a.pre = (uint32_t*)pre;
  hipError_t e = hipMemcpyAsync(pts, points_aff, n * 8u * fwords, hipMemcpyDefault, stream_);
  if (e == hipSuccess) {
    if (bls) launch_table<Bls12381G1>(stream_, a);
    else launch_table<Bn254G1>(stream_, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream_);
  for (hipEvent_t& ev : ev_)
    if (e == hipSuccess) e = hipEventCreate(&ev);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    give_back();
    for (hipEvent_t& ev : ev_) {
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
    }
    return fail(FX_HIP_ERROR, "table build: %s", hipGetErrorString(e));
  }
  (void)hipFree(pre);
  (void)hipFree(pts);
  tab_ = tab;
  curve_ = curve;
  c_ = c;
  cb_ = lay.cb;
  r_ = lay.r;
  W_ = (uint32_t)W;
  rows_ = rows;
  fwords_ = fwords;
  n_ = n;
  table_bytes_ = (size_t)table_bytes;
  build_ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return FX_OK;
}

int FixedTable::msm_batch(int coef_kind, const void* coefs, size_t m, void* out_aff, int flags) {
  if (!tab_) return fail(FX_REFUSED, "no table");
  if (!coefs || !out_aff) return fail(FX_REFUSED, "null coefficients or output");
  if (coef_kind != FX_COEF_BIG && coef_kind != FX_COEF_FR) return fail(FX_REFUSED, "coefficient kind %d", coef_kind);
  if (flags & ~(FX_COEFS_ON_DEVICE | FX_OUT_ON_DEVICE)) return fail(FX_REFUSED, "flags 0x%x", flags);
  if (m < 1 || m > (1ull << 26) || (uint64_t)m * n_ * 32u >= (1ull << 31))
    return fail(FX_REFUSED, "m = %zu rows of %zu scalars: 1 row or more, and m * n * 32 below 2^31", m, n_);
  const uint32_t chunks = (uint32_t)((n_ + FX_BLOCK - 1) / FX_BLOCK);
  // A launch has fewer than 2^32 work-items in x (the runtime refuses more as an invalid configuration): m * chunks blocks of FX_BLOCK
  // lanes, and the finish's ceil(m / 4) blocks of 256.  With m * n * 32 below 2^31 only n <= 3 with m >= 2^24 is refused here.
  const uint64_t sum_items = (uint64_t)m * chunks * FX_BLOCK;
  const uint64_t finish_items = ((uint64_t)m + FX_FINISH_ROWS - 1) / FX_FINISH_ROWS * FX_FINISH_BLOCK;
  if (sum_items >= (1ull << 32) || finish_items >= (1ull << 32))
    return fail(FX_REFUSED, "m = %zu rows of %u chunks: m * chunks * %u below 2^32 (the work-items of one launch)", m, chunks, FX_BLOCK);
  FxDeviceScope scope(device_);
  if (!scope.ok) return fail(FX_HIP_ERROR, "device %d cannot be selected", device_);
  const size_t coef_bytes = m * n_ * 32u, out_bytes = m * point_bytes();
  int rc;
  if ((rc = reserve(&part_, &part_bytes_, m * chunks * 2 * point_bytes())) != FX_OK) return rc;
  if ((rc = reserve(&out_, &out_bytes_, out_bytes)) != FX_OK) return rc;
  const void* d_coefs = coefs;
  if (!(flags & FX_COEFS_ON_DEVICE)) {
    if ((rc = reserve(&coefs_, &coefs_bytes_, coef_bytes)) != FX_OK) return rc;
    FX_HIP(hipMemcpyAsync(coefs_, coefs, coef_bytes, hipMemcpyHostToDevice, stream_));
    d_coefs = coefs_;
  }
  FxMsmArgs a;
  a.tab = (uint32_t*)tab_;
  a.n = (uint32_t)n_;
  a.W = W_;
  a.lay.cb = cb_;
  a.lay.r = r_;
  a.rows = rows_;
  a.stride = 2 * fwords_;
  a.coefs = (const uint32_t*)d_coefs;
  a.m = (uint32_t)m;
  a.fr = coef_kind == FX_COEF_FR;
  a.chunks = chunks;
  a.part = (uint32_t*)part_;
  const FxFinishArgs f{(const uint32_t*)part_, (uint32_t)m, chunks, (uint32_t*)out_};
  const bool bls = curve_ == FX_CURVE_BLS12_381_G1;
  FX_HIP(hipEventRecord(ev_[0], stream_));
  if (bls) launch_msm<Bls12381G1>(stream_, a);
  else launch_msm<Bn254G1>(stream_, a);
  FX_HIP(hipGetLastError());
  FX_HIP(hipEventRecord(ev_[1], stream_));
  if (bls) launch_finish<Bls12381G1>(stream_, f);
  else launch_finish<Bn254G1>(stream_, f);
  FX_HIP(hipGetLastError());
  FX_HIP(hipEventRecord(ev_[2], stream_));
  FX_HIP(hipStreamSynchronize(stream_));
  FX_HIP(hipEventElapsedTime(&last_ms_[0], ev_[0], ev_[1]));
  FX_HIP(hipEventElapsedTime(&last_ms_[1], ev_[1], ev_[2]));
  // the caller's buffer last, when everything else has succeeded
  FX_HIP(hipMemcpyAsync(out_aff, out_, out_bytes, (flags & FX_OUT_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream_));
  FX_HIP(hipStreamSynchronize(stream_));
  return FX_OK;
}

}  // namespace ctt
