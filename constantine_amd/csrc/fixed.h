// fixed.h -- the batched fixed-base MSM over BLS12-381 G1 and BN254 G1 (kernels: fixed.hip, bodies: fixed_bodies.h, DESIGN.md section
// 14): a table of window multiples of n <= 65536 fixed points, and m MSMs over it in one pass.  FixedTable is the one host path; it
// has two users, the C symbols of include/ctt_msm_hip_fixed.h (a stream of the handle's own) and the PeerDAS prover of protocols.hip
// (the engine's main stream, under the context's mutex).  It depends on the HIP runtime only: nothing of the engine, no exceptions,
// and nothing here terminates the process.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ctt {

enum { FX_OK = 0, FX_REFUSED = -1, FX_OUT_OF_MEMORY = -2, FX_HIP_ERROR = -3 };
enum { FX_COEFS_ON_DEVICE = 1, FX_OUT_ON_DEVICE = 2 };                      // msm_batch's where-flags
enum { FX_CURVE_BLS12_381_G1 = 0, FX_CURVE_BN254_G1 = 2 };                  // the curve ids of include/ctt_msm_hip.h
enum { FX_COEF_BIG = 0, FX_COEF_FR = 1 };                                   // CTT_HIP_COEF_BIG / _FR

static constexpr int FX_DEFAULT_WINDOW_BITS = 8;   // the fastest of 4, 5, 6, 8 measured at 128 rows of 4096; the table is 1.5 GiB there

class FixedTable {
 public:
  FixedTable(int device, hipStream_t stream) : device_(device), stream_(stream) {}
  ~FixedTable();
  FixedTable(const FixedTable&) = delete;
  FixedTable& operator=(const FixedTable&) = delete;

  // The table of `n` affine points (C-API layout, host or device memory), windows of at most `c` bits (0: the default).  Every argument
  // is checked before the first launch.  -> FX_OK, or a refusal code with error() set and no table.
  int build(int curve, const void* points_aff, size_t n, int c);
  // out_aff[k] = sum_i coefs[k][i] * P_i for k < m: coefs [m][n][32] (FX_COEF_BIG: canonical little-endian below 2^BITS, FX_COEF_FR:
  // Montgomery residues of the scalar field), out_aff [m] affine points.  flags say which of the two are device pointers.  m * n * 32 below 2^31
  // and m * ceil(n / 256) * 256 below 2^32 (one launch), checked before anything is reserved or launched.  out_aff is written only
  // on FX_OK.
  int msm_batch(int coef_kind, const void* coefs, size_t m, void* out_aff, int flags);

  bool built() const { return tab_ != nullptr; }
  int device() const { return device_; }
  size_t n() const { return n_; }
  int c() const { return c_; }
  uint32_t windows() const { return W_; }
  uint32_t rows() const { return rows_; }
  size_t table_bytes() const { return table_bytes_; }
  size_t point_bytes() const { return 8 * (size_t)fwords_; }
  float build_ms() const { return build_ms_; }
  float last_kernel_ms() const { return last_ms_[0]; }   // of the last msm_batch: the sum kernel, the finish
  float last_finish_ms() const { return last_ms_[1]; }
  const char* error() const { return err_; }

 private:
  int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
  int reserve(void** p, size_t* have, size_t want);
  void release();

  int device_;
  hipStream_t stream_;
  int curve_ = -1, c_ = 0, cb_ = 0, r_ = 0;
  uint32_t W_ = 0, rows_ = 0, fwords_ = 0;
  size_t n_ = 0, table_bytes_ = 0;
  void* tab_ = nullptr;
  void *part_ = nullptr, *out_ = nullptr, *coefs_ = nullptr;   // the workspace: partials, affine rows, uploaded coefficients
  size_t part_bytes_ = 0, out_bytes_ = 0, coefs_bytes_ = 0;
  hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};
  float build_ms_ = 0, last_ms_[2] = {0, 0};
  char err_[240] = {0};
};

}  // namespace ctt
