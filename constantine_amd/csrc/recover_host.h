// recover_host.h -- EIP-7594 recover_cells_and_kzg_proofs: what decides about the untrusted input, the per-cell constants of the
// vanishing polynomial, and the bodies of the three element-wise kernels.  Plain C++17 without the GPU runtime,
// like protocols_host.h: recover.hip (the kernels and the C symbols of include/ctt_msm_hip_peerdas.h) and the stand-alone
// tests/recover_harness.cpp (tests/test_peerdas_recover_cpu.py; sanitizers by hand, README) include the same definitions.
//
// The extended blob is 8192 evaluations in bit-reversed order: position p = 64 k + j of cell k holds the value at omega_8192^brp13(p),
// and brp13(64 k + j) = 128 brp6(j) + brp7(k), so X^64 = omega_128^brp7(k) = c_k on the whole of cell k (cell_coset_constants).  The
// vanishing polynomial of the missing cells, Z(X) = prod_{m missing} (X^64 - c_m), is therefore one constant per cell on the domain,
//   zc[k]   = Z_s(c_k),        Z_s(Y) = prod_{m missing} (Y - c_m)     (0 exactly on the missing cells)
// and one constant per cell on the coset 5 * <omega_8192> in the same layout, where X^64 = 5^64 c_k:
//   izc5[k] = 1 / Z_s(5^64 c_k)                                        (5^64 c_k is no 128th root of unity: never a division by 0)
// With E the received evaluations (0 where missing): (E Z) = (P Z) on the domain, so  P = INTT_coset( NTT_coset( INTT(E Z) ) * izc5 ).
#pragma once
#include "protocols_host.h"

namespace ctt::proto {

constexpr int N_EXT = 2 * N_BLOB;             // 8192
constexpr size_t RC_MAX_BLOBS = 4096;         // B * 128 * 2048 cell bytes < 2^31 and B * 8192 <= 2^26, the transform's cap
constexpr uint64_t RC_COSET_SHIFT = 5;        // the reference's and the consensus spec's coset of the division
constexpr int KZG_CellIndicesNotAscending = 9;

// ---- validation, in the reference's order (eth_eip7594_peerdas.nim:639-664): NULL pointers and the count, every index < 128, strictly
// ascending, then every element of every cell in input order < r.  cells: B * n cells of 2048 bytes.
inline int recover_validate_indices(const uint64_t* idx, size_t n) {
  if (!idx || n < (size_t)N_CELLS / 2 || n > (size_t)N_CELLS) return KZG_InputsLengthsMismatch;
  for (size_t i = 0; i < n; i++)
    if (idx[i] >= (uint64_t)N_CELLS) return KZG_InputsLengthsMismatch;
  for (size_t i = 1; i < n; i++)
    if (idx[i - 1] >= idx[i]) return KZG_CellIndicesNotAscending;
  return KZG_Success;
}
inline int recover_validate(const uint64_t* idx, const uint8_t* cells, size_t n, size_t B) {
  if (!cells) return KZG_InputsLengthsMismatch;
  const int st = recover_validate_indices(idx, n);
  if (st != KZG_Success) return st;
  const size_t elems = B * n * (size_t)CELL_ELEMS;
  for (size_t e = 0; e < elems; e++) {
    uint64_t v[4];
    if (bytes_to_bls_field(v, cells + 32 * e) != KZG_Success) return KZG_ScalarLargerThanCurveOrder;
  }
  return KZG_Success;
}

// ---- the constants of a validated index set, Montgomery: zc[128] and izc5[128] as above; slot[k] = the position of cell k among the
// supplied cells, -1 for a missing one.  128 * 64 multiplications for each table and one batch_inverse.
inline void recovery_constants(const uint64_t* idx, size_t n, FrH* zc, FrH* izc5, int32_t* slot) {
  for (int k = 0; k < N_CELLS; k++) slot[k] = -1;
  for (size_t i = 0; i < n; i++) slot[idx[i]] = (int32_t)i;
  const std::vector<FrH> ck = cell_coset_constants(root_of_unity(13));
  const uint64_t five[4] = {RC_COSET_SHIFT, 0, 0, 0}, e64[1] = {(uint64_t)CELL_ELEMS};
  const FrH s = fpow<FrH>(to_mont<FrH>(five), e64, 1);   // 5^64
  std::vector<FrH> z5(N_CELLS), inv;
  for (int k = 0; k < N_CELLS; k++) {
    const FrH y5 = FrH::mul(s, ck[k]);
    FrH a = FrH::one(), b = FrH::one();
    for (int m = 0; m < N_CELLS; m++) {
      if (slot[m] >= 0) continue;
      a = FrH::mul(a, FrH::sub(ck[k], ck[m]));
      b = FrH::mul(b, FrH::sub(y5, ck[m]));
    }
    zc[k] = a;
    z5[k] = b;
  }
  batch_inverse(z5, inv);
  for (int k = 0; k < N_CELLS; k++) izc5[k] = inv[k];
}

// ---- the kernel bodies: one lane per element of B rows of 8192.  Every index is stated for B rows: the largest B gives
// 4096 * 8192 = 2^25 lanes and 2^25 * 8 = 2^28 words per buffer, which fits 32 bits; the bytes of the cells (up to 2^31 - 2^20 of them
// counted from 0) are addressed in 64 bits.
struct RcLoadArgs {
  const uint8_t* cells;   // [B][n][64] elements of 32 big-endian bytes, validated (< r)
  const uint32_t* zcr2;   // [128] zc[k] * R^2 as Montgomery words: one multiplication converts the element and applies Z
  const int32_t* slot;    // [128]
  uint32_t* rows;         // [B][8192] Montgomery: the bit-reversed extended evaluations times Z, zero on the missing cells
  uint32_t n, B;
};
CTT_HD void rc_load_body(const RcLoadArgs& a, uint32_t lane) {
  if (lane >= a.B * (uint32_t)N_EXT) return;
  const uint32_t b = lane / (uint32_t)N_EXT, p = lane % (uint32_t)N_EXT, k = p / CELL_ELEMS, j = p % CELL_ELEMS;
  const int32_t i = a.slot[k];
  FrD v = FrD::zero();
  if (i >= 0) {
    const uint8_t* src = a.cells + (((uint64_t)b * a.n + (uint32_t)i) * CELL_ELEMS + j) * 32u;
    FrD c;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4* q = (const uint4*)src;   // (the buffer is 32-byte aligned, and so is every element)
    const uint4 hi = q[0], lo = q[1];
    c.l[7] = __builtin_bswap32(hi.x); c.l[6] = __builtin_bswap32(hi.y); c.l[5] = __builtin_bswap32(hi.z); c.l[4] = __builtin_bswap32(hi.w);
    c.l[3] = __builtin_bswap32(lo.x); c.l[2] = __builtin_bswap32(lo.y); c.l[1] = __builtin_bswap32(lo.z); c.l[0] = __builtin_bswap32(lo.w);
#else
    for (int w = 0; w < 8; w++) {
      const uint8_t* q = src + 28 - 4 * w;
      c.l[w] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
#endif
    v = FrD::mul(c, ntt_ld<FrD>(a.zcr2, k));
  }
  ntt_st<FrD>(a.rows, lane, v);
}

struct RcScaleArgs {
  uint32_t* rows;         // [B][8192] Montgomery, in place
  const uint32_t* izc5;   // [128] Montgomery
  uint32_t B;
};
CTT_HD void rc_scale_body(const RcScaleArgs& a, uint32_t lane) {
  if (lane >= a.B * (uint32_t)N_EXT) return;
  const uint32_t k = (lane % (uint32_t)N_EXT) / CELL_ELEMS;
  ntt_st<FrD>(a.rows, lane, FrD::mul(ntt_ld<FrD>(a.rows, lane), ntt_ld<FrD>(a.izc5, k)));
}

// The 8192 recovered coefficients of a row: the low half is the blob's polynomial, compacted into coef (Montgomery); a lane of the high
// half that holds anything but zero stores 1 into high[b] -- every such lane stores the same value, so no atomic is needed; the caller
// zeroes high[] first.  canon (test-facing): all 8192 coefficients in canonical form, in place, instead of the compaction.
struct RcSplitArgs {
  uint32_t* rows;         // [B][8192] Montgomery
  uint32_t* coef;         // [B][4096]
  uint32_t* high;         // [B]
  uint32_t B, canon;
};
CTT_HD void rc_split_body(const RcSplitArgs& a, uint32_t lane) {
  if (lane >= a.B * (uint32_t)N_EXT) return;
  const uint32_t b = lane / (uint32_t)N_EXT, p = lane % (uint32_t)N_EXT;
  const FrD v = ntt_ld<FrD>(a.rows, lane);
  if (p >= (uint32_t)N_BLOB) {
    if (!v.is_zero()) a.high[b] = 1u;
  } else if (!a.canon) {
    ntt_st<FrD>(a.coef, b * (uint32_t)N_BLOB + p, v);
  }
  if (a.canon) ntt_st<FrD>(a.rows, lane, FrD::from_mont(v));
}

}  // namespace ctt::proto
