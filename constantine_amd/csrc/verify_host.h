// verify_host.h -- EIP-7594 verify_cell_kzg_proof_batch: what decides about the untrusted input, the challenge, the constants, and the
// bodies of the three kernels of verify.hip as functions of a lane index.  Plain C++17 without the GPU runtime,
// like recover_host.h: verify.hip (the kernels and the C symbols of include/ctt_msm_hip_peerdas_verify.h) and the stand-alone
// tests/verify_harness.cpp (tests/test_peerdas_verify_cpu.py; sanitizers by hand, README) include the same definitions.
//
// The equation (the universal verification equation of the consensus spec; weights rho_k = r^(k+1) as the reference's skipOne):
//   LL = sum_k rho_k pi_k
//   RL = sum_i w_i C_i  -  sum_{i<64} c[i] [tau^i]_1  +  sum_k rho_k h_k^64 pi_k,      w_i = sum_{k -> i} rho_k
//   e(LL, [tau^64]_2) = e(RL, G_2)
// c[] are the coefficients of sum_k rho_k I_k(X), I_k the polynomial of degree < 64 that takes cell k's values on its coset
// h_j <omega_64>, h_j = omega_8192^brp7(j) for column j (element e of the cell at h_j omega_64^brp6(e)).  I_k(h_j Y) is the inverse
// transform of the cell, and the transform is linear, so the cells of a column are summed first:
//   S[j][e] = sum_{k in column j} rho_k cell_k[e]          (k_vf_colsum)
//   a_j     = INTT_64(S[j]), bit-reversed in                 (one batched transform of 128 rows)
//   c[i]    = sum_j h_j^(-i) a_j[i]                          (k_vf_interp)
#pragma once
#include <array>
#include <map>

#include "pairing_host.h"

namespace ctt::proto {

using FpD = Fp<BLS12_381_Fp>;                     // the canonical device field of fixed_bodies.h: 12 words, Montgomery
constexpr uint32_t VF_BLOCK = 256;
constexpr size_t VF_MAX_CELLS = (size_t)1 << 20;  // 2 n points and n * 64 elements are indexed in 32 bits; the cells' bytes in 64
constexpr uint32_t VF_COLSUM_LANES = (uint32_t)(N_CELLS * CELL_ELEMS);

// ---- the checks that need no arithmetic, in the reference's order (eth_eip7594_peerdas.nim:529-544) ---------------------------
inline int verify_check_arguments(bool have_verifier, const void* commitments, const uint64_t* idx, const void* cells, const void* proofs,
                                  const void* random_bytes, size_t n) {
  if (!have_verifier) return KZG_InputsLengthsMismatch;
  if (n == 0) return KZG_Success;
  if (!commitments || !idx || !cells || !proofs || !random_bytes || n > VF_MAX_CELLS) return KZG_InputsLengthsMismatch;
  for (size_t k = 0; k < n; k++)
    if (idx[k] >= (uint64_t)N_CELLS) return KZG_InputsLengthsMismatch;
  return KZG_Success;
}

// the commitments deduplicated on their bytes, first occurrences in input order: cidx[k] = the unique commitment of cell k,
// uniq = M * 48 bytes
inline void verify_dedup(const uint8_t* commitments, size_t n, std::vector<uint32_t>& cidx, std::vector<uint8_t>& uniq) {
  std::map<std::array<uint8_t, 48>, uint32_t> seen;
  cidx.resize(n);
  uniq.clear();
  for (size_t k = 0; k < n; k++) {
    std::array<uint8_t, 48> key;
    memcpy(key.data(), commitments + 48 * k, 48);
    const auto it = seen.emplace(key, (uint32_t)seen.size());
    if (it.second) uniq.insert(uniq.end(), key.begin(), key.end());
    cidx[k] = it.first->second;
  }
}

// ---- the challenge ----------------------------------------------------------------------------------------------------------------
inline void put_be64(std::vector<uint8_t>& t, uint64_t v) {
  for (int b = 7; b >= 0; b--) t.push_back((uint8_t)(v >> (8 * b)));
}
// the transcript of compute_verify_cell_kzg_proof_batch_challenge (eth_eip7594_peerdas.nim:475-510); its SHA-256 reduced mod r is r
template <class Index>
inline void verify_transcript(std::vector<uint8_t>& t, const uint8_t* uniq, size_t M, const Index* cidx, const uint64_t* idx,
                              const uint8_t* cells, const uint8_t* proofs, size_t n) {
  t.clear();
  t.reserve(48 + 48 * M + n * (16 + 2048 + 48));
  const char* domain = "RCKZGCBATCH__V1_";
  t.insert(t.end(), domain, domain + 16);
  put_be64(t, (uint64_t)N_BLOB);
  put_be64(t, (uint64_t)CELL_ELEMS);
  put_be64(t, (uint64_t)M);
  put_be64(t, (uint64_t)n);
  t.insert(t.end(), uniq, uniq + 48 * M);
  for (size_t k = 0; k < n; k++) {
    put_be64(t, (uint64_t)cidx[k]);
    put_be64(t, idx[k]);
    t.insert(t.end(), cells + 2048 * k, cells + 2048 * (k + 1));   // (validated: the canonical bytes of the elements)
    t.insert(t.end(), proofs + 48 * k, proofs + 48 * (k + 1));
  }
}
// getBatchBlindingFactor (ethereum_eip4844_kzg.nim:148-162): false = all zero, or zero mod r: use the Fiat-Shamir challenge
inline bool verify_blinding(uint64_t r[4], const uint8_t rnd[32]) {
  uint8_t any = 0;
  for (int i = 0; i < 32; i++) any |= rnd[i];
  if (!any) return false;
  reduce_256_mod_r(rnd, r);
  return (r[0] | r[1] | r[2] | r[3]) != 0;
}

// ---- constants ----------------------------------------------------------------------------------------------------------------------
// h_j^(-i), j < 128, i < 64, as Montgomery words [128][64][8]; h_j = omega_8192^brp7(j)
inline void verify_hinv_table(std::vector<uint32_t>& tab) {
  tab.resize((size_t)N_CELLS * CELL_ELEMS * 8);
  const FrH w = root_of_unity(13);
  for (int j = 0; j < N_CELLS; j++) {
    const uint64_t e[1] = {bit_reverse((uint32_t)j, 7)};
    const FrH hi = FrH::inv(e[0] ? fpow<FrH>(w, e, 1) : FrH::one());
    FrH x = FrH::one();
    for (int i = 0; i < CELL_ELEMS; i++) {
      memcpy(&tab[((size_t)j * CELL_ELEMS + i) * 8], x.l, 32);
      x = FrH::mul(x, hi);
    }
  }
}
// a counting sort of k by column: order[start[j] .. start[j + 1]) = the cells of column j in input order
inline void verify_column_lists(const uint64_t* idx, size_t n, uint32_t start[N_CELLS + 1], std::vector<uint32_t>& order) {
  uint32_t fill[N_CELLS];
  for (int j = 0; j <= N_CELLS; j++) start[j] = 0;
  for (size_t k = 0; k < n; k++) start[idx[k] + 1]++;
  for (int j = 0; j < N_CELLS; j++) {
    start[j + 1] += start[j];
    fill[j] = start[j];
  }
  order.resize(n);
  for (size_t k = 0; k < n; k++) order[fill[idx[k]]++] = (uint32_t)k;
}
// The scalar vectors of a call, Montgomery words of 32 bytes each:
//   rho_r2[n]        rho_k R^2: one Montgomery product in k_vf_colsum converts a cell's element and applies the weight
//   ll[n]            rho_k
//   rl[M + 64 + n]   w_i, then 64 words left zero for k_vf_interp's -c[i], then rho_k h_k^64
inline void verify_scalars(const uint64_t r_c[4], const uint64_t* idx, const uint32_t* cidx, size_t n, size_t M, const std::vector<FrH>& ck,
                           std::vector<uint64_t>& rho_r2, std::vector<uint64_t>& ll, std::vector<uint64_t>& rl) {
  rho_r2.resize(4 * n);
  ll.resize(4 * n);
  rl.assign(4 * (M + CELL_ELEMS + n), 0);
  std::vector<FrH> w(M, FrH::zero());
  const FrH r = to_mont<FrH>(r_c);
  FrH rho = FrH::one();
  for (size_t k = 0; k < n; k++) {
    rho = FrH::mul(rho, r);
    memcpy(&ll[4 * k], rho.l, 32);
    const FrH t = to_mont<FrH>(rho.l);
    memcpy(&rho_r2[4 * k], t.l, 32);
    w[cidx[k]] = FrH::add(w[cidx[k]], rho);
    const FrH p = FrH::mul(rho, ck[idx[k]]);
    memcpy(&rl[4 * (M + CELL_ELEMS + k)], p.l, 32);
  }
  for (size_t i = 0; i < M; i++) memcpy(&rl[4 * i], w[i].l, 32);
}

// the answer of the device's checks: the status of the first offender in the reference's order -- the unique commitments in
// first-occurrence order (each: encoding, x < p, on the curve, in the subgroup), the cells in input order, the proofs in input order.
// status, in_subgroup: M + n entries, the commitments first; bad: n entries
inline int verify_first_offender(const uint32_t* status, const uint8_t* in_subgroup, size_t M, const uint32_t* bad, size_t n) {
  for (size_t i = 0; i < M; i++) {
    if (status[i] != (uint32_t)KZG_Success) return (int)status[i];
    if (!in_subgroup[i]) return KZG_EccPointNotInSubgroup;
  }
  for (size_t k = 0; k < n; k++)
    if (bad[k]) return KZG_ScalarLargerThanCurveOrder;
  for (size_t k = M; k < M + n; k++) {
    if (status[k] != (uint32_t)KZG_Success) return (int)status[k];
    if (!in_subgroup[k]) return KZG_EccPointNotInSubgroup;
  }
  return KZG_Success;
}

// ---- the kernel bodies ------------------------------------------------------------------------------------------------------------
// (p + 1)/4 and (p - 1)/2 of a field whose modulus is 3 (mod 4), as words, at compile time
template <class PP>
struct VfExponents {
  uint32_t sqrt[PP::N], half[PP::N];
  constexpr VfExponents() : sqrt{}, half{} {
    uint32_t t[PP::N] = {};
    uint64_t c = 1;
    for (int i = 0; i < PP::N; i++) {
      const uint64_t s = (uint64_t)PP::P[i] + c;
      t[i] = (uint32_t)s;
      c = s >> 32;
    }
    for (int i = 0; i < PP::N; i++) {
      sqrt[i] = (t[i] >> 2) | (i + 1 < PP::N ? t[i + 1] << 30 : 0u);
      half[i] = (PP::P[i] >> 1) | (i + 1 < PP::N ? PP::P[i + 1] << 31 : 0u);
    }
  }
};
template <class PP>
struct VfExp {
  static constexpr VfExponents<PP> E = VfExponents<PP>();
};
static_assert((BLS12_381_Fp::P[0] & 3u) == 3u, "y = (y^2)^((p+1)/4) needs p = 3 (mod 4)");

// a >= b for little-endian words: the borrow of a - b
template <int N>
CTT_HD bool vf_geq(const uint32_t* a, const uint32_t* b) {
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - bw;
    bw = (uint32_t)(d >> 63);
  }
  return bw == 0;
}

// One lane per compressed G1 point (the ZCash encoding, compressed_x / g1_decompress of protocols_host.h word for word): the flags,
// x < p, y = (x^3 + 4)^((p+1)/4) with the square checked, the sign from the flag; the neutral becomes (0, 0).  out: affine Montgomery
// records in the C-API layout -- what ctt_hip_subgroup_check(points_on_device = 1) and ctt_hip_msm_device read; a refused point's
// record is zeroed, so that the subgroup check that follows reads defined memory.  status: KZG_Success or the Ecc status.
struct VfDecompressArgs {
  const uint8_t* in;   // [n][48]
  uint32_t* out;       // [n][24]
  uint32_t* status;    // [n]
  uint32_t n;
  uint32_t split, gap; // lane i writes record i, from lane `split` on record i + gap (verify.hip leaves room for the setup's points)
};
CTT_HD void vf_decompress_body(const VfDecompressArgs& a, uint32_t lane) {
  if (lane >= a.n) return;
  const uint8_t* src = a.in + (uint64_t)lane * 48u;
  FpD x;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = (const uint4*)src;   // (the buffer is 16-byte aligned, and so is every record of 48 bytes)
  const uint4 w0 = q[0], w1 = q[1], w2 = q[2];
  x.l[11] = __builtin_bswap32(w0.x); x.l[10] = __builtin_bswap32(w0.y); x.l[9] = __builtin_bswap32(w0.z); x.l[8] = __builtin_bswap32(w0.w);
  x.l[7] = __builtin_bswap32(w1.x); x.l[6] = __builtin_bswap32(w1.y); x.l[5] = __builtin_bswap32(w1.z); x.l[4] = __builtin_bswap32(w1.w);
  x.l[3] = __builtin_bswap32(w2.x); x.l[2] = __builtin_bswap32(w2.y); x.l[1] = __builtin_bswap32(w2.z); x.l[0] = __builtin_bswap32(w2.w);
#else
  for (int w = 0; w < 12; w++) {
    const uint8_t* b = src + 44 - 4 * w;
    x.l[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
  }
#endif
  const uint32_t flags = x.l[11] >> 29;   // 4: compressed, 2: infinity, 1: y is the larger root
  x.l[11] &= 0x1fffffffu;
  uint32_t st = (uint32_t)KZG_Success;
  FpD X = FpD::zero(), Y = FpD::zero();
  if (!(flags & 4u)) {
    st = (uint32_t)KZG_EccInvalidEncoding;
  } else if (flags & 2u) {
    if ((flags & 1u) || !x.is_zero()) st = (uint32_t)KZG_EccInvalidEncoding;
  } else if (vf_geq<FpD::N>(x.l, BLS12_381_Fp::P)) {
    st = (uint32_t)KZG_EccCoordinateGreaterThanOrEqualModulus;
  } else {
    X = FpD::to_mont(x);
    const FpD four = FpD::dbl(FpD::dbl(FpD::one()));
    const FpD y2 = FpD::add(FpD::mul(FpD::sqr(X), X), four);
    FpD y = y2;                                            // the exponent's leading bit
    for (int i = BLS12_381_Fp::BITS - 3 - 1; i >= 0; i--) {   // (p + 1)/4 has BITS - 2 bits
      y = FpD::sqr(y);
      if ((VfExp<BLS12_381_Fp>::E.sqrt[i >> 5] >> (i & 31)) & 1u) y = FpD::mul(y, y2);
    }
    if (!FpD::eq(FpD::sqr(y), y2)) {
      st = (uint32_t)KZG_EccPointNotOnCurve;
      X = FpD::zero();
    } else {
      const FpD yc = FpD::from_mont(y);
      // y > (p - 1)/2  <=>  not (half >= y)
      const bool larger = !vf_geq<FpD::N>(VfExp<BLS12_381_Fp>::E.half, yc.l);
      Y = FpD::cneg(y, larger != ((flags & 1u) != 0));
    }
  }
  uint32_t* dst = a.out + (uint64_t)(lane + (lane >= a.split ? a.gap : 0u)) * 24u;
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* o = (uint4*)dst;   // (96-byte records of a 16-byte aligned buffer)
  o[0] = make_uint4(X.l[0], X.l[1], X.l[2], X.l[3]);
  o[1] = make_uint4(X.l[4], X.l[5], X.l[6], X.l[7]);
  o[2] = make_uint4(X.l[8], X.l[9], X.l[10], X.l[11]);
  o[3] = make_uint4(Y.l[0], Y.l[1], Y.l[2], Y.l[3]);
  o[4] = make_uint4(Y.l[4], Y.l[5], Y.l[6], Y.l[7]);
  o[5] = make_uint4(Y.l[8], Y.l[9], Y.l[10], Y.l[11]);
#else
  for (int w = 0; w < 12; w++) {
    dst[w] = X.l[w];
    dst[12 + w] = Y.l[w];
  }
#endif
  a.status[lane] = st;
}

// One lane per (column j, element e), 128 * 64 lanes: S[j][e] = sum over the cells k of column j of rho_k cell_k[e], walking the
// column's list.  An element >= r is left out of the sum and stores 1 into bad[k] (every such lane stores the same value: no atomic;
// the caller zeroes bad[] first); the call then ends with a status and the sums are not used.
struct VfColsumArgs {
  const uint8_t* cells;     // [n][64] elements of 32 big-endian bytes
  const uint32_t* rho_r2;   // [n] rho_k R^2 as Montgomery words
  const uint32_t* start;    // [129]
  const uint32_t* order;    // [n]
  uint32_t* rows;           // [128][64] Montgomery
  uint32_t* bad;            // [n]
};
CTT_HD void vf_colsum_body(const VfColsumArgs& a, uint32_t lane) {
  if (lane >= VF_COLSUM_LANES) return;
  const uint32_t j = lane / CELL_ELEMS, e = lane % CELL_ELEMS;
  FrD acc = FrD::zero();
  for (uint32_t t = a.start[j]; t < a.start[j + 1]; t++) {
    const uint32_t k = a.order[t];
    const uint8_t* src = a.cells + ((uint64_t)k * CELL_ELEMS + e) * 32u;
    FrD c;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4* q = (const uint4*)src;   // (the buffer is 32-byte aligned, and so is every element)
    const uint4 hi = q[0], lo = q[1];
    c.l[7] = __builtin_bswap32(hi.x); c.l[6] = __builtin_bswap32(hi.y); c.l[5] = __builtin_bswap32(hi.z); c.l[4] = __builtin_bswap32(hi.w);
    c.l[3] = __builtin_bswap32(lo.x); c.l[2] = __builtin_bswap32(lo.y); c.l[1] = __builtin_bswap32(lo.z); c.l[0] = __builtin_bswap32(lo.w);
#else
    for (int w = 0; w < 8; w++) {
      const uint8_t* b = src + 28 - 4 * w;
      c.l[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
    }
#endif
    if (vf_geq<FrD::N>(c.l, BLS12_381_Fr::P)) {
      a.bad[k] = 1u;
      continue;
    }
    acc = FrD::add(acc, FrD::mul(c, ntt_ld<FrD>(a.rho_r2, k)));
  }
  ntt_st<FrD>(a.rows, lane, acc);
}

// Lane i < 64: -c[i] = -sum_j h_j^(-i) a_j[i], Montgomery, written where the MSM of RL reads its scalars.
struct VfInterpArgs {
  const uint32_t* rows;   // [128][64] a_j[i], Montgomery
  const uint32_t* hinv;   // [128][64] h_j^(-i), Montgomery
  uint32_t* out;          // [64]
};
CTT_HD void vf_interp_body(const VfInterpArgs& a, uint32_t lane) {
  if (lane >= (uint32_t)CELL_ELEMS) return;
  FrD acc = FrD::zero();
  for (uint32_t j = 0; j < (uint32_t)N_CELLS; j++)
    acc = FrD::add(acc, FrD::mul(ntt_ld<FrD>(a.rows, j * CELL_ELEMS + lane), ntt_ld<FrD>(a.hinv, j * CELL_ELEMS + lane)));
  ntt_st<FrD>(a.out, lane, FrD::neg(acc));
}

}  // namespace ctt::proto
