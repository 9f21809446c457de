// protocols_host.h -- the host logic of the protocol symbols: everything that decides about untrusted bytes, and the formulas that
// need no GPU.  Plain C++17 without the GPU runtime: protocols.hip (the GPU side and the C symbols) and the stand-alone
// tests/protocols_harness.cpp (tests/test_protocols_host.py; sanitizers by hand, README) include the same definitions.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <vector>

#include "host_fp64.h"
#include "ntt_bodies.h"

namespace ctt::proto {

using FpH = Fp64<BLS12_381_Fp>;
using FrH = Fp64<BLS12_381_Fr>;
using Fp2H = Fp2<FpH>;
using FrD = Fp<BLS12_381_Fr>;   // the device's 32-bit limbs: what cell_quotient_body computes on
constexpr int N_BLOB = 4096;
constexpr int N_CELLS = 128, CELL_ELEMS = 64;

// ---- field helpers (host, 64-bit limbs) ---------------------------------------------------------------------------------
template <class F>
inline F raw_const(const uint32_t* w) {
  F r;
  for (int i = 0; i < F::N; i++) r.l[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  return r;
}
// canonical little-endian limbs < modulus?
template <class F>
inline bool below_modulus(const uint64_t* v) {
  for (int i = F::N - 1; i >= 0; i--) {
    if (v[i] < F::P(i)) return true;
    if (v[i] > F::P(i)) return false;
  }
  return false;  // equal
}
// big-endian bytes (8*N of them) -> canonical limbs
template <class F>
inline void limbs_from_be(const uint8_t* be, uint64_t* v) {
  for (int i = 0; i < F::N; i++) {
    uint64_t w = 0;
    for (int b = 0; b < 8; b++) w = (w << 8) | be[8 * (F::N - 1 - i) + b];
    v[i] = w;
  }
}
template <class F>
inline void limbs_to_be(const uint64_t* v, uint8_t* be) {
  for (int i = 0; i < F::N; i++)
    for (int b = 0; b < 8; b++) be[8 * (F::N - 1 - i) + b] = (uint8_t)(v[i] >> (56 - 8 * b));
}
template <class F>
inline F to_mont(const uint64_t* canon) {
  F a;
  for (int i = 0; i < F::N; i++) a.l[i] = canon[i];
  return F::mul(a, raw_const<F>(F::Params::R2));
}
template <class F>
inline void from_mont(const F& a, uint64_t* canon) {
  F one_raw = F::zero();
  one_raw.l[0] = 1;
  const F r = F::mul(a, one_raw);
  for (int i = 0; i < F::N; i++) canon[i] = r.l[i];
}
template <class F>
inline F fpow(const F& base, const uint64_t* e, int nlimbs) {
  F r = F::one();
  bool started = false;
  for (int i = nlimbs * 64 - 1; i >= 0; i--) {
    if (started) r = F::sqr(r);
    if ((e[i >> 6] >> (i & 63)) & 1) {
      r = started ? F::mul(r, base) : base;
      started = true;
    }
  }
  return r;
}
// v > (p-1)/2 for a canonical value
inline bool fp_is_larger_half(const uint64_t* v) {
  for (int i = FpH::N - 1; i >= 0; i--) {
    const uint64_t h = (FpH::P(i) >> 1) | (i + 1 < FpH::N ? FpH::P(i + 1) << 63 : 0);   // limb i of (p-1)/2 = p >> 1: p is odd
    if (v[i] > h) return true;
    if (v[i] < h) return false;
  }
  return false;
}

// ---- SHA-256 (FIPS 180-4), for the Fiat-Shamir challenge of compute_blob_kzg_proof -------------------------------------
struct Sha256 {
  uint32_t h[8];
  uint8_t buf[64];
  uint64_t len = 0;
  size_t fill = 0;
  Sha256() {
    static const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    memcpy(h, iv, sizeof h);
  }
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
      0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
      0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
      0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
      0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
      0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g);
      const uint32_t t1 = hh + S1 + ch + K[i] + w[i];
      const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & b) ^ (a & c) ^ (b & c);
      const uint32_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
#if defined(__x86_64__)
  // the same compression function on the SHA extensions (the Fiat-Shamir challenge hashes a whole blob, 128 KiB: 0.35 ms with
  // the portable rounds, ~0.07 ms here); chosen at run time
  __attribute__((target("sha,sse4.1,ssse3"))) void blocks_shani(const uint8_t* p, size_t nblk) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bULL, 0x0405060700010203ULL);
    __m128i t = _mm_loadu_si128((const __m128i*)&h[0]);    // a b c d
    __m128i s1 = _mm_loadu_si128((const __m128i*)&h[4]);   // e f g h
    t = _mm_shuffle_epi32(t, 0xB1);                        // c d a b
    s1 = _mm_shuffle_epi32(s1, 0x1B);                      // h g f e
    __m128i s0 = _mm_alignr_epi8(t, s1, 8);                // a b e f
    s1 = _mm_blend_epi16(s1, t, 0xF0);                     // c d g h
    for (size_t b = 0; b < nblk; b++, p += 64) {
      const __m128i save0 = s0, save1 = s1;
      __m128i m[4];
      for (int i = 0; i < 4; i++) m[i] = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i*)(p + 16 * i)), bswap);
      for (int r = 0; r < 16; r++) {
        __m128i w = m[r & 3];
        if (r >= 4) {   // message schedule: w[4r .. 4r+3] from the previous four vectors
          __m128i x = _mm_sha256msg1_epu32(m[r & 3], m[(r + 1) & 3]);
          x = _mm_add_epi32(x, _mm_alignr_epi8(m[(r + 3) & 3], m[(r + 2) & 3], 4));
          w = _mm_sha256msg2_epu32(x, m[(r + 3) & 3]);
          m[r & 3] = w;
        }
        __m128i wk = _mm_add_epi32(w, _mm_loadu_si128((const __m128i*)&K[4 * r]));
        s1 = _mm_sha256rnds2_epu32(s1, s0, wk);
        wk = _mm_shuffle_epi32(wk, 0x0E);
        s0 = _mm_sha256rnds2_epu32(s0, s1, wk);
      }
      s0 = _mm_add_epi32(s0, save0);
      s1 = _mm_add_epi32(s1, save1);
    }
    t = _mm_shuffle_epi32(s0, 0x1B);                       // f e b a
    s1 = _mm_shuffle_epi32(s1, 0xB1);                      // d c h g
    s0 = _mm_blend_epi16(t, s1, 0xF0);                     // d c b a
    s1 = _mm_alignr_epi8(s1, t, 8);                        // h g f e
    _mm_storeu_si128((__m128i*)&h[0], s0);
    _mm_storeu_si128((__m128i*)&h[4], s1);
  }
  static bool have_shani() {
    static const bool v = __builtin_cpu_supports("sha") && __builtin_cpu_supports("sse4.1") && __builtin_cpu_supports("ssse3") &&
                          !(getenv("CTT_HIP_NO_SHANI") && atoi(getenv("CTT_HIP_NO_SHANI")) != 0);
    return v;
  }
#else
  void blocks_shani(const uint8_t*, size_t) {}
  static bool have_shani() { return false; }
#endif
  void update(const uint8_t* p, size_t n) {
    len += n;
    while (n) {
      if (fill == 0 && n >= 64) {
        if (have_shani()) {
          const size_t nb = n / 64;
          blocks_shani(p, nb);
          p += 64 * nb;
          n -= 64 * nb;
          continue;
        }
        block(p);
        p += 64;
        n -= 64;
        continue;
      }
      const size_t take = n < 64 - fill ? n : 64 - fill;
      memcpy(buf + fill, p, take);
      fill += take;
      p += take;
      n -= take;
      if (fill == 64) {
        if (have_shani()) blocks_shani(buf, 1); else block(buf);
        fill = 0;
      }
    }
  }
  void finish(uint8_t out[32]) {
    const uint64_t bits = len * 8;
    const uint8_t one = 0x80, zero = 0;
    update(&one, 1);
    while (fill != 56) update(&zero, 1);
    uint8_t lb[8];
    for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(lb, 8);
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(h[i] >> 24);
      out[4 * i + 1] = (uint8_t)(h[i] >> 16);
      out[4 * i + 2] = (uint8_t)(h[i] >> 8);
      out[4 * i + 3] = (uint8_t)h[i];
    }
  }
};

// ---- status codes of the reference's interfaces (values as in their headers) ---------------------------------------------
enum : int { KZG_Success = 0, KZG_VerificationFailure = 1, KZG_InputsLengthsMismatch = 2, KZG_ScalarZero = 3, KZG_ScalarLargerThanCurveOrder = 4,
             KZG_EccInvalidEncoding = 5, KZG_EccCoordinateGreaterThanOrEqualModulus = 6, KZG_EccPointNotOnCurve = 7, KZG_EccPointNotInSubgroup = 8 };
enum : int { TS_Success = 0, TS_MissingOrInaccessibleFile = 1, TS_InvalidFile = 2 };
enum : int { EVM_Success = 0, EVM_InvalidInputSize = 1, EVM_InvalidOutputSize = 2, EVM_IntLargerThanModulus = 3, EVM_PointNotOnCurve = 4,
             EVM_PointNotInSubgroup = 5 };

// ---- BLS12-381: y^2 = x^3 + b over the coordinate field F, b = 4 on G1 (Fp) and 4 (1 + i) on G2 (Fp2) -----------------------
template <class F> inline F curve_b();
template <> inline FpH curve_b<FpH>() { return FpH::dbl(FpH::dbl(FpH::one())); }
template <> inline Fp2H curve_b<Fp2H>() { return {curve_b<FpH>(), curve_b<FpH>()}; }
template <class F>
inline F curve_rhs(const F& x) { return F::add(F::mul(F::sqr(x), x), curve_b<F>()); }
template <class F>
inline bool on_curve(const F& x, const F& y) { return F::eq(F::sqr(y), curve_rhs(x)); }

// ---- the ZCash / IETF compressed encoding (serialization/codecs_bls12_381.nim) ---------------------------------------------
// The flag byte, the infinity encoding and the range of a compressed point's x over `coords` 48-byte big-endian coordinates (G1: 1,
// G2: 2): the compression flag set; infinity with every other bit zero; else every coordinate below p -> xc[coords][6] canonical.
// -> KZG_Success (inf says which form), KZG_EccInvalidEncoding or, after it, KZG_EccCoordinateGreaterThanOrEqualModulus
inline int compressed_x(const uint8_t* in, int coords, bool& inf, uint64_t (*xc)[FpH::N]) {
  inf = false;
  if (!(in[0] & 0x80)) return KZG_EccInvalidEncoding;   // only the compressed form
  if (in[0] & 0x40) {                                   // infinity: every other bit zero
    if (in[0] & 0x3f) return KZG_EccInvalidEncoding;
    for (int i = 1; i < 48 * coords; i++)
      if (in[i]) return KZG_EccInvalidEncoding;
    inf = true;
    return KZG_Success;
  }
  for (int k = 0; k < coords; k++) {
    uint8_t be[48];
    memcpy(be, in + 48 * k, 48);
    if (k == 0) be[0] &= 0x1f;
    limbs_from_be<FpH>(be, xc[k]);
    if (!below_modulus<FpH>(xc[k])) return KZG_EccCoordinateGreaterThanOrEqualModulus;
  }
  return KZG_Success;
}
// G1 -> affine Montgomery {x, y} in the C-API layout (96 bytes; the neutral is (0,0)).  No subgroup check here.
inline int g1_decompress(uint8_t aff[96], const uint8_t in[48]) {
  bool inf;
  uint64_t xc[1][FpH::N];
  const int st = compressed_x(in, 1, inf, xc);
  if (st != KZG_Success) return st;
  if (inf) {
    memset(aff, 0, 96);
    return KZG_Success;
  }
  const FpH x = to_mont<FpH>(xc[0]);
  const FpH y2 = curve_rhs(x);
  // p = 3 (mod 4): y = y2^((p+1)/4)
  uint64_t e[FpH::N];
  {
    uint64_t c = 1;   // p + 1
    for (int i = 0; i < FpH::N; i++) {
      const uint64_t s = FpH::P(i) + c;
      c = (s < c) ? 1 : 0;
      e[i] = s;
    }
    for (int i = 0; i < FpH::N; i++) e[i] = (e[i] >> 2) | (i + 1 < FpH::N ? e[i + 1] << 62 : 0);
  }
  FpH y = fpow<FpH>(y2, e, FpH::N);
  if (!FpH::eq(FpH::sqr(y), y2)) return KZG_EccPointNotOnCurve;
  uint64_t yc[FpH::N];
  from_mont<FpH>(y, yc);
  if (((in[0] & 0x20) != 0) != fp_is_larger_half(yc)) y = FpH::neg(y);
  memcpy(aff, x.l, 48);
  memcpy(aff + 48, y.l, 48);
  return KZG_Success;
}
inline void g1_compress(uint8_t out[48], const uint8_t aff[96]) {
  FpH x, y;
  memcpy(x.l, aff, 48);
  memcpy(y.l, aff + 48, 48);
  if (x.is_zero() && y.is_zero()) {
    memset(out, 0, 48);
    out[0] = 0xc0;
    return;
  }
  uint64_t xc[FpH::N], yc[FpH::N];
  from_mont<FpH>(x, xc);
  from_mont<FpH>(y, yc);
  limbs_to_be<FpH>(xc, out);
  out[0] |= 0x80 | (fp_is_larger_half(yc) ? 0x20 : 0);
}

// ---- EIP-4844: bytes_to_bls_field (ethereum_eip4844_kzg.nim:158-166): 32 big-endian bytes -> canonical limbs, which must be < r
inline int bytes_to_bls_field(uint64_t v[4], const uint8_t be[32]) {
  limbs_from_be<FrH>(be, v);
  return below_modulus<FrH>(v) ? KZG_Success : KZG_ScalarLargerThanCurveOrder;
}
// blob -> 4096 canonical little-endian scalars (blob_to_bigint_polynomial: every element < r)
inline int blob_to_scalars(uint8_t* out_le, const uint8_t* blob) {
  for (int i = 0; i < N_BLOB; i++) {
    uint64_t v[FrH::N];
    limbs_from_be<FrH>(blob + 32 * i, v);
    if (!below_modulus<FrH>(v)) return KZG_ScalarLargerThanCurveOrder;
    memcpy(out_le + 32 * i, v, 32);
  }
  return KZG_Success;
}
// 256-bit big-endian integer reduced mod r (fromDigest, ethereum_eip4844_kzg.nim:103-126; the EVM scalars, :941-952) -> canonical limbs
inline void reduce_256_mod_r(const uint8_t be[32], uint64_t v[4]) {
  limbs_from_be<FrH>(be, v);
  while (!below_modulus<FrH>(v)) {   // 2^256 < 3r: at most two subtractions
    uint64_t bw = 0;
    for (int i = 0; i < 4; i++) {
      const unsigned __int128 x = (unsigned __int128)v[i] - FrH::P(i) - bw;
      v[i] = (uint64_t)x;
      bw = (uint64_t)(x >> 64) & 1;
    }
  }
}
// fiatShamirChallenge (ethereum_eip4844_kzg.nim:126-148): sha256(domain | 16-byte big-endian degree | blob | commitment) mod r
inline void fiat_shamir_challenge(uint64_t z[4], const uint8_t* blob, const uint8_t commitment[48]) {
  Sha256 t;
  t.update((const uint8_t*)"FSBLOBVERIFY_V1_", 16);
  uint8_t deg[16] = {0};
  deg[14] = (uint8_t)(N_BLOB >> 8);
  deg[15] = (uint8_t)(N_BLOB & 0xff);
  t.update(deg, 16);
  t.update(blob, (size_t)N_BLOB * 32);
  t.update(commitment, 48);
  uint8_t d[32];
  t.finish(d);
  reduce_256_mod_r(d, z);
}

inline uint32_t bit_reverse(uint32_t i, int bits) {
  uint32_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((i >> b) & 1u) << (bits - 1 - b);
  return r;
}
// 7^((r-1)/2^log2n), Montgomery
inline FrH root_of_unity(int log2n) {
  uint64_t e[4];
  for (int i = 0; i < 4; i++) e[i] = FrH::P(i);
  e[0] -= 1;
  for (int i = 0; i < 4; i++) e[i] = (e[i] >> log2n) | (i + 1 < 4 ? e[i + 1] << (64 - log2n) : 0);
  const uint64_t seven[4] = {7, 0, 0, 0};
  return fpow<FrH>(to_mont<FrH>(seven), e, 4);
}
// the 4096 roots of unity in bit-reversed order, Montgomery residues (ctx.domain_brp, commitments_setups/ethereum_kzg_srs.nim)
inline std::vector<FrH> domain_brp() {
  const FrH w = root_of_unity(12);
  std::vector<FrH> nat(N_BLOB), brp(N_BLOB);
  FrH x = FrH::one();
  for (int i = 0; i < N_BLOB; i++) {
    nat[i] = x;
    x = FrH::mul(x, w);
  }
  for (int i = 0; i < N_BLOB; i++) brp[i] = nat[bit_reverse((uint32_t)i, 12)];
  return brp;
}

// Montgomery's trick: out[i] = 1/v[i]; every v[i] non-zero
inline void batch_inverse(const std::vector<FrH>& v, std::vector<FrH>& out) {
  const size_t n = v.size();
  out.resize(n);
  FrH run = FrH::one();
  for (size_t i = 0; i < n; i++) {
    out[i] = run;
    run = FrH::mul(run, v[i]);
  }
  FrH inv = FrH::inv(run);
  for (size_t i = n; i-- > 0;) {
    out[i] = FrH::mul(inv, out[i]);
    inv = FrH::mul(inv, v[i]);
  }
}

// getQuotientPoly (math/polynomials/polynomials.nim; kzg_prove, commitments/kzg.nim:204-223) on the host: y = p(z) and
// q = (p - y)/(X - z) in evaluation form over the bit-reversed domain, both branches (z outside / inside the domain).  The
// device runs the first branch (ctt_hip_fr_quotient); this is what serves "z is a root of unity" and what the device form is
// tested against.  poly, q: canonical little-endian scalars; z canonical limbs; y canonical limbs out.
inline void quotient_host(const std::vector<FrH>& dom, const uint8_t* poly_le, const uint64_t z_c[4], uint8_t* q_le, uint64_t y_c[4]) {
  const int n = N_BLOB;
  std::vector<FrH> p(n);
  for (int i = 0; i < n; i++) {
    uint64_t v[4];
    memcpy(v, poly_le + 32 * i, 32);
    p[i] = to_mont<FrH>(v);
  }
  const FrH z = to_mont<FrH>(z_c);
  int m = -1;
  for (int i = 0; i < n; i++)
    if (FrH::eq(dom[i], z)) {
      m = i;
      break;
    }
  std::vector<FrH> q(n), d, inv;
  FrH y;
  if (m < 0) {
    d.resize(n);
    for (int i = 0; i < n; i++) d[i] = FrH::sub(z, dom[i]);                       // z - w_i
    batch_inverse(d, inv);
    FrH s = FrH::zero();
    for (int i = 0; i < n; i++) s = FrH::add(s, FrH::mul(FrH::mul(p[i], dom[i]), inv[i]));
    const uint64_t nn[4] = {(uint64_t)n, 0, 0, 0};
    const FrH zn = fpow<FrH>(z, nn, 1);                                          // z^n
    const FrH ninv = FrH::inv(to_mont<FrH>(nn));
    y = FrH::mul(FrH::mul(FrH::sub(zn, FrH::one()), ninv), s);                    // barycentric evaluation
    for (int i = 0; i < n; i++) q[i] = FrH::mul(FrH::sub(y, p[i]), inv[i]);       // (p_i - y)/(w_i - z)
  } else {
    y = p[m];
    d.reserve(n - 1);
    for (int i = 0; i < n; i++)
      if (i != m) d.push_back(FrH::sub(dom[i], z));                               // w_i - z
    batch_inverse(d, inv);
    const FrH zinv = FrH::inv(z);
    FrH acc = FrH::zero();
    int k = 0;
    for (int i = 0; i < n; i++) {
      if (i == m) continue;
      q[i] = FrH::mul(FrH::sub(p[i], y), inv[k++]);
      acc = FrH::add(acc, FrH::mul(FrH::mul(q[i], dom[i]), zinv));                // q_m = - sum q_i w_i / z
    }
    q[m] = FrH::neg(acc);
  }
  from_mont<FrH>(y, y_c);
  for (int i = 0; i < n; i++) {
    uint64_t v[4];
    from_mont<FrH>(q[i], v);
    memcpy(q_le + 32 * i, v, 32);
  }
}

// ---- the c-kzg text format of the Ethereum ceremony ("4096\n65\n", one hex point per line; the reference ships it as
// constantine/commitments_setups/trusted_setup_ethereum_kzg4844_reference.dat).  The reader follows load_ckzg4844
// (constantine/commitments_setups/ethereum_kzg_srs.nim:242-350): "%4u" counts, then 4096 Lagrange G1 lines of exactly 96 hex
// characters, 65 monomial G2 lines of exactly 192, 4096 monomial G1 lines of 96, LF or CRLF line ends; anything else -- a short
// file, a long line, a character that is not a hex digit -- is cttEthTS_InvalidFile.  The G2 and monomial-G1 sections serve
// verification and the FK20 form of the cell proofs, neither of which this library has: their lines are checked for length, hex
// digits, the compression flag and coordinates below p (compressed_x), not decompressed (round 4 did not read them at all: a
// truncated file loaded -- ADVICE r4).
inline bool srs_hex_line(FILE* f, size_t hex_chars, uint8_t* out) {
  char buf[200];
  size_t got = 0;
  int ch;
  while ((ch = fgetc(f)) != EOF && ch != '\n' && ch != '\r') {
    if (got >= hex_chars || !isxdigit(ch)) return false;
    buf[got++] = (char)ch;
  }
  if (got != hex_chars) return false;
  while (ch == '\r' || ch == '\n') ch = fgetc(f);   // the line end (and blank lines, as fscanf's "%*[\r\n]" skips them)
  if (ch != EOF) ungetc(ch, f);
  auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10); };
  for (size_t i = 0; i < hex_chars / 2; i++) out[i] = (uint8_t)(nib(buf[2 * i]) << 4 | nib(buf[2 * i + 1]));
  return true;
}
// the file at `path` -> ctt_eth_trusted_setup_status; g1_lagrange: the 4096 x 48 bytes of the Lagrange section in file order (the
// commitment key; the caller decompresses and subgroup-checks it), defined on TS_Success only
inline int srs_read_ckzg4844(const char* path, uint8_t* g1_lagrange) {
  FILE* f = fopen(path, "rb");
  if (!f) return TS_MissingOrInaccessibleFile;
  unsigned n1 = 0, n2 = 0;
  bool ok = fscanf(f, "%4u\n", &n1) == 1 && n1 == (unsigned)N_BLOB && fscanf(f, "%4u\n", &n2) == 1 && n2 == 65u;
  bool inf;
  uint64_t xc[2][FpH::N];
  for (int i = 0; ok && i < N_BLOB; i++) ok = srs_hex_line(f, 96, g1_lagrange + (size_t)i * 48);
  for (int i = 0; ok && i < 65; i++) {
    uint8_t g2[96];
    ok = srs_hex_line(f, 192, g2) && compressed_x(g2, 2, inf, xc) == KZG_Success;
  }
  for (int i = 0; ok && i < N_BLOB; i++) {
    uint8_t g1[48];
    ok = srs_hex_line(f, 96, g1) && compressed_x(g1, 1, inf, xc) == KZG_Success;
  }
  fclose(f);
  return ok ? TS_Success : TS_InvalidFile;
}

// ---- EIP-2537 BLS12_G1MSM / BLS12_G2MSM (ethereum_evm_precompiles.h:386,419), one form over the coordinate field F: FpH for G1,
// Fp2H for G2.  A coordinate is K base-field elements of 64 bytes each (c0 then c1), the same order as the C-API's affine layout.
// parseRawUint: a 64-byte big-endian field element, top 16 bytes zero, below p
inline bool evm_fp(const uint8_t* b64, FpH& out) {
  for (int i = 0; i < 16; i++)
    if (b64[i]) return false;
  uint64_t v[FpH::N];
  limbs_from_be<FpH>(b64 + 16, v);
  if (!below_modulus<FpH>(v)) return false;
  out = to_mont<FpH>(v);
  return true;
}
template <class F>
struct EvmMsm {
  static constexpr int K = sizeof(F) / sizeof(FpH);
  static constexpr size_t AFF = 2 * sizeof(F);        // affine Montgomery {x, y}: 96 / 192 bytes
  static constexpr size_t OUT = 2 * K * 64;           // the encoded point: 128 / 256 bytes
  static constexpr size_t REC = OUT + 32;             // point | scalar: 160 / 288 bytes
  // the pairs in an input of `len` bytes; 0: not a positive multiple of REC (cttEVM_InvalidInputSize)
  static size_t pairs(size_t len) { return len % REC == 0 ? len / REC : 0; }
  // The host-side verdict parse[i] on every pair (the reference handles the pairs in order: fromRawCoords,
  // ethereum_evm_precompiles.nim:316-389), pts[i] = the point for an accepted pair that is not the neutral and zero otherwise,
  // coefs[i] = the scalar mod r for every pair (the spec allows any s < 2^256; the group is cyclic of order r)
  static void parse(const uint8_t* inputs, size_t n, std::vector<uint8_t>& pts, std::vector<uint8_t>& coefs, std::vector<int>& verdict) {
    pts.assign(n * AFF, 0);
    coefs.resize(n * 32);
    verdict.assign(n, EVM_Success);
    for (size_t i = 0; i < n; i++) {
      const uint8_t* rec = inputs + i * REC;
      FpH c[2 * K];
      int k = 0;
      while (k < 2 * K && evm_fp(rec + 64 * k, c[k])) k++;
      if (k < 2 * K) {
        verdict[i] = EVM_IntLargerThanModulus;
      } else {
        F xy[2];
        memcpy(xy, c, AFF);
        if (!(xy[0].is_zero() && xy[1].is_zero())) {
          if (!on_curve(xy[0], xy[1])) verdict[i] = EVM_PointNotOnCurve;
          else memcpy(&pts[i * AFF], c, AFF);
        }
      }
      uint64_t s[4];
      reduce_256_mod_r(rec + OUT, s);
      memcpy(&coefs[i * 32], s, 32);
    }
  }
  // the result: the neutral is (0,0) in both encodings
  static void encode(uint8_t* r, const uint8_t* aff) {
    for (int k = 0; k < 2 * K; k++) {
      FpH v;
      uint64_t c[FpH::N];
      memcpy(v.l, aff + 48 * k, 48);
      from_mont<FpH>(v, c);
      memset(r + 64 * k, 0, 16);
      limbs_to_be<FpH>(c, r + 64 * k + 16);
    }
  }
};

// ---- EIP-7594 cells and cell proofs -----------------------------------------------------------------------------------------
// c_k = omega_8192^(64 * brp7(k)), Montgomery: the coset of cell k is c_k^(1/64) * <omega_64>
inline std::vector<FrH> cell_coset_constants(const FrH& w8192) {
  std::vector<FrH> ck(N_CELLS);
  for (int k = 0; k < N_CELLS; k++) {
    const uint64_t e[1] = {64ull * bit_reverse((uint32_t)k, 7)};
    ck[k] = e[0] ? fpow<FrH>(w8192, e, 1) : FrH::one();
  }
  return ck;
}
// The quotients of the blob's polynomial p by X^64 - c_k, k < 128, in coefficient form: q_k[j] = p[j + 64] + c_k * q_k[j + 64] with
// q_k[j] = 0 from j = 4032 on -- a Horner walk with stride 64, so lane (k, s) owns the residue class s mod 64 of cell k and walks it
// downwards: 63 multiply-adds.  The 64 lanes of a cell read and write neighbouring elements.  The remainder (the cell's interpolant)
// is never needed.  p, c_k Montgomery; q Montgomery, or canonical with `canon` (the test-facing ctt_hip_eth_kzg_cell_quotients).
struct CellQuotArgs {
  const uint32_t* p;    // [4096]
  const uint32_t* ck;   // [128]
  uint32_t* q;          // [128][4096]
  uint32_t canon;
};
CTT_HD void cell_quotient_body(const CellQuotArgs& a, uint32_t lane) {
  if (lane >= (uint32_t)(N_CELLS * CELL_ELEMS)) return;
  const uint32_t k = lane / CELL_ELEMS, s = lane % CELL_ELEMS;
  const FrD c = ntt_ld<FrD>(a.ck, k);
  const uint64_t row = (uint64_t)k * N_BLOB;
  FrD acc = FrD::zero();
  ntt_st<FrD>(a.q, row + s + 64u * 63u, acc);
  for (int m = 62; m >= 0; m--) {
    acc = FrD::add(ntt_ld<FrD>(a.p, s + 64u * (uint32_t)(m + 1)), FrD::mul(c, acc));
    ntt_st<FrD>(a.q, row + s + 64u * (uint32_t)m, a.canon ? FrD::from_mont(acc) : acc);
  }
}

}  // namespace ctt::proto
