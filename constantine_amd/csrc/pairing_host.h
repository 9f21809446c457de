// pairing_host.h -- the BLS12-381 optimal ate pairing on the host, for the ONE pairing check that ends a batched cell-proof
// verification (verify.hip): two Miller loops into one accumulator and one final exponentiation, whatever the
// size of the batch.  Plain C++17 without the GPU runtime, over FpH / Fp2H of protocols_host.h; tests/verify_harness.cpp includes the
// same definitions.  Nothing here is constant-time and nothing needs to be: every input of a verification is public.
//
// Tower:  Fp2 = Fp[i]/(i^2 + 1),  Fp6 = Fp2[v]/(v^3 - xi),  Fp12 = Fp6[w]/(w^2 - v),  xi = 1 + i; so w^6 = xi, and an element of Fp12 is
//   a_0 + a_1 w + ... + a_5 w^5  with  a_0, a_2, a_4 = c0.{c0, c1, c2}  and  a_1, a_3, a_5 = c1.{c0, c1, c2}.
// Twist (M type):  E'(Fp2): y^2 = x^3 + 4 xi;  (x', y') -> (x'/w^2, y'/w^3) is on E(Fp12): y^2 = x^3 + 4.
// Lines:  G2 points stay affine on the twist (one Fp2 inversion per step: 68 + 5 steps per loop, a few microseconds each).  The line
//   through T with slope s, evaluated at P = (xP, yP) in G1 and scaled by w^3 (an element of Fp4: the final exponentiation sends it to 1):
//       (s x_T - y_T)  -  s xP w^2  +  yP w^3
// Miller loop:  over |x| = 0xd201000000010000 from its second-highest bit down; x is negative, so the value is conjugated at the end.
// Final exponentiation:  f^((p^12 - 1)/r) EXACTLY --
//   easy part  f^((p^6 - 1)(p^2 + 1)):  conj(f) * f^-1, then times its own p^2-Frobenius;
//   hard part  a plain square-and-multiply by (p^4 - p^2 + 1)/r (PairingBls12381::HARD_EXP of field_params.h, 1268 bits: ~1900 Fp12
//              operations).  No power of the pairing other than the first is produced: GT values equal those of any implementation
//              that raises the Miller value to (p^12 - 1)/r (tests/_pairingref.py does, with one pow).
// The Frobenius constants xi^(k (p^2 - 1)/6) are generated from integers by gen_params.py and compared with Python by the CPU test.
#pragma once
#include "protocols_host.h"

namespace ctt::proto {

constexpr uint64_t BLS_X_ABS = 0xd201000000010000ull;

inline FpH fp_const(const uint32_t* w) { return raw_const<FpH>(w); }
inline Fp2H fp2_mul_xi(const Fp2H& a) { return {FpH::sub(a.c0, a.c1), FpH::add(a.c0, a.c1)}; }   // (a0 + a1 i)(1 + i)
inline Fp2H fp2_mul_fp(const Fp2H& a, const FpH& k) { return {FpH::mul(a.c0, k), FpH::mul(a.c1, k)}; }
inline Fp2H fp2_conj(const Fp2H& a) { return {a.c0, FpH::neg(a.c1)}; }

struct Fp6H {
  Fp2H c0, c1, c2;
  static Fp6H zero() { return {Fp2H::zero(), Fp2H::zero(), Fp2H::zero()}; }
  static Fp6H one() { return {Fp2H::one(), Fp2H::zero(), Fp2H::zero()}; }
  static Fp6H add(const Fp6H& a, const Fp6H& b) { return {Fp2H::add(a.c0, b.c0), Fp2H::add(a.c1, b.c1), Fp2H::add(a.c2, b.c2)}; }
  static Fp6H sub(const Fp6H& a, const Fp6H& b) { return {Fp2H::sub(a.c0, b.c0), Fp2H::sub(a.c1, b.c1), Fp2H::sub(a.c2, b.c2)}; }
  static Fp6H neg(const Fp6H& a) { return {Fp2H::neg(a.c0), Fp2H::neg(a.c1), Fp2H::neg(a.c2)}; }
  static bool eq(const Fp6H& a, const Fp6H& b) { return Fp2H::eq(a.c0, b.c0) && Fp2H::eq(a.c1, b.c1) && Fp2H::eq(a.c2, b.c2); }
  // (c0 + c1 v + c2 v^2) v = xi c2 + c0 v + c1 v^2
  static Fp6H mul_v(const Fp6H& a) { return {fp2_mul_xi(a.c2), a.c0, a.c1}; }
  static Fp6H mul(const Fp6H& a, const Fp6H& b) {
    const Fp2H t0 = Fp2H::mul(a.c0, b.c0), t1 = Fp2H::mul(a.c1, b.c1), t2 = Fp2H::mul(a.c2, b.c2);
    const Fp2H m12 = Fp2H::sub(Fp2H::sub(Fp2H::mul(Fp2H::add(a.c1, a.c2), Fp2H::add(b.c1, b.c2)), t1), t2);   // a1 b2 + a2 b1
    const Fp2H m01 = Fp2H::sub(Fp2H::sub(Fp2H::mul(Fp2H::add(a.c0, a.c1), Fp2H::add(b.c0, b.c1)), t0), t1);   // a0 b1 + a1 b0
    const Fp2H m02 = Fp2H::sub(Fp2H::sub(Fp2H::mul(Fp2H::add(a.c0, a.c2), Fp2H::add(b.c0, b.c2)), t0), t2);   // a0 b2 + a2 b0
    return {Fp2H::add(t0, fp2_mul_xi(m12)), Fp2H::add(m01, fp2_mul_xi(t2)), Fp2H::add(m02, t1)};
  }
  static Fp6H inv(const Fp6H& a) {
    const Fp2H A = Fp2H::sub(Fp2H::sqr(a.c0), fp2_mul_xi(Fp2H::mul(a.c1, a.c2)));
    const Fp2H B = Fp2H::sub(fp2_mul_xi(Fp2H::sqr(a.c2)), Fp2H::mul(a.c0, a.c1));
    const Fp2H C = Fp2H::sub(Fp2H::sqr(a.c1), Fp2H::mul(a.c0, a.c2));
    const Fp2H F = Fp2H::add(Fp2H::mul(a.c0, A), fp2_mul_xi(Fp2H::add(Fp2H::mul(a.c2, B), Fp2H::mul(a.c1, C))));
    const Fp2H Fi = Fp2H::inv(F);
    return {Fp2H::mul(A, Fi), Fp2H::mul(B, Fi), Fp2H::mul(C, Fi)};
  }
};

struct Fp12H {
  Fp6H c0, c1;
  static Fp12H one() { return {Fp6H::one(), Fp6H::zero()}; }
  static bool eq(const Fp12H& a, const Fp12H& b) { return Fp6H::eq(a.c0, b.c0) && Fp6H::eq(a.c1, b.c1); }
  static Fp12H mul(const Fp12H& a, const Fp12H& b) {
    const Fp6H t0 = Fp6H::mul(a.c0, b.c0), t1 = Fp6H::mul(a.c1, b.c1);
    const Fp6H m = Fp6H::sub(Fp6H::sub(Fp6H::mul(Fp6H::add(a.c0, a.c1), Fp6H::add(b.c0, b.c1)), t0), t1);
    return {Fp6H::add(t0, Fp6H::mul_v(t1)), m};
  }
  static Fp12H sqr(const Fp12H& a) { return mul(a, a); }
  static Fp12H conj(const Fp12H& a) { return {a.c0, Fp6H::neg(a.c1)}; }   // a^(p^6): w -> -w
  static Fp12H inv(const Fp12H& a) {
    const Fp6H d = Fp6H::inv(Fp6H::sub(Fp6H::mul(a.c0, a.c0), Fp6H::mul_v(Fp6H::mul(a.c1, a.c1))));
    return {Fp6H::mul(a.c0, d), Fp6H::neg(Fp6H::mul(a.c1, d))};
  }
  // the coefficient of w^k, k < 6
  Fp2H& at(int k) { Fp6H& h = (k & 1) ? c1 : c0; return k / 2 == 0 ? h.c0 : k / 2 == 1 ? h.c1 : h.c2; }
  const Fp2H& at(int k) const { return const_cast<Fp12H*>(this)->at(k); }
};

// xi^(k (p^2 - 1)/6), k = 0 .. 5 (Montgomery; in Fp)
inline FpH frobenius2_constant(int k) {
  switch (k) {
    case 1: return fp_const(PairingBls12381::FROB2_1);
    case 2: return fp_const(PairingBls12381::FROB2_2);
    case 3: return fp_const(PairingBls12381::FROB2_3);
    case 4: return fp_const(PairingBls12381::FROB2_4);
    case 5: return fp_const(PairingBls12381::FROB2_5);
    default: return FpH::one();
  }
}
// a^(p^2): Fp2 is fixed, w^(p^2) = w * xi^((p^2 - 1)/6)
inline Fp12H fp12_frobenius2(const Fp12H& a) {
  Fp12H r = a;
  for (int k = 1; k < 6; k++) r.at(k) = fp2_mul_fp(a.at(k), frobenius2_constant(k));
  return r;
}

inline Fp12H final_exponentiation(const Fp12H& f) {
  const Fp12H g = Fp12H::mul(Fp12H::conj(f), Fp12H::inv(f));     // f^(p^6 - 1)
  const Fp12H e = Fp12H::mul(fp12_frobenius2(g), g);             // ^(p^2 + 1)
  Fp12H r = Fp12H::one();
  bool started = false;
  for (int i = 64 * PairingBls12381::HARD_LIMBS - 1; i >= 0; i--) {
    if (started) r = Fp12H::sqr(r);
    if ((PairingBls12381::HARD_EXP[i >> 6] >> (i & 63)) & 1) {
      r = started ? Fp12H::mul(r, e) : e;
      started = true;
    }
  }
  return r;
}

// ---- points: affine, Montgomery, the C-API layout; the neutral is all zero ---------------------------------------------------
struct G1Aff {
  FpH x, y;
  bool is_inf() const { return x.is_zero() && y.is_zero(); }
};
struct G2Aff {
  Fp2H x, y;
  bool is_inf() const { return x.is_zero() && y.is_zero(); }
};
inline G1Aff g1_from_bytes(const uint8_t* aff96) {
  G1Aff p;
  memcpy(p.x.l, aff96, 48);
  memcpy(p.y.l, aff96 + 48, 48);
  return p;
}
inline G2Aff g2_from_bytes(const uint8_t* aff192) {
  G2Aff q;
  memcpy(q.x.c0.l, aff192, 48);
  memcpy(q.x.c1.l, aff192 + 48, 48);
  memcpy(q.y.c0.l, aff192 + 96, 48);
  memcpy(q.y.c1.l, aff192 + 144, 48);
  return q;
}
inline void g2_to_bytes(const G2Aff& q, uint8_t* aff192) {
  memcpy(aff192, q.x.c0.l, 48);
  memcpy(aff192 + 48, q.x.c1.l, 48);
  memcpy(aff192 + 96, q.y.c0.l, 48);
  memcpy(aff192 + 144, q.y.c1.l, 48);
}
inline G2Aff g2_generator() {
  return {{fp_const(GenBls12381G2::C0), fp_const(GenBls12381G2::C1)}, {fp_const(GenBls12381G2::C2), fp_const(GenBls12381G2::C3)}};
}

// f *= the line through T with slope s at P (the header's form)
inline void miller_line(Fp12H& f, const Fp2H& s, const G2Aff& T, const G1Aff& P) {
  Fp12H l = {Fp6H::zero(), Fp6H::zero()};
  l.at(0) = Fp2H::sub(Fp2H::mul(s, T.x), T.y);
  l.at(2) = Fp2H::neg(fp2_mul_fp(s, P.x));
  l.at(3) = {P.y, FpH::zero()};
  f = Fp12H::mul(f, l);
}
// f *= f_{|x|, Q}(P) conjugated -- one pair's factor of the product of pairings before the final exponentiation.  A neutral P or Q
// contributes 1.  Q of order r never meets T = +-Q or a point of order 2 inside the loop; a Q outside the subgroup that does ends the
// walk with the vertical line's value dropped (it lies in Fp6, which the final exponentiation sends to 1).
inline void miller_loop_into(Fp12H& acc, const G1Aff& P, const G2Aff& Q) {
  if (P.is_inf() || Q.is_inf()) return;
  Fp12H f = Fp12H::one();
  G2Aff T = Q;
  bool t_inf = false;
  const FpH three = FpH::add(FpH::dbl(FpH::one()), FpH::one());
  for (int i = 62; i >= 0; i--) {   // bit 63 is the leading one
    f = Fp12H::sqr(f);
    if (!t_inf) {
      if (T.y.is_zero()) {
        t_inf = true;
      } else {
        const Fp2H s = Fp2H::mul(fp2_mul_fp(Fp2H::sqr(T.x), three), Fp2H::inv(Fp2H::dbl(T.y)));
        miller_line(f, s, T, P);
        const Fp2H x3 = Fp2H::sub(Fp2H::sqr(s), Fp2H::dbl(T.x));
        T = {x3, Fp2H::sub(Fp2H::mul(s, Fp2H::sub(T.x, x3)), T.y)};
      }
    }
    if ((BLS_X_ABS >> i) & 1) {
      if (t_inf) {
        T = Q;
        t_inf = false;
      } else if (Fp2H::eq(T.x, Q.x)) {
        if (Fp2H::eq(T.y, Q.y) && !T.y.is_zero()) {
          const Fp2H s = Fp2H::mul(fp2_mul_fp(Fp2H::sqr(T.x), three), Fp2H::inv(Fp2H::dbl(T.y)));
          miller_line(f, s, T, P);
          const Fp2H x3 = Fp2H::sub(Fp2H::sqr(s), Fp2H::dbl(T.x));
          T = {x3, Fp2H::sub(Fp2H::mul(s, Fp2H::sub(T.x, x3)), T.y)};
        } else {
          t_inf = true;
        }
      } else {
        const Fp2H s = Fp2H::mul(Fp2H::sub(Q.y, T.y), Fp2H::inv(Fp2H::sub(Q.x, T.x)));
        miller_line(f, s, T, P);
        const Fp2H x3 = Fp2H::sub(Fp2H::sub(Fp2H::sqr(s), T.x), Q.x);
        T = {x3, Fp2H::sub(Fp2H::mul(s, Fp2H::sub(T.x, x3)), T.y)};
      }
    }
  }
  acc = Fp12H::mul(acc, Fp12H::conj(f));
}

inline Fp12H pairing(const G1Aff& P, const G2Aff& Q) {
  Fp12H f = Fp12H::one();
  miller_loop_into(f, P, Q);
  return final_exponentiation(f);
}
// prod_i e(P_i, Q_i) == 1
inline bool pairing_check(const G1Aff* P, const G2Aff* Q, size_t n) {
  Fp12H f = Fp12H::one();
  for (size_t i = 0; i < n; i++) miller_loop_into(f, P[i], Q[i]);
  return Fp12H::eq(final_exponentiation(f), Fp12H::one());
}

// ---- G2, the ZCash compressed encoding: 96 bytes, x.c1 then x.c0, the flags of G1 in the first byte; the sign flag says that y is the
// larger root, compared on y.c1 unless that is zero, then on y.c0 (deserialize_g2_compressed, serialization/codecs_bls12_381.nim).
// p = 3 (mod 4): the square root in Fp2 of Adj and Rodriguez-Henriquez, algorithm 9 -- a1 = a^((p-3)/4), alpha = a1^2 a, x0 = a1 a;
// alpha^(p+1) = -1: no root; alpha = -1: i x0; else (1 + alpha)^((p-1)/2) x0.  The result is squared and compared.
inline bool fp2_sqrt(Fp2H& out, const Fp2H& a) {
  if (a.is_zero()) {
    out = a;
    return true;
  }
  uint64_t e34[FpH::N], e12[FpH::N];   // (p - 3)/4 = p >> 2 and (p - 1)/2 = p >> 1
  for (int i = 0; i < FpH::N; i++) {
    e34[i] = (FpH::P(i) >> 2) | (i + 1 < FpH::N ? FpH::P(i + 1) << 62 : 0);
    e12[i] = (FpH::P(i) >> 1) | (i + 1 < FpH::N ? FpH::P(i + 1) << 63 : 0);
  }
  const Fp2H a1 = fpow<Fp2H>(a, e34, FpH::N);
  const Fp2H alpha = Fp2H::mul(Fp2H::sqr(a1), a);
  const Fp2H x0 = Fp2H::mul(a1, a);
  const Fp2H minus_one = Fp2H::neg(Fp2H::one());
  Fp2H x;
  if (Fp2H::eq(alpha, minus_one)) {
    x = {FpH::neg(x0.c1), x0.c0};   // i x0
  } else {
    const Fp2H b = fpow<Fp2H>(Fp2H::add(Fp2H::one(), alpha), e12, FpH::N);
    x = Fp2H::mul(b, x0);
  }
  if (!Fp2H::eq(Fp2H::sqr(x), a)) return false;
  out = x;
  return true;
}
inline bool g2_is_larger(const Fp2H& y) {
  uint64_t c[FpH::N];
  from_mont<FpH>(y.c1.is_zero() ? y.c0 : y.c1, c);
  return fp_is_larger_half(c);
}
// -> affine Montgomery {x.c0, x.c1, y.c0, y.c1} in the C-API layout (192 bytes; the neutral is all zero).  No subgroup check here.
inline int g2_decompress(uint8_t aff[192], const uint8_t in[96]) {
  bool inf;
  uint64_t xc[2][FpH::N];
  const int st = compressed_x(in, 2, inf, xc);
  if (st != KZG_Success) return st;
  if (inf) {
    memset(aff, 0, 192);
    return KZG_Success;
  }
  G2Aff q;
  q.x = {to_mont<FpH>(xc[1]), to_mont<FpH>(xc[0])};   // the bytes hold c1 first
  if (!fp2_sqrt(q.y, curve_rhs(q.x))) return KZG_EccPointNotOnCurve;
  if (((in[0] & 0x20) != 0) != g2_is_larger(q.y)) q.y = Fp2H::neg(q.y);
  g2_to_bytes(q, aff);
  return KZG_Success;
}

}  // namespace ctt::proto
