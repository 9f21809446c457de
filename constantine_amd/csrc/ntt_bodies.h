// ntt_bodies.h -- the batched number-theoretic transform over a scalar field C::Fr (the saturated Fp<PP> of fp.h, 8 words), written
// CTT_HD like the quotient and Verkle bodies: the kernels of ntt.hip and the CPU harness tests/ntt_harness.cpp run the same code.
// Passes and tiles: ntt_plan.h; DESIGN.md section 13.
//
// A pass is split around its barriers into phases a harness calls lane by lane:
//   ntt_tile_load    every element of the tile read once from global memory into the image (first pass: the input's conversion
//                    to Montgomery form and the coset shift's g^i)
//   ntt_tile_stage   one radix-2 stage on the image: 2^(E-1) butterflies shared among the lanes
//   ntt_tile_store   every element written once (last pass: g^-i / n of an inverse, the conversion to the canonical form)
// The image is word-major, [8][2^E] u32: lanes that walk neighbouring elements hit distinct LDS banks.
#pragma once
#include "fp.h"
#include "ntt_plan.h"

namespace ctt {

enum : uint32_t {
  NTT_INVERSE = 1u,      // twiddles omega^-e = -omega^(n/2 - e)
  NTT_DIT = 2u,          // stages from bit 0 upwards, the twiddle before the butterfly (else DIF: from the top bit, twiddle behind)
  NTT_FIRST = 4u,        // the transform's first pass: pre_c and pre apply at the load
  NTT_LAST = 8u,         // its last pass: post and post_c apply at the store
  NTT_HAS_PRE_C = 16u,
  NTT_HAS_POST_C = 32u,
  NTT_PRE_BRP = 64u,     // the array is in bit-reversed order at the first load: natural index = brp(position)
  NTT_POST_BRP = 128u,   // the same at the last store
};

template <class Fr>
struct NttArgs {
  const uint32_t* in;    // batch rows of n elements of 8 words; == out from the second pass on
  uint32_t* out;
  const uint32_t* tw;    // [n/2] omega^i, Montgomery
  const uint32_t* pre;   // NULL, or [n] multipliers by natural index (g^i), Montgomery
  const uint32_t* post;  // NULL, or [n] multipliers by natural index (g^-i / n), Montgomery
  Fr pre_c, post_c;      // one multiplier for every element (R^2: canonical in; 1 or 1/n as plain words: canonical out)
  uint32_t log2n;
  uint32_t flags;
  NttPass pass;
};

template <class Fr>
CTT_HD Fr ntt_ld(const uint32_t* p, uint64_t i) {
  Fr r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = (const uint4*)(p + i * 8u);
  const uint4 a = q[0], b = q[1];
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
#else
  for (int w = 0; w < 8; w++) r.l[w] = p[i * 8u + w];
#endif
  return r;
}
template <class Fr>
CTT_HD void ntt_st(uint32_t* p, uint64_t i, const Fr& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = (uint4*)(p + i * 8u);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
#else
  for (int w = 0; w < 8; w++) p[i * 8u + w] = v.l[w];
#endif
}
template <class Fr>
CTT_HD Fr ntt_img_get(const uint32_t* img, uint32_t stride, uint32_t m) {
  Fr r;
#pragma unroll
  for (int w = 0; w < 8; w++) r.l[w] = img[(uint32_t)w * stride + m];
  return r;
}
template <class Fr>
CTT_HD void ntt_img_put(uint32_t* img, uint32_t stride, uint32_t m, const Fr& v) {
#pragma unroll
  for (int w = 0; w < 8; w++) img[(uint32_t)w * stride + m] = v.l[w];
}

// i with its low `bits` bits reversed (i < 2^bits, 1 <= bits <= 32)
CTT_HD uint32_t ntt_brp(uint32_t i, uint32_t bits) {
  i = ((i >> 1) & 0x55555555u) | ((i & 0x55555555u) << 1);
  i = ((i >> 2) & 0x33333333u) | ((i & 0x33333333u) << 2);
  i = ((i >> 4) & 0x0f0f0f0fu) | ((i & 0x0f0f0f0fu) << 4);
  i = ((i >> 8) & 0x00ff00ffu) | ((i & 0x00ff00ffu) << 8);
  i = (i >> 16) | (i << 16);
  return i >> (32u - bits);
}

// tile_id counts the tiles of all rows: 2^(L - E) per row
template <class Fr>
CTT_HD void ntt_tile_load(const NttArgs<Fr>& a, uint32_t* img, uint32_t tile_id, uint32_t lane, uint32_t nlanes) {
  const NttPass& q = a.pass;
  const uint32_t L = a.log2n, stride = 1u << q.E;
  const uint32_t row = tile_id >> (L - q.E), tile = tile_id & ((1u << (L - q.E)) - 1u);
  const uint64_t base = (uint64_t)row << L;
  for (uint32_t m = lane; m < stride; m += nlanes) {
    const uint32_t i = ntt_tile_index(q, tile, m);
    Fr v = ntt_ld<Fr>(a.in, base + i);
    if (a.flags & NTT_FIRST) {
      if (a.flags & NTT_HAS_PRE_C) v = Fr::mul(v, a.pre_c);
      if (a.pre) v = Fr::mul(v, ntt_ld<Fr>(a.pre, (a.flags & NTT_PRE_BRP) ? ntt_brp(i, L) : i));
    }
    ntt_img_put<Fr>(img, stride, m, v);
  }
}

// stage k of the pass (0 <= k < t): index bit lo + k, local bit sl + k.  DIF runs k = t-1 .. 0, DIT k = 0 .. t-1.
template <class Fr>
CTT_HD void ntt_tile_stage(const NttArgs<Fr>& a, uint32_t* img, uint32_t tile_id, uint32_t k, uint32_t lane, uint32_t nlanes) {
  const NttPass& q = a.pass;
  const uint32_t L = a.log2n, stride = 1u << q.E, half = stride >> 1;
  const uint32_t tile = tile_id & ((1u << (L - q.E)) - 1u);
  const uint32_t s = q.lo + k, lb = q.sl + k, hn = 1u << (L - 1u);
  for (uint32_t b = lane; b < half; b += nlanes) {
    const uint32_t m0 = ((b >> lb) << (lb + 1u)) | (b & ((1u << lb) - 1u)), m1 = m0 | (1u << lb);
    const uint32_t i = ntt_tile_index(q, tile, m0);
    const uint32_t e = (i & ((1u << s) - 1u)) << (L - 1u - s);   // omega^e, e < n/2
    Fr w;
    if (a.flags & NTT_INVERSE) {
      w = ntt_ld<Fr>(a.tw, e ? hn - e : 0u);
      w = Fr::cneg(w, e != 0u);
    } else {
      w = ntt_ld<Fr>(a.tw, e);
    }
    const Fr x = ntt_img_get<Fr>(img, stride, m0);
    Fr y = ntt_img_get<Fr>(img, stride, m1);
    if (a.flags & NTT_DIT) {
      y = Fr::mul(y, w);
      ntt_img_put<Fr>(img, stride, m0, Fr::add(x, y));
      ntt_img_put<Fr>(img, stride, m1, Fr::sub(x, y));
    } else {
      ntt_img_put<Fr>(img, stride, m0, Fr::add(x, y));
      ntt_img_put<Fr>(img, stride, m1, Fr::mul(Fr::sub(x, y), w));
    }
  }
}

template <class Fr>
CTT_HD void ntt_tile_store(const NttArgs<Fr>& a, const uint32_t* img, uint32_t tile_id, uint32_t lane, uint32_t nlanes) {
  const NttPass& q = a.pass;
  const uint32_t L = a.log2n, stride = 1u << q.E;
  const uint32_t row = tile_id >> (L - q.E), tile = tile_id & ((1u << (L - q.E)) - 1u);
  const uint64_t base = (uint64_t)row << L;
  for (uint32_t m = lane; m < stride; m += nlanes) {
    const uint32_t i = ntt_tile_index(q, tile, m);
    Fr v = ntt_img_get<Fr>(img, stride, m);
    if (a.flags & NTT_LAST) {
      if (a.post) v = Fr::mul(v, ntt_ld<Fr>(a.post, (a.flags & NTT_POST_BRP) ? ntt_brp(i, L) : i));
      if (a.flags & NTT_HAS_POST_C) v = Fr::mul(v, a.post_c);
    }
    ntt_st<Fr>(a.out, base + i, v);
  }
}

// out[i] = c0 * base^i for i < count, Montgomery: the twiddle table of a plan (c0 = 1, base = omega) and the multipliers of a coset
// shift.  A lane owns K neighbouring entries: base^(lane * K) by square and multiply, then K - 1 products.
template <class Fr>
struct NttPowArgs {
  uint32_t* out;
  Fr base, c0;
  uint32_t count, K;
};
template <class Fr>
CTT_HD void ntt_powers_body(const NttPowArgs<Fr>& a, uint32_t lane) {
  const uint64_t first = (uint64_t)lane * a.K;
  if (first >= a.count) return;
  Fr r = Fr::one();
  for (int b = 31; b >= 0; b--) {
    r = Fr::sqr(r);
    if ((first >> b) & 1u) r = Fr::mul(r, a.base);
  }
  r = Fr::mul(r, a.c0);
  for (uint32_t j = 0; j < a.K && first + j < a.count; j++) {
    ntt_st<Fr>(a.out, first + j, r);
    r = Fr::mul(r, a.base);
  }
}

// the rows of `buf` put into bit-reversed order in place: lane idx of batch * n swaps element i = idx mod n with brp(i) when i < brp(i)
template <class Fr>
CTT_HD void ntt_brp_swap_body(uint32_t* buf, uint32_t log2n, uint64_t total, uint64_t idx) {
  if (idx >= total) return;
  const uint32_t i = (uint32_t)(idx & ((1u << log2n) - 1u)), j = ntt_brp(i, log2n);
  if (i >= j) return;
  const uint64_t base = idx - i;
  const Fr x = ntt_ld<Fr>(buf, base + i), y = ntt_ld<Fr>(buf, base + j);
  ntt_st<Fr>(buf, base + i, y);
  ntt_st<Fr>(buf, base + j, x);
}

// ---- host side, shared by the launch path (ntt.hip) and the CPU harness: one transform as its passes' arguments ------------------
template <class Fr>
struct NttCall {
  NttArgs<Fr> common;              // everything but in, pass, the FIRST / LAST bits, pre and post
  const uint32_t* in;
  const uint32_t* mult;            // the coset shift's multipliers (g^i forward, g^-i / n inverse) or NULL
  NttPass passes[NTT_MAX_PASSES];
  int npass;
  bool inverse, swap;              // swap: the rows go through ntt_brp_swap_body behind the last pass
};
// flags: NTT_FLAG_*; ninv = 1/n, tw and mult Montgomery
template <class Fr>
inline void ntt_setup(NttCall<Fr>& c, int log2n, int tile_log2, int flags, const Fr& ninv, const uint32_t* tw, const uint32_t* mult,
                      void* out, const void* in) {
  using PP = typename Fr::Params;
  const bool inverse = flags & NTT_FLAG_INVERSE, dit = flags & NTT_FLAG_IN_BRP, out_brp = flags & NTT_FLAG_OUT_BRP;
  NttArgs<Fr>& a = c.common;
  a.in = nullptr;
  a.out = (uint32_t*)out;
  a.tw = tw;
  a.pre = a.post = nullptr;
  a.log2n = (uint32_t)log2n;
  a.pre_c = Fr::zero();
  a.post_c = Fr::zero();
  a.flags = (inverse ? NTT_INVERSE : 0u) | (dit ? NTT_DIT | NTT_PRE_BRP : NTT_POST_BRP);
  if (!(flags & NTT_FLAG_IN_MONT)) {
    a.flags |= NTT_HAS_PRE_C;
    for (int i = 0; i < Fr::N; i++) a.pre_c.l[i] = PP::R2[i];
  }
  if (inverse && !mult) {          // 1/n; as plain words it takes the result out of Montgomery form in the same product
    a.flags |= NTT_HAS_POST_C;
    a.post_c = (flags & NTT_FLAG_OUT_MONT) ? ninv : Fr::from_mont(ninv);
  } else if (!(flags & NTT_FLAG_OUT_MONT)) {
    a.flags |= NTT_HAS_POST_C;
    a.post_c.l[0] = 1u;
  }
  c.in = (const uint32_t*)in;
  c.mult = mult;
  c.inverse = inverse;
  c.npass = ntt_plan_passes(log2n, tile_log2, dit, c.passes);
  // DIF leaves the rows bit-reversed and DIT in natural order: the other order is a swap pass over the output
  c.swap = log2n >= 2 && out_brp == dit;
}
template <class Fr>
inline NttArgs<Fr> ntt_pass_args(const NttCall<Fr>& c, int k) {
  NttArgs<Fr> a = c.common;
  a.in = k == 0 ? c.in : a.out;
  a.pass = c.passes[k];
  a.flags |= (k == 0 ? NTT_FIRST : 0u) | (k == c.npass - 1 ? NTT_LAST : 0u);
  a.pre = (k == 0 && !c.inverse) ? c.mult : nullptr;
  a.post = (k == c.npass - 1 && c.inverse) ? c.mult : nullptr;
  return a;
}

}  // namespace ctt
