// verkle_bodies.h -- per-lane bodies of the batched Verkle commitment: a fixed-base table over at most 256 Banderwagon points, the
// commitment of one row of scalars, and the finish (affine point, 32-byte serialisation, map to the scalar field).
//
// A Verkle node commits 256 scalars against the 256 points of a fixed CRS (constantine/ethereum_verkle_ipa.nim:23-64) and a tree
// update does that thousands of times, so nothing of the MSM pipeline (sort, buckets, reduction passes) is used here:
//
//   table    for base i, window w of the balanced layout (msm_bodies.h window_layout) and j = 1 .. 2^(width(w)-1) the record
//            (x, y, d*x*y) of j * 2^off(w) * P_i, affine.  -(x, y, t) = (-x, y, -t).  All records of a base are consecutive, window
//            after window: record index = i * rows + vk_row_off(w) + j - 1.
//            VkTable is the view of it that every kernel's arguments hold and the one place a record's address is computed.
//   commit   lane i of a workgroup walks the Booth digits of scalar i of the row (booth_recode_packed, msm_bodies.h) and adds one record
//            per non-zero digit (vk_add_record: ed_madd_pre, 8M, ec.h); the workgroup then sums its lanes pairwise (the tree below).
//   update   a node in service changes a few of its 256 slots: new commitment = old commitment + sum (new - old) * P_i over those slots.
//            A row is a CSR list of (base index, delta); its entries x windows are spread over the lanes of one wave, one record per
//            non-zero digit as above, and the lane that ends up with the sum adds the old commitment.
//   tree     the pairwise sum of a group of lanes through slots of LDS, one level in two halves (vk_tree_put, vk_tree_take) with a
//            barrier after each; the commit kernel runs it over 128 slots, the update kernel over 32 per wave (vk_tree, verkle.hip).
//   finish   one inversion per chunk of points (Montgomery's trick over Y*Z) yields 1/Z and 1/Y of every point:
//            (x, y, 1), serializeBatch_vartime (serialization/codecs_banderwagon.nim:239-266), batchMapToScalarField (ethereum_verkle_ipa.nim:247-281).
//
// Bodies are __host__ __device__ like those of msm_bodies.h: the tests run them lane by lane on the CPU.
#pragma once
#include "msm_bodies.h"

namespace ctt {

static constexpr uint32_t VK_MAX_BASES = 256;      // lanes of a commit workgroup
static constexpr uint32_t VK_EXT_WORDS = 32;       // an extended point (X, Y, Z, T) between commit and finish
static constexpr uint32_t VK_REC_WORDS = 24;       // a packed table record (x, y, d*x*y); the padded form has a stride of 32 words
static constexpr uint32_t VK_FINISH_CHUNK = 8;     // points per inversion of the finish

// records of one base in front of window w: 2^(width - 1) per window, the r wide windows first
CTT_HD uint32_t vk_row_off(const WinLayout& L, uint32_t w) {
  const uint32_t wide = 1u << L.cb, narrow = 1u << (L.cb - 1), r = (uint32_t)L.r;
  return w < r ? w * wide : r * wide + (w - r) * narrow;
}

// The table as its users see it.  rec(i, w, j) is the record of (j + 1) * 2^off(w) * P_i; a walk over the windows of one base keeps
// the running vk_row_off itself and asks with rec_at.  The arguments of the table, commit and update kernels are this view (their
// base) followed by their own fields.
struct VkTable {
  uint32_t* tab;    // [n][rows] records
  uint32_t n, W;
  WinLayout lay;
  uint32_t rows;    // records per base = vk_row_off(lay, W)
  uint32_t stride;  // words per record: VK_REC_WORDS, or 32 (one 128-byte line per gather)
  CTT_HD uint32_t* rec_at(uint32_t i, uint32_t row_off, uint32_t j) const { return tab + ((uint64_t)i * rows + row_off + j) * stride; }
  CTT_HD uint32_t* rec(uint32_t i, uint32_t w, uint32_t j) const { return rec_at(i, vk_row_off(lay, w), j); }
};

template <class F>
CTT_HD F vk_load(const uint32_t* p) {
  F r;
#pragma unroll
  for (int k = 0; k < F::N; k++) r.l[k] = p[k];
  return r;
}
template <class F>
CTT_HD void vk_store(uint32_t* p, const F& v) {
#pragma unroll
  for (int k = 0; k < F::N; k++) p[k] = v.l[k];
}

// ---------------------------------------------------------------------------------------------
// table: one lane per (base, window)
// ---------------------------------------------------------------------------------------------
struct VkTableArgs : VkTable {
  const uint32_t* pts;   // [n] affine points, C-API layout (x, y Montgomery)
  uint32_t* pre;         // [n][rows][F::N] prefix products of Z while the lane's records are normalised
};

// 2^off(w) * P_i by doublings, its multiples by a running sum in extended coordinates parked in the records themselves, then one
// inversion for all Z of the lane.  (0, 1) and (0, -1) go through the law like any point.
template <class F>
CTT_HD void vk_table_body(const VkTableArgs& a, uint32_t lane) {
  if (lane >= a.n * a.W) return;
  const uint32_t i = lane % a.n, w = lane / a.n;
  const F px = vk_load<F>(a.pts + (uint64_t)i * 2 * F::N), py = vk_load<F>(a.pts + (uint64_t)i * 2 * F::N + F::N);
  XYZZ<F> q = {px, py, F::one(), F::mul(px, py)};
  for (int b = a.lay.off(w); b > 0; b--) q = ed_dbl<F>(q);
  const uint32_t half = 1u << (a.lay.width(w) - 1);
  const uint32_t row = vk_row_off(a.lay, w);
  const uint64_t e0 = (uint64_t)i * a.rows + row;   // the lane's first record, and first prefix product
  XYZZ<F> r = XYZZ<F>::inf();
  F run = F::one();
  for (uint32_t j = 0; j < half; j++) {
    r = ed_add<F>(r, q);
    uint32_t* rec = a.rec_at(i, row, j);
    vk_store<F>(rec, r.x);
    vk_store<F>(rec + F::N, r.y);
    vk_store<F>(rec + 2 * F::N, r.zz);
    vk_store<F>(a.pre + (e0 + j) * F::N, run);
    if (!r.zz.is_zero()) run = F::mul(run, r.zz);
  }
  F inv = F::inv(run);
  const F d = ed_d<F>();
  for (uint32_t j = half; j-- > 0;) {
    uint32_t* rec = a.rec_at(i, row, j);
    const F Z = vk_load<F>(rec + 2 * F::N);
    F x = F::zero(), y = F::zero();
    if (!Z.is_zero()) {   // (never zero for Banderwagon elements: the law is complete on them)
      const F zi = F::mul(inv, vk_load<F>(a.pre + (e0 + j) * F::N));
      inv = F::mul(inv, Z);
      x = F::mul(vk_load<F>(rec), zi);
      y = F::mul(vk_load<F>(rec + F::N), zi);
    }
    vk_store<F>(rec, x);
    vk_store<F>(rec + F::N, y);
    vk_store<F>(rec + 2 * F::N, F::mul(d, F::mul(x, y)));
  }
}

// ---------------------------------------------------------------------------------------------
// commit: lane i of row k
// ---------------------------------------------------------------------------------------------
struct VkCommitArgs : VkTable {
  const uint32_t* coefs;   // [m][n][8]
  uint32_t m;
  int fr;                  // 1: Montgomery residues of the scalar field, converted here
  uint32_t* out;           // [m] extended points, VK_EXT_WORDS each
};

// acc += (neg ? -1 : 1) * the record (x, y, d*x*y) at rec
template <class F>
CTT_HD void vk_add_record(XYZZ<F>& acc, bool& empty, const uint32_t* rec, bool neg) {
  const F x = vk_load<F>(rec), y = vk_load<F>(rec + F::N), t = vk_load<F>(rec + 2 * F::N);
  ed_madd_pre<F>(acc, empty, F::cneg(x, neg), y, F::cneg(t, neg));
}

// a[k][i] * P_i, or the in-memory neutral (all zero) when no digit is non-zero.  The scalar is shifted down window by window, so its
// words are only ever addressed with compile-time indices and the addition exists once in the code; the digit of a window is
// (its bits << 1 | the bit below) recoded by booth_recode_packed.
template <class F, class Fr>
CTT_HD XYZZ<F> vk_lane_sum(const VkCommitArgs& a, uint32_t k, uint32_t i) {
  XYZZ<F> acc = XYZZ<F>::inf();
  if (i >= a.n) return acc;
  uint32_t s[8];
  {
    Fr v = vk_load<Fr>(a.coefs + ((uint64_t)k * a.n + i) * 8);
    if (a.fr) v = Fr::from_mont(v);
#pragma unroll
    for (int t = 0; t < 8; t++) s[t] = v.l[t];
  }
  bool empty = true;
  uint32_t below = 0, row = 0;
  for (uint32_t w = 0; w < a.W; w++) {
    const uint32_t c = (uint32_t)a.lay.width(w), vmask = (1u << c) - 1u;
    const uint32_t d = ((s[0] & vmask) << 1) | below;
    below = (s[0] >> (c - 1)) & 1u;
#pragma unroll
    for (int t = 0; t < 7; t++) s[t] = (s[t] >> c) | (s[t + 1] << (32u - c));
    s[7] >>= c;
    const uint32_t dg = booth_recode_packed(d, c);
    if (dg != DIGIT_NONE) vk_add_record<F>(acc, empty, a.rec_at(i, row, dg >> 1), (dg & 1u) != 0);
    row += 1u << (c - 1);
  }
  if (empty) acc = XYZZ<F>::inf();
  return acc;
}

// what lane 0 writes: the sum, with the law's own neutral (0 : 1 : 1 : 0) for the in-memory one
template <class F>
CTT_HD void vk_store_ext(uint32_t* out, uint32_t k, const XYZZ<F>& sum) {
  const XYZZ<F> r = sum.is_inf() ? XYZZ<F>{F::zero(), F::one(), F::one(), F::zero()} : sum;
  uint32_t* o = out + (uint64_t)k * VK_EXT_WORDS;
  vk_store<F>(o, r.x);
  vk_store<F>(o + F::N, r.y);
  vk_store<F>(o + 2 * F::N, r.zz);
  vk_store<F>(o + 3 * F::N, r.zzz);
}

// ---------------------------------------------------------------------------------------------
// update: row k = old commitment + a few (base index, delta) entries; lane l of the row's group of G lanes
// ---------------------------------------------------------------------------------------------
struct VkUpdateArgs : VkTable {
  const uint32_t* row_ptr;   // [m + 1] first entry of every row, row_ptr[0] = 0 (CSR)
  const uint8_t* idx;        // [row_ptr[m]] base of every entry, below n
  const uint32_t* deltas;    // [row_ptr[m]][8]
  int fr;                    // 1: Montgomery residues of the scalar field, converted here
  const uint32_t* base;      // [m][24] old commitments (X, Y, Z), any non-zero Z; null: the neutral
  uint32_t m;
  uint32_t* out;             // [m] extended points, VK_EXT_WORDS each
};

// booth_digit_packed on a scalar held in registers, for a window that differs from lane to lane: the two words the window's bits
// lie in are picked by a select chain over compile-time indices, so the scalar never becomes a run-time-indexed array (scratch).
CTT_HD uint32_t vk_digit_regs(const uint32_t (&s)[8], uint32_t w, const WinLayout& L) {
  const uint32_t i = (uint32_t)L.off(w), c = (uint32_t)L.width(w);
  const uint32_t pos = i ? i - 1u : 0u, word = pos >> 5, sh = pos & 31u;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int t = 0; t < 8; t++) {
    lo = word == (uint32_t)t ? s[t] : lo;
    if (t < 7) hi = word == (uint32_t)t ? s[t + 1] : hi;
  }
  uint32_t d = i ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) : lo << 1;
  return booth_recode_packed(d & ((1u << (c + 1)) - 1u), c);
}

// The row's cnt * W items are (entry t / W, window t % W); lane l takes the items l, l + G, l + 2G, ... and adds one record per
// non-zero digit.  Two entries of a row may name the same base.  A canonical scalar's digit is read from global memory where it lies
// (booth_digit_packed); a Montgomery one is converted first, one product against the eight of the addition.
template <class F, class Fr>
CTT_HD XYZZ<F> vk_update_lane_sum(const VkUpdateArgs& a, uint32_t k, uint32_t l, uint32_t G) {
  XYZZ<F> acc = XYZZ<F>::inf();
  if (k >= a.m) return acc;
  const uint32_t e0 = a.row_ptr[k], cnt = a.row_ptr[k + 1] - e0;
  const uint32_t qG = G / a.W, rG = G % a.W;
  uint32_t ent = l / a.W, w = l % a.W;
  bool empty = true;
  while (ent < cnt) {
    const uint64_t e = (uint64_t)e0 + ent;
    uint32_t dg;
    if (a.fr) {
      const Fr v = Fr::from_mont(vk_load<Fr>(a.deltas + e * 8));
      uint32_t s[8];
#pragma unroll
      for (int t = 0; t < 8; t++) s[t] = v.l[t];
      dg = vk_digit_regs(s, w, a.lay);
    } else {
      dg = booth_digit_packed(a.deltas + e * 8, (int)w, a.lay);
    }
    if (dg != DIGIT_NONE) vk_add_record<F>(acc, empty, a.rec(a.idx[e], w, dg >> 1), (dg & 1u) != 0);
    ent += qG;
    w += rG;
    if (w >= a.W) {
      w -= a.W;
      ent++;
    }
  }
  if (empty) acc = XYZZ<F>::inf();
  return acc;
}

// what the lane that owns the row's sum writes: old commitment + sum.  (X : Y : Z) is the extended point (XZ : YZ : Z^2 : XY).
template <class F>
CTT_HD void vk_update_store(const VkUpdateArgs& a, uint32_t k, XYZZ<F> sum) {
  if (a.base) {
    const uint32_t* b = a.base + (uint64_t)k * 24u;
    const F X = vk_load<F>(b), Y = vk_load<F>(b + F::N), Z = vk_load<F>(b + 2 * F::N);
    sum = ed_add<F>(sum, XYZZ<F>{F::mul(X, Z), F::mul(Y, Z), F::sqr(Z), F::mul(X, Y)});
  }
  vk_store_ext<F>(a.out, k, sum);
}

// ---------------------------------------------------------------------------------------------
// tree: one level of the pairwise sum of a group of lanes through SLOTS slots of VK_EXT_WORDS words (LDS on the device, any array on
// the CPU).  At level s the lanes s <= lane < 2s put their point into slot lane - s, then -- after a barrier -- the lanes below s take
// slot `lane` and add it; a second barrier frees the slots for level s / 2.  A slot is stored word-major (word t of slot j at
// t * SLOTS + j) so that a wave's accesses fall into consecutive banks; SLOTS is a template argument so that the strides are immediates.
// The in-memory neutral passes through ed_add.
// ---------------------------------------------------------------------------------------------
template <class F, uint32_t SLOTS>
CTT_HD void vk_tree_put(uint32_t* slots, uint32_t lane, uint32_t s, const XYZZ<F>& acc) {
  if (lane < s || lane >= 2 * s) return;
  uint32_t* o = slots + (lane - s);
#pragma unroll
  for (int t = 0; t < F::N; t++) {
    o[t * SLOTS] = acc.x.l[t];
    o[(F::N + t) * SLOTS] = acc.y.l[t];
    o[(2 * F::N + t) * SLOTS] = acc.zz.l[t];
    o[(3 * F::N + t) * SLOTS] = acc.zzz.l[t];
  }
}
template <class F, uint32_t SLOTS>
CTT_HD void vk_tree_take(const uint32_t* slots, uint32_t lane, uint32_t s, XYZZ<F>& acc) {
  if (lane >= s) return;
  const uint32_t* o = slots + lane;
  XYZZ<F> q;
#pragma unroll
  for (int t = 0; t < F::N; t++) {
    q.x.l[t] = o[t * SLOTS];
    q.y.l[t] = o[(F::N + t) * SLOTS];
    q.zz.l[t] = o[(2 * F::N + t) * SLOTS];
    q.zzz.l[t] = o[(3 * F::N + t) * SLOTS];
  }
  acc = ed_add<F>(acc, q);
}

// the parent's delta: dfr[k] = fr[k] - base_fr[k] for the maps of the new and the old commitment (base_fr null: the old one is the
// neutral, whose map is 0).  One lane per row; dfr may be fr itself.
struct VkDeltaArgs {
  const uint32_t* fr;        // [m][8] map of the new commitments, Montgomery
  const uint32_t* base_fr;   // [m][8] map of the old ones, or null
  uint32_t m;
  uint32_t* dfr;             // [m][8]
};
template <class Fr>
CTT_HD void vk_delta_body(const VkDeltaArgs& a, uint32_t lane) {
  if (lane >= a.m) return;
  Fr v = vk_load<Fr>(a.fr + (uint64_t)lane * 8u);
  if (a.base_fr) v = Fr::sub(v, vk_load<Fr>(a.base_fr + (uint64_t)lane * 8u));
  vk_store<Fr>(a.dfr + (uint64_t)lane * 8u, v);
}

// ---------------------------------------------------------------------------------------------
// finish: lane l owns the points [l * K, (l + 1) * K)
// ---------------------------------------------------------------------------------------------
struct VkFinishArgs {
  const uint32_t* src;   // [m] points (X, Y, Z, ...), src_stride words each; any Z
  uint32_t src_stride;
  uint32_t m, K;
  uint32_t* out_prj;     // [m][24] (x, y, 1) Montgomery, or null
  uint32_t* out_ser;     // [m][8]  32 bytes big-endian: x if y >= (p-1)/2 else p - x, or null
  uint32_t* out_fr;      // [m][8]  ((x / y) mod p) mod r as a Montgomery residue of the scalar field, or null
};

// y >= (p - 1) / 2 for a canonical (non-Montgomery) y; p is odd, so (p - 1) / 2 = p >> 1
template <class F>
CTT_HD bool vk_lexicographically_largest(const F& y) {
  using PP = typename F::Params;
  bool ge = true;   // equal so far
#pragma unroll
  for (int k = 0; k < F::N; k++) {   // from the low word up: the highest differing word decides
    const uint32_t h = (PP::P[k] >> 1) | (k + 1 < F::N ? PP::P[k + 1] << 31 : 0u);
    if (y.l[k] != h) ge = y.l[k] > h;
  }
  return ge;
}

// The inverted quantity is Y*Z; a zero factor is left out of it (inv(0) = 0, the reference's convention), so a zero Z gives the point
// (0, 0, 1) and 32 zero bytes but still X / Y, a zero Y gives the scalar 0, and the neighbours of such a point are not affected.  The
// running products are parked in the first requested output until the backward sweep overwrites them.
template <class F, class Fr>
CTT_HD void vk_finish_body(const VkFinishArgs& a, uint32_t lane) {
  const uint64_t i0 = (uint64_t)lane * a.K;
  if (i0 >= a.m) return;
  const uint64_t i1 = i0 + a.K < a.m ? i0 + a.K : a.m;
  uint32_t* park = a.out_fr ? a.out_fr : a.out_ser ? a.out_ser : a.out_prj;
  const uint32_t park_stride = (a.out_fr || a.out_ser) ? 8u : 24u;
  F run = F::one();
  for (uint64_t i = i0; i < i1; i++) {
    const uint32_t* p = a.src + i * a.src_stride;
    const F Y = vk_load<F>(p + F::N), Z = vk_load<F>(p + 2 * F::N);
    vk_store<F>(park + i * park_stride, run);
    if (!Y.is_zero()) run = F::mul(run, Y);
    if (!Z.is_zero()) run = F::mul(run, Z);
  }
  F inv = F::inv(run);
  for (uint64_t i = i1; i-- > i0;) {
    const uint32_t* p = a.src + i * a.src_stride;
    const F X = vk_load<F>(p), Y = vk_load<F>(p + F::N), Z = vk_load<F>(p + 2 * F::N);
    const bool y0 = Y.is_zero(), z0 = Z.is_zero();
    const F den_inv = F::mul(inv, vk_load<F>(park + i * park_stride));   // 1 / (the non-zero ones of Y, Z)
    if (!y0) inv = F::mul(inv, Y);
    if (!z0) inv = F::mul(inv, Z);
    const F iz = z0 ? F::zero() : y0 ? den_inv : F::mul(den_inv, Y);
    const F iy = y0 ? F::zero() : z0 ? den_inv : F::mul(den_inv, Z);
    if (a.out_prj || a.out_ser) {
      const F x = F::mul(X, iz), y = F::mul(Y, iz);
      if (a.out_prj) {
        uint32_t* o = a.out_prj + i * 24u;
        vk_store<F>(o, x);
        vk_store<F>(o + F::N, y);
        vk_store<F>(o + 2 * F::N, F::one());
      }
      if (a.out_ser) {
        const F xs = F::from_mont(vk_lexicographically_largest<F>(F::from_mont(y)) ? x : F::neg(x));
        uint32_t* o = a.out_ser + i * 8u;
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = __builtin_bswap32(xs.l[7 - k]);
      }
    }
    if (a.out_fr) {
      const F v = F::from_mont(F::mul(X, iy));   // canonical, below p: up to four times r and more
      Fr s;
#pragma unroll
      for (int k = 0; k < 8; k++) s.l[k] = v.l[k];
      vk_store<Fr>(a.out_fr + i * 8u, Fr::to_mont(s));   // one Montgomery product with R^2 mod r: below 2r before its last subtraction
    }
  }
}

}  // namespace ctt
