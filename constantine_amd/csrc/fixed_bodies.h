// fixed_bodies.h -- per-lane bodies of the batched fixed-base MSM over a short-Weierstrass G1 (BLS12-381, BN254): m MSMs over one
// fixed set of n <= 2^16 points in one pass, without the pipeline's sort, buckets, reduction passes or tickets.
// The shape is that of the Verkle commitment (verkle_bodies.h), the group law that of ec.h's XYZZ formulas over the canonical Fp:
//
//   table    for base i, window w of the balanced layout (msm_bodies.h window_layout) and j = 1 .. 2^(width(w)-1) the record (x, y) of
//            j * 2^off(w) * P_i, affine Montgomery, 2 * F::N words.  -(x, y) = (x, -y); the neutral is (0, 0), and so is every record
//            of a neutral base.  All records of a base are consecutive, window after window: record index = i * rows + vk_row_off(w)
//            + j - 1.  FxTable is the view every kernel's arguments hold and the one place a record's address is computed.
//   sum      a lane owns one base of one row: it walks the Booth digits of its scalar (booth_recode_packed) and adds one record per
//            non-zero digit (xyzz_madd: empty accumulator, P = Q and P = -Q are its own cases).
//   tree     the 256 lanes of a workgroup are summed pairwise through 128 slots of LDS (vk_tree_put, fx_tree_take); the workgroup's
//            sum is the partial of (row, chunk of 256 bases).
//   finish   one wavefront per row sums the row's partials and runs the tree over its 64 lanes; the rows of a workgroup become affine
//            with one inversion (Montgomery's trick over ZZ * ZZZ), the neutral (0, 0).
//
// Bodies are __host__ __device__ like those of msm_bodies.h: tests/fixed_harness.cpp runs them lane by lane on the CPU.
#pragma once
#include "verkle_bodies.h"

namespace ctt {

static constexpr uint32_t FX_BLOCK = 256;            // lanes of an MSM workgroup = bases of a chunk
static constexpr uint32_t FX_TREE_SLOTS = FX_BLOCK / 2;
static constexpr uint32_t FX_MAX_BASES = 65536;      // at most 256 partials per row: one pass of the finish
static constexpr uint32_t FX_WAVE = 64;              // lanes per row of the finish
static constexpr uint32_t FX_FINISH_ROWS = 4;        // rows per workgroup of the finish = rows per inversion
static constexpr uint32_t FX_FINISH_SLOTS = FX_WAVE / 2;
static constexpr int FX_MIN_WINDOW_BITS = 2, FX_MAX_WINDOW_BITS = 12;

// The table as its users see it: rec_at(i, vk_row_off(lay, w), j) is the record of (j + 1) * 2^off(w) * P_i.
struct FxTable {
  uint32_t* tab;    // [n][rows] records
  uint32_t n, W;
  WinLayout lay;
  uint32_t rows;    // records per base = vk_row_off(lay, W)
  uint32_t stride;  // words per record = 2 * F::N
  CTT_HD uint32_t* rec_at(uint32_t i, uint32_t row_off, uint32_t j) const { return tab + ((uint64_t)i * rows + row_off + j) * stride; }
};

template <class F>
CTT_HD XYZZ<F> fx_load_xyzz(const uint32_t* p) {
  return {vk_load<F>(p), vk_load<F>(p + F::N), vk_load<F>(p + 2 * F::N), vk_load<F>(p + 3 * F::N)};
}
template <class F>
CTT_HD void fx_store_xyzz(uint32_t* p, const XYZZ<F>& v) {
  vk_store<F>(p, v.x);
  vk_store<F>(p + F::N, v.y);
  vk_store<F>(p + 2 * F::N, v.zz);
  vk_store<F>(p + 3 * F::N, v.zzz);
}

// ---------------------------------------------------------------------------------------------
// table: one lane per (base, window)
// ---------------------------------------------------------------------------------------------
struct FxTableArgs : FxTable {
  const uint32_t* pts;   // [n] affine points, C-API layout (x, y Montgomery); (0, 0) is the neutral
  uint32_t* pre;         // [n][rows][3 * F::N]: ZZ, ZZZ and the prefix product of every record while the lane's records are normalised
};

// 2^off(w) * P_i by doublings, its multiples by a running sum in XYZZ whose X, Y are parked in the records themselves, then one
// inversion for all ZZ * ZZZ of the lane.  A neutral sum (a neutral base) is left out of the product and becomes (0, 0).
template <class F>
CTT_HD void fx_table_body(const FxTableArgs& a, uint32_t lane) {
  if (lane >= a.n * a.W) return;
  const uint32_t i = lane % a.n, w = lane / a.n;
  const uint32_t* p = a.pts + (uint64_t)i * 2 * F::N;
  XYZZ<F> q = XYZZ<F>::from_affine(Affine<F>{vk_load<F>(p), vk_load<F>(p + F::N)});
  for (int b = a.lay.off(w); b > 0; b--) q = xyzz_dbl<F>(q);
  const uint32_t half = 1u << (a.lay.width(w) - 1);
  const uint32_t row = vk_row_off(a.lay, w);
  const uint64_t e0 = (uint64_t)i * a.rows + row;   // the lane's first record
  XYZZ<F> r = XYZZ<F>::inf();
  F run = F::one();
  for (uint32_t j = 0; j < half; j++) {
    r = xyzz_add_inl<F>(r, q);
    uint32_t* rec = a.rec_at(i, row, j);
    uint32_t* pre = a.pre + (e0 + j) * (3 * F::N);
    vk_store<F>(rec, r.x);
    vk_store<F>(rec + F::N, r.y);
    vk_store<F>(pre, r.zz);
    vk_store<F>(pre + F::N, r.zzz);
    vk_store<F>(pre + 2 * F::N, run);
    if (!r.zz.is_zero()) run = F::mul(run, F::mul(r.zz, r.zzz));
  }
  F inv = F::inv(run);
  for (uint32_t j = half; j-- > 0;) {
    uint32_t* rec = a.rec_at(i, row, j);
    const uint32_t* pre = a.pre + (e0 + j) * (3 * F::N);
    const F ZZ = vk_load<F>(pre), ZZZ = vk_load<F>(pre + F::N);
    F x = F::zero(), y = F::zero();
    if (!ZZ.is_zero()) {
      const F zi = F::mul(inv, vk_load<F>(pre + 2 * F::N));   // 1 / (ZZ * ZZZ)
      inv = F::mul(inv, F::mul(ZZ, ZZZ));
      x = F::mul(vk_load<F>(rec), F::mul(zi, ZZZ));
      y = F::mul(vk_load<F>(rec + F::N), F::mul(zi, ZZ));
    }
    vk_store<F>(rec, x);
    vk_store<F>(rec + F::N, y);
  }
}

// ---------------------------------------------------------------------------------------------
// sum: the lane of base i of row k
// ---------------------------------------------------------------------------------------------
struct FxMsmArgs : FxTable {
  const uint32_t* coefs;   // [m][n][8] canonical little-endian scalars below 2^BITS (not reduced mod r), or Montgomery residues (fr)
  uint32_t m;
  int fr;                  // 1: Montgomery residues of the scalar field, converted here
  uint32_t chunks;         // ceil(n / FX_BLOCK)
  uint32_t* part;          // [m][chunks] XYZZ partials, 4 * F::N words each
};

// a[k][i] * P_i.  The scalar is shifted down window by window, so its words are only ever addressed with compile-time indices and the
// addition exists once in the code; the digit of a window is (its bits << 1 | the bit below) recoded by booth_recode_packed.
template <class F, class Fr>
CTT_HD XYZZ<F> fx_lane_sum(const FxMsmArgs& a, uint32_t k, uint32_t i) {
  XYZZ<F> acc = XYZZ<F>::inf();
  if (i >= a.n) return acc;
  uint32_t s[8];
  {
    Fr v = vk_load<Fr>(a.coefs + ((uint64_t)k * a.n + i) * 8);
    if (a.fr) v = Fr::from_mont(v);
#pragma unroll
    for (int t = 0; t < 8; t++) s[t] = v.l[t];
  }
  uint32_t below = 0, row = 0;
  for (uint32_t w = 0; w < a.W; w++) {
    const uint32_t c = (uint32_t)a.lay.width(w), vmask = (1u << c) - 1u;
    const uint32_t d = ((s[0] & vmask) << 1) | below;
    below = (s[0] >> (c - 1)) & 1u;
#pragma unroll
    for (int t = 0; t < 7; t++) s[t] = (s[t] >> c) | (s[t + 1] << (32u - c));
    s[7] >>= c;
    const uint32_t dg = booth_recode_packed(d, c);
    if (dg != DIGIT_NONE) {
      const uint32_t* rec = a.rec_at(i, row, dg >> 1);
      xyzz_madd<F>(acc, Affine<F>{vk_load<F>(rec), vk_load<F>(rec + F::N)}, (dg & 1u) != 0);
    }
    row += 1u << (c - 1);
  }
  return acc;
}

// ---------------------------------------------------------------------------------------------
// tree: vk_tree_put hands a lane's point to a slot as it is (any XYZZ<F>); taking it is the short-Weierstrass addition.  Equal
// points take xyzz_add's doubling branch, opposite ones give the neutral, and the in-memory neutral (all zero) passes through.
// ---------------------------------------------------------------------------------------------
template <class F, uint32_t SLOTS>
CTT_HD void fx_tree_take(const uint32_t* slots, uint32_t lane, uint32_t s, XYZZ<F>& acc) {
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
  acc = xyzz_add_inl<F>(acc, q);
}

// ---------------------------------------------------------------------------------------------
// finish: lane l of the wavefront of row k adds up the partials l, l + 64, ... of the row (at most four); after the wave's tree its
// lane 0 parks the row's sum in `grp`, and one lane turns the parked sums of a workgroup into affine points.
// ---------------------------------------------------------------------------------------------
struct FxFinishArgs {
  const uint32_t* part;   // [m][chunks] XYZZ partials
  uint32_t m, chunks;
  uint32_t* out;          // [m] affine (x, y) Montgomery, 2 * F::N words each; the neutral is (0, 0)
};

template <class F>
CTT_HD XYZZ<F> fx_finish_lane_sum(const FxFinishArgs& a, uint32_t k, uint32_t l) {
  XYZZ<F> acc = XYZZ<F>::inf();
  if (k >= a.m) return acc;
  for (uint32_t s = l; s < a.chunks; s += FX_WAVE)
    acc = xyzz_add_inl<F>(acc, fx_load_xyzz<F>(a.part + ((uint64_t)k * a.chunks + s) * (4 * F::N)));
  return acc;
}

// grp: cnt points of 4 * F::N words, pre: cnt elements of F::N words (LDS on the device); row k0 + g goes to out
template <class F>
CTT_HD void fx_finish_group(const FxFinishArgs& a, uint32_t k0, uint32_t cnt, const uint32_t* grp, uint32_t* pre) {
  F run = F::one();
  for (uint32_t g = 0; g < cnt; g++) {
    const uint32_t* p = grp + g * (4 * F::N);
    const F ZZ = vk_load<F>(p + 2 * F::N), ZZZ = vk_load<F>(p + 3 * F::N);
    vk_store<F>(pre + g * F::N, run);
    if (!ZZ.is_zero()) run = F::mul(run, F::mul(ZZ, ZZZ));
  }
  F inv = F::inv(run);
  for (uint32_t g = cnt; g-- > 0;) {
    const uint32_t* p = grp + g * (4 * F::N);
    const F ZZ = vk_load<F>(p + 2 * F::N), ZZZ = vk_load<F>(p + 3 * F::N);
    F x = F::zero(), y = F::zero();
    if (!ZZ.is_zero()) {
      const F zi = F::mul(inv, vk_load<F>(pre + g * F::N));   // 1 / (ZZ * ZZZ)
      inv = F::mul(inv, F::mul(ZZ, ZZZ));
      x = F::mul(vk_load<F>(p), F::mul(zi, ZZZ));
      y = F::mul(vk_load<F>(p + F::N), F::mul(zi, ZZ));
    }
    uint32_t* o = a.out + (uint64_t)(k0 + g) * (2 * F::N);
    vk_store<F>(o, x);
    vk_store<F>(o + F::N, y);
  }
}

}  // namespace ctt
