// msm_pipeline.h -- host orchestration of one MSM over a Backend (HIP on the GPU; a CPU emulator in
// tests/emu that executes the same per-thread bodies).  See msm_bodies.h for the stage list.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include "host_fp64.h"
#include "msm_bodies.h"
#include "msm_place.h"
#include "msm_plan.h"

namespace ctt {

// thrown by a backend's alloc() when the device is out of memory: the engine releases what it holds for the call and the
// C ABI turns it into the call's error value (NULL / -1) where there is one (round 2 aborted the process)
struct OutOfDeviceMemory { size_t bytes; };

// Every sizing field of the sort's arguments from a plan (the pointers and the bucket region to clear are the caller's).
static inline void sort_sizing(SortArgs& sa, const MsmPlan& p, const MsmOptions& o) {
  sa.n = p.n; sa.c = p.c; sa.lay = p.lay; sa.W = (uint32_t)p.W; sa.B = p.B;
  sa.Wd = (uint32_t)p.Wd; sa.merged = p.merged; sa.nent = p.nent; sa.id_stride = p.id_stride;
  sa.NG = p.NG; sa.gshift = p.gshift; sa.gshift_narrow = p.gshift_narrow; sa.slice = p.slice; sa.nblk = p.S;
  sa.jbits = p.jbits;
  sa.cap = p.cap; sa.big = p.big;
  sa.kwords = p.glv ? 4u : 8u;
  sa.xcd_map = o.sort_xcd ? 1u : 0u;
  sa.staged = (o.sort_staged >= 2 || (o.sort_staged == 1 && p.NG >= 256u)) ? 1u : 0u;
}
// Bytes of the sort's six arrays (SortArgs has their shapes)
struct SortBytes { size_t part, cntA, gtot, gbase, bstart, entries; };
static inline SortBytes sort_bytes(const SortArgs& sa) {
  const size_t W = sa.W;
  return SortBytes{W * sa.nent * (sa.merged ? 8 : 4), (size_t)sa.nblk * W * sa.NG * 4, W * sa.NG * 4, W * (sa.NG + 1) * 4, W * (sa.B + 1) * 4, W * sa.nent * 4};
}

// Window combine (ec_multi_scalar_mul.nim:250-254; _parallel.nim:199-203), in two parts.
// On the device, fused into the second launch of the bucket reduction: per window the reduction leaves O_0..O_{c-2} (sum of
// the buckets whose index has bit l set) and TOP (sum of all buckets); the window sum is S_w = sum_l 2^l O_l + TOP.  The
// bits are cut into groups of h: P_{w,g} = sum_{l in group g} 2^(l - g*h) O_l (+ TOP in group 0), one quad of lanes per group
// (window_group_sum_body is what a quad computes) -- a chain of h-1 doublings instead of c-2.  On the host: the Horner over
// the windows, result = sum_w 2^(c*w) sum_g 2^(g*h) P_{w,g}: its W*c doublings are one dependent chain whatever h is (0.25 us
// per doubling on a CPU core against 5 us for four GPU lanes), the groups only add ngrp - 1 additions per window to it.
template <class F>
CTT_HD XYZZ<F> window_group_sum_body(const XYZZ<F>* ow, int c, int h, int g) {
  const int lo = g * h;
  int hi = lo + h;
  if (hi > c - 1) hi = c - 1;
  XYZZ<F> r = XYZZ<F>::inf();
  for (int l = hi - 1; l >= lo; l--) {
    r = xyzz_dbl<F>(r);
    xyzz_add<F>(r, ow[l]);
  }
  if (g == 0) xyzz_add<F>(r, ow[c - 1]);
  return r;
}
template <class F>
static inline XYZZ<F> combine_groups(const XYZZ<F>* s, int W, const WinLayout& L, int h, int ngrp) {
  XYZZ<F> r = XYZZ<F>::inf();
  for (int w = W - 1; w >= 0; w--) {
    // window w+1 starts width(w) bits above window w: those doublings are spread over the groups of window w
    const int cw = L.width((uint32_t)w);
    for (int g = ngrp - 1; g >= 0; g--) {
      const int nd = g == ngrp - 1 ? cw - g * h : h;
      for (int l = 0; l < nd; l++) r = xyzz_dbl<F>(r);
      xyzz_add<F>(r, s[(size_t)w * ngrp + g]);
    }
  }
  return r;
}

// Stage indices for timings
enum { ST_DIGITS = 0, ST_SORT, ST_ACCUM, ST_MERGE, ST_REDUCE, ST_TOTAL, ST_COUNT };

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#endif
}

template <class BK, class = void> struct HasGlvFront : std::false_type {};
template <class BK> struct HasGlvFront<BK, std::void_t<decltype(BK::GLV_FRONT)>> : std::true_type {};

template <class C, class BK>
struct MsmEngine {
  using F = typename C::F;    // reference representation (C API)
  using FD = typename C::FD;  // device representation
  static constexpr bool kConvert = !std::is_same<F, FD>::value;
  // the endomorphism split exists for this curve (msm_bodies.h GlvOf) and the backend has its front kernel (launch_glv_front; a backend says so
  // with a member GLV_FRONT -- one without it runs every MSM on the plain path)
  static constexpr bool kGlv = GlvOf<C>::HAS && kConvert && HasGlvFront<BK>::value;
  BK& bk;
  MsmOptions opt;
  MsmPlan last_plan;

  // grow-only workspace
  struct Buf { void* p = nullptr; size_t cap = 0; };
  // In-flight slots.  Rounds 1-5 had two; round 6 read the timeline of a pipelined 2^16-pair loop (profiles/cu_mask_r06.txt): with two
  // slots, submit(i+2) has to follow finish(i) -- the wait for MSM i's result copy, then its host tail (~0.1-0.2 ms: W c doublings on one
  // core), then the enqueueing of ~24 launches -- and the main stream idles ~90 us of every 450 us step because MSM i+2's first kernel
  // has not been enqueued yet when MSM i+1's main-stream chain ends.  With a third slot a caller submits MSM i+2 BEFORE it finishes MSM i.
  static constexpr int NSLOT = 3;
  // bstartS / maxcountS / bucketsS: one per in-flight slot -- the head merge and the first reduction pass of MSM i read them on the tail
  // stream while the sort of MSM i+1 already writes its own (submit(): early tail)
  Buf part, counts, bstartS[NSLOT], entries, bucketsS[NSLOT], heads, tails, hkey, tkey, rA[2], rP[2], scal, half, maxcountS[NSLOT], cpoints, totals, gbase, mqueue;

  explicit MsmEngine(BK& b) : bk(b) {}
  ~MsmEngine() {
    Buf* all[] = {&part, &gbase, &counts, &entries, &heads, &tails, &hkey, &tkey, &rA[0], &rA[1], &rP[0], &rP[1], &scal, &half, &cpoints, &totals, &mqueue};
    for (int i = 0; i < NSLOT; i++) {
      bk.free_quiet(bstartS[i].p);
      bk.free_quiet(bucketsS[i].p);
      bk.free_quiet(maxcountS[i].p);
    }
    // (a destructor is noexcept: the quiet forms -- ctt_hip_msm_ctx_destroy of a context lost to a HIP failure comes through here)
    for (Buf* b : all) if (b->p) bk.free_quiet(b->p);
    for (Slot& sl : slots) if (sl.hraw) bk.free_host_quiet(sl.hraw);
  }
  void* need(Buf& b, size_t bytes) {
    if (bytes > b.cap) {
      void* old = b.p;
      b.p = nullptr;      // (before the free: if it throws, the destructor must not free the pointer a second time)
      b.cap = 0;
      if (old) bk.free(old);
      size_t cap = bytes + bytes / 8 + 256;
      b.p = bk.alloc(cap);   // may throw OutOfDeviceMemory: the buffer is then simply empty
      b.cap = cap;
    }
    return b.p;
  }

  // Up to NSLOT MSMs may be in flight: submit() enqueues every kernel of one MSM plus the asynchronous copy of its
  // c points per window into a pinned host buffer; finish() waits for that copy and runs the host tail.
  // Calling submit(i+1) before finish(i) overlaps the host tail of MSM i with the GPU work of MSM i+1
  // (the workspace is shared: stream order keeps the two apart on the device).
  using HF = typename HostField<FD>::type;
  struct Slot {
    MsmPlan plan;
    bool busy = false;
    bool empty = false;   // len == 0
    void* hraw = nullptr; // pinned host buffer for the device output
    size_t hcap = 0;
  };
  Slot slots[NSLOT];
  int next_slot = 0;
  int busy_count() const {
    int k = 0;
    for (const Slot& s : slots) k += s.busy ? 1 : 0;
    return k;
  }
  // another MSM is in flight beside slot sl's: the caller is pipelining
  bool other_busy(int sl) const {
    for (int i = 0; i < NSLOT; i++) if (i != sl && slots[i].busy) return true;
    return false;
  }

  // d_coefs: canonical scalars [n][8] (coef_is_fr = false) or Montgomery Fr elements (true), device memory.
  // d_points: affine Montgomery points (reference representation), device memory.  Returns the slot.
  // Converted point records for base points that are reused across MSMs (the ZAL "base descriptor",
  // constantine-halo2-zal/src/lib.rs:68-71): returns a device buffer owned by the caller (free with bk.free).
  void* prepare_bases(const Affine<F>* d_points_in, uint32_t n) {
    if (n == 0) return nullptr;
    void* cp = bk.alloc((size_t)n * record_stride());
    make_records(d_points_in, cp, n);
    return cp;
  }
  // Bytes of one point record as the accumulate kernel reads it: the converted form, or the caller's points themselves
  static constexpr uint32_t record_stride() { return kConvert ? gather_stride<FD>() : (uint32_t)sizeof(Affine<F>); }
  // n records at `out` from the caller's points: converted, or copied
  void make_records(const Affine<F>* d_points_in, void* out, uint32_t n) {
    if constexpr (kConvert) bk.template launch_convert<F, FD>(d_points_in, out, n);
    else bk.d2d_async(out, d_points_in, (size_t)n * sizeof(Affine<F>));
  }
  // The points of the accumulate kernel (record_stride() bytes each): cached records, the records converted into d_converted
  // (convert: enqueue that conversion here), or the caller's points where the device reads them as they are
  const void* accum_points(const Affine<F>* d_points_in, const void* d_prepared, void* d_converted, uint32_t n, bool convert) {
    if (d_prepared) return d_prepared;
    if constexpr (kConvert) {
      if (convert) bk.template launch_convert<F, FD>(d_points_in, d_converted, n);
      return d_converted;
    } else {
      return d_points_in;
    }
  }

  // Window table over bases that are reused across MSMs (an SRS, a commitment key): T[w][j] = 2^(c*w) * P_j for the
  // Wd = bits/c + 1 digit windows, as converted point records.  With it every Booth digit of every window is a signed
  // multiple of a TABLE row, all windows share one bucket set, and the doublings of the window combine disappear: an MSM
  // is (bits/c + 1)*N accumulations and ONE bucket reduction over 2^(c-1) buckets -- so c is larger than without the
  // table (20 instead of 16 at N = 2^20: 13 instead of 16 accumulations per pair).  The price is memory, Wd times the
  // point records (1.7 GB for 2^20 BLS12-381 G1 bases: this is what 288 GB of HBM is for), and c*(Wd-1) doublings plus
  // Wd-1 inversions per base when the table is built.  The reference has no such table; its nearest relative is the ZAL
  // base descriptor (constantine-halo2-zal/src/lib.rs:68-95), which upstream passes through unchanged.
  // Returns the records (caller-owned, free with bk.free); c = 0 chooses the window bits.  *c_out = the bits used.
  void* prepare_table(const Affine<F>* d_points_in, uint32_t n, int c, int* c_out) {
    // c above what choose_table_window_bits searches (22: 2^21 buckets, 16384 bucket groups of the sort) is not a plan the
    // sort can run, c < 2 is no window at all: take the automatic choice instead
    if (c < 2 || c > 22 || !table_plan_fits(n, C::BITS, c)) c = choose_table_window_bits(n, C::BITS);
    *c_out = c;
    if (n == 0 || c == 0) return nullptr;
    int Wd;
    const WinLayout lay = window_layout(C::BITS, c, &Wd);
    const size_t stride = record_stride();
    char* tab = nullptr;
    Affine<F>* lvl[2] = {nullptr, nullptr};
    try {
      tab = (char*)bk.alloc((size_t)Wd * n * stride);
      lvl[0] = (Affine<F>*)bk.alloc((size_t)n * sizeof(Affine<F>));
      lvl[1] = (Affine<F>*)bk.alloc((size_t)n * sizeof(Affine<F>));
    } catch (const OutOfDeviceMemory&) {
      // (bits/c + 1) x the records did not fit: no table, the caller keeps plain records (c_out = 0)
      if (tab) bk.free(tab);
      if (lvl[0]) bk.free(lvl[0]);
      *c_out = 0;
      return nullptr;
    }
    const Affine<F>* cur = d_points_in;
    for (int w = 0; w < Wd; w++) {
      if (w > 0) {
        Affine<F>* nxt = lvl[w & 1];
        bk.template launch_table_next<F>(cur, nxt, n, lay.width((uint32_t)w - 1));   // level w = 2^width(w-1) x level w-1
        cur = nxt;
      }
      make_records(cur, tab + (size_t)w * n * stride, n);
    }
    bk.sync();
    bk.free(lvl[0]);
    bk.free(lvl[1]);
    return tab;
  }

  // ---- the stages of one MSM ---------------------------------------------------------------------------------------
  // Stage 1 (per MSM, or per chunk of a host-pointer MSM): scalars -> Booth digits -> entries sorted by bucket ->
  // bucket sums of these pairs in `d_buckets` (heads/tails of the runs that straddle lane ranges still to be merged).
  // Ends with the accumulate kernel enqueued.
  struct Staged {
    uint32_t* d_bstart;
    uint32_t* d_maxcount;
    XYZZ<FD>* d_buckets;
    XYZZ<FD>* d_heads;
    XYZZ<FD>* d_tails;
    uint32_t* d_hkey;
    uint32_t* d_tkey;
    uint32_t* d_mqueue;   // the queue form of the head merge (plan.merge_lmax > 0) only
    uint32_t* d_half;     // the endomorphism split (plan.glv) only: the half scalars [n][4] the sort reads
  };
  // The workspace of stage 1 and the head merge for plan p in slot sl: every buffer and its size, once.  `sa` gets the sort's sizing
  // and its arrays, `st` what the accumulation and the merge share; returns the canonical scalars' buffer (coef_is_fr only).
  uint32_t* stage1_workspace(int sl, const MsmPlan& p, bool coef_is_fr, SortArgs& sa, Staged& st) {
    sort_sizing(sa, p, opt);
    const SortBytes sb = sort_bytes(sa);
    const size_t lanes = (size_t)p.W * p.G;
    uint32_t* d_scal = coef_is_fr ? (uint32_t*)need(scal, (size_t)p.pairs() * 32) : nullptr;
    st.d_half = p.glv ? (uint32_t*)need(half, (size_t)p.n * 16) : nullptr;
    sa.part = (uint32_t*)need(part, sb.part);
    sa.cntA = (uint32_t*)need(counts, sb.cntA);
    sa.gtot = (uint32_t*)need(totals, sb.gtot);
    sa.gbase = (uint32_t*)need(gbase, sb.gbase);
    sa.bstart = st.d_bstart = (uint32_t*)need(bstartS[sl], sb.bstart);
    sa.entries = (uint32_t*)need(entries, sb.entries);
    // (d_maxcount: [0] the largest bucket, [2] the head merge's queue count -- zeroed by the sort's first kernel: no fill launch)
    sa.maxcount = st.d_maxcount = (uint32_t*)need(maxcountS[sl], 256);
    st.d_heads = (XYZZ<FD>*)need(heads, lanes * sizeof(XYZZ<FD>));
    st.d_tails = (XYZZ<FD>*)need(tails, lanes * sizeof(XYZZ<FD>));
    st.d_hkey = (uint32_t*)need(hkey, lanes * 4);
    st.d_tkey = (uint32_t*)need(tkey, lanes * 4);
    st.d_mqueue = p.merge_lmax > 0 ? (uint32_t*)need(mqueue, (size_t)merge_queue_capacity(p.W, p.G) * 4) : nullptr;
    return d_scal;
  }
  // the grow-only workspace sized for plan p up front (need() frees and reallocates -- a device-wide
  // synchronisation -- when a later, larger slice of a host-pointer MSM asks for more)
  void reserve_stage1(int sl, const MsmPlan& p, bool coef_is_fr) {
    SortArgs sa;
    Staged st;
    (void)stage1_workspace(sl, p, coef_is_fr, sa, st);
  }
  // points_arrive (submit_host, a slice copied by the submitting thread): the points of this slice are not on the device yet -- the
  // digits and the sort need the coefficients only, so they are enqueued first, the hook then copies the points (the thread sits in that
  // copy while the GPU sorts) and the conversion follows the sort instead of preceding it.
  // pl.front_side (small MSMs kept in flight): conversion, digits and sort on the backend's front stream, beside the previous MSM's
  // head merge and first reduction pass (HipBackend::front_begin has the ordering argument)
  Staged accumulate_pairs(int sl, const MsmPlan& p, const Placement& pl, const uint32_t* d_coefs, bool coef_is_fr, const Affine<F>* d_points_in,
                          const void* d_prepared, void* d_converted, XYZZ<FD>* d_buckets, bool into = false,
                          const std::function<void()>* points_arrive = nullptr) {
    const uint32_t n = p.n, W = p.W, B = p.B;
    SortArgs sa;
    Staged st;
    uint32_t* d_scal = stage1_workspace(sl, p, coef_is_fr, sa, st);
    if (pl.front_side) bk.front_begin();
    bk.stage_begin(sl, ST_DIGITS);
    sa.scalars = d_coefs;
    if (coef_is_fr) {
      bk.template launch_fr_from_mont<typename C::Fr>(d_coefs, d_scal, p.pairs());
      sa.scalars = d_scal;
    }
    const bool convert_late = points_arrive != nullptr;
    const void* d_points = nullptr;
    bool split = false;
    if constexpr (kGlv) {
      if (p.glv) {
        // The endomorphism split: ONE front kernel in place of the conversion reads the canonical scalar and the point of every pair and writes
        // the records of s1 P (record j) and s2 phi(P) (record n/2 + j) and the two half scalars; digits and sort then run on 4-word scalars,
        // and everything downstream on a plan of n entries whose windows cover 128 bits (submit(): device-resident inputs only).
        bk.template launch_glv_front<F, FD>(sa.scalars, d_points_in, d_converted, st.d_half, p.pairs());
        sa.scalars = st.d_half;
        d_points = d_converted;
        split = true;
      }
    }
    if (!split) d_points = accum_points(d_points_in, d_prepared, d_converted, n, !convert_late);
    bk.stage_end(sl, ST_DIGITS);

    // Booth digits + sort by bucket (two passes: partition by bucket group, then sort each group inside LDS)
    bk.stage_begin(sl, ST_SORT);
    // the sort leaves the empty buckets of the set neutral (round 5; a fill launch of the whole set before).  Not for a later
    // slice of a host-pointer MSM (into): its runs continue the stored sums.  The set is this slot's: the previous MSM of the
    // slot read it in its first reduction pass, which the accumulation before this sort waited for.
    sa.zero_base = into ? nullptr : (void*)d_buckets;
    sa.zero_bytes = into ? 0u : (uint32_t)sizeof(XYZZ<FD>);
    bk.launch_digits_sort(sa);   // (leaves the largest bucket in d_maxcount[0]: the merge kernels read it there)
    if (convert_late) {
      (*points_arrive)();
      (void)accum_points(d_points_in, d_prepared, d_converted, n, true);   // (the conversion is timed with the sort in this form)
    }
    bk.stage_end(sl, ST_SORT);
    if (pl.front_side) bk.front_end();     // the accumulation below (main stream) waits for the sort

    // The previous MSM's tail has had this MSM's conversion and sort to run underneath; whether the accumulation waits for all of it or
    // only for its wide passes is the placement's (msm_place.h place_accum).
    // (the sort above has left this slot's bucket set with its empty buckets neutral -- SortArgs::zero_base -- and the previous MSM
    // runs on the other slot's set)
    // (into: a later slice of a host-pointer MSM continues the sums of the earlier slices, accum_body_xyzz)
    if (pl.wait_whole_tail) bk.tail_wait();
    bk.wide_wait();   // (nothing to wait for unless the previous reduction put wide passes on the tail stream)
    bk.stage_begin(sl, ST_ACCUM);
    st.d_buckets = d_buckets;
    AccumArgs<FD> aa{sa.entries, st.d_bstart, d_points, record_stride(), d_buckets, st.d_heads, st.d_tails, st.d_hkey, st.d_tkey, p.nent, B, p.K, p.G};
    aa.handover = pl.handover;
    bk.template launch_accum<FD>(aa, W, into);
    bk.accum_mark(pl.front_side);       // (what the next small MSM's front stage waits for: the shared entry list and records are free again)
    bk.stage_end(sl, ST_ACCUM);
    return st;
  }

  // Stage 2: partial sums of the buckets that straddle lane ranges.  A bucket of m entries spans at most floor((m-1)/K)+1
  // heads, the tree over such a chain takes log2 steps; with chains of length one -- the common case, no bucket larger than
  // K -- the tail merge writes the buckets itself.  The largest bucket is known on the DEVICE (the sort leaves it in
  // d_maxcount before the accumulation starts) and the kernels decide there: the host enqueues the steps an ordinary digit
  // distribution needs (MsmPlan::merge_steps) plus the finishing launch that covers everything else, and never waits
  // (rounds 1-2 read the word back in the middle of submit: a host round-trip per MSM, 0.1 ms of a 0.7 ms step at 2^16).
  void merge_buckets(int sl, const MsmPlan& p, const Staged& st) {
    bk.stage_begin(sl, ST_MERGE);
    MergeArgs<FD> ma{st.d_bstart, st.d_buckets, st.d_heads, st.d_tails, st.d_hkey, st.d_tkey, st.d_maxcount, p.B, p.K, p.G};
    if (p.merge_lmax > 0) {
      // queue form (round 5; msm_bodies.h merge_tail_queue_body): tail merge + queue of the chains with work left, one lane per
      // queued chain, and the long chains of unusual inputs by one workgroup per window
      ma.queue = st.d_mqueue;
      ma.qcount = st.d_maxcount + 2;     // (zeroed with the largest-bucket word before the sort)
      bk.template launch_merge_tail_queue<FD>(ma, p.W);
      bk.template launch_merge_queue<FD>(ma, p.W, p.merge_lmax, opt.merge_queue_quad != 2);
      bk.template launch_merge_long<FD>(ma, p.W, p.merge_lmax);
    } else {
      merge_tree(ma, p.W, p.merge_steps);
    }
    bk.stage_end(sl, ST_MERGE);
  }
  // the tree form: tail merge, at most max_steps wide steps while chains of more than d heads can exist, and the finishing launch for the rest
  void merge_tree(const MergeArgs<FD>& ma, uint32_t W, int max_steps) {
    bk.template launch_merge_tail<FD>(ma, W);
    uint32_t d = 1;
    for (int i = 0; i < max_steps && d < ma.G; i++, d <<= 1) bk.template launch_merge_step<FD>(ma, W, d);
    bk.template launch_merge_finish<FD>(ma, W, d);
  }

  // Stage 3: bucket reduction (c-1 pyramid passes, one launch each: every wave of a launch runs the same straight-line
  // addition at the same time, which is what keeps its 64 KiB of code flowing through the instruction caches), the bit Horner
  // in groups, and the copy of the W*ngrp partial sums to the slot's pinned buffer.
  // Round 3 measured the alternative the round-2 review asked for -- an aligned block of 256..1024 buckets taken through its
  // pyramid levels by ONE workgroup, workgroup barriers instead of launches, and one workgroup per window for the rest: two
  // launches instead of c-1.  Same box, BLS12-381 G1 2^20: 332 + 217 us against 315 + 75 (+ 45 us of Horner in both); 2^16:
  // 128 + 91 against 67 + 88.  A narrow pass is ~10 us of which ~7 us is the latency of one four-lane addition, which a fused
  // kernel pays as well, and a launch spreads every level over the whole chip where a workgroup has 256 lanes; the waves of a
  // fused kernel also drift apart (different passes, different task kinds) and each then streams the addition's code through
  // the instruction cache on its own.  profiles/reduce_fused_vs_passes_r03.txt; the code is in the history (a64cd06).
  void reduce_buckets(int sl, const MsmPlan& p, const Placement& pl, XYZZ<FD>* d_buckets) {
    Slot& S = slots[sl];
    const uint32_t W = p.W, B = p.B;
    if (!pl.early_tail()) bk.tail_wait();   // (a no-op unless accumulate_pairs left the previous tail running: small MSMs)
    bk.stage_begin(sl, ST_REDUCE);
    XYZZ<FD>* d_pyr = (XYZZ<FD>*)need(rA[0], (size_t)W * B * sizeof(XYZZ<FD>));
    XYZZ<FD>* d_q = (XYZZ<FD>*)need(rA[1], (size_t)W * (B / 2 + 1) * sizeof(XYZZ<FD>));
    XYZZ<FD>* d_out = (XYZZ<FD>*)need(rP[0], (size_t)W * p.c * sizeof(XYZZ<FD>));
    XYZZ<FD>* d_wsum = (XYZZ<FD>*)need(rP[1], (size_t)W * p.ngrp * sizeof(XYZZ<FD>));
    // The narrow passes at the end, the bit Horner and the result copy move to the backend's tail stream, the wide passes too where the placement
    // says so (msm_place.h place_reduction; the tail_wait() before the accumulation also orders the previous tail before this MSM's first write to
    // the pyramid buffers).
    bk.narrow_priority(pl.narrow_priority);
    for (int pass = 0; pass <= p.c - 1; pass++) {   // (pass c - 1: behind the last one)
      if (pass == pl.tail_from) bk.tail_begin();
      if (pass == pl.wide_mark_at) bk.wide_mark();
      if (pass == p.c - 1) break;
      PyrArgs<FD> pa{d_buckets, d_pyr, d_q, d_out, B, p.c, pass, 1u};
      bk.template launch_pyr<FD>(pa, W, pyr_pass_tasks(B, p.c, pass));
    }
    bk.template launch_window_groups<FD>(d_out, d_wsum, W, p.c, p.h, p.ngrp);
    bk.stage_end(sl, ST_REDUCE);

    const size_t bytes = (size_t)W * p.ngrp * sizeof(XYZZ<FD>);
    if (bytes > S.hcap) {
      if (S.hraw) bk.free_host(S.hraw);
      S.hraw = bk.alloc_host(bytes);
      S.hcap = bytes;
    }
    bk.d2h_async(sl, S.hraw, d_wsum, bytes);
    bk.stage_end(sl, ST_TOTAL);
    if (pl.tail_from != Placement::NEVER) bk.tail_end();
  }

  // what the placement decisions look at, for the MSM in slot sl (msm_place.h); the cost model's figures are the curve's
  PlaceInputs place_inputs(int sl, const void* d_prepared, int table_c) {
    opt.acc_ns = C::TUNE.acc_ns;
    opt.red_ns = C::TUNE.red_ns;
    return PlaceInputs{opt, C::TUNE, other_busy(sl), bk.partitioned(), d_prepared != nullptr, table_c};
  }

  int claim_slot(uint32_t n) {
    int sl = next_slot;
    for (int k = 0; k < NSLOT && slots[sl].busy; k++) sl = (sl + 1) % NSLOT;    // tickets may be finished in any order: take whichever slot is free
    Slot& S = slots[sl];
    if (S.busy) return -1;  // NSLOT MSMs in flight already: the caller finishes the oldest first (C ABI: error code)
    next_slot = (sl + 1) % NSLOT;
    S.busy = true;
    S.empty = (n == 0);  // len == 0 is UB upstream; we return the neutral
    return sl;
  }

  // One MSM on device-resident inputs.  d_prepared (optional): records made by prepare_bases for the same points; skips
  // the per-MSM conversion.  Returns the slot, or -1 when all slots are in flight.
  // d_prepared with table_c > 0: a window table built by prepare_table over table_n bases with table_c window bits.
  int submit(const uint32_t* d_coefs, bool coef_is_fr, const Affine<F>* d_points_in, uint32_t n,
             const void* d_prepared = nullptr, int table_c = 0, uint32_t table_n = 0) {
    const int sl = claim_slot(n);
    if (sl < 0 || n == 0) return sl;
    // where and when everything below runs: decided here, once (msm_place.h has the decisions and the measurements behind them)
    const PlaceInputs pin = place_inputs(sl, d_prepared, table_c);
    Placement pl = place_lanes(pin, n, C::BITS, GlvOf<C>::BITS, kGlv);
    const uint32_t pn = pl.glv ? 2u * n : n;                    // entries per bucket set and bits of a scalar the plan is made for
    MsmOptions po = opt;
    po.c = pl.c;
    po.lanes = pl.lanes;
    MsmPlan planned = table_c > 0 ? make_table_plan(n, C::BITS, table_c, table_n, po) : make_plan(pn, pl.glv ? GlvOf<C>::BITS : C::BITS, po);
    planned.glv = pl.glv ? 1u : 0u;
    const MsmPlan p = planned;
    slots[sl].plan = p;
    last_plan = p;
    place_accum(pl, pin, p, /*device_resident=*/true);
    place_reduction(pl, pin, p, /*may_start_early=*/true, [&](uint32_t ntasks, uint32_t W) { return bk.pyr_goes_to_tail(ntasks, W); });
    try {
      bk.stage_begin(sl, ST_TOTAL);
      void* d_converted = (kConvert && !d_prepared) ? need(cpoints, (size_t)pn * record_stride()) : nullptr;
      XYZZ<FD>* d_buckets = (XYZZ<FD>*)need(bucketsS[sl], (size_t)p.W * p.B * sizeof(XYZZ<FD>));
      const Staged st = accumulate_pairs(sl, p, pl, d_coefs, coef_is_fr, d_points_in, d_prepared, d_converted, d_buckets);
      if (pl.early_tail()) {
        // (the previous tail ended long ago: it ran beside this accumulation.  Partitioned chip: it may still be crawling through its
        // wide passes on its few compute units -- the tail stream is in order, and nothing on the main stream touches what it uses)
        if (!pin.partitioned) bk.tail_wait();
        bk.tail_begin();
      }
      merge_buckets(sl, p, st);
      if (pl.wide_mark_at == Placement::AT_MERGE) bk.merge_mark();
      reduce_buckets(sl, p, pl, d_buckets);
    } catch (const OutOfDeviceMemory&) {
      return release_slot(sl);
    }
    return sl;
  }
  // a submit that ran out of device memory: what it enqueued so far runs to its end on buffers that stay valid (a buffer is
  // only ever freed by need(), and hipFree waits for the device); the slot is free again.  Returns the error value -2.
  int release_slot(int sl) {
    bk.front_abort();       // (an exception between front_begin and front_end must not leave the next MSM's sort on the front stream: ADVICE r5)
    slots[sl].busy = false;
    next_slot = sl;
    return -2;
  }

  // One MSM on HOST-resident inputs (what the Constantine C symbols hand over), uploaded in `chunks` slices of pairs so
  // that the upload of slice i+1 runs underneath the accumulation of slice i: the copies go through the backend's copy
  // stream (a pageable hipMemcpyAsync occupies the calling thread but not the GPU's compute queues, and runs at PCIe
  // speed while k_accum holds every wave slot: profiles/h2d_overlap_r02.jsonl).  Every slice is sorted and accumulated
  // into its own bucket set (one owner per bucket per launch, no atomics); the sets are summed before the one bucket
  // reduction.  d_stage_coefs / d_stage_points: device staging for all n pairs (caller-owned).  Blocking on the copies,
  // asynchronous from the last accumulation on; returns the slot, or -1 when all slots are in flight.
  // The slices of a host-pointer call (msm_plan.h host_slices has the model) with this curve's figures: windows x the accumulate time per
  // pair on the GPU; 32 bytes of scalar and the point cross the link (scalars_only: the bases are cached on the device)
  static std::vector<uint32_t> host_slices(uint32_t n, int want, bool scalars_only = false) {
    return ctt::host_slices(n, want, (double)((C::BITS + 16) / 16) * C::TUNE.acc_ns * 1.09, 32 + (scalars_only ? 0 : sizeof(Affine<F>)));
  }
  // d_prepared (with table_c / table_n for a window table): the bases are cached on the device (prepare_bases / prepare_table), only the
  // coefficients are host-resident -- the ZAL msm_with_cached_base shape with host scalars; h_points and d_stage_points are not used.
  int submit_host(const void* h_coefs, bool coef_is_fr, const void* h_points, uint32_t n, void* d_stage_coefs,
                  void* d_stage_points, int want_chunks, const void* d_prepared = nullptr, int table_c = 0, uint32_t table_n = 0) {
    const int sl = claim_slot(n);
    if (sl < 0 || n == 0) return sl;
    const std::vector<uint32_t> bound = host_slices(n, want_chunks, d_prepared != nullptr);
    auto plan_of = [&](uint32_t cnt, const MsmOptions& oo) {
      return table_c > 0 ? make_table_plan(cnt, C::BITS, table_c, table_n, oo) : make_plan(cnt, C::BITS, oo);
    };
    const uint32_t nch = (uint32_t)bound.size() - 1;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < nch; i++) largest = bound[i + 1] - bound[i] > largest ? bound[i + 1] - bound[i] : largest;
    const PlaceInputs pin = place_inputs(sl, d_prepared, table_c);
    Placement pl;
    place_host(pl, pin, nch, BK::THREADED_UPLOAD);
    MsmOptions o = opt;
    if (o.c <= 0) o.c = choose_window_bits(n, C::BITS, o.lanes, o.acc_ns, o.red_ns);  // one window size for the whole MSM
    try {
    bk.stage_begin(sl, ST_TOTAL);
    const MsmPlan p0 = plan_of(largest, o);   // the largest slice sizes the workspace
    // ONE bucket set for all slices (round 4): the accumulation of slice i > 0 continues the stored sums (k_accum<FD, true>).  Rounds
    // 2-3 gave every slice its own set and added the sets afterwards: a full addition per bucket and slice, 0.24 ms of a 4.6 ms call
    // at 2^20 BLS12-381 G1 in three slices (k_bucket_sum, profiles/hostptr_timeline_r04.txt).
    XYZZ<FD>* d_sets = (XYZZ<FD>*)need(bucketsS[sl], (size_t)p0.W * p0.B * sizeof(XYZZ<FD>));
    void* d_conv_all = (kConvert && !d_prepared) ? need(cpoints, (size_t)n * record_stride()) : nullptr;
    reserve_stage1(sl, p0, coef_is_fr);
    MsmPlan plast = p0;
    Staged st_prev{};
    MsmPlan p_prev = p0;
    auto upload_coefs = [&](uint32_t i) {
      const uint32_t start = bound[i], cnt = bound[i + 1] - bound[i];
      bk.h2d((uint32_t*)d_stage_coefs + (size_t)start * 8, (const char*)h_coefs + (size_t)start * 32, (size_t)cnt * 32);
    };
    auto upload_points = [&](uint32_t i) {
      const uint32_t start = bound[i], cnt = bound[i + 1] - bound[i];
      if (!d_prepared)
        bk.h2d((Affine<F>*)d_stage_points + start, (const char*)h_points + (size_t)start * sizeof(Affine<F>), (size_t)cnt * sizeof(Affine<F>));
    };
    bool threaded = pl.threaded;   // (msm_place.h place_host)
    std::atomic<uint32_t> uploaded{0}, coefs_up{0};
    std::atomic<bool> upload_failed{false};   // a HIP call failed on the uploader thread: reported by THIS thread (the one an entry point's error channel belongs to)
    std::thread uploader;
    struct Joiner {
      std::thread& t;
      ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{uploader};                          // (also on the out-of-memory exit: the staging buffers outlive this call)
    if (threaded) {
      try {
        uploader = std::thread([&]() {
          // (a failed copy on this thread must not abort a process whose entry point can report: the guard makes HIP_CHECK throw here,
          // the flag hands the failure to the submitting thread -- ADVICE r5; the emulator's guard is empty)
          typename BK::GuardScope guard;
          try {
          bk.uploader_begin();
          for (uint32_t i = 0; i < nch; i++) {
            upload_coefs(i);
            // An event between the two copies only for the first slice.  Measured with a record after every slice's coefficients
            // (rocprofv3 --memory-copy-trace): the copy behind such a record started only when the accumulation running on the main
            // stream had ended -- no overlap left, 2^20 pairs 5.5 ms instead of 4.4, 2^22 19.6 instead of 13.5.  (A record is a
            // barrier packet in a hardware queue, and the copy ordered behind it waits for it; giving the copy stream a priority
            // class of its own changed nothing.)  Behind the first slice's coefficients nothing long is running.
            if (i == 0 && !d_prepared) bk.h2d_coefs_done(i);
            coefs_up.store(i + 1, std::memory_order_release);
            upload_points(i);
            bk.h2d_slice_done(i);
            uploaded.store(i + 1, std::memory_order_release);
          }
          } catch (...) {
            upload_failed.store(true, std::memory_order_release);
            coefs_up.store(nch, std::memory_order_release);     // (release the submitting thread's waits)
            uploaded.store(nch, std::memory_order_release);
          }
        });
      } catch (const std::system_error&) {
        threaded = false;   // (no thread to be had: this one copies, as with two slices)
      }
    }
    for (uint32_t i = 0; i < nch; i++) {
      const uint32_t start = bound[i], cnt = bound[i + 1] - bound[i];
      bk.stage_chunk((int)i);   // stage events of this slice (the stage times of the call are the sums over its slices)
      uint32_t* d_c = (uint32_t*)d_stage_coefs + (size_t)start * 8;
      Affine<F>* d_p = (Affine<F>*)d_stage_points + start;
      auto await = [&](std::atomic<uint32_t>& flag, uint32_t i) {
        for (uint32_t spin = 0; flag.load(std::memory_order_acquire) <= i; spin++) {
          if (spin < 20000u) cpu_relax(); else std::this_thread::yield();
        }
        if (upload_failed.load(std::memory_order_acquire)) bk.uploader_failed();   // (throws to the entry point's boundary, or aborts where there is none)
      };
      const bool late_points = pl.late_points && i == 0;   // (msm_place.h place_host)
      if (threaded) {
        if (late_points) {
          await(coefs_up, i);
          bk.h2d_coefs_wait(i);                                                                   // main stream waits for the coefficients
        } else {
          await(uploaded, i);
          bk.h2d_slice_wait(i);                                                                   // ... for both copies
        }
      } else {
        upload_coefs(i);
        if (late_points) bk.h2d_done();
        else {
          upload_points(i);
          bk.h2d_done();
        }
      }
      const std::function<void()> points_arrive = [&, i]() {
        if (threaded) {
          await(uploaded, i);     // (the uploader thread has handed the slice's points to the link)
          bk.h2d_slice_wait(i);
        } else {
          upload_points(i);
          bk.h2d_done();
        }
      };

      if (i > 0) {   // slice i-1's merge goes in front of slice i's kernels (shared workspace)
        bk.stage_chunk((int)i - 1);
        merge_buckets(sl, p_prev, st_prev);
        bk.stage_chunk((int)i);
      }
      const MsmPlan p = plan_of(cnt, o);
      if (p.W != p0.W || p.B != p0.B) {   // (the slices share one bucket set: same windows, same buckets -- o.c is fixed above)
        fprintf(stderr, "[ctt_msm] FATAL: slice %u of a host-pointer MSM planned %u windows of %u buckets, the call %u of %u\n", i, p.W, p.B, p0.W, p0.B);
        abort();
      }
      void* d_conv = (kConvert && !d_prepared) ? (void*)((char*)d_conv_all + (size_t)start * record_stride()) : nullptr;
      // (cached bases: the slice's records -- or, in a window table, its column of every row block: row w * table_n + j -- start `start` records in)
      const void* d_prep = d_prepared ? (const void*)((const char*)d_prepared + (size_t)start * record_stride()) : nullptr;
      place_accum(pl, pin, p, /*device_resident=*/false);
      st_prev = accumulate_pairs(sl, p, pl, d_c, coef_is_fr, d_prepared ? nullptr : d_p, d_prep, d_conv, d_sets, /*into=*/i > 0,
                                 late_points ? &points_arrive : nullptr);
      p_prev = p;
      plast = p;
    }
    merge_buckets(sl, p_prev, st_prev);
    plast.n = n;
    slots[sl].plan = plast;
    last_plan = plast;
    last_chunks = nch;
    place_reduction(pl, pin, plast, /*may_start_early=*/false, [&](uint32_t ntasks, uint32_t W) { return bk.pyr_goes_to_tail(ntasks, W); });
    reduce_buckets(sl, plast, pl, d_sets);
    } catch (const OutOfDeviceMemory&) {
      return release_slot(sl);
    }
    return sl;
  }
  uint32_t last_chunks = 1;

  // Host tail of a submitted MSM: wait for its W window sums, Horner over the windows.
  // (Round 6 built this tail on a helper thread of the engine -- handed over at the end of submit(), finish() only collecting the result --
  // on the reading that the caller's thread, 0.1 ms of enqueueing + 0.1-0.2 ms of tail per MSM, is what starves the main stream of a small
  // pipelined MSM.  Measured, same box, same process, finishing thread / helper thread: 2^14 0.310 / 0.309 ms per MSM, 2^16 0.428 / 0.428,
  // 2^17 0.601 / 0.604 with three in flight, 2^16 0.449 / 0.444 with two -- nothing: with a third slot the GPU has the next MSM queued
  // whatever the host does meanwhile.  Removed again; EXPERIMENTS.md has the table.)
  XYZZ<HF> finish(int sl) {
    Slot& S = slots[sl];
    if (!S.busy) {
      fprintf(stderr, "[ctt_msm] FATAL: finish() of a slot that was not submitted\n");
      abort();
    }
    S.busy = false;
    if (S.empty) return XYZZ<HF>::inf();
    bk.d2h_wait(sl);
    const MsmPlan& p = S.plan;
    const XYZZ<FD>* raw = (const XYZZ<FD>*)S.hraw;
    const size_t cnt = (size_t)p.W * p.ngrp;
    std::vector<XYZZ<HF>> sums(cnt);
    for (size_t i = 0; i < cnt; i++) sums[i] = xyzz_to_host<FD>(raw[i]);
    return combine_groups<HF>(sums.data(), p.W, p.lay, p.h, p.ngrp);
  }

  bool in_flight(int sl) const { return sl >= 0 && sl < NSLOT && slots[sl].busy; }

  // r = sum of n affine points (sum_reduce_vartime, ec_shortweierstrass_batch_ops.nim:649-663).  One window, one
  // bucket: the identity entry list goes through the accumulate kernel (K points per lane) and the head-merging
  // tree; blocking.  Shares the MSM workspace (stream order keeps it apart from MSMs in flight).
  uint32_t last_sum_K = 0;
  XYZZ<HF> sum_reduce(const Affine<F>* d_points_in, uint32_t n) {
    if (n == 0) return XYZZ<HF>::inf();
    bk.tail_wait();  // shares the workspace with MSMs in flight
    const uint32_t lanes = opt.lanes ? opt.lanes : 65536;
    uint32_t K = (uint32_t)(((uint64_t)n + lanes - 1) / lanes);
    if (K < 16) K = 16;
    if (opt.K > 0) K = (uint32_t)opt.K;
    const uint32_t G = (n + K - 1) / K;
    last_sum_K = K;
    void* d_converted = kConvert ? need(cpoints, (size_t)n * record_stride()) : nullptr;
    const void* d_points = accum_points(d_points_in, nullptr, d_converted, n, true);
    uint32_t* d_entries = (uint32_t*)need(entries, (size_t)n * 4);
    uint32_t* d_bstart = (uint32_t*)need(bstartS[0], 8);
    uint32_t* d_maxcount = (uint32_t*)need(maxcountS[0], 256);
    bk.launch_iota(d_entries, n, d_bstart, d_maxcount);
    XYZZ<FD>* d_buckets = (XYZZ<FD>*)need(bucketsS[0], sizeof(XYZZ<FD>));
    bk.memset0(d_buckets, sizeof(XYZZ<FD>));
    XYZZ<FD>* d_heads = (XYZZ<FD>*)need(heads, (size_t)G * sizeof(XYZZ<FD>));
    XYZZ<FD>* d_tails = (XYZZ<FD>*)need(tails, (size_t)G * sizeof(XYZZ<FD>));
    uint32_t* d_hkey = (uint32_t*)need(hkey, (size_t)G * 4);
    uint32_t* d_tkey = (uint32_t*)need(tkey, (size_t)G * 4);
    AccumArgs<FD> aa{d_entries, d_bstart, d_points, record_stride(), d_buckets, d_heads, d_tails, d_hkey, d_tkey, n, 1, K, G};
    bk.template launch_accum<FD>(aa, 1);
    MergeArgs<FD> ma{d_bstart, d_buckets, d_heads, d_tails, d_hkey, d_tkey, d_maxcount, 1, K, G};
    merge_tree(ma, 1, 32);   // (every step: until d >= G)
    XYZZ<FD> raw;
    bk.d2h_sync(&raw, d_buckets, sizeof(raw));
    return xyzz_to_host<FD>(raw);
  }
};

// ---------------------------------------------------------------------------------------------
// Output conversion to the caller's coordinate system (C API structs, include/constantine/curves/*.h)
// ---------------------------------------------------------------------------------------------
enum { OUT_AFF = 0, OUT_JAC = 1, OUT_PRJ = 2 };

// EC_ShortW_Jac neutral (1,1,0) jacobian.nim:58-64; EC_ShortW_Prj neutral (0,1,0) projective.nim:56-62.
// Any representative of the same group element is a valid result (the reference's own raw coordinates
// differ between its serial and parallel paths); we emit the canonical one with Z = 1.
template <class F>
static inline void write_result(void* r, const XYZZ<F>& res, int out_kind) {
  Affine<F> a = xyzz_to_affine<F>(res);
  F* o = (F*)r;
  if (out_kind == OUT_AFF) {
    o[0] = a.x;
    o[1] = a.y;
    return;
  }
  if (a.is_inf()) {
    o[0] = out_kind == OUT_JAC ? F::one() : F::zero();
    o[1] = F::one();
    o[2] = F::zero();
  } else {
    o[0] = a.x;
    o[1] = a.y;
    o[2] = F::one();
  }
}

}  // namespace ctt
