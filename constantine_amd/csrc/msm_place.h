// msm_place.h -- where and when the stages of one MSM run: the endomorphism split, the lanes the plan is made for, which stages leave the
// main stream and what the accumulation waits for.  Host arithmetic only, no backend and no launches: MsmEngine (msm_pipeline.h) fills one
// Placement per call and follows it; tests/c_api/t_place.cpp records what it then asks of a backend, row by row.  The measurements beside
// each decision are why the thresholds are what they are.
#pragma once
#include "msm_plan.h"

namespace ctt {

// The environment knobs of the placement, read once per process (before the first MSM is placed).
struct PlaceKnobs {
  // every reduction pass but the first goes to the tail stream, the wide ones next to the following MSM's conversion and sort (place_reduction)
  bool wide_early = env_int("CTT_HIP_MSM_WIDE_EARLY", 1) != 0;
  // Wave slots the accumulate grid must leave free for the previous MSM's tail to run beside it (fewer: the accumulation waits
  // for that tail first), and how much of an accumulation place_lanes may spend on leaving slots free on purpose for an MSM kept
  // in flight ...
  uint32_t tail_min_free = (uint32_t)env_int("CTT_HIP_MSM_TAIL_MIN_FREE", 16);
  // ... as a fraction of the wait it removes, which is about one tenth of a millisecond for BLS12-381 G1 and scales with the
  // curve's addition time (the tail is a chain of dependent additions)
  double tail_free_ratio = env_double("CTT_HIP_MSM_TAIL_FREE_RATIO", 0.5);
  uint32_t small_free_32nds = (uint32_t)env_int("CTT_HIP_MSM_SMALL_FREE_32NDS", 2);   // lanes left free up to 2^17 pairs, in 32nds
  int front = env_int("CTT_HIP_MSM_FRONT", 1);             // front stream: 0 off, 1 automatic, 2 whenever pipelining
  int early_tail = env_int("CTT_HIP_MSM_EARLY_TAIL", 1);   // early tail: 0 off, 1 automatic, 2 whenever pipelining
  bool late_points = env_int("CTT_HIP_MSM_LATE_POINTS", 1) != 0;   // (0: both copies of a host-pointer call's first slice before its sort)
};
inline const PlaceKnobs& place_knobs() {
  static const PlaceKnobs k;
  return k;
}

// What a decision may look at besides the pair count and the plan.
struct PlaceInputs {
  const MsmOptions& opt;       // the caller's options; lanes = the resident lanes of the whole chip (of the main stream's part of it)
  const CurveTuning& tune;     // the curve's measured figures (msm_bodies.h)
  bool pipelining;             // another MSM is in flight beside this one
  bool partitioned;            // Backend::partitioned(): the tail stream has compute units of its own
  bool cached;                 // the bases are cached records
  int table_c;                 // > 0: ... a window table with this many window bits
};

struct Placement {
  static constexpr int AT_MERGE = -1, NEVER = 0x7fffffff;
  // ---- before the plan (place_lanes)
  bool glv = false;            // the endomorphism split runs
  uint32_t lanes = 0;          // the lanes the plan is made for
  int c = 0;                   // window bits, fixed for the whole chip before lanes were taken away (0: the plan builder chooses)
  // ---- one accumulation (place_accum; a host-pointer call: once per slice)
  bool front_side = false;     // conversion, digits and sort on the front stream
  bool wait_whole_tail = false;   // the accumulation waits for the end of the previous tail, not only for its wide passes
  uint32_t handover = 0;       // drop distance of the accumulate kernel's priority hand-over (hip_backend.h k_accum), 0 = none
  // ---- merge and reduction (place_reduction).  A position is a reduction pass, 0 .. c - 2, in front of which the thing happens; c - 1 = behind the
  // last pass; AT_MERGE = at the head merge; NEVER.
  int tail_from = NEVER;       // the tail stream begins (AT_MERGE: in front of the head merge -- the early tail)
  int wide_mark_at = NEVER;    // "the wide passes are done" is marked (AT_MERGE: behind the head merge -- partitioned chip)
  bool narrow_priority = false;   // raised wave priority for the narrow passes
  // ---- a host-pointer call (place_host)
  bool threaded = false;       // a thread of its own issues the copies
  bool late_points = false;    // the first slice's sort starts on its coefficients, the points follow
  bool early_tail() const { return tail_from == AT_MERGE; }
};

// The split, and the lanes the plan is made for.
// The endomorphism split (msm_bodies.h bls12_381_glv_split): 2n entries of 127 bits in place of n of 255 -- the same accumulations in half the
// bucket sets.  Device-resident points without cached records or a table, at the curve's sizes (glv_log2n .. glv_max_log2n) or as the option says
// (can_split: the curve has one and the backend its front kernel).  bits / glv_bits: of a scalar, whole / split.
static inline Placement place_lanes(const PlaceInputs& in, uint32_t n, int bits, int glv_bits, bool can_split) {
  const MsmOptions& opt = in.opt;
  const CurveTuning& t = in.tune;
  Placement pl;
  pl.glv = can_split && !in.cached && in.table_c <= 0 && n <= (1u << 30) && opt.glv != 2 &&
           (opt.glv == 1 || (t.glv_log2n > 0 && n >= (1u << t.glv_log2n) && n <= (1u << t.glv_max_log2n)));
  const uint32_t pn = pl.glv ? 2u * n : n;   // entries per bucket set and bits of a scalar the plan is made for
  const int pbits = pl.glv ? glv_bits : bits;
  pl.lanes = opt.lanes;
  pl.c = opt.c;
  // A caller that keeps MSMs in flight gets the tail of the previous MSM (reduction passes behind the first, bit Horner, result
  // copy: latency-bound, a few dozen waves at a time) run BESIDE this accumulation when the accumulate grid leaves wave slots free
  // (place_accum); it pays to leave them free on purpose.  Up to 2^17 pairs: 1/16 of the lanes.  (Round 2 took 5/32 -- BLS12-381
  // G1 2^17, ms per MSM with two in flight: 0.69 with 17 % of the slots free, 0.80 with 5 %; since the larger sizes stopped waiting
  // for the tail too, 1/16 measures level or better: 2^17 0.742 against 0.759 ms with 5/32, G2 2^16 1.048 against 1.074.)
  // (the window size is chosen for the whole chip first: fewer lanes must only lengthen K)
  // (partitioned chip: the tail runs on compute units the accumulate grid never sees -- opt.lanes counts the main stream's CUs only)
  if (in.partitioned || !in.pipelining || opt.K > 0 || in.table_c > 0) return pl;
  const PlaceKnobs& k = place_knobs();
  if (n <= (1u << 17)) {
    if (pl.c <= 0) pl.c = choose_window_bits(pn, pbits, opt.lanes, opt.acc_ns, opt.red_ns);
    pl.lanes = (uint32_t)((uint64_t)opt.lanes * (32u - (k.small_free_32nds < 31u ? k.small_free_32nds : 31u)) / 32u);
  } else if (opt.lanes >= 64u * 1024u && opt.acc_ns >= 0.1) {
    // Larger ones: the accumulation used to wait for the previous tail -- ten dependent narrow passes, the bit Horner and the result
    // copy, ~0.25 ms after the last wide pass, 0.1 ms longer than this MSM's sort (rocprof timeline, BLS12-381 2^20: the sort ends
    // at 177 us, the accumulation started at 281).  With 1/64 of the wave slots left free (32 of 2048; K 128 -> 131 at 2^20) the
    // tail finishes beside the accumulation instead.  Same box, ms per MSM with / without: BLS12-381 G1 2^19 1.72 / 1.82,
    // 2^20 2.92 / 2.98, 2^21 5.54 / 5.59, 2^22 10.60 / 10.47; G2 2^18 2.92 / 3.13, 2^20 9.50 / 9.46 -- it pays while that share of the
    // accumulation is well below the wait (profiles/sweep_free_wave_slots_r03.txt).  Not for the 254/255-bit G1 fields (acc_ns < 0.1):
    // their additions are twice as fast, their tail ends before their sort does, and the free slots only cost (Pallas 2^20 1.455 / 1.433).
    if (pl.c <= 0) pl.c = choose_window_bits(pn, pbits, opt.lanes, opt.acc_ns, opt.red_ns);
    int Wc;
    window_layout(pbits, pl.c, &Wc);
    // 32 slots at least: a narrow pass is up to 64 waves, and a G2 wave needs a SIMD to itself (16 free slots of its 1024
    // measured no gain, 32 did: 3.13 -> 2.92 ms at 2^18)
    const uint32_t nslots = opt.lanes / 64u, free_slots = nslots / 64u > 32u ? nslots / 64u : 32u;
    const double cost_ms = (double)Wc * pn * opt.acc_ns * 1e-6 * free_slots / nslots, wait_ms = 0.1 * opt.acc_ns / 0.142;
    if (cost_ms <= k.tail_free_ratio * wait_ms) pl.lanes = opt.lanes - 64u * free_slots;
  }
  return pl;
}

// One accumulation of plan p (an MSM's, or that of one slice of a host-pointer call).
static inline void place_accum(Placement& pl, const PlaceInputs& in, const MsmPlan& p, bool device_resident) {
  const MsmOptions& opt = in.opt;
  const CurveTuning& t = in.tune;
  const PlaceKnobs& k = place_knobs();
  // Front stream (round 5 experiment, option front_side = 1; off by default): conversion and sort of a small MSM submitted while another is in
  // flight on the front stream, beside that MSM's head merge and first reduction pass.  (A lone blocking call has nothing to run beside.)
  // Measured and NOT adopted (profiles/front_stream_small_msm_r05.txt, same box, ms per MSM with two in flight, main stream only / front stream):
  // BLS12-381 G1 2^12 0.278 / 0.287, 2^14 0.388-0.393 / 0.383-0.386, 2^16 0.470 / 0.494, 2^17 0.637 / 0.664, G2 2^16 1.077 / 1.227.  The overlap
  // is real (the sort leaves the main stream's chain), but with a second hardware queue active the dependent kernels of BOTH chains start later
  // (round 3 saw the same with two engine lanes: 50-70 us between dependent launches).  What the experiment did find: a process has FOUR hardware
  // queues (GPU_MAX_HW_QUEUES); with the front stream as a FIFTH stream of the context (null, main, tail, copy, front) two streams shared a queue
  // and every small pipelined MSM lost 8 % (2^16: 0.52 -> 0.56 ms) without a single kernel on the new stream -- the front stage therefore
  // runs on the copy stream (HipBackend::init), and nothing in the library may add a stream lightly.
  pl.front_side = device_resident && k.front != 0 && opt.front_side != 2 && in.pipelining && (k.front >= 2 || opt.front_side == 1);
  // The previous MSM's tail (narrow reduction passes + result copy on the backend's second stream) has had this MSM's
  // conversion and sort to run underneath; the accumulation must not start before it is done: k_accum takes every
  // wave slot of the chip for its whole duration, and a tail kernel enqueued behind it would wait it out (measured on
  // a slower box: reduce span 2.4 ms, the pipeline slower than the serial order).  Worst case this is the serial order.
  // When the accumulate grid leaves wave slots free (place_lanes sees to that for a caller that keeps MSMs in flight: 1/16 of the
  // slots up to 2^17 pairs, 1/64 of them while that costs less than half the wait), the previous tail's narrow passes run next to it, and the wait moves to the
  // start of this MSM's reduction (MsmEngine::reduce_buckets), the first kernel that writes what the tail still reads.
  // (partitioned chip: the tail stream has compute units of its own -- nothing to wait for, no slots to leave)
  // (whole_tail_log2n: large MSMs of the curves whose accumulate kernel owns every register wait for the whole tail whatever the grid leaves free)
  const uint64_t accum_waves = (uint64_t)p.W * ((p.G + 63u) / 64u);
  const bool whole_tail = t.whole_tail_log2n > 0 && p.pairs() >= (1u << t.whole_tail_log2n);
  pl.wait_whole_tail = !in.partitioned && (whole_tail || accum_waves + k.tail_min_free > (uint64_t)opt.lanes / 64u);
  // The hand-over: by the curve's measurement (accum_handover from 2^accum_handover_log2n pairs) unless the option names a distance: K / 8, and not
  // below the curve's floor.
  if (opt.accum_handover >= 2) pl.handover = (uint32_t)opt.accum_handover;
  else if (opt.accum_handover != 1 || t.accum_handover == 0 || p.pairs() < (1u << t.accum_handover_log2n)) pl.handover = 0u;
  else pl.handover = p.K / 8u > (uint32_t)t.accum_handover ? p.K / 8u : (uint32_t)t.accum_handover;
}

// Head merge and bucket reduction of plan p: what moves to the tail stream.  goes_to_tail(ntasks, W): Backend::pyr_goes_to_tail, a pass narrow
// enough to run underneath the next MSM's conversion and sort.  may_start_early: a device-resident MSM (not the one reduction of a host-pointer call).
template <class Pred>
static inline void place_reduction(Placement& pl, const PlaceInputs& in, const MsmPlan& p, bool may_start_early, Pred goes_to_tail) {
  const MsmOptions& opt = in.opt;
  const CurveTuning& t = in.tune;
  const PlaceKnobs& k = place_knobs();
  pl.narrow_priority = t.narrow_prio_log2n > 0 && p.pairs() <= (1u << t.narrow_prio_log2n);
  pl.tail_from = pl.wide_mark_at = Placement::NEVER;
  // The narrow passes at the end, the bit Horner and the result copy move to the backend's tail stream: they are
  // latency-bound and the next MSM's conversion and sort fit underneath them.
  // (only for a caller that keeps MSMs in flight -- the other slot is busy: a lone blocking call would pay the fork's
  // event record and wait, ~15 us, for nothing)
  if (!in.pipelining) return;
  // Early tail (round 4): a caller that keeps large MSMs in flight gets the head merge and EVERY reduction pass of this MSM on the
  // tail stream, so that the next MSM's conversion and sort -- memory-bound -- start right behind this accumulation instead of
  // behind the merge and the widest pass (VALU-bound additions, 0.16 ms at 2^20).  What those stages read is per slot (bstartS,
  // maxcountS, bucketsS); the next accumulation still waits for the end of the wide passes (wide_wait), so nothing of this tail
  // competes with an accumulation for wave slots (which is what sank round 3's version for small MSMs, section 5 of DESIGN.md).
  // From ~2^18 pairs on, and while the accumulation is shorter than ~6 ms.
  // Measured on one box, ms per MSM with two in flight, off / on, three repetitions (profiles/early_tail_r04.txt): BLS12-381 G1 2^19
  // 1.70 / 1.63, 2^20 2.90 / 2.81 (-3.1 %), BN254 2^20 1.62 / 1.58, 2^22 5.39 / 5.25, Pallas 2^20 1.46 / 1.40 (-3.9 %), 2^18 1.011 / 0.998;
  // but BLS12-381 G1 2^22 10.5 / 10.6 and G2 2^20 9.45 / 9.49: with a 8-10 ms accumulation the 0.16 ms are 1.5 % at best and the sort
  // (0.5 ms at 2^22) running beside the widest pass loses more than the overlap gives.
  const double additions = (double)p.nent * (double)p.W;
  if (may_start_early && k.early_tail != 0 && opt.early_tail != 0 &&
      (k.early_tail >= 2 || opt.early_tail >= 2 || (additions >= (double)(1u << 22) && additions * opt.acc_ns < 6.0e6))) {
    pl.tail_from = Placement::AT_MERGE;
    // Partitioned chip: the next accumulation shares the head / tail slots with this merge and nothing else with this
    // tail -- it waits for the merge, not for the wide reduction passes (which run on the tail stream's own compute units)
    if (in.partitioned) pl.wide_mark_at = Placement::AT_MERGE;
  }
  // wide_early: every pass but the first goes to the tail stream, the wide ones next to the following MSM's conversion and sort
  // (VALU-bound additions beside memory-bound kernels); that MSM's accumulation waits for the end of the WIDE passes only
  // (wide_mark / wide_wait) -- the narrow rest runs beside it in the wave slots its grid leaves free.
  // Same box, ms per MSM with / without (profiles/wide_passes_on_tail_r03.txt): BLS12-381 G1 2^20 2.92 / 2.97, 2^18 0.965 / 0.977, 2^22 10.70 /
  // 10.75; no difference for the other curves -- the kernels do slow each other down (round 2 measured the sort 0.19 -> 0.23 ms
  // under wide passes), a quarter of the overlap is what remains.
  const bool first_pass_on_tail = opt.pyr0_tail == 1 && p.pairs() <= (1u << 17) && !p.merged;   // (MsmOptions::pyr0_tail: measured, off)
  const int last = p.c - 1;   // behind the last pass
  for (int pass = 0; pass < last && pl.wide_mark_at == Placement::NEVER; pass++) {
    const bool narrow = goes_to_tail(pyr_pass_tasks(p.B, p.c, pass), (uint32_t)p.W);
    if (pl.tail_from == Placement::NEVER && (pass > 0 || first_pass_on_tail) && (narrow || k.wide_early)) pl.tail_from = pass;
    if (pl.tail_from != Placement::NEVER && narrow) pl.wide_mark_at = pass;
  }
  if (pl.tail_from == Placement::NEVER) pl.tail_from = last;
  if (pl.wide_mark_at == Placement::NEVER) pl.wide_mark_at = last;
}

// A host-pointer call of nch slices.
// threaded: several slices -- a thread of its own issues the copies back to back (HipBackend::h2d_slice_done has the reason), the submitting one
// enqueues slice i's kernels as soon as slice i has been handed to the link.  (Two slices: one gap of ~0.1 ms against a thread start of about
// as much -- measured: 2^18 1.85 ms without, 1.93 with.)
// late_points: the first slice starts on its coefficients: the digits and the sort need nothing else, and they run while the slice's points
// cross the link (MsmEngine::accumulate_pairs, points_arrive).  Later slices wait for both copies at once (their sort queues behind the
// previous accumulation anyway, and an event between their copies would hold the second one back: see the uploader).
static inline void place_host(Placement& pl, const PlaceInputs& in, uint32_t nch, bool backend_threads) {
  pl.threaded = backend_threads && nch > 2;
  pl.late_points = place_knobs().late_points && !in.cached;
}

}  // namespace ctt
