// msm_plan.h -- how one MSM is planned: window width, the sort's sizing, entries per accumulate lane, the merge form, the slices of a
// host-pointer call.  Host arithmetic only (msm_bodies.h for WinLayout and horner_groups); msm_pipeline.h runs a plan over a backend.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "msm_bodies.h"

namespace ctt {

// An environment knob: callers keep the value in a static, so each is read once per process, before its first use.
static inline int env_int(const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; }
static inline double env_double(const char* name, double dflt) { const char* s = getenv(name); return s ? atof(s) : dflt; }

struct MsmPlan {
  uint32_t n;
  int c, W;
  uint32_t B;      // buckets per window = 2^(c-1)
  uint32_t S;      // partition blocks (sort pass A): each handles `slice` consecutive scalars
  uint32_t slice;  // scalars per partition block
  uint32_t NG;     // bucket groups per window (sort pass A partitions by group, pass B sorts inside a group)
  uint32_t gshift; // group = bucket >> gshift
  uint32_t gshift_narrow;  // windows one bit narrower than c only reach B/2 buckets: their groups are half as wide
  WinLayout lay;       // widths / offsets of the W (Wd) digit windows; c = lay.cmax()
  uint32_t jbits;  // bits of a point index (sort records pack low bucket bits | sign | index into 32 bits)
  uint32_t cap, big;  // sort pass B: LDS tile entries; bucket size above which the LDS image is bypassed
  uint32_t K;      // sorted entries per accumulate lane
  uint32_t G;      // accumulate lanes per window
  // window-table form (make_table_plan): Wd digit windows share ONE bucket set (W = 1) of nent = Wd*n entries
  int Wd;              // digit windows per scalar (== W otherwise)
  uint32_t merged;     // 1 = window-table form
  uint32_t nent;       // entries per bucket set: n, or Wd*n
  uint32_t id_stride;  // table rows per window (the cached bases' length; a call may use a prefix)
  int h, ngrp;         // bit Horner: bits per group, groups per window (the device returns W*ngrp partial sums)
  int merge_steps;     // wide head-merge tree steps enqueued without knowing the largest bucket (plan_merge_steps)
  uint32_t merge_lmax; // > 0: the queue form of the head merge (msm_bodies.h merge_tail_queue_body) for chains of at most this many heads; 0: the tree
  // 1 = the endomorphism split (msm_bodies.h bls12_381_glv_split): n is TWICE the caller's pairs -- entry j the first half of pair j, entry n/2 + j
  // its second -- and the windows are those of a 127-bit scalar (MsmEngine::submit decides; every plan builder leaves 0)
  uint32_t glv = 0;
  uint32_t pairs() const { return glv ? n / 2u : n; }   // the caller's pairs
};

struct MsmOptions {
  int c = 0;          // window bits (0 = choose)
  int K = 0;          // entries per lane (0 = choose from resident lanes)
  int S = 0;          // sort: scalars per partition block (0 = choose)
  uint32_t lanes = 196608;  // resident lanes of the accumulate kernel (set by the backend)
  int host_window_sums = 0;  // legacy spelling of horner_bits: 1 = 1 bit per group (the whole bit Horner on the host),
                             // 2 = one group per window (the whole bit Horner on the device), 0 = horner_bits decides
  int horner_bits = 0;       // bits per group of the bit Horner the device runs (0 = choose: 4); see plan_horner
  // cost model of the window choice: ns per mixed addition (accumulate) / per full addition (reduction) with the chip busy;
  // the engine fills in its curve's figures (msm_bodies.h curve descriptors), the defaults are BLS12-381 G1's
  double acc_ns = 0.142, red_ns = 0.26;
  // sort pass A (hip_backend.hip).  sort_xcd: neighbouring slices on one XCD (1, default) or slice b to block b (0).  sort_staged:
  // records staged through an LDS image of the block's output -- 1 = where it pays (default: from 256 bucket groups per window,
  // i.e. ~2^22 pairs, on; measured, profiles/sort_staged_xcd_r04.txt: the sort of 2^22 / 2^24 BLS12-381 pairs 0.545 -> 0.486 /
  // 2.26 -> 2.06 ms, BN254 2^22 0.526 -> 0.464, but 0.148 -> 0.173 ms at 2^20 and 0.056 -> 0.081 at 2^16: there a block has one or
  // two window steps and the five barriers per step are what it sees), 2 = always, 0 = never (one store per record: the form
  // that also serves more than 1024 groups).  Options "sort_xcd" / "sort_staged", $CTT_SORT_XCD / $CTT_SORT_STAGED.
  int sort_xcd = 1, sort_staged = 1;
  int early_tail = 1;   // MsmEngine::submit: merge + every reduction pass on the tail stream for large pipelined MSMs (0 off, 1 automatic, 2 always)
  // head merge: 0 = the queue form (tail merge + one lane per chain with work left, msm_bodies.h merge_tail_queue_body) when the plan
  // expects chains of at most merge_lmax heads, else the tree; 1 = the queue form always; 2 = the tree always.  merge_lmax 0 = 8.
  int merge_chain = 0, merge_lmax = 0;
  int merge_queue_quad = 0;   // the queue kernel with four lanes per chain (hip_backend.h k_merge_queue_quad): 0 / 1 = on, 2 = one lane per chain
  int front_side = 0;         // small pipelined MSMs: conversion + sort on the front stream (0 automatic, 1 always when pipelining, 2 never)
  // experiment knob (round 5, measured and NOT adopted): 1 = small pipelined MSMs (up to 2^17 pairs) put the FIRST reduction pass on the tail
  // stream too, so that the next MSM's sort starts right behind the head merge.  Same box, ms per MSM with two in flight, off / on:
  // BLS12-381 G1 2^16 0.466-0.473 / 0.480, 2^17 0.654-0.657 / 0.676-0.680, BN254 2^16 0.345 / 0.350 -- the fork's event pair costs what the
  // 25 us of overlap give (gpurun_out/r5i)
  int pyr0_tail = 0;
  // the endomorphism split of a device-resident MSM (curves that have one: msm_bodies.h GlvOf): 0 = at the curve's sizes (CurveTuning::glv_log2n .. glv_max_log2n),
  // 1 = at every size, 2 = never.  Option "glv", $CTT_HIP_MSM_GLV.
  int glv = 0;
  // the priority hand-over of the accumulate kernel (hip_backend.h k_accum): 0 = off (no priority instruction runs), 1 = the curve's drop distance at the
  // curve's sizes (msm_bodies.h CurveTuning::accum_handover, accum_handover_log2n; msm_place.h place_accum), n >= 2 = this drop distance at every size.  Option "accum_handover", $CTT_HIP_MSM_ACCUM_HANDOVER.
  int accum_handover = 1;
};

// The sort's shipped constants: the floor of a partition slice, pass B's LDS tile (cap) and the bucket size above which its LDS image is
// bypassed (big).  The window-table form and the sort probe's "0 = default" take them as they are; the plain form reads them through
// $CTT_SORT_SLICE / _CAP / _BIG (make_plan).
static constexpr uint32_t SORT_SLICE_FLOOR = 2048u, SORT_CAP = 20480u, SORT_BIG = 1024u;

// bits of an index below n (at least 1, at most 31)
static inline uint32_t index_bits(uint64_t n) { uint32_t jb = 1; while (jb < 31 && (1ull << jb) < n) jb++; return jb; }
// steps of a binary tree over a chain of `chain` heads, at most `limit`
static inline int tree_steps(double chain, int limit = 0x7fffffff) { int steps = 0; while (chain > 1.0 && steps < limit) { chain *= 0.5; steps++; } return steps; }

// Window size for the GPU pipeline.  The reference's bestBucketBitSize
// (ec_multi_scalar_mul_scheduler.nim:172-223) models a CPU; any c yields the same group element, so the device
// uses its own cost model with constants measured on MI355X for BLS12-381 (profiles/): they only rank the
// candidates, so the same model serves the other curves.
//   accumulate  W*N mixed adds at 0.142 ns each (2.38 ms / 2^24 at full occupancy)
//   reduce      c-1 passes of 12 us latency each, plus 2*2^(c-1)*W adds of work at 0.24 ns (fitted to 0.43 ms at c = 16,
//               0.185 ms at c = 13)
//   merge       45 us + one 28 us tree step per doubling of the longest head chain.  The top window only has
//               bits - (W-1)*c significant bits: when that is small its few buckets each receive N/2^(top-1)
//               entries and the chain is long -- the model steers away from such c (e.g. c = 14 at N = 2^18)
//   sort        0.02 ns per (window, pair) + 60 us
// Round-2 check against measurements (BLS12-381 G1, ms per pipelined step): 2^16 c = 13 0.709 / c = 16 0.756; 2^18 c = 16
// 1.22 / c = 13 1.59; the round-1 constants still chose c = 13 at 2^17, where c = 16 is the faster plan.
// Scalars per partition block (sort pass A).  Large n: 512 blocks, two per CU, ALL of the same size -- a power-of-two slice
// made 257 blocks of 16384 scalars out of n = 2^22 + 77777, and the one CU that got two of them doubled the time of both
// partition kernels (measured: sort 1.00 ms instead of 0.65 ms).  Small n: at least ~64 blocks.
// From 2^23 pairs on: 2048 blocks.  A block walks its slice in steps of 4096 scalars and, per step, all windows; with 1024 group
// regions per window a step leaves 16 bytes in each run and the line is written back partially before the block returns to it
// (k_part_scatter writes 5.0x its 4 bytes per record at 2^24, 1.55x at 2^22: profiles/pmc_r03_hbm_bytes_*).  Shorter slices
// put the neighbouring pieces of a line into blocks that run at the same time: measured at 2^24, sort 3.40 ms with 32768
// scalars per block, 3.16 with 16384, 2.85 with 8192, 3.06 with 4096 (whose count table is 250 MB); no gain at 2^22.
static inline uint32_t plan_partition_slice(uint32_t n, uint32_t min_slice) {
  const uint32_t nblk = n >= (1u << 23) ? 2048u : 512u;
  uint32_t slice = (uint32_t)(((uint64_t)n + nblk - 1u) / nblk);
  slice = (slice + 255u) & ~255u;
  if (slice < min_slice) slice = min_slice;
  while (slice > 64u && (uint64_t)slice * 64u > n) slice >>= 1;
  return slice;
}

static inline uint32_t plan_entries_per_lane(uint32_t n, int W, uint32_t lanes) {
  uint64_t total = (uint64_t)W * n;
  uint32_t K = (uint32_t)((total + lanes - 1) / lanes);
  if (K < 4) K = 4;
  // The accumulate kernel is launched as W rows of ceil(ceil(n/K)/64) one-wave workgroups, and all of them must be resident
  // at once: with even one workgroup more than wave slots, a second round runs that single wave for a whole K entries
  // (measured, BN254 2^22: c = 15 -> 17 x 241 = 4097 workgroups on 4096 slots, accumulate 6.1 ms instead of ~4.9 ms).
  // The rounding of the rows can exceed the slots for any n that is not a power of two: grow K until the grid fits.
  const uint64_t slots = lanes / 64u;
  if (n > 0 && (uint64_t)W > slots) return K > 0x7ffffff0u ? K : 0x7ffffff0u;   // (more rows than slots: where the loop below ends, without walking there)
  while ((uint64_t)W * ((((uint64_t)n + K - 1) / K + 63u) / 64u) > slots && K < 0x7ffffff0u) K += 1u;
  return K;
}

// (c is the width asked for; the plan's windows are balanced: window_layout(), msm_bodies.h)
// Round-3 re-fit with balanced windows and per-curve constants, against one box's sweeps (gpurun_out/r3d -> profiles/
// sweep_window_bits_r03.jsonl; ms per MSM with two in flight): the model's choice is the measured best or within 3 % of it
// for BLS12-381 G1 2^12 .. 2^22 (13, 13, 13, 13/14, 14, 16, 16, 16), G2 2^16 .. 2^20, BN254 2^16 .. 2^22, Pallas 2^16 / 2^20.
// A latency term is weighted by the curve's addition time (a pass of the reduction is one addition deep).
static inline int choose_window_bits(uint32_t n, int bits, uint32_t lanes, double acc_ns = 0.142, double red_ns = 0.26) {
  double best = 1e300;
  int bc = 8;
  const double ratio = acc_ns / 0.142;
  // (c = 17, 18 only pay from ~2^23 pairs on -- measured BLS12-381 G1 2^24: 15 windows of 17-18 bits 41.3 ms per MSM against
  // 43.6 ms for 16 windows of 16, 2^22: 11.5 against 10.9 -- and the sort's 32-bit records hold c <= 44 - bits(n), see make_plan)
  for (int c = 6; c <= 18; c++) {
    int W;
    const WinLayout L = window_layout(bits, c, &W);
    const int cm = L.cmax();
    const double B = (double)(1u << (cm - 1));
    const double K = (double)plan_entries_per_lane(n, W, lanes);
    const double acc = (double)W * n * acc_ns * 1e-3;
    const double red = (cm - 1) * 8.0 * ratio + 2.0 * B * W * red_ns * 1e-3;
    const double maxcnt = 2.0 * n / (double)(1u << (L.cb - 1));   // the narrower windows fill 2^(cb-1) buckets; twice the mean
    const double mer = (45.0 + 28.0 * tree_steps(maxcnt / K)) * ratio;
    const double srt = (double)W * n * 0.02e-3 + 60.0;
    const double cost = acc + red + mer + srt;
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// Groups of the bit Horner (hip_backend.h k_window_groups, window_group_sum_body): h bits per group, the device returns
// ngrp = ceil((c-1)/h) partial sums per window.
static inline void plan_horner(MsmPlan& p, const MsmOptions& o) {
  int h = o.host_window_sums == 1 ? 1 : o.host_window_sums == 2 ? p.c : o.horner_bits > 0 ? o.horner_bits : 4;
  if (h > p.c) h = p.c;
  p.h = h;
  p.ngrp = horner_groups(p.c, h);
}
// Wide head-merge tree steps to enqueue: enough for the largest bucket an ordinary (uniform) digit distribution produces --
// the mean of the fullest buckets (those of the narrower windows) with a margin of 6 sigma + 8; whatever an unusual input
// needs on top of that is done by the merge-finish launch (one workgroup per window, msm_bodies.h merge_finish_body).
static inline int plan_merge_steps(const MsmPlan& p) {
  // entries per bucket: a window of width cw spreads its n digits over 2^(cw-1) buckets; the window table adds up all windows
  const double narrow = (double)p.n / (double)(1u << (p.lay.cb - 1));
  double m = narrow;
  if (p.merged) {
    const int wide = p.lay.r, nar = p.Wd - p.lay.r;   // (r = 0: every window has cb bits and counts as narrow here)
    m = (double)p.n * ((double)wide + 2.0 * (double)nar) / (double)p.B;
    if (p.lay.r == 0) m = (double)p.n * (double)p.Wd / (double)p.B;
  }
  double sd = 1.0;
  while (sd * sd < m) sd += 1.0;
  m += 6.0 * sd + 8.0;
  return tree_steps((m - 1.0) / (double)p.K + 1.0, 31);
}
// Queue form or tree (MsmPlan::merge_lmax)?  What is left of a chain behind its tail merge is walked by ONE lane, so the form pays while the chains an ordinary digit
// distribution produces are short: the same bound as plan_merge_steps (2^steps >= heads of the fullest ordinary bucket) against
// lmax.  Plans with tiny K against full buckets (a 4096-point commitment over a window table: K = 4, ~90 entries per bucket, chains
// of 20 heads) keep the tree; so does sum_reduce, whose single bucket spans every lane.
static inline uint32_t plan_merge_lmax(const MsmPlan& p, const MsmOptions& o) {
  const uint32_t lmax = o.merge_lmax > 0 ? (uint32_t)o.merge_lmax : 8u;
  if (o.merge_chain == 1) return lmax;
  if (o.merge_chain == 2) return 0u;
  // not over the quadratic extensions (acc_ns is the engine's curve constant: 0.47-0.5 for the G2 curves): a full addition there is 3.3 x a G1
  // one, and the queue kernel's one-lane additions cost more than the tree's four-lane steps -- same box, BLS12-381 G2 2^18, ms per MSM with
  // two in flight, tree / queue: 2.96 / 3.02, and 3.22-3.29 / 3.32-3.36 in the A/B against the round-4 library (profiles/ab_prev_vs_r05_first.txt)
  if (o.acc_ns >= 0.3) return 0u;
  return (p.merge_steps <= 30 && (1u << p.merge_steps) <= lmax) ? lmax : 0u;
}

// ---- the pieces of a plan.  make_plan and make_table_plan put them together; the sort probe (msm_engine.hip) overrides a plan's windows,
// groups and slice through the same three setters.
// The windows of n pairs for c bits asked for (p.n and p.merged are set): balanced windows over bits + 1 bits (msm_bodies.h WinLayout); the
// reference's count, bits/c + 1 windows when c | bits (ec_multi_scalar_mul_parallel.nim:157-158), comes out of the same formula
static inline void plan_set_windows(MsmPlan& p, int bits, int c) {
  p.lay = window_layout(bits, c, &p.Wd);
  p.c = p.lay.cmax();
  p.W = p.merged ? 1 : p.Wd;
  p.B = 1u << (p.c - 1);
  p.nent = p.merged ? (uint32_t)((uint64_t)p.Wd * p.n) : p.n;
}
static inline uint32_t group_shift(uint32_t B, uint32_t NG) { uint32_t s = 0; while ((B >> s) > NG) s++; return s; }
// NG bucket groups per set, and the shifts that go with them.  The windows one bit narrower than c reach half the buckets and get groups half
// as wide; in the window-table form all windows share the groups.
static inline void plan_set_groups(MsmPlan& p, uint32_t NG) {
  p.NG = NG;
  p.gshift = group_shift(p.B, NG);
  p.gshift_narrow = (!p.merged && p.lay.r > 0 && p.gshift > 0) ? p.gshift - 1 : p.gshift;
}
static inline void plan_set_slice(MsmPlan& p, uint32_t slice) { p.slice = slice; p.S = (uint32_t)(((uint64_t)p.n + slice - 1u) / slice); }

// What both plan forms end in, once the form has set n, its windows (plan_set_windows), jbits, id_stride, cap and big.
// Sort pass A: ~512 partition blocks of at least min_slice scalars.  Pass B: bucket groups of ~group_target entries -- `heavy` is what the
// fullest half of the groups hold between them -- (k_group_sort holds one in LDS; a group of up to 20480 is sorted in one sweep), at most
// 1024 buckets per group (LDS counters), and the packed record (low bucket bits | sign | index) must fit 32 bits.
// Then entries per lane (fill the resident lanes once), the bit Horner's groups and the head merge's form.
static inline void plan_finish(MsmPlan& p, const MsmOptions& o, uint32_t min_slice, uint32_t group_target, uint64_t heavy) {
  plan_set_slice(p, o.S > 0 ? (uint32_t)o.S : plan_partition_slice(p.n, min_slice));
  uint32_t NG = 1;
  while ((uint64_t)NG * group_target < heavy && NG < 4096u) NG <<= 1;  // beyond 2^26 pairs the groups grow instead (tiled in pass B)
  while (NG < p.B && p.B / NG > 1024u) NG <<= 1;
  if (NG > p.B) NG = p.B;
  while (NG < p.B && p.jbits + 1 + group_shift(p.B, NG) > 32) NG <<= 1;   // (never with jbits = 0: the 64-bit records of the window table)
  plan_set_groups(p, NG);
  // the packed record (low bucket bits | sign | index) of the sort: 32 bits for every plan that comes through here -- make_plan caps c for it and
  // the loop above narrows the groups down to single buckets if it must; the split's doubled entry count costs one index bit like any other n
  if (!p.merged && p.jbits + 1u + p.gshift > 32u) {
    fprintf(stderr, "[ctt_msm] FATAL: sort record of %u + 1 + %u bits (n = %u, c = %d)\n", p.jbits, p.gshift, p.n, p.c);
    abort();
  }
  uint32_t K = o.K > 0 ? (uint32_t)o.K : plan_entries_per_lane(p.nent, p.W, o.lanes);
  if (K < 4) K = 4;
  p.K = K;
  p.G = (p.nent + K - 1) / K;
  plan_horner(p, o);
  p.merge_steps = plan_merge_steps(p);
  p.merge_lmax = plan_merge_lmax(p, o);
}

static inline MsmPlan make_plan(uint32_t n, int bits, const MsmOptions& o) {
  MsmPlan p;
  p.n = n;
  p.merged = 0;
  p.id_stride = 0;
  p.jbits = index_bits(n);
  int c = o.c > 0 ? o.c : choose_window_bits(n, bits, o.lanes, o.acc_ns, o.red_ns);
  if (c < 2) c = 2;
  if (c > 20) c = 20;   // (the automatic choice stays <= 18; wider windows on request: 2^19 buckets per window at most)
  // the sort packs (low bucket bits | sign | point index) into 32 bits with at most 4096 bucket groups per window:
  // beyond 2^28 pairs that caps the window width (c <= 44 - bits(n): 15 at 2^29, 13 at 2^31)
  while (c > 2 && (int)p.jbits + 1 + (c - 1 - 12) > 32) c--;
  plan_set_windows(p, bits, c);
  static const uint32_t slenv = (uint32_t)env_int("CTT_SORT_SLICE", (int)SORT_SLICE_FLOOR);
  // (18432, not 16384: a size just above a power of two keeps the group count of that power of two -- 2^22 + 77777 pairs with
  // 512 groups of 8192 instead of 256 of 16384 sorted in 0.82 ms instead of 0.65 ms; a group may hold 20480 in one sweep)
  static const uint32_t gsz = (uint32_t)env_int("CTT_SORT_GROUP", 18432);
  static const uint32_t capenv = (uint32_t)env_int("CTT_SORT_CAP", (int)SORT_CAP);
  static const uint32_t bigenv = (uint32_t)env_int("CTT_SORT_BIG", (int)SORT_BIG);
  p.cap = capenv;
  p.big = bigenv;
  plan_finish(p, o, slenv, gsz, n);
  return p;
}

// Window bits of a window table over `ntab` bases (MsmEngine::prepare_table), chosen when the table is built: the table
// fixes c for every later call.  One bucket set serves all windows, so the reduction costs 2*2^(c-1) additions once
// instead of once per window and c can grow until those balance the (bits/c + 1)*N accumulations (an entry is a table row |
// sign << 31: at most 2^31 - 1 rows).
static inline bool table_plan_fits(uint32_t ntab, int bits, int c) {
  int Wd;
  (void)window_layout(bits, c, &Wd);
  const uint64_t rows = (uint64_t)Wd * ntab;   // an entry is a table row | sign << 31
  return rows <= 0x7fffffffull && Wd <= 128;
}
static inline int choose_table_window_bits(uint32_t ntab, int bits) {
  // Same constants as choose_window_bits, one bucket set: 2*2^(c-1) additions of reduction in total, not per window, so c
  // grows until those balance the Wd*N accumulations.  With balanced windows (round 3) the windows one bit narrower than
  // c fill only the lower half of the shared buckets -- twice the mean there, nothing worse: round 2's layout put all N
  // digits of a narrow top window into 2^top buckets and restricted the table to the few c with a wide remainder
  // (measured then, BLS12-381 G1 2^20: c = 20 2.68 ms per MSM, c = 19 3.17 ms, c = 21 4.42 ms).
  double best = 1e300;
  int bc = 0;
  for (int c = 4; c <= 22; c++) {
    if (!table_plan_fits(ntab, bits, c)) continue;
    int Wd;
    const WinLayout L = window_layout(bits, c, &Wd);
    const int cm = L.cmax();
    const double B = (double)(1u << (cm - 1));
    const double total = (double)Wd * ntab;
    const double K = (double)plan_entries_per_lane((uint32_t)(total > 4e9 ? 4e9 : total), 1, 131072);
    const double acc = total * 0.142e-3;
    const double red = (cm - 1) * 12.0 + 2.0 * B * 0.24e-3;
    const double maxcnt = 2.0 * (L.r ? (double)ntab * (L.r + 2.0 * (Wd - L.r)) / B : total / B);
    const double mer = 45.0 + 28.0 * tree_steps(maxcnt / K);
    const double srt = total * 0.02e-3 + 60.0;
    const double cost = acc + red + mer + srt;
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// Plan of one MSM over the first n bases of a window table built with c window bits over ntab bases.
static inline MsmPlan make_table_plan(uint32_t n, int bits, int c, uint32_t ntab, const MsmOptions& o) {
  MsmPlan p;
  p.n = n;
  p.merged = 1;
  p.id_stride = ntab;
  p.jbits = 0;   // (the 64-bit partition records of this form hold the whole table row)
  plan_set_windows(p, bits, c);
  p.cap = SORT_CAP;
  p.big = SORT_BIG;
  // bucket groups of ~12288 records over all windows (the groups of the top window's buckets receive its records on top)
  // (the narrower windows only reach the lower half of the buckets: the groups there hold `heavy` records between them)
  const uint64_t heavy = p.lay.r ? 2ull * ((uint64_t)p.nent - (uint64_t)p.lay.r * n / 2u) : (uint64_t)p.nent;
  plan_finish(p, o, SORT_SLICE_FLOOR, 12288u, heavy);
  return p;
}

// The slices of a host-pointer call: bound[0] = 0 < bound[1] < ... < bound[nch] = n.
// Model (round 4; fitted to the timeline in profiles/hostptr_timeline_r04.txt): the link moves a pair in copy_ns (56 GB/s pageable,
// profiles/h2d_overlap_r02.jsonl), the copies of slice i end at C_i = copy_ns * (pairs up to and including slice i); the GPU takes
// gpu_ns per pair (windows x the curve's accumulate time) plus a fixed fix_ns per slice (conversion, the sort's launch chain, the
// head merge: ~0.19 ms whatever the slice holds) and finishes slice i at F_i = max(F_(i-1), C_i) + gpu_ns * s_i + fix_ns.  Sizes
// s_i ~ r^i; the slice count (1..6, or the caller's) and r (0.5..2.5) are the pair with the smallest F_last, a further slice
// having to buy 3 %.  GPU-bound curves (BLS12-381 G1: 2.5 against 2.3 ns per pair; G2) come out with a small first slice -- its
// copy is the only one exposed -- and growing ones after it (2^20 BLS12-381 G1 pairs: 24 / 32 / 44 %, G2: 12 / 27 / 61 %); copy-bound
// curves (the 254/255-bit ones, 1.2 against 1.7 ns -- the Halo2-ZAL configuration) with shrinking ones, since what is exposed there
// is the last slice's GPU work (BN254 2^22: 24 / 20 / 17 / 15 / 13 / 11 %).  Small calls stay whole: one slice up to 2^17 pairs, two at
// 2^18.  Rounds 2-3 took weights g^i with g = gpu_ns / copy_ns clamped to [0.7, 1.4] and 2 / 3 / 4 slices from 2^18 / 3 * 2^18 / 2^21.
// Measured, same box, old / new (gpurun_out/r4l -> profiles/hostptr_r04.txt, ms per call): BLS12-381 G1 2^20 4.47-4.58 / 4.36-4.58 (level),
// 2^22 14.0-14.2 / 13.3-13.8, 2^24 52.1 / 49.6-50.1; G2 2^20 12.8-13.0 / 12.1-12.2; BN254 2^22 9.33-9.35 / 8.64-8.75; Pallas 2^20 2.87 / 2.86.
// Every slice a multiple of 64 pairs except the last.  An explicit slice count is honoured.
// gpu_ns: the curve's GPU time per pair; copy_bytes: what crosses the link per pair (MsmEngine::host_slices has both).
static constexpr double HOST_SLICE_FIX_NS = 1.9e5;
static inline std::vector<uint32_t> host_slices(uint32_t n, int want, double gpu_ns, size_t copy_bytes) {
  const double copy_ns = (double)copy_bytes / 56.0;
  if (want <= 0 && n < (1u << 15)) return std::vector<uint32_t>{0u, n};   // (small calls stay whole; no search for a 4096-point commitment)
  auto sizes = [&](uint32_t nch, double r) {
    std::vector<uint32_t> bound(nch + 1, 0);
    double wsum = 0, w = 1;
    for (uint32_t i = 0; i < nch; i++, w *= r) wsum += w;
    double acc = 0;
    w = 1;
    for (uint32_t i = 0; i + 1 < nch; i++, w *= r) {
      acc += w;
      uint64_t b = (uint64_t)((double)n * acc / wsum);
      b &= ~63ull;
      if (b <= bound[i]) b = bound[i] + 1;     // tiny inputs: at least one pair per slice
      if (b > n - (nch - 1 - i)) b = n - (nch - 1 - i);
      bound[i + 1] = (uint32_t)b;
    }
    bound[nch] = n;
    return bound;
  };
  auto finish_ns = [&](const std::vector<uint32_t>& bound) {
    double f = 0;
    // (two slices are copied by the submitting thread, which enqueues the first slice's launches in between: ~0.1 ms of idle link)
    const double gap_ns = bound.size() == 3 ? 1.0e5 : 0.0;
    for (size_t i = 0; i + 1 < bound.size(); i++) {
      const double c = copy_ns * (double)bound[i + 1] + gap_ns * (double)i;
      f = (f > c ? f : c) + gpu_ns * (double)(bound[i + 1] - bound[i]) + HOST_SLICE_FIX_NS;
    }
    return f;
  };
  uint32_t lo = 1, hi = 6;
  if (want > 0) lo = hi = (uint32_t)(want > 8 ? 8 : want);
  if (hi > n) hi = n;
  if (lo > hi) lo = hi;
  std::vector<uint32_t> best;
  double best_ns = 0;
  for (uint32_t nch = lo; nch <= hi; nch++) {
    std::vector<uint32_t> b = sizes(nch, 1.0);
    double t = finish_ns(b);
    for (int k = 0; k <= 40 && nch > 1; k++) {
      const std::vector<uint32_t> cand = sizes(nch, 0.5 + 0.05 * k);
      const double tc = finish_ns(cand);
      if (tc < t) { t = tc; b = cand; }
    }
    if (best.empty() || t < best_ns * 0.97) {   // (a further slice has to buy 3 %: small slices accumulate less efficiently than the model says)
      best_ns = t;
      best = b;
    }
  }
  return best;
}

}  // namespace ctt
