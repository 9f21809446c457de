// hip_backend.hip -- the out-of-line half of hip_backend.h: the curve-independent sort kernels (Booth digits, LDS counting sort) and
// HipBackend's init, shutdown and launch_digits_sort.  The context and the C ABI are in msm_engine.hip.
#include <vector>

#include "hip_backend.h"

using namespace ctt;

// ---------------------------------------------------------------------------------------------
// Curve-independent kernels: Booth digits and the LDS counting sort
// ---------------------------------------------------------------------------------------------
// --- digits + sort by bucket ----------------------------------------------------------------------------------
//
// Two passes, no global atomics, no scattered 4-byte writes to HBM:
//
//  A  partition: a block owns `slice` consecutive scalars, recodes them (Booth digits of every window) and
//     distributes (entry, bucket) records into W*NG group regions (group = top bits of the bucket index).  Counts
//     first (k_part_count), a column scan over the blocks (k_part_scan_blocks) and over the groups of a window
//     (k_scan_u32) give every block its private, contiguous run inside every group region, so the second sweep
//     (k_part_scatter) writes runs of ~32 records.
//  B  one workgroup per (window, group) sorts its ~16384 records by the low bucket bits entirely inside LDS
//     (counters + an LDS image of the output) and streams the sorted entries out with full-line writes
//     (k_group_sort).  Groups larger than the LDS image are done in tiles; buckets larger than BIG are written
//     straight to HBM (consecutive claims of one counter are dense anyway).
//
// The first version (one LDS histogram of all 2^(c-1) buckets per slice and a direct scatter) paid 4.8x write
// amplification: 0.24 ms at N = 2^20 and 1.7 ms at 2^22; see DESIGN.md section 4.2.
static constexpr uint32_t GS_LDS_WORDS = 39936;  // most LDS k_group_sort may ask for (156 KiB)
static constexpr uint32_t GS_RPT = 20;       // records per lane k_group_sort keeps in registers (ordinary groups)
static constexpr uint32_t GS_MAXBG = 1024;  // buckets per group (LDS counters; make_plan keeps B/NG below it)
static constexpr uint32_t ENTRY_INVALID = 0xffffffffu;  // never a valid entry: n <= 2^31 - 1

// kwords = 8, or 4 (the half scalars of the endomorphism split, SortArgs::kwords: the upper four words read as zero, and the digit walk
// below finds no window there -- the windows of such a plan cover 128 bits)
__device__ __forceinline__ void load_scalar(const uint32_t* __restrict__ scalars, uint32_t kwords, uint32_t j, uint32_t* k) {
  const uint4* p = reinterpret_cast<const uint4*>(scalars + (uint64_t)kwords * j);
  uint4 lo = p[0], hi = make_uint4(0u, 0u, 0u, 0u);
  if (kwords == 8u) hi = p[1];
  k[0] = lo.x; k[1] = lo.y; k[2] = lo.z; k[3] = lo.w;
  k[4] = hi.x; k[5] = hi.y; k[6] = hi.z; k[7] = hi.w;
}

// group of bucket b in window w.  The digits of a window one bit narrower than the widest only reach B/2 buckets; its groups
// are half as wide so that they stay balanced.  A scalar >= 2^bits (outside the API contract) could exceed the top window's
// range: it is clamped into the last group (the result is then meaningless, but nothing is written out of bounds).
__device__ __forceinline__ uint32_t sort_gshift(const SortArgs& a, uint32_t w) { return a.lay.is_wide(w) ? a.gshift : a.gshift_narrow; }
__device__ __forceinline__ uint32_t sort_group(const SortArgs& a, uint32_t w, uint32_t b) {
  const uint32_t g = b >> sort_gshift(a, w);
  return g < a.NG ? g : a.NG - 1u;
}

// pass A, sweep 1: per-block counts of every (window, group), windows [w0, w0 + nw).  A thread holds PA_NS scalars in
// registers at a time and walks their digits window by window (for_each_digit).
static constexpr int PA_NS = 4;   // k_part_count
static constexpr int PS_NS = 4;   // k_part_scatter (measured at 2^22, 256 groups: 4, 6 and 8 scalars per thread all take 311 - 317 us;
                                  // 8 spills, and 4 is the fastest at 2^20)
template <int NS>
__device__ __forceinline__ void load_scalars(const SortArgs& a, uint32_t jb, uint32_t j1, uint32_t (&k)[NS][8]) {
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const uint32_t j = jb + (uint32_t)s * blockDim.x + threadIdx.x;
    if (j < j1) {
      load_scalar(a.scalars, a.kwords, j, k[s]);
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) k[s][q] = 0u;   // a zero scalar has no digits: no records
    }
  }
}
// Partition blocks and XCDs.  Consecutive slices of the scalars fill consecutive pieces of every group region: the 128-byte lines at
// the seams -- with 8 .. 32 records per (block, window, group) run that is most lines -- are written by two to four neighbouring
// blocks.  Workgroup b is dispatched to XCD b % 8 (observed placement, MI355X_MICROARCH.md; a speed matter only), each XCD has its
// own L2, and a line that two L2s each hold a part of goes to memory as partial writes (k_part_scatter wrote 1.55x / 5.0x its
// records at 2^22 / 2^24 pairs, profiles/pmc_r03_hbm_bytes_*).  So the slice a workgroup takes is chosen such that neighbouring
// slices sit on ONE XCD and are dispatched back to back: XCD x owns the contiguous run of slices [start_x, start_x + count_x).
__device__ __forceinline__ uint32_t part_slice_of_block(const SortArgs& a, uint32_t b, uint32_t nblk) {
  if (!a.xcd_map) return b;
  const uint32_t q = nblk >> 3, r = nblk & 7u, x = b & 7u;
  return x * q + (x < r ? x : r) + (b >> 3);
}
// The pair forms (msm_bodies.h sort_by_pairs): a thread holds PP_NS pairs of half scalars -- pair p = halves p and n/2 + p, the entries
// of the same numbers -- and walks both halves of each (for_each_digit_pair): 2 x PP_NS records per window step, the registers of PP_NS
// whole scalars.  A slice of `slice` half scalars is slice / 2 pairs: 2048 of them for the 512 blocks of a large MSM, two per lane.
#ifndef CTT_SORT_PAIR_NS
#define CTT_SORT_PAIR_NS 2
#endif
static constexpr int PP_NS = CTT_SORT_PAIR_NS;
template <int NS>
__device__ __forceinline__ void load_pairs(const SortArgs& a, uint32_t pb, uint32_t p1, uint32_t (&k)[NS][8]) {
  const uint4* sc = reinterpret_cast<const uint4*>(a.scalars);
  const uint32_t np = a.n >> 1;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const uint32_t p = pb + (uint32_t)s * blockDim.x + threadIdx.x;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;   // a zero pair has no digits: no records
    if (p < p1) {
      lo = sc[p];
      hi = sc[(uint64_t)np + p];
    }
    k[s][0] = lo.x; k[s][1] = lo.y; k[s][2] = lo.z; k[s][3] = lo.w;
    k[s][4] = hi.x; k[s][5] = hi.y; k[s][6] = hi.z; k[s][7] = hi.w;
  }
}
// the pairs [p0, p1) of slice blk
__device__ __forceinline__ void pair_slice(const SortArgs& a, uint32_t blk, uint32_t& p0, uint32_t& p1) {
  const uint32_t hs = a.slice >> 1, np = a.n >> 1;
  p0 = blk * hs < np ? blk * hs : np;
  p1 = (np - p0 > hs) ? p0 + hs : np;
}
template <bool PAIR>
__global__ void __launch_bounds__(512) k_part_count(SortArgs a, uint32_t w0, uint32_t nw) {
  extern __shared__ uint32_t lds[];
  const uint32_t ncnt = a.merged ? a.NG : nw * a.NG;  // merged: every digit window counts into the one set of groups
  const uint32_t wstep = a.merged ? 0u : a.NG;
  for (uint32_t i = threadIdx.x; i < ncnt; i += blockDim.x) lds[i] = 0;
  // the words the later kernels of this MSM accumulate into (largest bucket: k_group_sort; queue count: the head merge) start at
  // zero -- written here, by the first kernel of the sort, instead of by a fill launch of their own
  if (blockIdx.x == 0 && w0 == 0 && threadIdx.x < 4) a.maxcount[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t blk = part_slice_of_block(a, blockIdx.x, gridDim.x);
  auto count = [&](uint32_t w, const auto& d) {
    constexpr int NR = (int)std::extent<std::remove_reference_t<decltype(d)>>::value;
#pragma unroll
    for (int s = 0; s < NR; s++)
      if (d[s] != DIGIT_NONE) atomicAdd(&lds[(w - w0) * wstep + sort_group(a, w, d[s] >> 1)], 1u);
  };
  if constexpr (PAIR) {
    uint32_t p0, p1;
    pair_slice(a, blk, p0, p1);
    for (uint32_t pb = p0; pb < p1; pb += PP_NS * blockDim.x) {
      uint32_t k[PP_NS][8];
      load_pairs<PP_NS>(a, pb, p1, k);
      for_each_digit_pair<PP_NS>(k, w0, nw, a.lay, [&](uint32_t w, const uint32_t (&da)[PP_NS], const uint32_t (&db)[PP_NS]) {
        count(w, da);
        count(w, db);
      });
    }
  } else {
    const uint32_t j0 = blk * a.slice;
    const uint32_t j1 = (j0 + a.slice < a.n) ? j0 + a.slice : a.n;
    for (uint32_t jb = j0; jb < j1; jb += PA_NS * blockDim.x) {
      uint32_t k[PA_NS][8];
      load_scalars<PA_NS>(a, jb, j1, k);
      for_each_digit<PA_NS>(k, w0, nw, a.lay, [&](uint32_t w, const uint32_t (&d)[PA_NS]) { count(w, d); });
    }
  }
  __syncthreads();
  uint32_t* out = a.cntA + (uint64_t)blk * (a.W * a.NG) + (uint64_t)(a.merged ? 0u : w0) * a.NG;
  for (uint32_t i = threadIdx.x; i < ncnt; i += blockDim.x) out[i] = lds[i];
}

// column scan over the partition blocks: cntA[blk][col] -> exclusive prefix over blk (in place), gtot[col] = total.
// SCAN_CX columns x SCAN_RG row groups per workgroup.  (Rounds 1-3: 64 columns x 16 row groups -- ncol / 64 = 16 workgroups for
// the 2 MB of counts of a 2^20-pair MSM, 22 us of a 150 us sort on 16 of 256 CUs; 16 x 64 gives 64 workgroups of eight rows per lane.)
static constexpr uint32_t SCAN_CX = 16, SCAN_RG = 64;
__global__ void __launch_bounds__(1024) k_part_scan_blocks(uint32_t* __restrict__ cntA, uint32_t* __restrict__ gtot,
                                                           uint32_t ncol, uint32_t nblk) {
  __shared__ uint32_t part[SCAN_RG][SCAN_CX];
  const uint32_t cx = threadIdx.x % SCAN_CX, rg = threadIdx.x / SCAN_CX;
  const uint32_t col = blockIdx.x * SCAN_CX + cx;
  const uint32_t R = (nblk + SCAN_RG - 1u) / SCAN_RG;
  const uint32_t r0 = rg * R < nblk ? rg * R : nblk, r1 = (r0 + R < nblk) ? r0 + R : nblk;
  uint32_t sum = 0;
  if (col < ncol)
    for (uint32_t r = r0; r < r1; r++) sum += cntA[(uint64_t)r * ncol + col];
  part[rg][cx] = sum;
  __syncthreads();
  uint32_t run = 0, tot = 0;
  for (uint32_t g = 0; g < SCAN_RG; g++) {
    const uint32_t v = part[g][cx];
    if (g < rg) run += v;
    tot += v;
  }
  if (col < ncol) {
    for (uint32_t r = r0; r < r1; r++) {
      uint32_t* p = cntA + (uint64_t)r * ncol + col;
      const uint32_t v = *p;
      *p = run;
      run += v;
    }
    if (rg == 0) gtot[col] = tot;
  }
}

// per row (blockIdx.x): exclusive prefix of in[row][0..len) -> out[row][0..len], out[row][len] = total.
// One workgroup per row, 1024 elements per step (len is the number of groups: a few thousand at most).
__global__ void __launch_bounds__(1024) k_scan_u32(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t len) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t* src = in + (uint64_t)blockIdx.x * len;
  uint32_t* dst = out + (uint64_t)blockIdx.x * (len + 1);
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < len; b0 += 1024u) {
    const uint32_t b = b0 + tid;
    const uint32_t v = b < len ? src[b] : 0u;
    uint32_t x = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t base = carry_s;
    for (uint32_t k = 0; k < wv; k++) base += wsum[k];
    if (b < len) dst[b] = base + x - v;
    __syncthreads();
    if (tid == 1023) carry_s = base + x;
    __syncthreads();
  }
  if (tid == 0) dst[len] = carry_s;
}

// pass A, sweep 2: write the (entry, bucket) records into the block's runs of the group regions.  The block takes PS_NS x 1024
// scalars at a time into registers and walks the windows one after the other, so that at any moment it is filling only the
// NG runs of ONE window: the partially written lines are few and complete within a few hundred cycles (emitting all W
// records of a scalar at once kept W*NG runs open per block -- 8x the L2 at N = 2^22, 0.71 ms).  Round 2: the scalars used to
// be staged in LDS as [scalar][8 words], which made every digit two 16-way bank-conflicted LDS reads.
// PAIR: the slice is walked pair by pair (load_pairs above); records 0 .. PP_NS-1 of a step are the first halves, the others the second.
template <bool MERGED, bool PAIR = false>   // the table-less form keeps its register count (two workgroups per CU)
__global__ void __launch_bounds__(1024) k_part_scatter(SortArgs a, uint32_t w0, uint32_t nw) {
  static_assert(!(MERGED && PAIR), "half scalars have no window table");
  extern __shared__ uint32_t lds[];
  const uint32_t ncnt = MERGED ? a.NG : nw * a.NG;
  const uint32_t wstep = MERGED ? 0u : a.NG;
  uint32_t* cur = lds;                       // [ncnt] claim cursors
  const uint32_t set0 = MERGED ? 0u : w0;    // first bucket set this launch writes
  const uint32_t blk = part_slice_of_block(a, blockIdx.x, gridDim.x);
  const uint32_t* off = a.cntA + (uint64_t)blk * (a.W * a.NG) + (uint64_t)set0 * a.NG;
  for (uint32_t i = threadIdx.x; i < ncnt; i += blockDim.x) {
    const uint32_t w = i / a.NG, g = i - w * a.NG;
    cur[i] = off[i] + a.gbase[(uint64_t)(set0 + w) * (a.NG + 1) + g];
  }
  __syncthreads();
  const uint32_t sh = a.jbits + 1u;
  // one window step of the block: d[] the digits of the NR records a lane holds, id_of(s) their entries
  auto step = [&](uint32_t w, const auto& d, auto&& id_of) {
    constexpr int NR = (int)std::extent<std::remove_reference_t<decltype(d)>>::value;
    // the waves of the block move from window to window together (w is uniform over the block): the runs a block has open
    // at any moment are those of ONE window, and their partially written lines complete while they are still in the L2
    __syncthreads();
    uint32_t* cw = cur + (w - w0) * wstep;
    const uint32_t gmask = (1u << sort_gshift(a, w)) - 1u;
    // claim the NR positions first, store afterwards: a store issued between two claims makes the next claim's
    // address / data registers wait for it (s_waitcnt vmcnt(0) per record: 383 -> 588 us at 2^22 when it was written so)
    uint32_t pos[NR];
#pragma unroll
    for (int s = 0; s < NR; s++) pos[s] = d[s] != DIGIT_NONE ? atomicAdd(&cw[sort_group(a, w, d[s] >> 1)], 1u) : 0u;
    if constexpr (MERGED) {  // window table: 64-bit records, the entry is the table row w*id_stride + j
      uint64_t* pw = reinterpret_cast<uint64_t*>(a.part);
#pragma unroll
      for (int s = 0; s < NR; s++)
        if (d[s] != DIGIT_NONE)
          pw[pos[s]] = ((uint64_t)((d[s] >> 1) & gmask) << 32) | ((d[s] & 1u) << 31) | (w * a.id_stride + id_of(s));
    } else {
      uint32_t* pw = a.part + (uint64_t)w * a.nent;
#pragma unroll
      for (int s = 0; s < NR; s++)
        if (d[s] != DIGIT_NONE)
          pw[pos[s]] = (((d[s] >> 1) & gmask) << sh) | ((d[s] & 1u) << a.jbits) | id_of(s);
    }
  };
  if constexpr (PAIR) {
    uint32_t p0, p1;
    pair_slice(a, blk, p0, p1);
    const uint32_t np = a.n >> 1;
    for (uint32_t pb = p0; pb < p1; pb += PP_NS * blockDim.x) {
      uint32_t k[PP_NS][8];
      load_pairs<PP_NS>(a, pb, p1, k);
      const uint32_t id0 = pb + threadIdx.x;
      for_each_digit_pair<PP_NS>(k, w0, nw, a.lay, [&](uint32_t w, const uint32_t (&da)[PP_NS], const uint32_t (&db)[PP_NS]) {
        uint32_t d[2 * PP_NS];
#pragma unroll
        for (int s = 0; s < PP_NS; s++) { d[s] = da[s]; d[PP_NS + s] = db[s]; }
        step(w, d, [&](int s) { return (s < PP_NS ? id0 : np + id0) + (uint32_t)(s < PP_NS ? s : s - PP_NS) * blockDim.x; });
      });
    }
  } else {
    const uint32_t j0 = blk * a.slice;
    const uint32_t j1 = (j0 + a.slice < a.n) ? j0 + a.slice : a.n;
    for (uint32_t jb = j0; jb < j1; jb += PS_NS * blockDim.x) {
      uint32_t k[PS_NS][8];
      load_scalars<PS_NS>(a, jb, j1, k);
      const uint32_t id0 = jb + threadIdx.x;
      for_each_digit<PS_NS>(k, w0, nw, a.lay, [&](uint32_t w, const uint32_t (&d)[PS_NS]) {
        step(w, d, [&](int s) { return id0 + (uint32_t)s * blockDim.x; });
      });
    }
  }
}

// pass A, sweep 2, staged form (round 4).  The kernel above issues one 4-byte store per record straight from the lanes: a wave's
// store instruction touches up to 64 different lines, and what bounds it is the rate of such requests (63 M records in 311 us at
// 2^22 pairs: the 4-byte writes of a block land in NG runs, 16 of them per run and window step).  Here the 4096 records of a
// (window step) are first ranked inside their group with an LDS histogram, placed group by group into an LDS image of what the block
// is about to write, and written out by consecutive lanes: the records of one group go out as one contiguous piece (64 bytes at
// 2^22 pairs, 16 bytes at 2^24), a wave's store instruction touches a handful of lines, and the piece of a line arrives in one go.
// The block's write cursors live in its own row of cntA (advanced in place by the lane that owns the group): no LDS for
// W x NG cursors, so one launch walks all windows.  NG <= 1024 (one group per lane in the scan); beyond that the direct form runs.
template <bool MERGED, bool PAIR = false>   // PAIR: as in k_part_scatter
__global__ void __launch_bounds__(1024) k_part_scatter_staged(SortArgs a) {
  static_assert(!(MERGED && PAIR), "half scalars have no window table");
  extern __shared__ uint32_t lds[];
  using R = typename std::conditional<MERGED, uint64_t, uint32_t>::type;
  constexpr int NR = PAIR ? 2 * PP_NS : PS_NS;   // records a lane holds per window step
  constexpr uint32_t STEP = (uint32_t)NR * 1024u;
  const uint32_t NG = a.NG;
  uint32_t* hist = lds;                 // [NG] records of the current (step, window) per group
  uint32_t* lbase = hist + NG;          // [NG] first slot of the group in the stage
  uint32_t* gposd = lbase + NG;         // [NG] (position of the group's piece in the output) - lbase
  uint32_t* wsum = gposd + NG;          // [16]
  uint16_t* stage_g = reinterpret_cast<uint16_t*>(wsum + 16);   // [STEP] group of the record in slot i
  R* stage_rec = reinterpret_cast<R*>(stage_g + STEP);           // [STEP]
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t blk = part_slice_of_block(a, blockIdx.x, gridDim.x);
  uint32_t* cursor = a.cntA + (uint64_t)blk * (a.W * NG);   // [W][NG]: offset of the block's run inside the group -> absolute position
  if (tid < NG) {
    for (uint32_t set = 0; set < a.W; set++) cursor[set * NG + tid] += a.gbase[(uint64_t)set * (NG + 1) + tid];
    hist[tid] = 0;
  }
  const uint32_t sh = a.jbits + 1u;
  // one window step of the block: d[] the digits of the NR records a lane holds, id_of(s) their entries
  auto step = [&](uint32_t w, const uint32_t (&d)[NR], auto&& id_of) {
    const uint32_t set = MERGED ? 0u : w;
    const uint32_t gmask = (1u << sort_gshift(a, w)) - 1u;
    __syncthreads();   // the previous flush has read the stage; hist is zero again
    uint32_t g[NR], rk[NR];
#pragma unroll
    for (int s = 0; s < NR; s++) {
      g[s] = d[s] != DIGIT_NONE ? sort_group(a, w, d[s] >> 1) : 0u;
      rk[s] = d[s] != DIGIT_NONE ? atomicAdd(&hist[g[s]], 1u) : 0u;
    }
    __syncthreads();
    const uint32_t v = tid < NG ? hist[tid] : 0u;
    uint32_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t base = x - v, total = 0;
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      const uint32_t t = wsum[q];
      if (q < wv) base += t;
      total += t;
    }
    if (tid < NG) {
      lbase[tid] = base;
      uint32_t* cp = cursor + set * NG + tid;
      const uint32_t gp = *cp;
      gposd[tid] = gp - base;
      *cp = gp + v;
      hist[tid] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NR; s++)
      if (d[s] != DIGIT_NONE) {
        const uint32_t slot = lbase[g[s]] + rk[s];
        stage_g[slot] = (uint16_t)g[s];
        if constexpr (MERGED) {
          stage_rec[slot] = ((uint64_t)((d[s] >> 1) & gmask) << 32) | ((d[s] & 1u) << 31) | (w * a.id_stride + id_of(s));
        } else {
          stage_rec[slot] = (((d[s] >> 1) & gmask) << sh) | ((d[s] & 1u) << a.jbits) | id_of(s);
        }
      }
    __syncthreads();
    R* pw = reinterpret_cast<R*>(a.part) + (MERGED ? 0ull : (uint64_t)w * a.nent);
    for (uint32_t i = tid; i < total; i += 1024u) pw[gposd[stage_g[i]] + i] = stage_rec[i];
  };
  if constexpr (PAIR) {
    uint32_t p0, p1;
    pair_slice(a, blk, p0, p1);
    const uint32_t np = a.n >> 1;
    for (uint32_t pb = p0; pb < p1; pb += PP_NS * 1024u) {
      uint32_t k[PP_NS][8];
      load_pairs<PP_NS>(a, pb, p1, k);
      const uint32_t id0 = pb + tid;
      for_each_digit_pair<PP_NS>(k, 0u, a.Wd, a.lay, [&](uint32_t w, const uint32_t (&da)[PP_NS], const uint32_t (&db)[PP_NS]) {
        uint32_t d[NR];
#pragma unroll
        for (int s = 0; s < PP_NS; s++) { d[s] = da[s]; d[PP_NS + s] = db[s]; }
        step(w, d, [&](int s) { return (s < PP_NS ? id0 : np + id0) + (uint32_t)(s < PP_NS ? s : s - PP_NS) * 1024u; });
      });
    }
  } else {
    const uint32_t j0 = blk * a.slice;
    const uint32_t j1 = (j0 + a.slice < a.n) ? j0 + a.slice : a.n;
    for (uint32_t jb = j0; jb < j1; jb += STEP) {
      uint32_t k[PS_NS][8];
      load_scalars<PS_NS>(a, jb, j1, k);
      const uint32_t id0 = jb + tid;
      for_each_digit<PS_NS>(k, 0u, a.Wd, a.lay, [&](uint32_t w, const uint32_t (&d)[PS_NS]) {
        step(w, d, [&](int s) { return id0 + (uint32_t)s * 1024u; });
      });
    }
  }
}

// pass B: one workgroup per (bucket set, group).  MERGED (window table): 64-bit records, kept as (bucket, entry) pairs; the
// table-less form keeps the packed 32-bit record -- one register per record, two workgroups per CU.
template <bool MERGED>
__global__ void __launch_bounds__(1024) k_group_sort(SortArgs a) {
  extern __shared__ uint32_t lds[];
  __shared__ uint32_t wtot[16];
  __shared__ uint32_t wmax[16];
  __shared__ uint32_t any_big;
  __shared__ uint32_t next_tile;
  const uint32_t w = blockIdx.x / a.NG, g = blockIdx.x - w * a.NG;   // w = bucket set (0 when merged)
  const uint32_t gs = sort_gshift(a, w);
  const uint32_t Bg = 1u << gs;             // buckets of this group (<= B / NG <= GS_MAXBG)
  uint32_t* off = lds;                      // [Bg + 1] start of every bucket inside the group (after the scan)
  uint32_t* cur = lds + (Bg + 1);           // [Bg] claim cursors
  uint32_t* arr = cur + Bg;                 // [cap + big] LDS image of one output tile
  const uint32_t GS_CAP = a.cap, GS_BIG = a.big;
  const uint32_t* gb = a.gbase + (uint64_t)w * (a.NG + 1);
  const uint32_t beg = gb[g], ng = gb[g + 1] - beg;
  const uint32_t* rec = a.part + (uint64_t)w * a.nent + beg;                      // 32-bit records
  const uint64_t* rec64 = reinterpret_cast<const uint64_t*>(a.part) + beg;        // MERGED: 64-bit records
  uint32_t* ent = a.entries + (uint64_t)w * a.nent + beg;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t sh = a.jbits + 1u, jmask = (1u << a.jbits) - 1u;
  // a record as held in registers (R), its low bucket bits and its entry (point index or table row | sign << 31)
  using R = typename std::conditional<MERGED, uint64_t, uint32_t>::type;
  auto load = [&](uint32_t i) -> R { if constexpr (MERGED) return rec64[i]; else return rec[i]; };
  auto bucket_of = [&](R r) -> uint32_t { if constexpr (MERGED) return (uint32_t)(r >> 32); else return r >> sh; };
  auto entry_of = [&](R r) -> uint32_t {
    if constexpr (MERGED) return (uint32_t)r; else return (r & jmask) | (((r >> a.jbits) & 1u) << 31);
  };

  if (tid < Bg) cur[tid] = 0;
  if (tid == 0) any_big = 0;
  __syncthreads();
  // the records of an ordinary group (<= GS_RPT per lane) stay in registers between the two sweeps
  const bool in_regs = ng <= GS_RPT * 1024u;
  R rr[GS_RPT];
  uint32_t rk[GS_RPT];
  if (in_regs) {
#pragma unroll
    for (uint32_t q = 0; q < GS_RPT; q++) {
      const uint32_t i = q * 1024u + tid;
      if (i < ng) rr[q] = load(i);
    }
    // one atomic per record: the value it returns is the record's rank inside its bucket
#pragma unroll
    for (uint32_t q = 0; q < GS_RPT; q++)
      if (q * 1024u + tid < ng) rk[q] = atomicAdd(&cur[bucket_of(rr[q])], 1u);
  } else {
    for (uint32_t i = tid; i < ng; i += 1024u) atomicAdd(&cur[bucket_of(load(i))], 1u);
  }
  __syncthreads();
  // exclusive scan of the Bg <= 1024 counters, one per lane
  const uint32_t cnt = tid < Bg ? cur[tid] : 0u;
  uint32_t x = cnt, mx = cnt;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wtot[wv] = x;
#pragma unroll
  for (uint32_t o = 32; o >= 1; o >>= 1) {
    const uint32_t y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
  }
  if (lane == 0) wmax[wv] = mx;
  if (lane == 0 && mx > GS_BIG) any_big = 1;
  __syncthreads();
  uint32_t base = x - cnt;
  for (uint32_t k = 0; k < wv; k++) base += wtot[k];
  if (tid == 0) {  // one device-scope atomic per workgroup (they all hit the same word)
    uint32_t m = 0;
    for (uint32_t k = 0; k < 16; k++) m = wmax[k] > m ? wmax[k] : m;
    if (m) atomicMax(a.maxcount, m);
  }
  if (tid < Bg) {
    off[tid] = base;
    cur[tid] = base;
    a.bstart[(uint64_t)w * (a.B + 1) + ((uint64_t)g << gs) + tid] = beg + base;
  }
  if (tid == 0) off[Bg] = ng;
  if (g == a.NG - 1)  // buckets above the last group (top window) are empty; slot B holds the set's total
    for (uint32_t b = (a.NG << gs) + tid; b <= a.B; b += 1024u) a.bstart[(uint64_t)w * (a.B + 1) + b] = beg + ng;
  __syncthreads();
  if (a.zero_bytes) {
    // the empty buckets of this group become the neutral element (all zero); the others are written by the accumulation
    // and the head merge.  16-byte stores, consecutive lanes on consecutive chunks.
    const uint32_t CH = a.zero_bytes >> 4;
    uint4* zw = reinterpret_cast<uint4*>((char*)a.zero_base + (uint64_t)w * a.B * a.zero_bytes);
    uint4* zg = zw + ((uint64_t)g << gs) * CH;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = tid; i < Bg * CH; i += 1024u) {
      const uint32_t b = i / CH;
      if (off[b + 1] == off[b]) zg[i] = z4;
    }
    if (g == a.NG - 1)
      for (uint64_t i = (uint64_t)(a.NG << gs) * CH + tid; i < (uint64_t)a.B * CH; i += 1024u) zw[i] = z4;
  }

  if (in_regs && ng <= GS_CAP && !any_big) {
    // ordinary group: one tile, every slot of arr[0, ng) is claimed exactly once
#pragma unroll
    for (uint32_t q = 0; q < GS_RPT; q++)
      if (q * 1024u + tid < ng) arr[off[bucket_of(rr[q])] + rk[q]] = entry_of(rr[q]);
    __syncthreads();
    for (uint32_t p = tid; p < ng; p += 1024u) ent[p] = arr[p];
    return;
  }

  // General path (skewed digit distributions).  Buckets above GS_BIG go straight to HBM in one sweep: consecutive
  // claims of one counter are dense anyway.  The others go through the LDS image tile by tile; only tiles in which a
  // small bucket starts are visited.
  if (any_big) {
    for (uint32_t i = tid; i < ng; i += 1024u) {
      const R r = load(i);
      const uint32_t b = bucket_of(r);
      if (off[b + 1] - off[b] > GS_BIG) ent[atomicAdd(&cur[b], 1u)] = entry_of(r);
    }
  }
  const uint32_t my_cnt = tid < Bg ? off[tid + 1] - off[tid] : 0u;
  const uint32_t my_tile = (my_cnt > 0 && my_cnt <= GS_BIG) ? off[tid] / GS_CAP : 0xffffffffu;
  uint32_t t_prev = 0xffffffffu;  // "none yet"
  for (;;) {
    __syncthreads();
    if (tid == 0) next_tile = 0xffffffffu;
    __syncthreads();
    if (my_tile != 0xffffffffu && (t_prev == 0xffffffffu || my_tile > t_prev)) atomicMin(&next_tile, my_tile);
    __syncthreads();
    const uint32_t t = next_tile;
    if (t == 0xffffffffu) break;
    t_prev = t;
    const uint32_t tbase = t * GS_CAP;
    const uint32_t lim = (ng - tbase < GS_CAP + GS_BIG) ? ng - tbase : GS_CAP + GS_BIG;
    for (uint32_t p = tid; p < lim; p += 1024u) arr[p] = ENTRY_INVALID;
    __syncthreads();
    for (uint32_t i = tid; i < ng; i += 1024u) {
      const R r = load(i);
      const uint32_t b = bucket_of(r);
      const uint32_t o = off[b];
      if (off[b + 1] - o <= GS_BIG && o >= tbase && o - tbase < GS_CAP) arr[atomicAdd(&cur[b], 1u) - tbase] = entry_of(r);
    }
    __syncthreads();
    for (uint32_t p = tid; p < lim; p += 1024u) {
      const uint32_t v = arr[p];
      if (v != ENTRY_INVALID) ent[tbase + p] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// HipBackend out-of-line members
// ---------------------------------------------------------------------------------------------
void HipBackend::init(int dev) {
  device = dev;
  HIP_CHECK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  num_cu = prop.multiProcessorCount;
  {
    const char* e;
    if ((e = getenv("CTT_HIP_MSM_QUAD"))) quad_adds = (uint32_t)atoi(e);
    if ((e = getenv("CTT_HIP_MSM_TAIL"))) tail_adds = (uint32_t)atoi(e);
    cu_tail = (e = getenv("CTT_HIP_CU_TAIL")) ? atoi(e) : 0;
    if (cu_tail < 0 || XCDS * cu_tail >= num_cu || num_cu % XCDS != 0) cu_tail = 0;
    cu_main = cu_tail > 0 && !((e = getenv("CTT_HIP_CU_MAIN")) && atoi(e) == 0);
  }
  if (cu_tail > 0) {
    // the user mask is dealt round-robin over the XCDs: bit b -> XCD b mod 8, its (b div 8)-th CU (tools/cu_mask_probe.hip)
    const uint32_t words = ((uint32_t)num_cu + 31u) / 32u;
    std::vector<uint32_t> tail_mask(words, 0u), main_mask(words, 0u);
    for (int b = 0; b < num_cu; b++) (b < XCDS * cu_tail ? tail_mask : main_mask)[b / 32] |= 1u << (b % 32);
    HIP_CHECK(hipExtStreamCreateWithCUMask(&aux, words, tail_mask.data()));
    if (cu_main) HIP_CHECK(hipExtStreamCreateWithCUMask(&stream, words, main_mask.data()));
    else HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
  } else {
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
    // the tail stream outranks the main one: its short kernels must not queue behind the next MSM's conversion and sort
    int lo = 0, hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_CHECK(hipStreamCreateWithPriority(&aux, hipStreamNonBlocking, hi));
  }
  HIP_CHECK(hipStreamCreateWithFlags(&cpy, hipStreamNonBlocking));
  // The front stream IS the copy stream: a process gets four hardware queues (GPU_MAX_HW_QUEUES), and this context already has three
  // streams beside the null stream -- a fifth stream shares a hardware queue with one of the others.  Measured when the front stream was a
  // stream of its own: 2^16 pairs 0.52 -> 0.56 ms per MSM (the tail stream's overlap with the main stream is what a small pipelined MSM
  // lives on), with not a single kernel on the new stream.  The copy stream carries the uploads of host-pointer calls only; the front
  // stage is used by device-resident MSMs kept in flight: the two do not meet in one call, and stream order keeps them apart otherwise.
  srt = cpy;
  HIP_CHECK(hipEventCreateWithFlags(&ev_accum_done, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&ev_front_done, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&ev_copy, hipEventDisableTiming));
  for (int i = 0; i < MAX_CHUNKS; i++) HIP_CHECK(hipEventCreateWithFlags(&ev_slice[i], hipEventDisableTiming));
  for (int i = 0; i < MAX_CHUNKS; i++) HIP_CHECK(hipEventCreateWithFlags(&ev_coefs[i], hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&ev_tail_fork, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&ev_tail_done, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&ev_wide_done, hipEventDisableTiming));
  for (int s = 0; s < NSLOT; s++) {
    for (int i = 0; i < ST_COUNT; i++) {
      for (int ch = 0; ch < MAX_CHUNKS; ch++) {
        HIP_CHECK(hipEventCreate(&ev_begin[s][i][ch]));
        HIP_CHECK(hipEventCreate(&ev_end[s][i][ch]));
      }
      ev_used[s][i] = 0;
    }
    HIP_CHECK(hipEventCreateWithFlags(&ev_done[s], hipEventDisableTiming));
  }
  for (int i = 0; i < ST_COUNT; i++) stage_ms[i] = 0.f;
  no_tail = getenv("CTT_HIP_MSM_NO_TAIL") && atoi(getenv("CTT_HIP_MSM_NO_TAIL")) != 0;
  // k_group_sort keeps its counters and an image of the output tile in LDS
  HIP_CHECK(hipFuncSetAttribute((const void*)k_group_sort<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(GS_LDS_WORDS * 4)));
  HIP_CHECK(hipFuncSetAttribute((const void*)k_group_sort<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(GS_LDS_WORDS * 4)));
}

// what init() created, on the way out of ctt_hip_msm_ctx_destroy: quiet (a context lost to a HIP failure comes through here too)
void HipBackend::shutdown() noexcept {
  auto ev = [](hipEvent_t& e) {
    if (e && hipEventDestroy(e) != hipSuccess) (void)hipGetLastError();
    e = nullptr;
  };
  auto st = [](hipStream_t& s) {
    if (s && hipStreamDestroy(s) != hipSuccess) (void)hipGetLastError();
    s = nullptr;
  };
  if (!own_stream) return;
  ev(ev_accum_done); ev(ev_front_done); ev(ev_copy); ev(ev_tail_fork); ev(ev_tail_done); ev(ev_wide_done);
  for (int i = 0; i < MAX_CHUNKS; i++) { ev(ev_slice[i]); ev(ev_coefs[i]); }
  for (int s = 0; s < NSLOT; s++) {
    for (int i = 0; i < ST_COUNT; i++)
      for (int ch = 0; ch < MAX_CHUNKS; ch++) { ev(ev_begin[s][i][ch]); ev(ev_end[s][i][ch]); }
    ev(ev_done[s]);
  }
  srt = nullptr;   // (= cpy)
  st(cpy); st(aux); st(stream);
  own_stream = false;
}

bool HipBackend::sort_plan_in_range(const SortArgs& a) {
  if (a.NG == 0u || a.NG > 16384u || a.B / a.NG > GS_MAXBG) return false;
  if (2ull * (a.B / a.NG) + 1ull + (uint64_t)a.cap + (uint64_t)a.big > GS_LDS_WORDS) return false;
  if (!a.merged && a.jbits + 1u + a.gshift > 32u) return false;
  if (a.kwords != 8u && (a.kwords != 4u || a.lay.off(a.Wd - 1u) + a.lay.width(a.Wd - 1u) > 128)) return false;
  return !(a.merged && (a.W != 1 || a.gshift_narrow != a.gshift));
}

void HipBackend::launch_digits_sort(const SortArgs& a) {
  const uint32_t ncol = a.W * a.NG;
  if (!sort_plan_in_range(a)) {
    fprintf(stderr, "[ctt_msm_hip] FATAL: sort plan out of range (n = %u, c = %d, groups = %u)\n", a.n, a.c, a.NG);
    abort();
  }
  // pass A in window batches whose (window, group) counters fit 64 KiB of LDS; merged (window table): one launch walks all
  // Wd digit windows, its counters are the NG groups of the one bucket set
  uint32_t wb = a.merged ? a.Wd : 16384u / a.NG;
  if (wb < 1) wb = 1;
  if (wb > a.Wd) wb = a.Wd;
  // half scalars: the slices are walked pair by pair (msm_bodies.h sort_by_pairs)
  const bool pair = sort_by_pairs(a);
  for (uint32_t w0 = 0; w0 < a.Wd; w0 += wb) {
    const uint32_t nw = (w0 + wb <= a.Wd) ? wb : a.Wd - w0;
    const size_t lds_bytes = (a.merged ? a.NG : (size_t)nw * a.NG) * 4;
    if (pair) hipLaunchKernelGGL(k_part_count<true>, dim3(a.nblk), dim3(512), lds_bytes, front(), a, w0, nw);
    else hipLaunchKernelGGL(k_part_count<false>, dim3(a.nblk), dim3(512), lds_bytes, front(), a, w0, nw);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_part_scan_blocks, dim3((ncol + SCAN_CX - 1) / SCAN_CX), dim3(1024), 0, front(), a.cntA, a.gtot, ncol, a.nblk);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_scan_u32, dim3(a.W), dim3(1024), 0, front(), (const uint32_t*)a.gtot, a.gbase, a.NG);
  HIP_CHECK(hipGetLastError());
  if (a.staged && a.NG <= 1024u && (a.NG & (a.NG - 1u)) == 0u) {
    // one launch over all windows: records staged through LDS and written piece by piece (k_part_scatter_staged)
    const size_t rec = a.merged ? 8 : 4;
    const size_t lds_bytes = ((size_t)3 * a.NG + 16) * 4 + (size_t)(pair ? 2 * PP_NS : PS_NS) * 1024 * (2 + rec);
    if (a.merged) hipLaunchKernelGGL(k_part_scatter_staged<true>, dim3(a.nblk), dim3(1024), lds_bytes, front(), a);
    else if (pair) hipLaunchKernelGGL((k_part_scatter_staged<false, true>), dim3(a.nblk), dim3(1024), lds_bytes, front(), a);
    else hipLaunchKernelGGL(k_part_scatter_staged<false>, dim3(a.nblk), dim3(1024), lds_bytes, front(), a);
    HIP_CHECK(hipGetLastError());
  } else {
    for (uint32_t w0 = 0; w0 < a.Wd; w0 += wb) {
      const uint32_t nw = (w0 + wb <= a.Wd) ? wb : a.Wd - w0;
      if (a.merged) hipLaunchKernelGGL(k_part_scatter<true>, dim3(a.nblk), dim3(1024), (size_t)a.NG * 4, front(), a, w0, nw);
      else if (pair) hipLaunchKernelGGL((k_part_scatter<false, true>), dim3(a.nblk), dim3(1024), (size_t)nw * a.NG * 4, front(), a, w0, nw);
      else hipLaunchKernelGGL(k_part_scatter<false>, dim3(a.nblk), dim3(1024), (size_t)nw * a.NG * 4, front(), a, w0, nw);
      HIP_CHECK(hipGetLastError());
    }
  }
  const uint32_t Bg = a.B / a.NG;
  const size_t lds = ((size_t)2 * Bg + 1 + a.cap + a.big) * 4;  // Bg of the ordinary windows (the top window's is smaller)
  if (a.merged) hipLaunchKernelGGL(k_group_sort<true>, dim3(a.W * a.NG), dim3(1024), lds, front(), a);
  else hipLaunchKernelGGL(k_group_sort<false>, dim3(a.W * a.NG), dim3(1024), lds, front(), a);
  HIP_CHECK(hipGetLastError());
}
