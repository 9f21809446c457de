// ntt_plan.h -- which index bits each pass of the scalar-field NTT covers (plain host C++: the library's launch path and the CPU
// harness of tests/ntt_harness.cpp share it).
//
// A transform of n = 2^L elements runs L radix-2 stages, stage s pairing the indices that differ in bit s.  A pass keeps a tile in
// LDS between one global read and one global write of each element and runs up to T = tile_log2 stages there, so L > T takes
// ceil(L / T) passes.  Two orders of the stages:
//   DIF  natural order in, bit-reversed out: bits L-1 down to 0, the first pass covers the top T bits, the last one what is left
//   DIT  bit-reversed in, natural order out: bits 0 up to L-1, the first pass covers the low T bits
// The image of a pass holds 2^E elements, E <= T + NTT_EXTRA_LOG2:
//   lo == 0  the tile is 2^E neighbouring elements (E = min(T + 2, L)); the stages run on the low t bits of the local index, so a pass
//            of few stages still fills the workgroup
//   lo >  0  the pass walks the array with stride 2^lo: the image is 2^t rows of 2^x neighbouring columns, x = min(2, lo) -- four
//            elements of 32 bytes are one 128-byte line; local index = column | row << x
#pragma once
#include <stdint.h>

namespace ctt {

static constexpr int NTT_BLOCK = 256;          // lanes of a workgroup
static constexpr int NTT_MAX_TILE_LOG2 = 9;    // stages per pass at most: an image of 2^(9+2) elements is 64 KiB of LDS
static constexpr int NTT_DEFAULT_TILE_LOG2 = 8;
static constexpr int NTT_EXTRA_LOG2 = 2;       // columns per row of a strided pass (log2): 4 x 32 bytes = one 128-byte line
static constexpr int NTT_MAX_LOG2N = 24;
static constexpr int NTT_MAX_PASSES = NTT_MAX_LOG2N;   // (tile_log2 = 1)

// the flag bits of ctt_hip_fr_ntt (include/ctt_msm_hip.h, Part 5)
enum : int { NTT_FLAG_INVERSE = 1, NTT_FLAG_IN_BRP = 2, NTT_FLAG_OUT_BRP = 4, NTT_FLAG_IN_MONT = 8, NTT_FLAG_OUT_MONT = 16, NTT_FLAG_ALL = 31 };

struct NttPass {
  uint32_t lo;      // first index bit the pass covers
  uint32_t t;       // stages: bits lo .. lo + t - 1
  uint32_t x;       // log2 of the neighbouring columns per row (0 when lo == 0)
  uint32_t rows;    // log2 of the rows of the image: t for a strided pass, E when lo == 0
  uint32_t E;       // log2 of the image's elements = x + rows
  uint32_t sl;      // local index bit of the pass's first stage: x for a strided pass, 0 when lo == 0
};

// -> the number of passes, in the order they run
inline int ntt_plan_passes(int log2n, int tile_log2, bool dit, NttPass* out) {
  const int L = log2n, T = tile_log2;
  const int npass = (L + T - 1) / T;
  for (int p = 0; p < npass; p++) {
    NttPass q;
    if (dit) {
      q.lo = (uint32_t)(p * T);
      q.t = (uint32_t)(L - p * T < T ? L - p * T : T);
    } else {
      const int hi = L - p * T;
      q.t = (uint32_t)(hi < T ? hi : T);
      q.lo = (uint32_t)hi - q.t;
    }
    if (q.lo == 0) {
      q.x = 0;
      q.rows = (uint32_t)(T + NTT_EXTRA_LOG2 < L ? T + NTT_EXTRA_LOG2 : L);
      q.sl = 0;
    } else {
      q.x = q.lo < (uint32_t)NTT_EXTRA_LOG2 ? q.lo : (uint32_t)NTT_EXTRA_LOG2;
      q.rows = q.t;
      q.sl = q.x;
    }
    q.E = q.x + q.rows;
    out[p] = q;
  }
  return npass;
}

// the array index of local element m of tile `tile` (tile < 2^(L - E)) within its row of n elements
inline
#if defined(__HIPCC__)
    __host__ __device__
#endif
    uint32_t
    ntt_tile_index(const NttPass& q, uint32_t tile, uint32_t m) {
  const uint32_t nlow = q.lo - q.x;                               // tile bits below the rows (0 when lo == 0)
  const uint32_t tlow = tile & ((1u << nlow) - 1u), thigh = tile >> nlow;
  const uint32_t hs = q.lo + q.rows;                              // (may be 32 only when the tile count is 1: thigh == 0)
  return (m & ((1u << q.x) - 1u)) | (tlow << q.x) | ((m >> q.x) << q.lo) | (hs < 32u ? thigh << hs : 0u);
}

}  // namespace ctt
