// fixed_harness.cpp -- the bodies of csrc/fixed_bodies.h run lane by lane on the CPU, the way the kernels of csrc/fixed.hip run them:
// table lanes, lane sums, the tree over a plain array, the chunk partials and the finish; `finish` runs the finish alone over partials
// given to it, up to the 256 of a row (test infrastructure: tests/test_fixed_msm_cpu.py builds and feeds it).  usage: fixed_harness <mode>, binary little-endian input on stdin, binary output
// on stdout.  curve: 0 = BLS12-381 G1, 2 = BN254 G1 (the ids of include/ctt_msm_hip.h).
#define CTT_HOST_INLINE_BY_COMPILER 1   // (fp.h: the field arithmetic exists once per field instead of once per use)
#include <cstdio>
#include <cstring>
#include <vector>
#include "fixed_bodies.h"
using namespace ctt;

template <class T> static bool rd(T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, stdin) == n; }
static void wr(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }

// fx_tree of fixed.hip for `groups` groups of `lanes` lanes at once, group g in the region lds + g * 4 * F::N * SLOTS: at every level
// all lanes hand over, then all lanes merge, which is what the kernel's two barriers enforce.
template <class F, uint32_t SLOTS>
static __attribute__((noinline)) void tree(uint32_t* lds, XYZZ<F>* acc, uint32_t groups, uint32_t lanes, uint32_t first) {
  for (uint32_t s = first; s >= 1; s >>= 1) {
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t l = 0; l < lanes; l++) vk_tree_put<F, SLOTS>(lds + g * 4 * F::N * SLOTS, l, s, acc[g * lanes + l]);
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t l = 0; l < lanes; l++) fx_tree_take<F, SLOTS>(lds + g * 4 * F::N * SLOTS, l, s, acc[g * lanes + l]);
  }
}

template <class C>
struct Table {
  using F = typename C::F;
  FxTableArgs a;
  std::vector<uint32_t> pts, tab, pre;
  bool read_and_build(uint32_t n, int c) {
    pts.resize((size_t)n * 2 * F::N);
    if (!rd(pts.data(), pts.size())) return false;
    FxTable& t = a;
    int W;
    t.lay = window_layout(C::BITS, c, &W);
    t.n = n; t.W = (uint32_t)W; t.rows = vk_row_off(t.lay, t.W); t.stride = 2 * F::N;
    tab.assign((size_t)n * t.rows * t.stride, 0xA5A5A5A5u);
    pre.assign((size_t)n * t.rows * 3 * F::N, 0);
    t.tab = tab.data(); a.pts = pts.data(); a.pre = pre.data();
    for (uint32_t lane = 0; lane < n * t.W + 3; lane++) fx_table_body<F>(a, lane);   // (three lanes past the end: they must do nothing)
    return true;
  }
};

template <class C>
static int run_table() {            // in: n, c, n points.  out: W, rows, the table
  uint32_t n, c;
  Table<C> t;
  if (!rd(&n, 1) || !rd(&c, 1) || !t.read_and_build(n, (int)c)) return 1;
  wr(&t.a.W, 4); wr(&t.a.rows, 4); wr(t.tab.data(), t.tab.size() * 4);
  return 0;
}

// k_fx_finish, workgroup k0 / 4 (the last one may hold waves without a row): the lanes' strided sums of the partials, the tree over
// 4 x 64 lanes, one inversion per workgroup.  part: [m][chunks] XYZZ partials, out: [m] affine points, followed here by the rows of
// the waves without a row, which must stay as they were (a workgroup that wrote all four of its rows would write past `out`).
template <class F>
static int finish(const uint32_t* part, uint32_t m, uint32_t chunks, std::vector<uint32_t>& out) {
  using Pt = XYZZ<F>;
  const size_t words = (size_t)m * 2 * F::N;
  out.assign(words + FX_FINISH_ROWS * 2 * F::N, 0x5A5A5A5Au);
  const FxFinishArgs f{part, m, chunks, out.data()};
  std::vector<uint32_t> lds(FX_FINISH_ROWS * 4 * F::N * FX_FINISH_SLOTS), grp(FX_FINISH_ROWS * 4 * F::N), pre(FX_FINISH_ROWS * F::N);
  std::vector<Pt> lanes(FX_FINISH_ROWS * FX_WAVE);
  for (uint32_t k0 = 0; k0 < m; k0 += FX_FINISH_ROWS) {
    for (uint32_t l = 0; l < FX_FINISH_ROWS * FX_WAVE; l++) lanes[l] = fx_finish_lane_sum<F>(f, k0 + l / FX_WAVE, l % FX_WAVE);
    for (uint32_t l = 0; l < FX_FINISH_ROWS * FX_WAVE; l++)
      if (k0 + l / FX_WAVE >= m && !lanes[l].is_inf()) return 3;
    tree<F, FX_FINISH_SLOTS>(lds.data(), lanes.data(), FX_FINISH_ROWS, FX_WAVE, FX_FINISH_SLOTS);
    for (uint32_t wave = 0; wave < FX_FINISH_ROWS; wave++) fx_store_xyzz<F>(grp.data() + wave * (4 * F::N), lanes[wave * FX_WAVE]);
    fx_finish_group<F>(f, k0, m - k0 < FX_FINISH_ROWS ? m - k0 : FX_FINISH_ROWS, grp.data(), pre.data());
  }
  for (size_t t = words; t < out.size(); t++)
    if (out[t] != 0x5A5A5A5Au) return 4;
  out.resize(words);
  return 0;
}

template <class C>
static int run_msm() {              // in: n, c, fr, m, n points, m rows of n scalars.  out: m affine points
  using F = typename C::F;
  using Pt = XYZZ<F>;
  uint32_t n, c, fr, m;
  Table<C> t;
  if (!rd(&n, 1) || !rd(&c, 1) || !rd(&fr, 1) || !rd(&m, 1) || !t.read_and_build(n, (int)c)) return 1;
  std::vector<uint32_t> coefs((size_t)m * n * 8);
  if (!rd(coefs.data(), coefs.size())) return 1;
  const uint32_t chunks = (n + FX_BLOCK - 1) / FX_BLOCK;
  std::vector<uint32_t> part((size_t)m * chunks * 4 * F::N, 0x5A5A5A5Au), out;
  FxMsmArgs a;
  static_cast<FxTable&>(a) = t.a;
  a.coefs = coefs.data(); a.m = m; a.fr = (int)fr; a.chunks = chunks; a.part = part.data();
  {                                   // k_fx_msm, workgroup (row k, chunk s)
    std::vector<uint32_t> lds(4 * F::N * FX_TREE_SLOTS);
    std::vector<Pt> lanes(FX_BLOCK);
    for (uint32_t b = 0; b < m * chunks; b++) {
      const uint32_t k = b / chunks, s = b % chunks;
      for (uint32_t l = 0; l < FX_BLOCK; l++) lanes[l] = fx_lane_sum<F, typename C::Fr>(a, k, s * FX_BLOCK + l);
      tree<F, FX_TREE_SLOTS>(lds.data(), lanes.data(), 1, FX_BLOCK, FX_TREE_SLOTS);
      fx_store_xyzz<F>(a.part + (uint64_t)b * (4 * F::N), lanes[0]);
    }
  }
  if (int rc = finish<F>(part.data(), m, chunks, out)) return rc;
  wr(out.data(), out.size() * 4);
  return 0;
}

template <class C>
static int run_finish() {           // in: m, chunks, m * chunks XYZZ partials.  out: m affine points
  using F = typename C::F;
  uint32_t m, chunks;
  if (!rd(&m, 1) || !rd(&chunks, 1) || m < 1 || m > 4096 || chunks < 1 || chunks > FX_MAX_BASES / FX_BLOCK) return 1;
  std::vector<uint32_t> part((size_t)m * chunks * 4 * F::N), out;
  if (!rd(part.data(), part.size())) return 1;
  if (int rc = finish<F>(part.data(), m, chunks, out)) return rc;
  wr(out.data(), out.size() * 4);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  uint32_t curve;
  if (!rd(&curve, 1) || (curve != 0 && curve != 2)) return 2;
  if (!strcmp(argv[1], "table")) return curve == 0 ? run_table<Bls12381G1>() : run_table<Bn254G1>();
  if (!strcmp(argv[1], "msm")) return curve == 0 ? run_msm<Bls12381G1>() : run_msm<Bn254G1>();
  if (!strcmp(argv[1], "finish")) return curve == 0 ? run_finish<Bls12381G1>() : run_finish<Bn254G1>();
  return 2;
}
