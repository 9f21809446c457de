// verkle_harness.cpp -- the bodies of csrc/verkle_bodies.h and ed_madd_pre of csrc/ec.h run lane by lane on the CPU, the way the kernels
// of csrc/verkle.hip run them (test infrastructure: tests/_verkle.py builds it, tests/test_verkle_commit.py and test_verkle_update.py
// feed it).  usage: verkle_harness <mode>, binary little-endian input on stdin, binary output on stdout.
#include <cstdio>
#include <cstring>
#include <vector>
#include "verkle_bodies.h"
using namespace ctt;
using F = Banderwagon::F;
using Fr = Banderwagon::Fr;
using Pt = XYZZ<F>;

template <class T> static bool rd(T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, stdin) == n; }
static void wr(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }

// every large body is instantiated once (they inline all of the field arithmetic)
static __attribute__((noinline)) void finish_lanes(const VkFinishArgs& f) {
  for (uint32_t lane = 0; lane < (f.m + f.K - 1) / f.K + 2; lane++) vk_finish_body<F, Fr>(f, lane);   // (two lanes past the end: they must do nothing)
}

struct Table {
  VkTableArgs a;
  std::vector<uint32_t> pts, tab, pre;
  bool read_and_build(uint32_t n, int c) {
    pts.resize(n * 16);
    if (!rd(pts.data(), n * 16)) return false;
    VkTable& t = a;
    int W;
    t.lay = window_layout(Banderwagon::BITS, c, &W);
    t.n = n; t.W = (uint32_t)W; t.rows = vk_row_off(t.lay, t.W); t.stride = VK_REC_WORDS;
    tab.assign((size_t)n * t.rows * t.stride, 0xA5A5A5A5u);
    pre.assign((size_t)n * t.rows * 8, 0);
    t.tab = tab.data(); a.pts = pts.data(); a.pre = pre.data();
    for (uint32_t lane = 0; lane < n * t.W + 3; lane++) vk_table_body<F>(a, lane);   // (three lanes past the end: they must do nothing)
    return true;
  }
};

// out: prj m x 96, ser m x 32, fr m x 32 (0x5A where mask does not request it); -> the fr words
static std::vector<uint32_t> finish(const uint32_t* src, uint32_t stride, uint32_t m, uint32_t K, uint32_t mask) {
  std::vector<uint32_t> prj((size_t)m * 24, 0x5A5A5A5Au), ser((size_t)m * 8, 0x5A5A5A5Au), fr((size_t)m * 8, 0x5A5A5A5Au);
  finish_lanes(VkFinishArgs{src, stride, m, K, (mask & 1) ? prj.data() : nullptr, (mask & 2) ? ser.data() : nullptr, (mask & 4) ? fr.data() : nullptr});
  wr(prj.data(), prj.size() * 4); wr(ser.data(), ser.size() * 4); wr(fr.data(), fr.size() * 4);
  return fr;
}

// vk_tree of verkle.hip for `groups` groups of `lanes` lanes at once, group g in the region lds + g * VK_EXT_WORDS * SLOTS: at every
// level all lanes hand over, then all lanes merge, which is what the kernel's two barriers enforce.
template <uint32_t SLOTS>
static void tree(uint32_t* lds, Pt* acc, uint32_t groups, uint32_t lanes, uint32_t first) {
  for (uint32_t s = first; s >= 1; s >>= 1) {
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t l = 0; l < lanes; l++) vk_tree_put<F, SLOTS>(lds + g * VK_EXT_WORDS * SLOTS, l, s, acc[g * lanes + l]);
    for (uint32_t g = 0; g < groups; g++)
      for (uint32_t l = 0; l < lanes; l++) vk_tree_take<F, SLOTS>(lds + g * VK_EXT_WORDS * SLOTS, l, s, acc[g * lanes + l]);
  }
}
static constexpr uint32_t COMMIT_SLOTS = VK_MAX_BASES / 2;           // k_vk_commit: one group of 256 lanes
static constexpr uint32_t UPDATE_G = 64, UPDATE_ROWS = 4;            // k_vk_update: four groups of one wavefront
static constexpr uint32_t UPDATE_SLOTS = UPDATE_G / 2;
static constexpr uint32_t GUARD = 64, SENTINEL = 0xC0DEC0DEu;        // tree mode: words around the stand-in for LDS

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char* mode = argv[1];
  if (!strcmp(mode, "table")) {           // in: n, c, n points.  out: W, rows, the table
    uint32_t n, c;
    Table t;
    if (!rd(&n, 1) || !rd(&c, 1) || !t.read_and_build(n, (int)c)) return 1;
    wr(&t.a.W, 4); wr(&t.a.rows, 4); wr(t.tab.data(), t.tab.size() * 4);
  } else if (!strcmp(mode, "madd")) {     // in: count, count records (x, y, d*x*y).  out: the accumulator after every addition
    uint32_t cnt;
    if (!rd(&cnt, 1)) return 1;
    Pt acc = Pt::inf();
    bool empty = true;
    for (uint32_t i = 0; i < cnt; i++) {
      F q[3];
      if (!rd(q, 3)) return 1;
      ed_madd_pre<F>(acc, empty, q[0], q[1], q[2]);
      wr(&acc, sizeof(acc));
    }
  } else if (!strcmp(mode, "tree")) {     // in: slots (128 | 32), groups, lanes, first, groups x lanes extended points
    uint32_t slots, groups, lanes, first;   // out: lane 0 of every group, the guard words in front of and behind the slots
    if (!rd(&slots, 1) || !rd(&groups, 1) || !rd(&lanes, 1) || !rd(&first, 1)) return 1;
    if ((slots != COMMIT_SLOTS && slots != UPDATE_SLOTS) || first > slots || 2 * first > lanes) return 2;
    std::vector<Pt> acc((size_t)groups * lanes);
    if (!rd(acc.data(), acc.size())) return 1;
    const size_t words = (size_t)groups * VK_EXT_WORDS * slots;
    std::vector<uint32_t> lds(GUARD + words + GUARD, SENTINEL);
    if (slots == COMMIT_SLOTS) tree<COMMIT_SLOTS>(lds.data() + GUARD, acc.data(), groups, lanes, first);
    else tree<UPDATE_SLOTS>(lds.data() + GUARD, acc.data(), groups, lanes, first);
    for (uint32_t g = 0; g < groups; g++) wr(&acc[(size_t)g * lanes], sizeof(Pt));
    wr(lds.data(), GUARD * 4); wr(lds.data() + GUARD + words, GUARD * 4);
  } else if (!strcmp(mode, "commit")) {   // in: n, c, fr, m, n points, m rows of n scalars.  out: per row prj, then ser, then fr
    uint32_t n, c, fr, m;
    Table t;
    if (!rd(&n, 1) || !rd(&c, 1) || !rd(&fr, 1) || !rd(&m, 1) || !t.read_and_build(n, (int)c)) return 1;
    std::vector<uint32_t> coefs((size_t)m * n * 8), ext((size_t)m * VK_EXT_WORDS), lds(VK_EXT_WORDS * COMMIT_SLOTS);
    if (!rd(coefs.data(), coefs.size())) return 1;
    VkCommitArgs a{VkTable(t.a), coefs.data(), m, (int)fr, ext.data()};
    std::vector<Pt> lanes(VK_MAX_BASES);
    for (uint32_t k = 0; k < m; k++) {      // k_vk_commit, workgroup k
      for (uint32_t i = 0; i < VK_MAX_BASES; i++) lanes[i] = vk_lane_sum<F, Fr>(a, k, i);
      uint32_t live = 1;
      while (live < n) live <<= 1;
      tree<COMMIT_SLOTS>(lds.data(), lanes.data(), 1, VK_MAX_BASES, live >> 1);
      vk_store_ext<F>(a.out, k, lanes[0]);
    }
    finish(ext.data(), VK_EXT_WORDS, m, VK_FINISH_CHUNK, 7);
  } else if (!strcmp(mode, "finish")) {   // in: m, K, mask, m points (X, Y, Z).  out: prj, ser, fr (0x5A where not requested)
    uint32_t m, K, mask;
    if (!rd(&m, 1) || !rd(&K, 1) || !rd(&mask, 1)) return 1;
    std::vector<uint32_t> src((size_t)m * 24);
    if (!rd(src.data(), src.size())) return 1;
    finish(src.data(), 24, m, K, mask);
  } else if (!strcmp(mode, "update")) {   // in: n, c, fr, m, has_base, E, n points, row_ptr[m + 1], idx[E] (bytes), deltas[E][8], base[m][24] if has_base
    uint32_t n, c, fr, m, has_base, E;      // out: prj m x 96, ser m x 32, fr m x 32, dfr m x 32
    Table t;
    if (!rd(&n, 1) || !rd(&c, 1) || !rd(&fr, 1) || !rd(&m, 1) || !rd(&has_base, 1) || !rd(&E, 1) || !t.read_and_build(n, (int)c)) return 1;
    std::vector<uint32_t> row_ptr(m + 1), deltas((size_t)E * 8 + 1), base((size_t)m * 24 + 1);
    std::vector<uint8_t> idx(E + 1);
    if (!rd(row_ptr.data(), m + 1) || !rd(idx.data(), E) || !rd(deltas.data(), (size_t)E * 8)) return 1;
    if (has_base && !rd(base.data(), (size_t)m * 24)) return 1;
    std::vector<uint32_t> ext((size_t)m * VK_EXT_WORDS, 0x5A5A5A5Au), lds(UPDATE_ROWS * VK_EXT_WORDS * UPDATE_SLOTS);
    VkUpdateArgs a{VkTable(t.a), row_ptr.data(), idx.data(), deltas.data(), (int)fr, has_base ? base.data() : nullptr, m, ext.data()};
    std::vector<Pt> lanes(UPDATE_ROWS * UPDATE_G);
    for (uint32_t k0 = 0; k0 < m + UPDATE_ROWS; k0 += UPDATE_ROWS) {   // k_vk_update, workgroup k0 / 4 (and one whole workgroup past the end)
      for (uint32_t l = 0; l < UPDATE_ROWS * UPDATE_G; l++) lanes[l] = vk_update_lane_sum<F, Fr>(a, k0 + l / UPDATE_G, l % UPDATE_G, UPDATE_G);
      for (uint32_t l = 0; l < UPDATE_ROWS * UPDATE_G; l++)              // a wave without a row holds neutrals (and reads nothing)
        if (k0 + l / UPDATE_G >= m && !lanes[l].is_inf()) return 3;
      tree<UPDATE_SLOTS>(lds.data(), lanes.data(), UPDATE_ROWS, UPDATE_G, UPDATE_SLOTS);
      for (uint32_t wave = 0; wave < UPDATE_ROWS; wave++)
        if (k0 + wave < m) vk_update_store<F>(a, k0 + wave, lanes[wave * UPDATE_G]);
    }
    const std::vector<uint32_t> rfr = finish(ext.data(), VK_EXT_WORDS, m, VK_FINISH_CHUNK, 7);
    std::vector<uint32_t> bfr((size_t)m * 8), dfr((size_t)m * 8, 0x5A5A5A5Au);
    if (has_base) finish_lanes(VkFinishArgs{base.data(), 24u, m, VK_FINISH_CHUNK, nullptr, nullptr, bfr.data()});
    VkDeltaArgs d{rfr.data(), has_base ? bfr.data() : nullptr, m, dfr.data()};
    for (uint32_t lane = 0; lane < m + 2; lane++) vk_delta_body<Fr>(d, lane);
    wr(dfr.data(), dfr.size() * 4);
  } else {
    return 2;
  }
  return 0;
}
