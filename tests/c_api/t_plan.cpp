// Plan invariants of the MSM engine over the whole supported size range (host-only; no GPU, no kernels run).
// Build: g++ -std=c++17 -O1 -I constantine_amd/csrc tests/c_api/t_plan.cpp -o t_plan
// t_plan --dump prints every plan, the sort's sizing and buffer sizes, both window choosers and the slices of a host-pointer call over
// a fixed grid, one row per line: tests/test_plan_invariants.py pins the digest of that text (what a refactoring of the planning must
// leave as it is).
#include "msm_pipeline.h"
using namespace ctt;

static const unsigned long long sizes[] = {1, 2, 5, 63, 64, 65, 1000, 4096, 16383, 16384, 16385, 65536, 1ull << 20, (1ull << 20) + 7,
                                           1ull << 22, 1ull << 24, 1ull << 26, (1ull << 26) + 1, 1ull << 27, 1ull << 28, 1ull << 29,
                                           1ull << 30, (1ull << 31) - 1};

// ---- what the dump asks of the engine's headers beyond make_plan / make_table_plan and the two choosers ----
static SortArgs dump_sort_args(const MsmPlan& p, const MsmOptions& o, size_t bytes[6]) {
  SortArgs sa{};
  sort_sizing(sa, p, o);
  const SortBytes sb = sort_bytes(sa);
  const size_t b[6] = {sb.part, sb.cntA, sb.gtot, sb.gbase, sb.bstart, sb.entries};
  for (int i = 0; i < 6; i++) bytes[i] = b[i];
  return sa;
}
struct NoBackend {};
template <class C>
static std::vector<uint32_t> slices_of(uint32_t n, int want, bool scalars_only) {
  return MsmEngine<C, NoBackend>::host_slices(n, want, scalars_only);   // (the engine's own figures for its curve)
}
// ---- end ----

static void dump_plan(const char* tag, int bits, const MsmPlan& p, const MsmOptions& o) {
  size_t by[6];
  const SortArgs sa = dump_sort_args(p, o, by);
  printf("%s bits=%d lanes=%u oc=%d oK=%d oS=%d mc=%d hb=%d st=%d xcd=%d acc=%g | n=%u c=%d W=%d B=%u S=%u slice=%u NG=%u gs=%u gsn=%u lay=%d,%d jb=%u cap=%u big=%u K=%u G=%u "
         "Wd=%d merged=%u nent=%u ids=%u h=%d ngrp=%d msteps=%d lmax=%u", tag, bits, o.lanes, o.c, o.K, o.S, o.merge_chain, o.horner_bits,
         o.sort_staged, o.sort_xcd, o.acc_ns, p.n, p.c, p.W, p.B, p.S, p.slice, p.NG, p.gshift, p.gshift_narrow, p.lay.cb, p.lay.r, p.jbits, p.cap,
         p.big, p.K, p.G, p.Wd, p.merged, p.nent, p.id_stride, p.h, p.ngrp, p.merge_steps, p.merge_lmax);
  printf(" | sa n=%u c=%d lay=%d,%d W=%u B=%u Wd=%u merged=%u nent=%u ids=%u NG=%u gs=%u gsn=%u slice=%u nblk=%u jb=%u cap=%u big=%u xcd=%u staged=%u", sa.n,
         sa.c, sa.lay.cb, sa.lay.r, sa.W, sa.B, sa.Wd, sa.merged, sa.nent, sa.id_stride, sa.NG, sa.gshift, sa.gshift_narrow, sa.slice, sa.nblk, sa.jbits,
         sa.cap, sa.big, sa.xcd_map, sa.staged);
  printf(" | bytes %zu %zu %zu %zu %zu %zu\n", by[0], by[1], by[2], by[3], by[4], by[5]);
}
template <class C>
static void dump_slices(const char* curve) {
  for (unsigned long long n : sizes)
    for (int only = 0; only <= 1; only++)
      for (int want = 0; want <= 8; want++) {
        printf("slices %s n=%llu only=%d want=%d:", curve, n, only, want);
        for (uint32_t b : slices_of<C>((uint32_t)n, want, only != 0)) printf(" %u", b);
        printf("\n");
      }
}
static int dump() {
  for (int bits : {253, 254, 255}) {
    for (unsigned long long nn : sizes) {
      const uint32_t n = (uint32_t)nn;
      for (int c : {0, 2, 8, 13, 16, 17, 20})
        for (uint32_t lanes : {4096u, 131072u, 196608u})
          for (int K : {0, 7})
            for (int S : {0, 4096}) {
              MsmOptions o;
              o.c = c; o.lanes = lanes; o.K = K; o.S = S;
              dump_plan("plain", bits, make_plan(n, bits, o), o);
            }
      const int ctab = choose_table_window_bits(n, bits);
      printf("choose bits=%d n=%u: g1 %d %d %d g2 %d bn %d table %d\n", bits, n, choose_window_bits(n, bits, 4096), choose_window_bits(n, bits, 131072),
             choose_window_bits(n, bits, 196608), choose_window_bits(n, bits, 196608, Bls12381G2::TUNE.acc_ns, Bls12381G2::TUNE.red_ns),
             choose_window_bits(n, bits, 196608, Bn254G1::TUNE.acc_ns, Bn254G1::TUNE.red_ns), ctab);
      for (int c : {0, 4, 8, 13, 16, 20, 22}) {
        const int ct = c ? c : ctab;
        if (ct <= 0 || !table_plan_fits(n, bits, ct)) continue;
        for (int K : {0, 7})
          for (int S : {0, 4096}) {
            MsmOptions o;
            o.lanes = 131072; o.K = K; o.S = S;
            dump_plan(c ? "table" : "table-chosen", bits, make_table_plan(n, bits, ct, n, o), o);
          }
      }
    }
    // the merge form, the bit Horner's groups and the sort's options, both plan forms
    for (unsigned long long nn : {1000ull, 4096ull, 65536ull, 1ull << 20, (1ull << 22) + 77777, 1ull << 24})
      for (int mc = 0; mc <= 2; mc++)
        for (int hb : {0, 1, 4})
          for (int st = 0; st <= 2; st++)
            for (double acc : {0.142, 0.467}) {
              MsmOptions o;
              o.merge_chain = mc; o.horner_bits = hb; o.sort_staged = st; o.sort_xcd = st != 1; o.acc_ns = acc;
              dump_plan("plain-opt", bits, make_plan((uint32_t)nn, bits, o), o);
              o.merge_lmax = 16; o.host_window_sums = mc;
              dump_plan("table-opt", bits, make_table_plan((uint32_t)nn, bits, 16, (uint32_t)nn + 5, o), o);
            }
  }
  dump_slices<Bls12381G1>("bls12_381_g1");
  dump_slices<Bls12381G2>("bls12_381_g2");
  dump_slices<Bn254G1>("bn254_snarks_g1");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--dump")) return dump();
  MsmOptions o;
  o.lanes = 131072;
  int bad = 0;
  for (int bits : {253, 254, 255}) {
    for (unsigned long long n : sizes) {
      for (int c = 0; c <= 20; c++) {
        if (c == 1) continue;
        o.c = c;
        const MsmPlan p = make_plan((uint32_t)n, bits, o);
        // balanced windows over bits + 1 bits: r windows of cb + 1 bits, the others cb; c is the widest
        bool ok = p.c >= 2 && p.c <= (c == 0 ? 18 : 20) && (c == 0 || p.c <= c) && p.B == (1u << (p.c - 1));
        ok = ok && p.lay.cb * p.W + p.lay.r == bits + 1 && p.lay.r >= 0 && p.lay.r < p.W && p.c == p.lay.cmax();
        ok = ok && p.lay.off((uint32_t)p.W - 1) + p.lay.width((uint32_t)p.W - 1) == bits + 1 && p.lay.off(0) == 0;
        ok = ok && p.NG >= 1 && p.NG <= 4096 && p.NG <= p.B && (p.B >> p.gshift) == p.NG && p.B / p.NG <= 1024;
        ok = ok && p.jbits + 1 + p.gshift <= 32 && (1ull << p.jbits) >= n && p.gshift_narrow <= p.gshift;
        ok = ok && (unsigned long long)p.S * p.slice >= n && (unsigned long long)(p.S - 1) * p.slice < n;
        ok = ok && p.K >= 4 && (unsigned long long)p.G * p.K >= n && (unsigned long long)(p.G - 1) * p.K < n;
        // every reachable bucket of a narrower window (2^(cb-1) of them) has a group
        ok = ok && (p.lay.r == 0 || ((1ull << (p.lay.cb - 1)) >> p.gshift_narrow) <= p.NG);
        if (!ok) {
          bad++;
          printf("BAD bits=%d n=%llu c_req=%d -> c=%d W=%d B=%u NG=%u gshift=%u/%u jbits=%u slice=%u S=%u K=%u G=%u\n", bits, n, c,
                 p.c, p.W, p.B, p.NG, p.gshift, p.gshift_narrow, p.jbits, p.slice, p.S, p.K, p.G);
        }
      }
    }
  }
  // plan_entries_per_lane: K is the smallest one from ceil(W*n/lanes) (at least 4) on whose grid -- W rows of ceil(ceil(n/K)/64) workgroups --
  // fits the wave slots; with more rows than slots no K does (a row is at least one workgroup) and the search ends at its cap 0x7ffffff0
  for (uint32_t lanes : {64u, 128u, 256u, 4096u})
    for (int W : {1, 2, 3, 5, 43, 128})
      for (uint32_t n : {1u, 63u, 64u, 65u, 1000u, 4097u, 100000u}) {
        const uint64_t slots = lanes / 64u;
        auto fits = [&](uint64_t K) { return (uint64_t)W * (((n + K - 1) / K + 63u) / 64u) <= slots; };
        const uint32_t K = plan_entries_per_lane(n, W, lanes);
        uint64_t K0 = ((uint64_t)W * n + lanes - 1) / lanes;
        if (K0 < 4) K0 = 4;
        bool ok;
        if ((uint64_t)W > slots) ok = K == 0x7ffffff0u && !fits(K) && !fits(n);
        else {
          uint64_t want = K0;
          while (!fits(want)) want++;     // (ends: K = n leaves one workgroup per row)
          ok = K == want;
        }
        if (!ok) {
          bad++;
          printf("BAD entries per lane: n=%u W=%d lanes=%u -> K=%u\n", n, W, lanes, K);
        }
      }
  printf("%s\n", bad ? "FAILED" : "plans ok");
  return bad ? 1 : 0;
}
