// Placement trace of the MSM pipeline (host-only; no GPU, no kernels run): where and when MsmEngine asks its backend to run each stage.
// Build: g++ -std=c++17 -O1 -pthread -I constantine_amd/csrc tests/c_api/t_place.cpp -o t_place
// t_place [--small] drives MsmEngine<C, RecBackend> -- a backend that launches nothing and writes down what it is asked to do -- over a
// fixed grid of curves, lane counts, sizes, pipeline depths, options and backend shapes, one row per submit: the plan fields a placement
// decision feeds, then every launch, wait and mark in the order the engine issued it.  tests/test_placement_trace.py pins the digest of
// that text (what a refactoring of the placement decisions must leave as it is).  --small: the grid the test repeats once per environment
// knob (a knob is read once per process).
//
// The backend names only what every backend has to provide (HipBackend, tests/emu's EmuBackend) and keeps the five flags HipBackend keeps
// with the same transitions, so a wait or a mark is in the row exactly when the GPU backend would enqueue one.  Tokens:
//   frm convert glv_front d2d     scalar conversion, point conversion, the split's front kernel, a device copy (suffix f: front stream)
//   sort(k,m,z)                   digits + sort: words per scalar, window-table form, whether it clears the bucket set
//   accum(G,K,h,i)                accumulate: lanes per window, entries per lane, hand-over distance, into (continues stored sums)
//   mt ms<d> mf<d> / mtq mq4 mq1 mlong    head merge, tree form (tail, steps, finish) / queue form (quad or one lane per chain)
//   prio<0|1>  p<ntasks>  wg  d2h  reduction: narrow priority, one pass, window groups, result copy (suffix t: tail stream)
//   tail_begin tail_end tail_wait wide_mark wide_wait merge_mark front_begin[r] front_end accum_mark<0|1>   stream ordering
//   h2d<bytes> h2d_done cdone<i> cwait<i> sdone<i> swait<i> ub    uploads of a host-pointer call (|| up: the uploader thread's own log)
#include <sys/mman.h>

#include <string>

#include "msm_pipeline.h"
using namespace ctt;

// "Device" memory: addresses inside one reservation nothing may touch -- a host dereference of one crashes the harness.
struct Arena {
  static constexpr size_t BYTES = (size_t)1 << 42;
  char* base;
  size_t used = 0;
  Arena() {
    base = (char*)mmap(nullptr, BYTES, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) { perror("mmap"); exit(2); }
  }
  void* take(size_t b) {
    b = (b + 255u) & ~(size_t)255u;
    if (b == 0) b = 256;
    if (used + b > BYTES) { fprintf(stderr, "t_place: device arena exhausted\n"); exit(2); }
    void* p = base + used;
    used += b;
    return p;
  }
};
static Arena arena;

template <bool THREADED>
struct RecBackend {
  // what the harness sets
  bool part = false;              // HipBackend::partitioned()
  uint32_t tail_adds = 131072u;   // HipBackend::tail_adds
  // the five flags of HipBackend
  bool on_aux = false, tail_pending = false, wide_pending = false, on_front = false, accum_marked = false;
  std::string log, ulog;          // the submitting thread's and the uploader thread's
  std::thread::id owner = std::this_thread::get_id();
  unsigned allocs = 0;
  RecBackend() { arena.used = 0; }   // (one rig at a time: every scenario starts on an empty device)

  std::string& L() { return THREADED && std::this_thread::get_id() != owner ? ulog : log; }
  void tok(const std::string& s) { std::string& l = L(); if (!l.empty()) l += ' '; l += s; }
  void clear() { log.clear(); ulog.clear(); allocs = 0; }
  const char* tl() const { return on_aux ? "t" : ""; }
  const char* fr() const { return on_front ? "f" : ""; }

  void* alloc(size_t b) { allocs++; return arena.take(b); }
  void free(void*) {}
  void free_quiet(void*) noexcept {}
  void* alloc_host(size_t b) { return calloc(b ? b : 1, 1); }
  void free_host(void* p) { ::free(p); }
  void free_host_quiet(void* p) noexcept { ::free(p); }
  bool partitioned() const { return part; }
  bool tail_forked() const { return on_aux; }
  bool pyr_goes_to_tail(uint32_t ntasks, uint32_t W) const { return (uint64_t)ntasks * W <= tail_adds; }

  void tail_begin() { tok("tail_begin"); on_aux = true; }
  void tail_end() { tok("tail_end"); on_aux = false; tail_pending = true; }
  void tail_wait() {
    if (!tail_pending) return;
    tok("tail_wait");
    tail_pending = false;
    wide_pending = false;
  }
  void wide_mark() {
    if (!on_aux) return;
    tok("wide_mark");
    wide_pending = true;
  }
  void merge_mark() {
    if (!on_aux) return;
    tok("merge_mark");
    wide_pending = true;
  }
  void wide_wait() {
    if (!wide_pending) return;
    tok("wide_wait");
    wide_pending = false;
  }
  void front_begin() { tok(accum_marked ? "front_begin" : "front_beginr"); on_front = true; }
  void front_end() { tok("front_end"); on_front = false; }
  void front_abort() { on_front = false; accum_marked = false; }
  void accum_mark(bool wanted) { tok(wanted ? "accum_mark1" : "accum_mark0"); accum_marked = wanted; }

  void stage_begin(int, int) {}
  void stage_end(int, int) {}
  void stage_chunk(int) {}
  void sync() {}
  void memset0(void*, size_t) {}
  void launch_iota(uint32_t*, uint32_t, uint32_t*, uint32_t*) { tok("iota"); }
  void d2d_async(void*, const void*, size_t) { tok(std::string("d2d") + fr()); }
  void d2h_async(int, void*, const void*, size_t) { tok(std::string("d2h") + tl()); }
  void d2h_wait(int) {}
  void d2h_sync(void* dst, const void*, size_t b) { memset(dst, 0, b); tok("d2h_sync"); }

  static constexpr bool THREADED_UPLOAD = THREADED;
  struct GuardScope {};
  void uploader_begin() { tok("ub"); }
  [[noreturn]] void uploader_failed() { abort(); }
  void h2d(void*, const void*, size_t b) { tok("h2d" + std::to_string(b)); }
  void h2d_done() { tok("h2d_done"); }
  void h2d_slice_done(uint32_t i) { tok("sdone" + std::to_string(i)); }
  void h2d_slice_wait(uint32_t i) { tok("swait" + std::to_string(i)); }
  void h2d_coefs_done(uint32_t i) { tok("cdone" + std::to_string(i)); }
  void h2d_coefs_wait(uint32_t i) { tok("cwait" + std::to_string(i)); }

  template <class Fr>
  void launch_fr_from_mont(const uint32_t*, uint32_t*, uint32_t) { tok(std::string("frm") + fr()); }
  template <class F, class FD>
  void launch_convert(const Affine<F>*, void*, uint32_t) { tok(std::string("convert") + fr()); }
  static constexpr bool GLV_FRONT = true;
  template <class F, class FD>
  void launch_glv_front(const uint32_t*, const Affine<F>*, void*, uint32_t*, uint32_t) { tok(std::string("glv_front") + fr()); }
  template <class F>
  void launch_table_next(const Affine<F>*, Affine<F>*, uint32_t, int) {}
  void launch_digits_sort(const SortArgs& a) {
    tok("sort(k" + std::to_string(a.kwords) + ",m" + std::to_string(a.merged) + ",z" + (a.zero_base ? "1" : "0") + ")" + fr());
  }
  template <class F>
  void launch_accum(const AccumArgs<F>& a, uint32_t, bool into = false) {
    tok("accum(G" + std::to_string(a.G) + ",K" + std::to_string(a.K) + ",h" + std::to_string(a.handover) + ",i" + (into ? "1" : "0") + ")");
  }
  template <class F>
  void launch_merge_tail(const MergeArgs<F>&, uint32_t) { tok(std::string("mt") + tl()); }
  template <class F>
  void launch_merge_step(const MergeArgs<F>&, uint32_t, uint32_t d) { tok("ms" + std::to_string(d) + tl()); }
  template <class F>
  void launch_merge_finish(const MergeArgs<F>&, uint32_t, uint32_t d) { tok("mf" + std::to_string(d) + tl()); }
  template <class F>
  void launch_merge_tail_queue(const MergeArgs<F>&, uint32_t) { tok(std::string("mtq") + tl()); }
  template <class F>
  void launch_merge_queue(const MergeArgs<F>&, uint32_t, uint32_t, bool quad) { tok(std::string(quad ? "mq4" : "mq1") + tl()); }
  template <class F>
  void launch_merge_long(const MergeArgs<F>&, uint32_t, uint32_t) { tok(std::string("mlong") + tl()); }
  void narrow_priority(bool on) { tok(on ? "prio1" : "prio0"); }
  template <class F>
  void launch_pyr(const PyrArgs<F>&, uint32_t, uint32_t ntasks) { tok("p" + std::to_string(ntasks) + tl()); }
  template <class F>
  void launch_window_groups(const XYZZ<F>*, XYZZ<F>*, uint32_t, int, int, int) { tok(std::string("wg") + tl()); }
};

// ---- the grid ----
struct Opt { const char* name; int MsmOptions::*field; int value; };
static const Opt NO_OPT = {"-", nullptr, 0};
static const Opt OPTIONS[] = {
    {"early_tail=0", &MsmOptions::early_tail, 0},         {"early_tail=2", &MsmOptions::early_tail, 2},
    {"front_side=1", &MsmOptions::front_side, 1},         {"front_side=2", &MsmOptions::front_side, 2},
    {"pyr0_tail=1", &MsmOptions::pyr0_tail, 1},           {"glv=1", &MsmOptions::glv, 1},
    {"glv=2", &MsmOptions::glv, 2},                       {"accum_handover=0", &MsmOptions::accum_handover, 0},
    {"accum_handover=2", &MsmOptions::accum_handover, 2}, {"accum_handover=40", &MsmOptions::accum_handover, 40},
    {"merge_chain=1", &MsmOptions::merge_chain, 1},       {"merge_chain=2", &MsmOptions::merge_chain, 2},
    {"merge_queue_quad=2", &MsmOptions::merge_queue_quad, 2}, {"K=7", &MsmOptions::K, 7},
    {"c=13", &MsmOptions::c, 13},
    {"early_tail=2,front_side=1", &MsmOptions::early_tail, 2},   // (the pair: see Setup::apply)
};
static const uint32_t SIZES[] = {1u, 3000u, 1u << 12, 1u << 14, 1u << 16, 70000u, 1u << 17, (1u << 17) + 1u, 1u << 18, (1u << 18) + 5u,
                                 1u << 19, 1u << 20, 1u << 21, (1u << 21) + 1u, 1u << 22, 1u << 24};
static const uint32_t SIZES_FEW[] = {3000u, 1u << 16, (1u << 17) + 1u, 1u << 18, 1u << 20, 1u << 22};
static const uint32_t SIZES_SMALL[] = {1u << 12, 1u << 16, (1u << 17) + 1u, 1u << 18, 1u << 20, 1u << 22};
static const uint32_t SIZES_HOST[] = {1u, 1000u, 1u << 16, 1u << 18, 1u << 20, 1u << 22};
static const uint32_t LANES[] = {65536u, 131072u, 196608u, 262144u};
struct Shape { bool part; uint32_t tail_adds; };
static const Shape SHAPES[] = {{false, 131072u}, {false, 16384u}, {false, 0u}, {true, 131072u}, {true, 16384u}, {true, 0u}};
enum Bases { PLAIN = 0, RECORDS, TABLE13, TABLE20 };
static const char* const BASES_NAME[] = {"points", "records", "table13", "table20"};

struct Setup {
  uint32_t lanes;
  Opt opt = NO_OPT;
  Shape shape = SHAPES[0];
  bool fr = false;
  Bases bases = PLAIN;
  void apply(MsmOptions& o) const {
    o.lanes = lanes;
    if (opt.field) o.*opt.field = opt.value;
    if (!strcmp(opt.name, "early_tail=2,front_side=1")) o.front_side = 1;
  }
};

template <class C, bool THREADED>
struct Rig {
  using F = typename C::F;
  using BK = RecBackend<THREADED>;
  BK bk;
  MsmEngine<C, BK> eng;
  const char* curve;
  Setup su;
  const uint32_t* d_coefs;
  const Affine<F>* d_points;
  void* stage_coefs;
  void* stage_points;
  void* prepared = nullptr;
  int table_c = 0;
  uint32_t nmax;

  Rig(const char* curve_, const Setup& s, uint32_t nmax_) : eng(bk), curve(curve_), su(s), nmax(nmax_) {
    bk.part = s.shape.part;
    bk.tail_adds = s.shape.tail_adds;
    s.apply(eng.opt);
    d_coefs = (const uint32_t*)arena.take((size_t)nmax * 32);
    d_points = (const Affine<F>*)arena.take((size_t)nmax * sizeof(Affine<F>));
    stage_coefs = arena.take((size_t)nmax * 32);
    stage_points = arena.take((size_t)nmax * sizeof(Affine<F>));
    if (s.bases == RECORDS) prepared = eng.prepare_bases(d_points, nmax);
    if (s.bases == TABLE13 || s.bases == TABLE20) {
      prepared = eng.prepare_table(d_points, nmax, s.bases == TABLE13 ? 13 : 20, &table_c);
      if (!prepared) prepared = eng.prepare_bases(d_points, nmax);   // (no table to be had: plain records, as the library's bases_create does)
    }
    bk.clear();
  }
  int submit(uint32_t n) {
    return eng.submit(d_coefs, su.fr, prepared ? nullptr : d_points, n, prepared, table_c, nmax);
  }
  // (the "host" arrays are addresses of the reservation too: the engine hands them to the backend's copies and never reads them)
  int submit_host(uint32_t n, int chunks) {
    return eng.submit_host(d_coefs, su.fr, d_points, n, stage_coefs, stage_points, chunks, prepared, table_c, nmax);
  }
  void row(const char* what, uint32_t n, int ret, int chunks = -1) {
    printf("%s lanes=%u part=%d tail=%u fr=%d %s opt=%s %s n=%u", curve, su.lanes, (int)su.shape.part, su.shape.tail_adds, (int)su.fr,
           BASES_NAME[su.bases], su.opt.name, what, n);
    if (chunks >= 0) printf(" chunks=%d threaded=%d", chunks, (int)THREADED);
    printf(" -> slot=%d", ret);
    if (ret >= 0) {
      const MsmPlan& p = eng.last_plan;
      // K / the K of the same plan over every lane of the chip: how many lanes the plan was made for shows in the difference
      const uint32_t kfull = eng.opt.K > 0 ? (uint32_t)eng.opt.K : plan_entries_per_lane(p.nent, p.W, eng.opt.lanes);
      printf(" c=%d W=%d Wd=%d K=%u/%u G=%u glv=%u", p.c, p.W, p.Wd, p.K, kfull, p.G, p.glv);
      if (chunks >= 0) printf(" slices=%u", eng.last_chunks);
    }
    printf(" allocs=%u | %s", bk.allocs, bk.log.c_str());
    if (!bk.ulog.empty()) printf(" || up: %s", bk.ulog.c_str());
    printf("\n");
    bk.clear();
  }
};

// first, second and third submit without a finish; `full`: the fourth (refused), finishes out of order and the resubmits (slot choice)
template <class C>
static void depth_rows(const char* curve, const Setup& s, uint32_t n, bool full) {
  Rig<C, true> r(curve, s, n);
  int sl[3];
  static const char* const D[] = {"depth=1", "depth=2", "depth=3"};
  for (int i = 0; i < 3; i++) {
    sl[i] = r.submit(n);
    r.row(D[i], n, sl[i]);
  }
  if (full) {
    r.row("depth=4", n, r.submit(n));
    (void)r.eng.finish(sl[1]);
    const int a = r.submit(n);
    r.row("refill-after-2nd", n, a);
    (void)r.eng.finish(sl[0]);
    (void)r.eng.finish(a);
    const int b = r.submit(n);
    r.row("refill-after-1st", n, b);
    (void)r.eng.finish(b);
    const int c = r.submit(n);
    r.row("refill-again", n, c);
    (void)r.eng.finish(c);
  } else {
    (void)r.eng.finish(sl[0]);
    (void)r.eng.finish(sl[1]);
  }
  (void)r.eng.finish(sl[2]);
}
// three tickets of different sizes in flight (what one MSM leaves pending meets the next one's decisions), twice over
template <class C>
static void mixed_rows(const char* curve, const Setup& s, const uint32_t (&n)[3]) {
  Rig<C, true> r(curve, s, n[0] > n[1] ? (n[0] > n[2] ? n[0] : n[2]) : (n[1] > n[2] ? n[1] : n[2]));
  int sl[3];
  for (int rep = 0; rep < 2; rep++) {
    for (int i = 0; i < 3; i++) {
      sl[i] = r.submit(n[i]);
      r.row(rep ? "mixed-again" : "mixed", n[i], sl[i]);
    }
    (void)r.eng.finish(sl[2]);
    (void)r.eng.finish(sl[0]);
    (void)r.eng.finish(sl[1]);
  }
}
template <class C, bool THREADED>
static void host_rows(const char* curve, const Setup& s, uint32_t n, int chunks, bool behind) {
  Rig<C, THREADED> r(curve, s, n);
  int first = -1;
  if (behind) {
    first = r.submit_host(n, chunks);
    r.row("host", n, first, chunks);
  }
  const int sl = r.submit_host(n, chunks);
  r.row(behind ? "host-behind" : "host", n, sl, chunks);
  if (first >= 0) (void)r.eng.finish(first);
  (void)r.eng.finish(sl);
}
template <class C>
static void sum_rows(const char* curve, const Setup& s, uint32_t n) {
  Rig<C, true> r(curve, s, n);
  const int sl = r.submit(n);
  r.row("before-sum", n, sl);
  (void)r.eng.sum_reduce(r.d_points, n);
  r.row("sum_reduce", n, -9);
  (void)r.eng.finish(sl);
  (void)r.eng.sum_reduce(r.d_points, 1000);
  r.row("sum_reduce-idle", 1000, -9);
}

template <class C>
// every_size / every_chunk: the cross product is thinned for some curves, no axis is
static void full_grid(const char* curve, uint32_t real_lanes, bool every_size, bool every_chunk) {
  Setup base;
  base.lanes = real_lanes;
  // lane counts: the curve's own (with the refused fourth submit and the refills) and two others
  int others = 0;
  for (uint32_t lanes : LANES) {
    if (lanes != real_lanes && others++ >= 2) continue;
    Setup s = base;
    s.lanes = lanes;
    for (uint32_t n : SIZES) depth_rows<C>(curve, s, n, lanes == real_lanes);
  }
  // Montgomery coefficients
  {
    Setup s = base;
    s.fr = true;
    if (every_size) for (uint32_t n : SIZES) depth_rows<C>(curve, s, n, false);
    else for (uint32_t n : SIZES_FEW) depth_rows<C>(curve, s, n, false);
  }
  // cached bases: records, window tables
  for (Bases b : {RECORDS, TABLE13, TABLE20}) {
    Setup s = base;
    s.bases = b;
    if (every_size) for (uint32_t n : SIZES) depth_rows<C>(curve, s, n, false);
    else for (uint32_t n : SIZES_FEW) depth_rows<C>(curve, s, n, false);
  }
  // options, each alone
  for (const Opt& o : OPTIONS) {
    Setup s = base;
    s.opt = o;
    if (every_size) for (uint32_t n : SIZES) depth_rows<C>(curve, s, n, false);
    else for (uint32_t n : SIZES_FEW) depth_rows<C>(curve, s, n, false);
  }
  // backend shapes (the first is the default above)
  for (size_t i = 1; i < sizeof(SHAPES) / sizeof(SHAPES[0]); i++) {
    Setup s = base;
    s.shape = SHAPES[i];
    if (every_size) for (uint32_t n : SIZES) depth_rows<C>(curve, s, n, false);
    else for (uint32_t n : SIZES_FEW) depth_rows<C>(curve, s, n, false);
  }
  // the early tail wherever pipelining, on a partitioned chip and over a window table (the arms the automatic choice reaches at few sizes)
  for (int k = 0; k < 2; k++) {
    Setup s = base;
    s.opt = OPTIONS[1];
    if (k == 0) s.shape = SHAPES[3]; else s.bases = TABLE13;
    for (uint32_t n : SIZES_FEW) depth_rows<C>(curve, s, n, false);
  }
  // host-pointer calls
  for (Bases b : {PLAIN, RECORDS, TABLE13}) {
    Setup s = base;
    s.bases = b;
    for (uint32_t n : SIZES_HOST)
      for (int chunks = 0; chunks <= 8; chunks++) {
        if (!every_chunk && chunks != 0 && chunks != 2 && chunks != 3) continue;
        host_rows<C, true>(curve, s, n, chunks, false);
        host_rows<C, false>(curve, s, n, chunks, false);
      }
  }
  {
    Setup s = base;
    s.fr = true;
    for (uint32_t n : {1u << 16, 1u << 20}) host_rows<C, true>(curve, s, n, 0, true);
  }
  // different sizes in flight together; sum_reduce behind a pending tail
  static const uint32_t MIX[][3] = {{3000u, 70000u, (1u << 18) + 5u}, {1u << 20, 1u << 12, 1u << 20}, {1u << 22, 1u << 17, 1u << 19}};
  for (const auto& m : MIX) {
    mixed_rows<C>(curve, base, m);
    Setup s = base;
    s.opt = OPTIONS[15];
    mixed_rows<C>(curve, s, m);
  }
  for (uint32_t n : {1u << 12, 1u << 20}) sum_rows<C>(curve, base, n);
}

template <class C>
static void small_grid(const char* curve, uint32_t real_lanes) {
  Setup base;
  base.lanes = real_lanes;
  for (uint32_t n : SIZES_SMALL) depth_rows<C>(curve, base, n, false);
  for (uint32_t n : {1000u, 1u << 18, 1u << 20})
    for (int chunks : {0, 3}) {
      host_rows<C, true>(curve, base, n, chunks, false);
      host_rows<C, false>(curve, base, n, chunks, false);
    }
  Setup s = base;
  s.bases = RECORDS;
  host_rows<C, true>(curve, s, 1u << 20, 3, false);
  // (what the front stream's knob can switch off: the option asks for it)
  Setup f = base;
  f.opt = OPTIONS[2];
  for (uint32_t n : {1u << 16, 1u << 20}) depth_rows<C>(curve, f, n, false);
}

int main(int argc, char** argv) {
  const bool small = argc > 1 && !strcmp(argv[1], "--small");
  // the lanes the accumulate kernel of each curve keeps resident on a 256-CU chip: two waves per SIMD for BLS12-381 G1 (and, taken as such,
  // Banderwagon), one for the quadratic extensions, four for the 9-limb fields
  if (small) {
    small_grid<Bls12381G1>("bls12_381_g1", 131072u);
    small_grid<Bls12381G2>("bls12_381_g2", 65536u);
    small_grid<Bn254G1>("bn254_snarks_g1", 262144u);
    return 0;
  }
  full_grid<Bls12381G1>("bls12_381_g1", 131072u, true, true);
  full_grid<Bls12381G2>("bls12_381_g2", 65536u, true, false);
  full_grid<Bn254G1>("bn254_snarks_g1", 262144u, true, false);
  full_grid<Bn254G2>("bn254_snarks_g2", 65536u, false, false);
  full_grid<PallasEc>("pallas", 262144u, true, false);
  full_grid<VestaEc>("vesta", 262144u, false, false);
  full_grid<Banderwagon>("banderwagon", 131072u, false, false);
  return 0;
}
