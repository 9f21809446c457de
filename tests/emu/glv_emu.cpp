// tests/emu/glv_emu.cpp -- TEST INFRASTRUCTURE ONLY: the CPU emulator (msm_emu.cpp, included as it is, BLS12-381 G1) with what the endomorphism split
// of that curve adds to a backend: the front body in place of the conversion and a digit sort that reads 4-word scalars.  A library of its own
// (tests/test_glv_split.py builds it), so that the emulator of every other test stays what it was: a backend without the front stage, on which the
// engine runs every MSM on the plain path (MsmEngine::kGlv).
// Build: g++ -O1 -std=c++17 -shared -fPIC -I constantine_amd/csrc tests/emu/glv_emu.cpp -o tests/emu/build/libglv_emu.so
#define EMU_CURVE 0
#include "msm_emu.cpp"

struct GlvEmuBackend : EmuBackend {
  static constexpr bool GLV_FRONT = true;
  // the front kernel of the split (msm_bodies.h glv_front_body): records of s1 P and s2 phi(P), the two half scalars
  template <class F, class FD>
  void launch_glv_front(const uint32_t* scalars, const Affine<F>* in, void* out, uint32_t* half, uint32_t n) {
    for (uint32_t j = 0; j < n; j++) glv_front_body<F, FD>(scalars, in, out, half, n, j);
  }
  // 4-word scalars (SortArgs::kwords): the sort kernels read the upper four words as zero -- here the scalars are widened and the emulator's sort
  // (which walks them with the kernels' for_each_digit and checks every digit against the plain form) runs on those
  void launch_digits_sort(const SortArgs& a) {
    if (a.kwords == 8u) return EmuBackend::launch_digits_sort(a);
    if (a.kwords != 4u) abort();
    std::vector<uint32_t> wide((size_t)a.n * 8u, 0u);
    for (uint32_t j = 0; j < a.n; j++)
      for (int q = 0; q < 4; q++) wide[8ull * j + q] = a.scalars[4ull * j + q];
    SortArgs b = a;
    b.scalars = wide.data();
    b.kwords = 8u;
    EmuBackend::launch_digits_sort(b);
  }
};

extern "C" {
// one MSM through MsmEngine<Bls12381G1, GlvEmuBackend>; glv = MsmOptions::glv (1 = the split at every size, 2 = never); the other arguments as
// emu_msm's.  plan_out: c, bucket sets, K, G, S, split ran, digit windows
int emu_glv_msm(int coef_is_fr, int out_kind, void* r, const void* coefs, const void* points, size_t n, int c, int K, int S, int glv, int* plan_out) {
  using C = Bls12381G1;
  using F = C::F;
  GlvEmuBackend bk;
  MsmEngine<C, GlvEmuBackend> eng(bk);
  eng.opt.c = c;
  eng.opt.K = K;
  eng.opt.S = S;
  eng.opt.lanes = 4096;
  emu_env_options(eng.opt);
  eng.opt.glv = glv;
  const int s0 = eng.submit((const uint32_t*)coefs, coef_is_fr != 0, (const Affine<F>*)points, (uint32_t)n);
  auto res = eng.finish(s0);
  write_result<typename MsmEngine<C, GlvEmuBackend>::HF>(r, res, out_kind);
  if (plan_out && n) {
    const MsmPlan& p = eng.last_plan;
    plan_out[0] = p.c; plan_out[1] = p.W; plan_out[2] = (int)p.K; plan_out[3] = (int)p.G; plan_out[4] = (int)p.S;
    plan_out[5] = (int)p.glv; plan_out[6] = p.Wd;
  }
  return 0;
}
// three MSMs in flight over two input sets (A, B, A), finished in order: the records, the half scalars and the canonical scalars are shared by the
// slots.  r3 = 3 affine results; returns the number of refused submits
int emu_glv_msm_slots(void* r3, const void* coefs_a, const void* points_a, size_t na, const void* coefs_b, const void* points_b, size_t nb, int coef_is_fr) {
  using C = Bls12381G1;
  using F = C::F;
  using HF = typename MsmEngine<C, GlvEmuBackend>::HF;
  GlvEmuBackend bk;
  MsmEngine<C, GlvEmuBackend> eng(bk);
  eng.opt.lanes = 4096;
  eng.opt.glv = 1;
  const int t0 = eng.submit((const uint32_t*)coefs_a, coef_is_fr != 0, (const Affine<F>*)points_a, (uint32_t)na);
  const int t1 = eng.submit((const uint32_t*)coefs_b, coef_is_fr != 0, (const Affine<F>*)points_b, (uint32_t)nb);
  const int t2 = eng.submit((const uint32_t*)coefs_a, coef_is_fr != 0, (const Affine<F>*)points_a, (uint32_t)na);
  if (t0 < 0 || t1 < 0 || t2 < 0) return 1;
  const int t[3] = {t0, t1, t2};
  for (int i = 0; i < 3; i++) write_result<HF>((char*)r3 + (size_t)i * sizeof(Affine<F>), eng.finish(t[i]), OUT_AFF);
  return 0;
}
// the front body alone (msm_bodies.h glv_front_body), the CPU twin of ctt_hip_glv_front_probe: n canonical scalars [n][8] and n affine points in,
// records [2n][gather_stride] and half scalars [2n][4] out.  shape (may be NULL): gather_stride, gather_flag_offset, limbs per coordinate, limb bits
int emu_glv_front(const uint32_t* scalars, const void* points, uint32_t n, void* records, uint32_t* half, uint32_t* shape) {
  using C = Bls12381G1;
  using F = C::F;
  using FD = C::FD;
  if (shape) {
    shape[0] = gather_stride<FD>(); shape[1] = gather_flag_offset<FD>(); shape[2] = (uint32_t)FD::NL; shape[3] = (uint32_t)FD::LB;
  }
  for (uint32_t j = 0; j < n; j++) glv_front_body<F, FD>(scalars, (const Affine<F>*)points, records, half, n, j);
  return 0;
}
// the split body (msm_bodies.h bls12_381_glv_split) of n scalars of 8 words: out[j] = k1 (4 words), k2 (4 words), neg1, neg2
int emu_glv_split(const uint32_t* scalars, uint32_t n, uint32_t* out) {
  for (uint32_t j = 0; j < n; j++) {
    const GlvHalves h = bls12_381_glv_split(scalars + 8ull * j);
    for (int i = 0; i < 4; i++) {
      out[10ull * j + i] = h.k1[i];
      out[10ull * j + 4 + i] = h.k2[i];
    }
    out[10ull * j + 8] = h.neg1 ? 1u : 0u;
    out[10ull * j + 9] = h.neg2 ? 1u : 0u;
  }
  return 0;
}
}
