// ntt_harness.cpp -- the bodies of the scalar-field NTT (constantine_amd/csrc/ntt_bodies.h) and its pass planner (ntt_plan.h) on the
// CPU: pass by pass, tile by tile, phase by phase and lane by lane over plain arrays, the way k_ntt_pass runs them between its
// barriers.  Built and driven by tests/test_ntt_cpu.py.
//
//   ntt_harness plan <log2n> <tile_log2> <dit>      one line per pass: lo t x rows E sl
//   ntt_harness ntt                                  stdin: 8 x u32 {field, log2n, tile_log2, batch, flags, has_shift, in_place, lanes},
//                                                    omega (32 bytes, canonical), shift (32 bytes, canonical), batch * n elements;
//                                                    stdout: batch * n elements
// field: 0 BLS12-381 Fr, 1 BN254-Snarks Fr, 2 Pallas' scalar field (Vesta's Fp), 3 Vesta's (Pallas' Fp), 4 Banderwagon Fr
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ntt_bodies.h"

using namespace ctt;

template <class Fr>
static Fr to_mont_bytes(const uint8_t* b) {
  Fr c;
  memcpy(c.l, b, 32);
  return Fr::to_mont(c);
}

template <class Fr>
static void powers(std::vector<uint32_t>& out, const Fr& base, const Fr& c0, uint32_t count) {
  out.assign((size_t)count * 8, 0xdeadbeefu);
  NttPowArgs<Fr> a{out.data(), base, c0, count, 16};
  const uint32_t lanes = (count + 15) / 16 + 3;   // (a few lanes past the end, as a grid rounded up to whole workgroups has)
  for (uint32_t l = 0; l < lanes; l++) ntt_powers_body<Fr>(a, l);
}

template <class Fr>
static int run_ntt(const uint32_t* h, const uint8_t* omega, const uint8_t* shift, std::vector<uint32_t>& data) {
  const int log2n = (int)h[1], tile_log2 = (int)h[2], flags = (int)h[4];
  const uint32_t batch = h[3], n = 1u << log2n, lanes = h[7];
  const bool inverse = flags & NTT_FLAG_INVERSE;
  std::vector<uint32_t> tw, mult;
  powers<Fr>(tw, to_mont_bytes<Fr>(omega), Fr::one(), n / 2);
  Fr nn = Fr::zero();
  nn.l[0] = n;
  const Fr ninv = Fr::inv(Fr::to_mont(nn));
  if (h[5]) {
    const Fr g = to_mont_bytes<Fr>(shift);
    if (inverse) powers<Fr>(mult, Fr::inv(g), ninv, n);
    else powers<Fr>(mult, g, Fr::one(), n);
  }
  std::vector<uint32_t> outbuf;
  uint32_t* out = data.data();
  if (!h[6]) {
    outbuf.assign(data.size(), 0xabababab);
    out = outbuf.data();
  }
  NttCall<Fr> c;
  ntt_setup<Fr>(c, log2n, tile_log2, flags, ninv, tw.data(), h[5] ? mult.data() : nullptr, out, data.data());
  const uint64_t total = (uint64_t)batch << log2n;
  std::vector<uint32_t> img;
  for (int k = 0; k < c.npass; k++) {
    const NttArgs<Fr> a = ntt_pass_args<Fr>(c, k);
    const uint32_t tiles = (uint32_t)(total >> a.pass.E);
    img.assign((size_t)8 << a.pass.E, 0xcdcdcdcd);
    for (uint32_t tile = 0; tile < tiles; tile++) {
      for (uint32_t l = 0; l < lanes; l++) ntt_tile_load<Fr>(a, img.data(), tile, l, lanes);
      for (uint32_t j = 0; j < a.pass.t; j++) {
        const uint32_t st = (a.flags & NTT_DIT) ? j : a.pass.t - 1 - j;
        for (uint32_t l = 0; l < lanes; l++) ntt_tile_stage<Fr>(a, img.data(), tile, st, l, lanes);
      }
      for (uint32_t l = 0; l < lanes; l++) ntt_tile_store<Fr>(a, img.data(), tile, l, lanes);
    }
  }
  if (c.swap)
    for (uint64_t i = 0; i < total + 5; i++) ntt_brp_swap_body<Fr>(out, (uint32_t)log2n, total, i);
  if (!h[6]) data = outbuf;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "plan")) {
    NttPass p[NTT_MAX_PASSES];
    const int np = ntt_plan_passes(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0, p);
    for (int i = 0; i < np; i++) printf("%u %u %u %u %u %u\n", p[i].lo, p[i].t, p[i].x, p[i].rows, p[i].E, p[i].sl);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "ntt")) {
    uint32_t h[8];
    uint8_t omega[32], shift[32];
    if (fread(h, 4, 8, stdin) != 8 || fread(omega, 1, 32, stdin) != 32 || fread(shift, 1, 32, stdin) != 32) return 2;
    if (h[1] < 1 || h[1] > 20 || h[2] < 1 || h[2] > (uint32_t)NTT_MAX_TILE_LOG2 || h[3] < 1 || h[3] > 64 || h[7] < 1) return 2;
    std::vector<uint32_t> data(((size_t)h[3] << h[1]) * 8);
    if (fread(data.data(), 4, data.size(), stdin) != data.size()) return 2;
    int rc = 2;
    switch (h[0]) {
      case 0: rc = run_ntt<Fp<BLS12_381_Fr>>(h, omega, shift, data); break;
      case 1: rc = run_ntt<Fp<BN254_Fr>>(h, omega, shift, data); break;
      case 2: rc = run_ntt<Fp<Vesta_Fp>>(h, omega, shift, data); break;
      case 3: rc = run_ntt<Fp<Pallas_Fp>>(h, omega, shift, data); break;
      case 4: rc = run_ntt<Fp<Banderwagon_Fr>>(h, omega, shift, data); break;
    }
    if (rc != 0) return rc;
    fwrite(data.data(), 4, data.size(), stdout);
    return 0;
  }
  fprintf(stderr, "usage: ntt_harness plan <log2n> <tile_log2> <dit> | ntt < case\n");
  return 2;
}
