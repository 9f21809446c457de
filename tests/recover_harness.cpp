// recover_harness.cpp -- EIP-7594 recovery on the CPU: the host logic and the three kernel bodies of constantine_amd/csrc/recover_host.h,
// lane by lane over plain arrays, between the transforms of ntt_bodies.h / ntt_plan.h run as tests/ntt_harness.cpp runs them -- the seven
// steps of recover.hip with the flags it passes to ctt_hip_fr_ntt.  Built and driven by tests/test_peerdas_recover_cpu.py.
//
//   recover_harness check | consts | recover     stdin: 2 x u32 {n, B}, n x u64 cell indices, then (check, recover) B * n cells of 2048 bytes
//     check    stdout: one status byte
//     consts   stdout: zc[128], izc5[128] as canonical little-endian scalars (the indices are taken as valid)
//     recover  stdout: the status byte; on Success B * 8192 canonical little-endian coefficients, B x u32 (1: the high half is zero),
//              B blobs of 131072 bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "recover_host.h"

using namespace ctt;
using namespace ctt::proto;

static void powers(std::vector<uint32_t>& out, const FrD& base, const FrD& c0, uint32_t count) {
  out.assign((size_t)count * 8, 0xdeadbeefu);
  NttPowArgs<FrD> a{out.data(), base, c0, count, 16};
  for (uint32_t l = 0; l < (count + 15) / 16 + 3; l++) ntt_powers_body<FrD>(a, l);
}

static FrD dev(const FrH& h) {
  FrD d;
  memcpy(d.l, h.l, 32);
  return d;
}

// ctt_hip_fr_ntt on `batch` rows of 2^log2n elements, default tile, 256 lanes
static void ntt_cpu(int log2n, uint32_t batch, int flags, const FrD* shift, uint32_t* out, const uint32_t* in) {
  const uint32_t n = 1u << log2n, lanes = 256;
  const bool inverse = flags & NTT_FLAG_INVERSE;
  std::vector<uint32_t> tw, mult;
  powers(tw, dev(root_of_unity(log2n)), FrD::one(), n / 2);
  FrD nn = FrD::zero();
  nn.l[0] = n;
  const FrD ninv = FrD::inv(FrD::to_mont(nn));
  if (shift) {
    if (inverse) powers(mult, FrD::inv(*shift), ninv, n);
    else powers(mult, *shift, FrD::one(), n);
  }
  NttCall<FrD> c;
  ntt_setup<FrD>(c, log2n, 8, flags, ninv, tw.data(), shift ? mult.data() : nullptr, out, in);
  const uint64_t total = (uint64_t)batch << log2n;
  std::vector<uint32_t> img;
  for (int k = 0; k < c.npass; k++) {
    const NttArgs<FrD> a = ntt_pass_args<FrD>(c, k);
    const uint32_t tiles = (uint32_t)(total >> a.pass.E);
    img.assign((size_t)8 << a.pass.E, 0xcdcdcdcd);
    for (uint32_t tile = 0; tile < tiles; tile++) {
      for (uint32_t l = 0; l < lanes; l++) ntt_tile_load<FrD>(a, img.data(), tile, l, lanes);
      for (uint32_t j = 0; j < a.pass.t; j++) {
        const uint32_t st = (a.flags & NTT_DIT) ? j : a.pass.t - 1 - j;
        for (uint32_t l = 0; l < lanes; l++) ntt_tile_stage<FrD>(a, img.data(), tile, st, l, lanes);
      }
      for (uint32_t l = 0; l < lanes; l++) ntt_tile_store<FrD>(a, img.data(), tile, l, lanes);
    }
  }
  if (c.swap)
    for (uint64_t i = 0; i < total + 5; i++) ntt_brp_swap_body<FrD>(out, (uint32_t)log2n, total, i);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: recover_harness check | consts | recover < case\n");
    return 2;
  }
  const bool check = !strcmp(argv[1], "check"), consts = !strcmp(argv[1], "consts"), recover = !strcmp(argv[1], "recover");
  uint32_t h[2];
  if (!(check || consts || recover) || fread(h, 4, 2, stdin) != 2 || h[0] > 4096 || h[1] > 64) return 2;
  const size_t n = h[0], B = h[1];
  std::vector<uint64_t> idx(n + 1);
  if (n && fread(idx.data(), 8, n, stdin) != n) return 2;
  FrH zc[N_CELLS], izc5[N_CELLS];
  int32_t slot[N_CELLS];
  if (consts) {
    recovery_constants(idx.data(), n, zc, izc5, slot);
    for (const FrH* t : {zc, izc5})
      for (int k = 0; k < N_CELLS; k++) {
        uint64_t v[4];
        from_mont<FrH>(t[k], v);
        fwrite(v, 8, 4, stdout);
      }
    return 0;
  }
  std::vector<uint8_t> cells(B * n * 2048 + 1);
  if (B * n && fread(cells.data(), 2048, B * n, stdin) != B * n) return 2;
  const uint8_t st = (uint8_t)recover_validate(idx.data(), cells.data(), n, B);
  fwrite(&st, 1, 1, stdout);
  if (check || st != KZG_Success || B == 0) return 0;

  recovery_constants(idx.data(), n, zc, izc5, slot);
  std::vector<uint32_t> zcr2(N_CELLS * 8), iz(N_CELLS * 8);
  for (int k = 0; k < N_CELLS; k++) {
    const FrH t = to_mont<FrH>(zc[k].l);
    memcpy(&zcr2[8 * k], t.l, 32);
    memcpy(&iz[8 * k], izc5[k].l, 32);
  }
  const uint32_t nb = (uint32_t)B, lanes = nb * N_EXT + 300;   // (a few lanes past the end, as a grid of whole workgroups may have)
  std::vector<uint32_t> rows((size_t)nb * N_EXT * 8, 0xabababab), coef((size_t)nb * N_BLOB * 8, 0xabababab), high(nb, 0);
  uint64_t five[4] = {RC_COSET_SHIFT, 0, 0, 0};
  const FrD g = dev(to_mont<FrH>(five));
  // 1. the received evaluations times Z
  RcLoadArgs la{cells.data(), zcr2.data(), slot, rows.data(), (uint32_t)n, nb};
  for (uint32_t l = 0; l < lanes; l++) rc_load_body(la, l);
  // 2. - 5. (E Z) -> coefficients -> the coset 5 <omega> -> / Z -> the coefficients of P
  ntt_cpu(13, nb, NTT_FLAG_INVERSE | NTT_FLAG_IN_BRP | NTT_FLAG_IN_MONT | NTT_FLAG_OUT_MONT, nullptr, rows.data(), rows.data());
  ntt_cpu(13, nb, NTT_FLAG_IN_MONT | NTT_FLAG_OUT_BRP | NTT_FLAG_OUT_MONT, &g, rows.data(), rows.data());
  RcScaleArgs sa{rows.data(), iz.data(), nb};
  for (uint32_t l = 0; l < lanes; l++) rc_scale_body(sa, l);
  ntt_cpu(13, nb, NTT_FLAG_INVERSE | NTT_FLAG_IN_BRP | NTT_FLAG_IN_MONT | NTT_FLAG_OUT_MONT, &g, rows.data(), rows.data());
  // 6. the low half, and whether the high half is zero; then the test-facing form on a copy
  RcSplitArgs pa{rows.data(), coef.data(), high.data(), nb, 0};
  for (uint32_t l = 0; l < lanes; l++) rc_split_body(pa, l);
  std::vector<uint32_t> high2(nb, 0);
  RcSplitArgs ca{rows.data(), nullptr, high2.data(), nb, 1};
  for (uint32_t l = 0; l < lanes; l++) rc_split_body(ca, l);
  if (high2 != high) return 4;
  // 7. back to the blob's evaluations
  ntt_cpu(12, nb, NTT_FLAG_IN_MONT | NTT_FLAG_OUT_BRP, nullptr, coef.data(), coef.data());
  fwrite(rows.data(), 4, rows.size(), stdout);
  for (uint32_t b = 0; b < nb; b++) {
    const uint32_t ok = high[b] ? 0u : 1u;
    fwrite(&ok, 4, 1, stdout);
  }
  std::vector<uint8_t> blob((size_t)N_BLOB * 32);
  for (uint32_t b = 0; b < nb; b++) {
    for (int i = 0; i < N_BLOB; i++) {
      uint64_t v[4];
      memcpy(v, &coef[((size_t)b * N_BLOB + i) * 8], 32);
      limbs_to_be<FrH>(v, &blob[32 * i]);
    }
    fwrite(blob.data(), 1, blob.size(), stdout);
  }
  return 0;
}
