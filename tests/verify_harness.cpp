// verify_harness.cpp -- EIP-7594 batch verification on the CPU: the host logic and the three kernel bodies of
// constantine_amd/csrc/verify_host.h, lane by lane over plain arrays, the inverse transform of 64 points between them run on the bodies
// of ntt_bodies.h as tests/recover_harness.cpp runs them, and the host pairing of pairing_host.h.  Built and driven by
// tests/test_peerdas_verify_cpu.py; all integers little-endian unless a wire format says otherwise.
//
//   verify_harness decompress   stdin: 4 x u32 {n, split, gap, subgroup?}, n x 48 compressed points
//                               stdout: n x u32 status, (n + gap) records of 96 bytes (affine Montgomery), n bytes: in the subgroup (0xff: not asked)
//   verify_harness colsum       stdin: u32 n, r (32 canonical bytes), n x u64 cell indices, n cells of 2048 bytes
//                               stdout: n x u32 bad, 64 canonical scalars: -c[i]
//   verify_harness challenge    stdin: 2 x u32 {m, n}, m x 48, n x u64 commitment indices, n x u64 cell indices, n cells, n x 48 proofs
//                               stdout: r, 32 big-endian bytes
//   verify_harness status       stdin: u32 n, 32 random bytes, n x 48 commitments, n x u64 cell indices, n cells, n x 48 proofs
//                               stdout: the status byte of every check before the MSMs; on Success r (32 big-endian bytes) and u32 M
//   verify_harness frobenius    stdout: xi^(k (p^2 - 1)/6), k = 1 .. 5, 48 canonical bytes each
//   verify_harness g2           stdin: 96 bytes            stdout: the status byte, x.c0 x.c1 y.c0 y.c1 as 48 canonical bytes each
//   verify_harness gt           stdin: u32 n, n x {x, y of G1; x.c0, x.c1, y.c0, y.c1 of G2} as 48 canonical bytes each, the neutral all zero
//                               stdout: the product of the n pairings: the coefficients of w^0 .. w^5, c0 then c1, 48 canonical bytes
//                               each; one byte: pairing_check
//   verify_harness verdict      stdin: LL (48), RL (48), [tau^64]_2 (96), compressed
//                               stdout: one byte: 0 when e(LL, [tau^64]_2) e(-RL, G_2) = 1, else 1; 0xff: a point was refused
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "verify_host.h"

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

// ctt_hip_fr_ntt on `batch` rows of 2^log2n elements without a shift, default tile, 256 lanes
static void ntt_cpu(int log2n, uint32_t batch, int flags, uint32_t* out, const uint32_t* in) {
  const uint32_t n = 1u << log2n, lanes = 256;
  std::vector<uint32_t> tw;
  powers(tw, dev(root_of_unity(log2n)), FrD::one(), n / 2);
  FrD nn = FrD::zero();
  nn.l[0] = n;
  const FrD ninv = FrD::inv(FrD::to_mont(nn));
  NttCall<FrD> c;
  ntt_setup<FrD>(c, log2n, 8, flags, ninv, tw.data(), nullptr, out, in);
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

// [r] P == neutral, by double-and-add in XYZZ on the host field (what ctt_hip_subgroup_check decides on the device)
static bool in_subgroup(const uint8_t* aff96) {
  const G1Aff p = g1_from_bytes(aff96);
  if (p.is_inf()) return true;
  const XYZZ<FpH> P = XYZZ<FpH>::from_affine(Affine<FpH>{p.x, p.y});
  XYZZ<FpH> acc = XYZZ<FpH>::inf();
  for (int i = 254; i >= 0; i--) {
    acc = xyzz_dbl<FpH>(acc);
    if ((FrH::P(i >> 6) >> (i & 63)) & 1) acc = xyzz_add_inl<FpH>(acc, P);
  }
  return acc.is_inf();
}

static bool read_all(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }

static void put_fp(const FpH& v) {
  uint64_t c[FpH::N];
  from_mont<FpH>(v, c);
  fwrite(c, 8, FpH::N, stdout);
}
static bool get_fp(FpH& v) {
  uint64_t c[FpH::N];
  if (!read_all(c, 48) || !below_modulus<FpH>(c)) return false;
  v = to_mont<FpH>(c);
  return true;
}

// colsum -> transform -> interp over validated indices; bad: n words; out: 64 Montgomery elements
static void interpolation(const uint64_t r[4], const uint64_t* idx, const uint8_t* cells, size_t n, std::vector<uint32_t>& bad, uint32_t* out) {
  std::vector<uint32_t> cidx(n, 0), order, hinv;
  std::vector<uint64_t> rho_r2, ll, rl;
  const std::vector<FrH> ck = cell_coset_constants(root_of_unity(13));
  verify_scalars(r, idx, cidx.data(), n, 1, ck, rho_r2, ll, rl);
  uint32_t start[N_CELLS + 1];
  verify_column_lists(idx, n, start, order);
  verify_hinv_table(hinv);
  std::vector<uint32_t> rows((size_t)VF_COLSUM_LANES * 8, 0xabababab);
  bad.assign(n, 0);
  VfColsumArgs ca{cells, (const uint32_t*)rho_r2.data(), start, order.data(), rows.data(), bad.data()};
  for (uint32_t l = 0; l < VF_COLSUM_LANES + 300; l++) vf_colsum_body(ca, l);   // (a few lanes past the end)
  ntt_cpu(6, N_CELLS, NTT_FLAG_INVERSE | NTT_FLAG_IN_BRP | NTT_FLAG_IN_MONT | NTT_FLAG_OUT_MONT, rows.data(), rows.data());
  VfInterpArgs ia{rows.data(), hinv.data(), out};
  for (uint32_t l = 0; l < 256; l++) vf_interp_body(ia, l);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: verify_harness decompress | colsum | challenge | status | frobenius | g2 | gt | verdict < case\n");
    return 2;
  }
  const char* cmd = argv[1];
  if (!strcmp(cmd, "decompress")) {
    uint32_t h[4];
    if (!read_all(h, 16) || h[0] > (1u << 16) || h[1] > h[0] || h[2] > 1024) return 2;
    const uint32_t n = h[0], split = h[1], gap = h[2];
    std::vector<uint8_t> in((size_t)n * 48 + 1);
    if (!read_all(in.data(), (size_t)n * 48)) return 2;
    std::vector<uint32_t> out((size_t)(n + gap) * 24, 0xabababab), status(n, 0xabababab);
    VfDecompressArgs a{in.data(), out.data(), status.data(), n, split, gap};
    for (uint32_t l = 0; l < n + 300; l++) vf_decompress_body(a, l);
    std::vector<uint8_t> sub(n, 0xff);
    if (h[3])
      for (uint32_t i = 0; i < n; i++) sub[i] = in_subgroup((const uint8_t*)&out[(size_t)(i + (i >= split ? gap : 0)) * 24]) ? 1 : 0;
    fwrite(status.data(), 4, n, stdout);
    fwrite(out.data(), 4, out.size(), stdout);
    fwrite(sub.data(), 1, n, stdout);
    return 0;
  }
  if (!strcmp(cmd, "colsum")) {
    uint32_t n;
    uint64_t r[4];
    if (!read_all(&n, 4) || n > 4096 || !read_all(r, 32)) return 2;
    std::vector<uint64_t> idx(n + 1);
    std::vector<uint8_t> cells((size_t)n * 2048 + 1);
    if (!read_all(idx.data(), 8 * (size_t)n) || !read_all(cells.data(), (size_t)n * 2048)) return 2;
    for (uint32_t k = 0; k < n; k++)
      if (idx[k] >= (uint64_t)N_CELLS) return 2;
    std::vector<uint32_t> bad;
    uint32_t out[CELL_ELEMS * 8];
    interpolation(r, idx.data(), cells.data(), n, bad, out);
    fwrite(bad.data(), 4, n, stdout);
    for (int i = 0; i < CELL_ELEMS; i++) {
      FrH m;
      memcpy(m.l, out + 8 * i, 32);
      uint64_t c[4];
      from_mont<FrH>(m, c);
      fwrite(c, 8, 4, stdout);
    }
    return 0;
  }
  if (!strcmp(cmd, "challenge")) {
    uint32_t h[2];
    if (!read_all(h, 8) || h[0] > 4096 || h[1] > 4096) return 2;
    const size_t m = h[0], n = h[1];
    std::vector<uint8_t> com(m * 48 + 1), cells(n * 2048 + 1), proofs(n * 48 + 1);
    std::vector<uint64_t> cidx(n + 1), idx(n + 1);
    if (!read_all(com.data(), m * 48) || !read_all(cidx.data(), 8 * n) || !read_all(idx.data(), 8 * n) || !read_all(cells.data(), n * 2048) ||
        !read_all(proofs.data(), n * 48))
      return 2;
    std::vector<uint8_t> t;
    verify_transcript(t, com.data(), m, cidx.data(), idx.data(), cells.data(), proofs.data(), n);
    Sha256 s;
    s.update(t.data(), t.size());
    uint8_t d[32], be[32];
    s.finish(d);
    uint64_t r[4];
    reduce_256_mod_r(d, r);
    limbs_to_be<FrH>(r, be);
    fwrite(be, 1, 32, stdout);
    return 0;
  }
  if (!strcmp(cmd, "status")) {
    uint32_t n32;
    uint8_t rnd[32];
    if (!read_all(&n32, 4) || n32 > 4096 || !read_all(rnd, 32)) return 2;
    const size_t n = n32;
    std::vector<uint8_t> com(n * 48 + 1), cells(n * 2048 + 1), proofs(n * 48 + 1);
    std::vector<uint64_t> idx(n + 1);
    if (!read_all(com.data(), n * 48) || !read_all(idx.data(), 8 * n) || !read_all(cells.data(), n * 2048) || !read_all(proofs.data(), n * 48)) return 2;
    uint8_t st = (uint8_t)verify_check_arguments(true, com.data(), idx.data(), cells.data(), proofs.data(), rnd, n);
    if (st != KZG_Success || n == 0) {
      fwrite(&st, 1, 1, stdout);
      return 0;
    }
    std::vector<uint32_t> cidx;
    std::vector<uint8_t> uniq;
    verify_dedup(com.data(), n, cidx, uniq);
    const size_t M = uniq.size() / 48, npts = M + n;
    std::vector<uint8_t> in(uniq);
    in.insert(in.end(), proofs.begin(), proofs.begin() + n * 48);
    std::vector<uint32_t> pts((npts + CELL_ELEMS) * 24, 0), status(npts, 0xabababab);
    VfDecompressArgs da{in.data(), pts.data(), status.data(), (uint32_t)npts, (uint32_t)M, (uint32_t)CELL_ELEMS};
    for (uint32_t l = 0; l < npts + 300; l++) vf_decompress_body(da, l);
    std::vector<uint8_t> ok(npts);
    for (size_t i = 0; i < npts; i++) ok[i] = in_subgroup((const uint8_t*)&pts[(i + (i >= M ? CELL_ELEMS : 0)) * 24]) ? 1 : 0;
    uint64_t r[4];
    if (!verify_blinding(r, rnd)) {
      std::vector<uint8_t> t;
      verify_transcript(t, uniq.data(), M, cidx.data(), idx.data(), cells.data(), proofs.data(), n);
      Sha256 s;
      s.update(t.data(), t.size());
      uint8_t d[32];
      s.finish(d);
      reduce_256_mod_r(d, r);
    }
    std::vector<uint32_t> bad;
    uint32_t out[CELL_ELEMS * 8];
    interpolation(r, idx.data(), cells.data(), n, bad, out);
    st = (uint8_t)verify_first_offender(status.data(), ok.data(), M, bad.data(), n);
    fwrite(&st, 1, 1, stdout);
    if (st == KZG_Success) {
      uint8_t be[32];
      limbs_to_be<FrH>(r, be);
      fwrite(be, 1, 32, stdout);
      const uint32_t m32 = (uint32_t)M;
      fwrite(&m32, 4, 1, stdout);
    }
    return 0;
  }
  if (!strcmp(cmd, "frobenius")) {
    for (int k = 1; k <= 5; k++) put_fp(frobenius2_constant(k));
    return 0;
  }
  if (!strcmp(cmd, "g2")) {
    uint8_t in[96], aff[192];
    if (!read_all(in, 96)) return 2;
    const uint8_t st = (uint8_t)g2_decompress(aff, in);
    fwrite(&st, 1, 1, stdout);
    if (st == KZG_Success) {
      const G2Aff q = g2_from_bytes(aff);
      put_fp(q.x.c0);
      put_fp(q.x.c1);
      put_fp(q.y.c0);
      put_fp(q.y.c1);
    }
    return 0;
  }
  if (!strcmp(cmd, "gt")) {
    uint32_t n;
    if (!read_all(&n, 4) || n > 16) return 2;
    std::vector<G1Aff> P(n);
    std::vector<G2Aff> Q(n);
    for (uint32_t i = 0; i < n; i++)
      if (!get_fp(P[i].x) || !get_fp(P[i].y) || !get_fp(Q[i].x.c0) || !get_fp(Q[i].x.c1) || !get_fp(Q[i].y.c0) || !get_fp(Q[i].y.c1)) return 2;
    Fp12H f = Fp12H::one();
    for (uint32_t i = 0; i < n; i++) miller_loop_into(f, P[i], Q[i]);
    const Fp12H e = final_exponentiation(f);
    for (int k = 0; k < 6; k++) {
      put_fp(e.at(k).c0);
      put_fp(e.at(k).c1);
    }
    const uint8_t ok = pairing_check(P.data(), Q.data(), n) ? 1 : 0;
    if ((ok == 1) != Fp12H::eq(e, Fp12H::one())) return 4;
    fwrite(&ok, 1, 1, stdout);
    return 0;
  }
  if (!strcmp(cmd, "verdict")) {
    uint8_t in[192], ll[96], rl[96], g2[192];
    if (!read_all(in, 192)) return 2;
    uint8_t out = 0xff;
    if (g1_decompress(ll, in) == KZG_Success && g1_decompress(rl, in + 48) == KZG_Success && g2_decompress(g2, in + 96) == KZG_Success) {
      G1Aff P[2] = {g1_from_bytes(ll), g1_from_bytes(rl)};
      P[1].y = FpH::neg(P[1].y);
      const G2Aff Q[2] = {g2_from_bytes(g2), g2_generator()};
      out = pairing_check(P, Q, 2) ? 0 : 1;
    }
    fwrite(&out, 1, 1, stdout);
    return 0;
  }
  return 2;
}
