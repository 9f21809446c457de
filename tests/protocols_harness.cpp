// protocols_harness.cpp -- the host logic of the protocol symbols (constantine_amd/csrc/protocols_host.h) as a stand-alone program:
// the wire-format parsers, the hash, the host formulas and the body of the cell-quotient kernel, lane by lane, with no GPU runtime.
// Built and driven by tests/test_protocols_host.py; the program to build with sanitizers (README).
//
// One command per run, its input on stdin, its output on stdout.  Exit status 0 when the command ran (a rejected input is an
// answer: its status byte), 2 for a wrong command line or an input of the wrong length.
//   sha256          bytes -> 32
//   decompress      48 -> status, then 96 (affine Montgomery) on Success
//   compress        96 -> 48
//   blob            131072 -> status, then 4096 x 32 canonical little-endian scalars on Success
//   challenge       131072 (blob) + 48 (commitment) -> 32 big-endian
//   quotient        4096 x 32 canonical little-endian scalars + 32 (z, little-endian) -> 4096 x 32 (q) + 32 (y)
//   srs <path>      -> status, then the 4096 x 48 bytes of the Lagrange section on Success
//   evm g1|g2       the precompile's input -> status of the length check, then per pair: parse[] (1 byte each), pts, coefs
//   evm-out g1|g2   96 | 192 (affine Montgomery) -> 128 | 256
//   cellq           4096 x 32 canonical little-endian coefficients -> 128 x 4096 x 32 canonical quotient coefficients
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "protocols_host.h"

using namespace ctt;
using namespace ctt::proto;

static std::vector<uint8_t> read_all(FILE* f) {
  std::vector<uint8_t> v;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  return v;
}
static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
static void put_status(int st) {
  const uint8_t b = (uint8_t)st;
  put(&b, 1);
}

template <class F>
static int evm(bool out, const std::vector<uint8_t>& in) {
  using E = EvmMsm<F>;
  if (out) {
    if (in.size() != E::AFF) return 2;
    uint8_t r[E::OUT];
    E::encode(r, in.data());
    put(r, sizeof r);
    return 0;
  }
  const size_t n = E::pairs(in.size());
  put_status(n ? EVM_Success : EVM_InvalidInputSize);
  if (!n) return 0;
  std::vector<uint8_t> pts, coefs;
  std::vector<int> verdict;
  E::parse(in.data(), n, pts, coefs, verdict);
  for (int v : verdict) put_status(v);
  put(pts.data(), pts.size());
  put(coefs.data(), coefs.size());
  return 0;
}

static int cellq(const std::vector<uint8_t>& in) {
  std::vector<FrH> p(N_BLOB);
  for (int i = 0; i < N_BLOB; i++) {
    uint64_t v[4];
    memcpy(v, &in[32 * (size_t)i], 32);
    p[i] = to_mont<FrH>(v);
  }
  const std::vector<FrH> ck = cell_coset_constants(root_of_unity(13));
  std::vector<uint32_t> pw((size_t)N_BLOB * 8), ckw((size_t)N_CELLS * 8), q((size_t)N_CELLS * N_BLOB * 8, 0xdeadbeefu);
  memcpy(pw.data(), p.data(), pw.size() * 4);
  memcpy(ckw.data(), ck.data(), ckw.size() * 4);
  const CellQuotArgs a{pw.data(), ckw.data(), q.data(), 1u};
  // (a few lanes past the end, as a grid rounded up to whole workgroups has)
  for (uint32_t lane = 0; lane < (uint32_t)(N_CELLS * CELL_ELEMS) + 256u; lane++) cell_quotient_body(a, lane);
  put(q.data(), q.size() * 4);
  return 0;
}

int main(int argc, char** argv) {
  const char* cmd = argc > 1 ? argv[1] : "";
  if (argc == 3 && !strcmp(cmd, "srs")) {
    std::vector<uint8_t> srs((size_t)N_BLOB * 48);
    const int st = srs_read_ckzg4844(argv[2], srs.data());
    put_status(st);
    if (st == TS_Success) put(srs.data(), srs.size());
    return 0;
  }
  if (argc == 3 && (!strcmp(cmd, "evm") || !strcmp(cmd, "evm-out")) && (!strcmp(argv[2], "g1") || !strcmp(argv[2], "g2"))) {
    const std::vector<uint8_t> in = read_all(stdin);
    return argv[2][1] == '1' ? evm<FpH>(cmd[3] == '-', in) : evm<Fp2H>(cmd[3] == '-', in);
  }
  if (argc != 2) {
    fprintf(stderr, "usage: protocols_harness sha256|decompress|compress|blob|challenge|quotient|cellq < input\n"
                    "       protocols_harness srs <path> | evm g1|g2 < input | evm-out g1|g2 < input\n");
    return 2;
  }
  const std::vector<uint8_t> in = read_all(stdin);
  const size_t blob_bytes = (size_t)N_BLOB * 32;
  if (!strcmp(cmd, "sha256")) {
    uint8_t d[32];
    Sha256 t;
    t.update(in.data(), in.size());
    t.finish(d);
    put(d, 32);
  } else if (!strcmp(cmd, "decompress") && in.size() == 48) {
    uint8_t aff[96];
    const int st = g1_decompress(aff, in.data());
    put_status(st);
    if (st == KZG_Success) put(aff, 96);
  } else if (!strcmp(cmd, "compress") && in.size() == 96) {
    uint8_t c[48];
    g1_compress(c, in.data());
    put(c, 48);
  } else if (!strcmp(cmd, "blob") && in.size() == blob_bytes) {
    std::vector<uint8_t> le(blob_bytes);
    const int st = blob_to_scalars(le.data(), in.data());
    put_status(st);
    if (st == KZG_Success) put(le.data(), le.size());
  } else if (!strcmp(cmd, "challenge") && in.size() == blob_bytes + 48) {
    uint64_t z[4];
    uint8_t z_be[32];
    fiat_shamir_challenge(z, in.data(), in.data() + blob_bytes);
    limbs_to_be<FrH>(z, z_be);
    put(z_be, 32);
  } else if (!strcmp(cmd, "quotient") && in.size() == blob_bytes + 32) {
    uint64_t z[4], y[4];
    memcpy(z, in.data() + blob_bytes, 32);
    std::vector<uint8_t> q(blob_bytes);
    quotient_host(domain_brp(), in.data(), z, q.data(), y);
    put(q.data(), q.size());
    put(y, 32);
  } else if (!strcmp(cmd, "cellq") && in.size() == blob_bytes) {
    return cellq(in);
  } else {
    return 2;
  }
  return 0;
}
