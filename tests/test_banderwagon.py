"""Banderwagon without a GPU: the oracle against the reference's Verkle vectors, the companion library's header and exports, the
host-side sum of ctt_hip_ec_sum_affine and the twisted Edwards bodies of csrc/ec.h compiled for the CPU."""
import ctypes
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import _banderwagon as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "constantine_amd")
COMPANION = os.path.join(PKG, "libctt_msm_hip_banderwagon.so")
HEADER = os.path.join(ROOT, "include", "ctt_msm_hip_banderwagon.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "banderwagon_verkle.json")
REF_INCLUDE = "/root/reference/include"
SYMS = ["ctt_banderwagon_ec_prj_multi_scalar_mul_big_coefs_vartime", "ctt_banderwagon_ec_prj_multi_scalar_mul_fr_coefs_vartime",
        "ctt_hip_msm_banderwagon_ec_prj_big", "ctt_hip_msm_banderwagon_ec_prj_fr"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_oracle_doublings_and_subgroup(golden):
    assert bw.on_curve(bw.G) and bw.in_subgroup(bw.G) and bw.mul(bw.R, bw.G) == bw.O
    pt = bw.G
    for h in golden["doublings"]:
        assert "0x" + bw.serialize(pt).hex() == h
        assert bw.deserialize(bytes.fromhex(h[2:])) in (pt, (bw.neg(pt)[0], (-pt[1]) % bw.P))
        pt = bw.add(pt, pt)
    for h in golden["not_in_subgroup"]:
        b = bytes.fromhex(h[2:])
        assert bw.deserialize(b, check_subgroup=False) is not None and bw.deserialize(b) is None


def test_oracle_verkle_crs_and_commitment(golden):
    crs = bw.crs(256)
    assert "0x" + bw.serialize(crs[0]).hex() == golden["crs0"]
    assert "0x" + bw.serialize(crs[255]).hex() == golden["crs255"]
    scalars = [int(h, 16) for h in golden["commit_scalars"]]
    assert "0x" + bw.serialize(bw.msm_fast(scalars, crs)).hex() == golden["commitment"]
    assert bw.msm_fast(scalars[:8], crs[:8]) == bw.msm(scalars[:8], crs[:8])


def _cc():
    return shutil.which("cc") or shutil.which("gcc")


def test_companion_header_compiles_as_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ctt_msm_hip_banderwagon.h"\n#include "ctt_msm_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(big253), sizeof(banderwagon_fr), '
                   'sizeof(banderwagon_ec_aff), sizeof(banderwagon_ec_prj)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([_cc(), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32", "32", "64", "96"]


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="Constantine's own headers are not on this box")
def test_links_against_constantine_header(tmp_path):
    src = tmp_path / "link.c"
    src.write_text('#include "constantine/curves/banderwagon.h"\n'
                   'int main(int argc, char** argv) { banderwagon_ec_prj r; big253 k[1]; banderwagon_fr f[1]; banderwagon_ec_aff p[1];\n'
                   '  if (argc > 5) { ctt_banderwagon_ec_prj_multi_scalar_mul_big_coefs_vartime(&r, k, p, 1);\n'
                   '                  ctt_banderwagon_ec_prj_multi_scalar_mul_fr_coefs_vartime(&r, f, p, 1); }\n  return 0; }\n')
    subprocess.run([_cc(), "-I", REF_INCLUDE, str(src), "-o", str(tmp_path / "link"), "-L", PKG, "-lctt_msm_hip_banderwagon",
                    "-Wl,--no-undefined", "-Wl,--unresolved-symbols=report-all", f"-Wl,-rpath,{PKG}"], check=True)
    subprocess.run(["ldd", "-r", str(tmp_path / "link")], check=True, capture_output=True)


def test_companion_exports_exactly_four():
    out = subprocess.run(["nm", "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == sorted(SYMS)
    needed = subprocess.run(["readelf", "-d", COMPANION], check=True, capture_output=True, text=True).stdout
    assert "[libctt_msm_hip.so]" in needed


def _sum(L, pts, kind):
    a = np.frombuffer(b"".join(bw.aff_bytes(p) for p in pts), dtype=np.uint8).copy()
    r = np.zeros(64 if kind == 0 else 96, dtype=np.uint8)
    rc = L.ctt_hip_ec_sum_affine(6, kind, r.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p), len(pts))
    return rc, bytes(r)


def test_host_sum_affine():
    from constantine_amd import _lib
    L = _lib.lib()
    P = bw.mul(0x1234567890abcdef, bw.G)
    cases = [[P, bw.neg(P)], [P, P], [bw.O], [bw.T2], [P, bw.T2], [bw.T2, bw.T2], [bw.G, P, bw.T2, bw.O, bw.neg(bw.G)], []]
    for pts in cases:
        expect = bw.O
        for q in pts:
            expect = bw.add(expect, q)
        rc, r = _sum(L, pts, 0)
        assert rc == 0 and bw.aff_from(r) == expect
        rc, r = _sum(L, pts, 2)
        assert rc == 0 and bw.fp_from(r[64:]) == 1 and bw.aff_from(r[:64]) == expect
    sentinel = np.full(96, 7, dtype=np.uint8)
    assert L.ctt_hip_ec_sum_affine(6, 1, sentinel.ctypes.data_as(ctypes.c_void_p), None, 0) == -1   # no Jacobian coordinates
    assert bytes(sentinel) == bytes([7] * 96)


HARNESS = r'''
#include <cstdio>
#include <cstring>
#include "msm_bodies.h"
using namespace ctt;
using F = Banderwagon::F;
static void put(const Affine<F>& a) { fwrite(&a, sizeof(a), 1, stdout); }
int main() {   // stdin: n, n affine points (64 bytes), n sign bytes.  stdout: see test_device_field_group_law
  uint32_t n;
  if (fread(&n, 4, 1, stdin) != 1) return 1;
  Affine<F> p[64];
  uint8_t s[64];
  if (n > 64 || fread(p, sizeof(Affine<F>), n, stdin) != n || fread(s, 1, n, stdin) != n) return 1;
  XYZZ<F> acc = XYZZ<F>::inf();
  bool empty = true;
  for (uint32_t i = 0; i < n; i++) xyzz_madd_flag<F, SignMask>(acc, empty, p[i].x, p[i].y, SignMask(s[i] ? 0x80000000u : 0u));
  if (empty) acc = XYZZ<F>::inf();
  put(xyzz_to_affine<F>(acc));                                    // sum of +-p[i], mixed additions
  XYZZ<F> full = XYZZ<F>::inf();
  for (uint32_t i = 0; i < n; i++) {
    XYZZ<F> q = XYZZ<F>::inf();
    xyzz_madd<F>(q, p[i], s[i] != 0);
    full = xyzz_add_inl<F>(full, q);
    put(xyzz_to_affine<F>(xyzz_dbl<F>(q)));                       // 2(+-p[i]), projective doubling
    put(xyzz_to_affine<F>(xyzz_mdbl<F>(p[i].x, p[i].y)));          // 2 p[i], affine doubling
    put(xyzz_to_affine<F>(xyzz_add_inl<F>(q, q)));                 // q + q through the addition
  }
  put(xyzz_to_affine<F>(full));                                   // the same sum, full additions
  put(xyzz_to_affine<F>(xyzz_dbl<F>(XYZZ<F>::inf())));            // neutral in memory
  return 0;
}
'''


def test_device_field_group_law(tmp_path):
    """the kernels' bodies (csrc/ec.h over the 32-bit-limb device field), compiled with the host compiler, against the oracle"""
    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "law.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "law"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    rng = random.Random(6)
    P = bw.mul(rng.randrange(bw.R), bw.G)
    pts = [P, P, bw.neg(P), bw.O, bw.T2, bw.G] + [bw.mul(rng.randrange(bw.R), bw.G) for _ in range(10)] + [bw.add(P, bw.T2)]
    signs = [0, 1, 0, 1, 0, 1] + [rng.randrange(2) for _ in range(10)] + [1]
    inp = len(pts).to_bytes(4, "little") + b"".join(bw.aff_bytes(p) for p in pts) + bytes(signs)
    out = subprocess.run([str(exe)], input=inp, check=True, capture_output=True).stdout
    res = [bw.aff_from(out[i:i + 64]) for i in range(0, len(out), 64)]
    signed = [bw.neg(p) if s else p for p, s in zip(pts, signs)]
    total = bw.O
    for q in signed:
        total = bw.add(total, q)
    assert res[0] == total
    for i, (p, q) in enumerate(zip(pts, signed)):
        assert res[1 + 3 * i: 4 + 3 * i] == [bw.add(q, q), bw.add(p, p), bw.add(q, q)], i
    assert res[1 + 3 * len(pts)] == total
    assert res[2 + 3 * len(pts)] == bw.O
