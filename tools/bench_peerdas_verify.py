#!/usr/bin/env python3
"""EIP-7594 batch verification: ms per call of Verifier.verify at n = 128, 768 and 8192 cells (all cells of 1, 6 and 64 blobs, made
with the GPU prover in this run) with the split of ctt_hip_peerdas_verify_last_timings (host clock, every stage waited for) -- and, as
the only comparison, the host's g1_decompress (ctt_hip_bls12_381_g1_decompress, one 381-bit exponentiation each) looped over the same
M + n points.  The reference cannot be timed where this runs: nothing is claimed against it.

    python tools/bench_peerdas_verify.py [--reps 10] > profiles/peerdas_verify.txt
"""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from constantine_amd import _lib, kzg, peerdas  # noqa: E402
from tests import _golden  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
STAGES = ("checks, challenge + upload", "decompress (k_vf_decompress)", "subgroup check", "colsum + transform + interp", "the two MSMs",
          "pairing (host)")


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blobs", type=int, nargs="*", default=[1, 6, 64])
    ap.add_argument("--box", default="1 x AMD Instinct MI355X", help="the box this runs on, for the profile's first line")
    a = ap.parse_args()
    import torch
    print(f"# {a.box} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), one process; python tools/bench_peerdas_verify.py")
    print(f"# wall clock of the Python call (numpy arrays in), median of {a.reps} after one warm-up call; all 128 cells of every blob, random"
          " blobs, the Fiat-Shamir challenge (zero random bytes) unless said otherwise")
    ctx = kzg.EthereumKZGContext(open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read())
    raw = open(os.path.join(_golden.HERE, "kzg4844_srs_verify.bin"), "rb").read()
    ver = peerdas.Verifier(0, g1_monomial=raw[:64 * 48], g2_tau64=raw[64 * 48:])
    rng = random.Random("bench-verify")
    B = max(a.blobs)
    coms = np.zeros((B * 128, 48), dtype=np.uint8)
    cells = np.zeros((B * 128, 2048), dtype=np.uint8)
    proofs = np.zeros((B * 128, 48), dtype=np.uint8)
    for b in range(B):
        blob = b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(4096))
        c, p = kzg.compute_cells_and_kzg_proofs(ctx, blob)
        coms[128 * b:128 * (b + 1)] = np.frombuffer(kzg.blob_to_kzg_commitment(ctx, blob), dtype=np.uint8)
        cells[128 * b:128 * (b + 1)] = np.frombuffer(b"".join(c), dtype=np.uint8).reshape(128, 2048)
        proofs[128 * b:128 * (b + 1)] = np.frombuffer(b"".join(p), dtype=np.uint8).reshape(128, 48)
    idx = np.tile(np.arange(128, dtype=np.uint64), B)
    L = _lib.lib()
    aff = (ctypes.c_uint8 * 96)()
    rnd = bytes(31) + b"\x07"
    for nb in a.blobs:
        n = 128 * nb
        args = (coms[:n], idx[:n], cells[:n], proofs[:n])
        assert ver.verify(*args) is True
        wrong = proofs[:n].copy()
        wrong[[0, n - 1]] = wrong[[n - 1, 0]]
        assert ver.verify(coms[:n], idx[:n], cells[:n], wrong) is False
        ms = med(lambda: ver.verify(*args), a.reps)
        splits = []
        for _ in range(a.reps):
            ver.verify(*args)
            splits.append(ver.last_timings())
        ms_rnd = med(lambda: ver.verify(*args, rnd), a.reps)
        print(f"n = {n:5d} ({nb:2d} blobs, M = {nb})   {ms:9.3f} ms per call   {1e3 * ms / n:9.3f} us per cell"
              f"   with random bytes (no transcript hash) {ms_rnd:9.3f} ms")
        for i, nm in enumerate(STAGES):
            print(f"  {nm:31s} {statistics.median(s[i] for s in splits):9.3f} ms")
        pts = [coms[128 * b].tobytes() for b in range(nb)] + [proofs[k].tobytes() for k in range(n)]

        def host_loop():
            for pt in pts:
                L.ctt_hip_bls12_381_g1_decompress(aff, pt)
        host = med(host_loop, max(1, a.reps // 3))
        print(f"  host g1_decompress over the same {len(pts)} points, one after another {host:9.3f} ms ({1e3 * host / len(pts):.1f} us per point)")
    ver.delete()
    ctx.delete()


if __name__ == "__main__":
    main()
