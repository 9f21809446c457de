#!/usr/bin/env python3
"""EIP-7594 on one context: ms per blob for the cells alone and for cells + proofs, the split of the proof call
(ctt_hip_eth_kzg_last_cell_timings: host clock, every step waited for), and in the same run what a caller had before --
128 x blob_to_kzg_commitment and one compute_kzg_proof.

    python tools/bench_peerdas.py [--reps 10] > profiles/peerdas.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from constantine_amd import kzg  # noqa: E402
from tests import _golden  # noqa: E402


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
    a = ap.parse_args()
    ctx = kzg.EthereumKZGContext(open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read())
    blob = next(b for name, b, com in _golden.kzg4844_raw_cases() if com is not None and name.endswith("19b3f3f8c98ea31e"))
    z = (12345).to_bytes(32, "big")
    print(f"# one blob, one context, wall clock of the Python call, median of {a.reps} after one warm-up call")
    print(f"compute_cells                     {med(lambda: kzg.compute_cells(ctx, blob), a.reps):9.3f} ms per blob")
    print(f"compute_cells_and_kzg_proofs      {med(lambda: kzg.compute_cells_and_kzg_proofs(ctx, blob), a.reps):9.3f} ms per blob")
    splits = []
    for _ in range(a.reps):
        kzg.compute_cells_and_kzg_proofs(ctx, blob)
        splits.append(kzg.last_cell_timings(ctx))
    names = ("parse + upload", "INTT", "coset NTT", "quotients", "batched NTT", "MSM loop (128)", "compress + copy back")
    for i, nm in enumerate(names):
        print(f"  {nm:31s} {statistics.median(s[i] for s in splits):9.3f} ms")
    print("# the comparison a caller had without the cell functions, same run")
    one = med(lambda: kzg.blob_to_kzg_commitment(ctx, blob), a.reps * 4)
    print(f"blob_to_kzg_commitment            {one:9.3f} ms; x 128 = {128 * one:9.3f} ms")
    print(f"compute_kzg_proof                 {med(lambda: kzg.compute_kzg_proof(ctx, blob, z), a.reps):9.3f} ms")
    ctx.delete()


if __name__ == "__main__":
    main()
