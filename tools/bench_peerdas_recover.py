#!/usr/bin/env python3
"""EIP-7594 recovery: ms per call of recover_blobs at B = 1, 6 and 64 blobs (every other cell given) with the split of
ctt_hip_peerdas_last_timings (host clock, every step waited for), and of the full recovery (blobs, then cells and proofs) at B = 1 and 6
beside compute_cells_and_kzg_proofs on the same blobs in the same run: recovery's own cost is the difference.

    python tools/bench_peerdas_recover.py [--reps 10] > profiles/peerdas_recover.txt
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from constantine_amd import kzg, peerdas  # noqa: E402
from tests import _golden  # noqa: E402

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


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
    ap.add_argument("--box", default="1 x AMD Instinct MI355X", help="the box this runs on, for the profile's first line")
    a = ap.parse_args()
    import torch
    print(f"# {a.box} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), one process; python tools/bench_peerdas_recover.py")
    print(f"# wall clock of the Python call (numpy arrays in and out), median of {a.reps} after one warm-up call; 64 of the 128 cells given"
          " (every other one), random blobs")
    ctx = kzg.EthereumKZGContext(open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read())
    rec = peerdas.Recovery(0)
    rng = random.Random("bench-recover")
    blobs = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(4096)) for _ in range(64)]
    idx = list(range(0, 128, 2))
    given = np.zeros((64, 64, 2048), dtype=np.uint8)
    for b, blob in enumerate(blobs):
        cells = kzg.compute_cells(ctx, blob)
        given[b] = np.frombuffer(b"".join(cells[i] for i in idx), dtype=np.uint8).reshape(64, 2048)
    names = ("checks + upload", "3 transforms of 8192", "3 element-wise kernels", "transform of 4096 + copy back")
    print("## recover_blobs (the data alone)")
    for B in (1, 6, 64):
        got, ok = rec.recover_blobs(idx, given[:B])
        assert ok.all() and all(got[b].tobytes() == blobs[b] for b in range(B))
        ms = med(lambda: rec.recover_blobs(idx, given[:B]), a.reps)
        splits = []
        for _ in range(a.reps):
            rec.recover_blobs(idx, given[:B])
            splits.append(rec.last_timings())
        print(f"B = {B:2d}   {ms:9.3f} ms per call   {ms / B:9.3f} ms per blob")
        for i, nm in enumerate(names):
            print(f"  {nm:31s} {statistics.median(s[i] for s in splits):9.3f} ms")
    print("## full recovery (all 128 cells and proofs) beside compute_cells_and_kzg_proofs on the same blobs")
    for B in (1, 6):
        want = [kzg.compute_cells_and_kzg_proofs(ctx, blobs[b]) for b in range(B)]
        cells, proofs = rec.recover_cells_and_kzg_proofs(ctx, idx, given[:B])
        assert all(cells[b].tobytes() == b"".join(want[b][0]) and proofs[b].tobytes() == b"".join(want[b][1]) for b in range(B))
        full = med(lambda: rec.recover_cells_and_kzg_proofs(ctx, idx, given[:B]), a.reps)
        prover_ms = rec.last_timings()[4]
        prove = med(lambda: [kzg.compute_cells_and_kzg_proofs(ctx, blobs[b]) for b in range(B)], a.reps)
        print(f"B = {B:2d}   recover_cells_and_kzg_proofs {full:9.3f} ms   compute_cells_and_kzg_proofs x {B} {prove:9.3f} ms   "
              f"difference {full - prove:9.3f} ms ({(full - prove) / B:.3f} per blob); the prover inside the last recovery call {prover_ms:9.3f} ms")
    if B == 6:
        one = med(lambda: kzg.recover_cells_and_kzg_proofs(ctx, idx, given[0]), a.reps)
        print(f"ctt_eth_kzg_recover_cells_and_kzg_proofs (the reference's symbol, one blob) {one:9.3f} ms")
    rec.delete()
    ctx.delete()


if __name__ == "__main__":
    main()
