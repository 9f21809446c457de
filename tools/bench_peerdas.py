#!/usr/bin/env python3
"""EIP-7594: ms per blob for the cells alone and for cells + proofs, the split of the proof call
(ctt_hip_eth_kzg_last_cell_timings: host clock, every step waited for) -- for a context on the table path of the cell proofs and for
one on the loop, in the same run -- and what a caller had before: 128 x blob_to_kzg_commitment and one compute_kzg_proof.

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


def context(srs, mode):
    """a context whose cell proofs take the table path (the batched fixed-base MSM) or the loop of 128 MSMs: read at creation"""
    old = os.environ.pop("CTT_HIP_CELL_PROOFS", None)
    if mode == "loop":
        os.environ["CTT_HIP_CELL_PROOFS"] = "loop"
    try:
        return kzg.EthereumKZGContext(srs)
    finally:
        os.environ.pop("CTT_HIP_CELL_PROOFS", None)
        if old is not None:
            os.environ["CTT_HIP_CELL_PROOFS"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default="1 x AMD Instinct MI355X", help="the box this runs on, for the profile's first line")
    a = ap.parse_args()
    import torch
    print(f"# {a.box} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), one process; python tools/bench_peerdas.py"
          + (f" with CTT_HIP_CELL_PROOFS_C={os.environ['CTT_HIP_CELL_PROOFS_C']}" if os.environ.get("CTT_HIP_CELL_PROOFS_C") else " (the table's default c)"))
    srs = open(os.path.join(_golden.HERE, "kzg4844_srs_g1_lagrange.bin"), "rb").read()
    blob = next(b for name, b, com in _golden.kzg4844_raw_cases() if com is not None and name.endswith("19b3f3f8c98ea31e"))
    z = (12345).to_bytes(32, "big")
    print(f"# one blob, wall clock of the Python call, median of {a.reps} after one warm-up call; two contexts in one process:")
    print("# `table` -- the 128 cell proofs in one pass of the batched fixed-base MSM -- and `loop` (CTT_HIP_CELL_PROOFS=loop)")
    names = ("parse + upload", "INTT", "coset NTT", "quotients", "batched NTT", "the 128 MSMs", "compress + copy back")
    proofs = {}
    for mode in ("table", "loop"):
        ctx = context(srs, mode)
        kzg.compute_cells_and_kzg_proofs(ctx, blob)
        path, build_ms = kzg.last_cell_proof_path(ctx)
        print(f"## {mode} context: first proof call served by the {path}" + (f", table build {build_ms:.1f} ms" if build_ms else "")
              + (f", c = {os.environ['CTT_HIP_CELL_PROOFS_C']}" if mode == "table" and os.environ.get("CTT_HIP_CELL_PROOFS_C") else ""))
        print(f"compute_cells                     {med(lambda: kzg.compute_cells(ctx, blob), a.reps):9.3f} ms per blob")
        print(f"compute_cells_and_kzg_proofs      {med(lambda: kzg.compute_cells_and_kzg_proofs(ctx, blob), a.reps):9.3f} ms per blob")
        splits = []
        for _ in range(a.reps):
            proofs[mode] = kzg.compute_cells_and_kzg_proofs(ctx, blob)
            splits.append(kzg.last_cell_timings(ctx))
        assert kzg.last_cell_proof_path(ctx) == (path, 0.0)
        for i, nm in enumerate(names):
            print(f"  {nm:31s} {statistics.median(s[i] for s in splits):9.3f} ms")
        if mode == "loop":
            print("# the comparison a caller had without the cell functions, same run")
            one = med(lambda: kzg.blob_to_kzg_commitment(ctx, blob), a.reps * 4)
            print(f"blob_to_kzg_commitment            {one:9.3f} ms; x 128 = {128 * one:9.3f} ms")
            print(f"compute_kzg_proof                 {med(lambda: kzg.compute_kzg_proof(ctx, blob, z), a.reps):9.3f} ms")
        ctx.delete()
    assert proofs["table"] == proofs["loop"]
    print("# cells and proofs of the two contexts are byte-identical")


if __name__ == "__main__":
    main()
