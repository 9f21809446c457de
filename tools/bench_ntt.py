#!/usr/bin/env python3
"""Times of the batched scalar-field NTT (ctt_hip_fr_ntt) on device-resident rows: HIP-event median of the calls after a warm-up,
the passes, the bytes they move (passes x 64 B x n x batch: each pass reads and writes every element once) and that rate as a
fraction of a 1 GiB device-to-device copy measured in the same run (read + write counted, best of 6).

    python tools/bench_ntt.py [--reps 30] [--quick] > profiles/ntt.txt
"""
import argparse
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from constantine_amd.ntt import NttPlan  # noqa: E402

MODULI = {
    "bls12_381_g1": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    "bn254_snarks_g1": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    "pallas": 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
    "vesta": 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
}


def root(p, lg):
    for x in (7, 2, 3, 5, 11, 13):
        w = pow(x, (p - 1) >> lg, p)
        if pow(w, 1 << (lg - 1), p) == p - 1:
            return w
    raise SystemExit("no root of unity")


def copy_rate():
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    best = 1e9
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return 2 * (1 << 30) / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="BLS12-381 and BN254 only, no 2^24")
    a = ap.parse_args()
    peak = copy_rate()
    print(f"# copy rate of this device, 1 GiB device to device, read + write: {peak:.0f} GB/s")
    print(f"# forward, natural in, bit-reversed out, canonical both sides; median of {a.reps} calls (HIP events), in place")
    print("curve log2n batch tile passes ms GB_moved GB/s frac_of_copy Melem/s")
    curves = ["bls12_381_g1", "bn254_snarks_g1"] + ([] if a.quick else ["pallas", "vesta"])
    for curve in curves:
        p = MODULI[curve]
        cfgs = [(12, 128, t) for t in (4, 6, 8, 9)] + [(16, 1, 0), (20, 1, 0)] + ([] if a.quick else [(24, 1, 0)])
        if curve == "bn254_snarks_g1":
            cfgs.append((22, 1, 0))
        for lg, batch, tile in cfgs:
            plan = NttPlan(curve, lg, root(p, lg), tile_log2=tile)
            x = torch.zeros(batch << lg, 32, dtype=torch.uint8, device="cuda")
            x[:, :3] = torch.randint(0, 256, (batch << lg, 3), dtype=torch.uint8, device="cuda")
            for _ in range(3):
                assert plan.ntt_ptr(x.data_ptr(), x.data_ptr(), batch, 4, None) == 0
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = plan.ntt_ptr(x.data_ptr(), x.data_ptr(), batch, 4, None)
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0
                ms.append(e0.elapsed_time(e1))
            t = statistics.median(ms)
            info = plan.info()
            moved = info["passes"] * 64 * (batch << lg)
            rate = moved / (t * 1e-3) / 1e9
            print(f"{curve} {lg} {batch} {info['tile_log2']} {info['passes']} {t:.4f} {moved / 1e9:.4f} {rate:.1f} {rate / peak:.3f} "
                  f"{(batch << lg) / (t * 1e-3) / 1e6:.1f}")
            plan.close()
            del x


if __name__ == "__main__":
    main()
