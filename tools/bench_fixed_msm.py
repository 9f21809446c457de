#!/usr/bin/env python3
"""The batched fixed-base G1 MSM (constantine_amd.fixed.FixedBaseMsm) on one GPU in one process: table size and build time per window
size, ms per batch of m rows over n = 4096 fixed points with device-resident coefficients (median of --reps runs, wall clock of the
call), the device-time split sum kernel / finish, the kernel's rate in mixed additions per second (m * n * W over its time), and in
the same run the loop a caller had before: CachedBases(table=True).msm over the same rows.

    python tools/bench_fixed_msm.py [--reps 20] > profiles/fixed_msm.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from constantine_amd import CachedBases, DeviceMsm, FixedBaseMsm  # noqa: E402
from oracle import cref  # noqa: E402

N = 4096


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def scalars(m, bits, seed):
    return torch.from_numpy(cref.synth_scalars(seed, m * N, bits).reshape(m, N, 32)).cuda()


def loop_ms(curve, pts, d_coefs, reps):
    """the baseline: one ticketed MSM per row over cached bases with a window table, three in flight"""
    dev = DeviceMsm(0)
    bases = CachedBases(curve, pts, ctx=dev.ctx, table=True)

    def run():
        tickets = []
        for k in range(d_coefs.shape[0]):
            if len(tickets) == 3:
                bases.finish(tickets.pop(0), coord="aff")
            tickets.append(bases.submit(d_coefs[k], N))
        for t in tickets:
            bases.finish(t, coord="aff")
    ms = med(run, reps)
    bases.close()
    dev.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ms", type=int, nargs="*", default=[1, 16, 128, 1024])
    ap.add_argument("--cs", type=int, nargs="*", default=[4, 5, 6, 8])
    ap.add_argument("--box", default="1 x AMD Instinct MI355X", help="the box this runs on, for the profile's first line")
    a = ap.parse_args()
    print(f"# {a.box} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), one process; python tools/bench_fixed_msm.py")
    print(f"# n = {N} fixed points, device-resident coefficients below 2^bits, median of {a.reps} runs")
    print("# ms/batch: wall clock of msm_batch (launches, the wait, the copy of the result); kernel / finish: device time of k_fx_msm / k_fx_finish")
    for curve, bits, ms_list, cs in (("bls12_381_g1", 255, a.ms, a.cs), ("bn254_snarks_g1", 254, [128], a.cs)):
        pts = cref.gen_points(curve, 5, N)
        d = {m: scalars(m, bits, 100 + m) for m in ms_list}
        print(f"## {curve}")
        base = {}
        for m in ms_list:
            base[m] = loop_ms(curve, pts, d[m], max(3, a.reps // 4) if m > 128 else a.reps)
            print(f"loop of CachedBases(table=True).msm   m = {m:5d}  {base[m]:10.3f} ms/batch")
        print("   c   W  table MiB  build ms      m    ms/batch   kernel ms  finish ms   Gadd/s   x loop")
        for c in cs:
            f = FixedBaseMsm(curve, pts, c=c)
            info = f.info()
            for m in ms_list:
                t = med(lambda: f.msm_batch(d[m]), a.reps)
                ks = []
                for _ in range(a.reps):
                    f.msm_batch(d[m])
                    ks.append(f.last_timings())
                k_ms, f_ms = statistics.median(k[0] for k in ks), statistics.median(k[1] for k in ks)
                rate = m * N * info["windows"] / (k_ms * 1e-3) / 1e9
                print(f"  {c:2d}  {info['windows']:2d}  {info['table_bytes'] / 2**20:9.1f}  {info['build_us'] / 1e3:8.1f}  {m:5d}  {t:10.3f}  {k_ms:10.3f}"
                      f"  {f_ms:9.3f}  {rate:7.2f}  {base[m] / t:7.1f}")
            f.close()


if __name__ == "__main__":
    main()
