#!/usr/bin/env python3
"""ms per Banderwagon MSM on one MI355X (same process: Pallas at the large sizes for a same-box comparison).

  device-resident, pipelined (two MSMs in flight: submit i+1, then finish i -- the way bench.py runs its workload)
  host-pointer, through the Constantine symbol ctt_banderwagon_ec_prj_multi_scalar_mul_big_coefs_vartime (blocking calls)

    python tools/bench_banderwagon.py [--sizes 8,12,16,18,20,22] [--host-sizes 8,16] [--pallas 20,22] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pipelined(dev, torch, curve, n, steps, warmup, aff_bytes):
    pts = torch.empty((n, aff_bytes), dtype=torch.uint8, device="cuda")
    dev.gen_points(curve, 7, n, pts)
    g = torch.Generator().manual_seed(n)
    ks = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    ks[:, 31] &= 0x0f
    ks = ks.cuda()
    torch.cuda.synchronize()

    def run(k):
        t = dev.submit(curve, ks, pts, n)
        for _ in range(k - 1):
            t2 = dev.submit(curve, ks, pts, n)
            dev.finish(t, coord="aff")
            t = t2
        dev.finish(t, coord="aff")

    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return (time.perf_counter() - t0) * 1e3 / steps


def hostptr(torch, dev, n, steps):
    from constantine_amd import multiScalarMul_vartime
    pts = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", 9, n, pts)
    pts = pts.cpu().numpy()
    ks = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    ks[:, 31] &= 0x0f
    for _ in range(3):
        multiScalarMul_vartime("banderwagon", ks, pts, coord="prj")
    t0 = time.perf_counter()
    for _ in range(steps):
        multiScalarMul_vartime("banderwagon", ks, pts, coord="prj")
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,12,16,18,20,22")
    ap.add_argument("--host-sizes", default="8,16")
    ap.add_argument("--pallas", default="20,22")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from constantine_amd import DeviceMsm
    dev = DeviceMsm(0)
    out = {}
    for lg in [int(s) for s in a.sizes.split(",") if s]:
        out[f"banderwagon_device_2^{lg}"] = pipelined(dev, torch, "banderwagon", 1 << lg, a.steps, a.warmup, 64)
        print(f"banderwagon device-resident 2^{lg}: {out[f'banderwagon_device_2^{lg}']:.3f} ms/MSM  plan {dev.last_plan()}", flush=True)
    for lg in [int(s) for s in a.pallas.split(",") if s]:
        out[f"pallas_device_2^{lg}"] = pipelined(dev, torch, "pallas", 1 << lg, a.steps, a.warmup, 64)
        print(f"pallas      device-resident 2^{lg}: {out[f'pallas_device_2^{lg}']:.3f} ms/MSM", flush=True)
    for lg in [int(s) for s in a.host_sizes.split(",") if s]:
        out[f"banderwagon_hostptr_2^{lg}"] = hostptr(torch, dev, 1 << lg, a.steps)
        print(f"banderwagon host-pointer (Constantine symbol) 2^{lg}: {out[f'banderwagon_hostptr_2^{lg}']:.3f} ms/call", flush=True)
    dev.close()
    print(json.dumps({k: round(v, 4) for k, v in out.items()}))


if __name__ == "__main__":
    main()
