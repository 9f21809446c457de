#!/usr/bin/env python3
"""us per Verkle commitment (256 scalars against a fixed 256-point Banderwagon basis) on one MI355X, one process, inputs resident
on the device: VerkleCrs.commit over batches of m rows at several window widths, against what the library offered before -- one
CachedBases(...).msm per row, with and without a window table -- in the same run.

    python tools/bench_verkle_commit.py [--bits 6,8,10] [--batches 1,16,256,4096,65536] [--out profiles/verkle_commit.txt]

Per (window bits, m): wall time of the blocking call per commitment, the commit and the finish kernel by HIP events, and the mixed
additions per second of the commit kernel (m * n * W / kernel time; the accumulate kernel of a 2^20-pair Banderwagon MSM beside it).
--pad also measures the table with 128-byte records ($CTT_HIP_VERKLE_PAD) at the first width.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 256


def windows(c):
    """(W, records per base) of window_layout(253, c)"""
    t = 254
    nw = (t + c - 1) // c
    cb, r = t // nw, t - (t // nw) * nw
    return nw, r * (1 << cb) + (nw - r) * (1 << (cb - 1))


def scalars(torch, shape, seed):
    g = torch.Generator().manual_seed(seed)
    ks = torch.randint(0, 256, shape + (32,), dtype=torch.uint8, generator=g)
    ks[..., 31] &= 0x0f
    return ks.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="6,8,10")
    ap.add_argument("--batches", default="1,16,256,4096,65536")
    ap.add_argument("--loop-rows", type=int, default=200)
    ap.add_argument("--pad", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verkle_commit.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from constantine_amd import CachedBases, DeviceMsm, VerkleCrs
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = DeviceMsm(0)
    pts = torch.empty((N, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", 11, N, pts)
    dev.sync()
    batches = [int(s) for s in a.batches.split(",") if s]
    coefs = scalars(torch, (max(batches), N), 1)
    torch.cuda.synchronize()
    say(f"# tools/bench_verkle_commit.py -- {torch.cuda.get_device_name(0)}, one process, one lease; n = {N} bases, device-resident inputs")

    # --- baseline: one MSM per row through the cached bases, blocking (submit + finish), the same rows
    say("# baseline: one CachedBases.msm per row (submit + finish), us per commitment")
    loop_us = {}
    for table in (True, False):
        cb = CachedBases("banderwagon", pts, ctx=dev.ctx, on_device=True, table=table)
        rows = min(a.loop_rows, coefs.shape[0])
        for i in range(10):
            cb.msm(coefs[i % rows], coord="prj")
        t0 = time.perf_counter()
        for i in range(rows):
            cb.msm(coefs[i], coord="prj")
        loop_us[table] = (time.perf_counter() - t0) * 1e6 / rows
        say(f"loop table={str(table):5s} window_bits={cb.window_bits:2d}  {loop_us[table]:9.1f} us/commitment  ({rows} rows)")
        cb.close()
    best_loop = min(loop_us.values())

    # --- the accumulate kernel of the MSM pipeline, for the rate comparison
    big_n = 1 << 20
    bpts = torch.empty((big_n, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", 12, big_n, bpts)
    bks = scalars(torch, (big_n,), 2)
    dev.enable_timings(1)
    for _ in range(3):
        dev.msm("banderwagon", bks, bpts, big_n, coord="aff")
    acc_ms, plan = dev.last_timings()["accumulate"], dev.last_plan()
    dev.set_option("timings", 0)
    del bpts, bks
    acc_rate = big_n * plan["W"] / (acc_ms * 1e-3)
    say(f"# k_accum, Banderwagon MSM of 2^20 pairs: {acc_ms:.3f} ms, W = {plan['W']} (c = {plan['c']}): {acc_rate / 1e9:.2f} G mixed additions/s (10M each, sorted gathers)")

    say("# batch: VerkleCrs.commit(want = prj, ser, fr); wall = the blocking call; kernel / finish = HIP events")
    say("#  c pad  W  table_MiB build_ms       m   wall_us/commit  kernel_us/commit  finish_us/commit  G madd/s  vs best loop")
    variants = [(int(s), False) for s in a.bits.split(",") if s]
    if a.pad:
        variants.insert(1, (variants[0][0], True))
    verdict = []
    for c, pad in variants:
        os.environ["CTT_HIP_VERKLE_PAD"] = "1" if pad else "0"
        crs = VerkleCrs(pts, ctx=dev.ctx, window_bits=c, on_device=True)
        W, rows = windows(crs.window_bits)
        mib = N * rows * (128 if pad else 96) / 2**20
        build_ms = crs.last_timings()["table"]
        for m in batches:
            reps = 3 if m >= 65536 else 10 if m >= 4096 else 30
            for _ in range(2):
                crs.commit(coefs[:m])
            t0 = time.perf_counter()
            for _ in range(reps):
                crs.commit(coefs[:m])
            wall = (time.perf_counter() - t0) * 1e6 / reps / m
            dev.enable_timings(1)
            ker, fin = [], []
            for _ in range(min(reps, 5)):
                crs.commit(coefs[:m])
                t = crs.last_timings()
                ker.append(t["commit"])
                fin.append(t["finish"])
            dev.set_option("timings", 0)
            k_ms, f_ms = min(ker), min(fin)
            rate = m * N * W / (k_ms * 1e-3)
            say(f"  {crs.window_bits:2d} {int(pad):3d} {W:3d} {mib:9.1f} {build_ms:8.2f} {m:7d} {wall:16.2f} {k_ms * 1e3 / m:17.2f} {f_ms * 1e3 / m:17.3f} "
                f"{rate / 1e9:9.2f} {best_loop / wall:10.1f}x")
            if m >= 16:
                verdict.append(wall < best_loop)
        crs.close()
    os.environ.pop("CTT_HIP_VERKLE_PAD", None)
    say(f"# acceptance (every m >= 16 below the faster loop, {best_loop:.1f} us): {'met' if all(verdict) else 'NOT met'}")
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
