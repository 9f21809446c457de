#!/usr/bin/env python3
"""us per sparse Verkle update (k changed slots of a 256-slot node, old commitment added, all of prj / ser / fr / dfr written) on one
MI355X, one process, inputs resident on the device: VerkleCrs.update over m rows of k entries, against what the library offered before
for the same rows -- VerkleCrs.commit on the rows scattered into dense (m, 256, 32) form, which does not even add the old commitment --
in the same run.

    python tools/bench_verkle_update.py [--entries 1,4,16,64,256] [--batches 1,16,256,4096,65536] [--out profiles/verkle_update.txt]

Per (k, m): wall time of the blocking call per row (the host's check and upload of row_ptr / idx included), the update kernel and the
finish (finish of the results, finish of the bases, subtraction) by HIP events, and the same for the dense baseline.  Combinations
whose deltas would pass 2^31 bytes are skipped.  Python does no dispatch between the two paths; the crossover is reported.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 256
ALL = ("prj", "ser", "fr", "dfr")


def timed(fn, reps):
    for _ in range(2):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1,4,16,64,256")
    ap.add_argument("--batches", default="1,16,256,4096,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verkle_update.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from constantine_amd import DeviceMsm, VerkleCrs
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ks = [int(s) for s in a.entries.split(",") if s]
    ms = [int(s) for s in a.batches.split(",") if s]
    combos = [(k, m) for k in ks for m in ms if k * m * 32 < 2**31]
    m_max, e_max = max(m for _, m in combos), max(k * m for k, m in combos)
    dev = DeviceMsm(0)
    pts = torch.empty((N, 64), dtype=torch.uint8, device="cuda")
    dev.gen_points("banderwagon", 11, N, pts)
    dev.sync()
    crs = VerkleCrs(pts, ctx=dev.ctx, on_device=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = torch.randint(0, 256, (max(e_max, m_max * N), 32), dtype=torch.uint8, device="cuda", generator=g)   # scalars below 2^252
    pool[:, 31] &= 0x0f
    # old commitments: dense commitments of random rows, in chunks
    base = torch.empty((m_max, 96), dtype=torch.uint8, device="cuda")
    for lo in range(0, m_max, 4096):
        hi = min(m_max, lo + 4096)
        base[lo:hi] = crs.commit(pool[lo * N:hi * N].view(hi - lo, N, 32), want=("prj",))["prj"]
    # k distinct slots per row: the first k of a random permutation of the 256
    perm = np.argsort(np.random.default_rng(2).random((m_max, N), dtype=np.float32), axis=1).astype(np.uint8)
    torch.cuda.synchronize()
    say(f"# tools/bench_verkle_update.py -- {torch.cuda.get_device_name(0)}, one process, one lease; n = {N} bases, window_bits = {crs.window_bits}, "
        "device-resident deltas, bases and outputs; row_ptr / idx on the host")
    say("# update: VerkleCrs.update(base = old commitments, want = prj, ser, fr, dfr); dense: VerkleCrs.commit(want = prj, ser, fr) on the same rows")
    say("# scattered into (m, 256, 32) -- the parent commit's route, which does not add the old commitment.  wall = the blocking call; kernel / finish = HIP events")
    say("#   k       m   update: wall_us/row kernel_us/row finish_us/row    dense: wall_us/row kernel_us/row finish_us/row   dense/update (wall)")
    ratio = {}
    for k, m in combos:
        E = k * m
        idx = np.ascontiguousarray(perm[:m, :k]).reshape(-1)
        row_ptr = (np.arange(m + 1, dtype=np.uint64) * k).astype(np.uint32)
        deltas = pool[:E]
        dense = torch.zeros((m * N, 32), dtype=torch.uint8, device="cuda")
        where = torch.from_numpy((np.repeat(np.arange(m, dtype=np.int64), k) * N + idx.astype(np.int64))).cuda()
        dense[where] = deltas
        dense = dense.view(m, N, 32)
        torch.cuda.synchronize()
        reps = 3 if E >= 1 << 20 else 10 if E >= 1 << 14 else 30
        dreps = 3 if m >= 65536 else 10 if m >= 4096 else 30
        up = lambda: crs.update(deltas, idx, row_ptr, base=base[:m], want=ALL)
        dn = lambda: crs.commit(dense)
        if m == ms[0] and k == ks[0]:      # the two routes mean the same: update without a base = the dense commitment
            assert bytes(crs.update(deltas, idx, row_ptr, want=("prj",))["prj"].cpu().numpy()) == bytes(dn()["prj"].cpu().numpy())
        u_wall, d_wall = timed(up, reps) * 1e6 / m, timed(dn, dreps) * 1e6 / m
        dev.enable_timings(1)
        ut, dt = [], []
        for _ in range(min(reps, 5)):
            up()
            ut.append(crs.last_timings())
            dn()
            dt.append(crs.last_timings())
        dev.set_option("timings", 0)
        uk, uf = min(t["commit"] for t in ut) * 1e3 / m, min(t["finish"] for t in ut) * 1e3 / m
        dk, df = min(t["commit"] for t in dt) * 1e3 / m, min(t["finish"] for t in dt) * 1e3 / m
        ratio[(k, m)] = d_wall / u_wall
        say(f"  {k:3d} {m:7d}   {u_wall:19.2f} {uk:13.3f} {uf:13.3f}   {d_wall:18.2f} {dk:13.3f} {df:13.3f}   {ratio[(k, m)]:10.2f}x")
        del dense, where
    say("# crossover: per m, the k of the sweep at which the dense kernel is ahead of the update (wall)")
    for m in ms:
        behind = [k for k in ks if (k, m) in ratio and ratio[(k, m)] < 1.0]
        say(f"#   m = {m:6d}: " + ("dense ahead at k = " + ", ".join(str(k) for k in behind) if behind else "update ahead at every k measured"))
    if (4, 4096) in ratio:
        r = ratio[(4, 4096)]
        say(f"# required (k = 4, m = 4096: update faster than the dense baseline of the same run): {r:.2f}x -- {'met' if r > 1.0 else 'NOT met'}")
    crs.close()
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
