#!/usr/bin/env python3
"""Many small fits in one launch (splpak_fit_many_dev_f64) beside a loop of splpak_plan_fit_dev over one cached plan.

Legs: batches of BASELINE config 1's shape (1-D, 10^3 points, 16 nodes, xtrap = 1, unit box) at nbatch = 1, 10^2, 10^4 and
10^5, and a 2-D leg at the largest near-square grid the LDS rule admits with 2 000 points per problem at nbatch = 10^4.  Every
problem has its own points and values (uniform points, a smooth field plus noise), resident on the device.  Per leg: `--warmup`
untimed calls, then `--reps` calls timed one by one with the host clock (every call ends in a synchronise of the stream), the
median with min and max; problems/s and points/s; what the call reports as device time; and the fraction of the HBM rate
(`--hbm-gbs`, default the MI355X's 8 000 GB/s) that the bytes of the points (coordinates and values) amount to.
The comparator, in the same run: one plan of the leg's grid, splpak_plan_fit_dev on `--loop` of the same problems one after the
other (default 1 000, or nbatch if that is smaller), timed as one loop, per problem.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_many_bench.py [--reps 5] [--warmup 2] [--loop 1000] [--legs 1,100,10000,100000,2d] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from splpak_amd import capi
from tools.fit_grid_bench import median3

LDS_BUDGET = 65536


def largest_square():
    n = 4
    while capi.fit_many_lds_bytes(2, [n + 1, n + 1]) <= LDS_BUDGET:
        n += 1
    return [n + 1, n] if capi.fit_many_lds_bytes(2, [n + 1, n]) <= LDS_BUDGET else [n, n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop", type=int, default=1000)
    ap.add_argument("--legs", default="1,100,10000,100000,2d")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_many_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    results = []
    for leg in a.legs.split(","):
        if leg == "2d":
            nd, nodes, npp, nbatch = 2, largest_square(), 2000, 10000
        else:
            nd, nodes, npp, nbatch = 1, [16], 1000, int(leg)
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol = int(np.prod(nodes))
        gen = torch.Generator(device=dev)
        gen.manual_seed(31)
        x = torch.rand((nbatch * npp, nd), dtype=torch.float64, device=dev, generator=gen)
        y = torch.sin(3.0 * x[:, 0]) + 0.5 * torch.cos(2.0 * x[:, -1]) + 0.05 * torch.randn(nbatch * npp, dtype=torch.float64, device=dev, generator=gen)
        y = y.contiguous()
        offsets = np.arange(nbatch + 1, dtype=np.int64) * npp
        coef = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
        t, infos = [], []
        for k in range(a.warmup + a.reps):
            stream.synchronize()
            t0 = time.perf_counter()
            rc, status, info = capi.fit_many_dev(nd, offsets, x, y, None, lo, hi, nodes, coef, xtrap=1.0, stream=st)
            stream.synchronize()
            dt = time.perf_counter() - t0
            assert rc == 0 and not status.any(), rc
            if k >= a.warmup:
                t.append(dt)
                infos.append(info)
        stats = capi.debug_fit_many_stats()
        med = median3(t)
        dev_s = float(np.median([i[0, 7] * nbatch for i in infos]))
        nbytes = nbatch * npp * (nd + 1) * 8
        # the comparator: one cached plan, one fit per problem
        nloop = min(a.loop, nbatch)
        plan = capi.Plan(nd, nodes, lo, hi, 1.0, npp)
        c1 = torch.zeros(ncol, dtype=torch.float64, device=dev)
        worst = 0.0
        try:
            for timed in (False, True):
                stream.synchronize()
                t0 = time.perf_counter()
                for k in range(nloop):
                    rc, _ = plan.fit(x[k * npp:(k + 1) * npp], y[k * npp:(k + 1) * npp], None, c1, st)
                    assert rc == 0, rc
                    if not timed and k < 8:
                        worst = max(worst, float((c1 - coef[k]).abs().max() / c1.abs().max()))
                stream.synchronize()
                t_loop = time.perf_counter() - t0
        finally:
            plan.close()
        r = {"leg": leg, "ndim": nd, "nodes": nodes, "points_per_problem": npp, "nbatch": nbatch, **med,
             "problems_per_s": nbatch / (1e-3 * med["ms"]), "points_per_s": nbatch * npp / (1e-3 * med["ms"]),
             "device_ms": 1e3 * dev_s, "points_bytes": nbytes, "hbm_fraction_host_clock": nbytes / (1e-3 * med["ms"]) / (a.hbm_gbs * 1e9),
             "hbm_fraction_device_time": nbytes / dev_s / (a.hbm_gbs * 1e9) if dev_s > 0 else None,
             "workgroups": stats[0], "lds_bytes": stats[1], "launches": stats[2], "max_refinement_steps": stats[5],
             "plan_loop_problems": nloop, "plan_loop_ms_per_problem": 1e3 * t_loop / nloop, "plan_loop_problems_per_s": nloop / t_loop,
             "plan_loop_points_per_s": nloop * npp / t_loop, "batch_vs_plan_loop_relmax_first8": worst,
             "speedup_per_problem": (t_loop / nloop) / (1e-3 * med["ms"] / nbatch)}
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del x, y, coef
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "reps": a.reps, "warmup": a.warmup, "hbm_gbs": a.hbm_gbs, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
