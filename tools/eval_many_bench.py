#!/usr/bin/env python3
"""A batch of small fits at each problem's own points in one launch (splpak_eval_many_dev_f64, splpak_residuals_many_dev_f64)
beside a loop of splpak_eval_dev_f64 over the problems.

Legs, each for both families: 1-D, 16 nodes, 10^3 points per problem at nbatch = 1, 10^2, 10^4 and 10^5; 2-D, 12 x 12 nodes, 2 000
points, nbatch = 10^4 ("2d"); 10^5 problems of 8 queries ("small"); 4 problems of 2.5 10^6 queries ("big").  Coefficients are
random normals, one set per problem; points are uniform on the unit box, values random, weights U[0.5, 2] with 10 % exact zeros;
everything is resident on the device.  Per leg: `--warmup` untimed calls, then `--reps` calls timed one by one with the host
clock around the _dev entry followed by a synchronise of the stream: the median with min and max; problems/s, queries/s, and the
fraction of the HBM rate (`--hbm-gbs`, default the MI355X's 8 000 GB/s) the algorithmic bytes amount to -- 8 (ndim + 1) per query,
plus 16 per point for y, w and resid in the residual legs.
The comparator, in the same run and timed the same way (each repetition is one loop): splpak_eval_dev_f64 under EVAL_DIRECT over
`--loop` of the same problems one after the other (default 1 000, or nbatch if that is smaller), per problem; for the residual
legs the loop adds the torch subtraction, weighting and reductions a caller would write.
Prints one JSON line; --out writes it to a file as well.

    python tools/eval_many_bench.py [--reps 5] [--warmup 2] [--loop 1000] [--legs 1,100,10000,100000,2d,small,big] [--out FILE]
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


def timed(fn, stream, warmup, reps):
    t = []
    for k in range(warmup + reps):
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        if k >= warmup:
            t.append(time.perf_counter() - t0)
    return median3(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop", type=int, default=1000)
    ap.add_argument("--legs", default="1,100,10000,100000,2d,small,big")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_many_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    results = []
    for leg in a.legs.split(","):
        if leg == "2d":
            nd, nodes, npp, nbatch = 2, [12, 12], 2000, 10000
        elif leg == "small":
            nd, nodes, npp, nbatch = 1, [16], 8, 100000
        elif leg == "big":
            nd, nodes, npp, nbatch = 1, [16], 2500000, 4
        else:
            nd, nodes, npp, nbatch = 1, [16], 1000, int(leg)
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol, n = int(np.prod(nodes)), nbatch * npp
        gen = torch.Generator(device=dev)
        gen.manual_seed(37)
        x = torch.rand((n, nd), dtype=torch.float64, device=dev, generator=gen)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        w = 0.5 + 1.5 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        w[torch.rand(n, dtype=torch.float64, device=dev, generator=gen) < 0.1] = 0.0
        w[::npp] = 1.0      # (a first weight that is not negative: the weights count)
        coef = torch.randn((nbatch, ncol), dtype=torch.float64, device=dev, generator=gen)
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        stats = torch.zeros((nbatch, 4), dtype=torch.float64, device=dev)
        offsets = np.arange(nbatch + 1, dtype=np.int64) * npp
        nloop = min(a.loop, nbatch)
        loop_stats = torch.zeros((nloop, 4), dtype=torch.float64, device=dev)

        def eval_many():
            assert capi.evaluate_many_dev(nd, offsets, x, None, coef, lo, hi, nodes, out, stream=st) == 0

        def residuals_many():
            assert capi.residuals_many_dev(nd, offsets, x, y, w, coef, lo, hi, nodes, out, stats, stream=st) == 0

        def eval_loop():
            for k in range(nloop):
                s = slice(k * npp, (k + 1) * npp)
                capi.evaluate_dev(nd, x[s], None, coef[k], lo, hi, nodes, out[s], st)

        def residuals_loop():
            for k in range(nloop):
                s = slice(k * npp, (k + 1) * npp)
                capi.evaluate_dev(nd, x[s], None, coef[k], lo, hi, nodes, out[s], st)
                r = y[s] - out[s]
                out[s] = r
                t = (w[s] * r).abs()
                m, idx = t.max(0)
                loop_stats[k, 0] = (w[s] != 0.0).sum()
                loop_stats[k, 1] = (t * t).sum()
                loop_stats[k, 2] = m
                loop_stats[k, 3] = idx

        capi.set_eval_mode(capi.EVAL_DIRECT)
        try:
            for family, many, loop, per_point in (("eval_many", eval_many, eval_loop, 8 * (nd + 1)),
                                                  ("residuals_many", residuals_many, residuals_loop, 8 * (nd + 1) + 16)):
                med = timed(many, stream, a.warmup, a.reps)
                counters = capi.debug_eval_many_stats()
                lp = timed(loop, stream, a.warmup, a.reps)
                per_many = {k: v / nbatch for k, v in med.items()}
                per_loop = {k: v / nloop for k, v in lp.items()}
                nbytes = n * per_point
                r = {"leg": leg, "family": family, "ndim": nd, "nodes": nodes, "points_per_problem": npp, "nbatch": nbatch, **med,
                     "problems_per_s": nbatch / (1e-3 * med["ms"]), "queries_per_s": n / (1e-3 * med["ms"]), "algorithmic_bytes": nbytes,
                     "hbm_fraction": nbytes / (1e-3 * med["ms"]) / (a.hbm_gbs * 1e9), "workgroups": counters[0], "launches": counters[1],
                     "sweep_queries": counters[4], "ms_per_problem": per_many["ms"], "ms_per_problem_min": per_many["ms_min"],
                     "ms_per_problem_max": per_many["ms_max"], "loop_problems": nloop, "loop_ms_per_problem": per_loop["ms"],
                     "loop_ms_per_problem_min": per_loop["ms_min"], "loop_ms_per_problem_max": per_loop["ms_max"],
                     "loop_over_batch_per_problem": per_loop["ms"] / per_many["ms"],
                     "ranges_overlap": not (per_many["ms_max"] < per_loop["ms_min"] or per_loop["ms_max"] < per_many["ms_min"])}
                results.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        finally:
            capi.set_eval_mode(capi.EVAL_AUTO)
        del x, y, w, coef, out, stats, loop_stats
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "reps": a.reps, "warmup": a.warmup, "hbm_gbs": a.hbm_gbs, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
