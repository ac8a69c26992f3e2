#!/usr/bin/env python3
"""Resampling a fit onto a regular grid: the grid route (splpak_eval_grid_dev_*) against what a caller does
without it -- splpak_eval_dev_* in automatic mode on the Cartesian product of the axes as a query list that is
already resident in device memory (its construction is timed separately and not counted against that leg).

Shapes: 3-D 64^3 nodes -> 512^3 outputs, 4-D 32^4 nodes -> 96^4 outputs; real64 and REAL32.  Per leg: `--warmup`
untimed calls, then `--reps` calls timed one by one with device events, the two legs alternating; medians.
Outputs are compared for equality once, outside the timed region.  Prints one JSON line.

    python tools/grid_eval_bench.py [--shapes 3d,4d] [--reps 10] [--warmup 3] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from splpak_amd import capi

HBM_PEAK = 8.0e12      # bytes/s (specification; the share of the store floor is quoted against it, as DESIGN section 6 does)
SHAPES = {"3d": ([64, 64, 64], [512, 512, 512]), "4d": ([32, 32, 32, 32], [96, 96, 96, 96])}
SMALL = {"3d": ([16, 16, 16], [64, 48, 40]), "4d": ([8, 8, 8, 8], [20, 12, 10, 9])}      # rehearsal sizes


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def one(name, nodes, npts, dtype, reps, warmup):
    nd = len(nodes)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    lo, hi = [0.0] * nd, [1.0] * nd
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    coef = torch.randn(int(np.prod(nodes)), dtype=torch.float64, device=dev, generator=gen).to(dtype)
    axes = [torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev).to(dtype) for n in npts]
    cat = torch.cat(axes)
    nout = int(np.prod(npts))
    out_g = torch.empty(nout, dtype=dtype, device=dev)
    out_p = torch.empty(nout, dtype=dtype, device=dev)
    # the query list of the point route, dimension 1 fastest (the ordering of the grid entry's output)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = torch.meshgrid(*axes[::-1], indexing="ij")
    q = torch.stack([m.reshape(-1) for m in mesh[::-1]], dim=1).contiguous()
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    del mesh
    grid = lambda: capi.evaluate_grid_dev(nd, npts, cat, None, coef, lo, hi, nodes, out_g, st)
    point = lambda: capi.evaluate_dev(nd, q, None, coef, lo, hi, nodes, out_p, st)
    capi.set_eval_mode(capi.EVAL_AUTO)
    for _ in range(warmup):
        assert grid() == 0 and point() == 0
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_g, out_p))
    tiles = capi.debug_eval_grid_stats()
    tg, tp = [], []
    for _ in range(reps):
        tg.append(timed(grid))
        tp.append(timed(point))
    g, p = statistics.median(tg), statistics.median(tp)
    esz = out_g.element_size()
    return {"shape": name, "dtype": str(dtype).replace("torch.", ""), "nodes": nodes, "npts": npts, "outputs": nout,
            "equal": equal, "tiles_lds": tiles[0], "tiles_general": tiles[1],
            "grid_s": g, "grid_s_min": min(tg), "grid_s_max": max(tg), "point_s": p, "point_s_min": min(tp), "point_s_max": max(tp),
            "grid_outputs_per_s": nout / g, "point_outputs_per_s": nout / p, "ratio": p / g,
            "store_floor_fraction": nout * esz / g / HBM_PEAK,
            "query_list_bytes": q.numel() * q.element_size(), "query_list_build_s": t_build,
            "grid_scratch_bytes": capi.eval_grid_scratch_bytes(npts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3d,4d")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (overheads only, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grid_eval_bench: no GPU; nothing is measured without one")
    res = []
    for name in a.shapes.split(","):
        nodes, npts = (SMALL if a.small else SHAPES)[name]
        for dtype in (torch.float64, torch.float32):
            res.append(one(name, nodes, npts, dtype, a.reps, a.warmup))
            torch.cuda.empty_cache()
    capi.shutdown()
    print(json.dumps({"device": capi.device_name(), "hbm_peak_bytes_per_s": HBM_PEAK, "small": a.small, "results": res}))


if __name__ == "__main__":
    main()
