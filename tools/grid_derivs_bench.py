#!/usr/bin/env python3
"""Value, gradient and Hessian on a regular grid: one fused call (splpak_eval_grid_derivs_dev_*) against what a caller
does without it -- one splpak_eval_grid_dev_* call per nderiv pattern into the same planes.

Rows: 3-D 64^3 nodes -> 256^3 outputs, order 1 and 2, real64 and REAL32; 4-D 32^4 nodes -> 64^4 outputs, order 1 and 2,
real64.  Per leg: `--warmup` untimed calls, then `--reps` calls timed one by one with device events, the two legs
alternating; medians with min and max.  Planes >= 1 are compared for equality once, outside the timed region (plane 0 of
the loop uses the closed-form value tables: equal to rounding only).  A row is DONE when the median of the fused call is
below the minimum of the loop.  Prints one JSON line.

    python tools/grid_derivs_bench.py [--shapes 3d,4d] [--reps 10] [--warmup 3] [--small]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from splpak_amd import capi

SHAPES = {"3d": ([64, 64, 64], [256, 256, 256], (torch.float64, torch.float32)),
          "4d": ([32, 32, 32, 32], [64, 64, 64, 64], (torch.float64,))}
SMALL = {"3d": ([16, 16, 16], [64, 48, 40], (torch.float64, torch.float32)),
         "4d": ([8, 8, 8, 8], [20, 12, 10, 9], (torch.float64,))}      # rehearsal sizes


def patterns(nd, order):
    pats = [None] + [[int(e == d) for e in range(nd)] for d in range(nd)]
    if order == 2:
        pats += [[int(e == d) + int(e == f) for e in range(nd)] for d in range(nd) for f in range(d, nd)]
    return pats


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def one(name, nodes, npts, dtype, order, reps, warmup):
    nd = len(nodes)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    lo, hi = [0.0] * nd, [1.0] * nd
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    coef = torch.randn(int(np.prod(nodes)), dtype=torch.float64, device=dev, generator=gen).to(dtype)
    cat = torch.cat([torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev).to(dtype) for n in npts])
    nout = int(np.prod(npts))
    pats = patterns(nd, order)
    out_f = torch.empty((len(pats), nout), dtype=dtype, device=dev)
    out_l = torch.empty((len(pats), nout), dtype=dtype, device=dev)

    def fused():
        assert capi.evaluate_grid_derivs_dev(nd, npts, cat, order, coef, lo, hi, nodes, out_f, st) == 0

    def loop():
        for e, pat in enumerate(pats):
            assert capi.evaluate_grid_dev(nd, npts, cat, pat, coef, lo, hi, nodes, out_l[e], st) == 0

    for _ in range(warmup):
        loop()
        fused()
    torch.cuda.synchronize()
    tiles = capi.debug_eval_grid_stats()          # of the fused call, the thread's last grid call
    equal = bool(torch.equal(out_f[1:], out_l[1:]))
    value_rel = float((out_f[0].double() - out_l[0].double()).abs().max() / out_l[0].double().abs().max())
    tf, tl = [], []
    for _ in range(reps):
        tf.append(timed(fused))
        tl.append(timed(loop))
    f, l = statistics.median(tf), statistics.median(tl)
    return {"shape": name, "dtype": str(dtype).replace("torch.", ""), "order": order, "nodes": nodes, "npts": npts, "planes": len(pats),
            "outputs_per_plane": nout, "planes_ge1_equal": equal, "plane0_relmax": value_rel,
            "tile": capi.debug_eval_grid_derivs_tile(nd, order), "tiles_lds": tiles[0], "tiles_general": tiles[1],
            "fused_s": f, "fused_s_min": min(tf), "fused_s_max": max(tf), "loop_s": l, "loop_s_min": min(tl), "loop_s_max": max(tl),
            "ratio": l / f, "done": f < min(tl),
            "scratch_bytes": capi.eval_grid_derivs_scratch_bytes(npts, order)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3d,4d")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (overheads only, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grid_derivs_bench: no GPU; nothing is measured without one")
    res = []
    for name in a.shapes.split(","):
        nodes, npts, dtypes = (SMALL if a.small else SHAPES)[name]
        for dtype in dtypes:
            for order in (1, 2):
                res.append(one(name, nodes, npts, dtype, order, a.reps, a.warmup))
                torch.cuda.empty_cache()
    capi.shutdown()
    print(json.dumps({"device": capi.device_name(), "small": a.small, "results": res}))


if __name__ == "__main__":
    main()
