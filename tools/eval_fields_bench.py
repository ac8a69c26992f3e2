#!/usr/bin/env python3
"""Several fields at the same points: one splpak_eval_fields_dev_* call (leg a) against what a caller does without it --
one splpak_eval_dev_* call per field on the same resident data (leg b) -- in automatic mode.

Shapes (nfields = 3, scattered uniform queries, random normal coefficients):
    3d      64^3 nodes, 5e7 queries, real64 and REAL32      the shared sort
    4d      32^4 nodes, 1e8 queries, real64                 the shared sort
    3d-few  64^3 nodes, 2^19 queries, real64                below the threshold of the sorted paths: the direct fields kernel
    2d      64 x 64 nodes, 1e7 queries, real64              2-D is never sorted: the direct fields kernel
    4d-few  32^4 nodes, 2^19 queries, real64                the direct fields kernel on a 256-coefficient window
Per row: `--warmup` untimed calls of each leg, then `--reps` rounds timed with device events, the two legs alternating;
medians with min and max.  Outputs are compared with torch.equal once, outside the timed region; the route leg (a) took is
read from splpak_debug_eval_fields_stats.  Prints one JSON line.

    python tools/eval_fields_bench.py [--shapes 3d,4d,3d-few,2d,4d-few] [--nfields 3] [--reps 10] [--warmup 3] [--small]
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

F64, F32 = torch.float64, torch.float32
SHAPES = {"3d": ([64, 64, 64], 50_000_000, (F64, F32)), "4d": ([32, 32, 32, 32], 100_000_000, (F64,)),
          "3d-few": ([64, 64, 64], 2 ** 19, (F64,)), "2d": ([64, 64], 10_000_000, (F64,)), "4d-few": ([32, 32, 32, 32], 2 ** 19, (F64,))}
SMALL = {"3d": ([40, 40, 40], 2 ** 20 + 5, (F64, F32)), "4d": ([16, 16, 16, 16], 2 ** 20 + 5, (F64,)),       # rehearsal sizes
         "3d-few": ([40, 40, 40], 2 ** 12, (F64,)), "2d": ([64, 64], 2 ** 16, (F64,)), "4d-few": ([16, 16, 16, 16], 2 ** 12, (F64,))}
ROUTES = {0: "none", 1: "direct fields kernel", 2: "shared sort", 3: "per-field loop"}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def one(name, nodes, nq, dtype, nfields, reps, warmup):
    nd = len(nodes)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    lo, hi = [0.0] * nd, [1.0] * nd
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ncol = int(np.prod(nodes))
    coef = torch.randn((nfields, ncol), dtype=F64, device=dev, generator=gen).to(dtype)
    q = torch.rand((nq, nd), dtype=F64, device=dev, generator=gen).to(dtype)
    out_a = torch.empty((nfields, nq), dtype=dtype, device=dev)
    out_b = torch.empty((nfields, nq), dtype=dtype, device=dev)

    def fields():
        assert capi.evaluate_fields_dev(nd, q, None, coef, lo, hi, nodes, out_a, st) == 0

    def singles():
        for k in range(nfields):
            assert capi.evaluate_dev(nd, q, None, coef[k], lo, hi, nodes, out_b[k], st) == 0

    capi.set_eval_mode(capi.EVAL_AUTO)
    for _ in range(warmup):
        fields()
        singles()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_a, out_b))
    stats = capi.debug_eval_fields_stats()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fields))
        tb.append(timed(singles))
    a, b = statistics.median(ta), statistics.median(tb)
    return {"shape": name, "dtype": str(dtype).replace("torch.", ""), "nodes": nodes, "queries": nq, "nfields": nfields,
            "equal": equal, "route": ROUTES[stats[0]], "place_passes": stats[1], "eval_launches": stats[2],
            "fields_s": a, "fields_s_min": min(ta), "fields_s_max": max(ta),
            "singles_s": b, "singles_s_min": min(tb), "singles_s_max": max(tb),
            "ratio": b / a, "fields_median_below_singles_min": a < min(tb), "fields_median_above_singles_max": a > max(tb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3d,4d,3d-few,2d,4d-few")
    ap.add_argument("--nfields", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (routes and overheads only, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_fields_bench: no GPU; nothing is measured without one")
    res = []
    for name in a.shapes.split(","):
        nodes, nq, dtypes = (SMALL if a.small else SHAPES)[name]
        for dtype in dtypes:
            res.append(one(name, nodes, nq, dtype, a.nfields, a.reps, a.warmup))
            torch.cuda.empty_cache()
    name = capi.device_name()
    capi.shutdown()
    print(json.dumps({"device": name, "small": a.small, "results": res}))


if __name__ == "__main__":
    main()
