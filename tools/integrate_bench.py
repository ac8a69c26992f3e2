#!/usr/bin/env python3
"""Integrals on a tensor grid (splpak_integrate_grid_dev_f64) beside the grid evaluation they are built on.

3-D coefficients on 64^3 nodes, box [0, 1]^3:
  eval  splpak_eval_grid_dev_f64 at 512^3 points (the yardstick of the ratios; also what is compared between two builds)
  (a)   512^3 cells on sorted uniform edges
  (b)   one box over the grid
  (c)   1024 x 1024 points with z integrated over the whole grid (a projection)
Per leg: `--warmup` untimed calls, then `--reps` calls timed one by one with the host clock, each ending in a synchronise
of the stream; the median with min and max.  Beside each leg the bytes its construction moves by the model of DESIGN 6c
(from the piece counts the call reports) and the ratio to `eval`.  A build without the integrate entries measures `eval`
alone, so that the same script compares two builds.  Prints one JSON line.

    python tools/integrate_bench.py [--reps 5] [--warmup 2] [--small] [--legs eval,a,b,c]
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


def timed(fn, stream):
    t0 = time.perf_counter()
    fn()
    stream.synchronize()
    return time.perf_counter() - t0


def measure(fn, stream, reps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    t = [timed(fn, stream) for _ in range(reps)]
    return {"ms": 1e3 * statistics.median(t), "ms_min": 1e3 * min(t), "ms_max": 1e3 * max(t)}


def model_bytes(pieces, ncell, mode, ncol, slabs):
    """the piece products written once; every reduction reads its input and writes its result (the last one the
    outputs themselves); the tables (36 bytes per entry, written and read), the axes and the coefficients (read per slab)."""
    nd = len(ncell)
    dims = list(pieces)
    total = 8 * int(np.prod(dims)) if any(mode) else 0
    for d in range(nd):
        if not mode[d]:
            continue
        total += 8 * int(np.prod(dims))
        dims[d] = ncell[d]
        total += 8 * int(np.prod(dims))
    if not any(mode):
        total += 8 * int(np.prod(ncell))
    return total + 2 * 36 * sum(pieces) + 8 * sum(n + m for n, m in zip(ncell, mode)) + 8 * ncol * slabs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="eval,a,b,c")
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (overheads only, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("integrate_bench: no GPU; nothing is measured without one")
    legs = a.legs.split(",")
    have = hasattr(capi, "integrate_grid_dev")
    nodes = [16, 16, 16] if a.small else [64, 64, 64]
    n3, n2 = (64, 128) if a.small else (512, 1024)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    lo, hi = [0.0] * 3, [1.0] * 3
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    ncol = int(np.prod(nodes))
    coef = torch.randn(ncol, dtype=torch.float64, device=dev, generator=gen)
    res = {}

    def lin(n):
        return torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)

    if "eval" in legs:
        npts = [n3] * 3
        axes = torch.cat([lin(n3)] * 3)
        out = torch.empty(n3 ** 3, dtype=torch.float64, device=dev)
        r = measure(lambda: capi.evaluate_grid_dev(3, npts, axes, None, coef, lo, hi, nodes, out, st), stream, a.reps, a.warmup)
        r["bytes_model"] = 8 * n3 ** 3 + 8 * ncol + 2 * 36 * 3 * n3
        res["eval"] = r
        del out

    def integrate_leg(ncell, mode, axes):
        out = torch.empty(int(np.prod(ncell)), dtype=torch.float64, device=dev)
        r = measure(lambda: capi.integrate_grid_dev(3, ncell, mode, axes, coef, lo, hi, nodes, out, st), stream, a.reps, a.warmup)
        s = capi.debug_integrate_grid_stats()
        r.update({"slabs": s[0], "intermediate_doubles": s[1], "pieces": list(s[2:5]), "reduction_launches": s[6],
                  "bytes_model": model_bytes(list(s[2:5]), ncell, mode, ncol, s[0])})
        if "eval" in res:
            r["ratio_to_eval"] = r["ms"] / res["eval"]["ms"]
        return r

    if have and "a" in legs:
        res["a_cells"] = integrate_leg([n3] * 3, [1, 1, 1], torch.cat([lin(n3 + 1)] * 3))
    if have and "b" in legs:
        res["b_one_box"] = integrate_leg([1, 1, 1], [1, 1, 1], torch.tensor([0.0, 1.0] * 3, dtype=torch.float64, device=dev))
    if have and "c" in legs:
        res["c_projection"] = integrate_leg([n2, n2, 1], [0, 0, 1],
                                            torch.cat([lin(n2), lin(n2), torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)]))
    capi.shutdown()
    print(json.dumps({"device": capi.device_name(), "small": a.small, "integrate_entries": have, "nodes": nodes, "reps": a.reps,
                      "results": res}))


if __name__ == "__main__":
    main()
