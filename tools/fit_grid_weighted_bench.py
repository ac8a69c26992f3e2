#!/usr/bin/env python3
"""The grid fit with a weight per sample (splpak_fit_grid_weighted_dev_*) at the sizes of an image and a volume, beside the
unweighted grid fit of the same samples and the point fit of the listed samples.

Shapes: 512^3 -> 64^3, 4096^2 -> 64^2 and 256^3 -> 64^3 nodes on the unit box, sorted evenly spaced axes, xtrap = 0, weights
U[0.5, 2] with 10 % of the samples dead (weight 0, value NaN); storage f64 and f32.  Per leg and storage: `--warmup` untimed
calls, then `--reps` calls timed one by one with the host clock (every call ends in a synchronise of the stream), the median with
min and max; what the call reports (info[7] seconds on the device, refinement steps) and its counters (conjugate-gradient
iterations counted up to the first iterate within the tolerance, solves).  The cost of ONE iteration is measured directly: the
device time of a call capped at 10 iterations minus that of one capped at 5, refinement off, over 5 (the scalars are read back
every 5 iterations, so both run exactly their cap).  Beside it, in the same run, splpak_fit_grid_dev_* on the same samples with
the dead ones filled in and no weights, refined and unrefined: the difference over the steps is the cost of one refinement step
of the unweighted entry -- one evaluation, one spread, the solves -- which an iteration should cost plus the weight read.  At
256^3 -> 64^3 the samples of non-zero weight are also listed and fitted by splpak_plan_fit_dev.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_grid_weighted_bench.py [--reps 5] [--warmup 2] [--small] [--legs 512c,4096s,256c] [--no-point-fit] [--out FILE]
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
from tools.fit_grid_bench import median3, samples

LEGS = {"512c": ([512] * 3, [64] * 3, False), "4096s": ([4096] * 2, [64] * 2, False), "256c": ([256] * 3, [64] * 3, True)}
SMALL = {"512c": ([64] * 3, [16] * 3, False), "4096s": ([512] * 2, [32] * 2, False), "256c": ([48] * 3, [12] * 3, True)}
DEAD = 0.10


def timed(call, stream, warmup, reps):
    for _ in range(warmup):
        call()
    stream.synchronize()
    t, infos = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        infos.append(call())
        stream.synchronize()
        t.append(time.perf_counter() - t0)
    return t, infos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="512c,4096s,256c")
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (overheads only, not a measurement)")
    ap.add_argument("--no-point-fit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_grid_weighted_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    results = []
    for leg in a.legs.split(","):
        npts, nodes, point_fit = (SMALL if a.small else LEGS)[leg]
        nd = len(npts)
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol = int(np.prod(nodes))
        gen = torch.Generator(device=dev)
        gen.manual_seed(12)
        w64 = 0.5 + 1.5 * torch.rand(npts[::-1], dtype=torch.float64, device=dev, generator=gen)
        w64 = w64 * (torch.rand(npts[::-1], dtype=torch.float64, device=dev, generator=gen) >= DEAD)
        coef64 = None
        for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
            axes = torch.cat([torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev) for n in npts]).to(dtype)
            filled = samples(npts, dev, dtype)
            weights = w64.to(dtype).contiguous()
            values = torch.where(weights != 0, filled, torch.full_like(filled, float("nan")))
            coef = torch.zeros(ncol, dtype=dtype, device=dev)
            nbytes = values.numel() * values.element_size()

            def weighted():
                rc, info = capi.fit_grid_weighted_dev(nd, npts, axes, values, weights, lo, hi, nodes, coef, stream=st)
                assert rc == 0, rc
                return info[0]

            t, infos = timed(weighted, stream, a.warmup, a.reps)
            stats = capi.debug_fit_grid_weighted_stats()
            if name == "f64":
                coef64 = coef.clone()
            # one iteration: 10 against 5, refinement off
            capped = {}
            capi.set_default_option("fit_grid_refine", 0)
            try:
                for cap in (5, 10):
                    capi.set_default_option("fit_grid_weighted_maxit", cap)
                    _, ci = timed(weighted, stream, 1, a.reps)
                    capped[cap] = statistics.median(i[7] for i in ci)
            finally:
                capi.set_default_option("fit_grid_weighted_maxit", None)
                capi.set_default_option("fit_grid_refine", None)
            # the unweighted entry on the same samples, refined and not
            plain = {}
            for refine in (None, 0):
                capi.set_default_option("fit_grid_refine", refine)
                try:
                    def unweighted():
                        rc, info = capi.fit_grid_dev(nd, npts, axes, filled, lo, hi, nodes, coef, stream=st)
                        assert rc == 0, rc
                        return info[0]
                    tu, iu = timed(unweighted, stream, a.warmup, a.reps)
                finally:
                    capi.set_default_option("fit_grid_refine", None)
                plain[refine] = (tu, statistics.median(i[7] for i in iu), int(iu[-1][2]))
            steps_u = max(plain[None][2], 1)
            step_ms = 1e3 * (plain[None][1] - plain[0][1]) / steps_u
            dev_s = statistics.median(i[7] for i in infos)
            r = {"leg": leg, "npts": npts, "nodes": nodes, "storage": name, "dead_fraction": DEAD, **median3(t),
                 "device_ms": 1e3 * dev_s, "host_tables_ms": 1e3 * statistics.median(i[5] for i in infos),
                 "refinement_steps": int(infos[-1][2]), "cg_iterations_counted": stats[5], "cg_solves": stats[6], "slabs": stats[0],
                 "ms_per_cg_iteration": 1e3 * (capped[10] - capped[5]) / 5.0, "values_bytes": nbytes,
                 "unweighted_refined_ms": 1e3 * statistics.median(plain[None][0]), "unweighted_refined_device_ms": 1e3 * plain[None][1],
                 "unweighted_refinement_steps": plain[None][2], "unweighted_plain_device_ms": 1e3 * plain[0][1],
                 "unweighted_ms_per_refinement_step": step_ms}
            results.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            del values, filled, weights, axes
        if point_fit and not a.no_point_fit:
            # the samples of non-zero weight listed as points, through the plan entry
            filled = samples(npts, dev, torch.float64)
            ax = [torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev) for n in npts]
            grids = torch.meshgrid(*ax[::-1], indexing="ij")
            keep = (w64 != 0).reshape(-1)
            x = torch.stack([g.reshape(-1)[keep] for g in grids[::-1]], dim=1).contiguous()
            del grids
            y = filled.reshape(-1)[keep].contiguous()
            w = w64.reshape(-1)[keep].contiguous()
            c = torch.zeros(ncol, dtype=torch.float64, device=dev)
            t0 = time.perf_counter()
            plan = capi.Plan(nd, nodes, lo, hi, 0.0, int(x.shape[0]))
            t_plan = time.perf_counter() - t0
            try:
                t = []
                info = None
                for k in range(1 + max(a.reps // 2, 1)):          # one untimed fit, then the timed ones
                    t0 = time.perf_counter()
                    rc, info = plan.fit(x, y, w, c, st)
                    stream.synchronize()
                    assert rc == 0, rc
                    if k > 0:
                        t.append(time.perf_counter() - t0)
                err = float((c - coef64).abs().max() / coef64.abs().max()) if coef64 is not None else None
                r = {"leg": leg, "npts": npts, "nodes": nodes, "point_fit": True, "points": int(x.shape[0]), **median3(t),
                     "plan_create_ms": 1e3 * t_plan, "xdata_bytes": x.numel() * 8, "refinement_steps": int(info[2]),
                     "factorisation": plan.factorisation()[1][:80], "weighted_grid_fit_vs_point_fit_relmax": err}
            finally:
                plan.close()
            results.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            del x, y, w, filled, c
        del w64
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "small": a.small, "reps": a.reps, "warmup": a.warmup, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
