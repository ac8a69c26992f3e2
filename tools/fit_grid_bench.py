#!/usr/bin/env python3
"""The fit of samples on a tensor-product grid (splpak_fit_grid_dev_*) at the sizes of an image and a volume, beside the point
fit of the same samples listed as points.

Shapes: 512^3 -> 64^3, 256^3 -> 64^3, 4096^2 -> 64^2, 48^4 -> 16^4 nodes on the unit box, sorted evenly spaced axes, unit weights,
xtrap = 0; storage f64 and f32; refinement on (the default) and off (option fit_grid_refine = 0).  Per leg: `--warmup` untimed
calls, then `--reps` calls timed one by one with the host clock -- every call ends in a synchronise of the stream --, the median
with min and max; beside it what the call itself reports (info[5] seconds in the host tables, info[7] seconds on the device,
the refinement steps) and the bytes of `values` per second of device time.  With refinement off the device time is the spread
passes, the solves and the store: values_TBps_device is then the rate at which the first pass would have to read `values` if
everything else were free, a LOWER bound of its rate, to be held against the copy bandwidth measured in the same run
(`copy`: torch clone of the same samples, bytes read + written) and the 4.4 - 6.3 TB/s of DESIGN section 6.
At 256^3 -> 64^3 and 48^4 -> 16^4 the same samples are also fitted by splpak_plan_fit_dev on the listed points.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_grid_bench.py [--reps 5] [--warmup 2] [--small] [--legs 512c,256c,4096s,48q] [--no-point-fit] [--out FILE]
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

LEGS = {"512c": ([512] * 3, [64] * 3, False), "256c": ([256] * 3, [64] * 3, True), "4096s": ([4096] * 2, [64] * 2, False),
        "48q": ([48] * 4, [16] * 4, True)}
SMALL = {"512c": ([64] * 3, [16] * 3, False), "256c": ([48] * 3, [12] * 3, True), "4096s": ([512] * 2, [32] * 2, False),
         "48q": ([12] * 4, [6] * 4, True)}


def median3(t):
    return {"ms": 1e3 * statistics.median(t), "ms_min": 1e3 * min(t), "ms_max": 1e3 * max(t)}


def samples(npts, dev, dtype):
    """A smooth field plus noise on the grid, dimension 1 fastest."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    v = torch.zeros(npts[::-1], dtype=torch.float64, device=dev)
    for d, n in enumerate(npts):
        shape = [1] * len(npts)
        shape[len(npts) - 1 - d] = n
        v = v + torch.sin((2.0 + d) * torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev)).reshape(shape)
    v = v + 0.01 * torch.randn(v.shape, dtype=torch.float64, device=dev, generator=gen)
    return v.to(dtype).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="512c,256c,4096s,48q")
    ap.add_argument("--small", action="store_true", help="rehearsal sizes (overheads only, not a measurement)")
    ap.add_argument("--no-point-fit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_grid_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    results = []
    for leg in a.legs.split(","):
        npts, nodes, point_fit = (SMALL if a.small else LEGS)[leg]
        nd = len(npts)
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol = int(np.prod(nodes))
        nsamp = int(np.prod(npts))
        coef64 = None
        for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
            axes = torch.cat([torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev) for n in npts]).to(dtype)
            values = samples(npts, dev, dtype)
            coef = torch.zeros(ncol, dtype=dtype, device=dev)
            nbytes = values.numel() * values.element_size()
            # the yardstick of this run: a device copy of the same samples
            for _ in range(2):
                values.clone()
            stream.synchronize()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                values.clone()
                stream.synchronize()
                t.append(time.perf_counter() - t0)
            copy_tbps = 2.0 * nbytes / statistics.median(t) / 1e12
            for refine in (None, 0):
                capi.set_default_option("fit_grid_refine", refine)
                try:
                    def call():
                        rc, info = capi.fit_grid_dev(nd, npts, axes, values, lo, hi, nodes, coef, stream=st)
                        assert rc == 0, rc
                        return info[0]
                    for _ in range(a.warmup):
                        call()
                    stream.synchronize()
                    t, infos = [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        infos.append(call())
                        stream.synchronize()
                        t.append(time.perf_counter() - t0)
                    stats = capi.debug_fit_grid_stats()
                finally:
                    capi.set_default_option("fit_grid_refine", None)
                dev_s = statistics.median(i[7] for i in infos)
                passes = 1 + 2 * int(infos[-1][2])          # over `values`-sized data: the spread; per step the evaluation and the spread
                r = {"leg": leg, "npts": npts, "nodes": nodes, "storage": name, "refine": "on" if refine is None else "off",
                     **median3(t), "host_tables_ms": 1e3 * statistics.median(i[5] for i in infos), "device_ms": 1e3 * dev_s,
                     "refinement_steps": int(infos[-1][2]), "last_correction": float(infos[-1][3]), "slabs": stats[0],
                     "values_bytes": nbytes, "values_TBps_device": nbytes / dev_s / 1e12,
                     "passes_over_the_data": passes, "copy_TBps_same_run": copy_tbps}
                if name == "f64" and refine is None:
                    coef64 = coef.clone()
                results.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
            del values, axes
        if point_fit and not a.no_point_fit:
            # the same samples listed as points, through the plan entry (the point fit is what the grid entry replaces)
            values = samples(npts, dev, torch.float64)
            ax = [torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=dev) for n in npts]
            grids = torch.meshgrid(*ax[::-1], indexing="ij")
            x = torch.stack([g.reshape(-1) for g in grids[::-1]], dim=1).contiguous()
            del grids
            y = values.reshape(-1)
            c = torch.zeros(ncol, dtype=torch.float64, device=dev)
            t0 = time.perf_counter()
            plan = capi.Plan(nd, nodes, lo, hi, 0.0, nsamp)
            t_plan = time.perf_counter() - t0
            try:
                t = []
                info = None
                for k in range(1 + max(a.reps // 2, 1)):          # one untimed fit, then the timed ones
                    t0 = time.perf_counter()
                    rc, info = plan.fit(x, y, None, c, st)
                    stream.synchronize()
                    assert rc == 0, rc
                    if k > 0:
                        t.append(time.perf_counter() - t0)
                err = float((c - coef64).abs().max() / coef64.abs().max()) if coef64 is not None else None
                r = {"leg": leg, "npts": npts, "nodes": nodes, "point_fit": True, **median3(t), "plan_create_ms": 1e3 * t_plan,
                     "xdata_bytes": x.numel() * 8, "refinement_steps": int(info[2]), "factorisation": plan.factorisation()[1][:80],
                     "grid_fit_vs_point_fit_relmax": err}
            finally:
                plan.close()
            results.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            del x, y, values, c
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "small": a.small, "reps": a.reps, "warmup": a.warmup, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
