#!/usr/bin/env python3
"""Kernel-trace summary of ONE batched refit at BASELINE config 3 (tools/refit_bench.py's set-up): profiles/refit_batch_kernel_stats.csv.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/refit_batch_profile.py run [--nfields 8]
    python tools/refit_batch_profile.py summary OUT profiles/refit_batch_kernel_stats.csv [--nfields 8]

`run`: a fit, a warm-up refit of `nfields` fields (it allocates the per-field copies) and the refit that is summarised.  `summary`:
the dispatches of that last refit -- everything from its first values gather on, the nfields-th `regather_values_kernel` from the
end of the trace -- by kernel, in the columns of rocprofv3's own kernel statistics.  A trace without counters, in a run of its own.
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a):
    import torch
    from splpak_amd import capi
    nd, m = 3, a.ndata
    nodes, lo, hi = [a.nodes] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    y = torch.empty(m, dtype=torch.float64, device=dev)
    w = torch.empty(m, dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, y, w, st)
    sx = x.sum(dim=1)
    Y = torch.stack([torch.cos((3.0 + k) * sx) for k in range(a.nfields)])
    ncol = a.nodes ** nd
    C = torch.zeros((a.nfields, ncol), dtype=torch.float64, device=dev)
    plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)
    rc, _ = plan.fit(x, y, w, C[0], st)
    assert rc == 0
    for _ in range(2):
        rc, info = plan.refit(Y, C, st)
        assert rc == 0 and plan.refit_stats()[0] == 2, plan.refit_stats()
    torch.cuda.synchronize()
    print("refit_batch_profile: steps", [int(v) for v in info[:, 2]], "stats", plan.refit_stats())
    plan.close()


def summary(a):
    files = sorted(glob.glob(os.path.join(a.trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {a.trace_dir}"
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    gathers = [i for i, r in enumerate(rows) if "regather_values_kernel" in r["Kernel_Name"]]
    assert len(gathers) >= a.nfields, (len(gathers), a.nfields)
    last = rows[gathers[-a.nfields]:]
    by = {}
    for r in last:
        by.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in by.values())
    with open(a.out, "w", newline="") as f:
        wr = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        wr.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
            d = np.array(v, dtype=np.float64)
            wr.writerow([name, len(v), int(d.sum()), round(float(d.mean()), 6), round(100.0 * d.sum() / total, 2), int(d.min()), int(d.max()),
                         round(float(d.std(ddof=1)) if len(v) > 1 else 0.0, 6)])
    span = int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])
    print(f"refit_batch_profile: {len(last)} dispatches of the last refit, {total / 1e6:.3f} ms in kernels over a span of {span / 1e6:.3f} ms -> {a.out}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--nodes", type=int, default=64)
    r.add_argument("--ndata", type=int, default=10_000_000)
    r.add_argument("--nfields", type=int, default=8)
    s = sub.add_parser("summary")
    s.add_argument("trace_dir")
    s.add_argument("out")
    s.add_argument("--nfields", type=int, default=8)
    a = ap.parse_args()
    run(a) if a.cmd == "run" else summary(a)


if __name__ == "__main__":
    main()
