#!/usr/bin/env python3
"""What the covariance costs: splpak_fit_many_cov_dev_f64 beside splpak_fit_many_dev_f64, and splpak_eval_many_var_dev_f64 beside
splpak_eval_many_dev_f64 on the same queries (every problem's own points).

Legs, those of DESIGN 4g's table: 1-D, 16 nodes, 10^3 points per problem, xtrap = 1, at nbatch = 10^2 and 10^4, and 2-D at the
largest near-square grid the LDS rule admits (12 x 12) with 2 000 points per problem at nbatch = 10^3.  Uniform points, a smooth
field plus noise, resident on the device.  Per pair of entries: `--warmup` untimed calls of each, then `--reps` timed calls of
each, ALTERNATING (a, b, a, b, ..) in one process, each timed with the host clock between two synchronisations of the stream;
the median with min and max, and the ratio of the medians.  Nobody has measured either entry before: no time is a bar.

--parent-lib FILE: a libsplpak_hip.so built from the parent commit.  splpak_fit_many_dev_f64 is then timed through BOTH
libraries in the same process, alternating, through the same ctypes call: its kernel is meant to be unchanged, so the two must
agree within the run-to-run spread DESIGN 4g documents (-3 % .. +2 %); the coefficients must be the same bits.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_many_cov_bench.py [--reps 5] [--warmup 2] [--legs 100,10000,2d] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes as C
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
from tools.fit_many_bench import largest_square

DP, IP, LP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def alternate(fa, fb, warmup, reps, stream):
    """-> (median3 of fa, median3 of fb): warm-up calls of each, then the timed calls a, b, a, b, .."""
    ta, tb = [], []
    for k in range(warmup + reps):
        for fn, t in ((fa, ta), (fb, tb)):
            stream.synchronize()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            if k >= warmup:
                t.append(time.perf_counter() - t0)
    return median3(ta), median3(tb)


def raw_fit_many(lib, nd, offsets, x, y, lo, hi, nodes, xtrap, coef, st):
    """splpak_fit_many_dev_f64 of `lib` through plain ctypes (the same call for the parent's library and this one)."""
    fn = lib.splpak_fit_many_dev_f64
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, LP, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, DP, DP, IP, C.c_double, C.c_void_p, C.c_int64, IP,
                   DP, C.c_void_p]
    nbatch = offsets.size - 1
    lo_a, hi_a, nod = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64), np.array(nodes, dtype=np.int32)
    status = np.zeros(nbatch, dtype=np.int32)
    ncol = int(np.prod(nodes))

    def call():
        rc = fn(nd, nbatch, offsets.ctypes.data_as(LP), x.data_ptr(), nd, y.data_ptr(), None, lo_a.ctypes.data_as(DP), hi_a.ctypes.data_as(DP),
                nod.ctypes.data_as(IP), xtrap, coef.data_ptr(), ncol, status.ctypes.data_as(IP), None, C.c_void_p(st))
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="100,10000,2d")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_many_cov_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_many_cov_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    new_lib = capi.lib()
    parent = C.CDLL(a.parent_lib) if a.parent_lib else None
    results = []
    for leg in a.legs.split(","):
        if leg == "2d":
            nd, nodes, npp, nbatch = 2, largest_square(), 2000, 1000
        else:
            nd, nodes, npp, nbatch = 1, [16], 1000, int(leg)
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol = int(np.prod(nodes))
        ln = capi.fit_many_cov_len(nd, nodes)
        gen = torch.Generator(device=dev)
        gen.manual_seed(31)
        x = torch.rand((nbatch * npp, nd), dtype=torch.float64, device=dev, generator=gen)
        y = (torch.sin(3.0 * x[:, 0]) + 0.5 * torch.cos(2.0 * x[:, -1])
             + 0.05 * torch.randn(nbatch * npp, dtype=torch.float64, device=dev, generator=gen)).contiguous()
        offsets = np.arange(nbatch + 1, dtype=np.int64) * npp
        coef = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
        coef_c = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
        cov = torch.zeros((nbatch, ln), dtype=torch.float64, device=dev)
        out = torch.zeros(nbatch * npp, dtype=torch.float64, device=dev)
        var = torch.zeros(nbatch * npp, dtype=torch.float64, device=dev)
        info = {}

        def fit():
            rc, status, info["fit"] = capi.fit_many_dev(nd, offsets, x, y, None, lo, hi, nodes, coef, xtrap=1.0, stream=st)
            assert rc == 0 and not status.any(), rc

        def fit_cov():
            rc, status, info["cov"] = capi.fit_many_cov_dev(nd, offsets, x, y, None, lo, hi, nodes, coef_c, cov, xtrap=1.0, stream=st)
            assert rc == 0 and not status.any(), rc

        def evaluate():
            assert capi.evaluate_many_dev(nd, offsets, x, None, coef, lo, hi, nodes, out, stream=st) == 0

        def variance():
            assert capi.evaluate_many_var_dev(nd, offsets, x, None, cov, lo, hi, nodes, var, stream=st) == 0

        t_fit, t_cov = alternate(fit, fit_cov, a.warmup, a.reps, stream)
        stats = capi.debug_fit_many_stats()
        t_eval, t_var = alternate(evaluate, variance, a.warmup, a.reps, stream)
        r = {"leg": leg, "ndim": nd, "nodes": nodes, "points_per_problem": npp, "nbatch": nbatch, "cov_words_per_problem": ln,
             "fit_many": t_fit, "fit_many_cov": t_cov, "cov_over_fit": t_cov["ms"] / t_fit["ms"],
             "fit_many_device_ms": 1e3 * float(info["fit"][0, 7]) * nbatch, "fit_many_cov_device_ms": 1e3 * float(info["cov"][0, 7]) * nbatch,
             "same_coef_bits": bool(torch.equal(coef, coef_c)), "workgroups": stats[0], "lds_bytes": stats[1],
             "eval_many": t_eval, "eval_many_var": t_var, "var_over_eval": t_var["ms"] / t_eval["ms"],
             "variance_min": float(var.min()), "variance_max": float(var.max())}
        if parent is not None:
            cp = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
            cn = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
            t_parent, t_new = alternate(raw_fit_many(parent, nd, offsets, x, y, lo, hi, nodes, 1.0, cp, st),
                                        raw_fit_many(new_lib, nd, offsets, x, y, lo, hi, nodes, 1.0, cn, st), a.warmup, a.reps, stream)
            r.update({"parent_fit_many": t_parent, "new_fit_many": t_new, "new_over_parent": t_new["ms"] / t_parent["ms"],
                      "parent_same_coef_bits": bool(torch.equal(cp, cn))})
            del cp, cn
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del x, y, coef, coef_c, cov, out, var
        capi.shutdown()
        if parent is not None:
            parent.splpak_shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "reps": a.reps, "warmup": a.warmup, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
