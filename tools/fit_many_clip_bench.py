#!/usr/bin/env python3
"""Sigma-clipped batch fits in one launch (splpak_fit_many_clip_dev_f64) beside what callers do today: the loop of
splpak_fit_many_dev + splpak_residuals_many_dev + a torch weight update over the WHOLE batch until no problem rejects a point.

Legs: 1-D, 16 nodes, 10^3 points per problem, xtrap = 1, at nbatch = 10^2, 10^4 and 10^5, and a 2-D leg at the largest
near-square grid the LDS rule admits with 2 000 points per problem at nbatch = 10^4 and xtrap = 0 (at 14 points per node the
0.75 rule calls a hundred nodes data-sparse, their constraint rows bias the fit, and ANY clipping loop then erodes the data pass
after pass: a property of the rule, not of the route, and no workload anyone times).  Uniform points, a smooth field plus
UNIFORM noise (nothing of it lies beyond 1.74 rms, so the noise itself is never clipped) and 1 % outliers of both signs without
noise, klo = khi = 3, at most 8 passes on both routes.  Four problems in five have all their outliers at 20 times the noise's
half width: one pass rejects them, the next rejects nothing (2 residual passes).  Every fifth problem has them in tiers that
only show once the larger ones have gone: it takes 3 or 4 passes (the histogram of clip[0] is in the output).  Per leg: `--warmup` untimed calls, then `--reps` calls timed
one by one with the host clock (every call ends with the stream synchronised), median with min and max, both routes in the same
process; the ratio; whether the two routes returned the same bits.  The leg named by --plain also times splpak_fit_many_dev
beside the fused entry at maxpass = 0.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_many_clip_bench.py [--reps 5] [--warmup 2] [--legs 100,10000,100000,2d] [--plain 10000] [--out FILE]
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
from tools.fit_many_bench import largest_square

KLO, KHI, MAXPASS, NOISE = 3.0, 3.0, 8, 0.05


def batch(nd, nbatch, npp, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(37)
    x = torch.rand((nbatch * npp, nd), dtype=torch.float64, device=dev, generator=gen)
    y = torch.sin(3.0 * x[:, 0]) + 0.5 * torch.cos(2.0 * x[:, -1])
    nout = npp // 100
    noise = NOISE * (2.0 * torch.rand((nbatch, npp), dtype=torch.float64, device=dev, generator=gen) - 1.0)
    noise[:, :nout] = 0.0      # (an outlier is its amplitude alone: noise on it would blur the tiers)
    y = y + noise.reshape(-1)
    # the outliers sit on the first points of a problem (the points are in random order anyway)
    amp = torch.zeros((nbatch, nout), dtype=torch.float64, device=dev)
    sign = torch.where(torch.arange(nout, device=dev) % 2 == 0, 1.0, -1.0).to(torch.float64)
    amp[:] = 20.0 * NOISE * sign
    k = torch.arange(nbatch, device=dev)
    third, fourth = (k % 5 == 4), (k % 10 == 9)
    tier2 = torch.zeros(nout, dtype=torch.bool, device=dev)
    tier2[int(0.4 * nout):int(0.7 * nout)] = True
    tier3 = torch.zeros(nout, dtype=torch.bool, device=dev)
    tier3[int(0.7 * nout):] = True
    big = 2.0 * sign
    amp[third] = torch.where(tier2 | tier3, 0.3 * sign, big)
    amp[fourth] = torch.where(tier3, 0.095 * sign, torch.where(tier2, 0.3 * sign, big))
    y = y.reshape(nbatch, npp)
    y[:, :nout] += amp
    return x, y.reshape(-1).contiguous()


def timed(fn, warmup, reps, stream):
    t, out = [], None
    for k in range(warmup + reps):
        stream.synchronize()
        t0 = time.perf_counter()
        out = fn()
        stream.synchronize()
        if k >= warmup:
            t.append(time.perf_counter() - t0)
    return median3(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="100,10000,100000,2d")
    ap.add_argument("--plain", default="10000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_many_clip_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    klo2, khi2 = KLO * KLO, KHI * KHI
    results = []
    for leg in a.legs.split(","):
        if leg == "2d":
            nd, nodes, npp, nbatch, xtrap = 2, largest_square(), 2000, 10000, 0.0
        else:
            nd, nodes, npp, nbatch, xtrap = 1, [16], 1000, int(leg), 1.0
        lo, hi = [0.0] * nd, [1.0] * nd
        ncol = int(np.prod(nodes))
        x, y = batch(nd, nbatch, npp, dev)
        offsets = np.arange(nbatch + 1, dtype=np.int64) * npp
        coef = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
        wout = torch.zeros(nbatch * npp, dtype=torch.float64, device=dev)

        def fused(maxpass=MAXPASS):
            rc, status, info, clip = capi.fit_many_clip_dev(nd, offsets, x, y, None, lo, hi, nodes, coef, wout, xtrap, KLO, KHI, maxpass, stream=st)
            assert rc == 0 and not status.any(), rc
            return info, clip

        coef_l = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)
        w_l = torch.ones(nbatch * npp, dtype=torch.float64, device=dev)
        resid = torch.zeros(nbatch * npp, dtype=torch.float64, device=dev)
        stats = torch.zeros((nbatch, 4), dtype=torch.float64, device=dev)

        def loop():
            w_l.fill_(1.0)
            fits = 0
            while True:
                rc, status, _ = capi.fit_many_dev(nd, offsets, x, y, w_l, lo, hi, nodes, coef_l, xtrap=xtrap, stream=st)
                assert rc == 0 and not status.any(), rc
                fits += 1
                if fits == MAXPASS + 1:
                    return fits
                assert capi.residuals_many_dev(nd, offsets, x, y, w_l, coef_l, lo, hi, nodes, resid, stats, stream=st) == 0
                v = (stats[:, 1] / stats[:, 0]).reshape(-1, 1)
                t = (w_l * resid).reshape(nbatch, npp)
                tt = t * t
                rej = (((t > 0) & (tt > khi2 * v)) | ((t < 0) & (tt > klo2 * v))).reshape(-1)
                if int(rej.sum().item()) == 0:
                    return fits
                w_l[rej] = 0.0

        t_fused, (info, clip) = timed(fused, a.warmup, a.reps, stream)
        fstats = capi.debug_fit_many_stats()
        t_loop, fits_loop = timed(loop, a.warmup, a.reps, stream)
        same = bool(torch.equal(coef, coef_l)) and bool(torch.equal(wout, w_l))
        hist = np.bincount(clip[:, 0].astype(np.int64), minlength=MAXPASS + 1).tolist()
        r = {"leg": leg, "ndim": nd, "nodes": nodes, "points_per_problem": npp, "nbatch": nbatch, "xtrap": xtrap, "klo": KLO, "khi": KHI, "maxpass": MAXPASS,
             "fused": t_fused, "fused_device_ms": 1e3 * float(info[0, 7]) * nbatch, "loop": t_loop, "loop_fits_of_the_whole_batch": fits_loop,
             "loop_over_fused": t_loop["ms"] / t_fused["ms"], "same_bits": same, "residual_passes_histogram": hist,
             "rejected_per_problem_mean": float(clip[:, 1].mean()), "residual_passes_total_fused": int(clip[:, 0].sum()),
             "residual_passes_total_loop": min(fits_loop, MAXPASS) * nbatch, "workgroups": fstats[0], "lds_bytes": fstats[1], "max_fits": fstats[7]}
        if leg == a.plain:
            cp = torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev)

            def plain():
                rc, status, _ = capi.fit_many_dev(nd, offsets, x, y, None, lo, hi, nodes, cp, xtrap=xtrap, stream=st)
                assert rc == 0
            r["fit_many"], _ = timed(plain, a.warmup, a.reps, stream)
            r["fused_maxpass0"], _ = timed(lambda: fused(0), a.warmup, a.reps, stream)
            r["maxpass0_same_bits_as_fit_many"] = bool(torch.equal(cp, coef))
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del x, y, coef, wout, coef_l, w_l, resid, stats
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "reps": a.reps, "warmup": a.warmup, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
