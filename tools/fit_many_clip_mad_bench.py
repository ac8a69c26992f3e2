#!/usr/bin/env python3
"""Robustly clipped batch fits in one launch (splpak_fit_many_clip_mad_dev_f64) beside the loop of entries it fuses and beside
the rms rule of splpak_fit_many_clip_dev_f64 on the same data: the protocol and the data of tools/fit_many_clip_bench.py.

Legs: 1-D, 16 nodes, 10^3 points per problem, xtrap = 1, at nbatch = 10^5 (and whatever --legs names), and the 2-D leg at the
largest near-square grid the LDS rule admits (12 x 12) with 2 000 points per problem at nbatch = 10^4 and xtrap = 0.  1 % outliers
of both signs, klo = khi = 3, at most 8 passes.  Measured in the same process, ALTERNATING (one call of every route per round, so
that a drift of the clocks hits all alike): `--warmup` untimed rounds, then `--reps` rounds timed call by call with the host clock
(every call ends with the stream synchronised), median with min and max:
  fused_regrow0, fused_regrow1   the fused robust entry;
  loop                           splpak_fit_many_dev -> splpak_residuals_many_dev -> t = resid -> splpak_mad_many_dev ->
                                 steps 4 and 5 of the rule in torch -> ..., over the WHOLE batch until no weight changes
                                 (regrow 0); its bits are compared with fused_regrow0;
  rms                            splpak_fit_many_clip_dev, the rms rule.
Reported beside the times: the residual passes per problem of every route (mean and histogram), and from them the cost per
pass of the robust entry over the rms entry -- the price of the selection.
Prints one JSON line; --out writes it to a file as well.

    python tools/fit_many_clip_mad_bench.py [--reps 5] [--warmup 2] [--legs 100000,2d] [--out FILE]
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
from tools.fit_many_clip_bench import KHI, KLO, MAXPASS, batch

MAD_TO_SIGMA = 1.482602218505602


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="100000,2d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_many_clip_mad_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
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
        coef = {k: torch.zeros((nbatch, ncol), dtype=torch.float64, device=dev) for k in ("g0", "g1", "loop", "rms")}
        wout = {k: torch.zeros(nbatch * npp, dtype=torch.float64, device=dev) for k in ("g0", "g1", "loop", "rms")}
        resid = torch.zeros(nbatch * npp, dtype=torch.float64, device=dev)
        stats = torch.zeros((nbatch, 4), dtype=torch.float64, device=dev)

        def fused(regrow):
            key = f"g{regrow}"
            rc, status, info, clip = capi.fit_many_clip_mad_dev(nd, offsets, x, y, None, lo, hi, nodes, coef[key], wout[key], xtrap, KLO, KHI,
                                                                MAXPASS, regrow, stream=st)
            assert rc == 0 and not status.any(), rc
            return info, clip

        def rms():
            rc, status, info, clip = capi.fit_many_clip_dev(nd, offsets, x, y, None, lo, hi, nodes, coef["rms"], wout["rms"], xtrap, KLO, KHI,
                                                            MAXPASS, stream=st)
            assert rc == 0 and not status.any(), rc
            return info, clip

        def loop():
            w = wout["loop"]
            w.fill_(1.0)
            fits = 0
            while True:
                rc, status, _ = capi.fit_many_dev(nd, offsets, x, y, w, lo, hi, nodes, coef["loop"], xtrap=xtrap, stream=st)
                assert rc == 0 and not status.any(), rc
                fits += 1
                if fits == MAXPASS + 1:
                    return fits
                assert capi.residuals_many_dev(nd, offsets, x, y, None, coef["loop"], lo, hi, nodes, resid, None, stream=st) == 0
                assert capi.mad_many_dev(offsets, resid, w, stats, stream=st) == 0      # (w0 = 1: t = resid)
                med, s = stats[:, 1].reshape(-1, 1), (MAD_TO_SIGMA * stats[:, 2]).reshape(-1, 1)
                e = resid.reshape(nbatch, npp) - med
                out = ((e > KHI * s) | (-e > KLO * s)) & (s != 0.0) & (w.reshape(nbatch, npp) != 0.0)
                if int(out.sum().item()) == 0:
                    return fits
                w[out.reshape(-1)] = 0.0

        routes = [("fused_regrow0", lambda: fused(0)), ("fused_regrow1", lambda: fused(1)), ("loop", loop), ("rms", rms)]
        times = {name: [] for name, _ in routes}
        last = {}
        for k in range(a.warmup + a.reps):
            for name, fn in routes:
                stream.synchronize()
                t0 = time.perf_counter()
                last[name] = fn()
                stream.synchronize()
                if k >= a.warmup:
                    times[name].append(time.perf_counter() - t0)
        r = {"leg": leg, "ndim": nd, "nodes": nodes, "points_per_problem": npp, "nbatch": nbatch, "xtrap": xtrap, "klo": KLO, "khi": KHI,
             "maxpass": MAXPASS}
        for name, _ in routes:
            r[name] = median3(times[name])
        r["loop_fits_of_the_whole_batch"] = last["loop"]
        r["loop_same_bits_as_fused_regrow0"] = bool(torch.equal(coef["g0"], coef["loop"])) and bool(torch.equal(wout["g0"], wout["loop"]))
        fits = {}
        for name in ("fused_regrow0", "fused_regrow1", "rms"):
            info, clip = last[name]
            passes = clip[:, 0]
            stopped_by_change = passes < MAXPASS      # a problem that stops by a pass without change ran as many fits as passes
            fits[name] = float(np.where(stopped_by_change, passes, passes + 1).mean())
            r[name + "_passes_mean"] = float(passes.mean())
            r[name + "_passes_histogram"] = np.bincount(passes.astype(np.int64), minlength=MAXPASS + 1).tolist()
            r[name + "_out_per_problem_mean"] = float(clip[:, 1].mean())
            r[name + "_device_ms"] = 1e3 * float(info[0, 7]) * nbatch
        r["returned_per_problem_mean_regrow1"] = float(last["fused_regrow1"][1][:, 5].mean())
        r["loop_over_fused_regrow0"] = r["loop"]["ms"] / r["fused_regrow0"]["ms"]
        r["fused_regrow0_over_rms"] = r["fused_regrow0"]["ms"] / r["rms"]["ms"]
        # per pass (a fit and, but for the last, a residual pass): the price of the selection
        r["ms_per_pass_fused_regrow0"] = r["fused_regrow0"]["ms"] / fits["fused_regrow0"]
        r["ms_per_pass_fused_regrow1"] = r["fused_regrow1"]["ms"] / fits["fused_regrow1"]
        r["ms_per_pass_rms"] = r["rms"]["ms"] / fits["rms"]
        r["per_pass_fused_regrow0_over_rms"] = r["ms_per_pass_fused_regrow0"] / r["ms_per_pass_rms"]
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del x, y, coef, wout, resid, stats
        capi.shutdown()
        torch.cuda.empty_cache()
    line = json.dumps({"device": capi.device_name(), "reps": a.reps, "warmup": a.warmup, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
