#!/usr/bin/env python3
"""Fit against refit at BASELINE config 3 (3-D, 64^3 nodes, 1e7 weighted points of the seeded stream, xtrap = 1) through ONE plan
on one MI355X: after a warm-up fit and refit, `--fits` fits and `--refits` refits of fresh values each, timed with a host clock
around calls that end in a stream synchronise (both entries synchronise before they return).  Medians, the spread and the ratio;
then, in a pass of its own with the plan's event timing on, the stages of one refit (splpak_plan_stage_timing).  Then `--nfields`
fresh fields cos((3 + k) sum x) three ways, median of 5 each: one call with refit_batch = 8 (shared sweeps of the factor), one call
with refit_batch = 1 (field by field: the yardstick), and that many single-field calls; the stages of a batched call.  One JSON line.

    python tools/refit_bench.py [--nodes 64] [--ndata 10000000] [--fits 3] [--refits 5] [--nfields 8]

A measurement, not a test: nothing here asserts a time.  The refits are checked against the fit of the same values (2e-10).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--ndata", type=int, default=10_000_000)
    ap.add_argument("--fits", type=int, default=3)
    ap.add_argument("--refits", type=int, default=5)
    ap.add_argument("--nfields", type=int, default=8)
    a = ap.parse_args()
    import torch
    from splpak_amd import capi
    if not torch.cuda.is_available():
        sys.exit("refit_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    nd, m = 3, a.ndata
    nodes, lo, hi = [a.nodes] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    y = torch.empty(m, dtype=torch.float64, device=dev)
    w = torch.empty(m, dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, y, w, st)
    sx = x.sum(dim=1)
    fields = [torch.cos((2.0 + k) * sx) + 0.25 * y for k in range(a.refits + 1)]      # fresh values for every refit
    del sx
    ncol = a.nodes ** nd
    coef = torch.zeros(ncol, dtype=torch.float64, device=dev)
    plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, info = call()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), rc, info

    # warm-up: every shape and path the timed window uses
    _, rc, _ = timed(lambda: plan.fit(x, fields[0], w, coef, st))
    assert rc == 0
    c_fit0 = coef.clone()
    _, rc, _ = timed(lambda: plan.refit(fields[1], coef, st))
    assert rc == 0
    fit_ms, refit_ms, steps = [], [], []
    for _ in range(a.fits):
        ms, rc, info = timed(lambda: plan.fit(x, y, w, coef, st))
        assert rc == 0
        fit_ms.append(ms)
    fit_steps = int(info[2])
    for k in range(a.refits):
        ms, rc, info = timed(lambda: plan.refit(fields[1 + k], coef, st))
        assert rc == 0 and info[6] == 0.0
        refit_ms.append(ms)
        steps.append(int(info[2]))
    # same values, same answer: the warm-up fit's field again
    _, rc, _ = timed(lambda: plan.refit(fields[0], coef, st))
    err = float((coef - c_fit0).abs().max() / c_fit0.abs().max())
    assert rc == 0 and err < 2e-10, err
    # the stages of one refit, with the event timing on (not part of the timed window)
    plan.enable_kernel_timing(True)
    ms_ev, rc, _ = timed(lambda: plan.refit(fields[1], coef, st))
    stages = plan.stage_timing()
    out = dict(config="3-D %d^3 nodes, %d weighted points" % (a.nodes, m), device=capi.device_name(),
               factorisation=plan.factorisation()[0],
               fit_ms_median=float(np.median(fit_ms)), fit_ms=[round(v, 3) for v in fit_ms], fit_refine_steps=fit_steps,
               refit_ms_median=float(np.median(refit_ms)), refit_ms=[round(v, 3) for v in refit_ms], refit_refine_steps=steps,
               ratio=float(np.median(fit_ms) / np.median(refit_ms)),
               refit_vs_fit_same_values=err,
               refit_stages_ms=dict(gather_and_rhs=float(stages["gram_ms"]), residual_pass=float(stages["residual_pass_ms"]),
                                    one_solve=float(stages["solve_ms"]), whole_call_with_events=ms_ev))
    plan.enable_kernel_timing(False)
    # ---- several fields in one call: batched sweeps against field by field
    nf = a.nfields
    if nf >= 1:
        sx = x.sum(dim=1)
        Y = torch.stack([torch.cos((3.0 + k) * sx) for k in range(nf)])
        del sx
        C = torch.zeros((nf, ncol), dtype=torch.float64, device=dev)

        def calls(batch):
            plan.set_option("refit_batch", str(batch))
            return timed(lambda: plan.refit(Y, C, st))

        def singles():
            info = np.zeros((nf, 10))
            rc = 0
            for k in range(nf):
                r, i = plan.refit(Y[k], C[k], st)
                rc, info[k] = rc or r, i
            return rc, info

        res = {}
        for label, run in (("batched", lambda: calls(8)), ("field_by_field", lambda: calls(1)), ("single_calls", lambda: timed(singles))):
            run()                                           # warm-up (the first batched call allocates the per-field copies)
            ms_all = []
            for _ in range(5):
                ms, rc, info = run()
                assert rc == 0
                ms_all.append(ms)
            res[label] = dict(ms_median=float(np.median(ms_all)), ms=[round(v, 3) for v in ms_all], steps=[int(v) for v in info[:, 2]],
                              stats=plan.refit_stats(), coef=C.clone())
        same = bool(torch.equal(res["batched"]["coef"], res["field_by_field"]["coef"]) and torch.equal(res["batched"]["coef"], res["single_calls"]["coef"]))
        assert same, "the batched refit does not give the bits of the field-by-field refit"
        for r in res.values():
            del r["coef"]
        plan.enable_kernel_timing(True)
        ms_ev, rc, _ = calls(8)
        stages = plan.stage_timing()
        plan.set_option("refit_batch", None)
        out["fields"] = dict(nfields=nf, **res, equal_bits=same,
                             ratio_field_by_field_over_batched=res["field_by_field"]["ms_median"] / res["batched"]["ms_median"],
                             batched_stages_ms=dict(last_gather_and_rhs=float(stages["gram_ms"]), residual_pass=float(stages["residual_pass_ms"]),
                                                    first_sweep=float(stages["solve_ms"]), whole_call_with_events=ms_ev))
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
