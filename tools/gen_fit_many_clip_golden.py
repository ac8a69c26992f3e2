#!/usr/bin/env python3
"""Writes tests/golden/fit_many_clip_ref.npz: the clipping loop of splpak_fit_many_clip_* (include/splpak_hip.h) run on the
unmodified reference (oracle/_ref) for every recorded case of tests/test_fit_many_clip.py -- Reference.fit on the listed points of
non-zero weight, Reference.evaluate at them, the rule in numpy, again -- and per case its inputs (x, y, w), the final mask, the
number of residual passes, the number of rejected points and the coefficients of the last fit.  CPU only.

A case is refused (nothing is written) when
  * a fit of any pass fails one of the guards of tools/gen_fit_many_golden.py on the weights of that pass: the reference is
    more than 1e-11 from its C restatement, more than 5e-11 from the least-squares solution of its own rows
    (reference_error), or a node's histogram lies within 1e-9 of its 0.75 threshold (threshold_margin);
  * a decision of any pass lies within 1e-6 relative of its threshold: the library sums S in its own fixed order and rounds the
    coefficients it evaluates, so it could decide such a point differently.

    python tools/gen_fit_many_clip_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.binding import Port, Reference, port_available, ref_available  # noqa: E402
from tests.test_fit_many import listed, ref_nwrk  # noqa: E402
from tests.test_fit_many_clip import GOLDEN_NAMES, KHI, KLO, MAXPASS, case, decide, start_weights  # noqa: E402
from tools.gen_fit_many_golden import fit_both, reference_error, threshold_margin  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fit_many_clip_ref.npz")


def reference_loop(ref, port, name, p):
    """-> (coef, wout, passes, rejected) of the loop on the reference, every fit guarded."""
    nd, nodes = p["ndim"], list(p["nodes"])
    lo, hi = [0.0] * nd, [1.0] * nd
    w = start_weights(p)
    passes = rejected = 0
    for j in range(MAXPASS + 1):
        q = dict(p)
        q["w"] = w
        c, ierr, cp, ierr_p = fit_both(ref, port, q)
        if ierr != 0 or ierr_p != 0:
            sys.exit(f"gen_fit_many_clip_golden: {name}, pass {j}: the reference returns {ierr}, its restatement {ierr_p}")
        diff = np.max(np.abs(c - cp)) / np.max(np.abs(c))
        # (weights of 0 and 1 alone: the unit bumps add up exactly in any order, and both sides compare the same numbers)
        margin = np.inf if np.all((w == 0.0) | (w == 1.0)) else threshold_margin(q)
        own = reference_error(q, c)
        print(f"{name}, fit {j}: {np.count_nonzero(w)} points, reference vs its C restatement {diff:.2e}, vs the solution of its rows "
              f"{'not checked' if own is None else format(own, '.2e')}, nearest 0.75 threshold {margin:.2e}", flush=True)
        if own is not None and own > 5e-11:
            sys.exit(f"gen_fit_many_clip_golden: the reference is {own:.2e} from the solution of its own rows on {name}, fit {j}")
        if diff > 1e-11:
            sys.exit(f"gen_fit_many_clip_golden: {name}, fit {j} is too ill-conditioned to be a yardstick")
        if margin < 1e-9:
            sys.exit(f"gen_fit_many_clip_golden: {name}, fit {j} has a node on its 0.75 threshold")
        if j == MAXPASS:
            break
        x, y, wl = listed(q)
        f, ierr = ref.evaluate(nd, x, None, c, lo, hi, nodes)
        if ierr != 0:
            sys.exit(f"gen_fit_many_clip_golden: {name}: the reference's evaluation returns {ierr}")
        t = wl * (y - np.asarray(f, dtype=np.float64))
        v = float(t @ t) / t.size
        passes += 1
        try:
            rej = decide(t, v, KLO, KHI, margin=1e-6, what=f"{name}, pass {j}")
        except AssertionError as e:
            sys.exit(f"gen_fit_many_clip_golden: {e}")
        print(f"{name}, pass {j}: v = {v:.6e}, {int(rej.sum())} rejected", flush=True)
        if not rej.any():
            break
        idx = np.nonzero(w != 0.0)[0]
        w[idx[rej]] = 0.0
        rejected += int(rej.sum())
    return c, w, passes, rejected


if __name__ == "__main__":
    if not ref_available() or not port_available():
        sys.exit("gen_fit_many_clip_golden: oracle/_ref or the C restatement is not built (make -C oracle ref port)")
    ref, port = Reference(), Port()
    out = {}
    for name in GOLDEN_NAMES:
        p = case(name)
        c, w, passes, rejected = reference_loop(ref, port, name, p)
        out["x_" + name], out["y_" + name] = p["x"], p["y"]
        out["w_" + name] = p["w"] if p["w"] is not None else np.zeros(0)
        out["mask_" + name] = w == 0.0
        out["passes_" + name] = np.int32(passes)
        out["rejected_" + name] = np.int32(rejected)
        out["coef_" + name] = c
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
