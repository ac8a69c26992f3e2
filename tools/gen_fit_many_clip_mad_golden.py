#!/usr/bin/env python3
"""Writes tests/golden/fit_many_clip_mad_ref.npz: the robust clipping rule of splpak_fit_many_clip_mad_* (include/splpak_hip.h)
run on the unmodified reference (oracle/_ref) for every recorded case of tests/test_fit_many_clip_mad.py, with regrow 0 and 1 --
Reference.fit on the listed points of non-zero weight, Reference.evaluate at every point of non-zero starting weight,
numpy.median for the centre and the MAD, the decision in numpy, again -- and per case and regrow the final mask, the number of
residual passes, the number of returned points and the coefficients of the last fit.  Data only.  CPU only.

A case is refused (nothing is written) when
  * a fit of any pass fails one of the guards of tools/gen_fit_many_golden.py on the weights of that pass (as
    tools/gen_fit_many_clip_golden.py);
  * a decision of any pass lies within 1e-6 relative of its threshold: the library rounds the coefficients it evaluates, so it
    could decide such a point differently;
  * it is the drag case and, with regrow = 1, fewer than 10 points return or more than 2 good points end rejected.

    python tools/gen_fit_many_clip_mad_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.binding import Port, Reference, port_available, ref_available  # noqa: E402
from tests.test_fit_many import listed  # noqa: E402
from tests.test_fit_many_clip import start_weights  # noqa: E402
from tests.test_fit_many_clip_mad import GOLDEN_NAMES, KHI, KLO, MAXPASS, apply_rule, mad_case  # noqa: E402
from tools.gen_fit_many_golden import fit_both, reference_error, threshold_margin  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fit_many_clip_mad_ref.npz")
ME = "gen_fit_many_clip_mad_golden"


def reference_loop(ref, port, name, p, regrow):
    """-> (coef, wout, passes, returned) of the rule on the reference, every fit guarded."""
    nd, nodes = p["ndim"], list(p["nodes"])
    lo, hi = [0.0] * nd, [1.0] * nd
    w0 = start_weights(p)
    w = w0.copy()
    q0 = dict(p)
    q0["w"] = w0
    x0, y0, wl0 = listed(q0)      # the points of non-zero starting weight
    passes = returned = 0
    for j in range(MAXPASS + 1):
        q = dict(p)
        q["w"] = w
        c, ierr, cp, ierr_p = fit_both(ref, port, q)
        if ierr != 0 or ierr_p != 0:
            sys.exit(f"{ME}: {name}, regrow {regrow}, pass {j}: the reference returns {ierr}, its restatement {ierr_p}")
        diff = np.max(np.abs(c - cp)) / np.max(np.abs(c))
        # (weights of 0 and 1 alone: the unit bumps add up exactly in any order, and both sides compare the same numbers)
        margin = np.inf if np.all((w == 0.0) | (w == 1.0)) else threshold_margin(q)
        own = reference_error(q, c)
        print(f"{name}, regrow {regrow}, fit {j}: {np.count_nonzero(w)} points, reference vs its C restatement {diff:.2e}, vs the solution "
              f"of its rows {'not checked' if own is None else format(own, '.2e')}, nearest 0.75 threshold {margin:.2e}", flush=True)
        if own is not None and own > 5e-11:
            sys.exit(f"{ME}: the reference is {own:.2e} from the solution of its own rows on {name}, fit {j}")
        if diff > 1e-11:
            sys.exit(f"{ME}: {name}, fit {j} is too ill-conditioned to be a yardstick")
        if margin < 1e-9:
            sys.exit(f"{ME}: {name}, fit {j} has a node on its 0.75 threshold")
        if j == MAXPASS:
            break
        f, ierr = ref.evaluate(nd, x0, None, c, lo, hi, nodes)
        if ierr != 0:
            sys.exit(f"{ME}: {name}: the reference's evaluation returns {ierr}")
        t_all = wl0 * (y0 - np.asarray(f, dtype=np.float64))
        passes += 1
        try:
            s, med, changed, back = apply_rule(t_all, w0, w, KLO, KHI, regrow, margin=1e-6, what=f"{name}, regrow {regrow}, pass {j}")
        except AssertionError as e:
            sys.exit(f"{ME}: {e}")
        returned += back
        print(f"{name}, regrow {regrow}, pass {j}: med = {med:.6e}, s = {s:.6e}, {changed} weights changed, {back} returned", flush=True)
        if s == 0.0 or changed == 0:
            break
    return c, w, passes, returned


if __name__ == "__main__":
    if not ref_available() or not port_available():
        sys.exit(f"{ME}: oracle/_ref or the C restatement is not built (make -C oracle ref port)")
    ref, port = Reference(), Port()
    out = {}
    for name in GOLDEN_NAMES:
        p = mad_case(name)
        for regrow in (0, 1):
            c, w, passes, returned = reference_loop(ref, port, name, p, regrow)
            key = f"{name}_g{regrow}"
            if name == "drag":
                good_lost = int(np.count_nonzero(w == 0.0)) - int(np.count_nonzero(w[p["raised"]] == 0.0))
                print(f"drag, regrow {regrow}: {returned} returned, {good_lost} good points end rejected", flush=True)
                if regrow and (returned < 10 or good_lost > 2):
                    sys.exit(f"{ME}: the drag case shows nothing: {returned} points return, {good_lost} good points end rejected")
            out["mask_" + key] = w == 0.0
            out["passes_" + key] = np.int32(passes)
            out["returned_" + key] = np.int32(returned)
            out["coef_" + key] = c
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
