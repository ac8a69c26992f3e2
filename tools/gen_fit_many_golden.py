#!/usr/bin/env python3
"""Writes tests/golden/fit_many_ref.npz: the coefficients and ierror the unmodified reference (oracle/_ref, Reference.fit)
returns for every parity problem of tests/test_fit_many.py, one call per problem on its listed points of non-zero weight, and
its ierror for the two problems the tests expect 107 from.  CPU only; the 17-fold problem of the largest 1-D grid takes the
reference's dense solver a few minutes.

A case is refused (nothing is written) when
  * the C restatement of the reference (Port) differs from the reference by more than 1e-11: too ill-conditioned to be a
    yardstick at 1e-10;
  * the reference itself is more than 5e-11 -- half the bar, which the yardstick's error and the library's share -- from the
    least-squares solution of its own rows, refined in extended precision (numpy.longdouble) until the corrections vanish.  The
    restatement repeats the reference operation by operation and agrees with it to the bit, so the first check cannot see
    this: the reference's row-by-row Householder steps lose eps times the ratio of the largest row to the smallest when the
    heavy rows come last, and its constraint rows do (1e6 on the largest 1-D grid with points placed at random in the cells:
    5.7e-10 from the solution).  Checked where the dense rows fit in memory (rows x ncol <= 4e6);
  * a node's histogram value lies within 1e-9 relative of its 0.75 threshold: the library adds the histogram and its total in
    its own fixed order and could decide such a node differently from the reference's running sums.  (Weighted problems only:
    the unit bumps of an unweighted one add up exactly in any order, and both sides then compare the same numbers.)

    python tools/gen_fit_many_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.binding import Port, Reference, port_available, ref_available  # noqa: E402
from tests.test_fit_many import NumpyManyFit, PARITY_NAMES, SINGULAR, listed, lo_hi, problem, ref_nwrk  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fit_many_ref.npz")


def threshold_margin(p):
    """min over the nodes of |hist - 0.75 expect| / (0.75 expect), by the reference's rule (:879-936); inf at xtrap = 0 and
    for unit weights."""
    x, _, w = listed(p)
    if p["xtrap"] == 0.0 or w is None or w[0] < 0.0:
        return np.inf
    nodes = list(p["nodes"])
    D = len(nodes)
    lo, hi = lo_hi(p)
    hist = np.zeros(int(np.prod(nodes)))
    for i in range(x.shape[0]):
        addr = 0
        for r in reversed(range(D)):
            t = int((1.0 / ((hi[r] - lo[r]) / (nodes[r] - 1))) * (x[i, r] - lo[r]) + 0.5)
            if 0 <= t <= nodes[r] - 1:
                addr = nodes[r] * addr + t
        hist[addr] += w[i]
    wtprrc = w.sum() / np.prod([n - 1 for n in nodes])
    worst = np.inf
    for node in range(hist.size):
        expect, rest = wtprrc, node
        for r in range(D):
            if rest % nodes[r] in (0, nodes[r] - 1):
                expect *= 0.5
            rest //= nodes[r]
        if expect > 0.0:
            worst = min(worst, abs(hist[node] - 0.75 * expect) / (0.75 * expect))
    return worst


def reference_error(p, c):
    """Relative max-norm distance of the reference's coefficients c from the least-squares solution of its rows; None where
    the dense rows would not fit."""
    f = NumpyManyFit(p)
    m, n = f.y.size, f.ncol
    if (m + f.C.shape[0]) * n > 4e6:
        return None
    A = np.zeros((m, n))
    np.add.at(A, (np.repeat(np.arange(m), f.cols.shape[1]), f.cols.ravel()), f.vals.ravel())
    M = np.vstack([A, f.C])
    b = np.concatenate([f.b, np.zeros(f.C.shape[0])])
    Ml, bl = M.astype(np.longdouble), b.astype(np.longdouble)
    N = M.T @ M
    x = np.linalg.solve(N, M.T @ b).astype(np.longdouble)
    for _ in range(12):
        dx = np.linalg.solve(N, (Ml.T @ (bl - Ml @ x)).astype(np.float64)).astype(np.longdouble)
        x = x + dx
        if float(np.max(np.abs(dx))) <= 1e-17 * float(np.max(np.abs(x))):
            break
    else:
        sys.exit("gen_fit_many_golden: the extended-precision refinement did not settle")
    ref_order = np.zeros(n)
    for node in range(n):
        inn = [node % f.nod[0], node // f.nod[0]][:f.ndim]
        ref_order[sum(inn[d] * f.refstride[d] for d in range(f.ndim))] = float(x[node])
    return float(np.max(np.abs(c - ref_order)) / np.max(np.abs(ref_order)))


def fit_both(ref, port, p):
    x, y, w = listed(p)
    lo, hi = lo_hi(p)
    ncol = int(np.prod(p["nodes"]))
    c, ierr, _ = ref.fit(p["ndim"], x, y, w, lo, hi, list(p["nodes"]), p["xtrap"], nwrk=ref_nwrk(p))
    cp, ierr_p, _ = port.fit(p["ndim"], x, y, w, lo, hi, list(p["nodes"]), p["xtrap"], nwrk=ref_nwrk(p))
    return np.asarray(c[:ncol], dtype=np.float64), int(ierr), np.asarray(cp[:ncol], dtype=np.float64), int(ierr_p)


if __name__ == "__main__":
    if not ref_available() or not port_available():
        sys.exit("gen_fit_many_golden: oracle/_ref or the C restatement is not built (make -C oracle ref port)")
    ref, port = Reference(), Port()
    out = {}
    for name in PARITY_NAMES:
        p = problem(name)
        c, ierr, cp, ierr_p = fit_both(ref, port, p)
        if ierr != 0 or ierr_p != 0:
            sys.exit(f"gen_fit_many_golden: {name}: the reference returns {ierr}, its restatement {ierr_p}")
        diff = np.max(np.abs(c - cp)) / np.max(np.abs(c))
        margin = threshold_margin(p)
        own = reference_error(p, c)
        print(f"{name}: nodes {p['nodes']}, {p['y'].size} points, reference vs its C restatement {diff:.2e}, vs the solution of its "
              f"rows {'not checked' if own is None else format(own, '.2e')}, nearest 0.75 threshold {margin:.2e}", flush=True)
        if own is not None and own > 5e-11:
            sys.exit(f"gen_fit_many_golden: the reference is {own:.2e} from the solution of its own rows on {name}")
        if diff > 1e-11:
            sys.exit(f"gen_fit_many_golden: {name} is too ill-conditioned to be a yardstick")
        if margin < 1e-9:
            sys.exit(f"gen_fit_many_golden: {name} has a node on its 0.75 threshold")
        out["coef_" + name] = c
        out["ierror_" + name] = np.int32(ierr)
    singular = dict(problem(SINGULAR))
    singular["xtrap"] = 0.0
    three = dict(problem("n4_x1_xt0"))
    three["x"], three["y"] = three["x"][:3], three["y"][:3]
    for key, p in (("singular", singular), ("three", three)):
        _, ierr, _, ierr_p = fit_both(ref, port, p)
        print(f"{key}: the reference returns {ierr}, its restatement {ierr_p}")
        out["ierror_" + key] = np.int32(ierr)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)
