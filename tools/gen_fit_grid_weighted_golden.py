#!/usr/bin/env python3
"""Writes tests/golden/fit_grid_weighted_ref.npz: the coefficients and ierror the unmodified reference (oracle/_ref,
Reference.fit) returns for the listed samples of non-zero weight of the parity cases of tests/test_fit_grid_weighted.py -- the
four xtrap = 0 shapes with "separable x 15 % dead x U[0.5, 2]" weights and the xtrap = 1 sample with weights U[0.9, 1.1].  CPU
only, a few seconds.

Beside every case it prints how far the numpy restatement of the algorithm (NumpyWeightedFit of the test file) is from the
reference, its conjugate-gradient iterations per solve and cond(N); for the xtrap = 1 case it confirms that the reference adds
no constraint rows, by fitting the same samples with xtrap = 0: with no data-sparse node the two fits have the same rows.

    python tools/gen_fit_grid_weighted_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.binding import Reference, ref_available  # noqa: E402
from tests.test_fit_grid import HI, LO, apply_axes  # noqa: E402
from tests.test_fit_grid_weighted import NumpyWeightedFit, W_PARITY_SHAPES, listed_nonzero, weighted_case  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fit_grid_weighted_ref.npz")


def cond_of_N(f):
    """cond(N) of N = A^T diag(w^2) A, assembled column by column through the operator (a few hundred columns at these sizes)."""
    n = int(np.prod(f.shape))
    N = np.empty((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        N[:, j] = f.op(e.reshape(f.shape)).ravel()
    return np.linalg.cond(N)


if __name__ == "__main__":
    if not ref_available():
        sys.exit("gen_fit_grid_weighted_golden: oracle/_ref is not built (make -C oracle ref)")
    ref = Reference()
    out = {}
    for name in list(W_PARITY_SHAPES) + ["xtrap1"]:
        ndim, axes, w, values, nodes, xtrap = weighted_case(name)
        x, y, wl = listed_nonzero(axes, w, values)
        c, ierr, _ = ref.fit(ndim, x, y, wl, LO[:ndim], HI[:ndim], nodes, xtrap)
        ncol = int(np.prod(nodes))
        c = np.asarray(c[:ncol], dtype=np.float64)
        out["coef_" + name] = c
        out["ierror_" + name] = np.int32(ierr)
        print(f"{name}: ierror {ierr}, {x.shape[0]} of {w.size} samples listed, {ncol} coefficients")
        if xtrap != 0.0:
            c0, ierr0, _ = ref.fit(ndim, x, y, wl, LO[:ndim], HI[:ndim], nodes, 0.0)
            same = np.max(np.abs(c - c0[:ncol])) / np.max(np.abs(c))
            print(f"    the reference with xtrap = 0 on the same samples: ierror {ierr0}, difference {same:.2e}")
            if ierr0 != 0 or same > 1e-12:
                sys.exit("gen_fit_grid_weighted_golden: the reference adds constraint rows to the xtrap = 1 case: narrow its weights")
        f = NumpyWeightedFit(ndim, axes, w, nodes)
        c_np = f.fit(values)
        print(f"    numpy restatement vs reference: {np.max(np.abs(c_np - c)) / np.max(np.abs(c)):.2e}, CG iterations per solve "
              f"{f.iters}, cond(N) = {cond_of_N(f):.1e}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)
