#!/usr/bin/env python3
"""Writes tests/golden/fit_grid_ref.npz: the coefficients the unmodified reference (oracle/_ref, Reference.fit) returns for the
listed Cartesian products of the parity cases of tests/test_fit_grid.py -- the four xtrap = 0 shapes with separable weights and
the xtrap = 1 sample that stays within the data-sparse rule.  CPU only, a few seconds.

Beside every case it prints how far a plain numpy restatement of the grid fit (per-axis normal equations on the library's
general-form window values, no refinement) is from the reference: the algebra the entry rests on, checked without a GPU.

    python tools/gen_fit_grid_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.binding import Reference, ref_available  # noqa: E402
from tests.test_fit_grid import HI, LO, PARITY_SHAPES, apply_axes, axis_matrix, listed_points, parity_case, xtrap_case  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fit_grid_ref.npz")


def numpy_grid_fit(ndim, axes, waxes, values, nodes):
    P = []
    for d in range(ndim):
        A = axis_matrix(d, nodes[d], axes[d])[0]
        w2 = np.ones(axes[d].size) if waxes is None else waxes[d] ** 2
        N = (A.T * w2) @ A
        print(f"    axis {d + 1}: cond(N) = {np.linalg.cond(N):.1e}")
        P.append(np.linalg.solve(N, A.T * w2))
    return apply_axes(P, values).ravel()


if __name__ == "__main__":
    if not ref_available():
        sys.exit("gen_fit_grid_golden: oracle/_ref is not built (make -C oracle ref)")
    ref = Reference()
    out = {}
    for name in list(PARITY_SHAPES) + ["xtrap1"]:
        xtrap = 1.0 if name == "xtrap1" else 0.0
        ndim, axes, waxes, values, nodes = xtrap_case() if name == "xtrap1" else parity_case(name)
        x, w = listed_points(axes, waxes)
        c, ierr, _ = ref.fit(ndim, x, values.ravel(), w, LO[:ndim], HI[:ndim], nodes, xtrap)
        ncol = int(np.prod(nodes))
        out["coef_" + name] = np.asarray(c[:ncol], dtype=np.float64)
        out["ierror_" + name] = np.int32(ierr)
        print(f"{name}: ierror {ierr}, {x.shape[0]} points, {ncol} coefficients")
        c_np = numpy_grid_fit(ndim, axes, waxes, values, nodes)
        print(f"    numpy grid fit vs reference: {np.max(np.abs(c_np - c[:ncol])) / np.max(np.abs(c[:ncol])):.2e}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)
