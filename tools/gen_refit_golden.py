#!/usr/bin/env python3
"""Writes tests/golden/refit_y2.npz: the coefficients of the second field of tests/test_refit.py,
y2 = cos(3 * sum_d x_d) + 0.25 * y, for every case of that file, from the dense oracle (oracle/binding.py Port.fit --
the way tests/test_gpu_parity.py::test_fit_fresh_inputs_vs_oracle obtains its reference).  CPU only; the two grids of
4 096 columns take the better part of an hour each, which is why the result is recorded instead of recomputed by the test.

    python tools/gen_refit_golden.py [case ...]
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.cases import CASES, make_inputs  # noqa: E402

REFIT_CASES = ["c1_1d16", "1d_sparse", "2d16_zero_w", "2d16_outside", "2d32_cc_xt0", "3d8_cc_clust", "3d_aniso", "3d16",
               "2d64_c2grid", "4d6"]
OUT = os.path.join(ROOT, "tests", "golden", "refit_y2.npz")


def second_field(inp):
    return np.cos(3.0 * inp["xdata"].sum(axis=1)) + 0.25 * inp["ydata"]


def one(name):
    from oracle.binding import Port
    inp = make_inputs(CASES[name])
    c, ierr, _ = Port().fit(inp["ndim"], inp["xdata"], second_field(inp), inp["wdata"], inp["xmin"], inp["xmax"],
                            inp["nodes"], inp["xtrap"])
    assert ierr == 0, (name, ierr)
    return name, np.asarray(c[:int(np.prod(inp["nodes"]))], dtype=np.float64)


if __name__ == "__main__":
    names = sys.argv[1:] or REFIT_CASES
    have = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    with ProcessPoolExecutor(max_workers=min(len(names), 8)) as ex:
        for name, c in ex.map(one, names):
            have[name] = c
            np.savez_compressed(OUT, **have)          # (after every case: the long ones come last)
            print(name, c.size, flush=True)
