#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- tests/golden/live_ref.npz: the outputs of the unmodified reference (oracle/_ref,
``make -C oracle ref``) on the seeded inputs of tests/test_oracle_golden.py::live_cases, so that
test_port_matches_live_reference runs where the reference cannot be built.  Per case <key>: coef_<key> and
hist_<key> (work(1:ncol)), ierror_<key>.

    python oracle/gen_live_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import binding  # noqa: E402
from tests.test_oracle_golden import live_cases  # noqa: E402


def main():
    if not binding.ref_available():
        raise SystemExit("oracle/_ref/libsplpak_ref.so is missing: make -C oracle ref")
    ref = binding.Reference()
    out = {}
    for key, nd, nodes, x, y, wd, xtrap in live_cases():
        n = int(np.prod(nodes))
        coef, ierr, work = ref.fit(nd, x, y, wd, [0.0] * nd, [1.0] * nd, nodes, xtrap)
        out["coef_" + key], out["hist_" + key], out["ierror_" + key] = coef[:n], work[:n], np.int64(ierr)
    path = os.path.join(ROOT, "tests", "golden", "live_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(out) // 3} cases")


if __name__ == "__main__":
    main()
