"""`evaluate_grid_derivatives` of the Fortran drop-in module (splpak_amd/fortran, test/test_evalgridderivs.f90): every
plane of the call -- value, gradient, Hessian -- against the module's scalar `evaluate` under the matching nderiv at every
grid point, on the eval_3d12 and eval_4d6 golden grids and on a 5-D grid, orders 1 and 2.

CPU tier : under set_host(.true.) -- the scalar evaluation per pattern -- at 1e-12, the bar of test_evalfix.
GPU tier : the same program without set_host: the HIP library's fused grid kernels against the host scalar evaluation at
           1e-10 (the 5-D grid is routed to the host by the module itself).
"""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_evalgridderivs")
FIXTURES = [os.path.join(ROOT, "tests", "golden", f"eval_{n}.txt") for n in ("3d12", "4d6", "5d4")]


def _ensure_built():
    if os.path.exists(PROG):
        return
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not available")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
    subprocess.check_call(["make", "-C", FDIR])


def _run(args):
    r = subprocess.run([PROG] + args + FIXTURES, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_evalgridderivs" in r.stdout
    # orders 1 and 2: (1 + D) + (1 + D + D (D + 1) / 2) planes per fixture
    for planes in (14, 20, 27):
        assert f"{planes} planes x" in r.stdout
    assert r.stdout.count(" grid points, worst relative difference") == 3


def test_fortran_evaluate_grid_derivatives_on_the_host_equals_scalar_evaluate():
    _ensure_built()
    _run(["host"])


@pytest.mark.gpu
def test_fortran_evaluate_grid_derivatives_on_gpu_matches_scalar_evaluate():
    _ensure_built()
    _run([])
