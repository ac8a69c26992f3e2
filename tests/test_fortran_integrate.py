"""`integrate_grid` and `integrate` of the Fortran drop-in module (splpak_amd/fortran, test/test_integrate.f90): cell integrals
and projections against a quadrature over the module's scalar `evaluate` that the program forms itself (cells cut at the node
lines, two Gauss-Legendre points per piece and dimension), on the eval_3d12 and eval_4d6 golden grids and on a 5-D grid.

CPU tier : under set_host(.true.) -- the module's own pieces and rule over the scalar evaluation -- at 1e-12, the bar of
           test_evalfix.
GPU tier : the same program without set_host: the HIP library's integrals against the host quadrature at 1e-10 (the 5-D grid
           is routed to the host by the module itself).
In both tiers the program also checks that `integrate` over a box has the bits of `integrate_grid` with that one cell, that a
reversed box is the exact negation and that an empty cell is 0.
"""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_integrate")
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
    assert "PASS test_integrate" in r.stdout
    assert r.stdout.count(" cells, worst relative difference") == 3


def test_fortran_integrate_on_the_host_equals_scalar_quadrature():
    _ensure_built()
    _run(["host"])


@pytest.mark.gpu
def test_fortran_integrate_on_gpu_matches_scalar_quadrature():
    _ensure_built()
    _run([])
