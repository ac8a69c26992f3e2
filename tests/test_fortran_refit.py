"""`refit` of the Fortran drop-in module (splpak_amd/fortran, test/test_refit.f90): new values on the points of the last
`initialize`, parity case 2d16 with a second field on the same points.

CPU tier : under set_host(.true.) and on an object that never fitted `refit` refuses with -4 and a message -- it never takes
           another path silently.
GPU tier : the refit of the second field against a fit of its own at 2e-10 (both within the 1e-10 bar of the same minimiser),
           two fields in one call, the diagnostics of the last field, and the refusals (nfields = 0, set_gpus(2), a fit that
           another fit of the process replaced).
"""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_refit")


def _ensure_built():
    if os.path.exists(PROG):
        return
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not available")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
    subprocess.check_call(["make", "-C", FDIR])


def _run(args):
    r = subprocess.run([PROG] + args, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_refit" in r.stdout and "FAILED" not in r.stdout
    return r.stdout


def test_fortran_refit_refuses_on_the_host():
    _ensure_built()
    out = _run(["host"])
    assert out.count("IERR=   -4") == 2
    assert "refit - not available under set_host" in out


@pytest.mark.gpu
def test_fortran_refit_on_gpu_matches_a_fit_of_the_same_values():
    _ensure_built()
    out = _run([])
    assert "refit vs fit of the second field" in out and "field 1 of 2 vs the fit" in out
    assert "the fit is no longer resident: fit again" in out
