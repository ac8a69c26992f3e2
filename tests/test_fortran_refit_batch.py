"""`refit` of the Fortran drop-in module with several fields in one call on a nested-dissection grid (splpak_amd/fortran,
test/test_refitbatch.f90): three fields on 16^3 nodes in one call -- solved in shared sweeps of the factor -- against three
single-field refits, equal bits."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_refitbatch")


@pytest.mark.gpu
def test_fortran_refit_of_three_fields_is_three_single_refits():
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_refitbatch" in r.stdout and "FAILED" not in r.stdout
    assert r.stdout.count("max |many - single|") == 3
