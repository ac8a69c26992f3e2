"""`evaluate_fields` of the Fortran drop-in module (splpak_amd/fortran, test/test_evalfields.f90): three fields formed from
the coefficients of the eval_3d12, eval_4d6 and eval_5d4 golden grids (the coefficients, -0.5 times and 4 times them), given
with ldcoef > ncol and ldf > nq, against the module's `evaluate_many` of every field -- exactly -- and against the stated
multiples of the first field -- exactly --, with the padding of `f` untouched.

CPU tier : under set_host(.true.): the module's host evaluation field by field, as evaluate_many on the host.
GPU tier : the same program without set_host: one splpak_eval_fields call of the HIP library against one splpak_eval call
           per field (the 5-D grid is routed to the host by the module itself).
"""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_evalfields")
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
    assert "PASS test_evalfields" in r.stdout
    assert r.stdout.count("query points, mismatches      0") == 3


def test_fortran_evaluate_fields_on_the_host_equals_evaluate_many():
    _ensure_built()
    _run(["host"])


@pytest.mark.gpu
def test_fortran_evaluate_fields_on_gpu_equals_evaluate_many():
    _ensure_built()
    _run([])
