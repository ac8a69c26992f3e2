"""CPU tier of the batched refit: the new entry is declared and exported, refuses null arguments without a device, and the option
refit_batch is known to the option table under both of its names."""
import ctypes as C
import os
import re

from splpak_amd import capi
from tests.conftest import ROOT


def test_refit_stats_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "splpak_hip.h")).read()
    assert re.search(r"int32_t\s+splpak_debug_plan_refit_stats\s*\(\s*const splpak_plan \*plan,\s*int64_t out4\[4\]\s*\)", text)
    assert "splpak_debug_plan_refit_stats" in capi.SYMBOLS
    assert hasattr(capi.lib(), "splpak_debug_plan_refit_stats")
    assert callable(getattr(capi.Plan, "refit_stats"))


def test_refit_stats_refuses_null_arguments_without_a_device():
    L = capi.lib()
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.splpak_debug_plan_refit_stats(None, out) == capi.E_BADARG
    assert list(out) == [7, 7, 7, 7]
    assert "null argument" in capi.last_error()
    assert L.splpak_debug_plan_refit_stats(None, None) == capi.E_BADARG


def test_refit_batch_is_a_known_option():
    L = capi.lib()
    try:
        assert capi.set_default_option("refit_batch", "4") == 0
        assert capi.set_default_option("SPLPAK_REFIT_BATCH", "4") == 0
        # (text that is no number is accepted too: it means the default.  What a plan created now reads back is checked where a
        #  plan can be created, tests/test_refit_batch.py::test_refit_batch_option_on_a_plan)
        assert L.splpak_set_default_option(b"Refit_Batch", b"not a number") == 0
    finally:
        assert capi.set_default_option("refit_batch", None) == 0
    src = open(os.path.join(ROOT, "splpak_amd", "csrc", "options.hip")).read()
    assert '{"SPLPAK_REFIT_BATCH", 1}' in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "refit_batch" in doc
