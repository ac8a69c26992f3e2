"""ctypes plumbing over the C ABI in ``include/splpak_hip.h``.

This is NOT a second implementation: every function forwards to
``libsplpak_hip.so`` (hand-written HIP for gfx950).  It exists so that the
pytest parity suite and ``bench.py`` can drive the same entry points the Fortran
``splpak_module`` binds.  Loading fails loudly when the library is missing, and
every compute entry point fails with ``SPLPAK_E_NODEVICE`` when there is no GPU;
there is no CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPLPAK_LIB") or os.path.join(_HERE, "libsplpak_hip.so")      # SPLPAK_LIB: another build of the same library (A/B measurements)

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)

# every symbol include/splpak_hip.h declares
SYMBOLS = [
    "splpak_fit_f64", "splpak_fit_f32", "splpak_eval_f64", "splpak_eval_f32",
    "splpak_fit_token", "splpak_refit_f64", "splpak_refit_f32", "splpak_plan_refit_dev", "splpak_debug_plan_refit_stats",
    "splpak_plan_comm_len", "splpak_plan_create", "splpak_plan_destroy",
    "splpak_plan_set_allreduce", "splpak_plan_set_allreduce_ex", "splpak_plan_set_rccl", "splpak_rccl_unique_id", "splpak_rccl_comm_create",
    "splpak_rccl_comm_create_from_file", "splpak_rccl_comm_create_from_file_ex", "splpak_rccl_comm_destroy", "splpak_plan_set_refine", "splpak_plan_fit_dev",
    "splpak_plan_hist_dev", "splpak_plan_factorisation", "splpak_plan_enable_kernel_timing", "splpak_plan_kernel_timing", "splpak_plan_stage_timing",
    "splpak_eval_dev_f64", "splpak_eval_dev_f32", "splpak_eval_derivs_f64", "splpak_eval_derivs_f32", "splpak_eval_derivs_dev_f64",
    "splpak_eval_grid_f64", "splpak_eval_grid_f32", "splpak_eval_grid_dev_f64", "splpak_eval_grid_dev_f32",
    "splpak_eval_grid_scratch_bytes", "splpak_debug_eval_grid_stats",
    "splpak_eval_grid_derivs_f64", "splpak_eval_grid_derivs_f32", "splpak_eval_grid_derivs_dev_f64", "splpak_eval_grid_derivs_dev_f32",
    "splpak_eval_grid_derivs_scratch_bytes", "splpak_debug_eval_grid_derivs_tile",
    "splpak_integrate_grid_f64", "splpak_integrate_grid_f32", "splpak_integrate_grid_dev_f64", "splpak_integrate_grid_dev_f32",
    "splpak_debug_integrate_grid_stats",
    "splpak_fit_grid_f64", "splpak_fit_grid_f32", "splpak_fit_grid_dev_f64", "splpak_fit_grid_dev_f32",
    "splpak_debug_fit_grid_stage_f64", "splpak_debug_fit_grid_stats",
    "splpak_fit_grid_weighted_f64", "splpak_fit_grid_weighted_f32", "splpak_fit_grid_weighted_dev_f64",
    "splpak_fit_grid_weighted_dev_f32", "splpak_debug_fit_grid_weighted_stage_f64", "splpak_debug_fit_grid_weighted_stats",
    "splpak_fit_many_f64", "splpak_fit_many_f32", "splpak_fit_many_dev_f64", "splpak_fit_many_dev_f32", "splpak_fit_many_lds_bytes",
    "splpak_debug_fit_many_stats",
    "splpak_fit_many_clip_f64", "splpak_fit_many_clip_f32", "splpak_fit_many_clip_dev_f64", "splpak_fit_many_clip_dev_f32",
    "splpak_fit_many_clip_mad_f64", "splpak_fit_many_clip_mad_f32", "splpak_fit_many_clip_mad_dev_f64", "splpak_fit_many_clip_mad_dev_f32",
    "splpak_mad_many_f64", "splpak_mad_many_f32", "splpak_mad_many_dev_f64", "splpak_mad_many_dev_f32",
    "splpak_fit_many_cov_f64", "splpak_fit_many_cov_f32", "splpak_fit_many_cov_dev_f64", "splpak_fit_many_cov_dev_f32", "splpak_fit_many_cov_len",
    "splpak_eval_many_f64", "splpak_eval_many_f32", "splpak_eval_many_dev_f64", "splpak_eval_many_dev_f32",
    "splpak_eval_many_var_f64", "splpak_eval_many_var_f32", "splpak_eval_many_var_dev_f64", "splpak_eval_many_var_dev_f32",
    "splpak_residuals_many_f64", "splpak_residuals_many_f32", "splpak_residuals_many_dev_f64", "splpak_residuals_many_dev_f32",
    "splpak_debug_eval_many_stats",
    "splpak_eval_fields_f64", "splpak_eval_fields_f32", "splpak_eval_fields_dev_f64", "splpak_eval_fields_dev_f32",
    "splpak_debug_eval_fields_stats",
    "splpak_synth_points_f64", "splpak_synth_queries_f64",
    "splpak_mplan_create", "splpak_mplan_destroy", "splpak_mplan_device", "splpak_mplan_rank_bytes", "splpak_mplan_factorisation", "splpak_mplan_fit_dev", "splpak_fit_multi_f64",
    "splpak_plan_device_bytes", "splpak_plan_pcg_stats", "splpak_set_default_option", "splpak_plan_set_option", "splpak_plan_get_option",
    "splpak_debug_spd_band_solve_f64", "splpak_debug_plan_normal_equations", "splpak_debug_plan_solve", "splpak_debug_nd_fronts",
    "splpak_debug_bin_points", "splpak_debug_plan_gram_shape",
    "splpak_debug_plan_rows_gradient", "splpak_debug_plan_precondition", "splpak_debug_plan_pcg_tables", "splpak_debug_plan_pcg_diagonal",
    "splpak_debug_nd_tree", "splpak_debug_nd_partition", "splpak_debug_nd_schedule", "splpak_debug_window_values", "splpak_shutdown", "splpak_set_eval_mode",
    "splpak_last_error_message", "splpak_device_name",
]

E_NODEVICE, E_NOMEM, E_BADARG, E_UNSUPPORTED, E_COMM = -1, -2, -3, -4, -5
AR_ANY_POINTER = 1
AR_STREAM_ORDERED = 4

_lib = None


class SplpakError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SplpakError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); the splpak HIP path has no CPU fallback")
    # PyTorch-ROCm ships its own copy of the HIP runtime.  Two HIP runtimes in one process do not share
    # the device (whichever comes second finds "no GPUs"), so if torch is installed it is imported FIRST:
    # libsplpak_hip.so then binds to the runtime that is already loaded.  Without torch (Fortran callers,
    # plain ctypes users) the system runtime under /opt/rocm is used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.splpak_fit_f64.restype = i32
    L.splpak_fit_f64.argtypes = [i32, _dp, i32, _dp, _dp, i64, _dp, _dp, _ip, dbl, _dp, i64, i64, _dp, _dp]
    L.splpak_fit_f32.restype = i32
    L.splpak_fit_f32.argtypes = [i32, _fp, i32, _fp, _fp, i64, _fp, _fp, _ip, C.c_float, _fp, i64, i64, _fp, _dp]
    L.splpak_fit_token.restype = i64
    L.splpak_fit_token.argtypes = []
    L.splpak_refit_f64.restype = i32
    L.splpak_refit_f64.argtypes = [i64, i32, _dp, i64, i64, _dp, i64, _dp]
    L.splpak_refit_f32.restype = i32
    L.splpak_refit_f32.argtypes = [i64, i32, _fp, i64, i64, _fp, i64, _dp]
    L.splpak_plan_refit_dev.restype = i32
    L.splpak_plan_refit_dev.argtypes = [vp, i32, vp, i64, vp, i64, vp, _dp]
    L.splpak_debug_plan_refit_stats.restype = i32
    L.splpak_debug_plan_refit_stats.argtypes = [vp, _lp]
    L.splpak_eval_f64.restype = i32
    L.splpak_eval_f64.argtypes = [i32, i64, _dp, i32, _ip, _dp, _dp, _dp, _ip, _dp]
    L.splpak_eval_f32.restype = i32
    L.splpak_eval_f32.argtypes = [i32, i64, _fp, i32, _ip, _fp, _fp, _fp, _ip, _fp]
    L.splpak_plan_comm_len.restype = i64
    L.splpak_plan_comm_len.argtypes = [i32, _ip]
    L.splpak_plan_create.restype = i32
    L.splpak_plan_create.argtypes = [i32, _ip, _dp, _dp, dbl, i64, vp, i64, C.POINTER(vp)]
    L.splpak_plan_destroy.restype = None
    L.splpak_plan_destroy.argtypes = [vp]
    L.splpak_plan_set_allreduce.restype = None
    L.splpak_plan_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp, i32, i32]
    L.splpak_plan_set_allreduce_ex.restype = i32
    L.splpak_plan_set_allreduce_ex.argtypes = [vp, ALLREDUCE_FN, vp, i32, i32, i32]
    L.splpak_plan_set_rccl.restype = i32
    L.splpak_plan_set_rccl.argtypes = [vp, vp, i32, i32]
    L.splpak_rccl_unique_id.restype = i32
    L.splpak_rccl_unique_id.argtypes = [C.c_char_p]
    L.splpak_rccl_comm_create.restype = i32
    L.splpak_rccl_comm_create.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.splpak_rccl_comm_create_from_file.restype = i32
    L.splpak_rccl_comm_create_from_file.argtypes = [C.c_char_p, i32, i32, dbl, C.POINTER(vp)]
    L.splpak_rccl_comm_create_from_file_ex.restype = i32
    L.splpak_rccl_comm_create_from_file_ex.argtypes = [C.c_char_p, C.c_char_p, i32, i32, dbl, C.POINTER(vp)]
    L.splpak_rccl_comm_destroy.restype = None
    L.splpak_rccl_comm_destroy.argtypes = [vp]
    L.splpak_plan_set_refine.restype = None
    L.splpak_plan_set_refine.argtypes = [vp, i32, dbl]
    L.splpak_plan_fit_dev.restype = i32
    L.splpak_plan_fit_dev.argtypes = [vp, vp, i32, vp, vp, i64, vp, vp, _dp]
    L.splpak_plan_hist_dev.restype = vp
    L.splpak_plan_hist_dev.argtypes = [vp]
    L.splpak_plan_factorisation.restype = i32
    L.splpak_plan_factorisation.argtypes = [vp, C.c_char_p, i32]
    L.splpak_plan_enable_kernel_timing.restype = None
    L.splpak_plan_enable_kernel_timing.argtypes = [vp, i32]
    L.splpak_plan_kernel_timing.restype = None
    L.splpak_plan_kernel_timing.argtypes = [vp, _dp]
    L.splpak_plan_stage_timing.restype = None
    L.splpak_plan_stage_timing.argtypes = [vp, _dp]
    L.splpak_eval_dev_f64.restype = i32
    L.splpak_eval_dev_f64.argtypes = [i32, i64, vp, i32, _ip, vp, _dp, _dp, _ip, vp, vp]
    L.splpak_eval_dev_f32.restype = i32
    L.splpak_eval_dev_f32.argtypes = [i32, i64, vp, i32, _ip, vp, _fp, _fp, _ip, vp, vp]
    L.splpak_eval_derivs_f64.restype = i32
    L.splpak_eval_derivs_f64.argtypes = [i32, i64, _dp, i32, i32, _dp, _dp, _dp, _ip, _dp, i32]
    L.splpak_eval_derivs_f32.restype = i32
    L.splpak_eval_derivs_f32.argtypes = [i32, i64, _fp, i32, i32, _fp, _fp, _fp, _ip, _fp, i32]
    L.splpak_eval_derivs_dev_f64.restype = i32
    L.splpak_eval_derivs_dev_f64.argtypes = [i32, i64, vp, i32, i32, vp, _dp, _dp, _ip, vp, i32, vp]
    L.splpak_eval_grid_f64.restype = i32
    L.splpak_eval_grid_f64.argtypes = [i32, _lp, _dp, _ip, _dp, _dp, _dp, _ip, _dp]
    L.splpak_eval_grid_f32.restype = i32
    L.splpak_eval_grid_f32.argtypes = [i32, _lp, _fp, _ip, _fp, _fp, _fp, _ip, _fp]
    L.splpak_eval_grid_dev_f64.restype = i32
    L.splpak_eval_grid_dev_f64.argtypes = [i32, _lp, vp, _ip, vp, _dp, _dp, _ip, vp, vp]
    L.splpak_eval_grid_dev_f32.restype = i32
    L.splpak_eval_grid_dev_f32.argtypes = [i32, _lp, vp, _ip, vp, _fp, _fp, _ip, vp, vp]
    L.splpak_eval_grid_scratch_bytes.restype = i64
    L.splpak_eval_grid_scratch_bytes.argtypes = [i32, _lp]
    L.splpak_debug_eval_grid_stats.restype = i32
    L.splpak_debug_eval_grid_stats.argtypes = [_lp]
    L.splpak_eval_grid_derivs_f64.restype = i32
    L.splpak_eval_grid_derivs_f64.argtypes = [i32, _lp, _dp, i32, _dp, _dp, _dp, _ip, _dp, i64]
    L.splpak_eval_grid_derivs_f32.restype = i32
    L.splpak_eval_grid_derivs_f32.argtypes = [i32, _lp, _fp, i32, _fp, _fp, _fp, _ip, _fp, i64]
    L.splpak_eval_grid_derivs_dev_f64.restype = i32
    L.splpak_eval_grid_derivs_dev_f64.argtypes = [i32, _lp, vp, i32, vp, _dp, _dp, _ip, vp, i64, vp]
    L.splpak_eval_grid_derivs_dev_f32.restype = i32
    L.splpak_eval_grid_derivs_dev_f32.argtypes = [i32, _lp, vp, i32, vp, _fp, _fp, _ip, vp, i64, vp]
    L.splpak_eval_grid_derivs_scratch_bytes.restype = i64
    L.splpak_eval_grid_derivs_scratch_bytes.argtypes = [i32, _lp, i32]
    L.splpak_debug_eval_grid_derivs_tile.restype = i32
    L.splpak_debug_eval_grid_derivs_tile.argtypes = [i32, i32, _ip]
    L.splpak_integrate_grid_f64.restype = i32
    L.splpak_integrate_grid_f64.argtypes = [i32, _lp, _ip, _dp, _dp, _dp, _dp, _ip, _dp]
    L.splpak_integrate_grid_f32.restype = i32
    L.splpak_integrate_grid_f32.argtypes = [i32, _lp, _ip, _fp, _fp, _fp, _fp, _ip, _fp]
    L.splpak_integrate_grid_dev_f64.restype = i32
    L.splpak_integrate_grid_dev_f64.argtypes = [i32, _lp, _ip, vp, vp, _dp, _dp, _ip, vp, vp]
    L.splpak_integrate_grid_dev_f32.restype = i32
    L.splpak_integrate_grid_dev_f32.argtypes = [i32, _lp, _ip, vp, vp, _fp, _fp, _ip, vp, vp]
    L.splpak_debug_integrate_grid_stats.restype = i32
    L.splpak_debug_integrate_grid_stats.argtypes = [_lp]
    L.splpak_fit_grid_f64.restype = i32
    L.splpak_fit_grid_f64.argtypes = [i32, _lp, _dp, _dp, i32, _dp, i64, _dp, _dp, _ip, dbl, _dp, i64, _dp]
    L.splpak_fit_grid_f32.restype = i32
    L.splpak_fit_grid_f32.argtypes = [i32, _lp, _fp, _fp, i32, _fp, i64, _fp, _fp, _ip, C.c_float, _fp, i64, _dp]
    L.splpak_fit_grid_dev_f64.restype = i32
    L.splpak_fit_grid_dev_f64.argtypes = [i32, _lp, vp, vp, i32, vp, i64, _dp, _dp, _ip, dbl, vp, i64, _dp, vp]
    L.splpak_fit_grid_dev_f32.restype = i32
    L.splpak_fit_grid_dev_f32.argtypes = [i32, _lp, vp, vp, i32, vp, i64, _fp, _fp, _ip, C.c_float, vp, i64, _dp, vp]
    L.splpak_debug_fit_grid_stage_f64.restype = i32
    L.splpak_debug_fit_grid_stage_f64.argtypes = [i32, i32, _lp, _dp, _dp, _dp, _dp, _ip, _dp, _dp]
    L.splpak_debug_fit_grid_stats.restype = i32
    L.splpak_debug_fit_grid_stats.argtypes = [_lp]
    L.splpak_fit_grid_weighted_f64.restype = i32
    L.splpak_fit_grid_weighted_f64.argtypes = [i32, _lp, _dp, i32, _dp, i64, _dp, i64, _dp, _dp, _ip, dbl, _dp, i64, _dp]
    L.splpak_fit_grid_weighted_f32.restype = i32
    L.splpak_fit_grid_weighted_f32.argtypes = [i32, _lp, _fp, i32, _fp, i64, _fp, i64, _fp, _fp, _ip, C.c_float, _fp, i64, _dp]
    L.splpak_fit_grid_weighted_dev_f64.restype = i32
    L.splpak_fit_grid_weighted_dev_f64.argtypes = [i32, _lp, vp, i32, vp, i64, vp, i64, _dp, _dp, _ip, dbl, vp, i64, _dp, vp]
    L.splpak_fit_grid_weighted_dev_f32.restype = i32
    L.splpak_fit_grid_weighted_dev_f32.argtypes = [i32, _lp, vp, i32, vp, i64, vp, i64, _fp, _fp, _ip, C.c_float, vp, i64, _dp, vp]
    L.splpak_debug_fit_grid_weighted_stage_f64.restype = i32
    L.splpak_debug_fit_grid_weighted_stage_f64.argtypes = [i32, i32, _lp, _dp, _dp, _dp, _dp, _ip, _dp, _dp]
    L.splpak_debug_fit_grid_weighted_stats.restype = i32
    L.splpak_debug_fit_grid_weighted_stats.argtypes = [_lp]
    L.splpak_fit_many_f64.restype = i32
    L.splpak_fit_many_f64.argtypes = [i32, i32, _lp, _dp, i32, _dp, _dp, _dp, _dp, _ip, dbl, _dp, i64, _ip, _dp]
    L.splpak_fit_many_f32.restype = i32
    L.splpak_fit_many_f32.argtypes = [i32, i32, _lp, _fp, i32, _fp, _fp, _fp, _fp, _ip, C.c_float, _fp, i64, _ip, _dp]
    L.splpak_fit_many_dev_f64.restype = i32
    L.splpak_fit_many_dev_f64.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _dp, _dp, _ip, dbl, vp, i64, _ip, _dp, vp]
    L.splpak_fit_many_dev_f32.restype = i32
    L.splpak_fit_many_dev_f32.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _fp, _fp, _ip, C.c_float, vp, i64, _ip, _dp, vp]
    L.splpak_fit_many_lds_bytes.restype = i64
    L.splpak_fit_many_lds_bytes.argtypes = [i32, _ip]
    L.splpak_debug_fit_many_stats.restype = i32
    L.splpak_debug_fit_many_stats.argtypes = [_lp]
    flt = C.c_float
    L.splpak_fit_many_clip_f64.restype = i32
    L.splpak_fit_many_clip_f64.argtypes = [i32, i32, _lp, _dp, i32, _dp, _dp, _dp, _dp, _ip, dbl, dbl, dbl, i32, _dp, _dp, i64, _ip, _dp, _dp]
    L.splpak_fit_many_clip_f32.restype = i32
    L.splpak_fit_many_clip_f32.argtypes = [i32, i32, _lp, _fp, i32, _fp, _fp, _fp, _fp, _ip, flt, flt, flt, i32, _fp, _fp, i64, _ip, _dp, _dp]
    L.splpak_fit_many_clip_dev_f64.restype = i32
    L.splpak_fit_many_clip_dev_f64.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _dp, _dp, _ip, dbl, dbl, dbl, i32, vp, vp, i64, _ip, _dp, _dp, vp]
    L.splpak_fit_many_clip_dev_f32.restype = i32
    L.splpak_fit_many_clip_dev_f32.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _fp, _fp, _ip, flt, flt, flt, i32, vp, vp, i64, _ip, _dp, _dp, vp]
    L.splpak_fit_many_cov_f64.restype = i32
    L.splpak_fit_many_cov_f64.argtypes = [i32, i32, _lp, _dp, i32, _dp, _dp, _dp, _dp, _ip, dbl, _dp, i64, _dp, i64, _ip, _dp]
    L.splpak_fit_many_cov_f32.restype = i32
    L.splpak_fit_many_cov_f32.argtypes = [i32, i32, _lp, _fp, i32, _fp, _fp, _fp, _fp, _ip, flt, _fp, i64, _fp, i64, _ip, _dp]
    L.splpak_fit_many_cov_dev_f64.restype = i32
    L.splpak_fit_many_cov_dev_f64.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _dp, _dp, _ip, dbl, vp, i64, vp, i64, _ip, _dp, vp]
    L.splpak_fit_many_cov_dev_f32.restype = i32
    L.splpak_fit_many_cov_dev_f32.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _fp, _fp, _ip, flt, vp, i64, vp, i64, _ip, _dp, vp]
    L.splpak_fit_many_cov_len.restype = i64
    L.splpak_fit_many_cov_len.argtypes = [i32, _ip]
    L.splpak_eval_many_var_f64.restype = i32
    L.splpak_eval_many_var_f64.argtypes = [i32, i32, _lp, _dp, i32, _ip, _dp, i64, _dp, _dp, _ip, _dp]
    L.splpak_eval_many_var_f32.restype = i32
    L.splpak_eval_many_var_f32.argtypes = [i32, i32, _lp, _fp, i32, _ip, _fp, i64, _fp, _fp, _ip, _fp]
    L.splpak_eval_many_var_dev_f64.restype = i32
    L.splpak_eval_many_var_dev_f64.argtypes = [i32, i32, _lp, vp, i32, _ip, vp, i64, _dp, _dp, _ip, vp, vp]
    L.splpak_eval_many_var_dev_f32.restype = i32
    L.splpak_eval_many_var_dev_f32.argtypes = [i32, i32, _lp, vp, i32, _ip, vp, i64, _fp, _fp, _ip, vp, vp]
    L.splpak_eval_many_f64.restype = i32
    L.splpak_eval_many_f64.argtypes = [i32, i32, _lp, _dp, i32, _ip, _dp, i64, _dp, _dp, _ip, _dp]
    L.splpak_eval_many_f32.restype = i32
    L.splpak_eval_many_f32.argtypes = [i32, i32, _lp, _fp, i32, _ip, _fp, i64, _fp, _fp, _ip, _fp]
    L.splpak_eval_many_dev_f64.restype = i32
    L.splpak_eval_many_dev_f64.argtypes = [i32, i32, _lp, vp, i32, _ip, vp, i64, _dp, _dp, _ip, vp, vp]
    L.splpak_eval_many_dev_f32.restype = i32
    L.splpak_eval_many_dev_f32.argtypes = [i32, i32, _lp, vp, i32, _ip, vp, i64, _fp, _fp, _ip, vp, vp]
    L.splpak_fit_many_clip_mad_f64.restype = i32
    L.splpak_fit_many_clip_mad_f64.argtypes = [i32, i32, _lp, _dp, i32, _dp, _dp, _dp, _dp, _ip, dbl, dbl, dbl, i32, i32, _dp, _dp, i64, _ip, _dp, _dp]
    L.splpak_fit_many_clip_mad_f32.restype = i32
    L.splpak_fit_many_clip_mad_f32.argtypes = [i32, i32, _lp, _fp, i32, _fp, _fp, _fp, _fp, _ip, flt, flt, flt, i32, i32, _fp, _fp, i64, _ip, _dp, _dp]
    L.splpak_fit_many_clip_mad_dev_f64.restype = i32
    L.splpak_fit_many_clip_mad_dev_f64.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _dp, _dp, _ip, dbl, dbl, dbl, i32, i32, vp, vp, i64, _ip, _dp, _dp, vp]
    L.splpak_fit_many_clip_mad_dev_f32.restype = i32
    L.splpak_fit_many_clip_mad_dev_f32.argtypes = [i32, i32, _lp, vp, i32, vp, vp, _fp, _fp, _ip, flt, flt, flt, i32, i32, vp, vp, i64, _ip, _dp, _dp, vp]
    L.splpak_mad_many_f64.restype = i32
    L.splpak_mad_many_f64.argtypes = [i32, _lp, _dp, _dp, _dp]
    L.splpak_mad_many_f32.restype = i32
    L.splpak_mad_many_f32.argtypes = [i32, _lp, _fp, _fp, _dp]
    L.splpak_mad_many_dev_f64.restype = i32
    L.splpak_mad_many_dev_f64.argtypes = [i32, _lp, vp, vp, vp, vp]
    L.splpak_mad_many_dev_f32.restype = i32
    L.splpak_mad_many_dev_f32.argtypes = [i32, _lp, vp, vp, vp, vp]
    L.splpak_residuals_many_f64.restype = i32
    L.splpak_residuals_many_f64.argtypes = [i32, i32, _lp, _dp, i32, _dp, _dp, _dp, i64, _dp, _dp, _ip, _dp, _dp]
    L.splpak_residuals_many_f32.restype = i32
    L.splpak_residuals_many_f32.argtypes = [i32, i32, _lp, _fp, i32, _fp, _fp, _fp, i64, _fp, _fp, _ip, _fp, _dp]
    L.splpak_residuals_many_dev_f64.restype = i32
    L.splpak_residuals_many_dev_f64.argtypes = [i32, i32, _lp, vp, i32, vp, vp, vp, i64, _dp, _dp, _ip, vp, vp, vp]
    L.splpak_residuals_many_dev_f32.restype = i32
    L.splpak_residuals_many_dev_f32.argtypes = [i32, i32, _lp, vp, i32, vp, vp, vp, i64, _fp, _fp, _ip, vp, vp, vp]
    L.splpak_debug_eval_many_stats.restype = i32
    L.splpak_debug_eval_many_stats.argtypes = [_lp]
    L.splpak_eval_fields_f64.restype = i32
    L.splpak_eval_fields_f64.argtypes = [i32, i64, _dp, i32, _ip, i32, _dp, i64, _dp, _dp, _ip, _dp, i64]
    L.splpak_eval_fields_f32.restype = i32
    L.splpak_eval_fields_f32.argtypes = [i32, i64, _fp, i32, _ip, i32, _fp, i64, _fp, _fp, _ip, _fp, i64]
    L.splpak_eval_fields_dev_f64.restype = i32
    L.splpak_eval_fields_dev_f64.argtypes = [i32, i64, vp, i32, _ip, i32, vp, i64, _dp, _dp, _ip, vp, i64, vp]
    L.splpak_eval_fields_dev_f32.restype = i32
    L.splpak_eval_fields_dev_f32.argtypes = [i32, i64, vp, i32, _ip, i32, vp, i64, _fp, _fp, _ip, vp, i64, vp]
    L.splpak_debug_eval_fields_stats.restype = i32
    L.splpak_debug_eval_fields_stats.argtypes = [_lp]
    L.splpak_synth_points_f64.restype = i32
    L.splpak_synth_points_f64.argtypes = [i32, i64, i64, vp, vp, vp, vp]
    L.splpak_synth_queries_f64.restype = i32
    L.splpak_synth_queries_f64.argtypes = [i32, i64, i64, i64, vp, vp]
    L.splpak_debug_spd_band_solve_f64.restype = i32
    L.splpak_debug_spd_band_solve_f64.argtypes = [i32, i32, _dp, _dp, _dp]
    L.splpak_debug_plan_normal_equations.restype = i32
    L.splpak_debug_plan_normal_equations.argtypes = [vp, _dp, _dp]
    L.splpak_debug_plan_solve.restype = i32
    L.splpak_debug_plan_solve.argtypes = [vp, _dp, _dp, _dp, _dp]
    L.splpak_debug_plan_gram_shape.restype = i32
    L.splpak_debug_plan_gram_shape.argtypes = [vp, _ip]
    L.splpak_debug_bin_points.restype = i32
    L.splpak_debug_bin_points.argtypes = [i32, _ip, _dp, _dp, i64, _dp, i32, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _dp, _dp, _dp,
                                          C.POINTER(i64), _dp]
    L.splpak_debug_plan_rows_gradient.restype = i32
    L.splpak_debug_plan_rows_gradient.argtypes = [vp, _dp, i32, _dp, _dp, _dp]
    L.splpak_debug_plan_precondition.restype = i32
    L.splpak_debug_plan_precondition.argtypes = [vp, i32, _dp, _dp]
    L.splpak_debug_plan_pcg_tables.restype = i32
    L.splpak_debug_plan_pcg_tables.argtypes = [vp, i32, _dp, _dp, _ip]
    L.splpak_debug_plan_pcg_diagonal.restype = i32
    L.splpak_debug_plan_pcg_diagonal.argtypes = [vp, _dp]
    L.splpak_debug_nd_fronts.restype = i32
    L.splpak_debug_nd_fronts.argtypes = [i32, _ip, i32, _ip, i32, _ip, _ip, _ip, _ip, _ip, _ip]
    L.splpak_debug_nd_tree.restype = i32
    L.splpak_debug_nd_tree.argtypes = [i32, _ip, i32, i32, _dp]
    L.splpak_debug_nd_schedule.restype = i32
    L.splpak_debug_nd_schedule.argtypes = [i32, _ip, i32, i32, i32, _dp]
    L.splpak_debug_nd_partition.restype = i32
    L.splpak_debug_nd_partition.argtypes = [i32, _ip, i32, i32, i32, _dp, _dp]
    L.splpak_debug_window_values.restype = i32
    L.splpak_debug_window_values.argtypes = [i32, dbl, dbl, i64, _dp, _ip, _dp, _dp, _ip]
    L.splpak_mplan_create.restype = i32
    L.splpak_mplan_create.argtypes = [i32, _ip, i32, i32, _ip, _dp, _dp, dbl, i64, C.POINTER(vp)]
    L.splpak_mplan_destroy.restype = None
    L.splpak_mplan_destroy.argtypes = [vp]
    L.splpak_mplan_device.restype = i32
    L.splpak_mplan_device.argtypes = [vp, i32]
    L.splpak_mplan_factorisation.restype = i32
    L.splpak_mplan_factorisation.argtypes = [vp, C.c_char_p, i32]
    L.splpak_mplan_rank_bytes.restype = i64
    L.splpak_mplan_rank_bytes.argtypes = [vp, i32]
    L.splpak_set_default_option.restype = i32
    L.splpak_set_default_option.argtypes = [C.c_char_p, C.c_char_p]
    L.splpak_plan_set_option.restype = i32
    L.splpak_plan_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.splpak_plan_get_option.restype = i32
    L.splpak_plan_get_option.argtypes = [vp, C.c_char_p, C.c_char_p, i32]
    L.splpak_plan_pcg_stats.restype = None
    L.splpak_plan_pcg_stats.argtypes = [vp, _dp]
    L.splpak_plan_device_bytes.restype = i64
    L.splpak_plan_device_bytes.argtypes = [vp]
    L.splpak_mplan_fit_dev.restype = i32
    L.splpak_mplan_fit_dev.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp, _dp]
    L.splpak_fit_multi_f64.restype = i32
    L.splpak_fit_multi_f64.argtypes = [i32, i32, _dp, i32, _dp, _dp, i64, _dp, _dp, _ip, dbl, _dp, i64, i64, _dp, _dp]
    L.splpak_shutdown.restype = None
    L.splpak_shutdown.argtypes = []
    L.splpak_set_eval_mode.restype = i32
    L.splpak_set_eval_mode.argtypes = [i32, i64]
    L.splpak_last_error_message.restype = i32
    L.splpak_last_error_message.argtypes = [C.c_char_p, i32]
    L.splpak_device_name.restype = i32
    L.splpak_device_name.argtypes = [C.c_char_p, i32]
    _lib = L
    import atexit
    atexit.register(L.splpak_shutdown)
    return L


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().splpak_last_error_message(buf, 512)
    return buf.value.decode(errors="replace")


def _check(rc: int) -> int:
    """Negative = infrastructure failure -> raise; >= 0 is the reference's ierror."""
    if rc < 0:
        raise SplpakError(f"splpak HIP library error {rc}: {last_error()}")
    return rc


def set_default_option(name, value) -> int:
    """Process-wide default of an option (what SPLPAK_<NAME> in the environment would set) for plans created afterwards;
    value None removes it.  Raises on an unknown name."""
    return _check(lib().splpak_set_default_option(name.encode(), None if value is None else str(value).encode()))


def shutdown() -> None:
    """Release the library's cached one-shot plan (28 GB at 64^3), staging buffers and evaluation scratch."""
    lib().splpak_shutdown()


def device_name() -> str:
    buf = C.create_string_buffer(256)
    _check(lib().splpak_device_name(buf, 256))
    return buf.value.decode()


def _p(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def _grid(ndim, xmin, xmax, nodes, dt=np.float64):
    xmin = np.ascontiguousarray(np.atleast_1d(xmin), dtype=dt)
    xmax = np.ascontiguousarray(np.atleast_1d(xmax), dtype=dt)
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    return xmin, xmax, nodes


# ---------------------------------------------------------------------------
# host-pointer entry points (what splpak_module binds)
# ---------------------------------------------------------------------------

def fit(ndim, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, ncf=None, nwrk=-1, ndata=None,
        l1xdat=None, want_hist=False, real32=False):
    """splcw (wdata given) / splcc (wdata None).  -> (coef, ierror, hist|None, info)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    xdata = np.ascontiguousarray(xdata, dtype=dt)
    if xdata.ndim == 1:
        xdata = xdata.reshape(-1, 1)
    ydata = np.ascontiguousarray(ydata, dtype=dt)
    if wdata is not None:
        wdata = np.ascontiguousarray(wdata, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    if ndata is None:
        ndata = xdata.shape[0]
    if l1xdat is None:
        l1xdat = xdata.shape[1]
    ncol = int(np.prod(np.maximum(nodes[:max(ndim, 1)].astype(np.int64), 1)))
    if ncf is None:
        ncf = ncol
    coef = np.zeros(max(ncf, 1), dtype=dt)
    hist = np.zeros(max(ncol, 1), dtype=dt) if want_hist else None
    info = np.zeros(10)
    fn = lib().splpak_fit_f32 if real32 else lib().splpak_fit_f64
    xt = C.c_float(xtrap) if real32 else C.c_double(xtrap)
    rc = _check(fn(ndim, _p(xdata, rp), l1xdat, _p(ydata, rp), _p(wdata, rp), ndata, _p(xmin, rp),
                   _p(xmax, rp), _p(nodes, _ip), xt, _p(coef, rp), ncf, nwrk, _p(hist, rp),
                   _p(info, _dp)))
    return coef, rc, hist, info


def fit_token() -> int:
    """Token of this thread's last successful one-shot fit() (0: none) -- what refit() takes."""
    return int(lib().splpak_fit_token())


def refit(token, ydata, ncol, real32=False, ldcoef=None):
    """New values on the points of the one-shot fit `token`: ydata is (nfields, ndata) or (ndata,), in that fit's point order;
    `ncol` the fit's number of coefficients.  -> (coef of shape (nfields, ldcoef or ncol) -- (ncol,) for a 1-D ydata --, ierror,
    info of shape (nfields, 10)).  Raises SplpakError when the fit is no longer resident (fit again)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    ydata = np.ascontiguousarray(ydata, dtype=dt)
    single = ydata.ndim == 1
    y2 = ydata.reshape(1, -1) if single else ydata
    nfields, ndata = y2.shape
    ldc = int(ncol if ldcoef is None else ldcoef)
    coef = np.zeros((max(nfields, 1), max(ldc, 1)), dtype=dt)
    info = np.zeros((max(nfields, 1), 10))
    fn = lib().splpak_refit_f32 if real32 else lib().splpak_refit_f64
    rc = _check(fn(int(token), int(nfields), _p(y2, rp), int(ndata), int(ndata), _p(coef, rp), ldc, _p(info, _dp)))
    return (coef[0] if single else coef), rc, (info[0] if single else info)


def fit_multi(ngpus, ndim, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, want_hist=False):
    """splcw / splcc on `ngpus` GPUs of this node (distributed band, one process).  -> (coef, ierror, hist|None, info)."""
    xdata = np.ascontiguousarray(xdata, dtype=np.float64)
    if xdata.ndim == 1:
        xdata = xdata.reshape(-1, 1)
    ydata = np.ascontiguousarray(ydata, dtype=np.float64)
    if wdata is not None:
        wdata = np.ascontiguousarray(wdata, dtype=np.float64)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    ncol = int(np.prod(np.maximum(nodes[:max(ndim, 1)].astype(np.int64), 1)))
    coef = np.zeros(max(ncol, 1))
    hist = np.zeros(max(ncol, 1)) if want_hist else None
    info = np.zeros(10)
    rc = _check(lib().splpak_fit_multi_f64(int(ngpus), ndim, _p(xdata, _dp), xdata.shape[1], _p(ydata, _dp), _p(wdata, _dp),
                                           xdata.shape[0], _p(xmin, _dp), _p(xmax, _dp), _p(nodes, _ip), float(xtrap),
                                           _p(coef, _dp), ncol, -1, _p(hist, _dp), _p(info, _dp)))
    return coef, rc, hist, info


class MultiPlan:
    """A fit plan over several GPUs of this node (one process; torch tensors own the shards)."""

    def __init__(self, ngpus, ndim, nodes, xmin, xmax, xtrap, max_ndata_per_gpu, devices=None, chunk=0):
        self._L = lib()
        self.ngpus = int(ngpus)
        self.xmin, self.xmax, self.nodes = _grid(ndim, xmin, xmax, nodes)
        dv = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        rc = self._L.splpak_mplan_create(self.ngpus, _p(dv, _ip), int(chunk), ndim, _p(self.nodes, _ip), _p(self.xmin, _dp),
                                         _p(self.xmax, _dp), float(xtrap), int(max_ndata_per_gpu), C.byref(h))
        if rc != 0:
            if rc < 0:
                _check(rc)
            raise SplpakError(f"multi-GPU plan rejected with ierror {rc}")
        self._h = h

    def device(self, rank):
        return int(self._L.splpak_mplan_device(self._h, int(rank)))

    def factorisation(self):
        """-> (code, description): 3 distributed band, 5 distributed nested dissection (one rank: the single-GPU codes)."""
        buf = C.create_string_buffer(640)
        code = self._L.splpak_mplan_factorisation(self._h, buf, 640)
        return int(code), buf.value.decode()

    def rank_bytes(self, rank):
        """Device memory rank `rank` of the plan holds (bytes)."""
        return int(self._L.splpak_mplan_rank_bytes(self._h, int(rank)))

    def fit(self, xs, ys, ws, coef):
        """xs/ys/ws: lists (one entry per rank) of float64 device tensors on that rank's GPU (ws may be
        None); coef: float64 tensor on rank 0's GPU.  Blocks.  -> (ierror, info)."""
        R = self.ngpus
        vp = C.c_void_p
        ax = (vp * R)(*[vp(t.data_ptr()) for t in xs])
        ay = (vp * R)(*[vp(t.data_ptr()) for t in ys])
        aw = None if ws is None else (vp * R)(*[vp(t.data_ptr()) for t in ws])
        nn = (C.c_int64 * R)(*[int(t.shape[0]) for t in xs])
        info = np.zeros(10)
        rc = self._L.splpak_mplan_fit_dev(self._h, ax, int(xs[0].shape[1]), ay, aw, nn, vp(coef.data_ptr()), _p(info, _dp))
        return _check(rc), info

    def close(self):
        if getattr(self, "_h", None):
            self._L.splpak_mplan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def evaluate(ndim, xq, nderiv, coef, xmin, xmax, nodes, real32=False):
    """Batched splde (nderiv given) / splfe (nderiv None).  -> (values, ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    xq = np.ascontiguousarray(xq, dtype=dt)
    if xq.ndim == 1:
        xq = xq.reshape(-1, 1)
    nq, ldx = xq.shape
    coef = np.ascontiguousarray(coef, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    out = np.zeros(nq, dtype=dt)
    fn = lib().splpak_eval_f32 if real32 else lib().splpak_eval_f64
    rc = _check(fn(ndim, nq, _p(xq, rp), ldx, _p(nd, _ip), _p(coef, rp), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp)))
    return out, rc


def _axes_cat(axes, dt):
    """(entries per axis as int64, the axes back to back) of a list of 1-D arrays."""
    axes = [np.ascontiguousarray(a, dtype=dt).ravel() for a in axes]
    sizes = np.array([a.size for a in axes], dtype=np.int64)
    return sizes, (np.ascontiguousarray(np.concatenate(axes)) if axes else np.zeros(0, dtype=dt))


def evaluate_grid(ndim, axes, nderiv, coef, xmin, xmax, nodes, real32=False):
    """splde (nderiv given) / splfe (nderiv None) at every point of the tensor-product grid axes[0] x axes[1] x ...
    `axes` is a list of `ndim` 1-D arrays (any order, repeats and points outside the grid allowed).
    -> (values of shape (len(axes[ndim-1]), ..., len(axes[0])), C-ordered: the LAST index runs along dimension 1; ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    npts, cat = _axes_cat(axes, dt)
    coef = np.ascontiguousarray(coef, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    out = np.zeros(tuple(int(n) for n in npts[::-1]), dtype=dt)
    fn = lib().splpak_eval_grid_f32 if real32 else lib().splpak_eval_grid_f64
    rc = _check(fn(ndim, _p(npts, _lp), _p(cat, rp), _p(nd, _ip), _p(coef, rp), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp)))
    return out, rc


def eval_grid_scratch_bytes(npts) -> int:
    """Bytes of per-thread device scratch a grid call of this shape keeps until shutdown()."""
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    return _check(lib().splpak_eval_grid_scratch_bytes(int(npts.size), _p(npts, _lp)))


def debug_eval_grid_stats():
    """(tiles that took the LDS form, tiles that took the general form) in this thread's last grid call; waits for it."""
    v = np.zeros(2, dtype=np.int64)
    _check(lib().splpak_debug_eval_grid_stats(_p(v, _lp)))
    return int(v[0]), int(v[1])


def evaluate_grid_derivs(ndim, axes, order, coef, xmin, xmax, nodes, real32=False):
    """Value, gradient and (order 2) Hessian at every point of the tensor-product grid axes[0] x axes[1] x ...
    (splpak_eval_grid_derivs_*).  -> (array of shape (nplanes, len(axes[ndim-1]), ..., len(axes[0])): plane e is entry e of
    evaluate_derivs, each plane a volume as evaluate_grid returns it; ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    npts, cat = _axes_cat(axes, dt)
    coef = np.ascontiguousarray(coef, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    out = np.zeros((derivs_nout(max(int(ndim), 0), order),) + tuple(int(n) for n in npts[::-1]), dtype=dt)
    fn = lib().splpak_eval_grid_derivs_f32 if real32 else lib().splpak_eval_grid_derivs_f64
    rc = _check(fn(ndim, _p(npts, _lp), _p(cat, rp), int(order), _p(coef, rp), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp), int(np.prod(npts)) if npts.size else 1))
    return out, rc


def eval_grid_derivs_scratch_bytes(npts, order) -> int:
    """Bytes of per-thread device scratch a grid-derivatives call of this shape keeps until shutdown()."""
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    return _check(lib().splpak_eval_grid_derivs_scratch_bytes(int(npts.size), _p(npts, _lp), int(order)))


def debug_eval_grid_derivs_tile(ndim, order):
    """Outputs per workgroup tile per dimension (1 beyond ndim) of a grid-derivatives call with this ndim and order."""
    v = np.zeros(4, dtype=np.int32)
    _check(lib().splpak_debug_eval_grid_derivs_tile(int(ndim), int(order), _p(v, _ip)))
    return tuple(int(t) for t in v)


def integrate_grid(ndim, axes, mode, coef, xmin, xmax, nodes, real32=False):
    """Integrals of the fit over the cells of a tensor grid (splpak_integrate_grid_*).  `axes` is a list of `ndim` 1-D arrays:
    the n + 1 edges of the n cells of a dimension with mode[d] = 1 (integrated), the n coordinates of one with mode[d] = 0
    (evaluated); mode None: every dimension is integrated.  Edges may be unsorted, repeated, reversed or outside the grid.
    -> (values of shape (n_ndim, ..., n_1), C-ordered as evaluate_grid returns its own; ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    sizes, cat = _axes_cat(axes, dt)
    md = None if mode is None else np.ascontiguousarray(mode, dtype=np.int32)
    ncell = np.array([n - (1 if md is None else int(md[d] == 1)) for d, n in enumerate(sizes)], dtype=np.int64)
    coef = np.ascontiguousarray(coef, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    out = np.zeros(tuple(max(int(n), 0) for n in ncell[::-1]), dtype=dt)
    fn = lib().splpak_integrate_grid_f32 if real32 else lib().splpak_integrate_grid_f64
    rc = _check(fn(ndim, _p(ncell, _lp), _p(md, _ip), _p(cat, rp), _p(coef, rp), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp)))
    return out, rc


def debug_integrate_grid_stats():
    """Host counters of this thread's last integrate_grid call: (slabs, doubles of intermediate held, table entries of the four
    axes, reduction launches, 0)."""
    v = np.zeros(8, dtype=np.int64)
    _check(lib().splpak_debug_integrate_grid_stats(_p(v, _lp)))
    return tuple(int(t) for t in v)


def _grid_axes(axes, waxes, dt):
    """(npts, the axes back to back, the weights back to back or None) of a list of 1-D arrays."""
    npts, cat = _axes_cat(axes, dt)
    wcat = None
    if waxes is not None:
        wsizes, wcat = _axes_cat(waxes, dt)
        if wsizes.tolist() != npts.tolist():
            raise SplpakError("fit_grid: waxes must hold one weight per axis coordinate")
    return npts, cat, wcat


def fit_grid(ndim, axes, values, xmin, xmax, nodes, xtrap=0.0, waxes=None, real32=False, ldv=None, ldcoef=None, coef=None):
    """The fit of samples on the tensor-product grid axes[0] x axes[1] x ... (splpak_fit_grid_*): what fit() returns for the
    listed product with the weights prod_d waxes[d][i_d], provided that fit has no constraint rows (xtrap == 0, or no
    data-sparse node: otherwise SplpakError from SPLPAK_E_UNSUPPORTED).  `axes` (and `waxes`, or None for all 1) are lists of
    `ndim` 1-D arrays; `values` has the shape evaluate_grid returns, (n_ndim, ..., n_1), or (nfields,) + that shape, or is
    flat with the fields `ldv` apart.  `coef`: an array to write into (fields `ldcoef` apart), else a new one.
    -> (coef of shape (ncol,) or (nfields, ncol) -- flat of nfields*ldcoef when ldcoef is given --, ierror, info (nfields, 10))."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    npts, cat, wcat = _grid_axes(axes, waxes, dt)
    nsamp = int(np.prod(npts)) if npts.size else 1
    values = np.ascontiguousarray(values, dtype=dt)
    if ldv is None:
        single = values.size == nsamp and values.ndim <= max(len(axes), 1)
        nfields = 1 if single else (values.size // nsamp if nsamp > 0 else 1)
        ldv_ = nsamp
    else:
        single = False
        ldv_ = int(ldv)
        nfields = max((values.size + ldv_ - nsamp) // ldv_, 1) if ldv_ > 0 else 1
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64))) if nodes.size else 0
    ldc = ncol if ldcoef is None else int(ldcoef)
    if coef is None:
        coef = np.zeros(max(nfields * ldc, 1), dtype=dt)
    info = np.zeros((nfields, 10))
    fn = lib().splpak_fit_grid_f32 if real32 else lib().splpak_fit_grid_f64
    rc = _check(fn(ndim, _p(npts, _lp), _p(cat, rp), _p(wcat, rp), nfields, _p(values, rp), ldv_, _p(xmin, rp),
                   _p(xmax, rp), _p(nodes, _ip), float(xtrap), _p(coef, rp), ldc, _p(info, _dp)))
    if ldcoef is None and coef.size == nfields * ncol:
        coef = coef[:ncol] if single else coef.reshape(nfields, ncol)
    return coef, rc, info


def fit_grid_dev(ndim, npts, axes, values, xmin, xmax, nodes, coef, xtrap=0.0, waxes=None, nfields=1, ldv=None, ldcoef=None,
                 stream=0):
    """fit_grid on torch device tensors: `axes` (and `waxes`, or None) hold the axes back to back, `values` the samples of
    field k from k*ldv on (default prod npts), `coef` receives its coefficients from k*ldcoef on (default ncol).  `stream`
    is synchronised (the axes come to the host; every refinement step).  float32 tensors take the REAL32 entry.
    -> (ierror, info (nfields, 10))."""
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    real32 = str(axes.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64)))
    info = np.zeros((int(nfields), 10))
    fn = lib().splpak_fit_grid_dev_f32 if real32 else lib().splpak_fit_grid_dev_f64
    rc = _check(fn(ndim, _p(npts, _lp), axes.data_ptr(), None if waxes is None else waxes.data_ptr(), int(nfields),
                   values.data_ptr(), int(np.prod(npts)) if ldv is None else int(ldv), _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip),
                   float(xtrap), coef.data_ptr(), ncol if ldcoef is None else int(ldcoef), _p(info, _dp), C.c_void_p(stream)))
    return rc, info


def debug_fit_grid_stage(stage, ndim, axes, data, xmin, xmax, nodes, waxes=None):
    """One stage of the grid fit alone (splpak_debug_fit_grid_stage_f64): stage 0 -> T[ncol], the spread of the samples
    `data`; stage 1 -> C[ncol] from `data` = T, the solves alone.  -> (array of ncol, ierror)."""
    npts, cat, wcat = _grid_axes(axes, waxes, np.float64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    out = np.zeros(int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64))))
    rc = _check(lib().splpak_debug_fit_grid_stage_f64(int(stage), ndim, _p(npts, _lp), _p(cat, _dp), _p(wcat, _dp),
                                                      _p(xmin, _dp), _p(xmax, _dp), _p(nodes, _ip), _p(data, _dp), _p(out, _dp)))
    return out, rc


def debug_fit_grid_stats():
    """Host counters of this thread's last fit_grid call: (slabs of a residual pass, doubles of residual scratch held, spread
    launches, solve launches, refinement steps of the last field, 0, 0, 0)."""
    v = np.zeros(8, dtype=np.int64)
    _check(lib().splpak_debug_fit_grid_stats(_p(v, _lp)))
    return tuple(int(t) for t in v)


def fit_grid_weighted(ndim, axes, values, weights, xmin, xmax, nodes, xtrap=0.0, real32=False, ldv=None, ldw=None, ldcoef=None,
                      coef=None):
    """fit_grid with a weight per sample (splpak_fit_grid_weighted_*): what fit() returns for the listed samples of non-zero
    weight, provided that fit has no constraint rows.  `values` as for fit_grid; `weights` has the shape of one field's values
    (one array for all fields, ldw = 0) or that of `values` (a weight array per field, `ldw` apart when flat; default prod
    npts).  A sample of weight 0 may hold NaN.  SplpakError from SPLPAK_E_BADARG for a negative or non-finite weight.
    -> (coef, ierror, info (nfields, 10)) as fit_grid."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    npts, cat = _axes_cat(axes, dt)
    nsamp = int(np.prod(npts)) if npts.size else 1
    values = np.ascontiguousarray(values, dtype=dt)
    weights = np.ascontiguousarray(weights, dtype=dt)
    if ldv is None:
        single = values.size == nsamp and values.ndim <= max(len(axes), 1)
        nfields = 1 if single else (values.size // nsamp if nsamp > 0 else 1)
        ldv_ = nsamp
    else:
        single = False
        ldv_ = int(ldv)
        nfields = max((values.size + ldv_ - nsamp) // ldv_, 1) if ldv_ > 0 else 1
    if ldw is None:
        if weights.size not in (nsamp, nfields * nsamp):
            raise SplpakError("fit_grid_weighted: weights must hold one weight per sample, for one field or for every field")
        ldw = 0 if weights.size == nsamp else nsamp
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64))) if nodes.size else 0
    ldc = ncol if ldcoef is None else int(ldcoef)
    if coef is None:
        coef = np.zeros(max(nfields * ldc, 1), dtype=dt)
    info = np.zeros((nfields, 10))
    fn = lib().splpak_fit_grid_weighted_f32 if real32 else lib().splpak_fit_grid_weighted_f64
    rc = _check(fn(ndim, _p(npts, _lp), _p(cat, rp), nfields, _p(values, rp), ldv_, _p(weights, rp), int(ldw), _p(xmin, rp),
                   _p(xmax, rp), _p(nodes, _ip), float(xtrap), _p(coef, rp), ldc, _p(info, _dp)))
    if ldcoef is None and coef.size == nfields * ncol:
        coef = coef[:ncol] if single else coef.reshape(nfields, ncol)
    return coef, rc, info


def fit_grid_weighted_dev(ndim, npts, axes, values, weights, xmin, xmax, nodes, coef, xtrap=0.0, nfields=1, ldv=None, ldw=0,
                          ldcoef=None, stream=0):
    """fit_grid_weighted on torch device tensors, as fit_grid_dev: `weights` in the layout of `values`, field k's from k*ldw
    on (0: one array for all fields).  -> (ierror, info (nfields, 10))."""
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    real32 = str(axes.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64)))
    info = np.zeros((int(nfields), 10))
    fn = lib().splpak_fit_grid_weighted_dev_f32 if real32 else lib().splpak_fit_grid_weighted_dev_f64
    rc = _check(fn(ndim, _p(npts, _lp), axes.data_ptr(), int(nfields), values.data_ptr(),
                   int(np.prod(npts)) if ldv is None else int(ldv), weights.data_ptr(), int(ldw), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), float(xtrap), coef.data_ptr(), ncol if ldcoef is None else int(ldcoef), _p(info, _dp),
                   C.c_void_p(stream)))
    return rc, info


def debug_fit_grid_weighted_stage(stage, ndim, axes, weights, data, xmin, xmax, nodes):
    """One stage of the weighted grid fit alone (splpak_debug_fit_grid_weighted_stage_f64): 0 -> A^T (w^2 o data), 1 -> N data,
    2 -> M^-1 data (arrays of ncol); 3 -> the D marginals of w^2, then diag(N) (sum npts + ncol; `data` is not read).
    -> (array, ierror)."""
    npts, cat = _axes_cat(axes, np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    data = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64)))
    out = np.zeros(ncol + (int(np.sum(npts)) if int(stage) == 3 else 0))
    rc = _check(lib().splpak_debug_fit_grid_weighted_stage_f64(int(stage), ndim, _p(npts, _lp), _p(cat, _dp), _p(weights, _dp),
                                                               _p(xmin, _dp), _p(xmax, _dp), _p(nodes, _ip), _p(data, _dp), _p(out, _dp)))
    return out, rc


def debug_fit_grid_weighted_stats():
    """Host counters of this thread's last fit_grid_weighted call: (slabs of an operator pass, doubles of slab scratch held,
    spread launches, axis-solve launches, refinement steps of the last field, its CG iterations over all solves, its CG
    solves, weight analyses of the call)."""
    v = np.zeros(8, dtype=np.int64)
    _check(lib().splpak_debug_fit_grid_weighted_stats(_p(v, _lp)))
    return tuple(int(t) for t in v)


def fit_many(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap=0.0, real32=False, ldcoef=None, coef=None, l1xdat=None):
    """Many small independent fits on one node grid in one launch (splpak_fit_many_*): problem k owns the points
    offsets[k] .. offsets[k+1]-1 of xdata (npoints, l1xdat), ydata and wdata (None: splcc); its coefficients go to row k of
    `coef` (nbatch, ldcoef), the layout evaluate_fields reads.  -> (coef, ierror, status (nbatch), info (nbatch, 10)); a
    problem without points has status 105 and its row of `coef` is left as it was."""
    coef, rc, status, info, _, _, _ = _fit_many_host("fit_many", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, real32, ldcoef,
                                                     coef, l1xdat)
    return coef, rc, status, info


def _fit_many_host(stem, ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, real32, ldcoef, coef, l1xdat, scalars=(), nclip=0,
                   wout=None, with_cov=False, ldcov=None, cov=None):
    """The host wrappers of the batch-fit family: the conversions and the outputs they share, then splpak_<stem>_f64 / _f32.
    A variant adds `scalars` (between xtrap and the outputs), with nclip > 0 the weights `wout` (before coef) and `clip`
    (nbatch, nclip) (last), with with_cov `cov` (nbatch, ldcov) after coef.
    -> (coef, ierror, status, info, wout, clip, cov), None for what the variant does not have."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    offsets, nbatch, xdata = _many_host(offsets, xdata, dt)
    ydata = np.ascontiguousarray(ydata, dtype=dt)
    if wdata is not None:
        wdata = np.ascontiguousarray(wdata, dtype=dt)
    if l1xdat is None:
        l1xdat = xdata.shape[1]
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    ncol = int(np.prod(np.maximum(nodes[:max(int(ndim), 0)].astype(np.int64), 1))) if nodes.size else 0
    ldc = ncol if ldcoef is None else int(ldcoef)
    n = max(nbatch, 1)
    if coef is None:
        coef = np.zeros((n, max(ldc, 1)), dtype=dt)
    status = np.full(n, -999, dtype=np.int32)
    info = np.zeros((n, 10))
    args = [ndim, nbatch, _p(offsets, _lp), _p(xdata, rp), int(l1xdat), _p(ydata, rp), _p(wdata, rp), _p(xmin, rp), _p(xmax, rp),
            _p(nodes, _ip), float(xtrap), *scalars]
    clip = None
    if nclip:
        if wout is None:
            wout = np.zeros(max(ydata.size, 1), dtype=dt)
        clip = np.zeros((n, nclip))
        args.append(_p(wout, rp))
    args += [_p(coef, rp), ldc]
    if with_cov:
        ldv = ncol * ((7 ** max(int(ndim), 0) + 1) // 2) if ldcov is None else int(ldcov)
        if cov is None:
            cov = np.zeros((n, max(ldv, 1)), dtype=dt)
        args += [_p(cov, rp), ldv]
    args += [_p(status, _ip), _p(info, _dp)]
    if nclip:
        args.append(_p(clip, _dp))
    rc = _check(getattr(lib(), f"splpak_{stem}_{'f32' if real32 else 'f64'}")(*args))
    return coef, rc, status, info, wout, clip, cov


def _fit_many_on_dev(stem, ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap, l1xdat, ldcoef, stream, scalars=(), nclip=0,
                     wout=None, cov=None, ldcov=None):
    """The _dev wrappers of the batch-fit family on torch device tensors, offsets on the host: splpak_<stem>_dev_f64 / _f32 by
    xdata's dtype.  `scalars`, `wout` with `clip` (nbatch, nclip), and `cov` with `ldcov` as _fit_many_host places them.
    -> (ierror, status, info, clip or None)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nbatch = offsets.size - 1
    real32 = str(xdata.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    ncol = int(np.prod(nodes[:max(int(ndim), 0)].astype(np.int64)))
    if l1xdat is None:
        l1xdat = xdata.shape[1] if xdata.dim() > 1 else 1
    n = max(nbatch, 1)
    status = np.full(n, -999, dtype=np.int32)
    info = np.zeros((n, 10))
    args = [ndim, nbatch, _p(offsets, _lp), xdata.data_ptr(), int(l1xdat), ydata.data_ptr(), None if wdata is None else wdata.data_ptr(),
            _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), float(xtrap), *scalars]
    clip = None
    if nclip:
        clip = np.zeros((n, nclip))
        args.append(wout.data_ptr())
    args += [coef.data_ptr(), ncol if ldcoef is None else int(ldcoef)]
    if cov is not None:
        if ldcov is None:
            ldcov = cov.stride(0) if cov.dim() > 1 else cov.shape[0]
        args += [cov.data_ptr(), int(ldcov)]
    args += [_p(status, _ip), _p(info, _dp)]
    if nclip:
        args.append(_p(clip, _dp))
    rc = _check(getattr(lib(), f"splpak_{stem}_dev_{'f32' if real32 else 'f64'}")(*args, C.c_void_p(stream)))
    return rc, status, info, clip


def fit_many_dev(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap=0.0, l1xdat=None, ldcoef=None, stream=0):
    """fit_many on torch device tensors: xdata, ydata, wdata (or None) and coef on the device, offsets on the host.
    -> (ierror, status (nbatch), info (nbatch, 10))."""
    return _fit_many_on_dev("fit_many", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap, l1xdat, ldcoef, stream)[:3]


def fit_many_clip(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap=0.0, klo=3.0, khi=3.0, maxpass=5, real32=False, ldcoef=None,
                  coef=None, l1xdat=None, wout=None):
    """Sigma-clipped batch fits in one launch (splpak_fit_many_clip_*): for every problem the loop fit_many -> residuals_many ->
    reject where t = w r lies beyond khi (above) or klo (below) times the rms of the counted t -> fit_many, until a pass rejects
    nothing or `maxpass` passes have run; bit for bit what that loop of the three entries gives.  Layouts as fit_many.
    -> (coef, wout, ierror, status (nbatch), info (nbatch, 10) of the last fit, clip (nbatch, 4) = (residual passes, points
    rejected, points counted by the last fit, S / cnt of the last pass)); wout (given, or zeros of ydata's length) holds the
    weights every problem ended with: 0 where a point was rejected."""
    coef, rc, status, info, wout, clip, _ = _fit_many_host("fit_many_clip", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, real32,
                                                           ldcoef, coef, l1xdat, scalars=(float(klo), float(khi), int(maxpass)), nclip=4,
                                                           wout=wout)
    return coef, wout, rc, status, info, clip


def fit_many_clip_dev(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, wout, xtrap=0.0, klo=3.0, khi=3.0, maxpass=5,
                      l1xdat=None, ldcoef=None, stream=0):
    """fit_many_clip on torch device tensors: xdata, ydata, wdata (or None), coef and wout on the device, offsets on the host.
    -> (ierror, status (nbatch), info (nbatch, 10), clip (nbatch, 4))."""
    return _fit_many_on_dev("fit_many_clip", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap, l1xdat, ldcoef, stream,
                            scalars=(float(klo), float(khi), int(maxpass)), nclip=4, wout=wout)


def fit_many_clip_mad(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap=0.0, klo=3.0, khi=3.0, maxpass=5, regrow=0, real32=False,
                      ldcoef=None, coef=None, l1xdat=None, wout=None):
    """Robustly clipped batch fits in one launch (splpak_fit_many_clip_mad_*): fit_many_clip's loop with the median of t = w0 r as
    the centre, 1.4826 MAD as the scale and, with regrow != 0, rejected points judged again in every pass against their original
    weight; bit for bit the loop fit_many -> residuals_many -> mad_many -> the rule -> fit_many.  Layouts as fit_many.
    -> (coef, wout, ierror, status (nbatch), info (nbatch, 10) of the last fit, clip (nbatch, 6) = (residual passes, points out
    at the end, points counted by the last fit, s and med of the last pass, points returned in total))."""
    coef, rc, status, info, wout, clip, _ = _fit_many_host("fit_many_clip_mad", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap,
                                                           real32, ldcoef, coef, l1xdat,
                                                           scalars=(float(klo), float(khi), int(maxpass), int(regrow)), nclip=6, wout=wout)
    return coef, wout, rc, status, info, clip


def fit_many_clip_mad_dev(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, wout, xtrap=0.0, klo=3.0, khi=3.0, maxpass=5,
                          regrow=0, l1xdat=None, ldcoef=None, stream=0):
    """fit_many_clip_mad on torch device tensors: xdata, ydata, wdata (or None), coef and wout on the device, offsets on the host.
    -> (ierror, status (nbatch), info (nbatch, 10), clip (nbatch, 6))."""
    return _fit_many_on_dev("fit_many_clip_mad", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap, l1xdat, ldcoef, stream,
                            scalars=(float(klo), float(khi), int(maxpass), int(regrow)), nclip=6, wout=wout)


def mad_many(offsets, values, wsel=None, real32=False):
    """The median and the MAD of every problem's segment of `values` in one launch (splpak_mad_many_*): problem k owns the global
    indices offsets[k] .. offsets[k+1]-1; a point is counted where wsel is not 0 (None: every point).  Exact order statistics,
    numpy.median's bits.  -> (stats (nbatch, 4) = (points counted, median, MAD, 0), ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nbatch = offsets.size - 1
    values = np.ascontiguousarray(values, dtype=dt)
    if wsel is not None:
        wsel = np.ascontiguousarray(wsel, dtype=dt)
    stats = np.full((max(nbatch, 1), 4), -999.0)
    rc = _check((lib().splpak_mad_many_f32 if real32 else lib().splpak_mad_many_f64)(nbatch, _p(offsets, _lp), _p(values, rp), _p(wsel, rp),
                                                                                  _p(stats, _dp)))
    return stats, rc


def mad_many_dev(offsets, values, wsel, stats, stream=0):
    """mad_many on torch device tensors (asynchronous on `stream`): values, wsel (or None) and stats (nbatch, 4) float64 on the
    device, offsets on the host.  float32 values take the REAL32 entry.  -> ierror."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    real32 = str(values.dtype).endswith("float32")
    fn = lib().splpak_mad_many_dev_f32 if real32 else lib().splpak_mad_many_dev_f64
    return _check(fn(offsets.size - 1, _p(offsets, _lp), values.data_ptr(), None if wsel is None else wsel.data_ptr(), stats.data_ptr(),
                     C.c_void_p(stream)))


def fit_many_cov_len(ndim, nodes) -> int:
    """Words of one problem's `cov` in fit_many_cov: ncol (7^ndim + 1) / 2 (host only; splpak_fit_many_cov_len); raises for a
    shape fit_many_lds_bytes rejects."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    return int(_check(lib().splpak_fit_many_cov_len(int(ndim), _p(nodes, _ip))))


def fit_many_cov(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap=0.0, real32=False, ldcoef=None, coef=None, l1xdat=None,
                 ldcov=None, cov=None):
    """fit_many with the covariance of the coefficients (splpak_fit_many_cov_*): beside `coef`, row k of `cov` (nbatch, ldcov)
    gets the half stencil of Z = (A^T W^2 A + C^T C)^-1 of problem k: cov[k, i * hst + code] = Z[i, i + o], hst = (7^ndim + 1) / 2,
    code = sum_d (o_d + 3) 7^d <= the centre, 0 where i + o is outside the grid -- the layout of Port.normal_equations' N.
    With wdata = 1 / sigma and no constraint rows Z is the covariance of the coefficients.
    -> (coef, cov, ierror, status (nbatch), info (nbatch, 10)); a problem of status 105 keeps its rows of coef and cov, one of
    status 107 has both zeroed."""
    coef, rc, status, info, _, _, cov = _fit_many_host("fit_many_cov", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, xtrap, real32,
                                                       ldcoef, coef, l1xdat, with_cov=True, ldcov=ldcov, cov=cov)
    return coef, cov, rc, status, info


def fit_many_cov_dev(ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, cov, xtrap=0.0, l1xdat=None, ldcoef=None, ldcov=None,
                     stream=0):
    """fit_many_cov on torch device tensors: xdata, ydata, wdata (or None), coef and cov on the device, offsets on the host.
    -> (ierror, status (nbatch), info (nbatch, 10))."""
    return _fit_many_on_dev("fit_many_cov", ndim, offsets, xdata, ydata, wdata, xmin, xmax, nodes, coef, xtrap, l1xdat, ldcoef, stream,
                            cov=cov, ldcov=ldcov)[:3]


def fit_many_lds_bytes(ndim, nodes) -> int:
    """LDS bytes a problem of this grid takes in fit_many (host only; splpak_fit_many_lds_bytes); raises for a shape the
    entry's ladder rejects."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    return int(_check(lib().splpak_fit_many_lds_bytes(int(ndim), _p(nodes, _ip))))


def debug_fit_many_stats():
    """Host counters of this thread's last fit_many call: (workgroups launched, LDS bytes per workgroup, launches, problems sent
    to the device, problems refused with 105, the largest number of refinement steps, device allocations (hipMalloc) the call
    made -- 0 for a fit_many_dev call whose per-thread scratch was large enough --, 0).  After a fit_many_clip call the same
    slots, the steps of the last fits, and in the last slot the largest number of fits any problem ran."""
    v = np.zeros(8, dtype=np.int64)
    _check(lib().splpak_debug_fit_many_stats(_p(v, _lp)))
    return tuple(int(t) for t in v)


def _many_host(offsets, x, dt):
    """(offsets as int64, nbatch, x as a (npoints, ld) array of dt) of a batch in fit_many's layout."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    x = np.ascontiguousarray(x, dtype=dt)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    return offsets, offsets.size - 1, x


def evaluate_many(ndim, offsets, xq, nderiv, coef, xmin, xmax, nodes, real32=False, ldxq=None, ldcoef=None, out=None):
    """A batch of small fits at each problem's own points in one launch (splpak_eval_many_*), the evaluation side of fit_many:
    problem k owns the queries offsets[k] .. offsets[k+1]-1 of xq (nqueries, ldxq) and has its coefficients in row k of `coef`
    (nbatch, ldcoef), where fit_many put them; one nderiv pattern (None: values).  -> (out, ierror): `out` (given, or zeros
    of xq's length) is written at the batch's indices only, each value with the bits of `evaluate` on that problem alone."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    offsets, nbatch, xq = _many_host(offsets, xq, dt)
    coef = np.ascontiguousarray(coef, dtype=dt)
    ldc = int(ldcoef) if ldcoef is not None else (coef.shape[1] if coef.ndim > 1 else coef.size)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    if out is None:
        out = np.zeros(max(xq.shape[0], int(offsets[-1]) if offsets.size else 0, 1), dtype=dt)
    rc = _check((lib().splpak_eval_many_f32 if real32 else lib().splpak_eval_many_f64)(
        ndim, nbatch, _p(offsets, _lp), _p(xq, rp), int(xq.shape[1] if ldxq is None else ldxq), _p(nd, _ip), _p(coef, rp), ldc,
        _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), _p(out, rp)))
    return out, rc


def evaluate_many_var(ndim, offsets, xq, nderiv, cov, xmin, xmax, nodes, real32=False, ldxq=None, ldcov=None, out=None):
    """The prediction variance of a batch of small fits at each problem's own points in one launch (splpak_eval_many_var_*):
    out[i] = a^T Z a, a the window row evaluate_many forms for query i with the same nderiv (the variance of that derivative),
    Z from row k of `cov` (nbatch, ldcov) as fit_many_cov wrote it.  The variance, not its root, not clamped.
    -> (out, ierror), `out` written at the batch's indices only."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    offsets, nbatch, xq = _many_host(offsets, xq, dt)
    cov = np.ascontiguousarray(cov, dtype=dt)
    ldv = int(ldcov) if ldcov is not None else (cov.shape[1] if cov.ndim > 1 else cov.size)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    if out is None:
        out = np.zeros(max(xq.shape[0], int(offsets[-1]) if offsets.size else 0, 1), dtype=dt)
    rc = _check((lib().splpak_eval_many_var_f32 if real32 else lib().splpak_eval_many_var_f64)(
        ndim, nbatch, _p(offsets, _lp), _p(xq, rp), int(xq.shape[1] if ldxq is None else ldxq), _p(nd, _ip), _p(cov, rp), ldv,
        _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), _p(out, rp)))
    return out, rc


def residuals_many(ndim, offsets, xdata, ydata, wdata, coef, xmin, xmax, nodes, real32=False, l1xdat=None, ldcoef=None,
                   want_resid=True, want_stats=True):
    """Residuals and per-problem statistics of a batch of small fits in one launch (splpak_residuals_many_*): the pass between two
    fit_many calls of a clipping loop.  Layouts as fit_many.  -> (resid or None, stats (nbatch, 4) or None, ierror); stats[k] =
    (points counted, sum (w r)^2, max |w r|, first local index of the max, -1 when nothing is counted).  resid is written at the
    batch's indices only (zeros elsewhere)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    offsets, nbatch, xdata = _many_host(offsets, xdata, dt)
    ydata = np.ascontiguousarray(ydata, dtype=dt)
    if wdata is not None:
        wdata = np.ascontiguousarray(wdata, dtype=dt)
    coef = np.ascontiguousarray(coef, dtype=dt)
    ldc = int(ldcoef) if ldcoef is not None else (coef.shape[1] if coef.ndim > 1 else coef.size)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    resid = np.zeros(max(ydata.size, 1), dtype=dt) if want_resid else None
    stats = np.full((max(nbatch, 1), 4), -999.0) if want_stats else None
    rc = _check((lib().splpak_residuals_many_f32 if real32 else lib().splpak_residuals_many_f64)(
        ndim, nbatch, _p(offsets, _lp), _p(xdata, rp), int(xdata.shape[1] if l1xdat is None else l1xdat), _p(ydata, rp), _p(wdata, rp),
        _p(coef, rp), ldc, _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), _p(resid, rp), _p(stats, _dp)))
    return resid, stats, rc


def debug_eval_many_stats():
    """Host counters of this thread's last evaluate_many / residuals_many call: (workgroups launched, launches, queries / points
    sent, problems, queries one sweep of an evaluate_many launch covers (residuals_many: 0), 1 evaluate_many / 2 residuals_many /
    3 evaluate_many_var / 4 mad_many, 0, 0)."""
    v = np.zeros(8, dtype=np.int64)
    _check(lib().splpak_debug_eval_many_stats(_p(v, _lp)))
    return tuple(int(t) for t in v)


def evaluate_fields(ndim, xq, nderiv, coefs, xmin, xmax, nodes, real32=False, ldcoef=None, ldout=None):
    """Several coefficient sets at the same points under one nderiv pattern (splpak_eval_fields_*): `coefs` is (nfields, ncol)
    or (ncol,), field k in row k.  ldcoef / ldout (>= ncol / nq) are the distances the library is given between the fields'
    coefficients / results (default: packed); the rows are staged with that padding.  -> (values (nfields, nq), ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    xq = np.ascontiguousarray(xq, dtype=dt)
    if xq.ndim == 1:
        xq = xq.reshape(-1, 1)
    nq, ldx = xq.shape
    coefs = np.atleast_2d(np.asarray(coefs, dtype=dt))
    nfields, ncol = coefs.shape
    ldc = int(ncol if ldcoef is None else ldcoef)
    ldo = int(nq if ldout is None else ldout)
    cpad = np.zeros((max(nfields, 1), max(ldc, ncol, 1)), dtype=dt)
    cpad[:nfields, :ncol] = coefs
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    out = np.zeros((max(nfields, 1), max(ldo, nq, 1)), dtype=dt)
    fn = lib().splpak_eval_fields_f32 if real32 else lib().splpak_eval_fields_f64
    rc = _check(fn(ndim, nq, _p(xq, rp), ldx, _p(nd, _ip), int(nfields), _p(cpad, rp), ldc, _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp), ldo))
    return out[:nfields, :nq], rc


def debug_eval_fields_stats():
    """(route, place passes, evaluation kernels) of this thread's last fields call -- route: 0 none yet, 1 the direct fields
    kernel, 2 the shared sort, 3 one single-field evaluation per field.  Host-side counters: nothing is waited for."""
    v = np.zeros(3, dtype=np.int64)
    _check(lib().splpak_debug_eval_fields_stats(_p(v, _lp)))
    return int(v[0]), int(v[1]), int(v[2])


def derivs_nout(ndim, order):
    return 1 + ndim + (ndim * (ndim + 1) // 2 if order == 2 else 0)


def evaluate_derivs(ndim, xq, order, coef, xmin, xmax, nodes, real32=False):
    """Value, gradient (order 1) and Hessian upper triangle (order 2) per query -> (array (nq, nout), ierror)."""
    dt = np.float32 if real32 else np.float64
    rp = _fp if real32 else _dp
    xq = np.ascontiguousarray(xq, dtype=dt)
    if xq.ndim == 1:
        xq = xq.reshape(-1, 1)
    nq, ldx = xq.shape
    coef = np.ascontiguousarray(coef, dtype=dt)
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, dt)
    nout = derivs_nout(max(ndim, 1), order) if order in (1, 2) else 1
    out = np.zeros((nq, nout), dtype=dt)
    fn = lib().splpak_eval_derivs_f32 if real32 else lib().splpak_eval_derivs_f64
    rc = _check(fn(ndim, nq, _p(xq, rp), ldx, int(order), _p(coef, rp), _p(xmin, rp), _p(xmax, rp),
                   _p(nodes, _ip), _p(out, rp), nout))
    return out, rc


def evaluate_derivs_dev(ndim, xq, order, coef, xmin, xmax, nodes, out, stream=0):
    """Same on torch device tensors; `out` is (nq, >= nout) float64."""
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    nq, ldx = xq.shape
    return _check(lib().splpak_eval_derivs_dev_f64(ndim, int(nq), xq.data_ptr(), int(ldx), int(order),
                                                   coef.data_ptr(), _p(xmin, _dp), _p(xmax, _dp), _p(nodes, _ip),
                                                   out.data_ptr(), int(out.shape[1]), C.c_void_p(stream)))


# ---------------------------------------------------------------------------
# resident-data API (torch tensors own the device memory)
# ---------------------------------------------------------------------------

class Plan:
    """A fit plan for one node grid on the current torch CUDA(HIP) device."""

    def __init__(self, ndim, nodes, xmin, xmax, xtrap, max_ndata, comm=None):
        self._L = lib()
        self.ndim = ndim
        self.xmin, self.xmax, self.nodes = _grid(ndim, xmin, xmax, nodes)
        self.ncol = int(np.prod(self.nodes.astype(np.int64)))
        self.comm_len = int(self._L.splpak_plan_comm_len(ndim, _p(self.nodes, _ip)))
        self.comm = comm          # optional torch tensor (float64, device) of >= comm_len elements
        self._cb = None
        h = C.c_void_p()
        comm_ptr = None if comm is None else C.c_void_p(comm.data_ptr())
        comm_n = 0 if comm is None else comm.numel()
        rc = self._L.splpak_plan_create(ndim, _p(self.nodes, _ip), _p(self.xmin, _dp),
                                        _p(self.xmax, _dp), float(xtrap), int(max_ndata), comm_ptr,
                                        comm_n, C.byref(h))
        if rc != 0:
            if rc < 0:
                _check(rc)
            raise SplpakError(f"plan rejected with ierror {rc}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.splpak_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_refine(self, max_steps, tol):
        self._L.splpak_plan_set_refine(self._h, int(max_steps), float(tol))

    def set_allreduce(self, fn, rank, world, any_pointer=None, stream_ordered=False):
        """fn(offset_elems, count) must sum-all-reduce self.comm[offset:offset+count] in place.  A hook that also takes a
        third argument -- fn(-1, count, view) with `view` a device tensor over the library's own memory -- declares
        SPLPAK_AR_ANY_POINTER (include/splpak_hip.h): the nested-dissection factorisation of the sharded fit is then
        distributed by subtrees and the fronts they report into arrive that way.  A two-argument hook (rounds 1-2) keeps
        the replicated factorisation.  `any_pointer` overrides the detection.  `stream_ordered`: the hook only ENQUEUES its
        work on the current stream (= the library's, made current for the call) -- SPLPAK_AR_STREAM_ORDERED: the library then does
        not synchronise the stream before and after the call."""
        if any_pointer is None:
            import inspect
            try:
                params = list(inspect.signature(fn).parameters.values())
                any_pointer = len(params) >= 3 or any(q.kind == q.VAR_POSITIONAL for q in params)
            except (TypeError, ValueError):
                any_pointer = False
        base = self.comm.data_ptr()
        ncomm = self.comm.numel()
        device = self.comm.device

        class _Raw:            # a device buffer of the library as a CUDA-array-interface object
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}

        def _call(ptr, count):
            off = (int(ptr) - base) // 8
            if 0 <= off and off + int(count) <= ncomm and (int(ptr) - base) % 8 == 0:
                fn(off, int(count))
            else:
                import torch
                fn(-1, int(count), torch.as_tensor(_Raw(ptr, count), device=device))

        def _cb(ptr, count, stream, user):
            # The C ABI's contract: the reduction is ordered ON `stream` (the stream the fit was
            # enqueued on).  torch.distributed orders a collective against torch's CURRENT stream, so
            # make the library's stream current for the duration of the call.
            try:
                import torch
                if torch.cuda.is_available():
                    with torch.cuda.stream(torch.cuda.ExternalStream(int(stream or 0))):
                        _call(ptr, count)
                else:
                    _call(ptr, count)
                return 0
            except Exception as exc:  # pragma: no cover - surfaced as SPLPAK_E_COMM
                print("all-reduce callback failed:", exc, flush=True)
                return 1

        self._cb = ALLREDUCE_FN(_cb)
        _check(self._L.splpak_plan_set_allreduce_ex(self._h, self._cb, None, int(rank), int(world),
                                                    (AR_ANY_POINTER if any_pointer else 0) | (AR_STREAM_ORDERED if stream_ordered else 0)))

    def device_bytes(self):
        return int(self._L.splpak_plan_device_bytes(self._h))

    def set_option(self, name, value):
        """A per-fit option of this plan (value as text, None removes it); options that shape the plan raise: set_default_option."""
        return _check(self._L.splpak_plan_set_option(self._h, name.encode(), None if value is None else str(value).encode()))

    def get_option(self, name):
        buf = C.create_string_buffer(256)
        return buf.value.decode() if _check(self._L.splpak_plan_get_option(self._h, name.encode(), buf, 256)) == 1 else None

    def pcg_stats(self):
        """Iterative solve of the last fit: dict(iterations, solves, last_iterations, last_residual, rho, lam); zeros without it."""
        out = np.zeros(6)
        self._L.splpak_plan_pcg_stats(self._h, _p(out, _dp))
        return dict(iterations=int(out[0]), solves=int(out[1]), last_iterations=int(out[2]), last_residual=float(out[3]),
                    rho=float(out[4]), lam=float(out[5]))

    def set_rccl(self, comm, rank, world):
        """The library's own RCCL hook (no Python in the reductions): `comm` is an ncclComm_t as an integer / c_void_p."""
        _check(self._L.splpak_plan_set_rccl(self._h, C.c_void_p(comm if isinstance(comm, int) else comm.value), int(rank), int(world)))

    def factorisation(self):
        """-> (code, description): 0/1 band Cholesky, 2 two-ended band, 3 distributed band, 4 nested dissection."""
        buf = C.create_string_buffer(640)
        code = self._L.splpak_plan_factorisation(self._h, buf, 640)
        return int(code), buf.value.decode()

    def enable_kernel_timing(self, on=True):
        self._L.splpak_plan_enable_kernel_timing(self._h, 1 if on else 0)

    def kernel_timing(self):
        out = np.zeros(7)
        self._L.splpak_plan_kernel_timing(self._h, _p(out, _dp))
        return dict(syrk_launches=out[0], syrk_ms=out[1], syrk_flop=out[2], factor_ms=out[3], total_flop=out[4],
                    bulk_launches=out[5], bulk_flop=out[6])

    def stage_timing(self):
        out = np.zeros(6)
        self._L.splpak_plan_stage_timing(self._h, _p(out, _dp))
        return dict(bin_ms=out[0], gram_ms=out[1], constraints_ms=out[2], expand_ms=out[3], residual_pass_ms=out[4], solve_ms=out[5])

    def fit(self, xdata, ydata, wdata, coef, stream=0):
        """All arguments are torch float64 device tensors; xdata is (ndata, l1xdat) row-major
        (= the reference's column-major xdata(l1xdat, ndata)).  Returns (ierror, info)."""
        info = np.zeros(10)
        ndata, l1 = xdata.shape
        rc = self._L.splpak_plan_fit_dev(self._h, xdata.data_ptr(), int(l1), ydata.data_ptr(),
                                         None if wdata is None else wdata.data_ptr(), int(ndata),
                                         coef.data_ptr(), C.c_void_p(stream), _p(info, _dp))
        return _check(rc), info

    def refit(self, ydata, coef, stream=0):
        """New values on the points of this plan's last fit (splpak_plan_refit_dev).  ydata: (nfields, ndata) or (ndata,) torch
        float64 device tensor, field k in row k (row stride >= ndata, unit stride inside a row), in that fit's point order;
        coef: (nfields, >= ncol) or (ncol,) likewise.  Returns (ierror, info) with info of shape (nfields, 10) -- (10,) for a 1-D
        ydata.  Raises SplpakError when there is nothing to refit."""
        single = ydata.dim() == 1
        nfields = 1 if single else int(ydata.shape[0])
        ldy = int(ydata.shape[0]) if single else int(ydata.stride(0))
        ldc = int(coef.shape[0]) if coef.dim() == 1 else int(coef.stride(0))
        if any(t.shape[-1] > 1 and t.stride(-1) != 1 for t in (ydata, coef)):
            raise SplpakError("refit: the values of a field, and its coefficients, must be contiguous")
        if (coef.dim() == 1) != single or (not single and int(coef.shape[0]) != nfields):
            raise SplpakError("refit: ydata and coef must name the same number of fields")
        info = np.zeros((max(nfields, 1), 10))
        rc = self._L.splpak_plan_refit_dev(self._h, nfields, ydata.data_ptr(), ldy, coef.data_ptr(), ldc,
                                           C.c_void_p(stream), _p(info, _dp))
        return _check(rc), (info[0] if single else info)

    def refit_stats(self):
        """The last refit of this plan (splpak_debug_plan_refit_stats) -> [route (0 none yet, 1 field by field, 2 batched sweeps),
        tree solves launched, right-hand sides they carried, fields run again field by field]."""
        out = (C.c_int64 * 4)()
        _check(self._L.splpak_debug_plan_refit_stats(self._h, out))
        return [int(v) for v in out]

    def hist_ptr(self):
        return self._L.splpak_plan_hist_dev(self._h)

    def histogram(self):
        """The histogram of the last fit (splpak_plan_hist_dev) copied to the host, (ncol,) as the device holds it; waits for
        the device."""
        import torch

        class _Raw:
            __cuda_array_interface__ = {"shape": (self.ncol,), "typestr": "<f8", "data": (int(self.hist_ptr()), False), "version": 2}

        torch.cuda.synchronize()
        return torch.as_tensor(_Raw(), device="cuda").cpu().numpy().copy()

    def normal_equations(self):
        """What the last fit assembled (diagnostics) -> (N, rhs): N the half stencil (ncol, (7^ndim + 1) // 2) in the caller's
        column numbering (include/splpak_hip.h splpak_debug_plan_normal_equations)."""
        hst = (7 ** self.ndim + 1) // 2
        N = np.zeros((self.ncol, hst))
        rhs = np.zeros(self.ncol)
        _check(self._L.splpak_debug_plan_normal_equations(self._h, _p(N, _dp), _p(rhs, _dp)))
        return N, rhs

    def gram_shape(self):
        """How the Gram pass of the last assembly was launched (diagnostics, splpak_debug_plan_gram_shape) -> dict(slabs, rows: hyper-rows
        of cells per slab, cells, run: of every slab but the last, last_cells, last_run); run 0: a cell kernel without runs."""
        out = np.zeros(6, dtype=np.int32)
        _check(self._L.splpak_debug_plan_gram_shape(self._h, _p(out, _ip)))
        return dict(zip(("slabs", "rows", "cells", "run", "last_cells", "last_run"), (int(v) for v in out)))

    def debug_solve(self, N, b):
        """Solve N x = b once with the plan's own factorisation, no refinement (diagnostics) -> (x, ierror, minpiv);
        ierror 0 or 107."""
        N = np.ascontiguousarray(N, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert N.shape == (self.ncol, (7 ** self.ndim + 1) // 2) and b.shape == (self.ncol,)
        x = np.zeros(self.ncol)
        mp = C.c_double(0.0)
        rc = _check(self._L.splpak_debug_plan_solve(self._h, _p(N, _dp), _p(b, _dp), _p(x, _dp), C.byref(mp)))
        return x, rc, mp.value

    def rows_gradient(self, coef, which=0):
        """The rows pass of the last fit at `coef` (diagnostics, splpak_debug_plan_rows_gradient) -> (rho, den, ssq); which: 0 the
        refinement's pass, 1 the fit's closing diagnostics pass (the only one that fills den and ssq), 2 the operator form y = 0."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        assert coef.shape == (self.ncol,)
        rho, den = np.zeros(self.ncol), np.zeros(self.ncol)
        ssq = C.c_double(0.0)
        _check(self._L.splpak_debug_plan_rows_gradient(self._h, _p(coef, _dp), int(which), _p(rho, _dp), _p(den, _dp), C.byref(ssq)))
        return rho, den, ssq.value

    def precondition(self, r, part=0):
        """z = M^-1 r with the preconditioner of the last fit (diagnostics); part: 0 whole, 1 separable part, 2 boxes."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape == (self.ncol,)
        z = np.zeros(self.ncol)
        _check(self._L.splpak_debug_plan_precondition(self._h, int(part), _p(r, _dp), _p(z, _dp)))
        return z

    def pcg_tables(self):
        """-> ([V_k], [VT_k], dinv): per dimension of the caller's order the (n_k, n_k) matrices of the separable part, and the
        reciprocal diagonal in the eigenbasis (ncol, caller's column order) as the last fit prepared it."""
        Vs, VTs = [], []
        for d in range(self.ndim):
            n = C.c_int32(0)
            _check(self._L.splpak_debug_plan_pcg_tables(self._h, d, None, None, C.byref(n)))
            V, VT = np.zeros((n.value, n.value)), np.zeros((n.value, n.value))
            _check(self._L.splpak_debug_plan_pcg_tables(self._h, d, _p(V, _dp), _p(VT, _dp), C.byref(n)))
            Vs.append(V)
            VTs.append(VT)
        dinv = np.zeros(self.ncol)
        _check(self._L.splpak_debug_plan_pcg_diagonal(self._h, _p(dinv, _dp)))
        return Vs, VTs, dinv


def evaluate_dev(ndim, xq, nderiv, coef, xmin, xmax, nodes, out, stream=0):
    """Batched evaluation on torch device tensors (asynchronous on `stream`); float32 tensors take the REAL32 entry."""
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    nq, ldx = xq.shape
    if str(xq.dtype).endswith("float32"):
        xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32)
        return _check(lib().splpak_eval_dev_f32(ndim, int(nq), xq.data_ptr(), int(ldx), _p(nd, _ip),
                                                coef.data_ptr(), _p(xmin, _fp), _p(xmax, _fp),
                                                _p(nodes, _ip), out.data_ptr(), C.c_void_p(stream)))
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    return _check(lib().splpak_eval_dev_f64(ndim, int(nq), xq.data_ptr(), int(ldx), _p(nd, _ip),
                                            coef.data_ptr(), _p(xmin, _dp), _p(xmax, _dp),
                                            _p(nodes, _ip), out.data_ptr(), C.c_void_p(stream)))


def evaluate_fields_dev(ndim, xq, nderiv, coef, xmin, xmax, nodes, out, stream=0):
    """Several coefficient sets at the same points on torch device tensors (asynchronous on `stream`): fields are rows --
    coef (nfields, >= ncol) or (ncol,), out (nfields, >= nq) or (nq,), unit stride inside a row; the row strides are passed as
    ldcoef / ldout, so the tensor Plan.refit filled can be given as it is.  float32 tensors take the REAL32 entry."""
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    nq, ldx = xq.shape
    nfields = 1 if coef.dim() == 1 else int(coef.shape[0])
    ldc = int(coef.shape[0]) if coef.dim() == 1 else int(coef.stride(0))
    ldo = int(out.shape[0]) if out.dim() == 1 else int(out.stride(0))
    if any(t.shape[-1] > 1 and t.stride(-1) != 1 for t in (coef, out)):
        raise SplpakError("evaluate_fields_dev: the coefficients of a field, and its results, must be contiguous")
    if (out.dim() == 1) != (coef.dim() == 1) or (out.dim() > 1 and int(out.shape[0]) != nfields):
        raise SplpakError("evaluate_fields_dev: coef and out must name the same number of fields")
    if int(out.shape[-1]) < int(nq):
        raise SplpakError("evaluate_fields_dev: out has fewer entries per field than there are queries")
    real32 = str(xq.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    fn = lib().splpak_eval_fields_dev_f32 if real32 else lib().splpak_eval_fields_dev_f64
    rp = _fp if real32 else _dp
    return _check(fn(ndim, int(nq), xq.data_ptr(), int(ldx), _p(nd, _ip), nfields, coef.data_ptr(), ldc, _p(xmin, rp), _p(xmax, rp),
                     _p(nodes, _ip), out.data_ptr(), ldo, C.c_void_p(stream)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def evaluate_many_dev(ndim, offsets, xq, nderiv, coef, xmin, xmax, nodes, out, ldxq=None, ldcoef=None, stream=0):
    """evaluate_many on torch device tensors (asynchronous on `stream`): xq (nqueries, ldxq), coef (nbatch, ldcoef) and out on the
    device, offsets and nderiv on the host.  float32 tensors take the REAL32 entry.  -> ierror."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    real32 = str(xq.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    if ldxq is None:
        ldxq = xq.shape[1] if xq.dim() > 1 else 1
    if ldcoef is None:
        ldcoef = coef.stride(0) if coef.dim() > 1 else coef.shape[0]
    fn = lib().splpak_eval_many_dev_f32 if real32 else lib().splpak_eval_many_dev_f64
    return _check(fn(ndim, offsets.size - 1, _p(offsets, _lp), xq.data_ptr(), int(ldxq), _p(nd, _ip), coef.data_ptr(), int(ldcoef),
                     _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), out.data_ptr(), C.c_void_p(stream)))


def evaluate_many_var_dev(ndim, offsets, xq, nderiv, cov, xmin, xmax, nodes, out, ldxq=None, ldcov=None, stream=0):
    """evaluate_many_var on torch device tensors (asynchronous on `stream`): xq (nqueries, ldxq), cov (nbatch, ldcov) and out on
    the device, offsets and nderiv on the host.  float32 tensors take the REAL32 entry.  -> ierror."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    real32 = str(xq.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    if ldxq is None:
        ldxq = xq.shape[1] if xq.dim() > 1 else 1
    if ldcov is None:
        ldcov = cov.stride(0) if cov.dim() > 1 else cov.shape[0]
    fn = lib().splpak_eval_many_var_dev_f32 if real32 else lib().splpak_eval_many_var_dev_f64
    return _check(fn(ndim, offsets.size - 1, _p(offsets, _lp), xq.data_ptr(), int(ldxq), _p(nd, _ip), cov.data_ptr(), int(ldcov),
                     _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), out.data_ptr(), C.c_void_p(stream)))


def residuals_many_dev(ndim, offsets, xdata, ydata, wdata, coef, xmin, xmax, nodes, resid, stats, l1xdat=None, ldcoef=None, stream=0):
    """residuals_many on torch device tensors (asynchronous on `stream`): xdata, ydata, wdata (or None), coef, resid (or None)
    and stats (nbatch, 4) float64 (or None) on the device, offsets on the host.  -> ierror."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    real32 = str(xdata.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    rp = _fp if real32 else _dp
    if l1xdat is None:
        l1xdat = xdata.shape[1] if xdata.dim() > 1 else 1
    if ldcoef is None:
        ldcoef = coef.stride(0) if coef.dim() > 1 else coef.shape[0]
    fn = lib().splpak_residuals_many_dev_f32 if real32 else lib().splpak_residuals_many_dev_f64
    return _check(fn(ndim, offsets.size - 1, _p(offsets, _lp), xdata.data_ptr(), int(l1xdat), ydata.data_ptr(), _ptr(wdata),
                     coef.data_ptr(), int(ldcoef), _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip), _ptr(resid), _ptr(stats),
                     C.c_void_p(stream)))


def evaluate_grid_dev(ndim, npts, axes, nderiv, coef, xmin, xmax, nodes, out, stream=0):
    """Grid evaluation on torch device tensors (asynchronous on `stream`): `axes` holds the npts[0] coordinates of dimension 1,
    then the npts[1] of dimension 2, ...; `out` has prod(npts) entries, dimension 1 fastest (a C-ordered tensor of shape
    npts[::-1]).  float32 tensors take the REAL32 entry."""
    nd = None if nderiv is None else np.ascontiguousarray(nderiv, dtype=np.int32)
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    if str(axes.dtype).endswith("float32"):
        xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32)
        return _check(lib().splpak_eval_grid_dev_f32(ndim, _p(npts, _lp), axes.data_ptr(), _p(nd, _ip), coef.data_ptr(),
                                                     _p(xmin, _fp), _p(xmax, _fp), _p(nodes, _ip), out.data_ptr(),
                                                     C.c_void_p(stream)))
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes)
    return _check(lib().splpak_eval_grid_dev_f64(ndim, _p(npts, _lp), axes.data_ptr(), _p(nd, _ip), coef.data_ptr(),
                                                 _p(xmin, _dp), _p(xmax, _dp), _p(nodes, _ip), out.data_ptr(),
                                                 C.c_void_p(stream)))


def integrate_grid_dev(ndim, ncell, mode, axes, coef, xmin, xmax, nodes, out, stream=0):
    """integrate_grid on torch device tensors: `axes` holds the axes back to back (ncell[d] + 1 edges of an integrated
    dimension, ncell[d] coordinates of an evaluated one), `out` has prod(ncell) entries, dimension 1 fastest.  `stream` is
    synchronised once (the piece counts come back to the host); the rest is queued on it.  float32 tensors take the REAL32 entry."""
    md = None if mode is None else np.ascontiguousarray(mode, dtype=np.int32)
    ncell = np.ascontiguousarray(ncell, dtype=np.int64)
    real32 = str(axes.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    fn = lib().splpak_integrate_grid_dev_f32 if real32 else lib().splpak_integrate_grid_dev_f64
    rp = _fp if real32 else _dp
    return _check(fn(ndim, _p(ncell, _lp), _p(md, _ip), axes.data_ptr(), coef.data_ptr(), _p(xmin, rp), _p(xmax, rp),
                     _p(nodes, _ip), out.data_ptr(), C.c_void_p(stream)))


def evaluate_grid_derivs_dev(ndim, npts, axes, order, coef, xmin, xmax, nodes, out, stream=0):
    """Value, gradient and (order 2) Hessian planes on torch device tensors (asynchronous on `stream`): `axes` as for
    evaluate_grid_dev; `out` is a 2-D tensor (nplanes, >= prod(npts)) with unit stride inside a row, its row stride is passed
    as ldout.  float32 tensors take the REAL32 entry."""
    npts = np.ascontiguousarray(npts, dtype=np.int64)
    if out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1):
        raise SplpakError("evaluate_grid_derivs_dev: out must be 2-D (planes, points) with contiguous planes")
    if order in (1, 2) and int(out.shape[0]) < derivs_nout(max(int(ndim), 0), order):
        raise SplpakError("evaluate_grid_derivs_dev: out has fewer rows than there are planes")
    ldo = int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1])
    real32 = str(axes.dtype).endswith("float32")
    xmin, xmax, nodes = _grid(ndim, xmin, xmax, nodes, np.float32 if real32 else np.float64)
    fn = lib().splpak_eval_grid_derivs_dev_f32 if real32 else lib().splpak_eval_grid_derivs_dev_f64
    rp = _fp if real32 else _dp
    return _check(fn(ndim, _p(npts, _lp), axes.data_ptr(), int(order), coef.data_ptr(), _p(xmin, rp), _p(xmax, rp), _p(nodes, _ip),
                     out.data_ptr(), ldo, C.c_void_p(stream)))


EVAL_AUTO, EVAL_DIRECT, EVAL_BINNED = 0, 1, 2


def set_eval_mode(mode=EVAL_AUTO, chunk=0):
    """Evaluation strategy of this thread (bit-identical results): auto / direct gathers / LDS-binned."""
    return _check(lib().splpak_set_eval_mode(int(mode), int(chunk)))


def synth_points_dev(ndim, first_point, ndata, xdata, ydata, wdata, stream=0):
    return _check(lib().splpak_synth_points_f64(ndim, int(first_point), int(ndata),
                                                None if xdata is None else xdata.data_ptr(),
                                                None if ydata is None else ydata.data_ptr(),
                                                None if wdata is None else wdata.data_ptr(),
                                                C.c_void_p(stream)))


def synth_queries_dev(ndim, ndata_before, first_query, nq, xq, stream=0):
    return _check(lib().splpak_synth_queries_f64(ndim, int(ndata_before), int(first_query), int(nq),
                                                 xq.data_ptr(), C.c_void_p(stream)))


def rccl_comm_create_from_file(path, rank, world, timeout_s=60.0, job=None):
    """ncclComm_t (as an int) made by the library: rank 0 draws the id and publishes it through `path` together with the
    job's tag (`job`: any string the ranks of ONE run share; None = SPLPAK_RCCL_JOB or what the launcher exports), the others
    wait for a file of THEIR job -- a file left by another run is ignored (include/splpak_hip.h)."""
    comm = C.c_void_p()
    rc = lib().splpak_rccl_comm_create_from_file_ex(str(path).encode(), None if job is None else str(job).encode(), int(rank), int(world),
                                                    float(timeout_s), C.byref(comm))
    if rc != 0:
        raise SplpakError(f"splpak_rccl_comm_create_from_file: {rc}: {last_error()}")
    return comm.value


def rccl_unique_id():
    """128-byte ncclUniqueId drawn by the library's RCCL (rank 0; hand it to the other ranks by any means)."""
    buf = C.create_string_buffer(128)
    rc = lib().splpak_rccl_unique_id(buf)
    if rc != 0:
        raise SplpakError(f"splpak_rccl_unique_id: {rc}: {last_error()}")
    return buf.raw


def rccl_comm_create(id128, rank, world):
    """ncclComm_t (as an int) on the CURRENT device from an id all ranks share."""
    comm = C.c_void_p()
    rc = lib().splpak_rccl_comm_create(bytes(id128), int(rank), int(world), C.byref(comm))
    if rc != 0:
        raise SplpakError(f"splpak_rccl_comm_create: {rc}: {last_error()}")
    return comm.value


def rccl_comm_destroy(comm):
    lib().splpak_rccl_comm_destroy(C.c_void_p(comm))


ND_TREE_FIELDS = ("fronts", "depth", "factor_bytes", "arena_bytes", "schur_bytes_per_fit", "flop", "flop_exact",
                  "max_separator", "max_border", "diag_blocks", "vec_len", "own_rows", "border_rows", "inverse_bytes")


def debug_nd_tree(nodes, split_min=0, check=True):
    """Host-only: size of the nested-dissection elimination tree the fit uses for large 3-D / 4-D grids
    (csrc/ndtree.hpp), optionally with its invariants verified.  -> dict (ND_TREE_FIELDS)."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    out = np.zeros(16)
    rc = _check(lib().splpak_debug_nd_tree(len(nodes), _p(nodes, _ip), int(split_min), 1 if check else 0, _p(out, _dp)))
    if rc != 0:
        raise SplpakError(f"grid rejected: {rc}")
    return dict(zip(ND_TREE_FIELDS, out.tolist()))


def debug_nd_schedule(nodes, cut=0, packed=True, split_min=0):
    """Host-only: the elimination schedule of the nested-dissection factorisation for a given cut depth (csrc/ndtree.hpp
    NdSchedule), its invariants verified.  -> dict(stages, arena_bytes, schur_bytes_per_fit, factor_bytes, cut, depth)."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    out = np.zeros(8)
    rc = _check(lib().splpak_debug_nd_schedule(len(nodes), _p(nodes, _ip), int(split_min), int(cut), 1 if packed else 0, _p(out, _dp)))
    if rc != 0:
        raise SplpakError(f"schedule rejected: {rc}: {last_error()}")
    return dict(stages=int(out[0]), arena_bytes=out[1], schur_bytes_per_fit=out[2], factor_bytes=out[3], cut=int(out[4]), depth=int(out[5]))


ND_RANK_FIELDS = ("bytes", "panel_bytes", "schur_bytes", "top_bytes", "inverse_bytes", "other_bytes", "flop_subtrees", "flop_top")


def debug_nd_partition(nodes, ngpus, chunk=0, split_min=0):
    """Host-only: how the one-process multi-GPU fit distributes the nested-dissection factorisation of a grid over
    `ngpus` GPUs (csrc/ndtree.hpp NdPartition).  -> (list of per-rank dicts (ND_RANK_FIELDS), summary dict)."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    per = np.zeros(8 * int(ngpus))
    out = np.zeros(8)
    rc = _check(lib().splpak_debug_nd_partition(len(nodes), _p(nodes, _ip), int(split_min), int(ngpus), int(chunk), _p(per, _dp), _p(out, _dp)))
    if rc != 0:
        raise SplpakError(f"grid rejected: {rc}")
    ranks = [dict(zip(ND_RANK_FIELDS, per[8 * r:8 * r + 8].tolist())) for r in range(int(ngpus))]
    summ = dict(dcut=int(out[0]), top_fronts=int(out[1]), top_steps=int(out[2]), max_panel_bytes=out[3], normal_eq_bytes=out[4],
                fronts=int(out[5]), depth=int(out[6]), flop=out[7])
    return ranks, summ


def debug_nd_fronts(nodes, split_min=0):
    """Host-only: the fronts of the nested-dissection elimination tree (postorder, root last) -> dict(depth, parent, w, h: per
    front; front_of, pos: per node in the caller's column numbering -- owning front and elimination position)."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    L = lib()
    nf = np.zeros(1, dtype=np.int32)
    rc = _check(L.splpak_debug_nd_fronts(len(nodes), _p(nodes, _ip), int(split_min), _p(nf, _ip), 0, None, None, None, None, None, None))
    if rc != 0:
        raise SplpakError(f"grid rejected: {rc}")
    n = int(nf[0])
    out = {k: np.zeros(n, dtype=np.int32) for k in ("depth", "parent", "w", "h")}
    ncol = int(np.prod(nodes.astype(np.int64)))
    out["front_of"] = np.zeros(ncol, dtype=np.int32)
    out["pos"] = np.zeros(ncol, dtype=np.int32)
    _check(L.splpak_debug_nd_fronts(len(nodes), _p(nodes, _ip), int(split_min), _p(nf, _ip), n,
                                    *(_p(out[k], _ip) for k in ("depth", "parent", "w", "h", "front_of", "pos"))))
    return out


def debug_window_values(nodes, xmin, xmax, x):
    """Host-only: the 4 basis values of the window of every x on a 1-D grid, as the evaluation kernels select the form
    (0 interior closed form / 1 next to an end / 2 general) and in the general form.  -> (ws, used[n,4], general[n,4], form)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    ws = np.zeros(n, dtype=np.int32)
    form = np.zeros(n, dtype=np.int32)
    used = np.zeros((n, 4))
    gen = np.zeros((n, 4))
    rc = _check(lib().splpak_debug_window_values(int(nodes), float(xmin), float(xmax), int(n), _p(x, _dp),
                                                 _p(ws, _ip), _p(used, _dp), _p(gen, _dp), _p(form, _ip)))
    if rc != 0:
        raise SplpakError(f"grid rejected: {rc}")
    return ws, used, gen, form


def debug_bin_points(nodes, xmin, xmax, x, y, w=None):
    """The binning of the points by window alone, without a plan (diagnostics, splpak_debug_bin_points), everything raw in the
    library's internal numbering.  x: (ndata, l1xdat) with l1xdat >= ndim.  -> dict(perm, cells, cellstride, route, cpt, key,
    offset, placed, nrows_data, idx [placed], xs [ndim, placed], ys, ws [placed])."""
    nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
    nd = len(nodes)
    xmin = np.ascontiguousarray(xmin, dtype=np.float64)
    xmax = np.ascontiguousarray(xmax, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    m, ldx = x.shape
    assert y.shape == (m,) and (w is None or w.shape == (m,)) and xmin.shape == (nd,) and xmax.shape == (nd,)
    ncell = int(np.prod(np.maximum(nodes.astype(np.int64) - 3, 1)))
    perm, cells, stride = (np.zeros(nd, dtype=np.int32) for _ in range(3))
    route, cpt = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    key, idx = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    offset = np.zeros(ncell + 1, dtype=np.int32)
    xs, ys, ws = np.zeros((nd, m)), np.zeros(m), np.zeros(m)
    placed = C.c_int64(-1)
    rows = C.c_double(-1.0)
    rc = _check(lib().splpak_debug_bin_points(nd, _p(nodes, _ip), _p(xmin, _dp), _p(xmax, _dp), m, _p(x, _dp), ldx, _p(y, _dp), _p(w, _dp),
                                              _p(perm, _ip), _p(cells, _ip), _p(stride, _ip), _p(route, _ip), _p(cpt, _ip), _p(key, _ip),
                                              _p(offset, _ip), _p(idx, _ip), _p(xs, _dp), _p(ys, _dp), _p(ws, _dp), C.byref(placed),
                                              C.byref(rows)))
    if rc != 0:
        raise SplpakError(f"grid rejected: {rc}")
    n = int(placed.value)
    return dict(perm=perm, cells=cells, cellstride=stride, route=int(route[0]), cpt=int(cpt[0]), key=key, offset=offset, placed=n,
                nrows_data=rows.value, idx=idx[:n], xs=xs[:, :n], ys=ys[:n], ws=ws[:n])


def debug_spd_band_solve(a_lower, halfbw, b):
    """Solve with the library's band Cholesky (diagnostics).  a_lower: (n, n) array, lower part used."""
    a = np.asfortranarray(a_lower, dtype=np.float64)
    n = a.shape[0]
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(n)
    rc = _check(lib().splpak_debug_spd_band_solve_f64(n, int(halfbw), _p(a, _dp), _p(b, _dp), _p(x, _dp)))
    return x, rc
