"""ctypes binding of libmanipula_hip.so (include/manipula_hip.h).

This is the whole FFI: no PyTorch, CuPy or Triton on the product path.  There is no CPU fallback
behind it — if the library or a GPU is missing the calls raise (`HipUnavailableError` /
`HipError`), they never silently compute somewhere else.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional, Sequence

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_ENV = "MANIPULAPY_HIP_LIB"  # override the library path
DEFAULT_LIB = os.path.join(_PKG, "libmanipula_hip.so")

MP_OK = 0
MP_MAX_DOF = 8    # fully unrolled / specialisable kernels
MP_BIG_DOF = 32   # run-time-n kernels (csrc/mp_dyn.h)
UNIQUE_ID_BYTES = 128


class HipError(RuntimeError):
    """A libmanipula_hip call returned a non-zero code (message from mp_last_error)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[manipula_hip rc={code}] {message}")
        self.code = code


class HipUnavailableError(RuntimeError):
    """The native library cannot be loaded, or no GPU is visible."""


_c_dp = ctypes.POINTER(ctypes.c_double)
_c_fp = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_i64 = ctypes.c_int64

# name -> (restype, argtypes); the list is also what tests/test_cabi_symbols.py checks against the header
SIGNATURES = {
    "mp_version": (ctypes.c_int, []),
    "mp_last_error": (ctypes.c_char_p, []),
    "mp_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "mp_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "mp_ctx_destroy": (ctypes.c_int, [_vp]),
    "mp_ctx_synchronize": (ctypes.c_int, [_vp]),
    "mp_ctx_get_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mp_ctx_wait_for_stream": (ctypes.c_int, [_vp, _vp]),
    "mp_ctx_stream_wait_for_ctx": (ctypes.c_int, [_vp, _vp]),
    "mp_ctx_properties": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    "mp_selftest": (ctypes.c_int, [_vp]),
    "mp_stream_bandwidth": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "mp_stream_bandwidth_mix": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "mp_clock_sample_begin": (ctypes.c_int, [_vp, ctypes.c_double]),
    "mp_clock_sample_end": (ctypes.c_int, [_vp, _c_dp, _c_dp]),
    "mp_ctx_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mp_ctx_profile": (ctypes.c_int, [_vp, _c_dp, ctypes.POINTER(ctypes.c_int64), _c_dp, ctypes.c_int]),
    "mp_malloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "mp_free": (ctypes.c_int, [_vp, _vp]),
    "mp_pool_trim": (ctypes.c_int, [_vp]),
    "mp_memcpy_h2d": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "mp_memcpy_d2h": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "mp_memset": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_size_t]),
    "mp_event_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mp_event_destroy": (ctypes.c_int, [_vp]),
    "mp_event_record": (ctypes.c_int, [_vp, _vp]),
    "mp_event_elapsed_ms": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_float)]),
    "mp_host_alloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "mp_host_free": (ctypes.c_int, [_vp, _vp]),
    "mp_inverse_kinematics_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "mp_inverse_kinematics_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "mp_graph_begin": (ctypes.c_int, [_vp]),
    "mp_graph_end": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mp_graph_launch": (ctypes.c_int, [_vp, _vp]),
    "mp_graph_destroy": (ctypes.c_int, [_vp]),
    "mp_model_create": (ctypes.c_int, [ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.POINTER(_vp)]),
    "mp_model_destroy": (ctypes.c_int, [_vp]),
    "mp_model_dof": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "mp_model_params": (ctypes.c_int, [_vp, _c_dp]),
    "mp_model_fk_host": (ctypes.c_int, [_vp, _c_dp, _c_dp]),
    "mp_model_specialize": (ctypes.c_int, [_vp, _vp]),
    "mp_model_is_specialized": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_int)]),
    "mp_model_specialize_compile": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    "mp_model_specialize_source": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]),
    "mp_model_blob": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_size_t)]),
    "mp_batch_trajectory_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]),
    "mp_id_trajectory_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp]),
    "mp_id_trajectory_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp]),
    "mp_traj_id_fused_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _vp]),
    "mp_fk_jac_id_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp]),
    "mp_fk_jac_id_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp]),
    "mp_mass_matrix_f64": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "mp_mass_matrix_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "mp_forward_dynamics_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp]),
    "mp_forward_dynamics_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp]),
    "mp_fd_trajectory_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]),
    "mp_fd_trajectory_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]),
    "mp_fd_trajectory_tm_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]),
    "mp_fd_trajectory_tm_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]),
    "mp_transpose_rows": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "mp_mass_matrix_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _i64, _c_dp]),
    "mp_forward_dynamics_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp]),
    "mp_id_derivatives_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_fd_derivatives_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_id_derivatives_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_fd_derivatives_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_id_vjp_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp]),
    "mp_fd_vjp_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_id_vjp_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_fd_vjp_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_id_vjp_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fd_vjp_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fk_jac_vjp_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "mp_fk_jac_vjp_host_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp]),
    "mp_fk_jac_vjp_cpu_f64": (ctypes.c_int, [_vp, ctypes.c_int, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_opspace_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp, _i64, _c_dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_opspace_host_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_opspace_cpu_f64": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_opspace_torque_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp, _vp, _vp, _i64, _c_dp, _vp]),
    "mp_opspace_torque_host_f64": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp]),
    "mp_opspace_torque_cpu_f64": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, ctypes.c_int]),
    "mp_id_regressor_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp]),
    "mp_id_regressor_normal_workspace_bytes": (ctypes.c_int64, [_vp, _i64]),
    "mp_id_regressor_normal_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_id_regressor_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_id_regressor_normal_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_fd_trajectory_vjp_workspace_bytes": (ctypes.c_int64, [_vp, _i64, _i64, ctypes.c_int]),
    "mp_fd_trajectory_vjp_tm_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_fd_trajectory_vjp_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_ilqr_backward_workspace_bytes": (ctypes.c_int64, [_vp, _i64, _i64]),
    "mp_ilqr_backward_tm_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _i64, _i64, ctypes.c_double, _vp, _vp, _vp, _vp, _vp]),
    "mp_ilqr_rollout_tm_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _i64, _i64, _c_dp, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "mp_ilqr_backward_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, _c_dp, _c_dp, _c_dp, _vp]),
    "mp_ilqr_rollout_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _i64, _c_dp, ctypes.c_double, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_ilqr_backward_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, _c_dp, _c_dp, _c_dp, _vp, ctypes.c_int]),
    "mp_ilqr_rollout_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _i64, _c_dp, ctypes.c_double, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_path_dynamics_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_toppra_tm_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_dp, _c_dp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_toppra_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _c_dp, _c_dp, _c_dp]),
    "mp_path_dynamics_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_toppra_sweep_cpu_f64": (ctypes.c_int, [ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_toppra_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fd_trajectory_host_f32": (ctypes.c_int, [_vp, _vp, _c_fp, _c_fp, _c_fp, _c_fp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp]),
    "mp_fd_trajectory_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp]),
    "mp_cartesian_trajectory_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "mp_cartesian_trajectory_host_f32": (ctypes.c_int, [_vp, _c_dp, _c_dp, _i64, _i64, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp, _c_fp]),
    "mp_potential_field_f32": (ctypes.c_int, [_vp, _vp, _c_fp, _vp, _i64, _i64, ctypes.c_float, _vp, _vp]),
    "mp_potential_field_host_f32": (ctypes.c_int, [_vp, _c_fp, _c_fp, _c_fp, _i64, _i64, ctypes.c_float, _c_fp, _c_fp]),
    "mp_batch_trajectory_host_f32": (ctypes.c_int, [_vp, _vp, _c_fp, _c_fp, _i64, _i64, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp]),
    "mp_id_trajectory_host_f32": (ctypes.c_int, [_vp, _vp, _c_fp, _c_fp, _c_fp, _i64, _c_dp, _c_dp, _c_fp]),
    "mp_id_trajectory_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp]),
    "mp_traj_id_fused_host_f32": (ctypes.c_int, [_vp, _vp, _c_fp, _c_fp, _i64, _i64, ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_fp]),
    "mp_fk_jac_id_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_pd_regulation_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_dp, _vp]),
    "mp_pd_regulation_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_dp, _vp, ctypes.c_int]),
    "mp_cpu_threads": (ctypes.c_int, [_i64]),
    "mp_id_trajectory_cpu_f32": (ctypes.c_int, [_vp, _c_fp, _c_fp, _c_fp, _i64, _c_dp, _c_dp, _c_fp, ctypes.c_int]),
    "mp_id_row_precision_cpu_f32": (ctypes.c_int, [_vp, _c_fp, _c_fp, _c_fp, _i64, _c_dp, _c_dp, _vp, ctypes.c_int]),
    "mp_id_trajectory_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fk_jac_id_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_mass_matrix_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _i64, _c_dp, ctypes.c_int]),
    "mp_forward_dynamics_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_id_derivatives_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fd_derivatives_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_id_regressor_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_id_regressor_normal_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fd_trajectory_vjp_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_fd_trajectory_cpu_f32": (ctypes.c_int, [_vp, _c_fp, _c_fp, _c_fp, _c_fp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp, ctypes.c_int]),
    "mp_fd_trajectory_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, _i64, _c_dp, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp, ctypes.c_int]),
    "mp_inverse_kinematics_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, ctypes.c_int64, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _c_dp, _vp, _vp, _vp, ctypes.c_int]),
    "mp_cartesian_trajectory_cpu_f32": (ctypes.c_int, [_c_dp, _c_dp, _i64, _i64, ctypes.c_double, ctypes.c_int, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_int]),
    "mp_collision_create": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _c_dp, _c_dp, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "mp_collision_destroy": (ctypes.c_int, [_vp]),
    "mp_collision_set_world": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _c_dp]),
    "mp_collision_set_cloud": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "mp_collision_cloud_info": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_collision_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_collision_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _i64, ctypes.c_double, ctypes.c_double, _c_dp, _vp, _c_dp, _vp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_collision_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _i64, ctypes.c_double, ctypes.c_double, _c_dp, _vp, _c_dp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_collision_motion_bounds": (ctypes.c_int, [_vp, _c_dp]),
    "mp_collision_edges_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mp_collision_edges_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _c_dp, _i64, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _c_dp, _vp, _c_dp, _vp]),
    "mp_collision_edges_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _i64, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _c_dp, _vp, _c_dp, _vp, ctypes.c_int]),
    "mp_rrt_connect_workspace_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mp_rrt_connect_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_rrt_connect_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _c_dp, _vp, _vp, _vp]),
    "mp_rrt_connect_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _c_dp, _vp, _vp, _vp, ctypes.c_int]),
    "mp_path_shortcut_workspace_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mp_path_shortcut_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_path_shortcut_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _vp, _i64, _i64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    "mp_path_shortcut_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _vp, _i64, _i64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "mp_path_blend_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int] + [_vp] * 13),
    "mp_path_blend_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _vp, _i64, _i64, _i64, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "mp_path_blend_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _vp, _i64, _i64, _i64, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int]),
    "mp_trajectory_sample_f64": (ctypes.c_int, [_vp] * 4 + [_i64, _i64] + [_vp] * 9 + [_i64, ctypes.c_double, _i64, _c_dp, _c_dp, ctypes.c_int] + [_vp] * 10),
    "mp_trajectory_sample_host_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _i64, _i64, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, ctypes.c_double, _i64, _c_dp, _c_dp, _vp, _vp, _vp] + [_c_dp] * 7),
    "mp_trajectory_sample_cpu_f64": (ctypes.c_int, [_vp, _c_dp, _c_dp, _i64, _i64, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _i64, ctypes.c_double, _i64, _c_dp, _c_dp, _vp, _vp, _vp] + [_c_dp] * 7 + [ctypes.c_int]),
    "mp_cartesian_path_workspace_bytes": (_i64, [_i64, _i64]),
    "mp_cartesian_path_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, _i64, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int] + [_vp] * 15),
    "mp_cartesian_path_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _i64, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _c_dp]),
    "mp_cartesian_path_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, _i64, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _c_dp, ctypes.c_int]),
    "mp_goal_ik_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mp_goal_ik_host_f64": (ctypes.c_int, [_vp, _vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _vp, _c_dp, _vp, _vp, _vp, _c_dp, _c_dp, _vp]),
    "mp_goal_ik_cpu_f64": (ctypes.c_int, [_vp, _vp, _c_dp, _c_dp, _i64, _c_dp, _c_dp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _vp, _c_dp, _vp, _vp, _vp, _c_dp, _c_dp, _vp, ctypes.c_int]),
    "mp_comm_unique_id": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint8)]),
    "mp_comm_create": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "mp_comm_destroy": (ctypes.c_int, [_vp]),
    "mp_comm_allgather": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "mp_comm_exchange_chunk": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]),
    "mp_comm_join": (ctypes.c_int, [_vp]),
    "mp_comm_allgatherv": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_size_t)]),
    "mp_comm_exchange_chunk_v": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
}

_lib = None
_lib_lock = threading.Lock()


def lib_path() -> str:
    return os.environ.get(LIB_ENV, DEFAULT_LIB)


def load_library():
    """Load (once) and type the shared library.  Raises HipUnavailableError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path) and path == DEFAULT_LIB:
            # a fresh checkout: compile the native library in-tree (hipcc cross-compiles without a GPU)
            try:
                from .build import build as _build

                _build(verbose=False)
            except Exception as exc:
                raise HipUnavailableError(
                    f"{path} not found and building it failed ({exc}); run `python -m manipulapy_amd.build` "
                    "(needs hipcc) - there is no CPU fallback for the HIP backend") from exc
        if not os.path.exists(path):
            raise HipUnavailableError(
                f"{path} not found: build it with `python -m manipulapy_amd.build` (needs hipcc); "
                "there is no CPU fallback for the HIP backend")
        try:
            lib = ctypes.CDLL(path)
        except OSError as exc:
            raise HipUnavailableError(f"cannot load {path}: {exc}") from exc
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _check(rc: int) -> None:
    if rc != MP_OK:
        msg = load_library().mp_last_error()
        raise HipError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")


def device_count() -> int:
    """Number of visible GPUs (0 if none).  Raises only when the library itself is missing."""
    n = ctypes.c_int(0)
    rc = load_library().mp_device_count(ctypes.byref(n))
    if rc != MP_OK:
        return 0
    return int(n.value)


def _dptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_c_dp)


def _fptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_c_fp)


def _as_c(a, dtype, shape=None, name="array") -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(arr.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(arr.shape)}")
    return arr


def _vec_or_none(v, k, name):
    if v is None:
        return None
    return _as_c(v, np.float64, (k,), name)


# operational-space dynamics (csrc/mp_opspace.h): the output names of mp_opspace_*_f64 in the order of its arguments
OPSPACE_OUTPUTS = ("T", "J", "Jdot_qd", "Lambda", "Jbar", "mu", "p")
_OPSPACE_FRAMES = {"space": 0, "body": 1, "hybrid": 2}
_OPSPACE_TASKS = {"full": 0, "linear": 1, "angular": 2}


class DeviceBuffer:
    """A pooled device allocation (mp_malloc / mp_free)."""

    def __init__(self, ctx: "HipContext", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = _vp()
        _check(ctx.lib.mp_malloc(ctx.handle, ctypes.c_size_t(max(self.nbytes, 1)), ctypes.byref(p)))
        self.ptr = p

    def upload(self, host: np.ndarray) -> "DeviceBuffer":
        host = np.ascontiguousarray(host)
        if host.nbytes > self.nbytes:
            raise ValueError("upload larger than the device buffer")
        _check(self.ctx.lib.mp_memcpy_h2d(self.ctx.handle, self.ptr, host.ctypes.data_as(_vp), ctypes.c_size_t(host.nbytes)))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download larger than the device buffer")
        _check(self.ctx.lib.mp_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(_vp), self.ptr, ctypes.c_size_t(out.nbytes)))
        return out

    def free(self) -> None:
        if self.ptr is not None and self.ctx.handle is not None:
            self.ctx.lib.mp_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def offset(self, nbytes: int) -> ctypes.c_void_p:
        return _vp(self.ptr.value + int(nbytes))


class HipEvent:
    def __init__(self, ctx: "HipContext"):
        self.ctx = ctx
        p = _vp()
        _check(ctx.lib.mp_event_create(ctx.handle, ctypes.byref(p)))
        self.handle = p

    def record(self) -> None:
        _check(self.ctx.lib.mp_event_record(self.ctx.handle, self.handle))

    def elapsed_ms_since(self, start: "HipEvent") -> float:
        ms = ctypes.c_float(0)
        _check(self.ctx.lib.mp_event_elapsed_ms(start.handle, self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def destroy(self) -> None:
        if self.handle is not None:
            self.ctx.lib.mp_event_destroy(self.handle)
            self.handle = None


class PinnedBuffer:
    """Page-locked host memory (mp_host_alloc).  ``np.asarray(buf)`` / ``buf.array(shape, dtype)`` give NumPy views that
    keep the allocation alive; on such arrays the *_host entry points overlap upload, kernels and download."""

    def __init__(self, ctx: "HipContext", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = _vp()
        _check(ctx.lib.mp_host_alloc(ctx.handle, ctypes.c_size_t(self.nbytes), ctypes.byref(p)))
        self.ptr = p.value
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def array(self, shape, dtype) -> np.ndarray:
        a = np.asarray(self).view(np.dtype(dtype))
        n = int(np.prod(shape))
        if n > a.size:
            raise ValueError("shape larger than the pinned buffer")
        return a[:n].reshape(shape)

    def __del__(self):
        try:
            if self.ptr:  # valid with or without the allocating context: the buffer does not belong to it
                self.ctx.lib.mp_host_free(None, _vp(self.ptr))
        except Exception:
            pass
        self.ptr = None


class HipGraph:
    """A captured sequence of device-pointer launches (mp_graph_*), replayed with one submission."""

    def __init__(self, ctx: "HipContext", handle):
        self.ctx, self.handle = ctx, handle

    def launch(self) -> None:
        _check(self.ctx.lib.mp_graph_launch(self.ctx.handle, self.handle))

    def destroy(self) -> None:
        if self.handle is not None:
            self.ctx.lib.mp_graph_destroy(self.handle)
            self.handle = None


class _Capture:
    def __init__(self, ctx: "HipContext"):
        self.ctx, self.graph = ctx, None

    def __enter__(self):
        _check(self.ctx.lib.mp_graph_begin(self.ctx.handle))
        return self

    def __exit__(self, exc_type, exc, tb):
        p = _vp()
        rc = self.ctx.lib.mp_graph_end(self.ctx.handle, ctypes.byref(p))
        if exc_type is None:
            _check(rc)
            self.graph = HipGraph(self.ctx, p)
        elif rc == 0:
            self.ctx.lib.mp_graph_destroy(p)
        return False


class HipModel:
    """Compiled robot model (mp_model_create).  Host-only object: no GPU needed to build one."""

    def __init__(self, S_list, Mlist_per_link, Glist, M_ee, joint_limits=None, torque_limits=None):
        self.lib = load_library()
        S = _as_c(S_list, np.float64, name="S_list")
        if S.ndim != 2 or S.shape[0] != 6:
            raise ValueError(f"S_list must be (6, n), got {S.shape}")
        n = S.shape[1]
        Mc = _as_c(Mlist_per_link, np.float64, (n, 4, 4), "Mlist_per_link")
        G = _as_c(Glist, np.float64, (n, 6, 6), "Glist")
        Me = _as_c(M_ee, np.float64, (4, 4), "M_list")
        jl = None if joint_limits is None else _as_c(joint_limits, np.float64, (n, 2), "joint_limits")
        tl = None if torque_limits is None else _as_c(torque_limits, np.float64, (n, 2), "torque_limits")
        p = _vp()
        _check(self.lib.mp_model_create(n, _dptr(S), _dptr(Mc), _dptr(G), _dptr(Me), _dptr(jl), _dptr(tl), ctypes.byref(p)))
        self.handle = p
        self.n = n

    def params(self) -> np.ndarray:
        out = np.zeros((self.n, 16))
        _check(self.lib.mp_model_params(self.handle, _dptr(out)))
        return out

    def specialize_source(self, part: int = 0) -> str:
        """One of the two translation units the run-time specialiser compiles for this robot (part 1: the one-row-per-lane float32
        inverse dynamics, built with the max-ILP scheduling strategy)."""
        n = ctypes.c_size_t(0)
        _check(self.lib.mp_model_specialize_source(self.handle, None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        _check(self.lib.mp_model_specialize_source(self.handle, buf, ctypes.byref(n)))
        both = buf.value.decode().split("\n// ==== second program", 1)
        return both[0] if part == 0 else "// ==== second program" + both[1]

    def specialize_compile(self):
        """hiprtc-compile the specialised kernels (no GPU needed): (code bytes, came from the disk cache)."""
        nb, cached = ctypes.c_size_t(0), ctypes.c_int(0)
        _check(self.lib.mp_model_specialize_compile(self.handle, ctypes.byref(nb), ctypes.byref(cached)))
        return int(nb.value), bool(cached.value)

    def blob(self, dtype=np.float32) -> dict:
        """The compiled model as the kernels see it, unpacked by field (csrc/mp_model.h layout)."""
        f64 = np.dtype(dtype) == np.float64
        nb = ctypes.c_size_t(0)
        _check(self.lib.mp_model_blob(self.handle, int(f64), None, ctypes.byref(nb)))
        raw = np.zeros(nb.value, dtype=np.uint8)
        _check(self.lib.mp_model_blob(self.handle, int(f64), raw.ctypes.data_as(_vp), ctypes.byref(nb)))
        w = 8 if f64 else 4
        head = 16 if not f64 else 16  # int n + 3 pad ints
        vals = raw[head:].view(np.float64 if f64 else np.float32)
        o = 0
        def take(k):
            nonlocal o
            v = vals[o:o + k].copy(); o += k
            return v
        d = {"n": int(raw[:4].view(np.int32)[0]), "base_R": take(9), "base_p": take(3), "tool_R": take(9), "tool_p": take(3)}
        F = 18                                           # MP_JOINT_FIELDS (csrc/mp_model.h): the 16 of params() + cos / sin of the offset
        cap = (nb.value - head - 24 * w) // ((F + 4) * w)   # MP_MAX_DOF, or MP_BIG_DOF for the looped kernels' model
        d["joints"] = take(F * cap).reshape(cap, F)
        for k in ("qmin", "qmax", "taumin", "taumax"):
            d[k] = take(cap)
        assert o * w + head == nb.value, (o * w + head, nb.value)
        return d

    def joint_limits_f32(self) -> np.ndarray:
        """(n, 2) float32 joint limits exactly as the kernels clip against them (+-inf where the model is unbounded)."""
        b = self.blob(np.float32)
        return np.stack([b["qmin"][:self.n], b["qmax"][:self.n]], axis=1).astype(np.float32)

    def fk_host(self, q) -> np.ndarray:
        q = _as_c(q, np.float64, (self.n,), "q")
        T = np.zeros((4, 4))
        _check(self.lib.mp_model_fk_host(self.handle, _dptr(q), _dptr(T)))
        return T

    def destroy(self) -> None:
        if getattr(self, "handle", None) is not None:
            self.lib.mp_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class HipContext:
    """One device context (streams + pooled device memory).  Fails loudly without a GPU."""

    def __init__(self, device_id: int = 0):
        self.lib = load_library()
        self.handle = None
        n = ctypes.c_int(0)
        rc = self.lib.mp_device_count(ctypes.byref(n))
        if rc != MP_OK or n.value <= 0:
            raise HipUnavailableError("no HIP device visible: the HIP backend has no CPU fallback")
        p = _vp()
        _check(self.lib.mp_ctx_create(int(device_id), ctypes.byref(p)))
        self.handle = p
        self.device_id = int(device_id)

    # ---- plumbing
    def synchronize(self) -> None:
        _check(self.lib.mp_ctx_synchronize(self.handle))

    def selftest(self) -> None:
        _check(self.lib.mp_selftest(self.handle))

    def stream_bandwidth(self, bytes_per_array: int, reads: int = 1, reps: int = 20, nontemporal: bool = False) -> float:
        """GB/s of a device copy (reads = 1) or of the 3-reads-1-write mix of the inverse-dynamics kernels (reads = 3), with plain
        or non-temporal accesses."""
        out = ctypes.c_double(0.0)
        _check(self.lib.mp_stream_bandwidth(self.handle, ctypes.c_size_t(int(bytes_per_array)), int(reads) + (10 if nontemporal else 0), int(reps),
                                            ctypes.byref(out)))
        return float(out.value)

    def stream_bandwidth_mix(self, bytes_per_array: int, reads: int, writes: int, reps: int = 10, nontemporal: bool = True) -> float:
        """GB/s of a streaming kernel that reads `reads` and writes `writes` arrays of bytes_per_array bytes (a kernel's own byte mix)."""
        out = ctypes.c_double(0.0)
        _check(self.lib.mp_stream_bandwidth_mix(self.handle, ctypes.c_size_t(int(bytes_per_array)), int(reads), int(writes),
                                                1 if nontemporal else 0, int(reps), ctypes.byref(out)))
        return float(out.value)

    def clock_sample_begin(self, duration_ms: float) -> None:
        """Start the bounded shader-clock sampler beside whatever is launched next (mp_clock_sample_begin)."""
        _check(self.lib.mp_clock_sample_begin(self.handle, ctypes.c_double(float(duration_ms))))

    def clock_sample_end(self):
        """(clock in Hz held while the sampler ran, milliseconds its stamps span)."""
        hz, ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _check(self.lib.mp_clock_sample_end(self.handle, ctypes.byref(hz), ctypes.byref(ms)))
        return float(hz.value), float(ms.value)

    def properties(self) -> dict:
        name = ctypes.create_string_buffer(256)
        cu = ctypes.c_int(0)
        mem = ctypes.c_uint64(0)
        _check(self.lib.mp_ctx_properties(self.handle, name, 256, ctypes.byref(cu), ctypes.byref(mem)))
        # key names follow the reference's get_gpu_properties() (cuda_kernels/registry.py:335-356)
        return {"name": name.value.decode(), "multiprocessor_count": int(cu.value), "total_memory": int(mem.value),
                "warp_size": 64}

    def specialize(self, model: "HipModel") -> None:
        """Load (compiling if needed) float32 kernels specialised for `model` on this device."""
        _check(self.lib.mp_model_specialize(self.handle, model.handle))

    def is_specialized(self, model: "HipModel") -> bool:
        yes = ctypes.c_int(0)
        _check(self.lib.mp_model_is_specialized(self.handle, model.handle, ctypes.byref(yes)))
        return bool(yes.value)

    def set_profiling(self, on: bool = True) -> None:
        """Timed HIP event pair + roctx range around every entry point's launches (mp_ctx_set_profiling)."""
        _check(self.lib.mp_ctx_set_profiling(self.handle, int(bool(on))))

    def profile(self, reset: bool = False) -> dict:
        """{"kernel_ms_total", "timed_calls", "kernel_ms_last"} since profiling was switched on (or the last reset);
        waits for the launches recorded so far."""
        tot, last, calls = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        _check(self.lib.mp_ctx_profile(self.handle, ctypes.byref(tot), ctypes.byref(calls), ctypes.byref(last), int(bool(reset))))
        return {"kernel_ms_total": float(tot.value), "timed_calls": int(calls.value), "kernel_ms_last": float(last.value)}

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, host: np.ndarray) -> DeviceBuffer:
        host = np.ascontiguousarray(host)
        return DeviceBuffer(self, host.nbytes).upload(host)

    def memset(self, buf, value: int, nbytes: int) -> None:
        """Asynchronous byte fill on the compute stream."""
        _check(self.lib.mp_memset(self.handle, _p(buf), int(value), ctypes.c_size_t(int(nbytes))))

    def event(self) -> HipEvent:
        return HipEvent(self)

    def pinned_empty(self, shape, dtype=np.float32) -> np.ndarray:
        """Uninitialised page-locked NumPy array (freed with its last view, or with the context)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        return PinnedBuffer(self, max(1, n) * dtype.itemsize).array(shape, dtype)

    def stream(self) -> int:
        """The compute stream (a hipStream_t as an integer) for callers that order their own HIP work behind the launches."""
        p = _vp()
        _check(self.lib.mp_ctx_get_stream(self.handle, ctypes.byref(p)))
        return p.value or 0

    def wait_for_stream(self, hip_stream: int) -> None:
        """The compute stream waits for what is enqueued on `hip_stream` (an integer hipStream_t; 0 = the null stream) so far."""
        _check(self.lib.mp_ctx_wait_for_stream(self.handle, _vp(int(hip_stream)) if hip_stream else None))

    def stream_wait_for_ctx(self, hip_stream: int) -> None:
        """`hip_stream` waits for what is enqueued on the compute stream so far (unlike `stream`, parking is left as it is)."""
        _check(self.lib.mp_ctx_stream_wait_for_ctx(self.handle, _vp(int(hip_stream)) if hip_stream else None))

    def capture(self) -> _Capture:
        """``with ctx.capture() as cap: <device-pointer launches>`` -> ``cap.graph`` (HipGraph)."""
        return _Capture(self)

    def trim_pool(self) -> None:
        _check(self.lib.mp_pool_trim(self.handle))

    def destroy(self) -> None:
        if self.handle is not None:
            self.lib.mp_ctx_destroy(self.handle)
            self.handle = None

    # ---- hot path on device buffers (asynchronous)
    def id_trajectory(self, model: HipModel, d_q, d_qd, d_qdd, rows: int, d_tau, g=None, Ftip=None, dtype=np.float32):
        fn = self.lib.mp_id_trajectory_f32 if np.dtype(dtype) == np.float32 else self.lib.mp_id_trajectory_f64
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(fn(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), int(rows), _dptr(g), _dptr(F), _p(d_tau)))

    def batch_trajectory(self, model, d_start, d_end, B, N, Tf, method, d_pos, d_vel, d_acc):
        _check(self.lib.mp_batch_trajectory_f32(self.handle, model.handle, _p(d_start), _p(d_end), int(B), int(N),
                                                float(Tf), int(method), _p(d_pos), _p(d_vel), _p(d_acc)))

    def traj_id_fused(self, model, d_start, d_end, B, N, Tf, method, d_tau, g=None, Ftip=None):
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(self.lib.mp_traj_id_fused_f32(self.handle, model.handle, _p(d_start), _p(d_end), int(B), int(N),
                                             float(Tf), int(method), _dptr(g), _dptr(F), _p(d_tau)))

    def fk_jac_id(self, model, d_q, d_qd, d_qdd, rows, d_T, d_J, d_tau, g=None, Ftip=None, dtype=np.float64):
        fn = self.lib.mp_fk_jac_id_f64 if np.dtype(dtype) == np.float64 else self.lib.mp_fk_jac_id_f32
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(fn(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), int(rows), _dptr(g), _dptr(F), _p(d_T), _p(d_J), _p(d_tau)))

    def mass_matrix(self, model, d_q, rows, d_M, dtype=np.float64):
        fn = self.lib.mp_mass_matrix_f64 if np.dtype(dtype) == np.float64 else self.lib.mp_mass_matrix_f32
        _check(fn(self.handle, model.handle, _p(d_q), int(rows), _p(d_M)))

    def forward_dynamics(self, model, d_q, d_qd, d_tau, rows, d_qdd, g=None, Ftip=None, dtype=np.float64):
        fn = self.lib.mp_forward_dynamics_f64 if np.dtype(dtype) == np.float64 else self.lib.mp_forward_dynamics_f32
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(fn(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_tau), int(rows), _dptr(g), _dptr(F), _p(d_qdd)))

    def id_derivatives(self, model, d_q, d_qd, d_qdd, rows, d_dtau_dq, d_dtau_dqd, d_tau=None, d_M=None, g=None, Ftip=None):
        """Analytical inverse-dynamics derivatives on device buffers (float64; csrc/mp_deriv.h); asynchronous."""
        _check(self.lib.mp_id_derivatives_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), int(rows),
                                              _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_tau),
                                              _p(d_dtau_dq), _p(d_dtau_dqd), _p(d_M)))

    def fd_derivatives(self, model, d_q, d_qd, d_tau, rows, d_dqdd_dq, d_dqdd_dqd, d_qdd=None, d_Minv=None, g=None, Ftip=None):
        """Analytical forward-dynamics derivatives on device buffers (float64; csrc/mp_deriv.h); asynchronous."""
        _check(self.lib.mp_fd_derivatives_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_tau), int(rows),
                                              _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_qdd),
                                              _p(d_dqdd_dq), _p(d_dqdd_dqd), _p(d_Minv)))

    def id_vjp(self, model, d_q, d_qd, d_qdd, d_gtau, rows, d_gq, d_gqd, d_gqdd=None, g=None, Ftip=None):
        """Inverse-dynamics vector-Jacobian product on device buffers (float64; csrc/mp_adjoint.h); asynchronous (capturable)."""
        _check(self.lib.mp_id_vjp_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), _p(d_gtau), int(rows),
                                      _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_gq), _p(d_gqd),
                                      _p(d_gqdd)))

    def fd_vjp(self, model, d_q, d_qd, d_tau, d_gqdd, rows, d_gq, d_gqd, d_qdd=None, d_gtau=None, g=None, Ftip=None):
        """Forward-dynamics vector-Jacobian product on device buffers (float64; csrc/mp_adjoint.h); asynchronous (capturable)."""
        _check(self.lib.mp_fd_vjp_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_tau), _p(d_gqdd), int(rows),
                                      _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_qdd), _p(d_gq),
                                      _p(d_gqd), _p(d_gtau)))

    def fk_jac_vjp(self, model, frame, d_q, d_gT, d_gJ, rows, d_T=None, d_J=None, d_gq=None):
        """Reverse mode through FK + Jacobian on device buffers (float64; csrc/mp_kin_vjp.h): frame "space" / "body"; the cotangents
        d_gT (rows,4,4) / d_gJ (rows,6,n) may be None (= 0), every output may be None (at least one given); asynchronous (capturable)."""
        _check(self.lib.mp_fk_jac_vjp_f64(self.handle, model.handle, _frame_code(frame), _p(d_q), _p(d_gT), _p(d_gJ), int(rows), _p(d_T),
                                          _p(d_J), _p(d_gq)))

    def opspace(self, model, frame, task, damping, d_q, d_qd, rows, g=None, d_T=None, d_J=None, d_Jdqd=None, d_Lambda=None, d_Jbar=None,
                d_mu=None, d_p=None):
        """Operational-space dynamics on device buffers (float64; csrc/mp_opspace.h): frame "space" / "body" / "hybrid", task "full" /
        "linear" / "angular" (m = 6 / 3 / 3 rows); outputs T (rows,4,4), J (rows,m,n), Jdqd (rows,m), Lambda (rows,m,m), Jbar (rows,n,m),
        mu / p (rows,m), each may be None (at least one given); asynchronous (capturable)."""
        _check(self.lib.mp_opspace_f64(self.handle, model.handle, _opspace_frame(frame), _opspace_task(task), float(damping), _p(d_q),
                                       _p(d_qd), int(rows), _dptr(_vec_or_none(g, 3, "g")), _p(d_T), _p(d_J), _p(d_Jdqd), _p(d_Lambda),
                                       _p(d_Jbar), _p(d_mu), _p(d_p)))

    def opspace_torque(self, model, frame, task, damping, d_q, d_qd, d_acc, d_tau0, rows, d_tau, g=None):
        """Task-space computed torque on device buffers: d_acc (rows,m), d_tau0 (rows,n) or None -> d_tau (rows,n); asynchronous
        (capturable)."""
        _check(self.lib.mp_opspace_torque_f64(self.handle, model.handle, _opspace_frame(frame), _opspace_task(task), float(damping),
                                              _p(d_q), _p(d_qd), _p(d_acc), _p(d_tau0), int(rows), _dptr(_vec_or_none(g, 3, "g")),
                                              _p(d_tau)))

    def collision(self, model, collision, d_q, rows, eps_world, eps_self, d_dist_world=None, d_arg_world=None, d_dist_self=None,
                  d_arg_self=None, d_grad_dist_world=None, d_grad_dist_self=None, d_cost=None, d_grad=None):
        """Sphere-model collision distances, cost and gradients on device buffers (float64; csrc/mp_collision.h): `collision` is a
        HipCollision; d_q (rows,n); outputs dist_* / cost (rows), arg_* (rows,2) int32, grad_* (rows,n), each may be None (at least one
        given); asynchronous (capturable once the handle has been used or given a world on this context)."""
        _check(self.lib.mp_collision_f64(self.handle, model.handle, collision.handle, _p(d_q), int(rows), float(eps_world),
                                         float(eps_self), _p(d_dist_world), _p(d_arg_world), _p(d_dist_self), _p(d_arg_self),
                                         _p(d_grad_dist_world), _p(d_grad_dist_self), _p(d_cost), _p(d_grad)))

    def collision_host(self, model, collision, q, eps_world, eps_self, want=None):
        """The same on host rows through the context's pool: a dict of the outputs named in `want` (default: all of COLLISION_OUTPUTS)."""
        return _collision((self.handle,), self.lib.mp_collision_host_f64, model, collision, q, eps_world, eps_self, want)

    def collision_edges(self, model, collision, d_q_from, d_q_to, edges, margin, tol, max_steps, d_status=None, d_t=None, d_steps=None,
                        d_clearance=None, d_witness=None, max_blocks: int = 0):
        """Continuous collision check of joint-space edges on device buffers (float64; csrc/mp_collision.h): d_q_from, d_q_to
        (edges,n); outputs status / steps (edges) int32, t / clearance (edges), witness (edges,3) int32, each may be None (at least
        one given).  `max_blocks` > 0 caps the grid of the work queue.  Asynchronous (capturable once the handle has been used or
        given a world on this context)."""
        _check(self.lib.mp_collision_edges_f64(self.handle, model.handle, collision.handle, _p(d_q_from), _p(d_q_to), int(edges),
                                               float(margin), float(tol), int(max_steps), int(max_blocks), _p(d_status), _p(d_t),
                                               _p(d_steps), _p(d_clearance), _p(d_witness)))

    def collision_edges_host(self, model, collision, q_from, q_to, margin, tol, max_steps, want=None):
        """The same on host rows through the context's pool: a dict of the outputs named in `want` (default: all of EDGE_OUTPUTS)."""
        return _collision_edges((self.handle,), self.lib.mp_collision_edges_host_f64, model, collision, q_from, q_to, margin, tol,
                                max_steps, want)

    def rrt_connect(self, model, collision, d_q_start, d_q_goal, problems, lo, hi, margin, tol, *, step, min_advance=None, max_iters,
                    max_nodes, max_waypoints, max_steps, seed, d_workspace, workspace_bytes, max_blocks: int = 0, d_status=None,
                    d_count=None, d_waypoints=None, d_iterations=None, d_nodes=None, d_evaluations=None):
        """Batched RRT-Connect on device buffers (float64; csrc/mp_rrt.h): d_q_start, d_q_goal (problems,n); lo, hi (n) host arrays;
        outputs status / count / iterations / evaluations (problems) int32, nodes (problems,2) int32, waypoints (problems,
        max_waypoints,n), each may be None (at least one given).  d_workspace holds the trees: rrt_connect_workspace_bytes(n,
        max_nodes, blocks).  `max_blocks` > 0 caps the grid.  Asynchronous (capturable once the handle has been used or given a
        world on this context)."""
        lo, hi, step, min_advance = _rrt_box(model, lo, hi, step, min_advance)
        _check(self.lib.mp_rrt_connect_f64(self.handle, model.handle, collision.handle, _p(d_q_start), _p(d_q_goal), int(problems),
                                           _dptr(lo), _dptr(hi), int(seed), step, min_advance, int(max_iters), int(max_nodes),
                                           int(max_waypoints), float(margin), float(tol), int(max_steps), _p(d_workspace),
                                           ctypes.c_size_t(int(workspace_bytes)), int(max_blocks), _p(d_status), _p(d_count),
                                           _p(d_waypoints), _p(d_iterations), _p(d_nodes), _p(d_evaluations)))

    def rrt_connect_arrays(self, model, collision, q_start, q_goal, lo, hi, margin, tol, *, step, min_advance=None, max_iters, max_nodes,
                         max_waypoints, max_steps, seed, want=None):
        """The same on host arrays (mp_rrt_connect_host_f64) through the context's pool, workspace included: a dict of the outputs
        named in `want` (default: all of PLAN_OUTPUTS).  (Not named `*_host`: that set of methods is the one
        tests/test_gpu_host_entries.py holds to hand-staged device launches; this entry's equality with its device form is held by
        tests/test_gpu_rrt.py.)"""
        return _rrt_connect((self.handle,), self.lib.mp_rrt_connect_host_f64, model, collision, q_start, q_goal, lo, hi, margin, tol,
                            step, min_advance, max_iters, max_nodes, max_waypoints, max_steps, seed, want)

    def path_shortcut(self, model, collision, d_waypoints_in, d_count_in, problems, w_in, margin, tol, *, max_iters, min_gain=0.0,
                      max_waypoints, max_steps, seed, d_workspace, workspace_bytes, max_blocks: int = 0, d_status=None, d_count=None,
                      d_waypoints=None, d_length_in=None, d_length_out=None, d_iterations=None, d_accepted=None, d_skipped_full=None,
                      d_evaluations=None):
        """Batched path shortcutting on device buffers (float64; csrc/mp_shortcut.h): d_waypoints_in (problems,w_in,n), d_count_in
        (problems) int32; outputs status / count / iterations / accepted / skipped_full / evaluations (problems) int32, length_in /
        length_out (problems), waypoints (problems,max_waypoints,n), each may be None (at least one given).  d_workspace holds the
        working paths: path_shortcut_workspace_bytes(n, max_waypoints, blocks).  `max_blocks` > 0 caps the grid.  Asynchronous
        (capturable once the handle has been used or given a world on this context)."""
        _check(self.lib.mp_path_shortcut_f64(self.handle, model.handle, collision.handle, _p(d_waypoints_in), _p(d_count_in),
                                             int(problems), int(w_in), int(seed), int(max_iters), float(min_gain), int(max_waypoints),
                                             float(margin), float(tol), int(max_steps), _p(d_workspace),
                                             ctypes.c_size_t(int(workspace_bytes)), int(max_blocks), _p(d_status), _p(d_count),
                                             _p(d_waypoints), _p(d_length_in), _p(d_length_out), _p(d_iterations), _p(d_accepted),
                                             _p(d_skipped_full), _p(d_evaluations)))

    def path_shortcut_arrays(self, model, collision, waypoints, count, margin, tol, *, max_iters, min_gain=0.0, max_waypoints=None,
                             max_steps, seed, want=None):
        """The same on host arrays (mp_path_shortcut_host_f64) through the context's pool, workspace included: a dict of the outputs
        named in `want` (default: all of SHORTCUT_OUTPUTS).  (Not named `*_host`, as rrt_connect_arrays is not; this entry's equality
        with its device form is held by tests/test_gpu_shortcut.py.)"""
        return _path_shortcut((self.handle,), self.lib.mp_path_shortcut_host_f64, model, collision, waypoints, count, margin, tol,
                              max_iters, min_gain, max_waypoints, max_steps, seed, want)

    def path_blend(self, model, collision, d_waypoints_in, d_count_in, problems, w_in, N, margin, tol, *, blend=0.5, max_halvings=6,
                   max_steps=64, max_blocks: int = 0, d_status=None, d_corner=None, d_count=None, d_points=None, d_cut=None, d_knot=None,
                   d_length=None, d_halvings=None, d_evaluations=None, d_clearance=None, d_q=None, d_dq=None, d_ddq=None):
        """C2 corner blending of waypoint paths on device buffers (float64; csrc/mp_blend.h): d_waypoints_in (problems,w_in,n),
        d_count_in (problems) int32; outputs status / corner / count / halvings / evaluations (problems) int32, length / clearance
        (problems), points (problems,w_in,n), cut / knot (problems,w_in), q / dq / ddq (problems,N,n), each may be None (at least one
        given; status, count, points, cut, knot and length are required with any of q, dq, ddq).  No workspace.  `max_blocks` > 0
        caps the grid of the corner launch.  Asynchronous (capturable once the handle has been used or given a world on this
        context)."""
        _check(self.lib.mp_path_blend_f64(self.handle, model.handle, collision.handle, _p(d_waypoints_in), _p(d_count_in), int(problems),
                                          int(w_in), int(N), float(blend), int(max_halvings), float(margin), float(tol), int(max_steps),
                                          int(max_blocks), _p(d_status), _p(d_corner), _p(d_count), _p(d_points), _p(d_cut), _p(d_knot),
                                          _p(d_length), _p(d_halvings), _p(d_evaluations), _p(d_clearance), _p(d_q), _p(d_dq), _p(d_ddq)))

    def path_blend_arrays(self, model, collision, waypoints, count, N, margin, tol, *, blend=0.5, max_halvings=6, max_steps=64, want=None):
        """The same on host arrays (mp_path_blend_host_f64) through the context's pool: a dict of the outputs named in `want` (default:
        all of BLEND_OUTPUTS).  (Not named `*_host`, as rrt_connect_arrays is not; this entry's equality with its device form is held
        by tests/test_gpu_blend.py.)"""
        return _path_blend((self.handle,), self.lib.mp_path_blend_host_f64, model, collision, waypoints, count, N, margin, tol, blend,
                           max_halvings, max_steps, want)

    def trajectory_sample(self, model, d_t, d_x, paths, N, dt, M, *, d_q=None, d_dq=None, d_ddq=None, d_blend_status=None,
                          d_blend_count=None, d_points=None, d_cut=None, d_knot=None, d_length=None, w_in: int = 0, g=None, Ftip=None,
                          max_blocks: int = 0, d_status=None, d_count=None, d_needed=None, d_s=None, d_sd=None, d_sdd=None,
                          d_positions=None, d_velocities=None, d_accelerations=None, d_torques=None):
        """Fixed-rate sampling of timed paths on device buffers (float64; csrc/mp_sample.h, contract in include/manipula_hip.h):
        d_t, d_x (paths, N) as the parameterisation returns "time" and "sd2"; the geometry is EITHER d_q / d_dq / d_ddq (paths, N, n)
        OR the blend's tables d_blend_status / d_blend_count (paths) int32, d_points (paths, w_in, n), d_cut / d_knot (paths, w_in),
        d_length (paths).  Outputs status / count / needed (paths) int32, s / sd / sdd (paths, M), positions / velocities /
        accelerations / torques (paths, M, n), each may be None (at least one given).  `max_blocks` > 0 caps the grid.  Asynchronous,
        allocates nothing, capturable - except torques of a 7- or 8-joint model without all of positions, velocities and
        accelerations: the missing rows come from the context's pool and the call is refused inside a capture."""
        _check(self.lib.mp_trajectory_sample_f64(self.handle, model.handle, _p(d_t), _p(d_x), int(paths), int(N), _p(d_q), _p(d_dq), _p(d_ddq),
                                                 _p(d_blend_status), _p(d_blend_count), _p(d_points), _p(d_cut), _p(d_knot), _p(d_length),
                                                 int(w_in), float(dt), int(M), _dptr(_vec_or_none(g, 3, "g")),
                                                 _dptr(_vec_or_none(Ftip, 6, "Ftip")), int(max_blocks), _p(d_status), _p(d_count),
                                                 _p(d_needed), _p(d_s), _p(d_sd), _p(d_sdd), _p(d_positions), _p(d_velocities),
                                                 _p(d_accelerations), _p(d_torques)))

    def trajectory_sample_arrays(self, model, t, x, dt, M, *, path=None, curve=None, g=None, Ftip=None, want=None):
        """The same on host arrays (mp_trajectory_sample_host_f64) through the context's pool: a dict of the outputs named in `want`
        (default: all of SAMPLE_OUTPUTS).  Its equality with the device form is held by tests/test_gpu_sample.py."""
        return _trajectory_sample((self.handle,), self.lib.mp_trajectory_sample_host_f64, model, t, x, dt, M, path, curve, g, Ftip, want)

    def goal_ik(self, model, collision, d_T_goal, d_q_seed, problems, lo, hi, margin, tol, *, eomg, ev, damping, step_cap, max_iters,
                max_attempts, seed, max_blocks: int = 0, d_status=None, d_q=None, d_attempts=None, d_iterations=None, d_converged=None,
                d_pose_error=None, d_clearance=None, d_witness=None):
        """Collision-free goal configurations for pose goals on device buffers (float64; csrc/mp_goal.h): d_T_goal (problems,16),
        d_q_seed (problems,n); lo, hi (n) host arrays; outputs status / attempts / iterations / converged (problems) int32, q
        (problems,n), pose_error (problems,2), clearance (problems), witness (problems,3) int32, each may be None (at least one
        given).  No workspace.  `max_blocks` > 0 caps the grid.  Asynchronous (capturable once the handle has been used or given a
        world on this context)."""
        lo, hi = _as_c(lo, np.float64, (model.n,), "lo"), _as_c(hi, np.float64, (model.n,), "hi")
        _check(self.lib.mp_goal_ik_f64(self.handle, model.handle, collision.handle, _p(d_T_goal), _p(d_q_seed), int(problems), _dptr(lo),
                                       _dptr(hi), int(seed), float(eomg), float(ev), float(damping), float(step_cap), int(max_iters),
                                       int(max_attempts), float(margin), float(tol), int(max_blocks), _p(d_status), _p(d_q),
                                       _p(d_attempts), _p(d_iterations), _p(d_converged), _p(d_pose_error), _p(d_clearance),
                                       _p(d_witness)))

    def goal_ik_arrays(self, model, collision, T_goal, q_seed, lo, hi, margin, tol, *, eomg, ev, damping, step_cap, max_iters,
                       max_attempts, seed, want=None):
        """The same on host arrays (mp_goal_ik_host_f64) through the context's pool: a dict of the outputs named in `want` (default:
        all of GOAL_OUTPUTS).  (Not named `*_host`, as rrt_connect_arrays is not; this entry's equality with its device form is held
        by tests/test_gpu_goal.py.)"""
        return _goal_ik((self.handle,), self.lib.mp_goal_ik_host_f64, model, collision, T_goal, q_seed, lo, hi, margin, tol, eomg, ev,
                        damping, step_cap, max_iters, max_attempts, seed, want)

    def cartesian_path(self, model, collision, d_q_start, d_T_goal, problems, lo, hi, N, margin, tol, *, task="full", eomg=1e-6,
                       ev=1e-6, damping=0.01, max_iters=20, max_joint_step=0.5, max_steps=64, d_workspace, workspace_bytes,
                       max_blocks: int = 0, d_status=None, d_reached=None, d_span=None, d_t=None, d_clearance=None,
                       d_deviation_pos=None, d_deviation_rot=None, d_pose_error=None, d_iterations=None, d_evaluations=None, d_q,
                       d_dq, d_ddq, d_span_status=None, d_span_clearance=None):
        """Cartesian straight-line paths on device buffers (float64; csrc/mp_cartesian.h, contract in include/manipula_hip.h):
        d_q_start (problems,n), d_T_goal (problems,16); lo, hi (n) host arrays; d_q / d_dq / d_ddq (problems,N,n) are required, the
        other outputs - status / reached / span / iterations / evaluations (problems) int32, t / clearance / deviation_pos /
        deviation_rot / pose_error (problems), span_status (problems,N-1) int32, span_clearance (problems,N-1) - may be None.
        d_workspace holds the spans' records: cartesian_path_workspace_bytes(problems, N).  `max_blocks` > 0 caps the grid of the
        span launch.  Asynchronous (capturable once the handle has been used or given a world on this context)."""
        lo, hi = _as_c(lo, np.float64, (model.n,), "lo"), _as_c(hi, np.float64, (model.n,), "hi")
        _check(self.lib.mp_cartesian_path_f64(self.handle, model.handle, collision.handle, _p(d_q_start), _p(d_T_goal), int(problems),
                                              _dptr(lo), _dptr(hi), int(N), _cartesian_task(task), float(eomg), float(ev), float(damping),
                                              int(max_iters), float(max_joint_step), float(margin), float(tol), int(max_steps),
                                              _p(d_workspace), ctypes.c_size_t(int(workspace_bytes)), int(max_blocks), _p(d_status),
                                              _p(d_reached), _p(d_span), _p(d_t), _p(d_clearance), _p(d_deviation_pos),
                                              _p(d_deviation_rot), _p(d_pose_error), _p(d_iterations), _p(d_evaluations), _p(d_q),
                                              _p(d_dq), _p(d_ddq), _p(d_span_status), _p(d_span_clearance)))

    def cartesian_path_arrays(self, model, collision, q_start, T_goal, lo, hi, N, margin, tol, *, task="full", eomg=1e-6, ev=1e-6,
                              damping=0.01, max_iters=20, max_joint_step=0.5, max_steps=64, want=None):
        """The same on host arrays (mp_cartesian_path_host_f64) through the context's pool, workspace included: a dict of the outputs
        named in `want` (default: all of CARTESIAN_OUTPUTS).  Its equality with the device form is held by
        tests/test_gpu_cartesian.py."""
        return _cartesian_path((self.handle,), self.lib.mp_cartesian_path_host_f64, model, collision, q_start, T_goal, lo, hi, N, margin,
                               tol, task, eomg, ev, damping, max_iters, max_joint_step, max_steps, want)

    def collision_set_world(self, collision, kinds, params):
        """Replaces the obstacle table of `collision` on this context's device, behind the launches already on its stream."""
        collision.set_world(kinds, params, ctx=self)

    def cartesian_trajectory(self, d_Xstart, d_Xend, B, N, Tf, method, d_pos, d_vel, d_acc, d_orient):
        _check(self.lib.mp_cartesian_trajectory_f32(self.handle, _p(d_Xstart), _p(d_Xend), int(B), int(N), float(Tf), int(method),
                                                    _p(d_pos), _p(d_vel), _p(d_acc), _p(d_orient)))

    def potential_field(self, d_positions, goal, d_obstacles, P, O, influence_distance, d_potential, d_gradient):
        goal = np.ascontiguousarray(goal, dtype=np.float32).reshape(3)
        _check(self.lib.mp_potential_field_f32(self.handle, _p(d_positions), _fptr(goal), _p(d_obstacles), int(P), int(O),
                                               float(influence_distance), _p(d_potential), _p(d_gradient)))

    # ---- hot path on host arrays (what the registry's gpu launchers call; synchronous)
    def id_trajectory_host(self, model: HipModel, q, qd, qdd, g=None, Ftip=None, dtype=np.float32, out=None) -> np.ndarray:
        """tau (rows, n) for host arrays.  `out`: optional C-contiguous array of q's shape and dtype to write into (a
        reused or page-locked buffer, see `pinned_empty`); a fresh array is allocated otherwise."""
        dtype = np.dtype(dtype)
        q = _as_c(q, dtype, name="q")
        if q.ndim != 2 or q.shape[1] != model.n:
            raise ValueError(f"q must be (rows, {model.n}), got {q.shape}")
        qd = _as_c(qd, dtype, q.shape, "qd")
        qdd = _as_c(qdd, dtype, q.shape, "qdd")
        tau = _out_or_new(out, q.shape, dtype)
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        if dtype == np.float32:
            _check(self.lib.mp_id_trajectory_host_f32(self.handle, model.handle, _fptr(q), _fptr(qd), _fptr(qdd),
                                                      q.shape[0], _dptr(g), _dptr(F), _fptr(tau)))
        else:
            _check(self.lib.mp_id_trajectory_host_f64(self.handle, model.handle, _dptr(q), _dptr(qd), _dptr(qdd),
                                                      q.shape[0], _dptr(g), _dptr(F), _dptr(tau)))
        return tau

    def batch_trajectory_host(self, model: HipModel, start, end, Tf, N, method):
        start = _as_c(start, np.float32, name="thetastart_batch")
        if start.ndim != 2 or start.shape[1] != model.n:
            raise ValueError(f"thetastart_batch must be (B, {model.n}), got {start.shape}")
        end = _as_c(end, np.float32, start.shape, "thetaend_batch")
        B = start.shape[0]
        out = [np.zeros((B, int(N), model.n), dtype=np.float32) for _ in range(3)]
        _check(self.lib.mp_batch_trajectory_host_f32(self.handle, model.handle, _fptr(start), _fptr(end), B, int(N),
                                                     float(Tf), int(method), _fptr(out[0]), _fptr(out[1]), _fptr(out[2])))
        return tuple(out)

    def traj_id_fused_host(self, model: HipModel, start, end, Tf, N, method, g=None, Ftip=None, out=None) -> np.ndarray:
        start = _as_c(start, np.float32, name="thetastart_batch")
        if start.ndim != 2 or start.shape[1] != model.n:
            raise ValueError(f"thetastart_batch must be (B, {model.n}), got {start.shape}")
        end = _as_c(end, np.float32, start.shape, "thetaend_batch")
        B = start.shape[0]
        tau = _out_or_new(out, (B, int(N), model.n), np.dtype(np.float32))
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(self.lib.mp_traj_id_fused_host_f32(self.handle, model.handle, _fptr(start), _fptr(end), B, int(N),
                                                  float(Tf), int(method), _dptr(g), _dptr(F), _fptr(tau)))
        return tau

    def fk_jac_id_host(self, model: HipModel, q, qd=None, qdd=None, g=None, Ftip=None, want_T=True, want_J=True, out_T=None,
                       out_J=None, out_tau=None):
        """(T (rows,4,4), J (rows,6,n), tau (rows,n)) float64; an output that was not asked for is None.  out_*: arrays to
        write into (reused or page-locked, see `pinned_empty`): with page-locked inputs and outputs a large call is chunked
        and its upload, kernels and download overlap."""
        q = _as_c(q, np.float64, name="q")
        if q.ndim != 2 or q.shape[1] != model.n:
            raise ValueError(f"q must be (rows, {model.n}), got {q.shape}")
        rows = q.shape[0]
        want_tau = qd is not None and qdd is not None
        qd = _as_c(qd, np.float64, q.shape, "qd") if want_tau else None
        qdd = _as_c(qdd, np.float64, q.shape, "qdd") if want_tau else None
        f64 = np.dtype(np.float64)
        T = _out_or_new(out_T, (rows, 4, 4), f64) if want_T else None
        J = _out_or_new(out_J, (rows, 6, model.n), f64) if want_J else None
        tau = _out_or_new(out_tau, (rows, model.n), f64) if want_tau else None
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(self.lib.mp_fk_jac_id_host_f64(self.handle, model.handle, _dptr(q), _dptr(qd), _dptr(qdd), rows,
                                              _dptr(g), _dptr(F), _dptr(T), _dptr(J), _dptr(tau)))
        return T, J, tau

    def cartesian_trajectory_host(self, Xstart, Xend, Tf, N, method):
        """B pose pairs (B,4,4) -> positions / velocities / accelerations (B,N,3), orientations (B,N,3,3), float32."""
        Xs = _as_c(Xstart, np.float64, name="Xstart")
        if Xs.ndim != 3 or Xs.shape[1:] != (4, 4):
            raise ValueError(f"Xstart must be (B, 4, 4), got {Xs.shape}")
        Xe = _as_c(Xend, np.float64, Xs.shape, "Xend")
        B, N = Xs.shape[0], int(N)
        pos, vel, acc = (np.zeros((B, N, 3), dtype=np.float32) for _ in range(3))
        ori = np.zeros((B, N, 3, 3), dtype=np.float32)
        _check(self.lib.mp_cartesian_trajectory_host_f32(self.handle, _dptr(Xs), _dptr(Xe), B, N, float(Tf), int(method),
                                                         _fptr(pos), _fptr(vel), _fptr(acc), _fptr(ori)))
        return pos, vel, acc, ori

    def potential_field_host(self, positions, goal, obstacles, influence_distance):
        """(potential (P,), gradient (P,3)) float32 for positions (P,3), goal (3,), obstacles (O,3)."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        goal = np.ascontiguousarray(goal, dtype=np.float32).reshape(3)
        obs = np.ascontiguousarray(obstacles, dtype=np.float32).reshape(-1, 3)
        P, O = pos.shape[0], obs.shape[0]
        pot, grad = np.zeros(P, dtype=np.float32), np.zeros((P, 3), dtype=np.float32)
        _check(self.lib.mp_potential_field_host_f32(self.handle, _fptr(pos), _fptr(goal), _fptr(obs) if O else None, P, O,
                                                    float(influence_distance), _fptr(pot), _fptr(grad)))
        return pot, grad

    def inverse_kinematics_host(self, model: HipModel, T_desired, theta0, joint_limits=None, eomg=1e-6, ev=1e-6,
                                max_iterations=10000, damping=2e-2, step_cap=0.3, weight_orientation=1.0, weight_position=1.0,
                                adaptive_tuning=False, backtracking=False, seed=1234):
        """B damped-least-squares IK problems in one launch: T_desired (B,4,4), theta0 (B,n) ->
        (theta (B,n) float64, success (B,) bool, iterations (B,) int32, restarts (B,) int32).
        joint_limits: (n,2) with +-inf / None for open ends, or None for no limits."""
        T = _as_c(T_desired, np.float64, name="T_desired")
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError(f"T_desired must be (B, 4, 4), got {T.shape}")
        B = T.shape[0]
        th0 = _as_c(theta0, np.float64, (B, model.n), "thetalist0")
        lim = None
        if joint_limits is not None:
            lim = np.array([[-np.inf if lo is None else lo, np.inf if hi is None else hi] for lo, hi in joint_limits], dtype=np.float64)
            if lim.shape != (model.n, 2):
                raise ValueError(f"joint_limits must be ({model.n}, 2), got {lim.shape}")
        th = np.zeros((B, model.n))
        ok, it, rs = (np.zeros(B, dtype=np.int32) for _ in range(3))
        _check(self.lib.mp_inverse_kinematics_host_f64(
            self.handle, model.handle, _dptr(T), _dptr(th0), B, _dptr(lim), float(eomg), float(ev), int(max_iterations), float(damping),
            float(step_cap), float(weight_orientation), float(weight_position), int(bool(adaptive_tuning)), int(bool(backtracking)),
            int(seed) & 0xFFFFFFFF, _dptr(th),
            ok.ctypes.data_as(_vp), it.ctypes.data_as(_vp), rs.ctypes.data_as(_vp)))
        return th, ok.astype(bool), it, rs

    def pd_regulation_host(self, model: HipModel, theta0, theta_des, Kp, Kd, g, dt, steps):
        """K closed-loop PD regulation runs in one launch (mp_pd_regulation_host_f64): theta0 / theta_des (K,n), Kp / Kd (K,) ->
        (errors (K,steps) float64 with NaN past each run's end, count (K,) int32)."""
        args = _pd_regulation_args(model, theta0, theta_des, Kp, Kd, g, steps)
        th0, des, kp, kd, gv, err, cnt = args
        _check(self.lib.mp_pd_regulation_host_f64(self.handle, model.handle, _dptr(th0), _dptr(des), _dptr(kp), _dptr(kd), th0.shape[0], _dptr(gv),
                                                  float(dt), int(steps), _dptr(err), cnt.ctypes.data_as(_vp)))
        return err, cnt

    def inverse_kinematics(self, model, d_T_desired, d_theta0, B, d_theta, d_success, d_iterations, d_restarts, joint_limits=None,
                           eomg=1e-6, ev=1e-6, max_iterations=10000, damping=2e-2, step_cap=0.3, weight_orientation=1.0,
                           weight_position=1.0, adaptive_tuning=False, backtracking=False, seed=1234):
        lim = None if joint_limits is None else np.ascontiguousarray(joint_limits, dtype=np.float64)
        _check(self.lib.mp_inverse_kinematics_f64(
            self.handle, model.handle, _p(d_T_desired), _p(d_theta0), int(B), _dptr(lim), float(eomg), float(ev), int(max_iterations),
            float(damping), float(step_cap), float(weight_orientation), float(weight_position), int(bool(adaptive_tuning)),
            int(bool(backtracking)), int(seed) & 0xFFFFFFFF, _p(d_theta),
            _p(d_success), _p(d_iterations), _p(d_restarts)))

    def mass_matrix_host(self, model: HipModel, q) -> np.ndarray:
        q = _as_c(q, np.float64, name="q")
        if q.ndim != 2 or q.shape[1] != model.n:
            raise ValueError(f"q must be (rows, {model.n}), got {q.shape}")
        M = np.zeros((q.shape[0], model.n, model.n))
        _check(self.lib.mp_mass_matrix_host_f64(self.handle, model.handle, _dptr(q), q.shape[0], _dptr(M)))
        return M

    def forward_dynamics_host(self, model: HipModel, q, qd, tau, g=None, Ftip=None) -> np.ndarray:
        q = _as_c(q, np.float64, name="q")
        if q.ndim != 2 or q.shape[1] != model.n:
            raise ValueError(f"q must be (rows, {model.n}), got {q.shape}")
        qd = _as_c(qd, np.float64, q.shape, "qd")
        tau = _as_c(tau, np.float64, q.shape, "tau")
        out = np.zeros_like(q)
        g = _vec_or_none(g, 3, "g")
        F = _vec_or_none(Ftip, 6, "Ftip")
        _check(self.lib.mp_forward_dynamics_host_f64(self.handle, model.handle, _dptr(q), _dptr(qd), _dptr(tau), q.shape[0],
                                                     _dptr(g), _dptr(F), _dptr(out)))
        return out

    def id_derivatives_host(self, model: HipModel, q, qd, qdd, g=None, Ftip=None):
        """(tau, dtau_dq, dtau_dqd, M) of (rows, n) host rows: [row, i, j] = d tau_i / d x_j; M = dtau_dqdd."""
        return _derivatives(self.lib.mp_id_derivatives_host_f64, (self.handle,), model, q, qd, qdd, g, Ftip, "qdd")

    def fd_derivatives_host(self, model: HipModel, q, qd, tau, g=None, Ftip=None):
        """(qdd, dqdd_dq, dqdd_dqd, Minv) of (rows, n) host rows: [row, i, j] = d qdd_i / d x_j; Minv = dqdd_dtau."""
        return _derivatives(self.lib.mp_fd_derivatives_host_f64, (self.handle,), model, q, qd, tau, g, Ftip, "tau")

    def id_vjp_host(self, model: HipModel, q, qd, qdd, gtau, g=None, Ftip=None):
        """(gq, gqd, gqdd = M gtau) of (rows, n) host rows and cotangents gtau."""
        return _vjp(self.lib.mp_id_vjp_host_f64, (self.handle,), model, q, qd, qdd, gtau, g, Ftip, False)

    def fd_vjp_host(self, model: HipModel, q, qd, tau, gqdd, g=None, Ftip=None):
        """(qdd, gq, gqd, gtau = M^-1 gqdd) of (rows, n) host rows and cotangents gqdd."""
        return _vjp(self.lib.mp_fd_vjp_host_f64, (self.handle,), model, q, qd, tau, gqdd, g, Ftip, True)

    def fk_jac_vjp_host(self, model: HipModel, q, gT=None, gJ=None, frame="space", want_T=False, want_J=False, want_gq=True):
        """(T (rows,4,4), J (rows,6,n) in `frame`, gq (rows,n)) of (rows, n) host rows and cotangents gT (rows,4,4) / gJ (rows,6,n)
        (None = 0); an output not asked for is None."""
        return _kin_vjp(self.lib.mp_fk_jac_vjp_host_f64, (self.handle,), model, frame, q, gT, gJ, want_T, want_J, want_gq)

    def opspace_host(self, model: HipModel, q, qd, g=None, frame="hybrid", task="full", damping=0.0, want=OPSPACE_OUTPUTS):
        """Operational-space dynamics of (rows, n) host rows: a dict of the outputs named in `want` (OPSPACE_OUTPUTS)."""
        return _opspace(self.lib.mp_opspace_host_f64, (self.handle,), model, frame, task, damping, q, qd, g, want)

    def opspace_torque_host(self, model: HipModel, q, qd, acc, g=None, tau0=None, frame="hybrid", task="full", damping=0.0):
        """tau (rows, n) for the task accelerations acc (rows, m) and the null-space torques tau0 (rows, n) or None."""
        return _opspace_torque(self.lib.mp_opspace_torque_host_f64, (self.handle,), model, frame, task, damping, q, qd, acc, tau0, g)

    def fd_trajectory_host(self, model: HipModel, theta0, dtheta0, taumat, g, Ftipmat, dt, intRes, dtype=np.float64,
                           layout: str = "batch_major", device_layout: str | None = None, out=None):
        """B trajectories: theta0/dtheta0 (B,n), taumat (B,N,n), Ftipmat (B,N,6) or None -> 3 x (B,N,n) float32.

        `out`: optional triple of C-contiguous float32 arrays of the result's shape to write into.  With page-locked inputs AND
        outputs (`pinned_empty`) a batch-major call is cut into chunks of whole trajectories whose upload, roll-out and download
        overlap (csrc/mp_capi.cpp, fdtraj_host_impl).

        layout="time_major": the HOST arrays are (N,B,n) / (N,B,6) and so are the results.  device_layout selects the kernel
        ("batch_major": 4-step LDS tiles on (B,N,n); "time_major": whole lines per step on (N,B,n)); when it differs from the
        host layout the arrays are converted on the device (mp_transpose_rows).  Default: the host layout's own kernel."""
        if layout not in ("batch_major", "time_major") or device_layout not in (None, "batch_major", "time_major"):
            raise ValueError("layout / device_layout must be 'batch_major' or 'time_major'")
        dtype = np.dtype(dtype)
        th = _as_c(theta0, dtype, name="thetalist")
        if th.ndim != 2 or th.shape[1] != model.n:
            raise ValueError(f"thetalist must be (B, {model.n}), got {th.shape}")
        B, n = th.shape
        dth = _as_c(dtheta0, dtype, th.shape, "dthetalist")
        tm = _as_c(taumat, dtype, name="taumat")
        bax = 0 if layout == "batch_major" else 1
        if tm.ndim != 3 or tm.shape[bax] != B or tm.shape[2] != n:
            raise ValueError(f"taumat must be {'(B, N, %d)' % n if bax == 0 else '(N, B, %d)' % n}, got {tm.shape}")
        N = tm.shape[1 - bax]
        Fm = None if Ftipmat is None else _as_c(Ftipmat, dtype, tm.shape[:2] + (6,), "Ftipmat")
        g = _vec_or_none(g, 3, "g")
        if out is None:
            out = [np.zeros(tm.shape[:2] + (n,), dtype=np.float32) for _ in range(3)]
        else:
            out = [_out_or_new(o, tm.shape[:2] + (n,), np.dtype(np.float32)) for o in out]
            if len(out) != 3:
                raise ValueError("out must hold three arrays (positions, velocities, accelerations)")
        if layout == "batch_major" and device_layout in (None, "batch_major"):
            if dtype == np.float32:
                fn, ptr = self.lib.mp_fd_trajectory_host_f32, _fptr
            else:
                fn, ptr = self.lib.mp_fd_trajectory_host_f64, _dptr
            _check(fn(self.handle, model.handle, ptr(th), ptr(dth), ptr(tm), ptr(Fm), B, N, _dptr(g), float(dt), int(intRes),
                      _fptr(out[0]), _fptr(out[1]), _fptr(out[2])))
            return tuple(out)
        if B == 0 or N == 0:
            return tuple(out)
        dev_tm = (device_layout or layout) == "time_major"
        convert = dev_tm != (layout == "time_major")
        outer, inner = tm.shape[0], tm.shape[1]      # of the host arrays
        bufs = []
        try:
            def up(a):
                bufs.append(self.to_device(a))
                return bufs[-1]

            def flip(d, row_bytes, o, i):
                bufs.append(self.alloc(o * i * row_bytes))
                self.transpose_rows(d, o, i, row_bytes, bufs[-1])
                return bufs[-1]

            d_th, d_dth, d_tau = up(th), up(dth), up(tm)
            d_F = up(Fm) if Fm is not None else None
            if convert:
                d_tau = flip(d_tau, n * dtype.itemsize, outer, inner)
                d_F = flip(d_F, 6 * dtype.itemsize, outer, inner) if d_F is not None else None
            d_out = [self.alloc(B * N * n * 4) for _ in range(3)]
            bufs.extend(d_out)
            self.fd_trajectory(model, d_th, d_dth, d_tau, d_F, B, N, g, dt, intRes, *d_out, dtype=dtype, time_major=dev_tm)
            for k in range(3):
                src = flip(d_out[k], n * 4, inner, outer) if convert else d_out[k]
                _check(self.lib.mp_memcpy_d2h(self.handle, out[k].ctypes.data, _p(src), out[k].nbytes))
        finally:
            for b in bufs:
                b.free()
        return tuple(out)

    def id_regressor(self, model, d_q, d_qd, d_qdd, rows, d_Y, d_tau_ext=None, g=None, Ftip=None):
        """Inverse-dynamics regressor on device buffers (float64, csrc/mp_regressor.h): Y (rows, n, 10n), tau_ext (rows, n) or None.
        Asynchronous (capturable)."""
        _check(self.lib.mp_id_regressor_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), int(rows),
                                            _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_Y), _p(d_tau_ext)))

    def id_regressor_normal(self, model, d_q, d_qd, d_qdd, d_rhs, rows, d_work, d_A, d_b, d_rr, g=None, Ftip=None):
        """Normal equations of the regressor on device buffers: A = sum Y^T Y (10n, 10n; d_A may be None), b = sum Y^T (rhs - tau_ext),
        rr = sum |rhs - tau_ext|^2; d_work holds id_regressor_normal_workspace_bytes(model, rows).  Asynchronous (capturable)."""
        _check(self.lib.mp_id_regressor_normal_f64(self.handle, model.handle, _p(d_q), _p(d_qd), _p(d_qdd), _p(d_rhs), int(rows),
                                                   _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_work),
                                                   _p(d_A), _p(d_b), _p(d_rr)))

    def id_regressor_host(self, model: HipModel, q, qd, qdd, g=None, Ftip=None):
        """(Y (rows, n, 10n), tau_ext (rows, n)) of (rows, n) host rows."""
        q, qd, qdd = _regressor_rows(model, q, qd, qdd)
        Y, te = np.empty((q.shape[0], model.n, 10 * model.n)), np.empty(q.shape)
        _check(self.lib.mp_id_regressor_host_f64(self.handle, model.handle, _dptr(q), _dptr(qd), _dptr(qdd), q.shape[0],
                                                 _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(Y), _dptr(te)))
        return Y, te

    def id_regressor_normal_host(self, model: HipModel, q, qd, qdd, rhs, g=None, Ftip=None, want_A: bool = True):
        """(A (10n, 10n) or None, b (10n), rr) of (rows, n) host rows."""
        q, qd, qdd, rhs = _regressor_rows(model, q, qd, qdd, rhs)
        w = 10 * model.n
        A, b, rr = (np.empty((w, w)) if want_A else None), np.empty(w), np.empty(1)
        _check(self.lib.mp_id_regressor_normal_host_f64(self.handle, model.handle, _dptr(q), _dptr(qd), _dptr(qdd), _dptr(rhs), q.shape[0],
                                                        _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(A),
                                                        _dptr(b), _dptr(rr)))
        return A, b, float(rr[0])

    def fd_trajectory_vjp(self, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes, d_gpos, d_gvel, d_gacc, d_work,
                          d_gtheta0, d_gdtheta0, d_gtaumat):
        """Gradients of the roll-out on device buffers (float64, csrc/mp_rollout_vjp.h), time-major taumat / Ftipmat / cotangents /
        d_gtaumat (N, B, *); d_Ftipmat and the cotangents may be None; d_work holds fd_trajectory_vjp_workspace_bytes(...).
        Asynchronous (capturable)."""
        _check(self.lib.mp_fd_trajectory_vjp_tm_f64(self.handle, model.handle, _p(d_theta0), _p(d_dtheta0), _p(d_taumat), _p(d_Ftipmat),
                                                    int(B), int(N), _dptr(_vec_or_none(g, 3, "g")), float(dt), int(intRes), _p(d_gpos),
                                                    _p(d_gvel), _p(d_gacc), _p(d_work), _p(d_gtheta0), _p(d_gdtheta0), _p(d_gtaumat)))

    def fd_trajectory_vjp_host(self, model: HipModel, theta0, dtheta0, taumat, g, Ftipmat, dt, intRes, gpos=None, gvel=None, gacc=None,
                               layout: str = "batch_major"):
        """(dL/dtheta0 (B,n), dL/ddtheta0 (B,n), dL/dtaumat) of host arrays, float64.  layout="batch_major": taumat / Ftipmat /
        cotangents / dL/dtaumat are (B,N,*) and go through mp_fd_trajectory_vjp_host_f64 (converted on the device, chunked);
        "time_major": they are (N,B,*) and go straight to the device form."""
        th, dth, tm, Fm, G = _vjp_arrays(model, theta0, dtheta0, taumat, Ftipmat, gpos, gvel, gacc, layout)
        gv3 = _vec_or_none(g, 3, "g")
        B, n = th.shape
        N = tm.shape[1] if layout == "batch_major" else tm.shape[0]
        gth, gdth, gtau = np.zeros((B, n)), np.zeros((B, n)), np.zeros(tm.shape)
        if layout == "batch_major":
            _check(self.lib.mp_fd_trajectory_vjp_host_f64(self.handle, model.handle, _dptr(th), _dptr(dth), _dptr(tm), _dptr(Fm), B, N,
                                                          _dptr(gv3), float(dt), int(intRes), *[_dptr(x) for x in G], _dptr(gth),
                                                          _dptr(gdth), _dptr(gtau)))
            return gth, gdth, gtau
        work = fd_trajectory_vjp_workspace_bytes(model, B, N, intRes)
        if B == 0 or N == 0:
            return gth, gdth, gtau
        bufs = []
        try:
            def up(a):
                bufs.append(self.to_device(a) if a is not None else None)
                return bufs[-1]

            d_in = [up(a) for a in (th, dth, tm, Fm)] + [up(x) for x in G]
            d_out = [self.alloc(a.nbytes) for a in (gth, gdth, gtau)]
            bufs.extend(d_out)
            bufs.append(self.alloc(work))
            self.fd_trajectory_vjp(model, d_in[0], d_in[1], d_in[2], d_in[3], B, N, gv3, dt, intRes, d_in[4], d_in[5], d_in[6], bufs[-1],
                                   *d_out)
            for a, d in zip((gth, gdth, gtau), d_out):
                _check(self.lib.mp_memcpy_d2h(self.handle, a.ctypes.data, _p(d), a.nbytes))
        finally:
            for b in bufs:
                if b is not None:
                    b.free()
        return gth, gdth, gtau

    def ilqr_backward(self, model, d_pos, d_vel, d_taumat, d_dq, d_dqd, d_Minv, d_xref, wq, wr, wf, d_reg, B, N, dt, d_work, d_K, d_k,
                      d_dV, d_status):
        """The Riccati backward pass on device buffers (float64, csrc/mp_ilqr.h), time-major pos / vel / taumat (N, B, n), xref
        (N, B, 2n), the blocks of mp_fd_derivatives_f64 over the (N - 1) B rows (pos[0:N-1], vel[0:N-1], taumat[1:N]), reg (B); writes
        K (N, B, n, 2n), k (N, B, n), dV (B, 2), status (B) int32; d_work holds ilqr_backward_workspace_bytes(model, B, N) (0: may be None).
        Asynchronous (capturable)."""
        wq, wr, wf = _ilqr_weights(model, wq, wr, wf)
        _check(self.lib.mp_ilqr_backward_tm_f64(self.handle, model.handle, _p(d_pos), _p(d_vel), _p(d_taumat), _p(d_dq), _p(d_dqd),
                                                _p(d_Minv), _p(d_xref), _dptr(wq), _dptr(wr), _dptr(wf), _p(d_reg), int(B), int(N),
                                                float(dt), _p(d_work), _p(d_K), _p(d_k), _p(d_dV), _p(d_status)))

    def ilqr_rollout(self, model, d_theta0, d_dtheta0, d_taumat, d_pos, d_vel, d_K, d_k, d_alpha, d_xref, wq, wr, wf, A, B, N, g, dt,
                     d_cost, d_opos=None, d_ovel=None, d_otau=None):
        """The closed-loop roll-out on device buffers: A B lanes, alpha / cost (A, B), the float64 rows (N, A B, n) when the three
        outputs are given; d_K / d_k (and then d_pos / d_vel) may be None for the open loop.  Asynchronous (capturable)."""
        wq, wr, wf = _ilqr_weights(model, wq, wr, wf)
        _check(self.lib.mp_ilqr_rollout_tm_f64(self.handle, model.handle, _p(d_theta0), _p(d_dtheta0), _p(d_taumat), _p(d_pos), _p(d_vel),
                                               _p(d_K), _p(d_k), _p(d_alpha), _p(d_xref), _dptr(wq), _dptr(wr), _dptr(wf), int(A), int(B),
                                               int(N), _dptr(_vec_or_none(g, 3, "g")), float(dt), _p(d_cost), _p(d_opos), _p(d_ovel),
                                               _p(d_otau)))

    def ilqr_backward_host(self, model: HipModel, pos, vel, taumat, xref, wq, wr, wf, reg, g, dt):
        """(K (B, N, n, 2n), k (B, N, n), dV (B, 2), status (B) int32) of batch-major host arrays; the derivative launch is part of it."""
        return _ilqr_backward(self.lib.mp_ilqr_backward_host_f64, (self.handle,), model, pos, vel, taumat, xref, wq, wr, wf, reg, g, dt)

    def ilqr_rollout_host(self, model: HipModel, theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref, wq, wr, wf, g, dt, want_rows=True):
        """(cost (A, B), pos, vel, tau (A, B, N, n) or None) of batch-major host arrays; alpha (A, B); K / k may be None."""
        return _ilqr_rollout(self.lib.mp_ilqr_rollout_host_f64, (self.handle,), model, theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref,
                             wq, wr, wf, g, dt, want_rows)

    def path_dynamics(self, model, d_q, d_dq, d_ddq, rows, velocity_limits, d_a, d_b, d_c, d_xbar, g=None, Ftip=None):
        """The path-dynamics coefficients on device rows in any layout (float64, csrc/mp_toppra.h): tau = a sdd + b sd^2 + c per row and
        xbar = min_j (vmax_j / |q'_j|)^2.  Asynchronous (capturable)."""
        _check(self.lib.mp_path_dynamics_f64(self.handle, model.handle, _p(d_q), _p(d_dq), _p(d_ddq), int(rows),
                                             _dptr(_as_c(velocity_limits, np.float64, (model.n,), "velocity_limits")),
                                             _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _p(d_a), _p(d_b), _p(d_c),
                                             _p(d_xbar)))

    def toppra(self, model, d_a, d_b, d_c, d_xbar, d_dq, d_ddq, torque_limits, acceleration_limits, d_sd_start, d_sd_end, B, N, d_K, d_x,
               d_u, d_t, d_duration, d_status, d_qd=None, d_qdd=None, d_tau=None):
        """The backward and forward sweep on time-major device buffers: a / b / c / dq / ddq (N, B, n), xbar (N, B), sd_start / sd_end (B)
        -> K (N, B, 2), x / u / t (N, B), duration (B), status (B) int32 and, when given, the rows qd / qdd / tau (N, B, n).
        Asynchronous, allocates nothing (capturable)."""
        tl, al = _toppra_limits(model.n, torque_limits, acceleration_limits)
        _check(self.lib.mp_toppra_tm_f64(self.handle, model.handle, _p(d_a), _p(d_b), _p(d_c), _p(d_xbar), _p(d_dq), _p(d_ddq), _dptr(tl),
                                         _dptr(al), _p(d_sd_start), _p(d_sd_end), int(B), int(N), _p(d_K), _p(d_x), _p(d_u), _p(d_t),
                                         _p(d_duration), _p(d_status), _p(d_qd), _p(d_qdd), _p(d_tau)))

    def toppra_host(self, model: HipModel, q, dq, ddq, velocity_limits, torque_limits=None, acceleration_limits=None, sd_start=0.0,
                    sd_end=0.0, g=None, Ftip=None, want_rows=True):
        """Time-optimal parameterisation of batch-major host paths q / dq / ddq (B, N, n): the dict of _toppra_call."""
        return _toppra_call(self.lib.mp_toppra_host_f64, (self.handle,), model, q, dq, ddq, velocity_limits, torque_limits,
                            acceleration_limits, sd_start, sd_end, g, Ftip, want_rows)

    def fd_trajectory(self, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes, d_pos, d_vel, d_acc,
                      dtype=np.float32, time_major: bool = False):
        """Device pointers.  time_major=False: taumat (B,N,n), Ftipmat (B,N,6), outputs (B,N,n); True: (N,B,*) throughout."""
        f32 = np.dtype(dtype) == np.float32
        if time_major:
            fn = self.lib.mp_fd_trajectory_tm_f32 if f32 else self.lib.mp_fd_trajectory_tm_f64
        else:
            fn = self.lib.mp_fd_trajectory_f32 if f32 else self.lib.mp_fd_trajectory_f64
        g = _vec_or_none(g, 3, "g")
        _check(fn(self.handle, model.handle, _p(d_theta0), _p(d_dtheta0), _p(d_taumat), _p(d_Ftipmat), int(B), int(N), _dptr(g),
                  float(dt), int(intRes), _p(d_pos), _p(d_vel), _p(d_acc)))

    def transpose_rows(self, d_src, outer, inner, row_bytes, d_dst):
        """d_dst (inner, outer, row_bytes) <- d_src (outer, inner, row_bytes), on the device."""
        _check(self.lib.mp_transpose_rows(self.handle, _p(d_src), int(outer), int(inner), int(row_bytes), _p(d_dst)))

    # ---- RCCL
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES)()
        _check(load_library().mp_comm_unique_id(buf))
        return bytes(buf)

    def comm_create(self, unique_id: bytes, nranks: int, rank: int) -> "HipComm":
        return HipComm(self, unique_id, nranks, rank)


# --------------------------------------------------------------------------- CPU twins (csrc/mp_cpu.cpp)
# Host arrays in, host arrays out, no context: the registry's cpu_launchers (reference cuda_kernels/registry.py:85-89).
def _ptr(a, dtype):
    if a is None:
        return None
    return a.ctypes.data_as(_c_fp if dtype == np.float32 else _c_dp)


def cpu_id_trajectory(model: "HipModel", q, qd, qdd, g=None, Ftip=None, dtype=np.float32, nthreads: int = 0) -> np.ndarray:
    lib = load_library()
    q = _as_c(q, dtype, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    qd, qdd = _as_c(qd, dtype, q.shape, "qd"), _as_c(qdd, dtype, q.shape, "qdd")
    tau = np.empty_like(q)
    fn = lib.mp_id_trajectory_cpu_f32 if dtype == np.float32 else lib.mp_id_trajectory_cpu_f64
    _check(fn(model.handle, _ptr(q, dtype), _ptr(qd, dtype), _ptr(qdd, dtype), q.shape[0], _dptr(_vec_or_none(g, 3, "g")),
              _dptr(_vec_or_none(Ftip, 6, "Ftip")), _ptr(tau, dtype), int(nthreads)))
    return tau


def cpu_id_row_precision(model: "HipModel", q, qd, qdd, g=None, Ftip=None, nthreads: int = 0) -> np.ndarray:
    """(rows,) bool: the rows the float32 inverse-dynamics kernels evaluate in float64 (ill-conditioned rows, csrc/mp_core.h)."""
    lib = load_library()
    q = _as_c(q, np.float32, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    rows = q.shape[0]
    qd, qdd = _as_c(qd, np.float32, q.shape, "qd"), _as_c(qdd, np.float32, q.shape, "qdd")
    out = np.zeros(rows, dtype=np.uint8)
    _check(lib.mp_id_row_precision_cpu_f32(model.handle, _ptr(q, np.float32), _ptr(qd, np.float32), _ptr(qdd, np.float32), rows,
                                           _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")),
                                           out.ctypes.data_as(_vp), nthreads))
    return out.astype(bool)


def cpu_fk_jac_id(model: "HipModel", q, qd=None, qdd=None, g=None, Ftip=None, want_T=True, want_J=True, nthreads: int = 0):
    lib = load_library()
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    rows, n = q.shape
    want_tau = qd is not None and qdd is not None
    qd = _as_c(qd, np.float64, q.shape, "qd") if want_tau else None
    qdd = _as_c(qdd, np.float64, q.shape, "qdd") if want_tau else None
    T = np.empty((rows, 4, 4)) if want_T else None
    J = np.empty((rows, 6, n)) if want_J else None
    tau = np.empty((rows, n)) if want_tau else None
    if not (want_T or want_J or want_tau):
        raise ValueError("at least one output is required")
    _check(lib.mp_fk_jac_id_cpu_f64(model.handle, _dptr(q), _dptr(qd), _dptr(qdd), rows, _dptr(_vec_or_none(g, 3, "g")),
                                    _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(T), _dptr(J), _dptr(tau), int(nthreads)))
    return T, J, tau


def cpu_mass_matrix(model: "HipModel", q, nthreads: int = 0) -> np.ndarray:
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    M = np.empty((q.shape[0], model.n, model.n))
    _check(load_library().mp_mass_matrix_cpu_f64(model.handle, _dptr(q), q.shape[0], _dptr(M), int(nthreads)))
    return M


def cpu_forward_dynamics(model: "HipModel", q, qd, tau, g=None, Ftip=None, nthreads: int = 0) -> np.ndarray:
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    qd, tau = _as_c(qd, np.float64, q.shape, "qd"), _as_c(tau, np.float64, q.shape, "tau")
    out = np.empty_like(q)
    _check(load_library().mp_forward_dynamics_cpu_f64(model.handle, _dptr(q), _dptr(qd), _dptr(tau), q.shape[0],
                                                      _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(out),
                                                      int(nthreads)))
    return out


def _derivatives(fn, lead, model, q, qd, x, g, Ftip, xname, nthreads=None):
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    qd, x = _as_c(qd, np.float64, q.shape, "qd"), _as_c(x, np.float64, q.shape, xname)
    rows, n = q.shape
    y = np.empty_like(q)
    dq, dqd, mat = np.empty((rows, n, n)), np.empty((rows, n, n)), np.empty((rows, n, n))
    args = list(lead) + [model.handle, _dptr(q), _dptr(qd), _dptr(x), rows, _dptr(_vec_or_none(g, 3, "g")),
                         _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(y), _dptr(dq), _dptr(dqd), _dptr(mat)]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return y, dq, dqd, mat


def cpu_id_derivatives(model: "HipModel", q, qd, qdd, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.id_derivatives_host: (tau, dtau_dq, dtau_dqd, M)."""
    return _derivatives(load_library().mp_id_derivatives_cpu_f64, (), model, q, qd, qdd, g, Ftip, "qdd", nthreads)


def cpu_fd_derivatives(model: "HipModel", q, qd, tau, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.fd_derivatives_host: (qdd, dqdd_dq, dqdd_dqd, Minv)."""
    return _derivatives(load_library().mp_fd_derivatives_cpu_f64, (), model, q, qd, tau, g, Ftip, "tau", nthreads)


def _vjp(fn, lead, model, q, qd, x, cot, g, Ftip, fd, nthreads=None):
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    qd = _as_c(qd, np.float64, q.shape, "qd")
    x = _as_c(x, np.float64, q.shape, "tau" if fd else "qdd")
    cot = _as_c(cot, np.float64, q.shape, "gqdd" if fd else "gtau")
    rows = q.shape[0]
    out = [np.empty_like(q) for _ in range(4 if fd else 3)]
    args = list(lead) + [model.handle, _dptr(q), _dptr(qd), _dptr(x), _dptr(cot), rows, _dptr(_vec_or_none(g, 3, "g")),
                         _dptr(_vec_or_none(Ftip, 6, "Ftip"))] + [_dptr(o) for o in out]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return tuple(out)


def cpu_id_vjp(model: "HipModel", q, qd, qdd, gtau, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.id_vjp_host: (gq, gqd, gqdd)."""
    return _vjp(load_library().mp_id_vjp_cpu_f64, (), model, q, qd, qdd, gtau, g, Ftip, False, nthreads)


def cpu_fd_vjp(model: "HipModel", q, qd, tau, gqdd, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.fd_vjp_host: (qdd, gq, gqd, gtau)."""
    return _vjp(load_library().mp_fd_vjp_cpu_f64, (), model, q, qd, tau, gqdd, g, Ftip, True, nthreads)


def _frame_code(frame) -> int:
    if frame in ("space", 0):
        return 0
    if frame in ("body", 1):
        return 1
    raise ValueError(f"frame must be 'space' or 'body', got {frame!r}")


def _kin_vjp(fn, lead, model, frame, q, gT, gJ, want_T, want_J, want_gq, nthreads=None):
    code = _frame_code(frame)
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    rows, n = q.shape
    gT = None if gT is None else _as_c(gT, np.float64, (rows, 4, 4), "gT")
    gJ = None if gJ is None else _as_c(gJ, np.float64, (rows, 6, n), "gJ")
    T = np.empty((rows, 4, 4)) if want_T else None
    J = np.empty((rows, 6, n)) if want_J else None
    gq = np.empty((rows, n)) if want_gq else None
    args = list(lead) + [model.handle, code, _dptr(q), _dptr(gT), _dptr(gJ), rows, _dptr(T), _dptr(J), _dptr(gq)]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return T, J, gq


def cpu_fk_jac_vjp(model: "HipModel", q, gT=None, gJ=None, frame="space", want_T=False, want_J=False, want_gq=True, nthreads: int = 0):
    """CPU twin of HipContext.fk_jac_vjp_host: (T, J, gq), None where not asked for."""
    return _kin_vjp(load_library().mp_fk_jac_vjp_cpu_f64, (), model, frame, q, gT, gJ, want_T, want_J, want_gq, nthreads)


def _opspace_frame(frame) -> int:
    if frame in _OPSPACE_FRAMES:
        return _OPSPACE_FRAMES[frame]
    if frame in (0, 1, 2) and not isinstance(frame, bool):
        return int(frame)
    raise ValueError(f"frame must be 'space', 'body' or 'hybrid', got {frame!r}")


def _opspace_task(task) -> int:
    if task in _OPSPACE_TASKS:
        return _OPSPACE_TASKS[task]
    if task in (0, 1, 2) and not isinstance(task, bool):
        return int(task)
    raise ValueError(f"task must be 'full', 'linear' or 'angular', got {task!r}")


def _opspace_rows(model, q, qd):
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    return q, _as_c(qd, np.float64, q.shape, "qd")


def _opspace(fn, lead, model, frame, task, damping, q, qd, g, want, nthreads=None):
    fc, tc = _opspace_frame(frame), _opspace_task(task)
    q, qd = _opspace_rows(model, q, qd)
    unknown = [w for w in want if w not in OPSPACE_OUTPUTS]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {OPSPACE_OUTPUTS}; got {tuple(want)!r}")
    rows, n = q.shape
    m = 6 if tc == 0 else 3
    shapes = {"T": (rows, 4, 4), "J": (rows, m, n), "Jdot_qd": (rows, m), "Lambda": (rows, m, m), "Jbar": (rows, n, m), "mu": (rows, m),
              "p": (rows, m)}
    out = {k: (np.empty(shapes[k]) if k in want else None) for k in OPSPACE_OUTPUTS}
    args = list(lead) + [model.handle, fc, tc, float(damping), _dptr(q), _dptr(qd), rows, _dptr(_vec_or_none(g, 3, "g"))]
    args += [_dptr(out[k]) for k in OPSPACE_OUTPUTS]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return {k: v for k, v in out.items() if v is not None}


def _opspace_torque(fn, lead, model, frame, task, damping, q, qd, acc, tau0, g, nthreads=None):
    fc, tc = _opspace_frame(frame), _opspace_task(task)
    q, qd = _opspace_rows(model, q, qd)
    rows = q.shape[0]
    acc = _as_c(acc, np.float64, (rows, 6 if tc == 0 else 3), "acc")
    tau0 = None if tau0 is None else _as_c(tau0, np.float64, q.shape, "tau0")
    tau = np.empty(q.shape)
    args = list(lead) + [model.handle, fc, tc, float(damping), _dptr(q), _dptr(qd), _dptr(acc), _dptr(tau0), rows,
                         _dptr(_vec_or_none(g, 3, "g")), _dptr(tau)]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return tau


def cpu_opspace(model: "HipModel", q, qd, g=None, frame="hybrid", task="full", damping=0.0, want=OPSPACE_OUTPUTS, nthreads: int = 0):
    """CPU twin of HipContext.opspace_host."""
    return _opspace(load_library().mp_opspace_cpu_f64, (), model, frame, task, damping, q, qd, g, want, nthreads)


def cpu_opspace_torque(model: "HipModel", q, qd, acc, g=None, tau0=None, frame="hybrid", task="full", damping=0.0, nthreads: int = 0):
    """CPU twin of HipContext.opspace_torque_host."""
    return _opspace_torque(load_library().mp_opspace_torque_cpu_f64, (), model, frame, task, damping, q, qd, acc, tau0, g, nthreads)


COLLISION_OUTPUTS = ("dist_world", "arg_world", "dist_self", "arg_self", "grad_dist_world", "grad_dist_self", "cost", "grad")
OBSTACLE_SPHERE, OBSTACLE_CAPSULE, OBSTACLE_BOX = 0, 1, 2
MP_COLLISION_MAX_SPHERES = 64


class HipCollision:
    """Sphere collision model of one robot (mp_collision_create).  Host-only object: no GPU needed to build one.  links (S) in 0..n,
    centres (S,3) in the space frame at q = 0, radii (S), pairs (P,2) of sphere indices."""

    def __init__(self, model: "HipModel", links, centres, radii, pairs=None):
        self.lib = load_library()
        self.handle = None
        lk = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
        S = lk.shape[0]
        c = _as_c(centres, np.float64, (S, 3), "centres")
        r = _as_c(radii, np.float64, (S,), "radii")
        pr = np.zeros((0, 2), dtype=np.int32) if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        p = _vp()
        _check(self.lib.mp_collision_create(model.handle, S, lk.ctypes.data_as(_vp), _dptr(c), _dptr(r), pr.shape[0],
                                            pr.ctypes.data_as(_vp) if pr.shape[0] else None, ctypes.byref(p)))
        self.handle = p
        self.n, self.S, self.P = model.n, S, pr.shape[0]

    def set_world(self, kinds, params, ctx: Optional["HipContext"] = None) -> None:
        """kinds (O) of OBSTACLE_*, params (O,16).  ctx=None sets the world the CPU twin reads; with a context the table is also copied
        to its device."""
        kd = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32).reshape(-1))
        O = kd.shape[0]
        pm = _as_c(np.zeros((0, 16)) if O == 0 else params, np.float64, (O, 16), "params")
        _check(self.lib.mp_collision_set_world(None if ctx is None else ctx.handle, self.handle, O, kd.ctypes.data_as(_vp) if O else None,
                                               _dptr(pm) if O else None))

    def set_cloud(self, points, radius: float, d_max: float, cell: float = 0.0, ctx: Optional["HipContext"] = None) -> None:
        """points (M,3) with one radius and the truncation distance d_max; M = 0 removes the cloud; cell <= 0: d_max + radius.  ctx=None
        sets the cloud the CPU twin reads; with a context its grid is also copied to the device."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        M = pts.shape[0]
        _check(self.lib.mp_collision_set_cloud(None if ctx is None else ctx.handle, self.handle, M, _dptr(pts) if M else None,
                                               float(radius), float(d_max), float(cell)))

    def cloud_info(self) -> dict:
        """{"M", "radius", "d_max", "cell", "dims"} of the cloud the CPU twin reads (M = 0: none)."""
        M, r, d, c = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        dims = (ctypes.c_int32 * 3)()
        _check(self.lib.mp_collision_cloud_info(self.handle, ctypes.byref(M), ctypes.byref(r), ctypes.byref(d), ctypes.byref(c), dims))
        return {"M": int(M.value), "radius": r.value, "d_max": d.value, "cell": c.value, "dims": tuple(int(v) for v in dims)}

    def motion_bounds(self) -> np.ndarray:
        """rho (n, n + 1): row j - 1, column k = the largest distance of a sphere centre of link k from the axis of revolute joint j."""
        rho = np.zeros((self.n, self.n + 1))
        _check(self.lib.mp_collision_motion_bounds(self.handle, _dptr(rho)))
        return rho

    def destroy(self) -> None:
        if getattr(self, "handle", None) is not None:
            self.lib.mp_collision_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _collision(lead, fn, model, collision, q, eps_world, eps_self, want, nthreads=None):
    want = COLLISION_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in COLLISION_OUTPUTS:
            raise ValueError(f"unknown collision output {w!r}; choose from {COLLISION_OUTPUTS}")
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    rows, n = q.shape
    shapes = {"dist_world": (rows,), "arg_world": (rows, 2), "dist_self": (rows,), "arg_self": (rows, 2), "grad_dist_world": (rows, n),
              "grad_dist_self": (rows, n), "cost": (rows,), "grad": (rows, n)}
    out = {w: np.empty(shapes[w], dtype=np.int32 if w.startswith("arg") else np.float64) for w in want}
    ptrs = []
    for w in COLLISION_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (a.ctypes.data_as(_vp) if w.startswith("arg") else _dptr(a)))
    args = list(lead) + [model.handle, collision.handle, _dptr(q), rows, float(eps_world), float(eps_self)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_collision(model: "HipModel", collision: "HipCollision", q, eps_world, eps_self, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.collision_host."""
    return _collision((), load_library().mp_collision_cpu_f64, model, collision, q, eps_world, eps_self, want, nthreads)


EDGE_OUTPUTS = ("status", "t", "steps", "clearance", "witness")
EDGE_FREE, EDGE_BLOCKED, EDGE_UNDECIDED, EDGE_INVALID = 0, 1, 2, -1


def _collision_edges(lead, fn, model, collision, q_from, q_to, margin, tol, max_steps, want, nthreads=None):
    want = EDGE_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in EDGE_OUTPUTS:
            raise ValueError(f"unknown edge output {w!r}; choose from {EDGE_OUTPUTS}")
    qa = _as_c(q_from, np.float64, name="q_from")
    if qa.ndim != 2 or qa.shape[1] != model.n:
        raise ValueError(f"q_from must be (edges, {model.n}); got {qa.shape}")
    E = qa.shape[0]
    qb = _as_c(q_to, np.float64, (E, model.n), "q_to")
    shapes = {"status": (E,), "t": (E,), "steps": (E,), "clearance": (E,), "witness": (E, 3)}
    out = {w: np.empty(shapes[w], dtype=np.float64 if w in ("t", "clearance") else np.int32) for w in want}
    ptrs = []
    for w in EDGE_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (_dptr(a) if w in ("t", "clearance") else a.ctypes.data_as(_vp)))
    args = list(lead) + [model.handle, collision.handle, _dptr(qa), _dptr(qb), E, float(margin), float(tol), int(max_steps)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_collision_edges(model: "HipModel", collision: "HipCollision", q_from, q_to, margin, tol, max_steps, want=None,
                        nthreads: int = 0) -> dict:
    """CPU twin of HipContext.collision_edges_host."""
    return _collision_edges((), load_library().mp_collision_edges_cpu_f64, model, collision, q_from, q_to, margin, tol, max_steps, want,
                            nthreads)


PLAN_OUTPUTS = ("status", "count", "waypoints", "iterations", "nodes", "evaluations")
PLAN_SOLVED, PLAN_EXHAUSTED, PLAN_TREE_FULL, PLAN_START_BLOCKED, PLAN_GOAL_BLOCKED, PLAN_PATH_TOO_LONG, PLAN_INVALID = 0, 1, 2, 3, 4, 5, -1


def rrt_connect_workspace_bytes(n: int, max_nodes: int, blocks: int) -> int:
    """Bytes of tree workspace for `blocks` one-wave blocks of HipContext.rrt_connect."""
    r = int(load_library().mp_rrt_connect_workspace_bytes(int(n), int(max_nodes), int(blocks)))
    if r < 0:
        _check(-r)
    return r


def _rrt_box(model, lo, hi, step, min_advance):
    lo, hi = _as_c(lo, np.float64, (model.n,), "lo"), _as_c(hi, np.float64, (model.n,), "hi")
    step = float(step)
    return lo, hi, step, step / 8 if min_advance is None else float(min_advance)


def _rrt_connect(lead, fn, model, collision, q_start, q_goal, lo, hi, margin, tol, step, min_advance, max_iters, max_nodes,
                 max_waypoints, max_steps, seed, want, nthreads=None):
    want = PLAN_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in PLAN_OUTPUTS:
            raise ValueError(f"unknown planner output {w!r}; choose from {PLAN_OUTPUTS}")
    qs = _as_c(q_start, np.float64, name="q_start")
    if qs.ndim != 2 or qs.shape[1] != model.n:
        raise ValueError(f"q_start must be (problems, {model.n}); got {qs.shape}")
    B, n = qs.shape
    qg = _as_c(q_goal, np.float64, (B, n), "q_goal")
    lo, hi, step, min_advance = _rrt_box(model, lo, hi, step, min_advance)
    W = max(int(max_waypoints), 0)  # (a value below 2 is the entry's to refuse)
    shapes = {"status": (B,), "count": (B,), "waypoints": (B, W, n), "iterations": (B,), "nodes": (B, 2), "evaluations": (B,)}
    out = {w: np.empty(shapes[w], dtype=np.float64 if w == "waypoints" else np.int32) for w in want}
    ptrs = []
    for w in PLAN_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (_dptr(a) if w == "waypoints" else a.ctypes.data_as(_vp)))
    args = list(lead) + [model.handle, collision.handle, _dptr(qs), _dptr(qg), B, _dptr(lo), _dptr(hi), int(seed), step, min_advance,
                         int(max_iters), int(max_nodes), int(max_waypoints), float(margin), float(tol), int(max_steps)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_rrt_connect(model: "HipModel", collision: "HipCollision", q_start, q_goal, lo, hi, margin, tol, *, step, min_advance=None,
                    max_iters, max_nodes, max_waypoints, max_steps, seed, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.rrt_connect_arrays."""
    return _rrt_connect((), load_library().mp_rrt_connect_cpu_f64, model, collision, q_start, q_goal, lo, hi, margin, tol, step,
                        min_advance, max_iters, max_nodes, max_waypoints, max_steps, seed, want, nthreads)


SHORTCUT_OUTPUTS = ("status", "count", "waypoints", "length_in", "length_out", "iterations", "accepted", "skipped_full", "evaluations")
SHORTCUT_DONE, SHORTCUT_STRAIGHT, SHORTCUT_SKIPPED, SHORTCUT_INVALID = 0, 1, 2, -1


def path_shortcut_workspace_bytes(n: int, max_waypoints: int, blocks: int) -> int:
    """Bytes of path workspace for `blocks` one-wave blocks of HipContext.path_shortcut."""
    r = int(load_library().mp_path_shortcut_workspace_bytes(int(n), int(max_waypoints), int(blocks)))
    if r < 0:
        _check(-r)
    return r


def _path_shortcut(lead, fn, model, collision, waypoints, count, margin, tol, max_iters, min_gain, max_waypoints, max_steps, seed, want,
                   nthreads=None):
    want = SHORTCUT_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in SHORTCUT_OUTPUTS:
            raise ValueError(f"unknown shortcut output {w!r}; choose from {SHORTCUT_OUTPUTS}")
    wp = _as_c(waypoints, np.float64, name="waypoints")
    if wp.ndim != 3 or wp.shape[2] != model.n:
        raise ValueError(f"waypoints must be (problems, W, {model.n}); got {wp.shape}")
    B, w_in, n = wp.shape
    cnt = np.asarray(count)
    if cnt.dtype.kind not in "iu":  # (a silent cast would turn 2.9 into 2)
        raise TypeError(f"count must be an integer array; got {cnt.dtype}")
    if cnt.size and (cnt.min() < np.iinfo(np.int32).min or cnt.max() > np.iinfo(np.int32).max):
        raise ValueError("count does not fit 32 bits")
    cnt = _as_c(cnt.astype(np.int32), np.int32, (B,), "count")
    W = w_in if max_waypoints is None else int(max_waypoints)
    rows = max(W, 0)  # (a value below 2 is the entry's to refuse)
    real = ("waypoints", "length_in", "length_out")
    out = {w: np.empty((B, rows, n) if w == "waypoints" else (B,), dtype=np.float64 if w in real else np.int32) for w in want}
    ptrs = []
    for w in SHORTCUT_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (_dptr(a) if w in real else a.ctypes.data_as(_vp)))
    args = list(lead) + [model.handle, collision.handle, _dptr(wp), cnt.ctypes.data_as(_vp), B, w_in, int(seed), int(max_iters),
                         float(min_gain), W, float(margin), float(tol), int(max_steps)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_path_shortcut(model: "HipModel", collision: "HipCollision", waypoints, count, margin, tol, *, max_iters, min_gain=0.0,
                      max_waypoints=None, max_steps, seed, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.path_shortcut_arrays."""
    return _path_shortcut((), load_library().mp_path_shortcut_cpu_f64, model, collision, waypoints, count, margin, tol, max_iters,
                          min_gain, max_waypoints, max_steps, seed, want, nthreads)


BLEND_OUTPUTS = ("status", "corner", "count", "points", "cut", "knot", "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq")
BLEND_DONE, BLEND_STRAIGHT, BLEND_SKIPPED, BLEND_POINT, BLEND_BLOCKED, BLEND_REVERSAL, BLEND_INVALID = 0, 1, 2, 3, 4, 5, -1


def _path_blend(lead, fn, model, collision, waypoints, count, N, margin, tol, blend, max_halvings, max_steps, want, nthreads=None):
    want = BLEND_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in BLEND_OUTPUTS:
            raise ValueError(f"unknown blend output {w!r}; choose from {BLEND_OUTPUTS}")
    wp = _as_c(waypoints, np.float64, name="waypoints")
    if wp.ndim != 3 or wp.shape[2] != model.n:
        raise ValueError(f"waypoints must be (problems, W, {model.n}); got {wp.shape}")
    B, w_in, n = wp.shape
    cnt = np.asarray(count)
    if cnt.dtype.kind not in "iu":  # (a silent cast would turn 2.9 into 2)
        raise TypeError(f"count must be an integer array; got {cnt.dtype}")
    if cnt.size and (cnt.min() < np.iinfo(np.int32).min or cnt.max() > np.iinfo(np.int32).max):
        raise ValueError("count does not fit 32 bits")
    cnt = _as_c(cnt.astype(np.int32), np.int32, (B,), "count")
    grid = max(int(N), 0)  # (a value below 3 is the entry's to refuse)
    shapes = {"points": (B, w_in, n), "cut": (B, w_in), "knot": (B, w_in), "q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n)}
    whole = ("status", "corner", "count", "halvings", "evaluations")
    out = {w: np.empty(shapes.get(w, (B,)), dtype=np.int32 if w in whole else np.float64) for w in want}
    ptrs = []
    for w in BLEND_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (a.ctypes.data_as(_vp) if w in whole else _dptr(a)))
    args = list(lead) + [model.handle, collision.handle, _dptr(wp), cnt.ctypes.data_as(_vp), B, w_in, int(N), float(blend),
                         int(max_halvings), float(margin), float(tol), int(max_steps)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_path_blend(model: "HipModel", collision: "HipCollision", waypoints, count, N, margin, tol, *, blend=0.5, max_halvings=6,
                   max_steps=64, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.path_blend_arrays."""
    return _path_blend((), load_library().mp_path_blend_cpu_f64, model, collision, waypoints, count, N, margin, tol, blend, max_halvings,
                       max_steps, want, nthreads)


SAMPLE_OUTPUTS = ("status", "count", "needed", "s", "sd", "sdd", "positions", "velocities", "accelerations", "torques")
SAMPLE_OK, SAMPLE_TRUNCATED, SAMPLE_STOPS, SAMPLE_UNTIMED, SAMPLE_INVALID = 0, 1, 2, 3, -1
SAMPLE_CURVE_TABLES = ("status", "count", "points", "cut", "knot", "length")


def sample_rows_needed(duration, dt) -> np.ndarray:
    """`needed` of the sampler's contract for durations T (any shape) at period dt, by the entry's own rule: k_end + 1 with k_end the
    smallest k >= 0 whose float64 product k * dt reaches T; 0 where T is not finite (or negative)."""
    T = np.asarray(duration, dtype=np.float64)
    dt = float(dt)
    ok = np.isfinite(T) & (T >= 0)
    Ts = np.where(ok, T, 0.0)
    k = np.ceil(Ts / dt)
    down = (k > 0) & ((k - 1.0) * dt >= Ts)
    up = ~down & (k * dt < Ts)
    k = k - down + up
    return np.where(ok, k + 1, 0).astype(np.int64)


def _trajectory_sample(lead, fn, model, t, x, dt, M, path, curve, g, Ftip, want, nthreads=None):
    want = SAMPLE_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in SAMPLE_OUTPUTS:
            raise ValueError(f"unknown sample output {w!r}; choose from {SAMPLE_OUTPUTS}")
    n = model.n
    t = _as_c(t, np.float64, name="time")
    if t.ndim != 2:
        raise ValueError(f"time must be (paths, N); got {t.shape}")
    B, N = t.shape
    x = _as_c(x, np.float64, (B, N), "sd2")
    geo = [None, None, None]
    if path is not None:
        if len(path) != 3:
            raise ValueError("path must be the three arrays (q, dq, ddq)")
        geo = [None if a is None else _as_c(a, np.float64, (B, N, n), name) for a, name in zip(path, ("q", "dq", "ddq"))]
    tab, w_in = [None] * 6, 0
    if curve is not None:
        pts = curve.get("points")
        if pts is not None:
            pts = _as_c(pts, np.float64, name="points")
            if pts.ndim != 3 or pts.shape[0] != B or pts.shape[2] != n:
                raise ValueError(f"curve points must be ({B}, W, {n}); got {pts.shape}")
            w_in = pts.shape[1]
        else:
            w_in = 0 if curve.get("cut") is None else np.shape(curve["cut"])[-1]
        shapes = {"status": (B,), "count": (B,), "points": (B, w_in, n), "cut": (B, w_in), "knot": (B, w_in), "length": (B,)}
        for i, k in enumerate(SAMPLE_CURVE_TABLES):
            a = curve.get(k)
            if a is not None:
                tab[i] = _as_c(a, np.int32 if k in ("status", "count") else np.float64, shapes[k], "curve " + k)
    rows = max(int(M), 0)  # (a value below 1 is the entry's to refuse)
    whole = ("status", "count", "needed")
    shapes = {"s": (B, rows), "sd": (B, rows), "sdd": (B, rows), "positions": (B, rows, n), "velocities": (B, rows, n),
              "accelerations": (B, rows, n), "torques": (B, rows, n)}
    out = {w: np.empty(shapes.get(w, (B,)), dtype=np.int32 if w in whole else np.float64) for w in want}
    ptrs = []
    for w in SAMPLE_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (a.ctypes.data_as(_vp) if w in whole else _dptr(a)))
    iptr = lambda a: None if a is None else a.ctypes.data_as(_vp)  # noqa: E731
    args = list(lead) + [model.handle, _dptr(t), _dptr(x), B, N, _dptr(geo[0]), _dptr(geo[1]), _dptr(geo[2]), iptr(tab[0]), iptr(tab[1]),
                         _dptr(tab[2]), _dptr(tab[3]), _dptr(tab[4]), _dptr(tab[5]), int(w_in), float(dt), int(M),
                         _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip"))] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_trajectory_sample(model: "HipModel", t, x, dt, M, *, path=None, curve=None, g=None, Ftip=None, want=None,
                          nthreads: int = 0) -> dict:
    """CPU twin of HipContext.trajectory_sample_arrays."""
    return _trajectory_sample((), load_library().mp_trajectory_sample_cpu_f64, model, t, x, dt, M, path, curve, g, Ftip, want, nthreads)


GOAL_OUTPUTS = ("status", "q", "attempts", "iterations", "converged", "pose_error", "clearance", "witness")
GOAL_FOUND, GOAL_IN_COLLISION, GOAL_UNREACHED, GOAL_INVALID = 0, 1, 2, -1


def _goal_ik(lead, fn, model, collision, T_goal, q_seed, lo, hi, margin, tol, eomg, ev, damping, step_cap, max_iters, max_attempts, seed,
             want, nthreads=None):
    want = GOAL_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in GOAL_OUTPUTS:
            raise ValueError(f"unknown goal output {w!r}; choose from {GOAL_OUTPUTS}")
    q0 = _as_c(q_seed, np.float64, name="q_seed")
    if q0.ndim != 2 or q0.shape[1] != model.n:
        raise ValueError(f"q_seed must be (problems, {model.n}); got {q0.shape}")
    B, n = q0.shape
    Tg = np.asarray(T_goal, dtype=np.float64)
    if Tg.shape != (B, 4, 4) and Tg.shape != (B, 16):
        raise ValueError(f"T_goal must be ({B}, 4, 4) or ({B}, 16); got {Tg.shape}")
    Tg = _as_c(Tg.reshape(B, 16), np.float64, (B, 16), "T_goal")
    lo, hi = _as_c(lo, np.float64, (n,), "lo"), _as_c(hi, np.float64, (n,), "hi")
    shapes = {"status": (B,), "q": (B, n), "attempts": (B,), "iterations": (B,), "converged": (B,), "pose_error": (B, 2),
              "clearance": (B,), "witness": (B, 3)}
    real = ("q", "pose_error", "clearance")
    out = {w: np.empty(shapes[w], dtype=np.float64 if w in real else np.int32) for w in want}
    ptrs = []
    for w in GOAL_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (_dptr(a) if w in real else a.ctypes.data_as(_vp)))
    args = list(lead) + [model.handle, collision.handle, _dptr(Tg), _dptr(q0), B, _dptr(lo), _dptr(hi), int(seed), float(eomg), float(ev),
                         float(damping), float(step_cap), int(max_iters), int(max_attempts), float(margin), float(tol)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_goal_ik(model: "HipModel", collision: "HipCollision", T_goal, q_seed, lo, hi, margin, tol, *, eomg, ev, damping, step_cap,
                max_iters, max_attempts, seed, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.goal_ik_arrays."""
    return _goal_ik((), load_library().mp_goal_ik_cpu_f64, model, collision, T_goal, q_seed, lo, hi, margin, tol, eomg, ev, damping,
                    step_cap, max_iters, max_attempts, seed, want, nthreads)


CARTESIAN_OUTPUTS = ("status", "reached", "span", "t", "clearance", "deviation_pos", "deviation_rot", "pose_error", "iterations",
                     "evaluations", "q", "dq", "ddq", "span_status", "span_clearance")
(CARTESIAN_DONE, CARTESIAN_STALLED, CARTESIAN_SINGULAR, CARTESIAN_LIMIT, CARTESIAN_JUMP, CARTESIAN_BLOCKED, CARTESIAN_UNDECIDED,
 CARTESIAN_INVALID) = 0, 1, 2, 3, 4, 5, 6, -1
CARTESIAN_TASKS = ("full", "position")


def _cartesian_task(task) -> int:
    if task in CARTESIAN_TASKS:
        return CARTESIAN_TASKS.index(task)
    if isinstance(task, (int, np.integer)) and not isinstance(task, bool):
        return int(task)  # (a value outside 0..1 is the entry's to refuse)
    raise ValueError(f"unknown task {task!r}; choose from {CARTESIAN_TASKS}")


def cartesian_path_workspace_bytes(problems: int, N: int) -> int:
    """Bytes of workspace for HipContext.cartesian_path over `problems` problems of N grid points."""
    r = int(load_library().mp_cartesian_path_workspace_bytes(int(problems), int(N)))
    if r < 0:
        _check(-r)
    return r


def _cartesian_path(lead, fn, model, collision, q_start, T_goal, lo, hi, N, margin, tol, task, eomg, ev, damping, max_iters,
                    max_joint_step, max_steps, want, nthreads=None):
    want = CARTESIAN_OUTPUTS if want is None else tuple(want)
    for w in want:
        if w not in CARTESIAN_OUTPUTS:
            raise ValueError(f"unknown cartesian output {w!r}; choose from {CARTESIAN_OUTPUTS}")
    q0 = _as_c(q_start, np.float64, name="q_start")
    if q0.ndim != 2 or q0.shape[1] != model.n:
        raise ValueError(f"q_start must be (problems, {model.n}); got {q0.shape}")
    B, n = q0.shape
    Tg = np.asarray(T_goal, dtype=np.float64)
    if Tg.shape != (B, 4, 4) and Tg.shape != (B, 16):
        raise ValueError(f"T_goal must be ({B}, 4, 4) or ({B}, 16); got {Tg.shape}")
    Tg = _as_c(Tg.reshape(B, 16), np.float64, (B, 16), "T_goal")
    lo, hi = _as_c(lo, np.float64, (n,), "lo"), _as_c(hi, np.float64, (n,), "hi")
    grid = max(int(N), 1)  # (a value below 2 is the entry's to refuse)
    shapes = {"q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n), "span_status": (B, grid - 1), "span_clearance": (B, grid - 1)}
    whole = ("status", "reached", "span", "iterations", "evaluations", "span_status")
    out = {w: np.empty(shapes.get(w, (B,)), dtype=np.int32 if w in whole else np.float64) for w in want}
    ptrs = []
    for w in CARTESIAN_OUTPUTS:
        a = out.get(w)
        ptrs.append(None if a is None else (a.ctypes.data_as(_vp) if w in whole else _dptr(a)))
    args = list(lead) + [model.handle, collision.handle, _dptr(q0), _dptr(Tg), B, _dptr(lo), _dptr(hi), int(N), _cartesian_task(task),
                         float(eomg), float(ev), float(damping), int(max_iters), float(max_joint_step), float(margin), float(tol),
                         int(max_steps)] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_cartesian_path(model: "HipModel", collision: "HipCollision", q_start, T_goal, lo, hi, N, margin, tol, *, task="full", eomg=1e-6,
                       ev=1e-6, damping=0.01, max_iters=20, max_joint_step=0.5, max_steps=64, want=None, nthreads: int = 0) -> dict:
    """CPU twin of HipContext.cartesian_path_arrays."""
    return _cartesian_path((), load_library().mp_cartesian_path_cpu_f64, model, collision, q_start, T_goal, lo, hi, N, margin, tol, task,
                           eomg, ev, damping, max_iters, max_joint_step, max_steps, want, nthreads)


def _pd_regulation_args(model, theta0, theta_des, Kp, Kd, g, steps):
    th0 = _as_c(theta0, np.float64, name="theta0")
    if th0.ndim != 2 or th0.shape[1] != model.n:
        raise ValueError(f"theta0 must be (K, {model.n}), got {th0.shape}")
    K = th0.shape[0]
    des = _as_c(theta_des, np.float64, (K, model.n), "theta_des")
    kp, kd = _as_c(Kp, np.float64, (K,), "Kp"), _as_c(Kd, np.float64, (K,), "Kd")
    gv = None if g is None else _as_c(g, np.float64, (3,), "g")
    if int(steps) < 0:
        raise ValueError("steps must be non-negative")
    return th0, des, kp, kd, gv, np.full((K, int(steps)), np.nan), np.zeros(K, dtype=np.int32)


def cpu_pd_regulation(model: "HipModel", theta0, theta_des, Kp, Kd, g, dt, steps, nthreads: int = 0):
    """HipContext.pd_regulation_host on the host cores (mp_pd_regulation_cpu_f64): same arguments, same results."""
    th0, des, kp, kd, gv, err, cnt = _pd_regulation_args(model, theta0, theta_des, Kp, Kd, g, steps)
    _check(load_library().mp_pd_regulation_cpu_f64(model.handle, _dptr(th0), _dptr(des), _dptr(kp), _dptr(kd), th0.shape[0], _dptr(gv), float(dt),
                                                   int(steps), _dptr(err), cnt.ctypes.data_as(_vp), int(nthreads)))
    return err, cnt


def cpu_inverse_kinematics(model: "HipModel", T_desired, theta0, joint_limits=None, eomg=1e-6, ev=1e-6, max_iterations=10000,
                           damping=2e-2, step_cap=0.3, weight_orientation=1.0, weight_position=1.0, adaptive_tuning=False,
                           backtracking=False, seed=1234, nthreads: int = 0):
    """HipContext.inverse_kinematics_host on the host cores (mp_inverse_kinematics_cpu_f64): same arguments, same results."""
    T = _as_c(T_desired, np.float64, name="T_desired")
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError(f"T_desired must be (B, 4, 4), got {T.shape}")
    B = T.shape[0]
    th0 = _as_c(theta0, np.float64, (B, model.n), "thetalist0")
    lim = None
    if joint_limits is not None:
        lim = np.array([[-np.inf if lo is None else lo, np.inf if hi is None else hi] for lo, hi in joint_limits], dtype=np.float64)
        if lim.shape != (model.n, 2):
            raise ValueError(f"joint_limits must be ({model.n}, 2), got {lim.shape}")
    th = np.zeros((B, model.n))
    ok, it, rs = (np.zeros(B, dtype=np.int32) for _ in range(3))
    _check(load_library().mp_inverse_kinematics_cpu_f64(
        model.handle, _dptr(T), _dptr(th0), B, _dptr(lim), float(eomg), float(ev), int(max_iterations), float(damping), float(step_cap),
        float(weight_orientation), float(weight_position), int(bool(adaptive_tuning)), int(bool(backtracking)), int(seed) & 0xFFFFFFFF,
        _dptr(th), ok.ctypes.data_as(_vp), it.ctypes.data_as(_vp), rs.ctypes.data_as(_vp), int(nthreads)))
    return th, ok.astype(bool), it, rs


def cpu_fd_trajectory(model: "HipModel", theta0, dtheta0, taumat, g, Ftipmat, dt, intRes, dtype=np.float64, nthreads: int = 0):
    lib = load_library()
    tm = _as_c(taumat, dtype, name="taumat")
    if tm.ndim != 3 or tm.shape[2] != model.n:
        raise ValueError(f"taumat must be (B, N, {model.n}); got {tm.shape}")
    B, N, n = tm.shape
    th, dth = _as_c(theta0, dtype, (B, n), "theta0"), _as_c(dtheta0, dtype, (B, n), "dtheta0")
    Fm = None if Ftipmat is None else _as_c(Ftipmat, dtype, (B, N, 6), "Ftipmat")
    out = [np.empty((B, N, n), dtype=np.float32) for _ in range(3)]
    fn = lib.mp_fd_trajectory_cpu_f32 if dtype == np.float32 else lib.mp_fd_trajectory_cpu_f64
    _check(fn(model.handle, _ptr(th, dtype), _ptr(dth, dtype), _ptr(tm, dtype), _ptr(Fm, dtype), B, N, _dptr(_vec_or_none(g, 3, "g")),
              float(dt), int(intRes), _fptr(out[0]), _fptr(out[1]), _fptr(out[2]), int(nthreads)))
    return out[0], out[1], out[2]


def _vjp_arrays(model, theta0, dtheta0, taumat, Ftipmat, gpos, gvel, gacc, layout="batch_major"):
    """float64 C-contiguous arrays of one roll-out VJP call; taumat (B,N,n) or, time-major, (N,B,n)."""
    if layout not in ("batch_major", "time_major"):
        raise ValueError("layout must be 'batch_major' or 'time_major'")
    tm = _as_c(taumat, np.float64, name="taumat")
    if tm.ndim != 3 or tm.shape[2] != model.n:
        raise ValueError(f"taumat must be {'(B, N, %d)' % model.n if layout == 'batch_major' else '(N, B, %d)' % model.n}; got {tm.shape}")
    B = tm.shape[0] if layout == "batch_major" else tm.shape[1]
    th, dth = _as_c(theta0, np.float64, (B, model.n), "theta0"), _as_c(dtheta0, np.float64, (B, model.n), "dtheta0")
    Fm = None if Ftipmat is None else _as_c(Ftipmat, np.float64, tm.shape[:2] + (6,), "Ftipmat")
    G = [None if x is None else _as_c(x, np.float64, tm.shape, name) for x, name in ((gpos, "grad_positions"), (gvel, "grad_velocities"),
                                                                                     (gacc, "grad_accelerations"))]
    return th, dth, tm, Fm, G


def fd_trajectory_vjp_workspace_bytes(model: "HipModel", B: int, N: int, intRes: int) -> int:
    """Device workspace of mp_fd_trajectory_vjp_tm_f64: (B N + B intRes) 2n doubles."""
    v = int(load_library().mp_fd_trajectory_vjp_workspace_bytes(model.handle, int(B), int(N), int(intRes)))
    if v < 0:
        _check(-v)
    return v


def _regressor_rows(model, q, *others):
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    return (q,) + tuple(_as_c(a, np.float64, q.shape, name) for a, name in zip(others, ("qd", "qdd", "rhs")))


def id_regressor_normal_workspace_bytes(model: "HipModel", rows: int) -> int:
    """Device workspace of mp_id_regressor_normal_f64 (per-workgroup partial sums)."""
    v = int(load_library().mp_id_regressor_normal_workspace_bytes(model.handle, int(rows)))
    if v < 0:
        _check(-v)
    return v


def cpu_id_regressor(model: "HipModel", q, qd, qdd, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.id_regressor_host: (Y (rows, n, 10n), tau_ext (rows, n))."""
    q, qd, qdd = _regressor_rows(model, q, qd, qdd)
    Y, te = np.empty((q.shape[0], model.n, 10 * model.n)), np.empty(q.shape)
    _check(load_library().mp_id_regressor_cpu_f64(model.handle, _dptr(q), _dptr(qd), _dptr(qdd), q.shape[0], _dptr(_vec_or_none(g, 3, "g")),
                                                  _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(Y), _dptr(te), int(nthreads)))
    return Y, te


def cpu_id_regressor_normal(model: "HipModel", q, qd, qdd, rhs, g=None, Ftip=None, want_A: bool = True, nthreads: int = 0):
    """CPU twin of HipContext.id_regressor_normal_host: (A or None, b, rr)."""
    q, qd, qdd, rhs = _regressor_rows(model, q, qd, qdd, rhs)
    w = 10 * model.n
    A, b, rr = (np.empty((w, w)) if want_A else None), np.empty(w), np.empty(1)
    _check(load_library().mp_id_regressor_normal_cpu_f64(model.handle, _dptr(q), _dptr(qd), _dptr(qdd), _dptr(rhs), q.shape[0],
                                                         _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(A),
                                                         _dptr(b), _dptr(rr), int(nthreads)))
    return A, b, float(rr[0])


def cpu_fd_trajectory_vjp(model: "HipModel", theta0, dtheta0, taumat, g, Ftipmat, dt, intRes, gpos=None, gvel=None, gacc=None,
                          nthreads: int = 0):
    """CPU twin of HipContext.fd_trajectory_vjp_host on batch-major arrays: (dL/dtheta0, dL/ddtheta0, dL/dtaumat), float64."""
    th, dth, tm, Fm, G = _vjp_arrays(model, theta0, dtheta0, taumat, Ftipmat, gpos, gvel, gacc)
    B, N, n = tm.shape
    gth, gdth, gtau = np.zeros((B, n)), np.zeros((B, n)), np.zeros(tm.shape)
    _check(load_library().mp_fd_trajectory_vjp_cpu_f64(model.handle, _dptr(th), _dptr(dth), _dptr(tm), _dptr(Fm), B, N,
                                                       _dptr(_vec_or_none(g, 3, "g")), float(dt), int(intRes), *[_dptr(x) for x in G],
                                                       _dptr(gth), _dptr(gdth), _dptr(gtau), int(nthreads)))
    return gth, gdth, gtau


def _ilqr_weights(model, wq, wr, wf):
    n = model.n
    return _as_c(wq, np.float64, (2 * n,), "wq"), _as_c(wr, np.float64, (n,), "wr"), _as_c(wf, np.float64, (2 * n,), "wf")


def _ilqr_rows(model, taumat, others):
    tm = _as_c(taumat, np.float64, name="taumat")
    if tm.ndim != 3 or tm.shape[2] != model.n:
        raise ValueError(f"taumat must be (B, N, {model.n}); got {tm.shape}")
    return tm, [None if a is None else _as_c(a, np.float64, tm.shape[:2] + (w,), name) for a, w, name in others]


def ilqr_backward_workspace_bytes(model: "HipModel", B: int, N: int) -> int:
    """Device workspace of mp_ilqr_backward_tm_f64: 0 for the cooperative kernel that ships (pass any buffer, or None); 12 n^2 B doubles
    under MANIPULAPY_HIP_ILQR_BACKWARD=lane."""
    v = int(load_library().mp_ilqr_backward_workspace_bytes(model.handle, int(B), int(N)))
    if v < 0:
        _check(-v)
    return v


def _ilqr_backward(fn, lead, model, pos, vel, taumat, xref, wq, wr, wf, reg, g, dt, nthreads=None):
    n = model.n
    tm, (p, v, x) = _ilqr_rows(model, taumat, ((pos, n, "pos"), (vel, n, "vel"), (xref, 2 * n, "xref")))
    B, N = tm.shape[:2]
    wq, wr, wf = _ilqr_weights(model, wq, wr, wf)
    rg = _as_c(np.broadcast_to(np.asarray(reg, dtype=np.float64), (B,)), np.float64, (B,), "reg")
    K, k, dV, st = np.zeros((B, N, n, 2 * n)), np.zeros((B, N, n)), np.zeros((B, 2)), np.zeros(B, dtype=np.int32)
    args = list(lead) + [model.handle, _dptr(p), _dptr(v), _dptr(tm), _dptr(x), _dptr(wq), _dptr(wr), _dptr(wf), _dptr(rg), B, N,
                         _dptr(_vec_or_none(g, 3, "g")), float(dt), _dptr(K), _dptr(k), _dptr(dV), st.ctypes.data_as(_vp)]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return K, k, dV, st


def _ilqr_rollout(fn, lead, model, theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref, wq, wr, wf, g, dt, want_rows, nthreads=None):
    n = model.n
    tm, (p, v, x, kk) = _ilqr_rows(model, taumat, ((pos, n, "pos"), (vel, n, "vel"), (xref, 2 * n, "xref"), (k, n, "k")))
    B, N = tm.shape[:2]
    th, dth = _as_c(theta0, np.float64, (B, n), "theta0"), _as_c(dtheta0, np.float64, (B, n), "dtheta0")
    KK = None if K is None else _as_c(K, np.float64, (B, N, n, 2 * n), "K")
    if (KK is None) != (kk is None) or (KK is not None and (p is None or v is None)):
        raise ValueError("K and k must both be given, with the nominal pos and vel, or both be None")
    al = _as_c(alpha, np.float64, name="alpha")
    if al.ndim != 2 or al.shape[1] != B:
        raise ValueError(f"alpha must be (A, {B}); got {al.shape}")
    A = al.shape[0]
    wq, wr, wf = _ilqr_weights(model, wq, wr, wf)
    cost = np.zeros((A, B))
    rows = [np.zeros((A, B, N, n)) for _ in range(3)] if want_rows else [None, None, None]
    args = list(lead) + [model.handle, _dptr(th), _dptr(dth), _dptr(tm), _dptr(p), _dptr(v), _dptr(KK), _dptr(kk), _dptr(al), _dptr(x),
                         _dptr(wq), _dptr(wr), _dptr(wf), A, B, N, _dptr(_vec_or_none(g, 3, "g")), float(dt), _dptr(cost)] \
        + [_dptr(r) for r in rows]
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return cost, rows[0], rows[1], rows[2]


def cpu_ilqr_backward(model: "HipModel", pos, vel, taumat, xref, wq, wr, wf, reg, g, dt, nthreads: int = 0):
    """CPU twin of HipContext.ilqr_backward_host: (K (B, N, n, 2n), k (B, N, n), dV (B, 2), status (B))."""
    return _ilqr_backward(load_library().mp_ilqr_backward_cpu_f64, (), model, pos, vel, taumat, xref, wq, wr, wf, reg, g, dt, nthreads)


def cpu_ilqr_rollout(model: "HipModel", theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref, wq, wr, wf, g, dt, want_rows=True,
                     nthreads: int = 0):
    """CPU twin of HipContext.ilqr_rollout_host: (cost (A, B), pos, vel, tau (A, B, N, n) or None)."""
    return _ilqr_rollout(load_library().mp_ilqr_rollout_cpu_f64, (), model, theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref, wq, wr,
                         wf, g, dt, want_rows, nthreads)


def _toppra_limits(n, torque_limits, acceleration_limits):
    tl = None if torque_limits is None else _as_c(torque_limits, np.float64, (n, 2), "torque_limits")
    al = None if acceleration_limits is None else _as_c(acceleration_limits, np.float64, (n,), "acceleration_limits")
    return tl, al


def _toppra_paths(n, q, dq, ddq, sd_start, sd_end):
    q = _as_c(q, np.float64, name="path_q")
    if q.ndim != 3 or q.shape[2] != n:
        raise ValueError(f"path_q must be (B, N, {n}); got {q.shape}")
    B = q.shape[0]
    dq, ddq = _as_c(dq, np.float64, q.shape, "path_dq"), _as_c(ddq, np.float64, q.shape, "path_ddq")
    s0 = _as_c(np.broadcast_to(np.asarray(sd_start, dtype=np.float64), (B,)), np.float64, (B,), "sd_start")
    s1 = _as_c(np.broadcast_to(np.asarray(sd_end, dtype=np.float64), (B,)), np.float64, (B,), "sd_end")
    return q, dq, ddq, s0, s1


def _toppra_outputs(B, N, n, want_rows):
    out = {"controllable": np.zeros((B, N, 2)), "sd2": np.zeros((B, N)), "sdd": np.zeros((B, N)), "time": np.zeros((B, N)),
           "duration": np.zeros(B), "status": np.zeros(B, dtype=np.int32)}
    rows = [np.zeros((B, N, n)) for _ in range(3)] if want_rows else [None, None, None]
    out["velocities"], out["accelerations"], out["torques"] = rows
    ptrs = [_dptr(out["controllable"]), _dptr(out["sd2"]), _dptr(out["sdd"]), _dptr(out["time"]), _dptr(out["duration"]),
            out["status"].ctypes.data_as(_vp)] + [_dptr(r) for r in rows]
    return out, ptrs


def _toppra_call(fn, lead, model, q, dq, ddq, velocity_limits, torque_limits, acceleration_limits, sd_start, sd_end, g, Ftip, want_rows,
                 nthreads=None):
    """{"sd2", "sdd", "time" (B, N), "duration" (B), "velocities", "accelerations", "torques" (B, N, n) or None, "controllable"
    (B, N, 2), "status" (B) int32} of mp_toppra_host_f64 / mp_toppra_cpu_f64."""
    n = model.n
    q, dq, ddq, s0, s1 = _toppra_paths(n, q, dq, ddq, sd_start, sd_end)
    B, N = q.shape[:2]
    vl = _as_c(velocity_limits, np.float64, (n,), "velocity_limits")
    tl, al = _toppra_limits(n, torque_limits, acceleration_limits)
    out, ptrs = _toppra_outputs(B, N, n, want_rows)
    args = list(lead) + [model.handle, _dptr(q), _dptr(dq), _dptr(ddq), _dptr(vl), _dptr(tl), _dptr(al), _dptr(s0), _dptr(s1), B, N,
                         _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip"))] + ptrs
    if nthreads is not None:
        args.append(int(nthreads))
    _check(fn(*args))
    return out


def cpu_path_dynamics(model: "HipModel", q, dq, ddq, velocity_limits, g=None, Ftip=None, nthreads: int = 0):
    """CPU twin of HipContext.path_dynamics on host rows (rows, n): (a, b, c (rows, n), xbar (rows,))."""
    q = _as_c(q, np.float64, name="q")
    if q.ndim != 2 or q.shape[1] != model.n:
        raise ValueError(f"q must be (rows, {model.n}); got {q.shape}")
    dq, ddq = _as_c(dq, np.float64, q.shape, "dq"), _as_c(ddq, np.float64, q.shape, "ddq")
    a, b, c, xbar = np.zeros_like(q), np.zeros_like(q), np.zeros_like(q), np.zeros(q.shape[0])
    _check(load_library().mp_path_dynamics_cpu_f64(model.handle, _dptr(q), _dptr(dq), _dptr(ddq), q.shape[0],
                                                   _dptr(_as_c(velocity_limits, np.float64, (model.n,), "velocity_limits")),
                                                   _dptr(_vec_or_none(g, 3, "g")), _dptr(_vec_or_none(Ftip, 6, "Ftip")), _dptr(a), _dptr(b),
                                                   _dptr(c), _dptr(xbar), int(nthreads)))
    return a, b, c, xbar


def cpu_toppra_sweep(a, b, c, xbar, dq, ddq, torque_limits=None, acceleration_limits=None, sd_start=0.0, sd_end=0.0, want_rows=True,
                     nthreads: int = 0):
    """The sweep alone (mp_toppra_sweep_cpu_f64) on given batch-major coefficients a / b / c / dq / ddq (B, N, n), xbar (B, N): the dict
    of _toppra_call."""
    a = _as_c(a, np.float64, name="a")
    if a.ndim != 3:
        raise ValueError(f"a must be (B, N, n); got {a.shape}")
    B, N, n = a.shape
    a, dq, ddq, s0, s1 = _toppra_paths(n, a, dq, ddq, sd_start, sd_end)
    b, c, xbar = _as_c(b, np.float64, a.shape, "b"), _as_c(c, np.float64, a.shape, "c"), _as_c(xbar, np.float64, (B, N), "xbar")
    tl, al = _toppra_limits(n, torque_limits, acceleration_limits)
    out, ptrs = _toppra_outputs(B, N, n, want_rows)
    _check(load_library().mp_toppra_sweep_cpu_f64(n, _dptr(a), _dptr(b), _dptr(c), _dptr(xbar), _dptr(dq), _dptr(ddq), _dptr(tl), _dptr(al),
                                                  _dptr(s0), _dptr(s1), B, N, *ptrs, int(nthreads)))
    return out


def cpu_toppra(model: "HipModel", q, dq, ddq, velocity_limits, torque_limits=None, acceleration_limits=None, sd_start=0.0, sd_end=0.0,
               g=None, Ftip=None, want_rows=True, nthreads: int = 0):
    """CPU twin of HipContext.toppra_host."""
    return _toppra_call(load_library().mp_toppra_cpu_f64, (), model, q, dq, ddq, velocity_limits, torque_limits, acceleration_limits,
                        sd_start, sd_end, g, Ftip, want_rows, nthreads)


def cpu_cartesian_trajectory(Xstart, Xend, Tf, N, method, nthreads: int = 0):
    Xs = _as_c(Xstart, np.float64, name="Xstart")
    if Xs.ndim != 3 or Xs.shape[1:] != (4, 4):
        raise ValueError(f"Xstart must be (B, 4, 4); got {Xs.shape}")
    Xe = _as_c(Xend, np.float64, Xs.shape, "Xend")
    B, N = Xs.shape[0], int(N)
    out = [np.empty((B, N, 3), dtype=np.float32) for _ in range(3)] + [np.empty((B, N, 3, 3), dtype=np.float32)]
    _check(load_library().mp_cartesian_trajectory_cpu_f32(_dptr(Xs), _dptr(Xe), B, N, float(Tf), int(method), *[_fptr(o) for o in out],
                                                          int(nthreads)))
    return tuple(out)


def cpu_threads(items: int = 1 << 30) -> int:
    return int(load_library().mp_cpu_threads(int(items)))


def _out_or_new(out, shape, dtype) -> np.ndarray:
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not isinstance(out, np.ndarray) or out.shape != tuple(shape) or out.dtype != dtype or not out.flags.c_contiguous \
            or not out.flags.writeable:
        raise ValueError(f"out must be a writeable C-contiguous {np.dtype(dtype).name} array of shape {tuple(shape)}")
    return out


def _p(buf):
    if buf is None:
        return None
    if isinstance(buf, DeviceBuffer):
        return buf.ptr
    return buf  # already a c_void_p


class HipComm:
    def __init__(self, ctx: HipContext, unique_id: bytes, nranks: int, rank: int):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self.ctx = ctx
        self.nranks, self.rank = int(nranks), int(rank)
        buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        p = _vp()
        _check(ctx.lib.mp_comm_create(ctx.handle, buf, self.nranks, self.rank, ctypes.byref(p)))
        self.handle = p

    def allgather(self, d_send, d_recv, bytes_per_rank: int) -> None:
        _check(self.ctx.lib.mp_comm_allgather(self.handle, _p(d_send), _p(d_recv), ctypes.c_size_t(int(bytes_per_rank))))

    def exchange_chunk(self, d_all, bytes_per_rank: int, offset: int, nbytes: int) -> None:
        """Bytes [offset, offset + nbytes) of this rank's slot of `d_all` (just written on the compute stream) go to every
        peer, the peers' same range arrives in their slots, on the communicator's own stream (overlaps later kernels)."""
        _check(self.ctx.lib.mp_comm_exchange_chunk(self.handle, _p(d_all), ctypes.c_size_t(int(bytes_per_rank)),
                                                   ctypes.c_size_t(int(offset)), ctypes.c_size_t(int(nbytes))))

    def _sizes(self, values):
        if len(values) != self.nranks:
            raise ValueError(f"expected {self.nranks} per-rank values, got {len(values)}")
        return (ctypes.c_size_t * self.nranks)(*[int(v) for v in values])

    def allgatherv(self, d_send, d_recv, bytes_of_rank) -> None:
        """Uneven shards: rank r contributes bytes_of_rank[r] bytes; d_recv gets them back to back in rank order."""
        _check(self.ctx.lib.mp_comm_allgatherv(self.handle, _p(d_send), _p(d_recv), self._sizes(bytes_of_rank)))

    def exchange_chunk_v(self, d_all, slot_offset, chunk_offset, chunk_bytes) -> None:
        _check(self.ctx.lib.mp_comm_exchange_chunk_v(self.handle, _p(d_all), self._sizes(slot_offset), self._sizes(chunk_offset),
                                                     self._sizes(chunk_bytes)))

    def join(self) -> None:
        """The compute stream waits for every exchange issued so far."""
        _check(self.ctx.lib.mp_comm_join(self.handle))

    def destroy(self) -> None:
        if self.handle is not None:
            self.ctx.lib.mp_comm_destroy(self.handle)
            self.handle = None
