"""ctypes binding of libsvsdf_hip.so (C ABI declared in include/svsdf_c.h)."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None

SHAPES = ["sdUnevenCapsule", "sdCutDisk", "sdTrapezoid", "sdRhombus", "star", "sdTunnel",
          "sdHorseshoe", "sdHeart", "sdOrientedVesica", "sdRoundedCross", "sdRoundedX", "bigX",
          "sdMoon", "sdPie", "sdPie2", "sdArc", "Polygon"]
SHAPE_ID = {n: i for i, n in enumerate(SHAPES)}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# every symbol include/svsdf_c.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "svsdf_create", "svsdf_destroy", "svsdf_config_default", "svsdf_shape_id_from_inputdata",
    "svsdf_shape_name", "svsdf_last_error_string", "svsdf_set_points", "svsdf_set_points_device",
    "svsdf_num_points", "svsdf_eval_penalty", "svsdf_eval_penalty_partial",
    "svsdf_accumulate_partial", "svsdf_lmbm_evaluate", "svsdf_last_costs", "svsdf_lmbm_begin",
    "svsdf_lmbm_finish", "svsdf_minco_coeffs", "svsdf_forward_T", "svsdf_backward_T",
    "svsdf_query_points", "svsdf_last_stats", "svsdf_shard_indices", "svsdf_set_profiling",
    "svsdf_shard_plan", "svsdf_lmbm_prepare", "svsdf_debug_sincos_mismatches", "svsdf_debug_sqrt_mismatches",
    "svsdf_map_create", "svsdf_map_destroy", "svsdf_map_info", "svsdf_map_gather", "svsdf_pcd_read_ascii",
    "svsdf_check_sub_sw_collision", "svsdf_shape_kernels",
    "svsdf_lbfgs_params_default", "svsdf_lbfgs_minimize", "svsdf_optimize_traj",
    "svsdf_set_conditions", "svsdf_sum_partials", "svsdf_shape_bound",
    "svsdf_mesh_outline", "svsdf_mesh_outline_obj", "svsdf_swept_outline", "svsdf_outline_extrude",
    "svsdf_get_plan", "svsdf_set_plan", "svsdf_set_combine", "svsdf_group_info", "svsdf_debug_sdf_at",
    "svsdf_group_stripe", "svsdf_set_group_serial", "svsdf_shape_selfcheck", "svsdf_mesh_section", "svsdf_mesh_section_obj",
    "svsdf_last_launches", "svsdf_set_scale", "svsdf_get_scale",
    "svsdf_frontend_set_map", "svsdf_frontend_yaw_free", "svsdf_kernel_bfs", "svsdf_astar_successors",
    "svsdf_astar_params_default", "svsdf_astar_search", "svsdf_astar_nodes", "svsdf_debug_live_allocations",
    "svsdf_map_build_device", "svsdf_map_device_get_info", "svsdf_map_device_cells", "svsdf_frontend_set_map_device",
    "svsdf_set_points_from_map", "svsdf_map_device_points", "svsdf_path_waypoints",
    "svsdf_clearance_params_default", "svsdf_min_clearance", "svsdf_motion_bounds",
    "svsdf_point_clearance_params_default", "svsdf_point_clearance", "svsdf_scale_bounds",
]


class LbfgsParams(C.Structure):
    """svsdf_lbfgs_params (include/svsdf_c.h), field for field lbfgs_parameter_t of the reference."""
    _fields_ = [("mem_size", C.c_int), ("g_epsilon", C.c_double), ("past", C.c_int), ("delta", C.c_double),
                ("max_iterations", C.c_int), ("max_linesearch", C.c_int), ("min_step", C.c_double),
                ("max_step", C.c_double), ("f_dec_coeff", C.c_double), ("s_curv_coeff", C.c_double),
                ("cautious_factor", C.c_double), ("machine_prec", C.c_double)]


EVALUATE_T = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
PROGRESS_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                         C.c_int, C.c_int, C.c_int)
LBFGS_STATUS = {0: "CONVERGENCE", 1: "STOP", 2: "CANCELED", -1012: "INVALID_FUNCVAL", -1011: "MINIMUMSTEP",
                -1010: "MAXIMUMSTEP", -1009: "MAXIMUMLINESEARCH", -1008: "MAXIMUMITERATION", -1007: "WIDTHTOOSMALL",
                -1006: "INVALIDPARAMETERS", -1005: "INCREASEGRADIENT"}


class Config(C.Structure):
    _fields_ = [("shape_id", C.c_int), ("poly_params", C.c_double * 3), ("safety_hor", C.c_double),
                ("weight_p", C.c_double), ("rho", C.c_double), ("head_state", C.c_double * 9),
                ("tail_state", C.c_double * 9), ("device", C.c_int), ("polygon_nverts", C.c_int),
                ("polygon_xy", _dp), ("rank", C.c_int), ("world_size", C.c_int), ("flags", C.c_int),
                ("n_devices", C.c_int), ("devices", C.c_int * 8), ("combine", C.c_int),
                ("polygon_nloops", C.c_int), ("polygon_loop_sizes", C.POINTER(C.c_int))]


class Stats(C.Structure):
    _fields_ = [("points", C.c_ulonglong), ("interior_points", C.c_ulonglong),
                ("solves", C.c_ulonglong), ("gsip_samples", C.c_ulonglong), ("sdf_evals", C.c_ulonglong),
                ("scan_evals", C.c_ulonglong), ("device_ms", C.c_double), ("solve_ms", C.c_double),
                ("solve_launches", C.c_uint), ("gsip_iterations", C.c_uint), ("culled_points", C.c_ulonglong),
                ("gsip_bound_mode", C.c_int), ("bound_mode_decided", C.c_int), ("bound_ratio", C.c_double),
                ("n_devices", C.c_int), ("combine", C.c_int), ("combine_ms", C.c_double), ("setup_ms", C.c_double),
                ("piece_time_exact", C.c_int), ("solve_ms_sum", C.c_double), ("round_scan_evals", C.c_ulonglong),
                ("round_ms", C.c_double), ("round_ms_sum", C.c_double), ("batches", C.c_int),
                ("speculative_evals", C.c_ulonglong), ("plan_settled", C.c_int), ("tail_iter", C.c_int),
                ("tail_launches", C.c_uint), ("tail_points", C.c_ulonglong), ("tail_ms", C.c_double),
                ("tail_ms_sum", C.c_double), ("shader_clock_mhz", C.c_double), ("fanout_ms", C.c_double)]


class Plan(C.Structure):
    _fields_ = [("bound_mode", C.c_int), ("batches", C.c_int), ("lanes_per_query", C.c_int), ("tail_iter", C.c_int),
                ("settled", C.c_int), ("layer_tables", C.c_int)]


PLAN_AUTO = -1


class LaunchRec(C.Structure):
    """svsdf_launch_rec (include/svsdf_c.h): one device launch of the last evaluation."""
    _fields_ = [("struct_size", C.c_int), ("kernel", C.c_int), ("shape", C.c_int), ("targ", C.c_int * 3), ("iter", C.c_int),
                ("batch", C.c_int), ("solo", C.c_int), ("points_per_wave", C.c_int), ("local_state", C.c_int),
                ("duo", C.c_int), ("anchors", C.c_int), ("fused", C.c_int), ("work", C.c_longlong), ("grid", C.c_uint),
                ("block", C.c_uint), ("lds_bytes", C.c_ulonglong)]


LAUNCH_REC_CAP = 512     # SVSDF_LAUNCH_REC_CAP
KERNELS = ["prep", "solve", "classify", "round", "tail", "reduce", "final", "finish",
           "solve_scaled", "classify_scaled", "reduce_scaled", "layer_tables"]   # svsdf_kernel_kind


class Scale(C.Structure):
    """svsdf_scale: s_a(t) = c[a] + sin(omega[a] t + phase[a]) amp[a] for a = x, y."""
    _fields_ = [("struct_size", C.c_int), ("enabled", C.c_int), ("c", C.c_double * 2), ("amp", C.c_double * 2),
                ("omega", C.c_double * 2), ("phase", C.c_double * 2)]


# the reference's worked example (sw_manager.hpp:498-500): s_x = 0.8 + sin(1.5 t - 1.0) * 0.6, s_y = sin(1.8 t) * 0.4 + 0.8
EXAMPLE_SCALE = {"c": (0.8, 0.8), "amp": (0.6, 0.4), "omega": (1.5, 1.8), "phase": (-1.0, 0.0)}


class AstarParams(C.Structure):
    """svsdf_astar_params (include/svsdf_c.h)."""
    _fields_ = [("struct_size", C.c_int), ("start_yaw", C.c_double), ("max_expansions", C.c_longlong), ("slice", C.c_int)]


class AstarResult(C.Structure):
    """svsdf_astar_result (include/svsdf_c.h)."""
    _fields_ = [("struct_size", C.c_int), ("status", C.c_int), ("path_len", C.c_size_t), ("expansions", C.c_ulonglong),
                ("pushes", C.c_ulonglong), ("relaxed_open", C.c_ulonglong), ("reopened", C.c_ulonglong),
                ("launches", C.c_ulonglong), ("stage_counts", C.c_ulonglong * 5), ("g_goal", C.c_double)]


ASTAR_STATUS = ["FOUND", "EXHAUSTED", "LIMIT", "OUT_OF_MAP"]     # svsdf_astar_status


class MapDeviceInfo(C.Structure):
    """svsdf_map_device_info (include/svsdf_c.h)."""
    _fields_ = [("struct_size", C.c_int), ("dims", C.c_int * 3), ("bmin", C.c_double * 3), ("bmax", C.c_double * 3),
                ("resolution", C.c_double), ("sta_threshold", C.c_int), ("n_cloud", C.c_size_t), ("occupied", C.c_size_t),
                ("gathered", C.c_size_t), ("build_ms", C.c_double), ("gather_ms", C.c_double)]


class ClearanceParams(C.Structure):
    """svsdf_clearance_params (include/svsdf_c.h)."""
    _fields_ = [("struct_size", C.c_size_t), ("eps", C.c_double), ("target", C.c_double), ("max_evals", C.c_ulonglong),
                ("pair_capacity", C.c_size_t)]


class ClearanceResult(C.Structure):
    """svsdf_clearance_result (include/svsdf_c.h)."""
    _fields_ = [("status", C.c_int), ("levels", C.c_int), ("lower", C.c_double), ("upper", C.c_double),
                ("t_witness", C.c_double), ("point_index", C.c_longlong), ("point_xy", C.c_double * 2),
                ("evals", C.c_ulonglong), ("pairs", C.c_ulonglong), ("tile_pairs", C.c_ulonglong),
                ("tile_pairs_kept", C.c_ulonglong), ("device_ms", C.c_double)]


CLEARANCE_STATUS = ["CONVERGED", "SAFE", "UNSAFE", "BUDGET"]     # SVSDF_CLEARANCE_*


class PointClearanceParams(C.Structure):
    """svsdf_point_clearance_params (include/svsdf_c.h)."""
    _fields_ = [("struct_size", C.c_size_t), ("eps", C.c_double), ("cap", C.c_double), ("target", C.c_double),
                ("max_evals", C.c_ulonglong), ("pair_capacity", C.c_size_t)]


class PointClearanceResult(C.Structure):
    """svsdf_point_clearance_result (include/svsdf_c.h)."""
    _fields_ = [("status", C.c_int), ("levels", C.c_int), ("counts", C.c_ulonglong * 5), ("lower", C.c_double),
                ("upper", C.c_double), ("t_witness", C.c_double), ("point_index", C.c_longlong), ("evals", C.c_ulonglong),
                ("pairs", C.c_ulonglong), ("tile_pairs", C.c_ulonglong), ("tile_pairs_kept", C.c_ulonglong),
                ("device_ms", C.c_double)]


POINT_STATE = ["CONVERGED", "FAR", "SAFE", "UNSAFE", "OPEN"]     # SVSDF_POINT_*


class OutlineStats(C.Structure):
    _fields_ = [("nodes_evaluated", C.c_ulonglong), ("dense_nodes", C.c_ulonglong), ("cells_marched", C.c_ulonglong),
                ("batches", C.c_ulonglong), ("open_chains", C.c_int)]


class SvsdfError(RuntimeError):
    pass


def lib_path():
    """In-tree HIP library.  SVSDF_LIB_VARIANT=<v> loads libsvsdf_hip_<v>.so instead (experimental builds
    made by tools/ scripts for A/B measurements; nothing in tests/ or bench.py sets it)."""
    v = os.environ.get("SVSDF_LIB_VARIANT", "")
    return os.path.join(_PKG, "libsvsdf_hip_%s.so" % v if v else "libsvsdf_hip.so")


def lib():
    """Load the HIP library.  Raises if it has not been built: there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise SvsdfError(f"{path} is missing: run `python __graft_entry__.py build` "
                         "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
    L = C.CDLL(path)
    L.svsdf_create.restype = C.c_void_p
    L.svsdf_create.argtypes = [C.POINTER(Config)]
    L.svsdf_destroy.argtypes = [C.c_void_p]
    L.svsdf_config_default.argtypes = [C.POINTER(Config)]
    L.svsdf_shape_id_from_inputdata.restype = C.c_int
    L.svsdf_shape_id_from_inputdata.argtypes = [C.c_char_p]
    L.svsdf_shape_name.restype = C.c_char_p
    L.svsdf_shape_name.argtypes = [C.c_int]
    L.svsdf_last_error_string.restype = C.c_char_p
    L.svsdf_last_error_string.argtypes = [C.c_void_p]
    L.svsdf_set_points.argtypes = [C.c_void_p, _dp, C.c_size_t]
    L.svsdf_set_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.svsdf_num_points.restype = C.c_size_t
    L.svsdf_num_points.argtypes = [C.c_void_p]
    L.svsdf_eval_penalty.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.svsdf_eval_penalty_partial.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_size_t)]
    L.svsdf_accumulate_partial.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    L.svsdf_sum_partials.argtypes = [_dp, C.c_int, C.c_size_t, _dp]
    L.svsdf_set_conditions.argtypes = [C.c_void_p, _dp, _dp]
    L.svsdf_shape_bound.argtypes = [C.c_void_p, _dp]
    L.svsdf_lmbm_evaluate.restype = C.c_double
    L.svsdf_lmbm_evaluate.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
    L.svsdf_last_costs.argtypes = [C.c_void_p, _dp]
    L.svsdf_lmbm_begin.argtypes = [C.c_void_p, _dp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.svsdf_lmbm_finish.restype = C.c_double
    L.svsdf_lmbm_finish.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
    L.svsdf_minco_coeffs.argtypes = [_dp, _dp, C.c_int, _dp, _dp, _dp]
    L.svsdf_forward_T.argtypes = [_dp, _dp, C.c_int]
    L.svsdf_backward_T.argtypes = [_dp, _dp, C.c_int]
    L.svsdf_query_points.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.svsdf_last_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.svsdf_last_launches.argtypes = [C.c_void_p, C.POINTER(LaunchRec), C.c_int, C.POINTER(C.c_int)]
    L.svsdf_set_scale.argtypes = [C.c_void_p, C.POINTER(Scale)]
    L.svsdf_get_scale.argtypes = [C.c_void_p, C.POINTER(Scale)]
    L.svsdf_shard_indices.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.svsdf_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.svsdf_shard_plan.argtypes = [_dp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong),
                                   C.POINTER(C.c_size_t)]
    L.svsdf_lmbm_prepare.argtypes = [C.c_void_p, _dp, C.c_int, _dp, _dp]
    _fp = C.POINTER(C.c_float)
    L.svsdf_map_create.restype = C.c_void_p
    L.svsdf_map_create.argtypes = [_fp, C.c_size_t, C.c_double, C.c_int]
    L.svsdf_map_destroy.argtypes = [C.c_void_p]
    L.svsdf_map_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_size_t)]
    L.svsdf_map_gather.argtypes = [C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.svsdf_pcd_read_ascii.argtypes = [C.c_char_p, _fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.svsdf_debug_sincos_mismatches.restype = C.c_longlong
    L.svsdf_debug_sincos_mismatches.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
    L.svsdf_debug_sqrt_mismatches.restype = C.c_longlong
    L.svsdf_debug_sqrt_mismatches.argtypes = [C.c_void_p, _dp, C.c_size_t, C.c_int]
    L.svsdf_lbfgs_params_default.argtypes = [C.POINTER(LbfgsParams)]
    L.svsdf_lbfgs_params_default.restype = None
    L.svsdf_lbfgs_minimize.argtypes = [C.c_int, _dp, EVALUATE_T, C.c_void_p, PROGRESS_T, C.c_void_p,
                                       C.POINTER(LbfgsParams), _dp, _ip, _ip]
    L.svsdf_optimize_traj.argtypes = [C.c_void_p, _dp, C.c_int, C.POINTER(LbfgsParams), PROGRESS_T, C.c_void_p,
                                      _dp, _ip, _ip]
    _u8p = C.POINTER(C.c_ubyte)
    L.svsdf_check_sub_sw_collision.argtypes = [C.c_void_p, C.c_size_t, _dp, _dp, C.POINTER(C.c_size_t), _dp, _u8p]
    L.svsdf_shape_kernels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, _u8p, _u8p, _dp,
                                      C.POINTER(C.c_int)]
    L.svsdf_frontend_set_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]
    L.svsdf_frontend_yaw_free.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_size_t, _ip]
    L.svsdf_map_build_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int]
    L.svsdf_map_device_get_info.argtypes = [C.c_void_p, C.POINTER(MapDeviceInfo)]
    L.svsdf_map_device_cells.argtypes = [C.c_void_p, _u8p, C.c_size_t]
    L.svsdf_frontend_set_map_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    L.svsdf_set_points_from_map.argtypes = [C.c_void_p, _dp, C.c_size_t, _dp, C.POINTER(C.c_size_t)]
    L.svsdf_map_device_points.argtypes = [C.c_void_p, _dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.svsdf_path_waypoints.argtypes = [C.c_size_t, C.c_double, C.c_double, C.POINTER(C.c_size_t), C.c_size_t,
                                       C.POINTER(C.c_size_t), _ip]
    L.svsdf_kernel_bfs.argtypes = [C.c_ulonglong, C.c_int, C.c_double, _dp, _ip]
    L.svsdf_astar_successors.argtypes = [C.c_void_p, C.c_size_t, _ip, _dp, _u8p, _dp, _u8p]
    L.svsdf_astar_params_default.argtypes = [C.POINTER(AstarParams)]
    L.svsdf_astar_params_default.restype = None
    L.svsdf_astar_search.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(AstarParams), _dp, _ip, C.c_size_t,
                                     C.POINTER(AstarResult)]
    L.svsdf_astar_nodes.argtypes = [C.c_void_p, C.POINTER(C.c_byte), _dp, _dp, _dp, _ip, C.c_size_t, _ip]
    L.svsdf_mesh_outline.argtypes = [_dp, C.c_size_t, _ip, C.c_size_t, C.c_double, _dp, C.c_size_t,
                                     C.POINTER(C.c_size_t), _ip]
    L.svsdf_mesh_outline_obj.argtypes = [C.c_char_p, C.c_double, _dp, C.c_size_t, C.POINTER(C.c_size_t), _ip]
    L.svsdf_swept_outline.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_size_t,
                                      C.POINTER(C.c_size_t), _ip, C.c_size_t, C.POINTER(C.c_size_t),
                                      C.POINTER(OutlineStats)]
    L.svsdf_outline_extrude.argtypes = [_dp, _ip, C.c_size_t, C.c_double, C.c_double, C.c_int, _dp, C.c_size_t,
                                        C.POINTER(C.c_size_t), _ip, C.c_size_t, C.POINTER(C.c_size_t)]
    L.svsdf_clearance_params_default.argtypes = [C.POINTER(ClearanceParams)]
    L.svsdf_clearance_params_default.restype = None
    L.svsdf_min_clearance.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(ClearanceParams), C.POINTER(ClearanceResult)]
    L.svsdf_motion_bounds.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_double, _dp]
    L.svsdf_scale_bounds.argtypes = [C.POINTER(Scale), C.c_double, C.c_double, _dp]
    L.svsdf_point_clearance_params_default.argtypes = [C.POINTER(PointClearanceParams)]
    L.svsdf_point_clearance_params_default.restype = None
    L.svsdf_point_clearance.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(PointClearanceParams), _dp, _dp, _dp,
                                        C.POINTER(C.c_ubyte), C.POINTER(PointClearanceResult)]
    if hasattr(L, "svsdf_mesh_section"):   # (the guards: absent only from A/B libraries built from older commits, tools/build_ref_variant.sh)
        L.svsdf_mesh_section.argtypes = [_dp, C.c_size_t, _ip, C.c_size_t, C.c_double, _dp, C.c_size_t, C.POINTER(C.c_size_t), _ip,
                                         C.c_size_t, C.POINTER(C.c_size_t)]
        L.svsdf_mesh_section_obj.argtypes = [C.c_char_p, C.c_double, _dp, C.c_size_t, C.POINTER(C.c_size_t), _ip, C.c_size_t,
                                             C.POINTER(C.c_size_t)]
    if hasattr(L, "svsdf_debug_sdf_at"):
        L.svsdf_debug_sdf_at.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_size_t, _dp, _dp, _dp]
    if hasattr(L, "svsdf_shape_selfcheck"):
        L.svsdf_shape_selfcheck.argtypes = [C.c_void_p, _dp]
    if hasattr(L, "svsdf_get_plan"):
        L.svsdf_get_plan.argtypes = [C.c_void_p, C.POINTER(Plan)]
        L.svsdf_set_plan.argtypes = [C.c_void_p, C.POINTER(Plan)]
        L.svsdf_set_combine.argtypes = [C.c_void_p, C.c_int]
        L.svsdf_group_info.argtypes = [C.c_void_p, _ip, _ip, _ip]
    if hasattr(L, "svsdf_debug_live_allocations"):
        L.svsdf_debug_live_allocations.restype = C.c_longlong
        L.svsdf_debug_live_allocations.argtypes = [C.POINTER(C.c_longlong)]
    if hasattr(L, "svsdf_group_stripe"):
        L.svsdf_group_stripe.argtypes = [C.c_void_p, C.c_int, _ip, C.POINTER(C.c_size_t), C.POINTER(Stats), C.POINTER(Plan)]
        L.svsdf_set_group_serial.argtypes = [C.c_void_p, C.c_int]
    _LIB = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _colmajor(m):
    """(rows, cols) array -> flat column-major copy (Eigen's default storage)."""
    return np.asfortranarray(_f64(m)).ravel(order="F").copy()


def _rows(cm, N):
    """flat column-major 3 x 6N coefficients (what the library takes and returns; _colmajor of (6N, 3)) -> (6N, 3)."""
    return cm.reshape(3, 6 * N).T.copy()


def kernel_bfs(mask, kernel_count, father_yaw):
    """checkKernelValue + visit_kernels_by_distance (sw_manager.hpp:1103-1169) on one cell's word of the yaw-free
    table (svsdf_kernel_bfs; host only).  Returns (child_yaw, kernel_index), None when no kernel is free within the
    search depth; raises ValueError for a yaw whose kernel index falls outside [0, kernel_count)."""
    cy, ki = C.c_double(0.0), C.c_int(0)
    rc = lib().svsdf_kernel_bfs(int(mask) & 0xFFFFFFFFFFFFFFFF, int(kernel_count), float(father_yaw), C.byref(cy), C.byref(ki))
    if rc < 0:
        raise ValueError(f"svsdf_kernel_bfs({int(mask):#x}, {kernel_count}, {father_yaw!r}) rejected its arguments ({rc})")
    return (cy.value, ki.value) if rc else None


def path_waypoints(path_len, grid_resolution, traj_parlength):
    """The waypoint indices of generateTraj (plan_manager.cpp:132-140, 157; svsdf_path_waypoints, host only): returns
    (indices int64 array, index_gap).  Raises ValueError for what the reference would not terminate on."""
    n, gap = C.c_size_t(), C.c_int()
    if int(path_len) < 0:
        raise ValueError("path_waypoints: negative path_len")
    args = (int(path_len), float(grid_resolution), float(traj_parlength))
    if lib().svsdf_path_waypoints(*args, None, 0, C.byref(n), C.byref(gap)):
        raise ValueError(f"svsdf_path_waypoints{args} rejected its arguments")
    idx = np.zeros(max(n.value, 1), dtype=np.uintp)
    if lib().svsdf_path_waypoints(*args, idx.ctypes.data_as(C.POINTER(C.c_size_t)), len(idx), C.byref(n), C.byref(gap)):
        raise ValueError(f"svsdf_path_waypoints{args} rejected its arguments")
    return idx[:n.value].astype(np.int64), gap.value


def motion_bounds(coeffs, T, ta, tb):
    """Rigorous (max planar speed, max |yaw rate|) of the trajectory on [ta, tb] clipped to [0, sum T]
    (svsdf_motion_bounds; host only).  coeffs (6N, 3), T (N,)."""
    T = _f64(T)
    cm = _colmajor(coeffs)
    o = np.zeros(2)
    rc = lib().svsdf_motion_bounds(len(T), _p(cm), _p(T), float(ta), float(tb), _p(o))
    if rc:
        raise SvsdfError(f"svsdf_motion_bounds failed ({rc}): " + lib().svsdf_last_error_string(None).decode())
    return float(o[0]), float(o[1])


def scale_bounds(schedule, ta, tb, enabled=True, struct_size=None):
    """Rigorous (Smin, Smax, Imax, Q) of a scale schedule over [ta, tb] (svsdf_scale_bounds; host only): the smallest and
    largest scale factor, the largest 1 / s_a and the largest |s_a'| / s_a^2.  schedule: None (the identity) or a dict
    c / amp / omega / phase like EXAMPLE_SCALE."""
    o = np.zeros(4)
    ref = None
    if schedule is not None:
        s = Scale()
        s.struct_size = C.sizeof(Scale) if struct_size is None else int(struct_size)
        s.enabled = int(bool(enabled))
        for name in ("c", "amp", "omega", "phase"):
            v = schedule.get(name, (1.0, 1.0) if name == "c" else (0.0, 0.0))
            getattr(s, name)[:] = [float(v[0]), float(v[1])]
        ref = C.byref(s)
    rc = lib().svsdf_scale_bounds(ref, float(ta), float(tb), _p(o))
    if rc:
        raise SvsdfError(f"svsdf_scale_bounds failed ({rc}): " + lib().svsdf_last_error_string(None).decode())
    return tuple(float(x) for x in o)


def live_allocations():
    """(count, bytes) of the library's live device + pinned allocations in this process (svsdf_debug_live_allocations)."""
    b = C.c_longlong(0)
    return int(lib().svsdf_debug_live_allocations(C.byref(b))), int(b.value)


def shape_id_from_inputdata(inputdata):
    return lib().svsdf_shape_id_from_inputdata(inputdata.encode())


def minco_coeffs(head_state, tail_state, inPs, T):
    """(3x3 head, 3x3 tail, (N-1, 3) waypoints, (N,) durations) -> (6N, 3) coefficients
    (row 6i+k = coefficient of s^k of piece i), via the product's host MINCO."""
    T = _f64(T)
    N = len(T)
    q = _f64(inPs).reshape(-1, 3).copy()
    out = np.zeros(18 * N)
    rc = lib().svsdf_minco_coeffs(_p(_colmajor(head_state)), _p(_colmajor(tail_state)), N, _p(q), _p(T), _p(out))
    if rc:
        raise SvsdfError(f"svsdf_minco_coeffs failed: {rc}")
    return _rows(out, N)


def mesh_outline(V, F, z0=0.0):
    """z = z0 cross-section of a triangle mesh (V (nv, 3), F (nf, 3) zero-based) -> (outline (n, 2), closed loops
    found); pure host (svsdf_mesh_outline).  The outline is what `polygon=` of SvsdfContext takes: BASELINE config 5."""
    V = _f64(V).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    n, loops = C.c_size_t(), C.c_int()
    rc = lib().svsdf_mesh_outline(_p(V), len(V), F.ctypes.data_as(_ip), len(F), float(z0), None, 0, C.byref(n), C.byref(loops))
    if rc:
        raise SvsdfError(f"svsdf_mesh_outline failed: {rc}")
    xy = np.zeros((n.value, 2))
    lib().svsdf_mesh_outline(_p(V), len(V), F.ctypes.data_as(_ip), len(F), float(z0), _p(xy), n.value, C.byref(n), C.byref(loops))
    return xy, loops.value


def mesh_section(V, F, z0=0.0):
    """All closed loops of the z = z0 section of a triangle mesh (svsdf_mesh_section): (xy (n, 2) loop after loop, largest
    enclosed area first; loop sizes)."""
    L = lib()
    V = _f64(V).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    n, nl = C.c_size_t(), C.c_size_t()
    rc = L.svsdf_mesh_section(_p(V), len(V), F.ctypes.data_as(_ip), len(F), float(z0), None, 0, C.byref(n), None, 0, C.byref(nl))
    if rc:
        raise SvsdfError("svsdf_mesh_section failed: " + L.svsdf_last_error_string(None).decode())
    xy = np.zeros((n.value, 2))
    sizes = np.zeros(nl.value, dtype=np.int32)
    rc = L.svsdf_mesh_section(_p(V), len(V), F.ctypes.data_as(_ip), len(F), float(z0), _p(xy), n.value, C.byref(n),
                              sizes.ctypes.data_as(_ip), nl.value, C.byref(nl))
    if rc:
        raise SvsdfError("svsdf_mesh_section failed: " + L.svsdf_last_error_string(None).decode())
    return xy, [int(v) for v in sizes]


def mesh_section_obj(path, z0=0.0):
    """The same for a Wavefront .obj file (svsdf_mesh_section_obj)."""
    L = lib()
    n, nl = C.c_size_t(), C.c_size_t()
    path = os.fspath(path)
    rc = L.svsdf_mesh_section_obj(path.encode(), float(z0), None, 0, C.byref(n), None, 0, C.byref(nl))
    if rc:
        raise SvsdfError("svsdf_mesh_section_obj failed: " + L.svsdf_last_error_string(None).decode())
    xy = np.zeros((n.value, 2))
    sizes = np.zeros(nl.value, dtype=np.int32)
    rc = L.svsdf_mesh_section_obj(path.encode(), float(z0), _p(xy), n.value, C.byref(n), sizes.ctypes.data_as(_ip), nl.value,
                                  C.byref(nl))
    if rc:
        raise SvsdfError("svsdf_mesh_section_obj failed: " + L.svsdf_last_error_string(None).decode())
    return xy, [int(v) for v in sizes]


def mesh_outline_obj(path, z0=0.0):
    """Same from a Wavefront .obj file (svsdf_mesh_outline_obj)."""
    n, loops = C.c_size_t(), C.c_int()
    rc = lib().svsdf_mesh_outline_obj(str(path).encode(), float(z0), None, 0, C.byref(n), C.byref(loops))
    if rc:
        raise SvsdfError(f"svsdf_mesh_outline_obj({path}) failed: {rc}")
    xy = np.zeros((n.value, 2))
    lib().svsdf_mesh_outline_obj(str(path).encode(), float(z0), _p(xy), n.value, C.byref(n), C.byref(loops))
    return xy, loops.value


def outline_extrude(loops, z0=-0.5, z1=0.5, caps=True):
    """Surface of the extrusion of closed polylines (svsdf_outline_extrude): V (nv, 3), F (nf, 3); walls and, with caps,
    the bottom and top faces (a closed surface).  Host only."""
    xy = _f64(np.vstack(loops))
    sizes = np.ascontiguousarray([len(lp) for lp in loops], dtype=np.int32)
    nv, nf = C.c_size_t(), C.c_size_t()
    L = lib()
    rc = L.svsdf_outline_extrude(_p(xy), sizes.ctypes.data_as(_ip), len(sizes), z0, z1, int(bool(caps)), None, 0,
                                 C.byref(nv), None, 0, C.byref(nf))
    if rc:
        raise SvsdfError(f"svsdf_outline_extrude failed: {rc}")
    V = np.zeros((nv.value, 3))
    F = np.zeros((nf.value, 3), dtype=np.int32)
    L.svsdf_outline_extrude(_p(xy), sizes.ctypes.data_as(_ip), len(sizes), z0, z1, int(bool(caps)), _p(V), nv.value,
                            C.byref(nv), F.ctypes.data_as(_ip), nf.value, C.byref(nf))
    return V, F


def forward_T(tau):
    tau = _f64(tau)
    T = np.zeros_like(tau)
    lib().svsdf_forward_T(_p(tau), _p(T), len(tau))
    return T


def backward_T(T):
    T = _f64(T)
    tau = np.zeros_like(T)
    lib().svsdf_backward_T(_p(T), _p(tau), len(T))
    return tau


class OccupancyMap:
    """Host-side query-point producer (PCSmapManager + the plan_manager waypoint loop)."""

    def __init__(self, cloud_xyz, resolution=1.0, sta_threshold=1):
        self.L = lib()
        pts = np.ascontiguousarray(cloud_xyz, dtype=np.float32).reshape(-1, 3)
        h = self.L.svsdf_map_create(pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts), float(resolution), int(sta_threshold))
        if not h:
            raise SvsdfError("svsdf_map_create failed")
        self.h = C.c_void_p(h)

    @staticmethod
    def read_pcd(path):
        L = lib()
        n = C.c_size_t()
        if L.svsdf_pcd_read_ascii(path.encode(), None, 0, C.byref(n)):
            raise SvsdfError(f"cannot read {path} as ASCII PCD (FIELDS x y z)")
        xyz = np.zeros((n.value, 3), dtype=np.float32)
        L.svsdf_pcd_read_ascii(path.encode(), xyz.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n))
        return xyz

    def info(self):
        dims = (C.c_int * 3)()
        bmin, bmax = np.zeros(3), np.zeros(3)
        occ = C.c_size_t()
        self.L.svsdf_map_info(self.h, dims, _p(bmin), _p(bmax), C.byref(occ))
        return dict(dims=tuple(dims), bmin=bmin, bmax=bmax, occupied=occ.value)

    def gather(self, centres, halfbd):
        c = _f64(centres).reshape(-1, 3)
        hb = _f64(halfbd).reshape(3)
        n = C.c_size_t()
        rc = self.L.svsdf_map_gather(self.h, _p(c), len(c), _p(hb), None, 0, C.byref(n))
        if rc:
            raise SvsdfError(f"svsdf_map_gather failed: {rc}")
        out = np.zeros((n.value, 3))
        if n.value:
            self.L.svsdf_map_gather(self.h, _p(c), len(c), _p(hb), _p(out), n.value, C.byref(n))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.svsdf_map_destroy(self.h)
                self.h = None
        except Exception:
            pass


FLAG_KEEP_INPUT_ORDER = 1
FLAG_HOST_ONLY = 2
FLAG_EXACT_PIECE_TIME = 4
FLAG_FAST_PIECE_TIME = 8
FLAG_POLYGON_YAW_KERNELS = 16   # Polygon contexts: yaw kernels and the front end (svsdf_c.h)
FLAG_SCALED_CLEARANCE = 32      # min_clearance / point_clearance under a scale schedule (svsdf_c.h)
COMBINE_AUTO, COMBINE_HOST, COMBINE_RCCL = 0, 1, 2


def sum_partials(partials):
    """(G, len) per-device partials -> their fixed-order sum (the multi-device context's host combine)."""
    p = np.ascontiguousarray(partials, dtype=np.float64)
    out = np.zeros(p.shape[1])
    rc = lib().svsdf_sum_partials(_p(p), p.shape[0], p.shape[1], _p(out))
    if rc:
        raise SvsdfError(f"svsdf_sum_partials failed: {rc}")
    return out


def shard_plan(xyz, rank, world_size, flags=0):
    """Original indices owned by `rank` (pure host; same plan svsdf_set_points uses)."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = C.c_size_t()
    idx = np.zeros(len(xyz), dtype=np.int64)
    rc = lib().svsdf_shard_plan(_p(xyz), len(xyz), rank, world_size, flags,
                                idx.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(n))
    if rc:
        raise SvsdfError(f"svsdf_shard_plan failed: {rc}")
    return idx[:n.value].copy()


def lbfgs_params(**kw):
    p = LbfgsParams()
    lib().svsdf_lbfgs_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown L-BFGS parameter %r" % k)
        setattr(p, k, v)
    return p


def _wrap_progress(progress):
    if progress is None:
        return C.cast(None, PROGRESS_T)

    def _cb(_user, x, g, fx, step, n, k, ls):
        xs = np.ctypeslib.as_array(x, shape=(n,)).copy()
        gs = np.ctypeslib.as_array(g, shape=(n,)).copy()
        return int(bool(progress(xs, gs, fx, step, k, ls)))
    return PROGRESS_T(_cb)


def lbfgs_minimize(fun, x0, progress=None, **params):
    """Generic driver over a Python callable fun(x) -> (f, g).  Returns (x, f, status, iterations, evaluations)."""
    x = _f64(x0).copy()
    n = len(x)

    def _ev(_inst, xp, gp, nn):
        f, g = fun(np.ctypeslib.as_array(xp, shape=(nn,)).copy())
        np.ctypeslib.as_array(gp, shape=(nn,))[:] = g
        return float(f)
    p = lbfgs_params(**params)
    f, it, ev = C.c_double(0.0), C.c_int(0), C.c_int(0)
    rc = lib().svsdf_lbfgs_minimize(n, _p(x), EVALUATE_T(_ev), None, _wrap_progress(progress), None, C.byref(p),
                                    C.byref(f), C.byref(it), C.byref(ev))
    return x, f.value, rc, it.value, ev.value


class SvsdfContext:
    """Owns one svsdf_ctx (one GPU, one shard of the query points)."""

    def __init__(self, shape="star", safety_hor=0.7, weight_p=60.0, rho=3.8,
                 poly_params=(0.0, 0.0, 0.0), polygon=None, head_state=None, tail_state=None,
                 device=-1, rank=0, world_size=1, flags=0, devices=None, combine=COMBINE_AUTO, polygon_loops=None):
        """polygon_loops: vertex counts of the closed loops `polygon` is made of (mesh_section); None: one loop."""
        self.L = lib()
        cfg = Config()
        self.L.svsdf_config_default(C.byref(cfg))
        cfg.shape_id = SHAPE_ID[shape] if isinstance(shape, str) else int(shape)
        cfg.poly_params[:] = list(map(float, poly_params))
        cfg.safety_hor, cfg.weight_p, cfg.rho = float(safety_hor), float(weight_p), float(rho)
        hs = np.zeros((3, 3)) if head_state is None else _f64(head_state)
        ts = np.zeros((3, 3)) if tail_state is None else _f64(tail_state)
        cfg.head_state[:] = list(_colmajor(hs))
        cfg.tail_state[:] = list(_colmajor(ts))
        cfg.device, cfg.rank, cfg.world_size, cfg.flags = int(device), int(rank), int(world_size), int(flags)
        if devices is not None and (len(devices) >= 2 or int(combine) == COMBINE_RCCL):    # in-process multi-GPU
            cfg.n_devices = len(devices)
            for k, d in enumerate(devices):
                cfg.devices[k] = int(d)
        elif devices is not None and len(devices) == 1:                                    # a list of one: that device
            cfg.device = int(devices[0])
        cfg.combine = int(combine)
        self._poly = None
        if polygon is not None:
            self._poly = _f64(polygon).reshape(-1, 2).copy()
            cfg.polygon_nverts = len(self._poly)
            cfg.polygon_xy = _p(self._poly)
            if polygon_loops is not None and len(polygon_loops) >= 2:
                self._loops = (C.c_int * len(polygon_loops))(*[int(v) for v in polygon_loops])
                cfg.polygon_nloops = len(polygon_loops)
                cfg.polygon_loop_sizes = C.cast(self._loops, C.POINTER(C.c_int))
        h = self.L.svsdf_create(C.byref(cfg))
        if not h:
            raise SvsdfError("svsdf_create failed: " + self.L.svsdf_last_error_string(None).decode())
        self.ctx = C.c_void_p(h)
        self.head_state, self.tail_state = hs, ts
        self._world_size = int(world_size)

    def close(self):
        if getattr(self, "ctx", None):
            self.L.svsdf_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise SvsdfError(f"{what} failed ({rc}): " + self.L.svsdf_last_error_string(self.ctx).decode())

    def set_conditions(self, head_state, tail_state):
        hs, ts = _f64(head_state).reshape(3, 3), _f64(tail_state).reshape(3, 3)
        self._chk(self.L.svsdf_set_conditions(self.ctx, _p(_colmajor(hs)), _p(_colmajor(ts))), "svsdf_set_conditions")
        self.head_state, self.tail_state = hs, ts

    # ---- points ----
    def set_points(self, xyz):
        xyz = _f64(xyz).reshape(-1, 3)
        self._chk(self.L.svsdf_set_points(self.ctx, _p(xyz), len(xyz)), "svsdf_set_points")

    def set_points_device(self, dev_ptr, P):
        self._chk(self.L.svsdf_set_points_device(self.ctx, C.c_void_p(int(dev_ptr)), int(P)), "svsdf_set_points_device")

    def num_points(self):
        return int(self.L.svsdf_num_points(self.ctx))

    def shard_indices(self):
        idx = np.zeros(self.num_points(), dtype=np.int64)
        if len(idx):
            self._chk(self.L.svsdf_shard_indices(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_longlong))), "svsdf_shard_indices")
        return idx

    # ---- inner operator ----
    def eval_penalty(self, coeffs, T, cost0=0.0, gradT0=None, gradC0=None):
        """coeffs (6N, 3), T (N,) -> (cost, gradT (N,), gradC (6N, 3)); accumulates like BEO:774-869."""
        T = _f64(T)
        N = len(T)
        cm = _colmajor(coeffs)
        cost = C.c_double(cost0)
        gT = np.zeros(N) if gradT0 is None else _f64(gradT0).copy()
        gC = np.zeros(18 * N) if gradC0 is None else _colmajor(gradC0)
        self._chk(self.L.svsdf_eval_penalty(self.ctx, N, _p(cm), _p(T), C.byref(cost), _p(gT), _p(gC)), "svsdf_eval_penalty")
        return cost.value, gT, _rows(gC, N)

    def eval_penalty_partial(self, coeffs, T):
        """Runs the device pipeline; returns (device pointer, length) of [cost, gradC, gradT]."""
        T = _f64(T)
        N = len(T)
        cm = _colmajor(coeffs)
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.svsdf_eval_penalty_partial(self.ctx, N, _p(cm), _p(T), C.byref(ptr), C.byref(n)), "svsdf_eval_penalty_partial")
        return ptr.value, n.value

    def accumulate_partial(self, N, partial, cost0=0.0, gradT0=None, gradC0=None):
        partial = _f64(partial)
        cost = C.c_double(cost0)
        gT = np.zeros(N) if gradT0 is None else _f64(gradT0).copy()
        gC = np.zeros(18 * N) if gradC0 is None else _colmajor(gradC0)
        self._chk(self.L.svsdf_accumulate_partial(self.ctx, N, _p(partial), C.byref(cost), _p(gT), _p(gC)), "svsdf_accumulate_partial")
        return cost.value, gT, _rows(gC, N)

    # ---- full callback ----
    def lmbm_evaluate(self, x):
        x = _f64(x)
        g = np.zeros_like(x)
        f = self.L.svsdf_lmbm_evaluate(self.ctx, _p(x), _p(g), len(x))
        if not np.isfinite(f):
            raise SvsdfError("svsdf_lmbm_evaluate failed: " + self.L.svsdf_last_error_string(self.ctx).decode())
        return f, g

    def last_costs(self):
        c = np.zeros(3)
        self.L.svsdf_last_costs(self.ctx, _p(c))
        return c

    def lmbm_begin(self, x):
        x = _f64(x)
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.svsdf_lmbm_begin(self.ctx, _p(x), len(x), C.byref(ptr), C.byref(n)), "svsdf_lmbm_begin")
        return ptr.value, n.value

    def lmbm_prepare(self, x):
        """Host half of lmbm_begin: returns (coeffs (6N, 3), T (N,)) the device stage receives."""
        x = _f64(x)
        N = (len(x) + 3) // 4
        cm, T = np.zeros(18 * N), np.zeros(N)
        self._chk(self.L.svsdf_lmbm_prepare(self.ctx, _p(x), len(x), _p(cm), _p(T)), "svsdf_lmbm_prepare")
        return _rows(cm, N), T

    def lmbm_finish(self, partial, n):
        partial = _f64(partial)
        g = np.zeros(n)
        f = self.L.svsdf_lmbm_finish(self.ctx, _p(partial), _p(g), n)
        if not np.isfinite(f):
            raise SvsdfError("svsdf_lmbm_finish failed: " + self.L.svsdf_last_error_string(self.ctx).decode())
        return f, g

    # ---- diagnostics ----
    def swept_outline(self, coeffs, T, cell=0.05, margin=0.0):
        """Boundary of the swept volume's z = 0 section (svsdf_swept_outline; what the reference's sw_calculate /
        calculateSwept are for): list of (n_i, 2) closed polylines, inside on the left, + the work statistics."""
        T = _f64(T)
        N = len(T)
        cm = _colmajor(coeffs)
        nv, nl, st = C.c_size_t(), C.c_size_t(), OutlineStats()
        self._chk(self.L.svsdf_swept_outline(self.ctx, N, _p(cm), _p(T), float(cell), float(margin), None, 0,
                                             C.byref(nv), None, 0, C.byref(nl), C.byref(st)), "svsdf_swept_outline")
        xy = np.zeros((nv.value, 2))
        sizes = np.zeros(max(nl.value, 1), dtype=np.int32)
        if nv.value:
            self._chk(self.L.svsdf_swept_outline(self.ctx, N, _p(cm), _p(T), float(cell), float(margin), _p(xy), nv.value,
                                                 C.byref(nv), sizes.ctypes.data_as(_ip), nl.value, C.byref(nl),
                                                 C.byref(st)), "svsdf_swept_outline")
        loops, off = [], 0
        for n in sizes[:nl.value]:
            loops.append(xy[off:off + int(n)].copy())
            off += int(n)
        return loops, {k: getattr(st, k) for k, _ in OutlineStats._fields_}

    def query_points(self, coeffs, T):
        """Per-point (sdf, t*, grad_xy) in the ORIGINAL order of the points given to set_points
        (world_size == 1) or of this rank's shard (see shard_indices)."""
        T = _f64(T)
        N = len(T)
        cm = _colmajor(coeffs)
        P = self.num_points()
        sdf, ts, g = np.zeros(P), np.zeros(P), np.zeros((P, 2))
        self._chk(self.L.svsdf_query_points(self.ctx, N, _p(cm), _p(T), _p(sdf), _p(ts), _p(g)), "svsdf_query_points")
        idx = self.shard_indices()
        order = np.argsort(idx, kind="stable")
        return sdf[order], ts[order], g[order], idx[order]

    # ---- optimizer driver ----
    def optimize_traj(self, x, progress=None, **params):
        """optimize_traj_lmbm analogue (back_end_optimizer.cpp:3-95) with the in-library L-BFGS driver.
        Returns (x_opt, final_cost, status, iterations, evaluations)."""
        x = _f64(x).copy()
        p = lbfgs_params(**params)
        f, it, ev = C.c_double(0.0), C.c_int(0), C.c_int(0)
        cb = _wrap_progress(progress)
        rc = self.L.svsdf_optimize_traj(self.ctx, _p(x), len(x), C.byref(p), cb, None, C.byref(f), C.byref(it),
                                        C.byref(ev))
        return x, f.value, rc, it.value, ev.value

    # ---- front end ----
    def check_sub_sw_collision(self, father_states, child_states, points_per_edge):
        """Batched SweptVolumeManager::checkSubSWCollision (sw_manager.hpp:1171-1211).

        father_states / child_states: (E, 3) arrays of (x, y, yaw); points_per_edge: sequence of E
        (n_e, 2) obstacle-point arrays.  Returns a bool array, True where the reference returns true."""
        fs = _f64(father_states).reshape(-1, 3)
        cs = _f64(child_states).reshape(-1, 3)
        E = len(fs)
        if len(cs) != E or len(points_per_edge) != E:
            raise ValueError("check_sub_sw_collision: one child state and one point set per edge")
        pts = [_f64(q).reshape(-1, 2) for q in points_per_edge]
        offs = np.zeros(E + 1, dtype=np.uintp)
        if E:
            offs[1:] = np.cumsum([len(q) for q in pts])
        flat = np.ascontiguousarray(np.concatenate(pts, axis=0)) if E and offs[-1] else np.zeros((0, 2))
        out = np.zeros(max(E, 1), dtype=np.uint8)
        self._chk(self.L.svsdf_check_sub_sw_collision(
            self.ctx, E, _p(fs), _p(cs), offs.ctypes.data_as(C.POINTER(C.c_size_t)), _p(flat),
            out.ctypes.data_as(C.POINTER(C.c_ubyte))), "svsdf_check_sub_sw_collision")
        return out[:E].astype(bool)

    def shape_kernels(self, kernel_size, kernel_count, resolution, safemargin):
        """BasicShape::initShape (Shape.hpp:386-430): returns (map (K, ks, ks) bool, bytes (K, ks, (ks+7)//8)
        uint8, yaws (K,), loop_count)."""
        ks, K = int(kernel_size), int(kernel_count)
        m = np.zeros((K, ks, ks), dtype=np.uint8)
        b = np.zeros((K, ks, (ks + 7) // 8), dtype=np.uint8)
        yaws = np.zeros(K)
        n = C.c_int(0)
        u8 = C.POINTER(C.c_ubyte)
        self._chk(self.L.svsdf_shape_kernels(self.ctx, ks, K, float(resolution), float(safemargin),
                                             m.ctypes.data_as(u8), b.ctypes.data_as(u8), _p(yaws), C.byref(n)),
                  "svsdf_shape_kernels")
        return m.astype(bool), b, yaws, n.value

    def frontend_set_map(self, occupancy_map, kernel_size, kernel_count, safemargin):
        """Make `occupancy_map` (an OccupancyMap) the resident front-end map: layer 0 as a bitmap, the yaw kernels of
        shape_kernels at the map's resolution, and the yaw-free table (svsdf_frontend_set_map)."""
        self._chk(self.L.svsdf_frontend_set_map(self.ctx, occupancy_map.h, int(kernel_size), int(kernel_count),
                                                float(safemargin)), "svsdf_frontend_set_map")

    # ---- the producer on the device (svsdf_map_build_device ...) ----
    def map_build(self, cloud, resolution=1.0, sta_threshold=1):
        """Build the device-resident occupancy map (svsdf_map_build_device).  cloud: (n, 3) float32 numpy array, or a
        contiguous float32 torch tensor on the context's (first) device, passed by data_ptr()."""
        if hasattr(cloud, "data_ptr"):
            if str(cloud.dtype) != "torch.float32" or not cloud.is_contiguous() or cloud.numel() % 3:
                raise ValueError("map_build: a device cloud must be a contiguous float32 tensor of n x 3 values")
            ptr, n, on_dev = C.c_void_p(cloud.data_ptr() if cloud.numel() else None), cloud.numel() // 3, int(cloud.is_cuda)
            keep = cloud
        else:
            keep = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
            ptr, n, on_dev = C.c_void_p(keep.ctypes.data if len(keep) else None), len(keep), 0
        self._chk(self.L.svsdf_map_build_device(self.ctx, ptr, n, on_dev, float(resolution), int(sta_threshold)),
                  "svsdf_map_build_device")
        del keep

    def map_info(self):
        """svsdf_map_device_get_info as a dict: dims (tuple), bmin, bmax (arrays), resolution, sta_threshold, n_cloud,
        occupied, gathered, build_ms, gather_ms."""
        s = MapDeviceInfo()
        s.struct_size = C.sizeof(MapDeviceInfo)
        self._chk(self.L.svsdf_map_device_get_info(self.ctx, C.byref(s)), "svsdf_map_device_get_info")
        out = {k: getattr(s, k) for k, _ in MapDeviceInfo._fields_ if k not in ("struct_size", "dims", "bmin", "bmax")}
        out.update(dims=tuple(s.dims), bmin=np.array(list(s.bmin)), bmax=np.array(list(s.bmax)))
        return out

    def map_cells(self):
        """The resident map's occupancy as a uint8 (X, Y, Z) array (svsdf_map_device_cells); dims below 1 count as 0."""
        X, Y, Z = (max(0, d) for d in self.map_info()["dims"])
        out = np.zeros((X, Y, Z), dtype=np.uint8)
        self._chk(self.L.svsdf_map_device_cells(self.ctx, out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size),
                  "svsdf_map_device_cells")
        return out

    def frontend_set_map_resident(self, kernel_size, kernel_count, safemargin):
        """frontend_set_map from the resident map, packed on the device (svsdf_frontend_set_map_device)."""
        self._chk(self.L.svsdf_frontend_set_map_device(self.ctx, int(kernel_size), int(kernel_count), float(safemargin)),
                  "svsdf_frontend_set_map_device")

    def set_points_from_map(self, centres, halfbd):
        """Gather the resident map's occupied voxels around `centres` (n, 3) -- boxes of half extents `halfbd` (3,), each
        minus the previous centre's -- and make them the resident cloud (svsdf_set_points_from_map).  Returns the count."""
        c = _f64(centres).reshape(-1, 3)
        hb = _f64(halfbd).reshape(3)
        n = C.c_size_t()
        self._chk(self.L.svsdf_set_points_from_map(self.ctx, _p(c), len(c), _p(hb), C.byref(n)), "svsdf_set_points_from_map")
        return int(n.value)

    def map_points(self):
        """The last gather in unified-voxel-id order, (n, 3) float64: what OccupancyMap.gather returns (svsdf_map_device_points)."""
        n = C.c_size_t()
        self._chk(self.L.svsdf_map_device_points(self.ctx, None, 0, C.byref(n)), "svsdf_map_device_points")
        out = np.zeros((n.value, 3))
        if n.value:
            self._chk(self.L.svsdf_map_device_points(self.ctx, _p(out), n.value, C.byref(n)), "svsdf_map_device_points")
        return out

    def yaw_free(self):
        """The yaw-free table as a uint64 (X, Y) array: bit k of [ix, iy] is set iff kernelConv<true>(k, (ix, iy, 0))
        (sw_manager.hpp:1033-1099) returns true."""
        dims = (C.c_int * 2)()
        self._chk(self.L.svsdf_frontend_yaw_free(self.ctx, None, 0, dims), "svsdf_frontend_yaw_free")
        out = np.zeros((dims[0], dims[1]), dtype=np.uint64)
        self._chk(self.L.svsdf_frontend_yaw_free(self.ctx, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size, dims),
                  "svsdf_frontend_yaw_free")
        return out

    def astar_successors(self, parent_ij, parent_yaw):
        """AstarGetSucc's test (front_end_Astar.hpp:192-241) of the 9 neighbours of every parent on the resident map.
        parent_ij: (n, 2) cell indices, parent_yaw: (n,).  Returns (ok (n, 9) bool, child_yaw (n, 9), stage (n, 9) uint8),
        slot 3 (i + 1) + (j + 1); stage 0 accepted, 1 invalid, 2 occupied, 3 no yaw kernel, 4 sub-swept collision."""
        ij = np.ascontiguousarray(parent_ij, dtype=np.int32).reshape(-1, 2)
        yaw = _f64(parent_yaw).reshape(-1)
        n = len(ij)
        if len(yaw) != n:
            raise ValueError("astar_successors: one yaw per parent")
        ok = np.zeros((n, 9), dtype=np.uint8)
        cy = np.full((n, 9), np.nan)
        stage = np.zeros((n, 9), dtype=np.uint8)
        u8 = C.POINTER(C.c_ubyte)
        self._chk(self.L.svsdf_astar_successors(self.ctx, n, ij.ctypes.data_as(_ip), _p(yaw), ok.ctypes.data_as(u8), _p(cy),
                                                stage.ctypes.data_as(u8)), "svsdf_astar_successors")
        return ok.astype(bool), cy, stage

    def astar_search(self, start, end, start_yaw=0.0, max_expansions=0, slice=0, capacity=None):
        """AstarPathSearch(start, end) + getPath (front_end_Astar.hpp:243-390) on the resident map, on the device
        (svsdf_astar_search).  start / end: world points (x, y, z).  Returns a dict: status ("FOUND", "EXHAUSTED", "LIMIT",
        "OUT_OF_MAP"), path (n, 3) float64 (centre x, centre y, yaw), cells (n, 2) int32, path_len, and the counters
        expansions, pushes, relaxed_open, reopened, launches, stage_counts (5,), g_goal.  `capacity` (cells; default: ask
        first, then fetch) is what the output arrays are sized to."""
        s, e = _f64(start).reshape(3).copy(), _f64(end).reshape(3).copy()
        prm = AstarParams()
        self.L.svsdf_astar_params_default(C.byref(prm))
        prm.start_yaw, prm.max_expansions, prm.slice = float(start_yaw), int(max_expansions), int(slice)
        res = AstarResult()
        res.struct_size = C.sizeof(AstarResult)
        if capacity is None:     # the search runs once: the first call leaves the path on the device side of the result
            dims = (C.c_int * 2)()
            self._chk(self.L.svsdf_astar_nodes(self.ctx, None, None, None, None, None, 0, dims), "svsdf_astar_nodes")
            capacity = dims[0] * dims[1] + 1
        n = int(capacity)
        path = np.zeros((n, 3))
        cells = np.zeros((n, 2), dtype=np.int32)
        self._chk(self.L.svsdf_astar_search(self.ctx, _p(s), _p(e), C.byref(prm), _p(path), cells.ctypes.data_as(_ip), n,
                                            C.byref(res)), "svsdf_astar_search")
        k = int(res.path_len)
        out = {"status": ASTAR_STATUS[res.status], "path": path[:k].copy(), "cells": cells[:k].copy(), "path_len": k,
               "stage_counts": np.array(list(res.stage_counts), dtype=np.uint64), "g_goal": float(res.g_goal)}
        for key in ("expansions", "pushes", "relaxed_open", "reopened", "launches"):
            out[key] = int(getattr(res, key))
        return out

    def astar_nodes(self):
        """The node records the last astar_search left behind (svsdf_astar_nodes), a dict of (X, Y) arrays: id int8 (0
        untouched, 1 open, -1 closed), g, f, yaw float64, father_cell int32 (ix * Y + iy; -1 none, -2 the start node)."""
        dims = (C.c_int * 2)()
        self._chk(self.L.svsdf_astar_nodes(self.ctx, None, None, None, None, None, 0, dims), "svsdf_astar_nodes")
        X, Y = dims[0], dims[1]
        out = {"id": np.zeros((X, Y), dtype=np.int8), "g": np.zeros((X, Y)), "f": np.zeros((X, Y)), "yaw": np.zeros((X, Y)),
               "father_cell": np.zeros((X, Y), dtype=np.int32)}
        self._chk(self.L.svsdf_astar_nodes(self.ctx, out["id"].ctypes.data_as(C.POINTER(C.c_byte)), _p(out["g"]), _p(out["f"]),
                                           _p(out["yaw"]), out["father_cell"].ctypes.data_as(_ip), X * Y, dims),
                  "svsdf_astar_nodes")
        return out

    def debug_sdf_at(self, coeffs, T, points_xy, t):
        """SDF-at-time of (point, time) pairs on the device with its intermediates (svsdf_debug_sdf_at): (n, 8) array
        sdf, pose x, y, cos, sin, body-frame x, y, piece-time mode."""
        T = _f64(T)
        cm = _colmajor(coeffs)
        xy = _f64(points_xy).reshape(-1, 2).copy()
        tt = _f64(t).ravel().copy()
        out = np.zeros((len(tt), 8))
        self._chk(self.L.svsdf_debug_sdf_at(self.ctx, len(T), _p(cm), _p(T), len(tt), _p(xy), _p(tt), _p(out)), "svsdf_debug_sdf_at")
        return out

    def min_clearance(self, coeffs, T, eps=1e-3, target=None, max_evals=0, pair_capacity=0, struct_size=None):
        """Certified bracket lower <= c* <= upper on the minimum over the resident cloud and over [0, sum T] of the
        SDF-at-time, with a witness (svsdf_min_clearance).  Under a scale schedule (a context created with
        FLAG_SCALED_CLEARANCE) the value is the scaled one, debug_sdf_at's under the schedule.  Returns the fields of svsdf_clearance_result as a dict
        (status as one of CLEARANCE_STATUS, point_xy as a tuple).  target=None: no target."""
        T = _f64(T)
        cm = _colmajor(coeffs)
        prm = ClearanceParams()
        self.L.svsdf_clearance_params_default(C.byref(prm))
        prm.eps = float(eps)
        if target is not None:
            prm.target = float(target)
        prm.max_evals, prm.pair_capacity = int(max_evals), int(pair_capacity)
        if struct_size is not None:
            prm.struct_size = int(struct_size)
        res = ClearanceResult()
        self._chk(self.L.svsdf_min_clearance(self.ctx, len(T), _p(cm), _p(T), C.byref(prm), C.byref(res)), "svsdf_min_clearance")
        out = {k: getattr(res, k) for k, _ in ClearanceResult._fields_}
        out["status"] = CLEARANCE_STATUS[res.status]
        out["point_xy"] = (res.point_xy[0], res.point_xy[1])
        return out

    def point_clearance(self, coeffs, T, eps=1e-3, cap=None, target=None, max_evals=0, pair_capacity=0, struct_size=None):
        """Certified bracket lower[p] <= c_p <= upper[p] on every resident point's minimum over [0, sum T] of the
        SDF-at-time, with the time of the evaluation that gave upper[p] (svsdf_point_clearance).  Returns (lower, upper,
        t_witness, state names, result): four arrays in the svsdf_set_points order (the states as POINT_STATE names) and
        the fields of svsdf_point_clearance_result as a dict (status as one of CLEARANCE_STATUS, counts keyed by state
        name).  cap=None: no cap; target=None: no target."""
        T = _f64(T)
        cm = _colmajor(coeffs)
        prm = PointClearanceParams()
        self.L.svsdf_point_clearance_params_default(C.byref(prm))
        prm.eps = float(eps)
        if cap is not None:
            prm.cap = float(cap)
        if target is not None:
            prm.target = float(target)
        prm.max_evals, prm.pair_capacity = int(max_evals), int(pair_capacity)
        if struct_size is not None:
            prm.struct_size = int(struct_size)
        P = int(self.num_points())
        if P and self._world_size > 1:      # a rank's shard: the arrays span the whole svsdf_set_points array
            P = int(self.shard_indices().max()) + 1
        lower, upper, tw = np.zeros(P), np.zeros(P), np.zeros(P)
        state = np.zeros(P, dtype=np.uint8)
        res = PointClearanceResult()
        self._chk(self.L.svsdf_point_clearance(self.ctx, len(T), _p(cm), _p(T), C.byref(prm), _p(lower), _p(upper), _p(tw),
                                               state.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(res)), "svsdf_point_clearance")
        out = {k: getattr(res, k) for k, _ in PointClearanceResult._fields_}
        out["status"] = CLEARANCE_STATUS[res.status]
        out["counts"] = {name: int(res.counts[i]) for i, name in enumerate(POINT_STATE)}
        return lower, upper, tw, np.array(POINT_STATE)[state], out

    def sincos_mismatches(self, lo, hi, n):
        return int(self.L.svsdf_debug_sincos_mismatches(self.ctx, float(lo), float(hi), int(n)))

    def sqrt_mismatches(self, x, flavour):
        """Operands of x (float64 bit patterns kept as given) whose unscaled device sqrt differs from sqrt; flavour 0 / 1."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        return int(self.L.svsdf_debug_sqrt_mismatches(self.ctx, _p(x), x.size, int(flavour)))

    def shape_bound(self):
        """(analytic R with sdf(q) >= |q| - R, largest |q| - sdf(q) sampled at creation)."""
        o = np.zeros(2)
        self._chk(self.L.svsdf_shape_bound(self.ctx, _p(o)), "svsdf_shape_bound")
        return float(o[0]), float(o[1])

    def shape_selfcheck(self):
        """(R analytic, R sampled, Lipschitz excess: 0 = the shape SDF passed the 1-Lipschitz self-check)."""
        o = np.zeros(3)
        self._chk(self.L.svsdf_shape_selfcheck(self.ctx, _p(o)), "svsdf_shape_selfcheck")
        return float(o[0]), float(o[1]), float(o[2])

    def set_scale(self, c=None, amp=(0.0, 0.0), omega=(0.0, 0.0), phase=(0.0, 0.0), enabled=True, struct_size=None):
        """Time-varying robot scale (svsdf_set_scale): s_a(t) = c[a] + sin(omega[a] t + phase[a]) amp[a], a = x, y.
        c=None (or enabled=False) restores the rigid path; EXAMPLE_SCALE holds the reference's worked example."""
        if c is None:
            self._chk(self.L.svsdf_set_scale(self.ctx, None), "svsdf_set_scale")
            return
        s = Scale()
        s.struct_size = C.sizeof(Scale) if struct_size is None else int(struct_size)
        s.enabled = int(bool(enabled))
        for name, v in (("c", c), ("amp", amp), ("omega", omega), ("phase", phase)):
            getattr(s, name)[:] = [float(v[0]), float(v[1])]
        self._chk(self.L.svsdf_set_scale(self.ctx, C.byref(s)), "svsdf_set_scale")

    def get_scale(self):
        """The schedule in force (svsdf_get_scale): None on the rigid path, else a dict c / amp / omega / phase."""
        s = Scale()
        s.struct_size = C.sizeof(Scale)
        self._chk(self.L.svsdf_get_scale(self.ctx, C.byref(s)), "svsdf_get_scale")
        if not s.enabled:
            return None
        return {k: (float(getattr(s, k)[0]), float(getattr(s, k)[1])) for k in ("c", "amp", "omega", "phase")}

    def get_plan(self):
        """Launch plan in force (svsdf_get_plan): bound_mode, batches, lanes_per_query, tail_iter, settled, layer_tables."""
        pl = Plan()
        self._chk(self.L.svsdf_get_plan(self.ctx, C.byref(pl)), "svsdf_get_plan")
        return {k: getattr(pl, k) for k, _ in Plan._fields_}

    def set_plan(self, bound_mode=PLAN_AUTO, batches=PLAN_AUTO, lanes_per_query=PLAN_AUTO, tail_iter=PLAN_AUTO,
                 layer_tables=PLAN_AUTO):
        """Pin fields of the launch plan (svsdf_set_plan; PLAN_AUTO leaves a field to its rule; batches=-2: measured).
        Only moves time: every plan returns the same bits."""
        pl = Plan(int(bound_mode), int(batches), int(lanes_per_query), int(tail_iter), 0, int(layer_tables))
        self._chk(self.L.svsdf_set_plan(self.ctx, C.byref(pl)), "svsdf_set_plan")

    def set_combine(self, combine):
        """Multi-device contexts: 'host' or 'rccl' sum of the devices' partials (svsdf_set_combine)."""
        code = {"host": 1, "rccl": 2}.get(combine, combine)
        self._chk(self.L.svsdf_set_combine(self.ctx, int(code)), "svsdf_set_combine")

    def group_info(self):
        """(devices, combine mode, ranks of the RCCL communicator as the communicator reports them; 0: none)."""
        nd, cb, rk = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.svsdf_group_info(self.ctx, C.byref(nd), C.byref(cb), C.byref(rk)), "svsdf_group_info")
        return {"n_devices": nd.value, "combine": ["auto", "host", "rccl"][cb.value], "rccl_ranks": rk.value}

    def group_stripe(self, k):
        """Stripe k of a multi-device context (svsdf_group_stripe): device, points, its stats and plan."""
        dev, pts, st, pl = C.c_int(), C.c_size_t(), Stats(), Plan()
        self._chk(self.L.svsdf_group_stripe(self.ctx, int(k), C.byref(dev), C.byref(pts), C.byref(st), C.byref(pl)), "svsdf_group_stripe")
        return {"device": dev.value, "points": pts.value, "stats": {n: getattr(st, n) for n, _ in Stats._fields_},
                "plan": {n: getattr(pl, n) for n, _ in Plan._fields_}}

    def set_group_serial(self, serial=True):
        """Diagnostic: the stripes of a multi-device context one after the other (svsdf_set_group_serial)."""
        self._chk(self.L.svsdf_set_group_serial(self.ctx, int(bool(serial))), "svsdf_set_group_serial")

    def set_profiling(self, enable=True):
        self._chk(self.L.svsdf_set_profiling(self.ctx, int(enable)), "svsdf_set_profiling")   # 2: serialised batches

    def last_launches(self):
        """Launch record of the last evaluation (svsdf_last_launches): one dict per device launch, in launch order, with
        `kernel` as a name ("solve", "round", "tail", ...) and `targ` as a tuple of the template arguments.  Raises when
        the evaluation made more launches than the library records."""
        recs = (LaunchRec * LAUNCH_REC_CAP)()
        recs[0].struct_size = C.sizeof(LaunchRec)
        n = C.c_int(0)
        self._chk(self.L.svsdf_last_launches(self.ctx, recs, LAUNCH_REC_CAP, C.byref(n)), "svsdf_last_launches")
        if n.value > LAUNCH_REC_CAP:
            raise SvsdfError(f"svsdf_last_launches: {n.value} launches, {LAUNCH_REC_CAP} recorded")
        out = []
        for r in recs[:n.value]:
            d = {k: getattr(r, k) for k, _ in LaunchRec._fields_ if k != "struct_size"}
            d["kernel"] = KERNELS[r.kernel]
            d["targ"] = tuple(r.targ)
            out.append(d)
        return out

    def stats(self):
        s = Stats()
        self.L.svsdf_last_stats(self.ctx, C.byref(s))
        return {k: getattr(s, k) for k, _ in Stats._fields_}
