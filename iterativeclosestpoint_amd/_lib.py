"""ctypes binding of libicp_hip.so (harness only; the product is the C-ABI library)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
LIB_PATH = Path(os.environ.get("ICP_HIP_LIB", PKG_DIR / "libicp_hip.so"))  # override: A/B of builds

RULES_ENGINE = 0
RULES_CLI = 1
FLAG_NO_EARLY_STOP = 1
SEARCH_CERTIFIED = 0
SEARCH_REFERENCE = 1
BUILD_AUTO = 0
BUILD_HOST = 1
XPORT_AUTO = 0
XPORT_RCCL = 1
XPORT_HOST = 2
XPORT_CALLBACK = 3
# icp_hip.h error codes (IcpError.code)
OK, EINVAL, ENOMEM, EDEVICE, ERCCL, ENOTREADY, EEXCHANGE = 0, -1, -2, -3, -4, -5, -6
COPY_H2D, COPY_D2H, COPY_D2D = 0, 1, 2  # icp_hip_dev_copy directions
DBG_SLOTS = 40
METRIC_POINT, METRIC_PLANE, METRIC_GICP = 0, 1, 2  # icp_engine.h ICP_METRIC_*
REJECT_SIGMA, REJECT_TRIM, REJECT_MAX_DIST = 0, 1, 2  # icp_engine.h ICP_REJECT_*
RUN_OPTIONS_VERSION = 1  # icp_engine.h ICP_RUN_OPTIONS_VERSION
KNN_MAX = 32
VOXEL_CENTROID, VOXEL_FIRST = 0, 1  # icp_hip.h ICP_VOXEL_*
OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1  # icp_hip.h ICP_OUTLIER_*
# icp_hip.h ICP_DBG_* slot names
DBG_NAMES = {0: "waves", 1: "overflow_waves", 2: "not_joined", 3: "not_covered", 4: "scanned_points",
             8: "fp64_scan_waves", 9: "staged_points", 10: "scan_pairs", 11: "scan_rounds",
             12: "cache_hits", 13: "cache_stores",
             5: "walk_batches", 6: "no_guess", 7: "candidates", 14: "ball_overflow", 15: "ball_points",
             21: "start_nodes", 20: "winner_prev_waves", 22: "prewalk_retries", 23: "prewalk_kept_old",
             18: "prev_cert_waves", 19: "prev_cert_lanes", 16: "halves", 17: "reused_entries",
             24: "walk_moved", 25: "walk_loose", 26: "group_points", 27: "bb_queries", 28: "bb_steps",
             29: "lane_handed", 30: "fz_recompute", 31: "fz_band", 32: "wide_waves", 33: "wide_segments",
             34: "wide_stack", 35: "wide_undecided", 36: "wide_points", 37: "bb_overflow", 38: "lane_exact",
             39: "prewalk_stores"}

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I32 = C.POINTER(C.c_int32)


class IcpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"icp error {code}: {msg}")
        self.code = code


class IterStats(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("mean", C.c_double), ("std", C.c_double), ("threshold", C.c_double),
        ("valid", C.c_int64), ("rmse", C.c_double), ("sum_d2", C.c_double), ("min_d", C.c_double),
        ("max_d", C.c_double), ("n_bad", C.c_int64), ("centroid_src", C.c_double * 3),
        ("centroid_tgt", C.c_double * 3), ("H", C.c_double * 9), ("n_fallback", C.c_int64),
        ("n_lane_search", C.c_int64), ("n_ball_search", C.c_int64),
    ]

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if not isinstance(v, (int, float)) else v
        return out


class HipConfig(C.Structure):
    """icp_hip_config (include/icp_hip.h): explicit search options of a context."""
    _fields_ = [
        ("config_version", C.c_uint32), ("search", C.c_int32), ("scan32", C.c_int32), ("cell_starts", C.c_int32),
        ("octree_builder", C.c_int32), ("join_factor", C.c_double), ("debug_counters", C.c_int32),
        ("xcd_blocks", C.c_int32), ("scan_groups", C.c_int32), ("candidate_cache", C.c_int32),
        ("candidate_margin", C.c_int32), ("certify_prev", C.c_int32), ("query_order", C.c_int32),
        ("overflow_halves", C.c_int32), ("device_loop", C.c_int32), ("timing_stride", C.c_int32),
        ("candidate_loose", C.c_int32), ("candidate_lead", C.c_int32), ("fused_cull", C.c_int32),
        ("peer_timeout_ms", C.c_int32), ("no_warmup", C.c_int32), ("ball_mode", C.c_int32), ("wide_pass", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


class Params(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32), ("tolerance", C.c_double), ("sigma_multiplier", C.c_double),
        ("octree_max_points", C.c_int32), ("octree_max_depth", C.c_int32), ("rules", C.c_int32),
        ("flags", C.c_int32),
    ]


class IterationRecord(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32), ("rmse", C.c_double), ("valid_points", C.c_int32),
        ("outlier_points", C.c_int32), ("transform", C.c_double * 16),
        ("rotation_angle_deg", C.c_double), ("translation_distance", C.c_double),
        ("has_transform", C.c_int32), ("mean", C.c_double), ("std", C.c_double),
        ("threshold", C.c_double), ("increment", C.c_double * 16),
    ]


class Result(C.Structure):
    _fields_ = [
        ("success", C.c_int32), ("status", C.c_int32), ("total_iterations", C.c_int32),
        ("final_rmse", C.c_double), ("final_R", C.c_double * 9), ("final_t", C.c_double * 3),
        ("n_history", C.c_int32), ("message", C.c_char * 160),
    ]


ITER_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(IterationRecord))
PROGRESS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_double)
LOG_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)


class Hooks(C.Structure):
    _fields_ = [
        ("user", C.c_void_p), ("on_iteration", ITER_CB), ("on_progress", PROGRESS_CB),
        ("on_log", LOG_CB), ("stop_flag", C.POINTER(C.c_int32)),
    ]


class OctreeInfo(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64), ("n_leaves", C.c_int64), ("n_points", C.c_int64),
        ("max_depth", C.c_int32), ("max_inner_depth", C.c_int32), ("pos_of_orig0", C.c_int32),
    ]


class LasHeader(C.Structure):
    _fields_ = [
        ("offset_to_points", C.c_uint32), ("num_points", C.c_uint32), ("record_length", C.c_uint16),
        ("scale", C.c_double * 3), ("offset", C.c_double * 3), ("max", C.c_double * 3), ("min", C.c_double * 3),
    ]


class SynthSpec(C.Structure):
    _fields_ = [
        ("sigma", C.c_double * 3), ("yaw_deg", C.c_double), ("pitch_deg", C.c_double),
        ("roll_deg", C.c_double), ("t", C.c_double * 3), ("noise_sigma", C.c_double),
        ("outlier_fraction", C.c_double), ("seed_target", C.c_uint64), ("seed_source", C.c_uint64),
    ]


class SceneSpec(C.Structure):
    _fields_ = [
        ("site_radius", C.c_double), ("scanner_height", C.c_double), ("n_walls", C.c_int32),
        ("wall_height", C.c_double), ("terrain_amp", C.c_double), ("elev_min_deg", C.c_double),
        ("elev_max_deg", C.c_double), ("range_noise", C.c_double), ("quantum", C.c_double),
        ("yaw_deg", C.c_double), ("pitch_deg", C.c_double), ("roll_deg", C.c_double), ("t", C.c_double * 3),
        ("outlier_fraction", C.c_double), ("seed_target", C.c_uint64), ("seed_source", C.c_uint64),
    ]


class PlaneSums(C.Structure):
    """icp_plane_sums (include/icp_hip.h): the point-to-plane normal equations of an iterate."""
    _fields_ = [
        ("A", C.c_double * 36), ("g", C.c_double * 6), ("sum_r2", C.c_double), ("n", C.c_int64),
        ("n_skipped", C.c_int64), ("origin", C.c_double * 3),
    ]


class GicpSums(C.Structure):
    """icp_gicp_sums (include/icp_hip.h): the generalized-ICP normal equations of an iterate."""
    _fields_ = [
        ("A", C.c_double * 36), ("g", C.c_double * 6), ("sum_r2", C.c_double), ("n", C.c_int64),
        ("n_iso_src", C.c_int64), ("n_iso_tgt", C.c_int64), ("origin", C.c_double * 3), ("epsilon", C.c_double),
    ]


class SelectResult(C.Structure):
    """icp_select_result (include/icp_hip.h): a rank select over the last iterate's residuals."""
    _fields_ = [("value", C.c_double), ("rank", C.c_int64), ("n_finite", C.c_int64), ("n_less", C.c_int64),
                ("n_equal", C.c_int64)]


class PairSums(C.Structure):
    """icp_pair_sums (include/icp_hip.h): the valid-pair statistics at a caller's threshold."""
    _fields_ = [("threshold", C.c_double), ("n_finite", C.c_int64), ("valid", C.c_int64), ("sum_d2", C.c_double),
                ("rmse", C.c_double), ("centroid_src", C.c_double * 3), ("centroid_tgt", C.c_double * 3),
                ("H", C.c_double * 9)]


class RunOptions(C.Structure):
    """icp_run_options (include/icp_engine.h): the options of icp_engine_run_options."""
    _fields_ = [("version", C.c_uint32), ("metric", C.c_int32), ("reject", C.c_int32), ("reject_param", C.c_double)]


class OutlierStats(C.Structure):
    """icp_outlier_stats (include/icp_hip.h): what an outlier call reports beside its arrays."""
    _fields_ = [("n", C.c_int64), ("kept", C.c_int64), ("mean", C.c_double), ("std", C.c_double),
                ("threshold", C.c_double)]


_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double))

# (name, restype, argtypes) for every exported symbol; also the list the ABI test checks
SIGNATURES = {
    # icp_hip.h
    "icp_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "icp_hip_config_default": (None, [C.POINTER(HipConfig)]),
    "icp_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "icp_hip_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(HipConfig)]),
    "icp_hip_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, _I32, C.POINTER(HipConfig), C.c_int]),
    "icp_hip_ctx_devices": (C.c_int, [_P, _I32, _I32, C.c_int32, _I32]),
    "icp_hip_debug_counters": (C.c_int, [_P, _P]),
    "icp_hip_destroy": (None, [_P]),
    "icp_hip_get_unique_id": (C.c_int, [C.c_char_p]),
    "icp_hip_comm_init": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p]),
    "icp_hip_comm_init_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_void_p, _P]),
    "icp_hip_set_target": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "icp_hip_set_source": (C.c_int, [_P, _P, C.c_int64]),
    "icp_hip_iterate": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.POINTER(IterStats)]),
    "icp_hip_apply": (C.c_int, [_P, _P]),
    "icp_hip_get_source": (C.c_int, [_P, _P]),
    "icp_hip_get_correspondences": (C.c_int, [_P, _P, _P]),
    "icp_hip_nn": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "icp_hip_dev_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_void_p)]),
    "icp_hip_dev_free": (C.c_int, [_P, _P]),
    "icp_hip_dev_copy": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    "icp_hip_set_target_device": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "icp_hip_set_source_device": (C.c_int, [_P, _P, C.c_int64]),
    "icp_hip_get_source_device": (C.c_int, [_P, _P]),
    "icp_hip_get_correspondences_device": (C.c_int, [_P, _P, _P]),
    "icp_hip_nn_device": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "icp_hip_knn": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P]),
    "icp_hip_knn_device": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P]),
    "icp_hip_estimate_target_normals": (C.c_int, [_P, C.c_int, _P]),
    "icp_hip_set_target_normals": (C.c_int, [_P, _P]),
    "icp_hip_set_target_normals_device": (C.c_int, [_P, _P]),
    "icp_hip_get_target_normals": (C.c_int, [_P, _P]),
    "icp_hip_get_target_normals_device": (C.c_int, [_P, _P]),
    "icp_hip_plane_sums": (C.c_int, [_P, _P, C.POINTER(PlaneSums)]),
    "icp_plane_solve": (None, [C.POINTER(PlaneSums), _P, _I32]),
    "icp_hip_residual_select": (C.c_int, [_P, C.c_double, C.c_int64, C.POINTER(SelectResult)]),
    "icp_hip_pair_sums": (C.c_int, [_P, C.c_double, C.POINTER(PairSums)]),
    "icp_hip_plane_sums_at": (C.c_int, [_P, _P, C.c_double, C.POINTER(PlaneSums)]),
    "icp_hip_estimate_source_normals": (C.c_int, [_P, C.c_int, _P]),
    "icp_hip_set_source_normals": (C.c_int, [_P, _P]),
    "icp_hip_set_source_normals_device": (C.c_int, [_P, _P]),
    "icp_hip_get_source_normals": (C.c_int, [_P, _P]),
    "icp_hip_get_source_normals_device": (C.c_int, [_P, _P]),
    "icp_hip_gicp_sums": (C.c_int, [_P, _P, _P, C.c_double, C.POINTER(GicpSums)]),
    "icp_hip_gicp_sums_at": (C.c_int, [_P, _P, _P, C.c_double, C.c_double, C.POINTER(GicpSums)]),
    "icp_gicp_solve": (None, [C.POINTER(GicpSums), _P, _I32]),
    "icp_hip_set_gicp_epsilon": (C.c_int, [_P, C.c_double]),
    "icp_hip_voxel_downsample": (C.c_int, [_P, _P, C.c_int64, C.c_double, _P, C.c_int, C.c_int64, _P, _P, _P,
                                           C.POINTER(C.c_int64), _P]),
    "icp_hip_voxel_downsample_device": (C.c_int, [_P, _P, C.c_int64, C.c_double, _P, C.c_int, C.c_int64, _P, _P, _P,
                                                  C.POINTER(C.c_int64), _P]),
    "icp_hip_voxel_last_timing": (C.c_int, [_P, _P]),
    "icp_hip_outlier_filter": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int64, _P, _P, _P, _P,
                                         _P]),
    "icp_hip_outlier_filter_device": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int64, _P, _P, _P,
                                                _P, _P]),
    "icp_hip_outlier_last_timing": (C.c_int, [_P, _P]),
    "icp_hip_traversal_counts": (C.c_int, [_P, _D, _D]),
    "icp_hip_target_info": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _I32, _I32]),
    "icp_hip_last_timing": (C.c_int, [_P, _D, _D]),
    "icp_hip_last_cull_path": (C.c_int, [_P, _I32]),
    "icp_hip_timings": (C.c_int, [_P, C.c_int, _P, _P]),
    "icp_hip_exchange_timings": (C.c_int, [_P, C.c_int, _P]),
    "icp_hip_comm_info": (C.c_int, [_P, C.c_int, _I32, _I32, _I32, _I32]),
    "icp_hip_target_build_info": (C.c_int, [_P, _I32, _D]),
    "icp_hip_copy_target": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "icp_hip_target_separation": (C.c_int, [_P, _P]),
    "icp_hip_copy_target_aux": (C.c_int, [_P, _P, _P, C.c_int64, _I32]),
    "icp_hip_copy_query_order": (C.c_int, [_P, _P]),
    "icp_hip_set_prewalk": (C.c_int, [_P, C.c_double]),
    "icp_hip_synchronize": (C.c_int, [_P]),
    "icp_hip_comm_abort": (C.c_int, [_P]),
    "icp_hip_debug_inject_failure": (C.c_int, [_P, C.c_int, C.c_int]),
    "icp_hip_last_error": (C.c_char_p, []),
    # icp_engine.h
    "icp_params_default": (None, [C.POINTER(Params)]),
    "icp_engine_register": (C.c_int, [C.POINTER(Params), _P, C.c_int64, _P, C.c_int64, C.c_int,
                                      C.POINTER(Result), C.POINTER(IterationRecord), C.c_int32,
                                      C.POINTER(Hooks)]),
    "icp_engine_register_devices": (C.c_int, [C.POINTER(Params), _P, C.c_int64, _P, C.c_int64, C.c_int, _I32,
                                              C.POINTER(Result), C.POINTER(IterationRecord), C.c_int32,
                                              C.POINTER(Hooks)]),
    "icp_engine_run": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Result), C.POINTER(IterationRecord),
                                 C.c_int32, C.POINTER(Hooks)]),
    "icp_session_create": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Hooks), C.POINTER(C.c_void_p)]),
    "icp_session_step": (C.c_int, [_P, C.POINTER(IterationRecord), _I32, _I32]),
    "icp_session_step_n": (C.c_int, [_P, C.c_int32, _I32, _I32]),
    "icp_session_step_n_timed": (C.c_int, [_P, C.c_int32, _I32, _I32, _P]),
    "icp_session_finish": (C.c_int, [_P, C.POINTER(Result)]),
    "icp_session_set_metric": (C.c_int, [_P, C.c_int32]),
    "icp_session_last_plane": (C.c_int, [_P, C.POINTER(PlaneSums), _I32]),
    "icp_session_last_gicp": (C.c_int, [_P, C.POINTER(GicpSums), _I32]),
    "icp_engine_run_metric": (C.c_int, [_P, C.POINTER(Params), C.c_int32, C.POINTER(Result),
                                        C.POINTER(IterationRecord), C.c_int32, C.POINTER(Hooks)]),
    "icp_session_set_rejection": (C.c_int, [_P, C.c_int32, C.c_double]),
    "icp_run_options_default": (None, [C.POINTER(RunOptions)]),
    "icp_engine_run_options": (C.c_int, [_P, C.POINTER(Params), C.POINTER(RunOptions), C.POINTER(Result),
                                         C.POINTER(IterationRecord), C.c_int32, C.POINTER(Hooks)]),
    "icp_session_transform": (None, [_P, _P]),
    "icp_session_destroy": (None, [_P]),
    "icp_cli_icp": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_double, _P, _P, _P, C.c_int32,
                              _I32, C.c_int]),
    "icp_cli_icp_devices": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_double, _P, _P, _P, C.c_int32,
                                      _I32, C.c_int, _I32]),
    "icp_jacobi_svd3": (None, [_P, _P, _P, _P]),
    "icp_best_fit_transform": (None, [_P, _P, C.c_int64, _P]),
    "icp_best_fit_from_stats": (None, [C.POINTER(IterStats), _P]),
    "icp_mat4_mul": (None, [_P, _P, _P]),
    # icp_host.h
    "icp_octree_build": (C.c_void_p, [_P, C.c_int64, C.c_int, C.c_int]),
    "icp_octree_free": (None, [_P]),
    "icp_octree_get_info": (None, [_P, C.POINTER(OctreeInfo)]),
    "icp_octree_copy_nodes": (None, [_P, _P, _P, _P, _P]),
    "icp_octree_copy_points": (None, [_P, _P, _P]),
    "icp_moments_from_values": (None, [_P, C.c_int64, _P]),
    "icp_moments_merge": (None, [_P, C.c_int32, _P]),
    "icp_cov_from_pairs": (None, [_P, _P, _P, C.c_int64, C.c_double, _P]),
    "icp_cov_merge": (None, [_P, C.c_int32, _P]),
    "icp_cull_threshold": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]),
    "icp_trim_rank": (C.c_int64, [C.c_double, C.c_int64]),
    "icp_synth_default": (None, [C.POINTER(SynthSpec)]),
    "icp_synth_pair": (C.c_int, [C.POINTER(SynthSpec), C.c_int64, C.c_int64, _P, _P, _P]),
    "icp_source_shard_order": (C.c_int, [_P, C.c_int64, _P]),
    "icp_scene_default": (None, [C.POINTER(SceneSpec)]),
    "icp_synth_scene": (C.c_int, [C.POINTER(SceneSpec), C.c_int64, C.c_int64, _P, _P, _P]),
    "icp_voxel_downsample": (C.c_int64, [_P, C.c_int64, C.c_double, _P, C.c_int, C.c_int64, _P, _P, _P, _P]),
    # icp_las.h
    "icp_las_read_header": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(LasHeader)]),
    "icp_las_read": (C.c_int64, [C.c_char_p, C.c_int, C.c_int64, _P, C.POINTER(LasHeader)]),
    "icp_las_write_core": (C.c_int, [C.c_char_p, _P, C.c_int64]),
    "icp_las_write_core_bounds": (C.c_int, [C.c_char_p, _P, C.c_int64, _P]),
    "icp_las_write_cli": (C.c_int, [C.c_char_p, _P, C.c_int64, _P, _P]),
    "icp_write_transform_report": (C.c_int, [C.c_char_p, _P, _P, _P, C.c_int32]),
    "icp_hip_read_las_device": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int64, C.c_int64, _P, C.POINTER(LasHeader),
                                          C.POINTER(C.c_int64)]),
    "icp_hip_set_target_las": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(LasHeader), C.POINTER(C.c_int64)]),
    "icp_hip_set_source_las": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(LasHeader),
                                         C.POINTER(C.c_int64)]),
    "icp_hip_write_las_device": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "icp_hip_write_source_las": (C.c_int, [_P, C.c_char_p, C.c_int, _P, _P, _P]),
    "icp_hip_last_las_path": (C.c_int, [_P, _I32]),
    "icp_hip_set_las_chunk_bytes": (C.c_int, [_P, C.c_size_t]),
}

_LIB = None


def build(verbose: bool = False) -> None:
    """Compile libicp_hip.so in-tree for gfx950 (hipcc; no GPU needed)."""
    jobs = str(min(16, os.cpu_count() or 4))
    r = subprocess.run(["make", "-j", jobs, "-C", str(PKG_DIR / "csrc")], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libicp_hip.so failed")


def lib() -> C.CDLL:
    """Load libicp_hip.so; raises if it is missing (there is no fallback path)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built: run `make -C iterativeclosestpoint_amd/csrc` "
                          "or __graft_entry__.build() (no CPU fallback exists)")
    L = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        if "ICP_HIP_LIB" in os.environ and not hasattr(L, name):
            continue  # an older build under A/B: it lacks the newer entry points
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _aos(a) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("expected an (n, 3) float64 array")
    return a


def _check(rc: int) -> None:
    if rc != 0:
        raise IcpError(rc, lib().icp_hip_last_error().decode(errors="replace"))


def params_default(**kw) -> Params:
    p = Params()
    lib().icp_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def config(**kw) -> HipConfig:
    """icp_hip_config with the library defaults, then the given fields."""
    c = HipConfig()
    lib().icp_hip_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise KeyError(f"icp_hip_config has no field {k!r}")
        setattr(c, k, v)
    return c


class Context:
    """One GPU context (icp_hip_ctx) — see include/icp_hip.h. `cfg` is an icp_hip_config (or a
    dict of its fields); None = the library defaults."""

    def __init__(self, device: int = 0, cfg=None, devices=None, transport: int = XPORT_AUTO):
        """devices = a list of HIP ordinals: one context over all of them (icp_hip_create_multi)."""
        self._h = C.c_void_p()
        if isinstance(cfg, dict):
            cfg = config(**cfg)
        if devices is not None:
            ids = (C.c_int32 * len(devices))(*devices)
            _check(lib().icp_hip_create_multi(C.byref(self._h), len(devices), ids,
                                              None if cfg is None else C.byref(cfg), transport))
        elif cfg is None:
            _check(lib().icp_hip_create(C.byref(self._h), device))
        else:
            _check(lib().icp_hip_create_ex(C.byref(self._h), device, C.byref(cfg)))
        self.n_src = 0

    def close(self):
        if self._h:
            lib().icp_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def devices(self):
        """(device ids, transport) of this context (ICP_XPORT_*)."""
        n, tr = C.c_int32(), C.c_int32()
        ids = (C.c_int32 * 64)()
        _check(lib().icp_hip_ctx_devices(self._h, C.byref(n), ids, 64, C.byref(tr)))
        return [ids[k] for k in range(n.value)], tr.value

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().icp_hip_get_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        _check(lib().icp_hip_comm_init(self._h, nranks, rank, C.c_char_p(bytes(uid))))

    def comm_init_host(self, nranks: int, rank: int, exchange):
        """Multi-rank with the all-gathers done by `exchange(local) -> (nranks, count) array`
        (rank order) instead of RCCL (icp_hip_comm_init_host): rehearses several ranks on one GPU."""
        def _cb(_user, local, count, gathered):
            try:
                loc = np.ctypeslib.as_array(local, shape=(count,)).copy()
                out = np.ascontiguousarray(exchange(loc), dtype=np.float64).reshape(-1)
                if out.shape[0] != nranks * count:
                    return 1
                C.memmove(gathered, out.ctypes.data, out.nbytes)
                return 0
            except Exception:
                return 1
        new_cb = _EXCHANGE_FN(_cb)
        # the previous callback may still run on the context's exchange thread (abandoned at the
        # deadline) until icp_hip_comm_init_host joins it: its thunk stays alive for the whole
        # call, and for the context's life (retired callbacks are kept until close)
        if getattr(self, "_xcb", None) is not None:
            self._xcb_retired = getattr(self, "_xcb_retired", []) + [self._xcb]
        rc = lib().icp_hip_comm_init_host(self._h, nranks, rank, C.cast(new_cb, C.c_void_p), None)
        self._xcb = new_cb  # kept alive as long as the context
        _check(rc)

    def set_target(self, xyz, max_points=10, max_depth=20, rules=RULES_ENGINE):
        xyz = _aos(xyz)
        _check(lib().icp_hip_set_target(self._h, _ptr(xyz), xyz.shape[0], max_points, max_depth, rules))
        self._n_tgt = xyz.shape[0]

    def set_source(self, xyz):
        xyz = _aos(xyz)
        _check(lib().icp_hip_set_source(self._h, _ptr(xyz), xyz.shape[0]))
        self.n_src = xyz.shape[0]

    def iterate(self, T_apply=None, iteration=0, rules=RULES_ENGINE, sigma=3.0) -> IterStats:
        st = IterStats()
        T = None if T_apply is None else np.ascontiguousarray(T_apply, dtype=np.float64).reshape(16)
        _check(lib().icp_hip_iterate(self._h, _ptr(T), iteration, rules, sigma, C.byref(st)))
        return st

    def apply(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        _check(lib().icp_hip_apply(self._h, _ptr(T)))

    def get_source(self) -> np.ndarray:
        out = np.empty((self.n_src, 3), np.float64)
        _check(lib().icp_hip_get_source(self._h, _ptr(out)))
        return out

    def get_correspondences(self):
        idx = np.empty(self.n_src, np.int32)
        d = np.empty(self.n_src, np.float64)
        _check(lib().icp_hip_get_correspondences(self._h, _ptr(idx), _ptr(d)))
        return idx, d

    def nn(self, q):
        q = _aos(q)
        idx = np.empty(q.shape[0], np.int32)
        d = np.empty(q.shape[0], np.float64)
        _check(lib().icp_hip_nn(self._h, _ptr(q), q.shape[0], _ptr(idx), _ptr(d)))
        return idx, d

    # --- device-resident clouds (icp_hip_*_device): buffers are DeviceBuffer objects or raw
    # device addresses (ints)
    def device_buffer(self, nbytes: int) -> "DeviceBuffer":
        """HBM on this context's device (icp_hip_dev_alloc)."""
        return DeviceBuffer(self, nbytes)

    def to_device(self, a: np.ndarray) -> "DeviceBuffer":
        """A DeviceBuffer holding a copy of the array's bytes."""
        a = np.ascontiguousarray(a)
        buf = DeviceBuffer(self, a.nbytes)
        buf.upload(a)
        return buf

    def set_target_device(self, d_xyz, n: int, max_points=10, max_depth=20, rules=RULES_ENGINE):
        _check(lib().icp_hip_set_target_device(self._h, _dptr(d_xyz), n, max_points, max_depth, rules))
        self._n_tgt = n

    def set_source_device(self, d_xyz, n: int):
        _check(lib().icp_hip_set_source_device(self._h, _dptr(d_xyz), n))
        self.n_src = n

    def get_source_device(self, d_xyz_out):
        _check(lib().icp_hip_get_source_device(self._h, _dptr(d_xyz_out)))

    def get_correspondences_device(self, d_idx_out=None, d_dist_out=None):
        _check(lib().icp_hip_get_correspondences_device(self._h, _dptr(d_idx_out), _dptr(d_dist_out)))

    def nn_device(self, d_q, n: int, d_idx_out=None, d_dist_out=None):
        _check(lib().icp_hip_nn_device(self._h, _dptr(d_q), n, _dptr(d_idx_out), _dptr(d_dist_out)))

    # --- k nearest neighbours, target normals, the point-to-plane sums (include/icp_hip.h)
    def knn(self, q, k: int):
        """The k nearest target points of each query under (fl(d2), original index), ascending:
        (indices (n, k) int32, fl(d2) (n, k) float64)."""
        q = _aos(q)
        idx = np.empty((q.shape[0], max(k, 0)), np.int32)
        d2 = np.empty((q.shape[0], max(k, 0)), np.float64)
        _check(lib().icp_hip_knn(self._h, _ptr(q), q.shape[0], k, _ptr(idx), _ptr(d2)))
        return idx, d2

    def knn_device(self, d_q, n: int, k: int, d_idx_out=None, d_d2_out=None):
        _check(lib().icp_hip_knn_device(self._h, _dptr(d_q), n, k, _dptr(d_idx_out), _dptr(d_d2_out)))

    def estimate_target_normals(self, k: int = 16, viewpoint=None):
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        _check(lib().icp_hip_estimate_target_normals(self._h, k, _ptr(v)))

    def set_target_normals(self, n_xyz):
        """Normals in the caller's target order: a DeviceBuffer / device address, or an (n, 3) array."""
        if isinstance(n_xyz, (DeviceBuffer, int)):
            _check(lib().icp_hip_set_target_normals_device(self._h, _dptr(n_xyz)))
            return
        n_xyz = _aos(n_xyz)
        if n_xyz.shape[0] != self._n_tgt:
            raise ValueError("one normal per target point")
        _check(lib().icp_hip_set_target_normals(self._h, _ptr(n_xyz)))

    def get_target_normals(self, d_out=None):
        """The target's normals, caller's order: an (n, 3) array, or written to the device buffer d_out."""
        if d_out is not None:
            _check(lib().icp_hip_get_target_normals_device(self._h, _dptr(d_out)))
            return d_out
        out = np.empty((self._n_tgt, 3), np.float64)
        _check(lib().icp_hip_get_target_normals(self._h, _ptr(out)))
        return out

    def plane_sums(self, origin=(0.0, 0.0, 0.0)) -> PlaneSums:
        """The point-to-plane sums of the last iterate's valid pairs about `origin`."""
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        out = PlaneSums()
        _check(lib().icp_hip_plane_sums(self._h, _ptr(o), C.byref(out)))
        return out

    # --- the rejectors (include/icp_hip.h): rank select, pair sums and plane sums at a threshold
    def residual_select(self, fraction: float = 1.0, rank: int = 0) -> SelectResult:
        """The rank-th smallest finite residual of the last iterate (rank 0: trim_rank(fraction,
        n_finite)). An IcpError of a rank past n_finite carries n_finite in its attribute n_finite."""
        out = SelectResult()
        rc = lib().icp_hip_residual_select(self._h, fraction, rank, C.byref(out))
        if rc != 0:
            e = IcpError(rc, lib().icp_hip_last_error().decode(errors="replace"))
            e.n_finite = out.n_finite
            raise e
        return out

    def pair_sums(self, threshold: float) -> PairSums:
        """The valid-pair statistics of the last iterate over the pairs with a finite d <= threshold."""
        out = PairSums()
        _check(lib().icp_hip_pair_sums(self._h, threshold, C.byref(out)))
        return out

    def plane_sums_at(self, origin, threshold: float) -> PlaneSums:
        """plane_sums over the pairs with a finite d <= threshold."""
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        out = PlaneSums()
        _check(lib().icp_hip_plane_sums_at(self._h, _ptr(o), threshold, C.byref(out)))
        return out

    # --- generalized ICP (include/icp_hip.h): source normals and the plane-to-plane sums
    def estimate_source_normals(self, k: int = 16, viewpoint=None):
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        _check(lib().icp_hip_estimate_source_normals(self._h, k, _ptr(v)))

    def set_source_normals(self, n_xyz):
        """Normals in the caller's source order: a DeviceBuffer / device address, or an (n, 3) array."""
        if isinstance(n_xyz, (DeviceBuffer, int)):
            _check(lib().icp_hip_set_source_normals_device(self._h, _dptr(n_xyz)))
            return
        n_xyz = _aos(n_xyz)
        if n_xyz.shape[0] != self.n_src:
            raise ValueError("one normal per source point")
        _check(lib().icp_hip_set_source_normals(self._h, _ptr(n_xyz)))

    def get_source_normals(self, d_out=None):
        """The source's normals, caller's order: an (n, 3) array, or written to the device buffer d_out."""
        if d_out is not None:
            _check(lib().icp_hip_get_source_normals_device(self._h, _dptr(d_out)))
            return d_out
        out = np.empty((self.n_src, 3), np.float64)
        _check(lib().icp_hip_get_source_normals(self._h, _ptr(out)))
        return out

    def gicp_sums(self, origin=(0.0, 0.0, 0.0), R_src=None, epsilon: float = 1e-3) -> GicpSums:
        """The generalized-ICP sums of the last iterate's valid pairs about `origin`; R_src (3, 3):
        the rotation of the resident source since its normals were made (default: none)."""
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        R = np.ascontiguousarray(np.eye(3) if R_src is None else R_src, np.float64).reshape(9)
        out = GicpSums()
        _check(lib().icp_hip_gicp_sums(self._h, _ptr(o), _ptr(R), epsilon, C.byref(out)))
        return out

    def gicp_sums_at(self, origin, R_src, epsilon: float, threshold: float) -> GicpSums:
        """gicp_sums over the pairs with a finite d <= threshold."""
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        R = np.ascontiguousarray(np.eye(3) if R_src is None else R_src, np.float64).reshape(9)
        out = GicpSums()
        _check(lib().icp_hip_gicp_sums_at(self._h, _ptr(o), _ptr(R), epsilon, threshold, C.byref(out)))
        return out

    def set_gicp_epsilon(self, epsilon: float):
        _check(lib().icp_hip_set_gicp_epsilon(self._h, epsilon))

    # --- voxel-grid down-sampling (include/icp_hip.h; the host's: voxel_downsample below)
    def voxel_downsample(self, xyz, voxel, origin=None, mode=VOXEL_CENTROID, cap=None, count_only=False):
        """The voxels of an (n, 3) cloud: (xyz (m, 3), first (m,), count (m,), origin (3,)), or with
        count_only (m, origin). cap: the outputs' capacity (default n). An IcpError of a capacity
        too small carries the number of voxels in its attribute m."""
        xyz = _aos(xyz)
        o_in, o_out = _origin3(origin), np.empty(3)
        m = C.c_int64(0)
        n = xyz.shape[0]
        cap = n if cap is None else int(cap)
        if count_only:
            _check_m(lib().icp_hip_voxel_downsample(self._h, _ptr(xyz), n, voxel, _ptr(o_in), mode, 0, None, None, None,
                                                    C.byref(m), _ptr(o_out)), m)
            return m.value, o_out
        p, f, k = _kept(cap, np.int32, np.int32)
        _check_m(lib().icp_hip_voxel_downsample(self._h, _ptr(xyz), n, voxel, _ptr(o_in), mode, cap, _ptr(p), _ptr(f),
                                                _ptr(k), C.byref(m), _ptr(o_out)), m)
        return *(a[: m.value].copy() for a in (p, f, k)), o_out

    def voxel_downsample_device(self, d_xyz, n: int, voxel, origin=None, mode=VOXEL_CENTROID, cap: int = 0,
                                d_xyz_out=None, d_first_out=None, d_count_out=None):
        """icp_hip_voxel_downsample_device: the cloud and the outputs (cap entries each; any may be
        None, all None counts only) in device buffers. Returns (m, origin (3,))."""
        o_in, o_out = _origin3(origin), np.empty(3)
        m = C.c_int64(0)
        _check_m(lib().icp_hip_voxel_downsample_device(self._h, _dptr(d_xyz), n, voxel, _ptr(o_in), mode, cap,
                                                       _dptr(d_xyz_out), _dptr(d_first_out), _dptr(d_count_out),
                                                       C.byref(m), _ptr(o_out)), m)
        return m.value, o_out

    def voxel_last_timing(self) -> np.ndarray:
        """Device ms of the last voxel call's phases: bounds, keys, sort, runs, reduce."""
        ms = np.zeros(5)
        _check(lib().icp_hip_voxel_last_timing(self._h, _ptr(ms)))
        return ms

    # --- outlier removal (include/icp_hip.h)
    def outlier_filter(self, xyz, mode, k, param, cap=None):
        """The points of an (n, 3) cloud that the statistical (k, std_ratio) or the radius (minimum
        neighbours, radius) filter keeps: (xyz (m, 3), index (m,), score (n,), stats). cap: the
        kept outputs' capacity (default n). An IcpError of a capacity too small carries the number
        kept in its attribute m."""
        xyz = _aos(xyz)
        n = xyz.shape[0]
        cap = n if cap is None else int(cap)
        m, st = C.c_int64(0), OutlierStats()
        (p, ix), sc = _kept(cap, np.int32), np.empty(max(n, 1))
        _check_m(lib().icp_hip_outlier_filter(self._h, _ptr(xyz), n, mode, k, param, cap, _ptr(p), _ptr(ix), _ptr(sc),
                                              C.byref(m), C.byref(st)), m)
        return p[: m.value].copy(), ix[: m.value].copy(), sc[:n], st

    def outlier_filter_device(self, d_xyz, n: int, mode, k, param, cap: int = 0, d_xyz_out=None, d_index_out=None,
                              d_score_out=None):
        """icp_hip_outlier_filter_device: the cloud and the outputs (cap kept entries, n scores; any
        may be None, all None counts only) in device buffers. Returns (m, stats)."""
        m, st = C.c_int64(0), OutlierStats()
        _check_m(lib().icp_hip_outlier_filter_device(self._h, _dptr(d_xyz), n, mode, k, param, cap, _dptr(d_xyz_out),
                                                     _dptr(d_index_out), _dptr(d_score_out), C.byref(m), C.byref(st)), m)
        return m.value, st

    def outlier_last_timing(self) -> np.ndarray:
        """Device ms of the last outlier call's phases: octree build, scores, statistics, compaction."""
        ms = np.zeros(4)
        _check(lib().icp_hip_outlier_last_timing(self._h, _ptr(ms)))
        return ms

    # --- LAS files to and from device-resident clouds (include/icp_las.h)
    def read_las_device(self, path, rules=1, max_points=0, stride=1):
        """Decode a LAS file into a new DeviceBuffer. Returns (buffer, n points, header)."""
        hdr, n = LasHeader(), C.c_int64()
        bpath = str(path).encode()
        _check(lib().icp_hip_read_las_device(self._h, bpath, rules, max_points, stride, None, C.byref(hdr), C.byref(n)))
        buf = DeviceBuffer(self, 24 * max(1, n.value))
        try:
            _check(lib().icp_hip_read_las_device(self._h, bpath, rules, max_points, stride, _dptr(buf), C.byref(hdr),
                                                 C.byref(n)))
        except Exception:
            buf.free()
            raise
        return buf, n.value, hdr

    def set_target_las(self, path, las_rules=1, max_points=0, stride=1, max_tree_points=10, max_depth=20,
                       rules=RULES_ENGINE):
        hdr, n = LasHeader(), C.c_int64()
        _check(lib().icp_hip_set_target_las(self._h, str(path).encode(), las_rules, max_points, stride, max_tree_points,
                                            max_depth, rules, C.byref(hdr), C.byref(n)))
        self._n_tgt = n.value
        return n.value, hdr

    def set_source_las(self, path, las_rules=1, max_points=0, stride=1):
        hdr, n = LasHeader(), C.c_int64()
        _check(lib().icp_hip_set_source_las(self._h, str(path).encode(), las_rules, max_points, stride, C.byref(hdr),
                                            C.byref(n)))
        self.n_src = n.value
        return n.value, hdr

    @staticmethod
    def _las_vec(v):
        return None if v is None else np.ascontiguousarray(v, np.float64)

    def write_las_device(self, path, d_xyz, n, flavour=1, scale=None, offset=None, bounds=None):
        sc, of, bd = self._las_vec(scale), self._las_vec(offset), self._las_vec(bounds)
        _check(lib().icp_hip_write_las_device(self._h, str(path).encode(), _dptr(d_xyz), n, flavour, _ptr(sc), _ptr(of),
                                              _ptr(bd)))

    def write_source_las(self, path, flavour=1, scale=None, offset=None, bounds=None):
        sc, of, bd = self._las_vec(scale), self._las_vec(offset), self._las_vec(bounds)
        _check(lib().icp_hip_write_source_las(self._h, str(path).encode(), flavour, _ptr(sc), _ptr(of), _ptr(bd)))

    def last_las_path(self) -> int:
        """1: the last LAS call went through the decode / encode kernels; 0: the host reader / writer."""
        f = C.c_int32()
        _check(lib().icp_hip_last_las_path(self._h, C.byref(f)))
        return f.value

    def set_las_chunk_bytes(self, nbytes: int):
        _check(lib().icp_hip_set_las_chunk_bytes(self._h, nbytes))

    def traversal_counts(self):
        a, b = C.c_double(), C.c_double()
        _check(lib().icp_hip_traversal_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def target_info(self):
        nn_, nl = C.c_int64(), C.c_int64()
        md, lv = C.c_int32(), C.c_int32()
        _check(lib().icp_hip_target_info(self._h, C.byref(nn_), C.byref(nl), C.byref(md), C.byref(lv)))
        return {"n_nodes": nn_.value, "n_leaves": nl.value, "max_depth": md.value, "stack_levels": lv.value}

    def target_build_info(self):
        """(built on the device?, set_target milliseconds on the context stream)."""
        od, ms = C.c_int32(), C.c_double()
        _check(lib().icp_hip_target_build_info(self._h, C.byref(od), C.byref(ms)))
        return bool(od.value), ms.value

    def copy_target(self) -> dict:
        """The resident octree, in the layout of octree_build() (host builder)."""
        info = self.target_info()
        nn_ = info["n_nodes"]
        npts = self._n_tgt
        box = np.empty((nn_, 6))
        first = np.empty(nn_, np.int32)
        meta = np.empty(nn_, np.uint32)
        depth = np.empty(nn_, np.int32)
        pts = np.empty((npts, 3))
        orig = np.empty(npts, np.int32)
        _check(lib().icp_hip_copy_target(self._h, _ptr(box), _ptr(first), _ptr(meta), _ptr(depth), _ptr(pts),
                                         _ptr(orig)))
        return {"box": box, "first": first, "meta": meta, "depth": depth, "pts": pts, "orig": orig,
                "n_leaves": info["n_leaves"], "max_depth": info["max_depth"]}

    def target_separation(self) -> np.ndarray:
        """Per target point (caller's order): lower bound of its distance to every other point."""
        out = np.empty(self._n_tgt, np.float32)
        _check(lib().icp_hip_target_separation(self._h, _ptr(out)))
        return out

    def copy_target_aux(self) -> dict:
        """The searches' derived target structures (icp_hip_copy_target_aux): "tbox" (n_nodes, 6)
        float32, lo then hi; "cell_lmax" (-1: no tables); "cells", the tables of levels
        0..cell_lmax back to back (level l at offset (8^l - 1) / 7), empty without tables."""
        lmax = C.c_int32()
        _check(lib().icp_hip_copy_target_aux(self._h, None, None, 0, C.byref(lmax)))
        tbox = np.empty((self.target_info()["n_nodes"], 6), np.float32)
        cells = np.empty((8 ** (lmax.value + 1) - 1) // 7 if lmax.value >= 0 else 0, np.int32)
        _check(lib().icp_hip_copy_target_aux(self._h, _ptr(tbox), _ptr(cells), cells.shape[0], C.byref(lmax)))
        return {"tbox": tbox, "cells": cells, "cell_lmax": lmax.value}

    def query_order(self) -> np.ndarray:
        """The installed query order (icp_hip_copy_query_order): slot k holds caller index out[k]."""
        out = np.empty(max(1, self.n_src), np.int32)
        _check(lib().icp_hip_copy_query_order(self._h, _ptr(out)))
        return out[: self.n_src]

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        _check(lib().icp_hip_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_cull_path(self) -> int:
        """1: the last iterate's covariance sums came from the wave search's records + the band
        pairs; 0: a full cull pass (icp_hip_last_cull_path)."""
        f = C.c_int32()
        _check(lib().icp_hip_last_cull_path(self._h, C.byref(f)))
        return f.value

    def timings(self, k: int):
        """(search kernel ms, iterate device ms) of each of the last k iterates, oldest first."""
        a, b = np.zeros(k), np.zeros(k)
        _check(lib().icp_hip_timings(self._h, k, _ptr(a), _ptr(b)))
        return a, b

    def exchange_timings(self, k: int):
        """ms of the two record all-gathers of each of the last k iterates (NaN: not timed)."""
        a = np.zeros(k)
        _check(lib().icp_hip_exchange_timings(self._h, k, _ptr(a)))
        return a

    def comm_info(self, member: int = 0) -> dict:
        """The communicator of member `member` as RCCL reports it (icp_hip_comm_info)."""
        n, r, d, t = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().icp_hip_comm_info(self._h, member, C.byref(n), C.byref(r), C.byref(d), C.byref(t)))
        return {"count": n.value, "rank": r.value, "device": d.value, "transport": t.value}

    def set_prewalk(self, look_ahead: float):
        """The candidate cache's prewalk (icp_hip_set_prewalk): look-ahead in iterates, 0 = off."""
        _check(lib().icp_hip_set_prewalk(self._h, float(look_ahead)))

    def synchronize(self):
        _check(lib().icp_hip_synchronize(self._h))

    def comm_abort(self):
        """Abort this rank's RCCL communicator (icp_hip_comm_abort)."""
        _check(lib().icp_hip_comm_abort(self._h))

    def inject_failure(self, member: int = 0, where: int = 1):
        """Testing hook: member's next iterate fails before its first record exchange."""
        _check(lib().icp_hip_debug_inject_failure(self._h, member, where))

    def debug_counters(self) -> dict:
        """The wave search's diagnostic counters of the last iterate (needs debug_counters=1)."""
        out = np.zeros(DBG_SLOTS, np.uint64)
        _check(lib().icp_hip_debug_counters(self._h, _ptr(out)))
        return {name: int(out[k]) for k, name in DBG_NAMES.items()}

    def session(self, params: Params, metric: int | None = None, reject=None) -> "Session":
        """metric None: the session's default (ICP_METRIC_POINT), no icp_session_set_metric call.
        reject = (mode, param): icp_session_set_rejection; None: no such call (ICP_REJECT_SIGMA)."""
        return Session(self, params, metric=metric, reject=reject)

    def run(self, params: Params, history_cap: int = 1024, metric: int = METRIC_POINT, reject=None):
        """reject = (mode, param): the run goes through icp_engine_run_options."""
        res = Result()
        hist = (IterationRecord * max(1, history_cap))()
        if reject is not None:
            opt = run_options(metric=metric, reject=reject[0], reject_param=reject[1])
            rc = lib().icp_engine_run_options(self._h, C.byref(params), C.byref(opt), C.byref(res), hist, history_cap,
                                              None)
        elif metric == METRIC_POINT:
            rc = lib().icp_engine_run(self._h, C.byref(params), C.byref(res), hist, history_cap, None)
        else:
            rc = lib().icp_engine_run_metric(self._h, C.byref(params), metric, C.byref(res), hist, history_cap, None)
        return rc, res, [hist[k] for k in range(res.n_history)]


def run_options(**kw) -> RunOptions:
    """icp_run_options with the library defaults, then the given fields."""
    o = RunOptions()
    lib().icp_run_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def trim_rank(fraction: float, n_finite: int) -> int:
    """icp_trim_rank (host, no GPU): the trimmed rejector's rank."""
    return int(lib().icp_trim_rank(fraction, n_finite))


def _origin3(origin):
    return None if origin is None else np.ascontiguousarray(origin, np.float64).reshape(3)


def _check_m(rc: int, m) -> None:
    """_check, the error carrying the number of entries (voxels, kept points) the call reported (0: none)."""
    if rc != 0:
        e = IcpError(rc, lib().icp_hip_last_error().decode(errors="replace"))
        e.m = m.value
        raise e


def _kept(cap: int, *dtypes):
    """A compacting call's outputs of capacity cap (never empty): the (cap, 3) cloud, then one array per dtype."""
    return (np.empty((max(cap, 1), 3)), *(np.empty(max(cap, 1), t) for t in dtypes))


def voxel_downsample(xyz, voxel, origin=None, mode=VOXEL_CENTROID, cap=None, count_only=False):
    """Voxel-grid down-sampling on the host (icp_voxel_downsample, no GPU): the function of
    Context.voxel_downsample, the same bits. (xyz (m, 3), first (m,), count (m,), origin (3,)), or
    with count_only (m, origin)."""
    xyz = _aos(xyz)
    o_in, o_out = _origin3(origin), np.empty(3)
    n = xyz.shape[0]
    cap = n if cap is None else int(cap)
    if count_only:
        m = lib().icp_voxel_downsample(_ptr(xyz), n, voxel, _ptr(o_in), mode, 0, None, None, None, _ptr(o_out))
        _check(min(m, 0))
        return m, o_out
    p, f, k = _kept(cap, np.int32, np.int32)
    m = lib().icp_voxel_downsample(_ptr(xyz), n, voxel, _ptr(o_in), mode, cap, _ptr(p), _ptr(f), _ptr(k), _ptr(o_out))
    _check(min(m, 0))
    return *(a[:m].copy() for a in (p, f, k)), o_out


def outlier_filter(xyz, mode, k, param, cap=None, device: int = 0):
    """Context.outlier_filter on a context of its own on `device` (the filters run on the GPU only):
    (xyz (m, 3), index (m,), score (n,), stats)."""
    with Context(device) as ctx:
        return ctx.outlier_filter(xyz, mode, k, param, cap)


def _dptr(b):
    """A device address for the C-ABI: a DeviceBuffer, an int, or None."""
    if b is None:
        return None
    return C.c_void_p(b.ptr if isinstance(b, DeviceBuffer) else int(b))


class DeviceBuffer:
    """HBM owned through a context (icp_hip_dev_alloc / _dev_copy / _dev_free): what a caller
    without a HIP runtime of its own hands to the *_device entry points."""

    def __init__(self, ctx: Context, nbytes: int):
        self._ctx = ctx  # keep alive: the buffer is freed through it
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().icp_hip_dev_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise ValueError("upload past the end of the device buffer")
        _check(lib().icp_hip_dev_copy(self._ctx.handle, C.c_void_p(self.ptr + offset), _ptr(a), a.nbytes, COPY_H2D))

    def download(self, dtype=np.uint8, shape=None, offset: int = 0) -> np.ndarray:
        """The buffer's bytes from `offset` as an array of dtype (shape: default all of them, flat)."""
        dt = np.dtype(dtype)
        if shape is None:
            shape = ((self.nbytes - offset) // dt.itemsize,)
        out = np.empty(shape, dt)
        if offset < 0 or offset + out.nbytes > self.nbytes:
            raise ValueError("download past the end of the device buffer")
        _check(lib().icp_hip_dev_copy(self._ctx.handle, _ptr(out), C.c_void_p(self.ptr + offset), out.nbytes, COPY_D2H))
        return out

    def free(self):
        if self.ptr and self._ctx.handle:
            lib().icp_hip_dev_free(self._ctx.handle, C.c_void_p(self.ptr))
        self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Session:
    """Steppable ICP loop on a context (icp_session_*): one step = one reference loop body."""

    def __init__(self, ctx: Context, params: Params, metric: int | None = None, reject=None):
        self._ctx = ctx  # keep alive
        self._h = C.c_void_p()
        _check(lib().icp_session_create(ctx.handle, C.byref(params), None, C.byref(self._h)))
        self.done = False
        if metric is not None:
            self.set_metric(metric)
        if reject is not None:
            self.set_rejection(*reject)

    def set_rejection(self, mode: int, param: float = 0.0):
        """ICP_REJECT_SIGMA / _TRIM (fraction kept) / _MAX_DIST (metres), before the first step
        (icp_session_set_rejection)."""
        _check(lib().icp_session_set_rejection(self._h, mode, param))

    def set_metric(self, metric: int):
        """ICP_METRIC_POINT / _PLANE / _GICP, before the first step (icp_session_set_metric)."""
        _check(lib().icp_session_set_metric(self._h, metric))

    def last_plane(self):
        """(sums, used_plane) of the last step of a plane session (icp_session_last_plane)."""
        out, used = PlaneSums(), C.c_int32(0)
        _check(lib().icp_session_last_plane(self._h, C.byref(out), C.byref(used)))
        return out, used.value

    def last_gicp(self):
        """(sums, used) of the last step of a generalized-ICP session (icp_session_last_gicp)."""
        out, used = GicpSums(), C.c_int32(0)
        _check(lib().icp_session_last_gicp(self._h, C.byref(out), C.byref(used)))
        return out, used.value

    def step(self):
        rec = IterationRecord()
        produced, done = C.c_int32(0), C.c_int32(0)
        rc = lib().icp_session_step(self._h, C.byref(rec), C.byref(produced), C.byref(done))
        self.done = bool(done.value)
        _check(rc)
        return rec if produced.value else None

    def step_n(self, k: int) -> int:
        """Up to k steps in one native call (no records); returns the steps taken."""
        if not hasattr(lib(), "icp_session_step_n"):  # an older build under A/B
            taken = 0
            while taken < k and not self.done:
                self.step()
                taken += 1
            return taken
        n, done = C.c_int32(0), C.c_int32(0)
        rc = lib().icp_session_step_n(self._h, k, C.byref(n), C.byref(done))
        self.done = bool(done.value)
        _check(rc)
        return n.value

    def step_n_timed(self, k: int) -> np.ndarray:
        """Up to k steps in one native call; returns each step's host wall time (ms)."""
        ms = np.zeros(max(1, k))
        n, done = C.c_int32(0), C.c_int32(0)
        rc = lib().icp_session_step_n_timed(self._h, k, C.byref(n), C.byref(done), _ptr(ms))
        self.done = bool(done.value)
        _check(rc)
        return ms[: n.value]

    def transform(self) -> np.ndarray:
        T = np.empty(16)
        lib().icp_session_transform(self._h, _ptr(T))
        return T.reshape(4, 4)

    def finish(self):
        res = Result()
        rc = lib().icp_session_finish(self._h, C.byref(res))
        return rc, res

    def close(self):
        if self._h:
            lib().icp_session_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def engine_register(params: Params, src, tgt, device: int = -1, history_cap: int = 1024, stop_flag=None,
                    on_log=None, on_progress=None, stop_at: int = -1, devices=None, metric: int = METRIC_POINT,
                    reject=None, normals_k: int = 16):
    """ICPEngine::registerPointClouds drop-in. Returns (rc, result, history, src_out).
    stop_at >= 0 raises the stop flag from the progress hook of that iteration (the reference's
    cross-thread ICPEngine::stop(), checked at the next iteration, icpengine.cpp:160).
    metric / reject = (mode, param): the registration's steps on one context through
    icp_engine_run_options (one device, no hooks; the plane and generalized-ICP metrics' normals
    from normals_k neighbours); the source is written back when the run finished, as the engine does."""
    src = _aos(src).copy()
    tgt = _aos(tgt)
    if metric != METRIC_POINT or reject is not None:
        cli = params.rules == RULES_CLI
        with Context(device if devices is None else devices[0]) as ctx:
            ctx.set_target(tgt, 10 if cli else params.octree_max_points, 20 if cli else params.octree_max_depth,
                           params.rules)
            if metric in (METRIC_PLANE, METRIC_GICP):
                ctx.estimate_target_normals(normals_k)
            ctx.set_source(src)
            if metric == METRIC_GICP:
                ctx.estimate_source_normals(normals_k)
            rc, res, hist = ctx.run(params, history_cap, metric=metric,
                                    reject=reject if reject is not None else (REJECT_SIGMA, 0.0))
            if rc == 0:
                src = ctx.get_source()
        return rc, res, hist, src
    res = Result()
    hist = (IterationRecord * max(1, history_cap))()
    hooks = None
    keep = []
    if stop_at >= 0 and stop_flag is None:
        stop_flag = C.c_int32(0)
    if stop_flag is not None or on_log is not None or on_progress is not None:
        hooks = Hooks()
        if stop_flag is not None:
            hooks.stop_flag = C.cast(C.addressof(stop_flag), C.POINTER(C.c_int32))
        if on_log is not None:
            cb = LOG_CB(lambda u, m: on_log(m.decode(errors="replace")))
            keep.append(cb)
            hooks.on_log = cb
        if on_progress is not None or stop_at >= 0:
            def _progress(_u, it, total, rmse):
                if on_progress is not None:
                    on_progress(it, total, rmse)
                if stop_at >= 0 and it == stop_at:
                    stop_flag.value = 1
            pcb = PROGRESS_CB(_progress)
            keep.append(pcb)
            hooks.on_progress = pcb
    devs = [device] if devices is None else list(devices)
    ids = (C.c_int32 * len(devs))(*devs)
    rc = lib().icp_engine_register_devices(C.byref(params), _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0],
                                           len(devs), ids, C.byref(res), hist, history_cap,
                                           C.byref(hooks) if hooks else None)
    return rc, res, [hist[k] for k in range(res.n_history)], src


def cli_icp(src, tgt, max_iterations=20, tolerance=1e-2, device: int = -1, devices=None):
    """ICP() of icp_registration.cpp drop-in. Returns (R, t, transforms, src_out)."""
    src = _aos(src).copy()
    tgt = _aos(tgt)
    R = np.zeros(9)
    t = np.zeros(3)
    cap = max(1, max_iterations)
    tr = np.zeros((cap, 16))
    n = C.c_int32()
    devs = [device] if devices is None else list(devices)
    ids = (C.c_int32 * len(devs))(*devs)
    _check(lib().icp_cli_icp_devices(_ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], max_iterations, tolerance,
                                     _ptr(R), _ptr(t), _ptr(tr), cap, C.byref(n), len(devs), ids))
    return R.reshape(3, 3), t, tr[: n.value].reshape(-1, 4, 4), src


def source_shard_order(xyz: np.ndarray) -> np.ndarray:
    """Permutation whose contiguous ranges are spatially compact (icp_source_shard_order): rank r
    of W takes xyz[order[lo:hi]] for its balanced contiguous range."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    order = np.empty(len(xyz), np.int32)
    rc = lib().icp_source_shard_order(_ptr(xyz), len(xyz), _ptr(order))
    if rc != 0:
        raise IcpError(rc, lib().icp_hip_last_error().decode())
    return order


def synth_pair(n_tgt: int, n_src: int | None = None, **overrides):
    spec = SynthSpec()
    lib().icp_synth_default(C.byref(spec))
    for k, v in overrides.items():
        if k in ("sigma", "t"):
            getattr(spec, k)[:] = list(v)
        else:
            setattr(spec, k, v)
    n_src = n_tgt if n_src is None else n_src
    tgt = np.empty((n_tgt, 3))
    src = np.empty((n_src, 3))
    T = np.empty(16)
    _check(lib().icp_synth_pair(C.byref(spec), n_tgt, n_src, _ptr(tgt), _ptr(src), _ptr(T)))
    return tgt, src, T.reshape(4, 4)


def synth_scene(n_tgt: int, n_src: int | None = None, **overrides):
    """A LiDAR-like scene pair (icp_synth_scene, include/icp_host.h): ground + walls scanned from
    two poses, 1 mm grid. Returns (target, source, T_true)."""
    spec = SceneSpec()
    lib().icp_scene_default(C.byref(spec))
    for k, v in overrides.items():
        if k == "t":
            spec.t[:] = list(v)
        else:
            setattr(spec, k, v)
    n_src = n_tgt if n_src is None else n_src
    tgt = np.empty((n_tgt, 3))
    src = np.empty((n_src, 3))
    T = np.empty(16)
    _check(lib().icp_synth_scene(C.byref(spec), n_tgt, n_src, _ptr(tgt), _ptr(src), _ptr(T)))
    return tgt, src, T.reshape(4, 4)


def octree_build(xyz, max_points=10, max_depth=20) -> dict:
    """Host linear-octree build (the exact arrays the device path uploads)."""
    xyz = _aos(xyz)
    h = lib().icp_octree_build(_ptr(xyz), xyz.shape[0], max_points, max_depth)
    if not h:
        raise IcpError(-1, lib().icp_hip_last_error().decode())
    try:
        info = OctreeInfo()
        lib().icp_octree_get_info(h, C.byref(info))
        nn_ = info.n_nodes
        box = np.empty((nn_, 6))
        first = np.empty(nn_, np.int32)
        meta = np.empty(nn_, np.uint32)
        depth = np.empty(nn_, np.int32)
        lib().icp_octree_copy_nodes(h, _ptr(box), _ptr(first), _ptr(meta), _ptr(depth))
        pts = np.empty((info.n_points, 3))
        orig = np.empty(info.n_points, np.int32)
        lib().icp_octree_copy_points(h, _ptr(pts), _ptr(orig))
    finally:
        lib().icp_octree_free(h)
    return {"box": box, "first": first, "meta": meta, "depth": depth, "pts": pts, "orig": orig,
            "n_leaves": info.n_leaves, "max_depth": info.max_depth, "max_inner_depth": info.max_inner_depth,
            "pos_of_orig0": info.pos_of_orig0}


def jacobi_svd3(H):
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    U, S, V = np.empty(9), np.empty(3), np.empty(9)
    lib().icp_jacobi_svd3(_ptr(H), _ptr(U), _ptr(S), _ptr(V))
    return U.reshape(3, 3), S, V.reshape(3, 3)


def plane_solve(sums: PlaneSums):
    """The point-to-plane step of the sums (icp_plane_solve): (T (4, 4), ok). ok = 0: the solve
    refused and T is returned as the NaN-filled array it was handed."""
    T = np.full(16, np.nan)
    ok = C.c_int32(0)
    lib().icp_plane_solve(C.byref(sums), _ptr(T), C.byref(ok))
    return T.reshape(4, 4), ok.value


def gicp_solve(sums: GicpSums):
    """The generalized-ICP step of the sums (icp_gicp_solve): (T (4, 4), ok), as plane_solve."""
    T = np.full(16, np.nan)
    ok = C.c_int32(0)
    lib().icp_gicp_solve(C.byref(sums), _ptr(T), C.byref(ok))
    return T.reshape(4, 4), ok.value


def best_fit_transform(a, b):
    a, b = _aos(a), _aos(b)
    T = np.empty(16)
    lib().icp_best_fit_transform(_ptr(a), _ptr(b), a.shape[0], _ptr(T))
    return T.reshape(4, 4)


def best_fit_from_stats(st: IterStats):
    T = np.empty(16)
    lib().icp_best_fit_from_stats(C.byref(st), _ptr(T))
    return T.reshape(4, 4)


def moments_from_values(d):
    d = np.ascontiguousarray(d, np.float64)
    out = np.empty(8)
    lib().icp_moments_from_values(_ptr(d), d.shape[0], _ptr(out))
    return out


def moments_merge(parts):
    parts = np.ascontiguousarray(parts, np.float64).reshape(-1, 8)
    out = np.empty(8)
    lib().icp_moments_merge(_ptr(parts), parts.shape[0], _ptr(out))
    return out


def cov_from_pairs(a, b, d, thr):
    a, b = _aos(a), _aos(b)
    d = np.ascontiguousarray(d, np.float64)
    out = np.empty(20)
    lib().icp_cov_from_pairs(_ptr(a), _ptr(b), _ptr(d), d.shape[0], thr, _ptr(out))
    return out


def cov_merge(parts):
    parts = np.ascontiguousarray(parts, np.float64).reshape(-1, 20)
    out = np.empty(20)
    lib().icp_cov_merge(_ptr(parts), parts.shape[0], _ptr(out))
    return out


def cull_threshold(mean, sd, k_sigma, iteration, engine_rules):
    return lib().icp_cull_threshold(mean, sd, k_sigma, iteration, engine_rules)


LAS_CORE = 0
LAS_CLI = 1


def las_read(path, rules=LAS_CLI, max_points=0):
    """Read a LAS 1.2 file (core LASIO::readLAS or CLI readLASFile rules). Returns (xyz, header)."""
    hdr = LasHeader()
    bpath = str(path).encode()
    rc = lib().icp_las_read_header(bpath, rules, C.byref(hdr))
    if rc != 0:
        raise IcpError(rc, f"cannot read LAS header of {path}")
    n = hdr.num_points if max_points <= 0 or rules == LAS_CLI else min(hdr.num_points, max_points)
    xyz = np.empty((max(n, 1), 3))
    got = lib().icp_las_read(bpath, rules, max_points, _ptr(xyz), C.byref(hdr))
    if got < 0:
        raise IcpError(int(got), f"cannot read LAS points of {path}")
    return xyz[:got], hdr


def las_write_core(path, xyz, bounds=None):
    """LASIO::writeLAS. bounds = the caller's PointCloud (minX, maxX, minY, maxY, minZ, maxZ) as they
    stand; None = computeBounds() of xyz."""
    xyz = _aos(xyz)
    if bounds is None:
        rc = lib().icp_las_write_core(str(path).encode(), _ptr(xyz), xyz.shape[0])
    else:
        b = np.ascontiguousarray(bounds, np.float64)
        rc = lib().icp_las_write_core_bounds(str(path).encode(), _ptr(xyz), xyz.shape[0], _ptr(b))
    if rc != 0:
        raise IcpError(rc, f"cannot write {path}")


def las_write_cli(path, xyz, scale=(0.001, 0.001, 0.001), offset=(0.0, 0.0, 0.0)):
    xyz = _aos(xyz)
    sc = np.ascontiguousarray(scale, np.float64)
    of = np.ascontiguousarray(offset, np.float64)
    rc = lib().icp_las_write_cli(str(path).encode(), _ptr(xyz), xyz.shape[0], _ptr(sc), _ptr(of))
    if rc != 0:
        raise IcpError(rc, f"cannot write {path}")


def write_transform_report(path, R, t, transforms=None):
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    if transforms is None or len(transforms) == 0:
        T, n = None, 0
    else:
        T = np.ascontiguousarray(transforms, np.float64).reshape(-1, 16)
        n = T.shape[0]
    rc = lib().icp_write_transform_report(str(path).encode(), _ptr(R), _ptr(t), _ptr(T), n)
    if rc != 0:
        raise IcpError(rc, f"cannot write {path}")
