"""ctypes binding of include/fitslam_frontier.h (libfitslam_frontier.so).

This is the thin Python host layer over the C ABI: it owns no algorithm.  There is no CPU
fallback — if the HIP library cannot be built/loaded or no gfx950 device is present, creating a
`FrontierScorer` raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import _build

FS_OK, FS_E_INVALID, FS_E_NO_DEVICE, FS_E_HIP, FS_E_STATE, FS_E_IO, FS_E_RANGE = 0, -1, -2, -3, -4, -5, -6
STATUS_OK, STATUS_OFF_MAP, STATUS_BLACKLISTED = 0, 1, 2
FS_MAX_ELEV = 16
FS_SEEDS_NEAREST, FS_SEEDS_REFERENCE = 0, 1
SEED_ORDERS = {"nearest": FS_SEEDS_NEAREST, "reference": FS_SEEDS_REFERENCE}
FS_ROADMAP_SEARCH_TREE, FS_ROADMAP_SEARCH_REFERENCE = 0, 1
ROADMAP_SEARCHES = {"tree": FS_ROADMAP_SEARCH_TREE, "reference": FS_ROADMAP_SEARCH_REFERENCE}
FS_GRID_SEARCH_CONVERGED, FS_GRID_SEARCH_REFERENCE = 0, 1
GRID_SEARCHES = {"converged": FS_GRID_SEARCH_CONVERGED, "reference": FS_GRID_SEARCH_REFERENCE}
FS_REFINE_SEARCH_FIELD, FS_REFINE_SEARCH_REFERENCE = 0, 1
REFINE_SEARCHES = {"field": FS_REFINE_SEARCH_FIELD, "reference": FS_REFINE_SEARCH_REFERENCE}
FS_ALLOC_HUNGARIAN, FS_ALLOC_MINPOS = 0, 1
ALLOC_METHODS = {"hungarian": FS_ALLOC_HUNGARIAN, "minpos": FS_ALLOC_MINPOS}
FS_ALLOC_MAX_ROBOTS, FS_ALLOC_MAX_TASKS = 64, 4096

# every symbol include/fitslam_frontier.h declares
EXPORTED_SYMBOLS = [
    "fs_abi_version", "fs_ctx_create", "fs_ctx_destroy", "fs_last_error", "fs_synchronize",
    "fs_enable_kernel_timing", "fs_kernel_time", "fs_set_option", "fs_get_counter",
    "fs_set_ray_params", "fs_ray_fan_shape", "fs_upload_grid", "fs_upload_grid_bricks", "fs_update_grid_region", "fs_frontier_cells", "fs_frontier_clusters", "fs_max_arrival", "fs_set_arrival_limits",
    "fs_score_arrival", "fs_trace_segments",
    "fs_upload_landmarks", "fs_lookup_generate", "fs_lookup_load", "fs_lookup_save", "fs_lookup_set_records",
    "fs_lookup_num_records", "fs_lookup_get_records", "fs_lookup_query", "fs_set_fim_params", "fs_score_fim", "fs_information_frontier_pair",
    "fs_upload_keyframes", "fs_information_for_pose",
    "fs_score_candidates", "fs_score_candidates_dev", "fs_rank_candidates", "fs_rank_candidates_dev", "fs_get_frontier_costs", "fs_selftest_fp64",
    "fs_multi_create", "fs_multi_destroy", "fs_multi_num_devices", "fs_multi_ctx", "fs_multi_last_error", "fs_multi_shard_bounds",
    "fs_multi_set_option", "fs_multi_set_ray_params", "fs_multi_upload_grid", "fs_multi_update_grid_region", "fs_multi_upload_landmarks", "fs_multi_lookup_generate",
    "fs_multi_lookup_load", "fs_multi_set_fim_params", "fs_multi_max_arrival", "fs_multi_score_arrival", "fs_multi_score_candidates",
    "fs_multi_score_fim", "fs_multi_get_frontier_costs", "fs_multi_gather_mode",
    "fs_plan_paths", "fs_navfn_potential", "fs_get_frontier_costs_planned", "fs_plan_paths_information",
    "fs_set_roadmap_params", "fs_roadmap_add_nodes", "fs_roadmap_rebuild", "fs_roadmap_connect", "fs_roadmap_get_graph", "fs_roadmap_plan",
    "fs_get_frontier_costs_roadmap", "fs_roadmap_next_goal", "fs_refine_paths", "fs_refine_field",
    "fs_roadmap_set_keyframes", "fs_roadmap_optimize", "fs_roadmap_get_anchors",
    "fs_search_frontiers", "fs_get_frontier_costs_searched", "fs_set_frontier_seed_order", "fs_set_roadmap_search",
    "fs_roadmap_routes", "fs_set_grid_search", "fs_navfn_wave_potential", "fs_set_refine_search",
    "fs_roadmap_update", "fs_get_frontier_costs_searched_roadmap",
    "fs_allocate_tasks", "fs_allocate_tasks_dev", "fs_fleet_allocate_roadmap",
    "fs_keepout_add_fov", "fs_keepout_add_disc", "fs_keepout_clear", "fs_keepout_get", "fs_mark_lethal_fov", "fs_read_grid_region",
    "fs_multi_keepout_add_fov", "fs_multi_keepout_add_disc", "fs_multi_keepout_clear", "fs_multi_mark_lethal_fov",
    "fs_set_occlusion", "fs_get_occlusion", "fs_line_of_sight", "fs_multi_set_occlusion",
    "fs_landmarks_in_view",
    "fs_upload_world", "fs_sense", "fs_goals_mapped", "fs_grid_census", "fs_drive",
    "fs_upload_world_landmarks", "fs_sense_landmarks", "fs_world_landmarks_get", "fs_staged_cloud_get",
    "fs_drive_slam",
    "fs_inflate", "fs_inflation_costs", "fs_multi_inflate",
    "fs_information_layer", "fs_multi_information_layer",
]
FS_KEEPOUT_MAX_ZONES = 1024
FS_INFLATE_MAX_CELLS = 512
FS_INFO_LAYER_MAX_STRIDE, FS_INFO_LAYER_MAX_YAW = 32, 64
FS_INFO_REDUCE_MIN, FS_INFO_REDUCE_MEAN, FS_INFO_REDUCE_MAX = 0, 1, 2
INFO_REDUCE = {"min": FS_INFO_REDUCE_MIN, "mean": FS_INFO_REDUCE_MEAN, "max": FS_INFO_REDUCE_MAX}
FS_DRIVE_ARRIVED, FS_DRIVE_BLOCKED, FS_DRIVE_COLLIDED, FS_DRIVE_OFF_MAP, FS_DRIVE_MAPPED = 0, 1, 2, 3, 4
FS_DRIVE_UNSAFE = 5
FS_DRIVE_MAX_STATIONS, FS_DRIVE_MAX_ROBOTS = 2048, 4096
KEEPOUT_FOV, KEEPOUT_DISC = 0, 1

RECORD_DTYPE = np.dtype([("arrival", "<i4"), ("argmax", "<i4"), ("yaw", "<f4"), ("info_ref", "<f4"),
                         ("trace", "<f4"), ("logdet", "<f4"), ("n_visible", "<i4"), ("flags", "<u4")])
assert RECORD_DTYPE.itemsize == 32


class KeyframeParamsC(C.Structure):
    _fields_ = [("max_depth", C.c_double), ("hfov", C.c_double), ("max_depth_error", C.c_double),
                ("q_diag", C.c_float), ("radius", C.c_double)]


class PathInfoParamsC(C.Structure):
    _fields_ = [("sample_distance_m", C.c_double), ("lookahead_points", C.c_int32), ("fi_threshold", C.c_double)]


class RouteParamsC(C.Structure):
    _fields_ = [("refine", C.c_int32), ("with_information", C.c_int32), ("fi_threshold", C.c_double)]


class FrontierClusterC(C.Structure):
    _fields_ = [("label", C.c_int32), ("size", C.c_int32), ("centroid_x", C.c_double), ("centroid_y", C.c_double),
                ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32)]


CLUSTER_DTYPE = np.dtype([("label", "<i4"), ("size", "<i4"), ("centroid_x", "<f8"), ("centroid_y", "<f8"),
                          ("min_x", "<i4"), ("min_y", "<i4"), ("max_x", "<i4"), ("max_y", "<i4")])
assert CLUSTER_DTYPE.itemsize == C.sizeof(FrontierClusterC) == 40


# fs_frontier_record: one Frontier record of fs_search_frontiers
FRONTIER_RECORD_DTYPE = np.dtype([("goal_x", "<f8"), ("goal_y", "<f8"), ("size", "<i4"), ("label", "<i4"),
                                  ("goal_cell", "<i4"), ("seed_cell", "<i4")])
assert FRONTIER_RECORD_DTYPE.itemsize == 32


class RayParamsC(C.Structure):
    _fields_ = [("max_camera_depth", C.c_double), ("delta_theta", C.c_double), ("camera_fov", C.c_double),
                ("robot_radius", C.c_double), ("n_rays", C.c_int32), ("n_elev", C.c_int32),
                ("elev", C.c_double * FS_MAX_ELEV),
                ("obst_min", C.c_int32), ("obst_max", C.c_int32), ("trace_min", C.c_int32), ("trace_max", C.c_int32),
                ("factor_max", C.c_double), ("factor_min", C.c_double), ("polygon", C.c_double * 4)]


class FimParamsC(C.Structure):
    _fields_ = [("max_dist", C.c_double), ("max_angle", C.c_double)]


class OcclusionParamsC(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("occ_min", C.c_int32), ("occ_max", C.c_int32), ("end_margin_m", C.c_double)]


class LandmarkSensorC(C.Structure):
    _fields_ = [("max_dist", C.c_double), ("max_angle", C.c_double), ("line_of_sight", C.c_int32), ("min_views", C.c_int32),
                ("occ_min", C.c_int32), ("occ_max", C.c_int32), ("end_margin_m", C.c_double)]


assert C.sizeof(LandmarkSensorC) == 40


class DriveParamsC(C.Structure):
    _fields_ = [("block_min", C.c_int32), ("block_max", C.c_int32), ("stop_when_mapped", C.c_int32)]


assert C.sizeof(DriveParamsC) == 12


class DriveSlamParamsC(C.Structure):
    _fields_ = [("block_min", C.c_int32), ("block_max", C.c_int32), ("stop_when_mapped", C.c_int32), ("gate", C.c_int32),
                ("information_threshold", C.c_double), ("gate_first_station", C.c_int32)]


assert C.sizeof(DriveSlamParamsC) == 32


class InflationParamsC(C.Structure):
    _fields_ = [("inflation_radius", C.c_double), ("inscribed_radius", C.c_double), ("cost_scaling_factor", C.c_double),
                ("inflate_unknown", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(InflationParamsC) == 32


class InfoLayerParamsC(C.Structure):
    _fields_ = [("stride_cells", C.c_int32), ("n_yaw", C.c_int32), ("yaw0", C.c_double), ("pose_z", C.c_double),
                ("reduce", C.c_int32), ("info_lo", C.c_double), ("info_hi", C.c_double), ("max_cost", C.c_int32), ("write", C.c_int32)]


assert C.sizeof(InfoLayerParamsC) == 56


class ViewLandmarkC(C.Structure):
    _fields_ = [("index", C.c_int32), ("p_camera", C.c_float * 3), ("table_value", C.c_float)]


# fs_view_landmark: one entry of fs_landmarks_in_view
VIEW_DTYPE = np.dtype([("index", "<i4"), ("p_camera", "<f4", (3,)), ("table_value", "<f4")])
assert VIEW_DTYPE.itemsize == C.sizeof(ViewLandmarkC) == 20


class FsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fitslam_frontier error {code}: {msg}")
        self.code = code


_lib = None


def load_library(build: bool = True, path: str | None = None):
    """Load (building first if needed) the HIP library.  Raises if it is missing: no CPU fallback.
    `path`: load THAT build of the library instead, next to the process's own and never in its place (an A/B probe holds two
    builds in one process and hands one to FrontierScorer(library=...)); nothing is built for it."""
    global _lib
    other = path is not None
    if not other and _lib is not None:
        return _lib
    if not other:
        path = _build.LIB
        if build and _build.needs_build():
            path = _build.build()
    if not os.path.exists(path):
        raise FsError(FS_E_NO_DEVICE, f"{path} is missing and could not be built; there is no CPU fallback")
    L = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.fs_abi_version.restype = C.c_int
    L.fs_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.fs_ctx_destroy.argtypes = [vp]
    L.fs_ctx_destroy.restype = None
    L.fs_last_error.argtypes = [vp]
    L.fs_last_error.restype = C.c_char_p
    L.fs_synchronize.argtypes = [vp]
    L.fs_enable_kernel_timing.argtypes = [vp, C.c_int]
    L.fs_kernel_time.argtypes = [vp, C.c_int, C.POINTER(dbl), C.POINTER(i64)]
    L.fs_set_option.argtypes = [vp, C.c_char_p, dbl]
    L.fs_get_counter.argtypes = [vp, C.c_int, C.POINTER(i64), C.c_int]
    L.fs_set_ray_params.argtypes = [vp, C.POINTER(RayParamsC)]
    L.fs_ray_fan_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.fs_upload_grid.argtypes = [vp, vp, i32, i32, i32, C.POINTER(dbl * 3), dbl]
    L.fs_upload_grid_bricks.argtypes = [vp, i32, i32, i32, C.POINTER(dbl * 3), dbl, C.c_uint8, i64, vp, vp]
    L.fs_update_grid_region.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64]
    L.fs_multi_update_grid_region.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64]
    L.fs_frontier_cells.argtypes = [vp, i32, vp, C.POINTER(i64)]
    L.fs_frontier_clusters.argtypes = [vp, C.POINTER(dbl * 2), i32, dbl, i32, vp, i32, vp, C.POINTER(i32), C.POINTER(i64)]
    L.fs_max_arrival.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]
    L.fs_set_arrival_limits.argtypes = [vp, dbl, dbl]
    L.fs_score_arrival.argtypes = [vp, i32] + [vp] * 10
    L.fs_trace_segments.argtypes = [vp, i32, vp, vp, dbl, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.fs_upload_landmarks.argtypes = [vp, vp, i32]
    L.fs_lookup_generate.argtypes = [vp, vp]
    L.fs_lookup_load.argtypes = [vp, C.c_char_p]
    L.fs_lookup_save.argtypes = [vp, C.c_char_p]
    L.fs_lookup_set_records.argtypes = [vp, vp, i64]
    L.fs_lookup_num_records.argtypes = [vp, C.POINTER(i64)]
    L.fs_lookup_get_records.argtypes = [vp, vp]
    L.fs_lookup_query.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.fs_set_fim_params.argtypes = [vp, C.POINTER(FimParamsC)]
    L.fs_set_occlusion.argtypes = [vp, C.POINTER(OcclusionParamsC)]
    L.fs_get_occlusion.argtypes = [vp, C.POINTER(OcclusionParamsC)]
    L.fs_line_of_sight.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.fs_score_fim.argtypes = [vp, i32] + [vp] * 7
    L.fs_landmarks_in_view.argtypes = [vp, i32, vp, i64, vp, vp]
    L.fs_upload_world.argtypes = [vp, vp, i32, i32, i32]
    L.fs_sense.argtypes = [vp, i32, vp, vp, C.POINTER(RayParamsC), vp, vp, vp, C.POINTER(i64), C.POINTER(i64), vp]
    L.fs_goals_mapped.argtypes = [vp, i32, vp, vp]
    L.fs_grid_census.argtypes = [vp, vp]
    L.fs_drive.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(RayParamsC), C.POINTER(DriveParamsC), vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), vp]
    L.fs_upload_world_landmarks.argtypes = [vp, vp, i32, vp]
    L.fs_sense_landmarks.argtypes = [vp, i32, vp, C.POINTER(LandmarkSensorC), vp, C.POINTER(i32), C.POINTER(i32)]
    L.fs_drive_slam.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(RayParamsC), C.POINTER(LandmarkSensorC), C.POINTER(DriveSlamParamsC),
                                vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), vp, C.POINTER(i32), C.POINTER(i32)]
    L.fs_world_landmarks_get.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), vp, vp]
    L.fs_staged_cloud_get.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), vp, vp, vp]
    L.fs_information_frontier_pair.argtypes = [vp, i32, vp, vp, vp]
    L.fs_upload_keyframes.argtypes = [vp, i32, vp, vp, vp]
    L.fs_information_for_pose.argtypes = [vp, i32, vp, C.POINTER(KeyframeParamsC), vp, vp, vp]
    L.fs_score_candidates.argtypes = [vp, i32] + [vp] * 5
    L.fs_score_candidates_dev.argtypes = [vp, i32] + [vp] * 5
    L.fs_rank_candidates.argtypes = [vp, i32, vp, vp, vp, vp, dbl, dbl, dbl, dbl, vp, vp, vp, vp]
    L.fs_rank_candidates_dev.argtypes = [vp, i32, vp, vp, vp, vp, dbl, dbl, dbl, dbl, vp, vp, vp, vp, vp]
    L.fs_get_frontier_costs.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, dbl, dbl, dbl, dbl, C.c_int, vp, vp, vp, vp, vp]
    L.fs_selftest_fp64.argtypes = [vp, i32, C.POINTER(i64)]
    L.fs_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.fs_multi_destroy.argtypes = [vp]
    L.fs_multi_destroy.restype = None
    L.fs_multi_num_devices.argtypes = [vp]
    L.fs_multi_ctx.argtypes = [vp, C.c_int]
    L.fs_multi_ctx.restype = vp
    L.fs_multi_last_error.argtypes = [vp]
    L.fs_multi_last_error.restype = C.c_char_p
    L.fs_multi_shard_bounds.argtypes = [i32, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32)]
    L.fs_multi_set_option.argtypes = [vp, C.c_char_p, dbl]
    L.fs_multi_set_ray_params.argtypes = [vp, C.POINTER(RayParamsC)]
    L.fs_multi_upload_grid.argtypes = [vp, vp, i32, i32, i32, C.POINTER(dbl * 3), dbl]
    L.fs_multi_upload_landmarks.argtypes = [vp, vp, i32]
    L.fs_multi_lookup_generate.argtypes = [vp, vp]
    L.fs_multi_lookup_load.argtypes = [vp, C.c_char_p]
    L.fs_multi_set_fim_params.argtypes = [vp, C.POINTER(FimParamsC)]
    L.fs_multi_set_occlusion.argtypes = [vp, C.POINTER(OcclusionParamsC)]
    L.fs_multi_max_arrival.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]
    L.fs_multi_score_arrival.argtypes = [vp, i32] + [vp] * 10
    L.fs_multi_score_candidates.argtypes = [vp, i32] + [vp] * 5
    L.fs_multi_score_fim.argtypes = [vp, i32] + [vp] * 7
    L.fs_multi_get_frontier_costs.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, dbl, dbl, dbl, dbl, C.c_int, vp, vp, vp, vp, vp]
    L.fs_multi_gather_mode.argtypes = [vp]
    L.fs_plan_paths.argtypes = [vp, C.POINTER(dbl * 7), i32, i32, vp, vp, vp, vp, vp, vp]
    L.fs_navfn_potential.argtypes = [vp, C.POINTER(dbl * 7), i32, vp]
    L.fs_plan_paths_information.argtypes = [vp, C.POINTER(dbl * 7), i32, i32, vp, vp, C.POINTER(PathInfoParamsC), vp, vp, vp, vp, vp, vp, vp, vp,
                                            i64, C.POINTER(i64), vp, vp, vp]
    L.fs_get_frontier_costs_planned.argtypes = [vp, C.POINTER(dbl * 7), i32, i32, vp, vp, vp, dbl, dbl, dbl, dbl, C.c_int, vp, vp, vp, vp, vp, vp]
    L.fs_set_roadmap_params.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.fs_roadmap_add_nodes.argtypes = [vp, i32, vp, i32]
    L.fs_roadmap_rebuild.argtypes = [vp]
    L.fs_roadmap_connect.argtypes = [vp, i32, vp]
    L.fs_roadmap_update.argtypes = [vp, i32, vp, C.POINTER(dbl * 2), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.fs_get_frontier_costs_searched_roadmap.argtypes = [vp, C.POINTER(dbl * 7), i32, dbl, i32, i32, i32, i32, vp, dbl, dbl, dbl, dbl, C.c_int,
                                                         i32, vp, C.POINTER(i32), vp, vp, vp, vp, vp, vp]
    L.fs_roadmap_get_graph.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), vp, vp, vp, vp]
    L.fs_roadmap_plan.argtypes = [vp, C.POINTER(dbl * 7), i32, vp, vp, vp, vp, vp, vp]
    L.fs_get_frontier_costs_roadmap.argtypes = [vp, C.POINTER(dbl * 7), i32, vp, vp, vp, dbl, dbl, dbl, dbl, C.c_int, vp, vp, vp, vp, vp, vp]
    L.fs_roadmap_routes.argtypes = [vp, C.POINTER(dbl * 7), i32, vp, vp, C.POINTER(RouteParamsC), vp, vp, vp, vp, vp, i32, C.POINTER(i32),
                                    vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64), vp, vp, C.POINTER(i64), vp, vp, vp, vp]
    L.fs_roadmap_next_goal.argtypes = [vp, C.POINTER(dbl * 7), i32, vp, vp, vp, vp, i32, vp, i32, dbl, vp, dbl,
                                       C.POINTER(i32), C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(dbl), C.POINTER(i64), vp, vp]
    L.fs_roadmap_set_keyframes.argtypes = [vp, i32, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.fs_roadmap_optimize.argtypes = [vp]
    L.fs_roadmap_get_anchors.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), vp, vp]
    L.fs_refine_paths.argtypes = [vp, i32, vp, vp, i32, dbl, dbl, i32, vp, vp, vp, vp, vp, vp]
    L.fs_refine_field.argtypes = [vp, C.POINTER(dbl * 2), i32, dbl, dbl, i32, vp]
    L.fs_search_frontiers.argtypes = [vp, C.POINTER(dbl * 2), i32, dbl, i32, i32, i32, vp, i32, vp, C.POINTER(i32), i64, vp, C.POINTER(i64)]
    L.fs_set_frontier_seed_order.argtypes = [vp, i32]
    L.fs_set_roadmap_search.argtypes = [vp, i32]
    L.fs_set_grid_search.argtypes = [vp, i32]
    L.fs_set_refine_search.argtypes = [vp, i32]
    L.fs_navfn_wave_potential.argtypes = [vp, C.POINTER(dbl * 7), i32, C.POINTER(dbl * 3), vp, C.POINTER(i32)]
    L.fs_get_frontier_costs_searched.argtypes = [vp, C.POINTER(dbl * 7), i32, dbl, i32, i32, i32, i32, vp, dbl, dbl, dbl, dbl, C.c_int,
                                                 i32, vp, C.POINTER(i32), vp, vp, vp, vp, vp, vp]
    L.fs_allocate_tasks.argtypes = [vp, i32, i32, vp, vp, i32, vp, C.POINTER(dbl), vp, vp]
    L.fs_allocate_tasks_dev.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.fs_fleet_allocate_roadmap.argtypes = [vp, i32, vp, i32, vp, vp, vp, dbl, dbl, dbl, dbl, i32, vp, C.POINTER(dbl), vp, vp, vp, vp, vp]
    L.fs_keepout_add_fov.argtypes = [vp, dbl, dbl, dbl, dbl, C.POINTER(i32), C.POINTER(i64)]
    L.fs_keepout_add_disc.argtypes = [vp, dbl, dbl, dbl, C.POINTER(i32), C.POINTER(i64)]
    L.fs_keepout_clear.argtypes = [vp]
    L.fs_keepout_get.argtypes = [vp, C.POINTER(i32), vp, vp, vp]
    L.fs_mark_lethal_fov.argtypes = [vp, C.POINTER(dbl * 7), C.POINTER(dbl * 7), C.POINTER(i32), C.POINTER(i64)]
    L.fs_read_grid_region.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64]
    L.fs_multi_keepout_add_fov.argtypes = [vp, dbl, dbl, dbl, dbl, C.POINTER(i32), C.POINTER(i64)]
    L.fs_multi_keepout_add_disc.argtypes = [vp, dbl, dbl, dbl, C.POINTER(i32), C.POINTER(i64)]
    L.fs_multi_keepout_clear.argtypes = [vp]
    L.fs_multi_mark_lethal_fov.argtypes = [vp, C.POINTER(dbl * 7), C.POINTER(dbl * 7), C.POINTER(i32), C.POINTER(i64)]
    L.fs_inflate.argtypes = [vp, C.POINTER(InflationParamsC), i32, i32, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.fs_inflation_costs.argtypes = [vp, C.POINTER(InflationParamsC), C.POINTER(i32), vp]
    L.fs_multi_inflate.argtypes = [vp, C.POINTER(InflationParamsC), i32, i32, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    for f in (L.fs_information_layer, L.fs_multi_information_layer):
        f.argtypes = [vp, C.POINTER(InfoLayerParamsC), i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    for name in EXPORTED_SYMBOLS:
        f = getattr(L, name)
        if name not in ("fs_ctx_destroy", "fs_last_error", "fs_multi_destroy", "fs_multi_last_error", "fs_multi_ctx"):
            f.restype = C.c_int
    if not other:
        _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _inflation_params_c(inflation_radius, inscribed_radius, cost_scaling_factor, inflate_unknown):
    return InflationParamsC(float(inflation_radius), float(inscribed_radius), float(cost_scaling_factor), 1 if inflate_unknown else 0, 0)


class InformationLayerResult:
    """What fs_information_layer returns: info [nby][nbx] (NaN: unscored block), anchor_cell [nby][nbx] (y * nx + x, or -1),
    info_per_yaw [K][nby][nbx] or None, quat_zw [K][2], pose7 [n_scored * K][7] (scored blocks in block order, headings in
    order — rebuilt on the host from the anchors and quat_zw: the poses that were scored), n_scored, n_changed."""

    def __init__(self, info, anchor_cell, info_per_yaw, quat_zw, pose7, n_scored, n_changed):
        self.info, self.anchor_cell, self.info_per_yaw, self.quat_zw = info, anchor_cell, info_per_yaw, quat_zw
        self.pose7, self.n_scored, self.n_changed = pose7, n_scored, n_changed


def _information_layer(call, handle, check, grid_shape, grid_geom, stride_cells, n_yaw, yaw0, pose_z, reduce, info_lo, info_hi, max_cost,
                       window, write, want_per_yaw):
    """The body of FrontierScorer.information_layer and MultiScorer.information_layer."""
    nz, ny, nx = grid_shape
    x0, y0, sx, sy = (0, 0, nx, ny) if window is None else [int(v) for v in window]
    if reduce not in INFO_REDUCE:
        raise FsError(FS_E_INVALID, "reduce must be one of %s" % sorted(INFO_REDUCE))
    p = InfoLayerParamsC(int(stride_cells), int(n_yaw), float(yaw0), float(pose_z), INFO_REDUCE[reduce], float(info_lo), float(info_hi),
                         int(max_cost), 1 if write else 0)
    s, K = max(1, p.stride_cells), max(0, p.n_yaw)           # (room for the outputs; the call refuses what is out of range)
    nbx, nby = max(0, -(-sx // s)), max(0, -(-sy // s))
    info = np.full((nby, nbx), np.nan, dtype=np.float32)
    anchor = np.full((nby, nbx), -1, dtype=np.int32)
    per_yaw = np.full((K, nby, nbx), np.nan, dtype=np.float32) if want_per_yaw else None
    quat = np.zeros((max(K, FS_INFO_LAYER_MAX_YAW), 2), dtype=np.float64)
    n_scored, n_changed = C.c_int64(), C.c_int64()
    check(call(handle, C.byref(p), x0, y0, sx, sy, _p(info), _p(anchor), _p(per_yaw), _p(quat), C.byref(n_scored), C.byref(n_changed)))
    quat = quat[:K].copy()
    cells = anchor.reshape(-1)
    cells = cells[cells >= 0].astype(np.int64)
    (ox, oy, _oz), res = grid_geom
    pose7 = np.zeros((cells.size, K, 7), dtype=np.float64)
    pose7[:, :, 0] = (ox + ((cells % nx).astype(np.float64) + 0.5) * res)[:, None]
    pose7[:, :, 1] = (oy + ((cells // nx).astype(np.float64) + 0.5) * res)[:, None]
    pose7[:, :, 2] = float(pose_z)
    pose7[:, :, 5] = quat[None, :, 0]
    pose7[:, :, 6] = quat[None, :, 1]
    return InformationLayerResult(info, anchor, per_yaw, quat, pose7.reshape(-1, 7), n_scored.value, n_changed.value)


def _window_args(window, view):
    """(pointer, sx, sy, sz, row_stride, slice_stride, keep-alive) of a window given as its own array [sz][sy][sx] (or [sy][sx]),
    or — view=True — as a numpy VIEW into the caller's whole map: the view's strides are passed on and nothing is packed"""
    w = np.asarray(window, dtype=np.uint8)
    if w.ndim == 2:
        w = w[None]
    if not view or w.size == 0:
        w = np.ascontiguousarray(w)
        sz, sy, sx = w.shape
        return _p(w), sx, sy, sz, 0, 0, w
    if w.strides[2] != 1:
        raise ValueError("a window view must be contiguous along x")
    sz, sy, sx = w.shape
    return C.c_void_p(w.ctypes.data), sx, sy, sz, (w.strides[1] if sy > 1 else 0), (w.strides[0] if sz > 1 else 0), w


class FrontierScorer:
    """One scoring context = one GPU + one HIP stream.  Mirrors the call order of the reference:
    construct (parameters) -> grid snapshot -> max-arrival calibration -> score."""

    def __init__(self, device: int = 0, stream: int | None = None, library=None):
        self._L = library if library is not None else load_library()
        h = C.c_void_p()
        rc = self._L.fs_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != FS_OK:
            raise FsError(rc, "fs_ctx_create failed: no gfx950 device / HIP runtime (no CPU fallback exists)")
        self._h = h
        self._elev = (0.0,)
        self._grid_shape = None          # (nz, ny, nx) of the staged grid: what fs_navfn_potential writes
        self._seed_order = "nearest"     # the context's frontier seed order (fs_set_frontier_seed_order)
        self._roadmap_search = "tree"    # the context's roadmap search (fs_set_roadmap_search)
        self._grid_search = "converged"  # the context's grid search (fs_set_grid_search)
        self._refine_search = "field"    # the context's refine search (fs_set_refine_search)
        self.n_yaw = self.n_elev = self.window = 0

    # -- plumbing
    def _check(self, rc):
        if rc != FS_OK:
            raise FsError(rc, (self._L.fs_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            if os.environ.get("FS_BOUNDS"):
                # library built with FS_BOUNDS=1 (range-checked global accesses): counters 29 (ray walks) and 30 (FIM
                # kernels) hold the code of a violated check, 0 if none
                ray, fim = self.get_counter(29), self.get_counter(30)
                if ray or fim:
                    raise FsError(f"FS_BOUNDS: range check violated (ray walk code {ray}, FIM kernel code {fim})")
            self._L.fs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self._L.fs_synchronize(self._h))

    def enable_kernel_timing(self, on=True):
        self._check(self._L.fs_enable_kernel_timing(self._h, 1 if on else 0))

    def kernel_time(self, kind: int):
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._L.fs_kernel_time(self._h, kind, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def set_option(self, key: str, value: float):
        self._check(self._L.fs_set_option(self._h, key.encode(), float(value)))

    def get_counter(self, which: int, reset: bool = False) -> int:
        v = C.c_int64()
        self._check(self._L.fs_get_counter(self._h, int(which), C.byref(v), 1 if reset else 0))
        return v.value

    # -- arrival information
    def set_ray_params(self, max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, robot_radius=0.60,
                       n_rays=0, elev=(0.0,), obst=(240, 254), trace=(255, 255), factor_max=1.2,
                       factor_min=0.70, polygon=(-1e300, -1e300, 1e300, 1e300)):
        p = _ray_params_c(max_camera_depth, delta_theta, camera_fov, robot_radius, n_rays, elev, obst, trace, factor_max, factor_min, polygon)
        self._check(self._L.fs_set_ray_params(self._h, C.byref(p)))
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.fs_ray_fan_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_yaw, self.n_elev, self.window = a.value, b.value, c.value
        self._delta_theta, self._camera_fov = float(delta_theta), float(camera_fov)

    def upload_grid(self, cells: np.ndarray, origin, resolution: float):
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        if c.ndim == 2:
            c = c[None]
        nz, ny, nx = c.shape
        o = (C.c_double * 3)(*[float(v) for v in origin])
        self._grid_shape = None
        self._check(self._L.fs_upload_grid(self._h, _p(c), nx, ny, nz, C.byref(o), float(resolution)))
        self._grid_shape = (nz, ny, nx)
        self._grid_geom = (tuple(float(v) for v in origin), float(resolution))

    def update_grid_region(self, x0, y0, z0, window, view=False):
        """fs_update_grid_region: `window` [sz][sy][sx] (or [sy][sx]) replaces the cells from (x0, y0, z0) on; view=True passes a
        numpy view into the caller's whole map with its strides (nothing packed on the Python side)"""
        ptr, sx, sy, sz, rs, ss, keep = _window_args(window, view)
        self._check(self._L.fs_update_grid_region(self._h, int(x0), int(y0), int(z0), sx, sy, sz, ptr, rs, ss))

    def read_grid_region(self, x0=0, y0=0, z0=0, shape=None, out=None):
        """fs_read_grid_region: the window [sz][sy][sx] of the staged grid from (x0, y0, z0) on, as a new array of `shape`
        ((sy, sx) or (sz, sy, sx); default: the rest of the grid) — or written into `out`, which may be a numpy VIEW into a
        larger array (contiguous along x): its strides are passed on."""
        if out is None:
            if shape is None:
                nz, ny, nx = self._staged_shape()
                shape = (nz - int(z0), ny - int(y0), nx - int(x0))
            out = np.zeros(tuple(int(v) for v in shape), dtype=np.uint8)
        if out.dtype != np.uint8 or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writable uint8 array")
        ptr, sx, sy, sz, rs, ss, keep = _window_args(out, True)
        self._check(self._L.fs_read_grid_region(self._h, int(x0), int(y0), int(z0), sx, sy, sz, ptr, rs, ss))
        return out

    # -- keep-out zones (the costmap layer LethalMarker)
    def keepout_add_fov(self, wx, wy, yaw, height_m=3.5):
        """fs_keepout_add_fov (addNewMarkedAreaFOV): returns (zone id, distinct cells marked on the staged map)."""
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_keepout_add_fov(self._h, float(wx), float(wy), float(yaw), float(height_m), C.byref(zid), C.byref(n)))
        return zid.value, n.value

    def keepout_add_disc(self, wx, wy, radius_m=1.7):
        """fs_keepout_add_disc (the older layer's addNewMarkedArea): returns (zone id, distinct cells)."""
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_keepout_add_disc(self._h, float(wx), float(wy), float(radius_m), C.byref(zid), C.byref(n)))
        return zid.value, n.value

    def keepout_clear(self):
        """fs_keepout_clear: forgets the zones; cells already painted stay 253 until the map is staged again."""
        self._check(self._L.fs_keepout_clear(self._h))

    def keepout_get(self, want_mask=True):
        """fs_keepout_get: (spec [n][5] = kind, wx, wy, yaw, size; n_cells [n]; union mask [ny][nx] or None)."""
        spec = np.zeros((FS_KEEPOUT_MAX_ZONES, 5), dtype=np.float64)
        cells = np.zeros(FS_KEEPOUT_MAX_ZONES, dtype=np.int64)
        mask = None
        if want_mask and self._grid_shape is not None:
            mask = np.zeros(self._grid_shape[1:], dtype=np.uint8)
        n = C.c_int32()
        self._check(self._L.fs_keepout_get(self._h, C.byref(n), _p(spec), _p(cells), _p(mask)))
        return spec[:n.value].copy(), cells[:n.value].copy(), mask

    def mark_lethal_fov(self, robot_pose7):
        """fs_mark_lethal_fov (MarkLethalFOV::tick): returns (blacklisted pose [7], zone id, distinct cells)."""
        pose = (C.c_double * 7)(*[float(v) for v in robot_pose7])
        black = (C.c_double * 7)()
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_mark_lethal_fov(self._h, C.byref(pose), C.byref(black), C.byref(zid), C.byref(n)))
        return np.array(black[:], dtype=np.float64), zid.value, n.value

    # -- inflation layer (nav2's InflationLayer on the exact distance to the nearest lethal cell)
    def inflate(self, inflation_radius, inscribed_radius, cost_scaling_factor, window=None, inflate_unknown=False):
        """fs_inflate: inflates the staged 2-D grid in place inside window = (x0, y0, sx, sy) (None: the whole map);
        returns (seeds in the window grown by the radius, window cells whose byte changed)."""
        if window is None:
            nz, ny, nx = self._staged_shape()
            window = (0, 0, nx, ny)
        p = _inflation_params_c(inflation_radius, inscribed_radius, cost_scaling_factor, inflate_unknown)
        seeds, changed = C.c_int64(), C.c_int64()
        self._check(self._L.fs_inflate(self._h, C.byref(p), *[int(v) for v in window], C.byref(seeds), C.byref(changed)))
        return seeds.value, changed.value

    def information_layer(self, stride_cells=5, n_yaw=8, yaw0=0.0, pose_z=0.0, reduce="mean", info_lo=550.0, info_hi=1100.0, max_cost=252,
                          window=None, write=True, want_per_yaw=False):
        """fs_information_layer — this project's own extension, the reference has no such layer: the Fisher information of a
        lattice of poses (one per block of stride_cells x stride_cells cells, n_yaw headings each, reduced by "min" | "mean" | "max")
        as costs of the staged 2-D grid inside window = (x0, y0, sx, sy) (None: the whole map): cost max_cost at info_lo and below,
        0 at info_hi and above, linear between, stored by max into the writable cells (write=False: the field only).
        info_lo = 550 is the reference's isPoseSafe threshold (FisherInfoBTPlugin.cpp:20); info_hi = 2 * info_lo is a default
        nobody has measured.  Call it after staging and inflate, before planning.  Returns an InformationLayerResult."""
        return _information_layer(self._L.fs_information_layer, self._h, self._check, self._staged_shape(), self._grid_geom, stride_cells,
                                  n_yaw, yaw0, pose_z, reduce, info_lo, info_hi, max_cost, window, write, want_per_yaw)

    def inflation_costs(self, inflation_radius, inscribed_radius, cost_scaling_factor):
        """fs_inflation_costs: (R = the radius in cells of the staged grid, cost_by_d2 [R * R + 1] = the table fs_inflate uses)."""
        p = _inflation_params_c(inflation_radius, inscribed_radius, cost_scaling_factor, False)
        r = C.c_int32()
        self._check(self._L.fs_inflation_costs(self._h, C.byref(p), C.byref(r), None))
        table = np.zeros(r.value * r.value + 1, dtype=np.uint8)
        self._check(self._L.fs_inflation_costs(self._h, C.byref(p), C.byref(r), _p(table)))
        return r.value, table

    def upload_grid_bricks(self, shape_zyx, origin, resolution, brick_xyz, brick_cells, default_value=255):
        nz, ny, nx = shape_zyx
        xyz = np.ascontiguousarray(brick_xyz, dtype=np.int32).reshape(-1, 3)
        cells = np.ascontiguousarray(brick_cells, dtype=np.uint8).reshape(-1, 512)
        o = (C.c_double * 3)(*[float(v) for v in origin])
        self._grid_shape = None
        self._check(self._L.fs_upload_grid_bricks(self._h, nx, ny, nz, C.byref(o), float(resolution), int(default_value),
                                                  xyz.shape[0], _p(xyz), _p(cells)))
        self._grid_shape = (int(nz), int(ny), int(nx))
        self._grid_geom = (tuple(float(v) for v in origin), float(resolution))

    def frontier_cells(self, shape_zyx, lethal_threshold=160, want_mask=True):
        mask = np.zeros(shape_zyx, dtype=np.uint8) if want_mask else None
        n = C.c_int64()
        self._check(self._L.fs_frontier_cells(self._h, int(lethal_threshold), _p(mask), C.byref(n)))
        return mask, n.value

    def frontier_clusters(self, shape_yx, robot_xy, lethal_threshold=160, max_frontier_distance=50.0, max_frontier_cluster_size=20,
                          max_clusters=65536, want_labels=True):
        """FrontierSearch::searchFrom as clusters: returns (labels [ny][nx] or None, clusters (CLUSTER_DTYPE, ascending label),
        n_clusters, n_cells)."""
        ny, nx = shape_yx[-2], shape_yx[-1]
        labels = np.zeros((ny, nx), dtype=np.int32) if want_labels else None
        cl = np.zeros(max_clusters, dtype=CLUSTER_DTYPE)
        n, cells = C.c_int32(), C.c_int64()
        xy = (C.c_double * 2)(float(robot_xy[0]), float(robot_xy[1]))
        self._check(self._L.fs_frontier_clusters(self._h, C.byref(xy), int(lethal_threshold), float(max_frontier_distance),
                                                 int(max_frontier_cluster_size), _p(labels), int(max_clusters), _p(cl),
                                                 C.byref(n), C.byref(cells)))
        return labels, cl[:min(n.value, max_clusters)].copy(), n.value, cells.value

    # first-round output capacity of the search calls when the caller gives none: frontier lists are far shorter than the grid, so
    # a longer one costs a second call with exact sizes instead of nx * ny zeroed records every time
    SEARCH_FIRST_RECORDS, SEARCH_FIRST_CELLS = 4096, 65536

    def set_frontier_seed_order(self, order: str):
        """The seeds of search_frontiers without seeds and of get_frontier_costs_searched (fs_set_frontier_seed_order):
        "nearest" (a fresh context's) or "reference" (the reference's outer search decides seeds and list order)."""
        self._set_mode("_seed_order", order)

    # the context's named modes, by the attribute that remembers the setting: (names, C setter, what an error calls it)
    _MODES = {"_seed_order": (SEED_ORDERS, "fs_set_frontier_seed_order", "frontier seed order"),
              "_grid_search": (GRID_SEARCHES, "fs_set_grid_search", "grid search"),
              "_roadmap_search": (ROADMAP_SEARCHES, "fs_set_roadmap_search", "roadmap search"),
              "_refine_search": (REFINE_SEARCHES, "fs_set_refine_search", "refine search")}

    def _set_mode(self, attr, name):
        names, setter, what = self._MODES[attr]
        if name not in names:
            raise FsError(FS_E_INVALID, f"unknown {what} {name!r} ({' | '.join(names)})")
        self._check(getattr(self._L, setter)(self._h, names[name]))
        setattr(self, attr, name)

    @contextlib.contextmanager
    def _mode_for_call(self, attr, name):
        """seed_order= / search= of one call: set for the call, the context's own setting restored afterwards"""
        if name is None:
            yield
            return
        prev = getattr(self, attr)
        self._set_mode(attr, name)
        try:
            yield
        finally:
            self._set_mode(attr, prev)

    def search_frontiers(self, robot_xy, lethal_threshold=160, max_frontier_distance=50.0, min_frontier_cluster_size=1,
                         max_frontier_cluster_size=20, seeds=None, max_records=None, want_every=True, seed_order=None):
        """FrontierSearch::searchFrom on the device, pieces and goal points included (fs_search_frontiers): returns (frontiers
        (FRONTIER_RECORD_DTYPE, output order), every_xy [n_cells][2] or None).  seeds None: the context's seed order
        (set_frontier_seed_order; seed_order= "nearest" / "reference" for this call only); else the cells (y * nx + x) that start
        one buildNewFrontier each, in order.  max_records None: every record (the buffers grow to what the search reports, at most
        the grid's cell count); else at most that many (last_search_counts has the full counts)."""
        with self._mode_for_call("_seed_order", seed_order):
            return self._search_frontiers(robot_xy, lethal_threshold, max_frontier_distance, min_frontier_cluster_size,
                                          max_frontier_cluster_size, seeds, max_records, want_every)

    def _search_frontiers(self, robot_xy, lethal_threshold, max_frontier_distance, min_frontier_cluster_size,
                          max_frontier_cluster_size, seeds, max_records, want_every):
        _, ny, nx = self._staged_shape()
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        xy = (C.c_double * 2)(float(robot_xy[0]), float(robot_xy[1]))
        cap = min(nx * ny, self.SEARCH_FIRST_RECORDS) if max_records is None else int(max_records)
        ecap = min(nx * ny, self.SEARCH_FIRST_CELLS) if want_every else 0
        while True:
            rec = np.zeros(max(cap, 0), dtype=FRONTIER_RECORD_DTYPE)
            every = np.zeros((ecap, 2)) if want_every else None
            n, cells = C.c_int32(), C.c_int64()
            self._check(self._L.fs_search_frontiers(self._h, C.byref(xy), int(lethal_threshold), float(max_frontier_distance),
                                                    int(min_frontier_cluster_size), int(max_frontier_cluster_size),
                                                    0 if sd is None else sd.shape[0], _p(sd), cap, _p(rec), C.byref(n),
                                                    ecap, _p(every), C.byref(cells)))
            grow = (max_records is None and n.value > cap) or (want_every and cells.value > ecap)
            if not grow:
                break
            cap = max(cap, n.value) if max_records is None else cap
            ecap = max(ecap, cells.value) if want_every else 0
        self.last_search_counts = (n.value, cells.value)
        return rec[:min(n.value, cap)].copy(), None if every is None else every[:cells.value].copy()

    def get_frontier_costs_searched(self, robot_pose7, lethal_threshold=160, max_frontier_distance=50.0, min_frontier_cluster_size=1,
                                    max_frontier_cluster_size=20, blacklist_xy=None, allow_unknown=False, with_fim=False, alpha=0.25,
                                    beta=1.0, max_vx=0.5, max_wz=0.5, max_records=None, seed_order=None):
        """searchFrom -> plan -> score -> rank in one call (fs_get_frontier_costs_searched): returns (frontiers, the dict
        get_frontier_costs_planned returns).  blacklist_xy [k][2]: goal points to mark blacklisted (exact equality).
        max_records None: as many as the search finds (a longer list than the first round holds is searched again with exact
        sizes); else more records than that raise FsError.  seed_order: as search_frontiers'."""
        with self._mode_for_call("_seed_order", seed_order):
            return self._get_frontier_costs_searched(robot_pose7, lethal_threshold, max_frontier_distance, min_frontier_cluster_size,
                                                     max_frontier_cluster_size, blacklist_xy, allow_unknown, with_fim, alpha, beta,
                                                     max_vx, max_wz, max_records)

    def _get_frontier_costs_searched(self, robot_pose7, lethal_threshold, max_frontier_distance, min_frontier_cluster_size,
                                     max_frontier_cluster_size, blacklist_xy, allow_unknown, with_fim, alpha, beta, max_vx, max_wz,
                                     max_records):
        _, ny, nx = self._staged_shape()
        cap = min(nx * ny, self.SEARCH_FIRST_RECORDS) if max_records is None else int(max_records)
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        bl = None if blacklist_xy is None else np.ascontiguousarray(np.asarray(blacklist_xy, dtype=np.float64).reshape(-1, 2))
        while True:
            fr = np.zeros(max(cap, 0), dtype=FRONTIER_RECORD_DTYPE)
            rec = np.zeros(max(cap, 0), dtype=RECORD_DTYPE)
            cost = np.zeros(max(cap, 0)); au = np.zeros(max(cap, 0)); du = np.zeros(max(cap, 0))
            order = np.zeros(max(cap, 0), dtype=np.int32); plm = np.zeros(max(cap, 0))
            n = C.c_int32()
            rc = self._L.fs_get_frontier_costs_searched(self._h, C.byref(pose), int(lethal_threshold), float(max_frontier_distance),
                                                        int(min_frontier_cluster_size), int(max_frontier_cluster_size), 1 if allow_unknown else 0,
                                                        0 if bl is None else bl.shape[0], _p(bl), alpha, beta, max_vx, max_wz,
                                                        1 if with_fim else 0, cap, _p(fr), C.byref(n), _p(rec), _p(cost), _p(au), _p(du),
                                                        _p(order), _p(plm))
            if rc == FS_E_INVALID and max_records is None and n.value > cap:
                cap = n.value
                continue
            self._check(rc)
            break
        k = n.value
        return fr[:k].copy(), dict(records=rec[:k].copy(), weighted_cost=cost[:k].copy(), arrival_utility=au[:k].copy(),
                                   distance_utility=du[:k].copy(), order=order[:k].copy(), path_length_m=plm[:k].copy())

    def get_frontier_costs_searched_roadmap(self, robot_pose7, lethal_threshold=160, max_frontier_distance=50.0, min_frontier_cluster_size=1,
                                            max_frontier_cluster_size=20, blacklist_xy=None, add_robot_pose=True, with_fim=False,
                                            alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5, max_records=None, seed_order=None, search=None):
        """The default planner's tick in one call (fs_get_frontier_costs_searched_roadmap): search -> roadmap_update -> roadmap plan ->
        score -> rank.  Returns (frontiers, the dict get_frontier_costs_roadmap returns).  max_records None: as many as the search finds (a list longer than the first
        round holds is refused before the roadmap is touched, and searched again).  seed_order as search_frontiers', search as roadmap_plan's.  A cell overfilled by the update
        raises FsError(FS_E_RANGE); self.last_searched_frontiers then holds the frontier records."""
        _, ny, nx = self._staged_shape()
        cap = min(nx * ny, self.SEARCH_FIRST_RECORDS) if max_records is None else int(max_records)
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        bl = None if blacklist_xy is None else np.ascontiguousarray(np.asarray(blacklist_xy, dtype=np.float64).reshape(-1, 2))
        with self._mode_for_call("_seed_order", seed_order), self._mode_for_call("_roadmap_search", search):
            while True:
                fr = np.zeros(max(cap, 0), dtype=FRONTIER_RECORD_DTYPE)
                rec = np.zeros(max(cap, 0), dtype=RECORD_DTYPE)
                cost = np.zeros(max(cap, 0)); au = np.zeros(max(cap, 0)); du = np.zeros(max(cap, 0))
                order = np.zeros(max(cap, 0), dtype=np.int32); plm = np.zeros(max(cap, 0))
                n = C.c_int32()
                rc = self._L.fs_get_frontier_costs_searched_roadmap(self._h, C.byref(pose), int(lethal_threshold), float(max_frontier_distance),
                                                                    int(min_frontier_cluster_size), int(max_frontier_cluster_size),
                                                                    1 if add_robot_pose else 0, 0 if bl is None else bl.shape[0], _p(bl),
                                                                    alpha, beta, max_vx, max_wz, 1 if with_fim else 0, cap, _p(fr), C.byref(n),
                                                                    _p(rec), _p(cost), _p(au), _p(du), _p(order), _p(plm))
                if rc == FS_E_INVALID and max_records is None and n.value > cap:      # (refused before the roadmap was touched)
                    cap = n.value
                    continue
                break
        k = min(n.value, cap)
        self.last_searched_frontiers = fr[:k].copy()
        self._check(rc)
        return fr[:k].copy(), dict(records=rec[:k].copy(), weighted_cost=cost[:k].copy(), arrival_utility=au[:k].copy(),
                                   distance_utility=du[:k].copy(), order=order[:k].copy(), path_length_m=plm[:k].copy())

    def _staged_shape(self):
        if self._grid_shape is None:
            raise FsError(FS_E_STATE, "no grid staged (upload_grid)")
        return self._grid_shape

    def max_arrival(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._L.fs_max_arrival(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(max_value=a.value, max_gt=b.value, min_gt=c.value)

    def set_arrival_limits(self, max_gt, min_gt):
        self._check(self._L.fs_set_arrival_limits(self._h, float(max_gt), float(min_gt)))

    def score_arrival(self, goal_xyz, frontier_size=None, blacklisted=None, achievable_in=None, want_ray_counts=True):
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rc_arr = np.zeros((n, self.n_elev, self.n_yaw), dtype=np.int32) if want_ray_counts else None
        arrival = np.zeros(n, dtype=np.int32); argmax = np.zeros(n, dtype=np.int32)
        yaw = np.zeros(n, dtype=np.float64); ach = np.zeros(n, dtype=np.uint8); status = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_score_arrival(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(rc_arr),
                                             _p(arrival), _p(argmax), _p(yaw), _p(ach), _p(status)))
        return dict(ray_counts=rc_arr, arrival=arrival, argmax=argmax, yaw=yaw, achievable=ach, status=status)

    def trace_segments(self, start_xyz, end_xyz, max_length_cells, obst=(253, 254), trace=(0, 255)):
        a = np.ascontiguousarray(start_xyz, dtype=np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(end_xyz, dtype=np.float64).reshape(-1, 3)
        n = a.shape[0]
        ok = np.zeros(n, np.uint8); hit = np.zeros(n, np.uint8)
        traced = np.zeros(n, np.int32); unknown = np.zeros(n, np.int32); allc = np.zeros(n, np.int32)
        self._check(self._L.fs_trace_segments(self._h, n, _p(a), _p(b), float(max_length_cells), int(obst[0]), int(obst[1]),
                                              int(trace[0]), int(trace[1]), _p(ok), _p(traced), _p(hit), _p(unknown), _p(allc)))
        return dict(ok=ok, traced=traced, hit=hit, unknown=unknown, all=allc)

    # -- Fisher information
    def upload_landmarks(self, xyz):
        lm = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._check(self._L.fs_upload_landmarks(self._h, _p(lm), lm.shape[0]))

    def lookup_generate(self, bounds=None):
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float32)
        self._check(self._L.fs_lookup_generate(self._h, _p(b)))

    def lookup_load(self, path: str):
        self._check(self._L.fs_lookup_load(self._h, path.encode()))

    def lookup_save(self, path: str):
        self._check(self._L.fs_lookup_save(self._h, path.encode()))

    def lookup_set_records(self, records):
        r = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 4)
        self._check(self._L.fs_lookup_set_records(self._h, _p(r), r.shape[0]))

    def lookup_records(self) -> np.ndarray:
        n = C.c_int64()
        self._check(self._L.fs_lookup_num_records(self._h, C.byref(n)))
        out = np.zeros((n.value, 4), dtype=np.float32)
        self._check(self._L.fs_lookup_get_records(self._h, _p(out)))
        return out

    def lookup_query(self, p) -> float:
        a = np.ascontiguousarray(p, dtype=np.float32)
        v = C.c_float()
        self._check(self._L.fs_lookup_query(self._h, _p(a), C.byref(v)))
        return v.value

    def set_fim_params(self, max_dist=14.0, max_angle=1.0):
        p = FimParamsC(max_dist, max_angle)
        self._check(self._L.fs_set_fim_params(self._h, C.byref(p)))

    def set_occlusion(self, enabled, occ=(254, 254), end_margin_m=0.3):
        """fs_set_occlusion: with `enabled`, a landmark counts only if the line from the pose to it crosses no cell with a cost
        in occ = (min, max) on the staged grid; the last 1 + int(end_margin_m / resolution) cells at the landmark's end are
        not tested."""
        p = OcclusionParamsC(1 if enabled else 0, int(occ[0]), int(occ[1]), float(end_margin_m))
        self._check(self._L.fs_set_occlusion(self._h, C.byref(p)))

    def get_occlusion(self):
        p = OcclusionParamsC()
        self._check(self._L.fs_get_occlusion(self._h, C.byref(p)))
        return dict(enabled=bool(p.enabled), occ=(p.occ_min, p.occ_max), end_margin_m=p.end_margin_m)

    def line_of_sight(self, from_xyz, to_xyz):
        """fs_line_of_sight: the rule of set_occlusion (its range and margin, enabled or not) for pairs of points."""
        a = np.ascontiguousarray(from_xyz, dtype=np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(to_xyz, dtype=np.float64).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError("from_xyz and to_xyz must hold the same number of points")
        n = a.shape[0]
        ok = np.zeros(n, np.uint8); blocked = np.zeros(n, np.uint8); tested = np.zeros(n, np.int32)
        self._check(self._L.fs_line_of_sight(self._h, n, _p(a), _p(b), _p(ok), _p(blocked), _p(tested)))
        return dict(ok=ok, blocked=blocked, tested_cells=tested)

    def score_fim(self, pose7, want_fim=True, info_only=False):
        """info_only: what isPoseSafe itself needs — info_ref (and n_voxels); every other column is passed as NULL, which
        selects the worker without the 6x6 sums and with the exact table-box cull."""
        ps = np.ascontiguousarray(pose7, dtype=np.float64).reshape(-1, 7)
        n = ps.shape[0]
        info = np.zeros(n, dtype=np.float32)
        if info_only:
            nvox = np.zeros(n, dtype=np.int32)
            self._check(self._L.fs_score_fim(self._h, n, _p(ps), _p(info), None, None, None, None, _p(nvox)))
            return dict(info_ref=info, n_voxels=nvox)
        fim21 = np.zeros((n, 21), dtype=np.float32) if want_fim else None
        trace = np.zeros(n, dtype=np.float32); logdet = np.zeros(n, dtype=np.float32)
        nvis = np.zeros(n, dtype=np.int32); nvox = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_score_fim(self._h, n, _p(ps), _p(info), _p(fim21), _p(trace), _p(logdet), _p(nvis), _p(nvox)))
        return dict(info_ref=info, fim21=fim21, trace=trace, logdet=logdet, n_visible=nvis, n_voxels=nvox)

    def landmarks_in_view(self, pose7, max_total=None):
        """fs_landmarks_in_view: (offsets [n + 1] int64, entries VIEW_DTYPE) — the landmarks score_fim counts in n_visible, per pose
        in ascending upload index; pose i's entries are entries[offsets[i]:offsets[i + 1]].  max_total None: the count-only form,
        then a fill of exactly offsets[n] entries.  An integer is passed straight through: `entries` is the stored prefix,
        min(offsets[n], max_total) long, and offsets still holds the true counts."""
        ps = np.ascontiguousarray(pose7, dtype=np.float64).reshape(-1, 7)
        n = ps.shape[0]
        off = np.zeros(n + 1, dtype=np.int64)
        if max_total is None:
            self._check(self._L.fs_landmarks_in_view(self._h, n, _p(ps), 0, _p(off), None))
            max_total = int(off[n])
        max_total = int(max_total)
        out = np.zeros(max_total, dtype=VIEW_DTYPE)
        self._check(self._L.fs_landmarks_in_view(self._h, n, _p(ps), max_total, _p(off), _p(out) if max_total > 0 else None))
        return off, out[:min(int(off[n]), max_total)]

    def staged_cloud(self):
        """fs_staged_cloud_get: the staged cloud as the kernels read it — a dict with m, n_chunks,
        soa [3][n_chunks * 64] (x, y, z in k-d leaf order, sentinels in the padding), spheres [n_chunks][4], perm [n_chunks * 64]."""
        m, nc = C.c_int32(), C.c_int32()
        self._check(self._L.fs_staged_cloud_get(self._h, C.byref(m), C.byref(nc), None, None, None))
        soa = np.zeros((3, nc.value * 64), dtype=np.float32)
        sph = np.zeros((nc.value, 4), dtype=np.float32)
        perm = np.zeros(nc.value * 64, dtype=np.int32)
        self._check(self._L.fs_staged_cloud_get(self._h, C.byref(m), C.byref(nc), _p(soa), _p(sph), _p(perm)))
        return dict(m=m.value, n_chunks=nc.value, soa=soa, spheres=sph, perm=perm)

    # -- the sensor sweep on a ground-truth world (this project's own extension)
    def upload_world(self, cells):
        """fs_upload_world: the ground truth behind the staged grid, of its shape ([nz][ny][nx] or [ny][nx]); None releases it."""
        if cells is None:
            self._check(self._L.fs_upload_world(self._h, None, 0, 0, 0))
            return
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        if c.ndim == 2:
            c = c[None]
        nz, ny, nx = c.shape
        self._check(self._L.fs_upload_world(self._h, _p(c), nx, ny, nz))

    def sense(self, origins, first_ray=None, sensor=None, rays=False):
        """fs_sense: one sweep of the arrival fan from each of origins [n][3] through the world; what it sees is copied into the staged
        grid on the device.  first_ray [n]: -1 = all yaw rays, else the FOV window starting there (`argmax` of the scoring calls);
        None = all rays for every pose.  sensor: a dict of set_ray_params' keyword arguments for a fan of its own (None: the
        context's).  Returns a dict: status [n], seen_unknown [n], ray_unknown [n][n_elev][n_yaw] (rays=True, else None), n_seen,
        n_revealed, window (x0, y0, z0, sx, sy, sz)."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        fr = None if first_ray is None else np.ascontiguousarray(first_ray, dtype=np.int32).reshape(-1)
        if fr is not None and fr.shape[0] != n:
            raise ValueError("first_ray must hold one entry per pose")
        sp, n_elev, n_yaw = None, self.n_elev, self.n_yaw
        if sensor is not None:
            sp = _ray_params_c(**sensor)
            n_elev, n_yaw = sp.n_elev, fan_n_yaw(sp.delta_theta, sp.n_rays)
        ru = np.zeros((n, n_elev, n_yaw), dtype=np.int32) if rays else None
        seen = np.zeros(n, dtype=np.int32); status = np.zeros(n, dtype=np.int32)
        n_seen, n_rev = C.c_int64(), C.c_int64()
        win = np.zeros(6, dtype=np.int32)
        self._check(self._L.fs_sense(self._h, n, _p(o), _p(fr), None if sp is None else C.byref(sp), _p(ru), _p(seen), _p(status),
                                     C.byref(n_seen), C.byref(n_rev), _p(win)))
        return dict(status=status, seen_unknown=seen, ray_unknown=ru, n_seen=n_seen.value, n_revealed=n_rev.value,
                    window=tuple(int(v) for v in win))

    def goals_mapped(self, goals):
        """fs_goals_mapped: surroundingCellsMapped (what CheckIfGoalMapped asks) for goals [n][3] on the staged 2-D grid -> uint8 [n]."""
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(g.shape[0], dtype=np.uint8)
        self._check(self._L.fs_goals_mapped(self._h, g.shape[0], _p(g), _p(out)))
        return out

    def grid_census(self):
        """fs_grid_census: cells of the staged grid that are known (!= 255), unknown (== 255), lethal (== 254), free (== 0)."""
        v = np.zeros(4, dtype=np.int64)
        self._check(self._L.fs_grid_census(self._h, _p(v)))
        return dict(known=int(v[0]), unknown=int(v[1]), lethal=int(v[2]), free=int(v[3]))

    def drive(self, stations, goals, first_ray=None, sensor=None, block=(253, 254), stop_when_mapped=True):
        """fs_drive: robot r drives stations[r] ([n_r][3], n_r >= 1) through the world, sensing at every station,
        and stops at a cost in `block` on the staged map (FS_DRIVE_BLOCKED), at one only the world holds (COLLIDED), off the map
        (OFF_MAP), when goals[r] is mapped (MAPPED, with stop_when_mapped) or out of stations (ARRIVED) — one call and one wait for
        all robots and stations.  first_ray: None (every station sweeps all rays) or one [n_r] array per robot, as sense()'s;
        sensor: as sense()'s.  Returns a dict: status [R], reached [R], station_status and seen_unknown (a list of [n_r] arrays;
        -1 and 0 for stations never reached), n_seen, n_revealed, window (x0, y0, z0, sx, sy, sz)."""
        st = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in stations]
        R = len(st)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        if g.shape[0] != R:
            raise ValueError("goals must hold one entry per robot")
        ns = np.array([a.shape[0] for a in st], dtype=np.int32)
        T = int(ns.sum())
        xyz = np.ascontiguousarray(np.concatenate(st, axis=0)) if R else np.zeros((0, 3))
        fr = None
        if first_ray is not None:
            if len(first_ray) != R:
                raise ValueError("first_ray must hold one array per robot")
            parts = [np.asarray(f, dtype=np.int32).reshape(-1) for f in first_ray]
            if any(f.shape[0] != n for f, n in zip(parts, ns)):
                raise ValueError("first_ray must hold one entry per station")
            fr = np.ascontiguousarray(np.concatenate(parts)) if R else np.zeros(0, dtype=np.int32)
        sp = None if sensor is None else _ray_params_c(**sensor)
        dp = DriveParamsC(int(block[0]), int(block[1]), 1 if stop_when_mapped else 0)
        status = np.zeros(R, dtype=np.int32); reached = np.zeros(R, dtype=np.int32)
        sst = np.zeros(T, dtype=np.int32); seen = np.zeros(T, dtype=np.int32)
        n_seen, n_rev = C.c_int64(), C.c_int64()
        win = np.zeros(6, dtype=np.int32)
        self._check(self._L.fs_drive(self._h, R, _p(xyz), _p(ns), _p(fr), _p(g), None if sp is None else C.byref(sp), C.byref(dp),
                                     _p(status), _p(reached), _p(sst), _p(seen), C.byref(n_seen), C.byref(n_rev), _p(win)))
        cut = np.cumsum(ns)[:-1] if R else []
        return dict(status=status, reached=reached, station_status=np.split(sst, cut) if R else [], seen_unknown=np.split(seen, cut) if R else [],
                    n_seen=n_seen.value, n_revealed=n_rev.value, window=tuple(int(v) for v in win))

    def first_ray_for_yaw(self, yaw):
        """The window start i whose pose yaw i * delta_theta + camera_fov / 2 (DEP/src/CostCalculator.cpp:119) is nearest to `yaw`,
        in [0, n_yaw - window]: what sense() takes as first_ray for a camera looking that way."""
        if not self.n_yaw:
            raise FsError(FS_E_STATE, "no ray parameters set (set_ray_params)")
        return first_ray_for_yaw(yaw, self._delta_theta, self._camera_fov, self.n_yaw)

    # -- the landmark sensor on a ground-truth cloud (this project's own extension)
    def upload_world_landmarks(self, xyz, known=None):
        """fs_upload_world_landmarks: the ground-truth cloud [m_world][3] behind the staged one; known [m_world] marks landmarks
        discovered from the start.  Afterwards the staged cloud is the known set.  xyz None releases the world cloud and leaves
        the staged cloud alone."""
        if xyz is None:
            self._check(self._L.fs_upload_world_landmarks(self._h, None, 0, None))
            return
        lm = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        m = lm.shape[0]
        kn = None
        if known is not None:
            kn = np.ascontiguousarray(np.asarray(known).reshape(-1) != 0, dtype=np.uint8)
            if kn.shape[0] != m:
                raise ValueError("known must hold one entry per world landmark")
        buf = lm if m > 0 else np.zeros((1, 3), dtype=np.float32)        # (an empty world is xyz != NULL with m_world == 0)
        self._check(self._L.fs_upload_world_landmarks(self._h, _p(buf), m, _p(kn) if m > 0 else None))

    def drive_slam(self, poses, goals, first_ray=None, sensor=None, lm_sensor=None, block=(253, 254), stop_when_mapped=True, threshold=550.0,
                   gate=True, gate_first_station=1):
        """fs_drive_slam: drive() whose stations are poses ([n_r][7], xyz + quaternion xyzw) and which, at every
        station, sweeps the world landmarks (lm_sensor: as sense_landmarks()'s `sensor`) and scores the pose's Fisher information
        against what has been discovered so far; with `gate`, a robot at a station >= gate_first_station whose information is not
        above `threshold` stops there, FS_DRIVE_UNSAFE.  Returns drive()'s dict plus information, voxels and in_view (lists of
        [n_r] arrays; 0, 0 and -1 for stations never reached), n_new and n_discovered."""
        st = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 7) for a in poses]
        R = len(st)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        if g.shape[0] != R:
            raise ValueError("goals must hold one entry per robot")
        ns = np.array([a.shape[0] for a in st], dtype=np.int32)
        T = int(ns.sum())
        p7 = np.ascontiguousarray(np.concatenate(st, axis=0)) if R else np.zeros((0, 7))
        fr = None
        if first_ray is not None:
            if len(first_ray) != R:
                raise ValueError("first_ray must hold one array per robot")
            parts = [np.asarray(f, dtype=np.int32).reshape(-1) for f in first_ray]
            if any(f.shape[0] != n for f, n in zip(parts, ns)):
                raise ValueError("first_ray must hold one entry per station")
            fr = np.ascontiguousarray(np.concatenate(parts)) if R else np.zeros(0, dtype=np.int32)
        sp = None if sensor is None else _ray_params_c(**sensor)
        lp = _landmark_sensor_c(lm_sensor)
        dp = DriveSlamParamsC(int(block[0]), int(block[1]), 1 if stop_when_mapped else 0, int(gate), float(threshold), int(gate_first_station))
        status = np.zeros(R, dtype=np.int32); reached = np.zeros(R, dtype=np.int32)
        sst = np.zeros(T, dtype=np.int32); seen = np.zeros(T, dtype=np.int32)
        info = np.zeros(T, dtype=np.float32); vox = np.zeros(T, dtype=np.int32); inv = np.zeros(T, dtype=np.int32)
        n_seen, n_rev = C.c_int64(), C.c_int64()
        n_new, n_disc = C.c_int32(), C.c_int32()
        win = np.zeros(6, dtype=np.int32)
        self._check(self._L.fs_drive_slam(self._h, R, _p(p7), _p(ns), _p(fr), _p(g), None if sp is None else C.byref(sp),
                                          None if lp is None else C.byref(lp), C.byref(dp), _p(status), _p(reached), _p(sst), _p(seen),
                                          _p(info), _p(vox), _p(inv), C.byref(n_seen), C.byref(n_rev), _p(win), C.byref(n_new), C.byref(n_disc)))
        cut = np.cumsum(ns)[:-1] if R else []
        split = lambda a: np.split(a, cut) if R else []
        return dict(status=status, reached=reached, station_status=split(sst), seen_unknown=split(seen), n_seen=n_seen.value,
                    n_revealed=n_rev.value, window=tuple(int(v) for v in win), information=split(info), voxels=split(vox),
                    in_view=split(inv), n_new=n_new.value, n_discovered=n_disc.value)

    def sense_landmarks(self, pose7, sensor=None):
        """fs_sense_landmarks: one sweep of the world cloud from each of pose7 [n][7]; what the poses see is counted, what reaches
        min_views sightings is discovered, and the staged cloud becomes the discovered set on the device.  sensor: None (the
        context's volume and occlusion settings) or a dict with max_dist, max_angle and optionally line_of_sight (default 1),
        min_views (1), occ ((254, 254)), end_margin_m (0.3).  Returns a dict: n_in_view [n], n_new, n_discovered."""
        ps = np.ascontiguousarray(pose7, dtype=np.float64).reshape(-1, 7)
        n = ps.shape[0]
        sp = _landmark_sensor_c(sensor)
        niv = np.zeros(n, dtype=np.int32)
        n_new, n_disc = C.c_int32(), C.c_int32()
        self._check(self._L.fs_sense_landmarks(self._h, n, _p(ps), None if sp is None else C.byref(sp), _p(niv), C.byref(n_new),
                                               C.byref(n_disc)))
        return dict(n_in_view=niv, n_new=n_new.value, n_discovered=n_disc.value)

    def world_landmarks(self, views=True):
        """fs_world_landmarks_get: a dict with m_world, n_discovered, world_index [n_discovered] (ascending; entry r is the landmark
        landmarks_in_view calls r while the staged cloud is the discovered set) and views [m_world] (None with views=False)."""
        m, nd = C.c_int32(), C.c_int32()
        self._check(self._L.fs_world_landmarks_get(self._h, C.byref(m), C.byref(nd), None, None))
        idx = np.zeros(nd.value, dtype=np.int32)
        v = np.zeros(m.value, dtype=np.int32) if views else None
        self._check(self._L.fs_world_landmarks_get(self._h, C.byref(m), C.byref(nd), _p(idx) if nd.value > 0 else None,
                                                   _p(v) if views and m.value > 0 else None))
        return dict(m_world=m.value, n_discovered=nd.value, world_index=idx, views=v)

    def information_frontier_pair(self, est_pose7, triangles_xy):
        ps = np.ascontiguousarray(est_pose7, dtype=np.float64).reshape(-1, 7)
        tr = np.ascontiguousarray(triangles_xy, dtype=np.float64).reshape(-1, 6)
        out = np.zeros(ps.shape[0], dtype=np.float32)
        self._check(self._L.fs_information_frontier_pair(self._h, ps.shape[0], _p(ps), _p(tr), _p(out)))
        return out

    # -- key-frame pose information (computeInformationForPose)
    def upload_keyframes(self, kf_pose7, kf_offsets, points_xyz):
        kf = np.ascontiguousarray(kf_pose7, dtype=np.float64).reshape(-1, 7)
        off = np.ascontiguousarray(kf_offsets, dtype=np.int32)
        pts = np.ascontiguousarray(points_xyz, dtype=np.float32).reshape(-1, 3)
        if off.shape[0] != kf.shape[0] + 1 or (off.shape[0] and off[-1] != pts.shape[0]):
            raise ValueError("kf_offsets must have n_keyframes + 1 entries ending at the number of points")
        self._check(self._L.fs_upload_keyframes(self._h, kf.shape[0], _p(kf), _p(off), _p(pts)))

    def information_for_pose(self, pose7, max_depth=2.0, hfov=1.089, max_depth_error=0.5, q_diag=0.01, radius=4.5):
        ps = np.ascontiguousarray(pose7, dtype=np.float64).reshape(-1, 7)
        n = ps.shape[0]
        prm = KeyframeParamsC(float(max_depth), float(hfov), float(max_depth_error), float(np.float32(q_diag)), float(radius))
        info = np.zeros(n, dtype=np.float32)
        cells = np.zeros(n, dtype=np.int32)
        pts = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_information_for_pose(self._h, n, _p(ps), C.byref(prm), _p(info), _p(cells), _p(pts)))
        return dict(information=info, n_cells=cells, n_points=pts)

    # -- fused
    def score_candidates(self, goal_xyz, frontier_size=None, blacklisted=None, achievable_in=None) -> np.ndarray:
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        self._check(self._L.fs_score_candidates(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(rec)))
        return rec

    def score_candidates_dev(self, n, d_goal, d_fsize, d_black, d_achin, d_records):
        """Device-pointer form (ints from tensor.data_ptr()); asynchronous on the context's stream."""
        vp = C.c_void_p
        self._check(self._L.fs_score_candidates_dev(self._h, int(n), vp(d_goal), vp(d_fsize) if d_fsize else None,
                                                    vp(d_black) if d_black else None,
                                                    vp(d_achin) if d_achin else None, vp(d_records)))

    def rank_candidates(self, records, path_length, path_heading, blacklisted=None,
                        alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5):
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        n = rec.shape[0]
        pl = np.ascontiguousarray(path_length, dtype=np.float64)
        ph = np.ascontiguousarray(path_heading, dtype=np.float64)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        cost = np.zeros(n); au = np.zeros(n); du = np.zeros(n); order = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_rank_candidates(self._h, n, _p(rec), _p(bl), _p(pl), _p(ph), alpha, beta, max_vx, max_wz,
                                               _p(cost), _p(au), _p(du), _p(order)))
        return dict(weighted_cost=cost, arrival_utility=au, distance_utility=du, order=order)

    def get_frontier_costs(self, goal_xyz, path_length, path_heading, frontier_size=None, blacklisted=None, achievable_in=None,
                           with_fim=False, alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5):
        """CostAssigner::getFrontierCosts as one call: arrival information (+ Fisher information) + U1 costs + order."""
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        pl = np.ascontiguousarray(path_length, dtype=np.float64)
        ph = np.ascontiguousarray(path_heading, dtype=np.float64)
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        cost = np.zeros(n); au = np.zeros(n); du = np.zeros(n); order = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_get_frontier_costs(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(pl), _p(ph), alpha, beta, max_vx, max_wz,
                                                  1 if with_fim else 0, _p(rec), _p(cost), _p(au), _p(du), _p(order)))
        return dict(records=rec, weighted_cost=cost, arrival_utility=au, distance_utility=du, order=order)

    def rank_candidates_dev(self, n, d_records, d_path_length, d_path_heading, d_cost, d_au=0, d_du=0, d_order=0, d_black=0,
                            d_err=0, alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5):
        """Device-pointer form (ints from tensor.data_ptr()); asynchronous on the context's stream."""
        vp = C.c_void_p
        o = lambda p: vp(p) if p else None
        self._check(self._L.fs_rank_candidates_dev(self._h, int(n), vp(d_records), o(d_black), vp(d_path_length), vp(d_path_heading),
                                                   alpha, beta, max_vx, max_wz, vp(d_cost), o(d_au), o(d_du), o(d_order), o(d_err)))

    # -- grid planner (the path columns)
    def set_grid_search(self, name: str):
        """How plan_paths, plan_paths_information, get_frontier_costs_planned and get_frontier_costs_searched plan on the grid
        (fs_set_grid_search): "converged" (a fresh context's: one converged field per robot cell) or "reference" (the reference's
        per-frontier A* wave, one per distinct goal cell, bit for bit)."""
        self._set_mode("_grid_search", name)

    def navfn_wave_potential(self, robot_pose7, goal_xyz, allow_unknown=False):
        """(field, limit): the field of ONE wave of the "reference" grid search, float32 [ny][nx] — the reference's potarr after
        calcNavFnAstar from the robot cell, stopped at the goal's cell — and its limit bits (1: the cycle budget ran out, 2: a push was
        dropped at the buffer cap).  Works whatever the grid search is."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        g = np.asarray(goal_xyz, dtype=np.float64).reshape(-1)
        goal = (C.c_double * 3)(float(g[0]), float(g[1]), float(g[2]) if g.shape[0] > 2 else 0.0)
        if self._grid_shape is None:
            raise FsError(FS_E_STATE, "no grid staged through this scorer (upload_grid / upload_grid_bricks)")
        nz, ny, nx = self._grid_shape
        if nz != 1:
            raise FsError(FS_E_INVALID, "the grid planner is defined on a 2-D costmap (nz == 1)")
        pot = np.zeros((ny, nx), dtype=np.float32)
        limit = C.c_int32()
        self._check(self._L.fs_navfn_wave_potential(self._h, C.byref(pose), 1 if allow_unknown else 0, C.byref(goal), _p(pot), C.byref(limit)))
        return pot, limit.value

    def plan_paths(self, robot_pose7, goal_xyz, achievable_in=None, allow_unknown=False, search=None):
        """setPlanForFrontier ("A*PlannerDistance") for every goal, by the context's grid search (set_grid_search; search=
        "converged" / "reference" for this call only): one potential field from the robot and a descent per goal, or the reference's
        wave per distinct goal cell and the descent on it."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8).reshape(-1)
        if ai is not None and ai.shape[0] != n:
            raise ValueError(f"achievable_in has {ai.shape[0]} entries for {n} goals")
        pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
        ach = np.zeros(n, dtype=np.uint8)
        with self._mode_for_call("_grid_search", search):
            self._check(self._L.fs_plan_paths(self._h, C.byref(pose), 1 if allow_unknown else 0, n, _p(goal), _p(ai), _p(pl), _p(plm), _p(ph), _p(ach)))
        return dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach)

    def plan_paths_information(self, robot_pose7, goal_xyz, achievable_in=None, allow_unknown=False, sample_distance=1.5, lookahead=10,
                               fi_threshold=550.0, want_waypoints=False, search=None):
        """plan_paths (search= as plan_paths'), and the Fisher information along every planned path: setPlanForFrontier's way points (one once more than
        int(sample_distance / resolution) path points have gone by, looking `lookahead` points ahead), isPoseSafe's scalar at each.
        Per frontier: n_waypoints, info_mean, info_min, first_unsafe (-1: every way point is above fi_threshold).
        want_waypoints: also waypoint_offset [n + 1], waypoint_pose7 [total][7] and waypoint_info [total], in list order."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8).reshape(-1)
        if ai is not None and ai.shape[0] != n:
            raise ValueError(f"achievable_in has {ai.shape[0]} entries for {n} goals")
        prm = PathInfoParamsC(float(sample_distance), int(lookahead), float(fi_threshold))
        pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
        ach = np.zeros(n, dtype=np.uint8)
        nwp = np.zeros(n, dtype=np.int32)
        mean = np.zeros(n)
        mn = np.zeros(n, dtype=np.float32)
        unsafe = np.zeros(n, dtype=np.int32)
        out = dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach, n_waypoints=nwp, info_mean=mean, info_min=mn,
                   first_unsafe=unsafe)

        def call(room, total, off, poses, info):
            return self._L.fs_plan_paths_information(self._h, C.byref(pose), 1 if allow_unknown else 0, n, _p(goal), _p(ai), C.byref(prm),
                                                     _p(pl), _p(plm), _p(ph), _p(ach), _p(nwp), _p(mean), _p(mn), _p(unsafe), room,
                                                     total, _p(off), _p(poses), _p(info))
        with self._mode_for_call("_grid_search", search):
            return self._plan_paths_information_call(call, out, n, want_waypoints)

    def _plan_paths_information_call(self, call, out, n, want_waypoints):
        if not want_waypoints:
            self._check(call(0, None, None, None, None))
            return out
        # the room of the first try: the default sampling leaves a way point per 1.5 m; a longer list costs a second call
        total = C.c_int64()
        off = np.zeros(n + 1, dtype=np.int32)
        room = 64 * n + 64
        for _ in range(2):
            poses = np.zeros((room, 7))
            info = np.zeros(room, dtype=np.float32)
            rc = call(room, C.byref(total), off, poses, info)
            if rc != FS_E_RANGE or total.value <= room:
                break
            room = total.value
        self._check(rc)
        out.update(waypoint_offset=off, waypoint_pose7=poses[:total.value], waypoint_info=info[:total.value])
        return out

    def navfn_potential(self, robot_pose7, allow_unknown=False) -> np.ndarray:
        """The potential field plan_paths descends, float32 [ny][nx] of the grid this scorer staged."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        if self._grid_shape is None:
            raise FsError(FS_E_STATE, "no grid staged through this scorer (upload_grid / upload_grid_bricks)")
        nz, ny, nx = self._grid_shape
        if nz != 1:
            raise FsError(FS_E_INVALID, "the grid planner is defined on a 2-D costmap (nz == 1)")
        pot = np.zeros((ny, nx), dtype=np.float32)
        self._check(self._L.fs_navfn_potential(self._h, C.byref(pose), 1 if allow_unknown else 0, _p(pot)))
        return pot

    def get_frontier_costs_planned(self, robot_pose7, goal_xyz, frontier_size=None, blacklisted=None, allow_unknown=False,
                                   with_fim=False, alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5, search=None):
        """get_frontier_costs with the path columns planned on the device in the same call (plan -> score -> rank); search= as
        plan_paths'."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        cost = np.zeros(n); au = np.zeros(n); du = np.zeros(n); order = np.zeros(n, dtype=np.int32); plm = np.zeros(n)
        with self._mode_for_call("_grid_search", search):
            self._check(self._L.fs_get_frontier_costs_planned(self._h, C.byref(pose), 1 if allow_unknown else 0, n, _p(goal), _p(fs), _p(bl),
                                                              alpha, beta, max_vx, max_wz, 1 if with_fim else 0, _p(rec), _p(cost), _p(au), _p(du),
                                                              _p(order), _p(plm)))
        return dict(records=rec, weighted_cost=cost, arrival_utility=au, distance_utility=du, order=order, path_length_m=plm)

    # -- frontier roadmap (the reference's default planner, "RoadmapPlannerDistance")
    def set_roadmap_params(self, grid_cell_size=1.0, radius_to_decide_edges=6.1, min_distance_between_two_frontier_nodes=0.25,
                           min_distance_between_robot_pose_and_node=0.25):
        """FrontierRoadMap's parameters; a new set starts an empty roadmap."""
        self._check(self._L.fs_set_roadmap_params(self._h, float(grid_cell_size), float(radius_to_decide_edges),
                                                  float(min_distance_between_two_frontier_nodes), float(min_distance_between_robot_pose_and_node)))

    def roadmap_add_nodes(self, xy, is_robot_pose=False):
        """populateNodes: addNodes (frontier goal points) or addRobotPoseAsNode.  xy [n][2] (extra columns ignored)."""
        p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, np.asarray(xy).shape[-1])[:, :2])
        self._check(self._L.fs_roadmap_add_nodes(self._h, p.shape[0], _p(p), 1 if is_robot_pose else 0))

    def roadmap_rebuild(self):
        """reConstructGraph(entireGraph = true) on the staged 2-D grid, on the device."""
        self._check(self._L.fs_roadmap_rebuild(self._h))

    def roadmap_connect(self, xy):
        """constructNewEdges for the points xy [n][2] (append the robot pose for constructNewEdgeRobotPose)."""
        p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, np.asarray(xy).shape[-1])[:, :2])
        self._check(self._L.fs_roadmap_connect(self._h, p.shape[0], _p(p)))

    def roadmap_update(self, frontier_xy, robot_xy, add_robot_pose=True):
        """UpdateRoadmapBT in one call, decided on the device (fs_roadmap_update): addNodes(frontier_xy), addRobotPoseAsNode(robot_xy) if
        add_robot_pose, constructNewEdges(frontier_xy), constructNewEdgeRobotPose(robot_xy).  Returns dict(n_nodes_added, robot_added,
        n_edges_added, n_walks).  A cell overfilled raises FsError(FS_E_RANGE) with the nodes up to the tripping one added."""
        p = np.ascontiguousarray(np.asarray(frontier_xy, dtype=np.float64).reshape(-1, 2))
        r = (C.c_double * 2)(*[float(v) for v in np.asarray(robot_xy, dtype=np.float64).reshape(-1)[:2]])
        a, b, e = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._L.fs_roadmap_update(self._h, p.shape[0], _p(p), C.byref(r), 1 if add_robot_pose else 0, C.byref(a), C.byref(b),
                                              C.byref(e)))
        return dict(n_nodes_added=a.value, robot_added=bool(b.value), n_edges_added=e.value, n_walks=self.get_counter(1033))

    def roadmap_graph(self):
        """dict(xy [n][2], key [n], row_ptr [n + 1], col [n_edges]) of the roadmap as the context holds it."""
        n, e = C.c_int32(), C.c_int64()
        self._check(self._L.fs_roadmap_get_graph(self._h, C.byref(n), C.byref(e), None, None, None, None))
        xy = np.zeros((n.value, 2)); key = np.zeros(n.value, np.uint8)
        row = np.zeros(n.value + 1, np.int32); col = np.zeros(e.value, np.int32)
        self._check(self._L.fs_roadmap_get_graph(self._h, C.byref(n), C.byref(e), _p(xy), _p(key), _p(row), _p(col)))
        return dict(xy=xy, key=key, row_ptr=row, col=col)

    def roadmap_set_keyframes(self, kf_id, pose7):
        """mapDataCallback for one map message: kf_id [n], pose7 [n][7] (x y z qx qy qz qw).  Anchors every pending node; returns
        (n_anchored, n_orphaned)."""
        ids = np.ascontiguousarray(np.asarray(kf_id, dtype=np.int32).reshape(-1))
        poses = np.ascontiguousarray(np.asarray(pose7, dtype=np.float64).reshape(-1, 7))
        if poses.shape[0] != ids.shape[0]:
            raise ValueError("one pose per key-frame id")
        a, o = C.c_int32(), C.c_int32()
        self._check(self._L.fs_roadmap_set_keyframes(self._h, ids.shape[0], _p(ids), _p(poses), C.byref(a), C.byref(o)))
        return a.value, o.value

    def roadmap_optimize(self):
        """reConstructGraph(entireGraph = true, optimizeRoadmap = true): re-place every anchor, de-duplicate, rebuild the edges."""
        self._check(self._L.fs_roadmap_optimize(self._h))

    def roadmap_anchors(self):
        """dict(n_pending, kf_id [n_records], point_c [n_records][3] float32): keyframe_mapping_ in the order roadmap_optimize
        consumes it."""
        k, r = C.c_int32(), C.c_int64()
        self._check(self._L.fs_roadmap_get_anchors(self._h, C.byref(k), C.byref(r), None, None))
        ids = np.zeros(r.value, np.int32); pts = np.zeros((r.value, 3), np.float32)
        self._check(self._L.fs_roadmap_get_anchors(self._h, C.byref(k), C.byref(r), _p(ids), _p(pts)))
        return dict(n_pending=k.value, kf_id=ids, point_c=pts)

    def set_roadmap_search(self, name: str):
        """How roadmap_plan, get_frontier_costs_roadmap and roadmap_next_goal's pair lengths search the roadmap
        (fs_set_roadmap_search): "tree" (a fresh context's: one shortest-path tree per start node) or "reference" (the reference's
        per-goal A*, bit for bit)."""
        self._set_mode("_roadmap_search", name)

    def roadmap_plan(self, robot_pose7, goal_xyz, achievable_in=None, search=None):
        """setPlanForFrontierRoadmap for every goal, by the context's roadmap search (set_roadmap_search; search= "tree" /
        "reference" for this call only): one shortest-path tree from the robot's closest key node, or the reference's A* per goal
        node."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8).reshape(-1)
        if ai is not None and ai.shape[0] != n:
            raise ValueError(f"achievable_in has {ai.shape[0]} entries for {n} goals")
        pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
        ach = np.zeros(n, dtype=np.uint8)
        with self._mode_for_call("_roadmap_search", search):
            self._check(self._L.fs_roadmap_plan(self._h, C.byref(pose), n, _p(goal), _p(ai), _p(pl), _p(plm), _p(ph), _p(ach)))
        return dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach)

    def roadmap_routes(self, robot_pose7, goal_xyz, achievable_in=None, refine=True, with_information=True, fi_threshold=550.0,
                       want_nodes=False, want_legs=False, search=None):
        """roadmap_plan, and the routes behind its numbers (fs_roadmap_routes): one route per distinct goal node the plan reached —
        getPlan's node list, refinePath's shortcut of it on the staged grid (refine) and the Fisher information of the legs of
        the refined (or raw) list (with_information).  Per frontier: roadmap_plan's columns and route_of; per route: goal_node,
        complete, n_legs and, with_information, info_mean, info_min, first_unsafe.  want_nodes: node_offset / node and, with refine,
        refined_offset / refined_node (CSR).  want_legs: leg_pose7 [legs][7] and leg_info [legs], route by route."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8).reshape(-1)
        if ai is not None and ai.shape[0] != n:
            raise ValueError(f"achievable_in has {ai.shape[0]} entries for {n} goals")
        prm = RouteParamsC(1 if refine else 0, 1 if with_information else 0, float(fi_threshold))
        pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
        ach = np.zeros(n, dtype=np.uint8)
        route_of = np.zeros(n, dtype=np.int32)
        n_routes, total, total_ref = C.c_int32(), C.c_int64(), C.c_int64()
        dump = want_nodes or want_legs
        room_r, room_n = max(n, 1), (64 * n + 64) if dump else 0
        with self._mode_for_call("_roadmap_search", search):
            for _ in range(2):
                gn, nl = np.zeros(room_r, dtype=np.int32), np.zeros(room_r, dtype=np.int32)
                comp = np.zeros(room_r, dtype=np.uint8)
                mean = np.zeros(room_r) if with_information else None
                mn = np.zeros(room_r, dtype=np.float32) if with_information else None
                unsafe = np.zeros(room_r, dtype=np.int32) if with_information else None
                off = np.zeros(room_r + 1, dtype=np.int64) if dump else None
                nodes = np.zeros(max(room_n, 1), dtype=np.int32) if dump else None
                ref = want_nodes and refine
                roff = np.zeros(room_r + 1, dtype=np.int64) if ref else None
                rnodes = np.zeros(max(room_n, 1), dtype=np.int32) if ref else None
                p7 = np.zeros((max(room_n, 1), 7)) if want_legs else None
                li = np.zeros(max(room_n, 1), dtype=np.float32) if want_legs else None
                rc = self._L.fs_roadmap_routes(self._h, C.byref(pose), n, _p(goal), _p(ai), C.byref(prm), _p(pl), _p(plm), _p(ph), _p(ach),
                                               _p(route_of), room_r, C.byref(n_routes), _p(gn), _p(comp), _p(nl), _p(mean), _p(mn),
                                               _p(unsafe), room_n, C.byref(total) if dump else None, _p(off), _p(nodes),
                                               C.byref(total_ref) if ref else None, _p(roff), _p(rnodes), _p(p7), _p(li))
                if rc != FS_E_RANGE or (n_routes.value <= room_r and total.value <= room_n):
                    break
                room_r, room_n = max(n_routes.value, 1), total.value
        self._check(rc)
        k = n_routes.value
        out = dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach, route_of=route_of, goal_node=gn[:k],
                   complete=comp[:k], n_legs=nl[:k])
        if with_information:
            out.update(info_mean=mean[:k], info_min=mn[:k], first_unsafe=unsafe[:k])
        if want_nodes:
            out.update(node_offset=off[:k + 1], node=nodes[:total.value])
            if refine:
                out.update(refined_offset=roff[:k + 1], refined_node=rnodes[:total_ref.value])
        if want_legs:
            legs = int(nl[:k].sum())
            out.update(leg_pose7=p7[:legs], leg_info=li[:legs])
        return out

    def get_frontier_costs_roadmap(self, robot_pose7, goal_xyz, frontier_size=None, blacklisted=None, with_fim=False,
                                   alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5, search=None):
        """get_frontier_costs with the path columns planned on the roadmap in the same call (plan -> score -> rank); search= as
        roadmap_plan's."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        cost = np.zeros(n); au = np.zeros(n); du = np.zeros(n); order = np.zeros(n, dtype=np.int32); plm = np.zeros(n)
        with self._mode_for_call("_roadmap_search", search):
            self._check(self._L.fs_get_frontier_costs_roadmap(self._h, C.byref(pose), n, _p(goal), _p(fs), _p(bl), alpha, beta, max_vx,
                                                              max_wz, 1 if with_fim else 0, _p(rec), _p(cost), _p(au), _p(du), _p(order),
                                                              _p(plm)))
        return dict(records=rec, weighted_cost=cost, arrival_utility=au, distance_utility=du, order=order, path_length_m=plm)

    def allocate_tasks(self, cost, distance=None, method="hungarian", want_rank=False):
        """The reference's TaskAllocator on cost [R][n] (robot-major, as addRobotTasks pushes the rows): "hungarian"
        (solveAllocationHungarian) or "minpos" (solveAllocationMinPos, which needs distance [R][n]), bit for bit.
        dict(assignment [R] (-1: none), total_cost), plus rank [R][n] (MinPos' P) and modified_cost [R][n] with want_rank under
        "minpos"."""
        if method not in ALLOC_METHODS:
            raise FsError(FS_E_INVALID, f"unknown allocation method {method!r} (hungarian | minpos)")
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        if cost.ndim != 2:
            raise ValueError("cost must be [robots][tasks]")
        R, n = cost.shape
        dist = None if distance is None else np.ascontiguousarray(distance, dtype=np.float64)
        if dist is not None and dist.shape != cost.shape:
            raise ValueError(f"distance is {dist.shape}, cost {cost.shape}")
        assignment = np.full(R, -2, dtype=np.int32)
        total = C.c_double(float("nan"))
        wanted = want_rank and method == "minpos"
        rank = np.zeros((R, n), dtype=np.int32) if wanted else None
        mod = np.zeros((R, n)) if wanted else None
        self._check(self._L.fs_allocate_tasks(self._h, R, n, _p(cost), _p(dist), ALLOC_METHODS[method], _p(assignment), C.byref(total),
                                              _p(rank), _p(mod)))
        out = dict(assignment=assignment, total_cost=total.value)
        if wanted:
            out.update(rank=rank, modified_cost=mod)
        return out

    def allocate_tasks_dev(self, n_robots, n_tasks, d_cost, d_distance, method, d_assignment, d_total_cost, d_status, d_rank=0,
                           d_modified_cost=0):
        """allocate_tasks on device pointers (integers), enqueued on the context's stream and not waited for; d_status [1] int32."""
        self._check(self._L.fs_allocate_tasks_dev(self._h, int(n_robots), int(n_tasks), C.c_void_p(d_cost), C.c_void_p(d_distance or None),
                                                  ALLOC_METHODS[method], C.c_void_p(d_assignment), C.c_void_p(d_total_cost),
                                                  C.c_void_p(d_rank or None), C.c_void_p(d_modified_cost or None), C.c_void_p(d_status)))

    def fleet_allocate_roadmap(self, robot_poses, goal_xyz, frontier_size=None, blacklisted=None, method="hungarian", search=None,
                               want_matrix=False, want_records=False, alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5):
        """One tick of a fleet on the shared map: every robot's get_frontier_costs_roadmap rows (robot_poses [R][7]) built on the
        device — arrival information once, a tree per distinct start node, one plan launch — and allocate_tasks on them with
        distance = path_length_m.  dict(assignment [R], total_cost, assigned_cost [R] (DBL_MAX: a dead frontier, NaN for -1)), plus
        weighted_cost, path_length_m, achievable [R][n] with want_matrix and records [n] (scored with achievable_in = all) with
        want_records.  search= as roadmap_plan's."""
        if method not in ALLOC_METHODS:
            raise FsError(FS_E_INVALID, f"unknown allocation method {method!r} (hungarian | minpos)")
        poses = np.ascontiguousarray(robot_poses, dtype=np.float64).reshape(-1, 7)
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        R, n = poses.shape[0], goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32).reshape(-1)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8).reshape(-1)
        for name, a in (("frontier_size", fs), ("blacklisted", bl)):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"{name} has {a.shape[0]} entries for {n} goals")
        assignment = np.full(R, -2, dtype=np.int32)
        total = C.c_double(float("nan"))
        assigned = np.zeros(R)
        rec = np.zeros(n, dtype=RECORD_DTYPE) if want_records else None
        cost = np.zeros((R, n)) if want_matrix else None
        plm = np.zeros((R, n)) if want_matrix else None
        ach = np.zeros((R, n), dtype=np.uint8) if want_matrix else None
        with self._mode_for_call("_roadmap_search", search):
            self._check(self._L.fs_fleet_allocate_roadmap(self._h, R, _p(poses), n, _p(goal), _p(fs), _p(bl), alpha, beta, max_vx, max_wz,
                                                          ALLOC_METHODS[method], _p(assignment), C.byref(total), _p(assigned), _p(rec),
                                                          _p(cost), _p(plm), _p(ach)))
        out = dict(assignment=assignment, total_cost=total.value, assigned_cost=assigned)
        if want_matrix:
            out.update(weighted_cost=cost, path_length_m=plm, achievable=ach)
        if want_records:
            out["records"] = rec
        return out

    def roadmap_next_goal(self, robot_pose7, goal_xyz, path_length_m, achievable, blacklisted=None, blacklist_xy=None,
                          n_local=5, local_radius=12.0, fi_pose7=None, fi_threshold=550.0, want_matrix=False, want_selection=False,
                          search=None):
        """FullPathOptimizer::getNextGoal on the staged roadmap: the selection, the pair matrix over [robot, locals, closest global]
        and the exhaustive tour search over the locals.  dict(next_index (-1: the zero frontier), status (0 SAFE, 1 UNSAFE,
        2 UNDETERMINED), tour (input indices: the locals in visiting order, then the closest global), tour_length, n_tied, n_locals),
        plus selection [n] (1 local, 2 global, | 4 closest global) with want_selection and pair_length_m [(k + 2)][(k + 2)] (None
        without locals) with want_matrix.  fi_pose7 None: no Fisher-information check.  The pair lengths by the context's roadmap
        search; search= as roadmap_plan's."""
        pose = (C.c_double * 7)(*[float(v) for v in np.asarray(robot_pose7, dtype=np.float64).reshape(7)])
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        plm = np.ascontiguousarray(path_length_m, dtype=np.float64).reshape(-1)
        ach = np.ascontiguousarray(achievable, dtype=np.uint8).reshape(-1)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8).reshape(-1)
        for name, a in (("path_length_m", plm), ("achievable", ach), ("blacklisted", bl)):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"{name} has {a.shape[0]} entries for {n} goals")
        circ = np.zeros((0, 2)) if blacklist_xy is None else np.ascontiguousarray(np.asarray(blacklist_xy, dtype=np.float64).reshape(-1, 2))
        fi = None if fi_pose7 is None else np.ascontiguousarray(fi_pose7, dtype=np.float64).reshape(7)
        nl = int(n_local)
        room = max(nl, 0) + 2
        nxt, st, tsz = C.c_int32(), C.c_int32(), C.c_int32()
        tl, nt = C.c_double(), C.c_int64()
        tour = np.zeros(max(nl, 0) + 1, dtype=np.int32)
        sel = np.zeros(n, dtype=np.uint8)
        mat = np.zeros(room * room) if want_matrix else None
        with self._mode_for_call("_roadmap_search", search):
            self._check(self._L.fs_roadmap_next_goal(self._h, C.byref(pose), n, _p(goal), _p(plm), _p(ach), _p(bl), circ.shape[0],
                                                     _p(circ) if circ.shape[0] else None, nl, float(local_radius), _p(fi),
                                                     float(fi_threshold), C.byref(nxt), C.byref(st), _p(tour), C.byref(tsz), C.byref(tl),
                                                     C.byref(nt), _p(sel), _p(mat)))
        k = int(np.count_nonzero((sel & 3) == 1))
        out = dict(next_index=nxt.value, status=st.value, tour=tour[:tsz.value].copy(), tour_length=tl.value, n_tied=nt.value,
                   n_locals=k)
        if want_selection:
            out["selection"] = sel
        if want_matrix:
            out["pair_length_m"] = mat[:(k + 2) * (k + 2)].reshape(k + 2, k + 2).copy() if k else None
        return out

    # -- leg refinement (computePathBetweenPointsThetaStar: the path the robot drives)
    def set_refine_search(self, name: str):
        """How refine_paths and refine_tour plan a leg (fs_set_refine_search): "field" (a fresh context's: a converged cost field per
        start cell, a descent, Theta*'s parent rule along it) or "reference" (the reference's own Theta* search, one wavefront per
        distinct leg: its status — 5 also where its loop drops the entry popped last —, vertices and poses bit for bit)."""
        self._set_mode("_refine_search", name)

    def refine_paths(self, starts, goals, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8, search=None):
        """computePathBetweenPointsThetaStar for every leg starts[i] -> goals[i] ([n][2] world; extra columns ignored), by the
        context's refine search (set_refine_search; search= "field" / "reference" for this call only): one cost field per distinct
        start cell, a descent and Theta*'s parent rule per leg, or the reference's own search per distinct leg.  dict(status [n]
        (0 path, 1 start off the map, 2 goal off the map, 3 start unsafe, 4 goal unsafe, 5 no path), cost [n], vertices (a [V][2]
        array per leg, start first), poses (a [N][2] array per leg: the interpolated path the reference publishes))."""
        def pts(a):
            a = np.asarray(a, dtype=np.float64)
            a = a.reshape(-1, a.shape[-1]) if a.ndim else a.reshape(-1, 2)
            return np.ascontiguousarray(a[:, :2])
        s, g = pts(starts), pts(goals)
        n = s.shape[0]
        if g.shape[0] != n:
            raise ValueError(f"{g.shape[0]} goals for {n} starts")
        st = np.zeros(n, dtype=np.int32); cost = np.zeros(n)
        nv = np.zeros(n, dtype=np.int32); npz = np.zeros(n, dtype=np.int32)
        args = (1 if allow_unknown else 0, float(w_euc), float(w_traversal), int(corners))
        with self._mode_for_call("_refine_search", search):
            # size first (the fields are cached, so the second call only repeats the legs; "reference" searches twice)
            self._check(self._L.fs_refine_paths(self._h, n, _p(s), _p(g), *args, _p(st), _p(cost), _p(nv), None, _p(npz), None))
            vert = np.zeros((int(nv.sum()), 2)); pose = np.zeros((int(npz.sum()), 2))
            self._check(self._L.fs_refine_paths(self._h, n, _p(s), _p(g), *args, _p(st), _p(cost), _p(nv), _p(vert), _p(npz), _p(pose)))
        vo, po = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(npz)])
        return dict(status=st, cost=cost, n_vertices=nv, n_poses=npz,
                    vertices=[vert[vo[i]:vo[i + 1]] for i in range(n)], poses=[pose[po[i]:po[i + 1]] for i in range(n)])

    def refine_field(self, start_xy, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8) -> np.ndarray:
        """The cost field refine_paths descends from start_xy, float64 [ny][nx] of the grid this scorer staged (DBL_MAX: not reached)."""
        if self._grid_shape is None:
            raise FsError(FS_E_STATE, "no grid staged through this scorer (upload_grid / upload_grid_bricks)")
        nz, ny, nx = self._grid_shape
        if nz != 1:
            raise FsError(FS_E_INVALID, "the leg refinement is defined on a 2-D costmap (nz == 1)")
        xy = np.asarray(start_xy, dtype=np.float64).reshape(-1)
        start = (C.c_double * 2)(float(xy[0]), float(xy[1]))
        out = np.zeros((ny, nx))
        self._check(self._L.fs_refine_field(self._h, C.byref(start), 1 if allow_unknown else 0, float(w_euc), float(w_traversal),
                                            int(corners), _p(out)))
        return out

    def refine_tour(self, robot_pose7, goal_xyz, tour, search=None):
        """getNextGoal's published plan for a roadmap_next_goal result: the legs robot -> goal[tour[0]] -> goal[tour[1]] -> ...,
        planned as computePathBetweenPointsThetaStar(..., true) does.  refine_paths' dict plus `path`: the poses of the legs that
        found a path, back to back (what FullPathOptimizer accumulates into its plan).  search= as refine_paths'."""
        robot = np.asarray(robot_pose7, dtype=np.float64).reshape(7)[:2]
        goal = np.asarray(goal_xyz, dtype=np.float64).reshape(-1, 3)[:, :2]
        idx = np.asarray(tour["tour"] if isinstance(tour, dict) else tour, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            return dict(status=np.zeros(0, np.int32), cost=np.zeros(0), n_vertices=np.zeros(0, np.int32), n_poses=np.zeros(0, np.int32),
                        vertices=[], poses=[], path=np.zeros((0, 2)))
        pts = np.vstack([robot[None], goal[idx]])
        out = self.refine_paths(pts[:-1], pts[1:], search=search)
        ok = [p for p, s in zip(out["poses"], out["status"]) if s == 0]
        out["path"] = np.vstack(ok) if ok else np.zeros((0, 2))
        return out

    def selftest_fp64(self, max_abs=256) -> int:
        bad = C.c_int64()
        self._check(self._L.fs_selftest_fp64(self._h, int(max_abs), C.byref(bad)))
        return bad.value


def _ray_params_c(max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, robot_radius=0.60, n_rays=0, elev=(0.0,),
                  obst=(240, 254), trace=(255, 255), factor_max=1.2, factor_min=0.70, polygon=(-1e300, -1e300, 1e300, 1e300)):
    p = RayParamsC()
    p.max_camera_depth, p.delta_theta, p.camera_fov, p.robot_radius = max_camera_depth, delta_theta, camera_fov, robot_radius
    p.n_rays, p.n_elev = int(n_rays), len(elev)
    for i, e in enumerate(elev[:FS_MAX_ELEV]):
        p.elev[i] = float(e)
    p.obst_min, p.obst_max, p.trace_min, p.trace_max = int(obst[0]), int(obst[1]), int(trace[0]), int(trace[1])
    p.factor_max, p.factor_min = factor_max, factor_min
    for i in range(4):
        p.polygon[i] = float(polygon[i])
    return p


def fan_n_yaw(delta_theta, n_rays=0):
    """Yaw rays of a fan: n_rays, or the reference's loop `theta <= 2 * pi` over the accumulated theta (DEP/src/CostCalculator.cpp:36)."""
    if n_rays > 0:
        return int(n_rays)
    import math
    n, t = 0, 0.0
    while t <= 2 * math.pi and n <= 4096:
        n += 1
        t += delta_theta
    return n


def _landmark_sensor_c(sensor):
    """a landmark sensor dict (sense_landmarks' `sensor`) as the C struct; None stays None: the context's defaults"""
    if sensor is None:
        return None
    occ = sensor.get("occ", (254, 254))
    return LandmarkSensorC(float(sensor["max_dist"]), float(sensor["max_angle"]), int(sensor.get("line_of_sight", 1)),
                           int(sensor.get("min_views", 1)), int(occ[0]), int(occ[1]), float(sensor.get("end_margin_m", 0.3)))


def first_ray_for_yaw(yaw, delta_theta, camera_fov, n_yaw):
    """The window start i in [0, n_yaw - window], window = (int)(camera_fov / delta_theta), whose pose yaw
    i * delta_theta + camera_fov / 2 (DEP/src/CostCalculator.cpp:119) is nearest to `yaw` (the first of equally near ones)."""
    window = int(camera_fov / delta_theta)
    best, best_d = 0, None
    for i in range(n_yaw - window + 1):
        d = abs((i * delta_theta) + (camera_fov / 2) - yaw)
        if best_d is None or d < best_d:
            best, best_d = i, d
    return best


def stations_along(poses_xy, spacing_m, look=10, delta_theta=0.10, camera_fov=1.04, n_rays=0, z=0.0):
    """Stations for FrontierScorer.drive from a pose list [N][2] (refine_paths' `poses`): the first pose, then every pose at which
    the way driven since the last station reaches spacing_m, and always the last pose.  Each station looks along the path: its
    first_ray is first_ray_for_yaw — for the fan of delta_theta, camera_fov, n_rays (set_ray_params' arguments and defaults) — of the
    direction from it to the pose `look` entries ahead (the last pose when there are fewer; the last station keeps the station's
    before it, a lone station gets window 0).  Host only, numpy.  Returns (stations [n][3] with z in the third column,
    first_ray [n] int32, index [n]: the pose each station is)."""
    import math
    n_yaw = fan_n_yaw(delta_theta, n_rays)
    p = np.asarray(poses_xy, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])[:, :2] if p.size else p.reshape(0, 2)
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    keep, since = [0], 0.0
    for i in range(1, n):
        since += math.hypot(p[i, 0] - p[i - 1, 0], p[i, 1] - p[i - 1, 1])
        if since >= spacing_m:
            keep.append(i)
            since = 0.0
    if keep[-1] != n - 1:
        keep.append(n - 1)
    first = np.zeros(len(keep), dtype=np.int32)
    for j, i in enumerate(keep):
        a = min(i + int(look), n - 1)
        dx, dy = p[a, 0] - p[i, 0], p[a, 1] - p[i, 1]
        if dx == 0.0 and dy == 0.0:
            first[j] = first[j - 1] if j else 0
            continue
        yaw = math.atan2(dy, dx)
        first[j] = first_ray_for_yaw(yaw if yaw >= 0.0 else yaw + 2 * math.pi, delta_theta, camera_fov, n_yaw)
    st = np.zeros((len(keep), 3))
    st[:, :2] = p[keep]
    st[:, 2] = z
    return st, first, np.asarray(keep, dtype=np.int64)


def poses_along(poses_xy, index, look=10, z=0.0):
    """Pose rows for FrontierScorer.drive_slam from a pose list [N][2] and stations_along's `index`: station j stands at pose
    index[j] and looks — a rotation about Z, quaternion xyzw — at the pose `look` entries ahead, by stations_along's direction rule
    (the last pose when there are fewer; a station with nothing ahead keeps the yaw of the station before it, a lone one looks
    along +x).  Host only, numpy.  Returns [n][7]."""
    import math
    p = np.asarray(poses_xy, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])[:, :2] if p.size else p.reshape(0, 2)
    n = p.shape[0]
    keep = np.asarray(index, dtype=np.int64).reshape(-1)
    out = np.zeros((keep.shape[0], 7))
    yaw = 0.0
    for j, i in enumerate(keep):
        a = min(int(i) + int(look), n - 1)
        dx, dy = p[a, 0] - p[i, 0], p[a, 1] - p[i, 1]
        if dx != 0.0 or dy != 0.0:
            yaw = math.atan2(dy, dx)
        out[j, :2] = p[i]
        out[j, 2] = z
        out[j, 5], out[j, 6] = math.sin(yaw / 2), math.cos(yaw / 2)
    return out


def shard_bounds(n: int, n_shards: int, shard: int):
    """fs_multi_shard_bounds: the block of `shard` — the partition rule of the multi-device scorer (needs no GPU)."""
    L = load_library()
    lo, hi = C.c_int32(), C.c_int32()
    rc = L.fs_multi_shard_bounds(int(n), int(n_shards), int(shard), C.byref(lo), C.byref(hi))
    if rc != FS_OK:
        raise FsError(rc, "fs_multi_shard_bounds: bad arguments")
    return lo.value, hi.value


class MultiScorer:
    """fs_multi: ONE process and ONE calling thread over several GPUs (or several contexts on one: repeat the ordinal).
    Staging calls are broadcast; score_candidates cuts the list into contiguous blocks, runs them side by side and returns
    the records in list order."""

    def __init__(self, devices=(0,)):
        self._L = load_library()
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._L.fs_multi_create(ids, len(devices), C.byref(h))
        if rc != FS_OK:
            raise FsError(rc, "fs_multi_create failed: no gfx950 device under one of the ordinals (no CPU fallback exists)")
        self._h = h
        self.n_devices = len(devices)

    def _check(self, rc):
        if rc != FS_OK:
            raise FsError(rc, (self._L.fs_multi_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.fs_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._check(self._L.fs_multi_set_option(self._h, key.encode(), float(value)))

    def set_ray_params(self, **kw):
        p = _ray_params_c(**kw)
        self._check(self._L.fs_multi_set_ray_params(self._h, C.byref(p)))

    def upload_grid(self, cells, origin, resolution):
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        if c.ndim == 2:
            c = c[None]
        nz, ny, nx = c.shape
        o = (C.c_double * 3)(*[float(v) for v in origin])
        self._check(self._L.fs_multi_upload_grid(self._h, _p(c), nx, ny, nz, C.byref(o), float(resolution)))
        self._grid_shape = (nz, ny, nx)
        self._grid_geom = (tuple(float(v) for v in origin), float(resolution))

    def update_grid_region(self, x0, y0, z0, window, view=False):
        ptr, sx, sy, sz, rs, ss, keep = _window_args(window, view)
        self._check(self._L.fs_multi_update_grid_region(self._h, int(x0), int(y0), int(z0), sx, sy, sz, ptr, rs, ss))

    def inflate(self, inflation_radius, inscribed_radius, cost_scaling_factor, window=None, inflate_unknown=False):
        """fs_multi_inflate: FrontierScorer.inflate on every member; the counts are member 0's."""
        if window is None:
            if getattr(self, "_grid_shape", None) is None:
                raise FsError(FS_E_STATE, "no grid staged (upload_grid)")
            window = (0, 0, self._grid_shape[2], self._grid_shape[1])
        p = _inflation_params_c(inflation_radius, inscribed_radius, cost_scaling_factor, inflate_unknown)
        seeds, changed = C.c_int64(), C.c_int64()
        self._check(self._L.fs_multi_inflate(self._h, C.byref(p), *[int(v) for v in window], C.byref(seeds), C.byref(changed)))
        return seeds.value, changed.value

    def information_layer(self, stride_cells=5, n_yaw=8, yaw0=0.0, pose_z=0.0, reduce="mean", info_lo=550.0, info_hi=1100.0, max_cost=252,
                          window=None, write=True, want_per_yaw=False):
        """fs_multi_information_layer: FrontierScorer.information_layer on every member; the result is member 0's."""
        if getattr(self, "_grid_shape", None) is None:
            raise FsError(FS_E_STATE, "no grid staged (upload_grid)")
        return _information_layer(self._L.fs_multi_information_layer, self._h, self._check, self._grid_shape, self._grid_geom, stride_cells,
                                  n_yaw, yaw0, pose_z, reduce, info_lo, info_hi, max_cost, window, write, want_per_yaw)

    def keepout_add_fov(self, wx, wy, yaw, height_m=3.5):
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_multi_keepout_add_fov(self._h, float(wx), float(wy), float(yaw), float(height_m), C.byref(zid), C.byref(n)))
        return zid.value, n.value

    def keepout_add_disc(self, wx, wy, radius_m=1.7):
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_multi_keepout_add_disc(self._h, float(wx), float(wy), float(radius_m), C.byref(zid), C.byref(n)))
        return zid.value, n.value

    def keepout_clear(self):
        self._check(self._L.fs_multi_keepout_clear(self._h))

    def mark_lethal_fov(self, robot_pose7):
        pose = (C.c_double * 7)(*[float(v) for v in robot_pose7])
        black = (C.c_double * 7)()
        zid, n = C.c_int32(), C.c_int64()
        self._check(self._L.fs_multi_mark_lethal_fov(self._h, C.byref(pose), C.byref(black), C.byref(zid), C.byref(n)))
        return np.array(black[:], dtype=np.float64), zid.value, n.value

    def upload_landmarks(self, xyz):
        lm = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._check(self._L.fs_multi_upload_landmarks(self._h, _p(lm), lm.shape[0]))

    def lookup_generate(self, bounds=None):
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float32)
        self._check(self._L.fs_multi_lookup_generate(self._h, _p(b)))

    def set_fim_params(self, max_dist=14.0, max_angle=1.0):
        p = FimParamsC(max_dist, max_angle)
        self._check(self._L.fs_multi_set_fim_params(self._h, C.byref(p)))

    def set_occlusion(self, enabled, occ=(254, 254), end_margin_m=0.3):
        """fs_multi_set_occlusion: FrontierScorer.set_occlusion on every member."""
        p = OcclusionParamsC(1 if enabled else 0, int(occ[0]), int(occ[1]), float(end_margin_m))
        self._check(self._L.fs_multi_set_occlusion(self._h, C.byref(p)))

    def get_occlusion(self):
        """member 0's settings (a broadcast keeps the members equal)"""
        p = OcclusionParamsC()
        rc = self._L.fs_get_occlusion(self.member(0), C.byref(p))
        if rc != FS_OK:
            raise FsError(rc, "fs_get_occlusion on member 0")
        return dict(enabled=bool(p.enabled), occ=(p.occ_min, p.occ_max), end_margin_m=p.end_margin_m)

    def max_arrival(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._L.fs_multi_max_arrival(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(max_value=a.value, max_gt=b.value, min_gt=c.value)

    def score_arrival(self, goal_xyz, frontier_size=None, blacklisted=None, achievable_in=None, n_rays_total=0):
        """n_rays_total = n_elev * n_yaw to get the per-ray counts back (0: not requested)."""
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rc_arr = np.zeros((n, n_rays_total), dtype=np.int32) if n_rays_total else None
        arrival = np.zeros(n, dtype=np.int32); argmax = np.zeros(n, dtype=np.int32)
        yaw = np.zeros(n, dtype=np.float64); ach = np.zeros(n, dtype=np.uint8); status = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_multi_score_arrival(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(rc_arr),
                                                   _p(arrival), _p(argmax), _p(yaw), _p(ach), _p(status)))
        return dict(ray_counts=rc_arr, arrival=arrival, argmax=argmax, yaw=yaw, achievable=ach, status=status)

    def score_candidates(self, goal_xyz, frontier_size=None, blacklisted=None, achievable_in=None) -> np.ndarray:
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        self._check(self._L.fs_multi_score_candidates(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(rec)))
        return rec


    def score_fim(self, pose7, want_fim=True, info_only=False):
        """fs_multi_score_fim: FrontierScorer.score_fim over all members, every column in list order."""
        ps = np.ascontiguousarray(pose7, dtype=np.float64).reshape(-1, 7)
        n = ps.shape[0]
        info = np.zeros(n, dtype=np.float32)
        if info_only:
            nvox = np.zeros(n, dtype=np.int32)
            self._check(self._L.fs_multi_score_fim(self._h, n, _p(ps), _p(info), None, None, None, None, _p(nvox)))
            return dict(info_ref=info, n_voxels=nvox)
        fim21 = np.zeros((n, 21), dtype=np.float32) if want_fim else None
        trace = np.zeros(n, dtype=np.float32); logdet = np.zeros(n, dtype=np.float32)
        nvis = np.zeros(n, dtype=np.int32); nvox = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_multi_score_fim(self._h, n, _p(ps), _p(info), _p(fim21), _p(trace), _p(logdet), _p(nvis), _p(nvox)))
        return dict(info_ref=info, fim21=fim21, trace=trace, logdet=logdet, n_visible=nvis, n_voxels=nvox)

    def get_frontier_costs(self, goal_xyz, path_length, path_heading, frontier_size=None, blacklisted=None, achievable_in=None,
                           with_fim=False, alpha=0.25, beta=1.0, max_vx=0.5, max_wz=0.5):
        """fs_multi_get_frontier_costs: blocks scored on their devices, gathered device to device, ranked on member 0's GPU."""
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        pl = np.ascontiguousarray(path_length, dtype=np.float64)
        ph = np.ascontiguousarray(path_heading, dtype=np.float64)
        fs = None if frontier_size is None else np.ascontiguousarray(frontier_size, dtype=np.int32)
        bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        cost = np.zeros(n); au = np.zeros(n); du = np.zeros(n); order = np.zeros(n, dtype=np.int32)
        self._check(self._L.fs_multi_get_frontier_costs(self._h, n, _p(goal), _p(fs), _p(bl), _p(ai), _p(pl), _p(ph), alpha, beta, max_vx, max_wz,
                                                        1 if with_fim else 0, _p(rec), _p(cost), _p(au), _p(du), _p(order)))
        return dict(records=rec, weighted_cost=cost, arrival_utility=au, distance_utility=du, order=order)

    def gather_mode(self) -> int:
        rc = self._L.fs_multi_gather_mode(self._h)
        if rc < 0:
            self._check(rc)
        return rc

    def last_error(self) -> str:
        return (self._L.fs_multi_last_error(self._h) or b"").decode()

    def member(self, i: int):
        """fs_multi_ctx(m, i) as a borrowed handle for fs_* calls on one member (counters, options, limits)."""
        h = self._L.fs_multi_ctx(self._h, int(i))
        if not h:
            raise FsError(FS_E_INVALID, f"no member {i}")
        return C.c_void_p(h)

    def set_arrival_limits(self, max_gt, min_gt):
        for i in range(self.n_devices):
            rc = self._L.fs_set_arrival_limits(self.member(i), float(max_gt), float(min_gt))
            if rc != FS_OK:
                raise FsError(rc, f"fs_set_arrival_limits on member {i}")


def record_status(rec):
    return (rec["flags"] >> 8) & 0xFF


def record_achievable(rec):
    return (rec["flags"] & 1).astype(np.uint8)


def record_nvoxels(rec):
    return (rec["flags"] >> 16) & 0xFFFF
