"""sea_current_amd -- Python plumbing over libsea_current_hip.so (MI355X / gfx950).

The product is the C-ABI library (include/sea_current_hip.h) and the C++ header
sea-current_amd/sea_current.hpp; this module only binds the C ABI with ctypes so that
tests/ and bench.py can drive it with torch device tensors.  There is NO CPU fallback:
if the HIP library is missing or no GPU is present, calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
NATIVE_DIR = os.path.normpath(os.path.join(_PKG, "..", ".."))          # sea-current_amd/
REPO_ROOT = os.path.normpath(os.path.join(NATIVE_DIR, ".."))
LIB_PATH = os.environ.get("SC_LIB_PATH") or os.path.join(NATIVE_DIR, "libsea_current_hip.so")   # SC_LIB_PATH: experiment builds
HEADER_PATH = os.path.join(REPO_ROOT, "include", "sea_current_hip.h")

EDT_INF = 2**31 - 1
FIELD_INF = 2**31 - 1
FIELD_SEED_COST_MAX = 1 << 24
Q_OK, Q_NO_PATH, Q_BAD_ENDPOINT, Q_TRUNCATED, Q_RING_OVERFLOW, Q_BAD_PATH = 0, 1, 2, 3, 4, 5
K_EDT_COLBITS, K_EDT_BAND, K_MOVES, K_ASTAR, K_TOPPRA, K_TOPPRA_SAMPLE, K_BEZIER, K_ARCLENGTH, K_RESAMPLE, K_OCC, K_NEAREST, K_FMT, K_GATHER = range(13)
K_WAYPOINTS = 13
K_SMOOTH = 14
SMOOTH_OK, SMOOTH_BAD_INPUT, SMOOTH_NONFINITE, SMOOTH_TOPPRA_FAILED, SMOOTH_TRUNCATED, SMOOTH_EMPTY_SEGMENT = range(6)
SMOOTH_COLLIDES = 6
CURVE_MAX_LEGS, CURVE_MAX_LEVEL = 1024, 30
TRAJ_OK, TRAJ_SKIPPED, TRAJ_BAD = range(3)
TRAJ_MAX_TICKS = 65535
SLOT_UNRESOLVED, SLOT_NOT_OK, SLOT_UNNAMED = -1, -2, -3
TP_OK, TP_NO_PATH, TP_BAD_ENDPOINT, TP_START_BLOCKED = range(4)
ASSIGN_MAX_DIM = 1024
ASSIGN_BIG = 1 << 42
ASSIGN_OK, ASSIGN_BAD = 0, 1

_lib = None


class SeaCurrentError(RuntimeError):
    pass


def build(force=False):
    """Compile libsea_current_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", NATIVE_DIR, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", NATIVE_DIR])
    return LIB_PATH


_vp, _i, _d, _i64p = C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int64)
_SIGNATURES = {
    "sc_abi_version": (C.c_int, []),
    "sc_status_string": (C.c_char_p, [_i]),
    "sc_last_error": (C.c_char_p, [_vp]),
    "sc_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "sc_ctx_destroy": (_i, [_vp]),
    "sc_ctx_set_stream": (_i, [_vp, _vp]),
    "sc_ctx_use_own_stream": (_i, [_vp]),
    "sc_ctx_synchronize": (_i, [_vp]),
    "sc_ctx_set_timing": (_i, [_vp, _i]),
    "sc_ctx_reset_timing": (_i, [_vp]),
    "sc_ctx_get_timing": (_i, [_vp, _i, C.POINTER(_d), _i64p]),
    "sc_ctx_scratch_bytes": (_i, [_vp, _i64p]),
    "sc_edt_u8_i32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sc_edt_u8_i32_host": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sc_moves_i32_u8": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp]),
    "sc_astar_batch": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_astar_batch_multi": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_astar_batch_host": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_astar_last_expansions": (_i, [_vp, _i64p]),
    "sc_astar_debug_stats": (_i, [_vp, _vp, _i]),
    "sc_astar_debug_peek": (_i, [_vp, _vp]),
    "sc_astar_gfield": (_i, [_vp, _vp, _i, _i, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sc_path_waypoints_batch": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sc_path_waypoints_batch_host": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sc_cost_field_batch": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _i, _i, _vp, _vp]),
    "sc_cost_field_batch_host": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _i, _i, _vp, _vp]),
    "sc_field_paths_batch": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_field_paths_batch_host": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_clearance_penalty_u8": (_i, [_vp, _vp, _i, _i, _i, C.c_int32, C.c_int32, _i, _vp]),
    "sc_clearance_penalty_u8_host": (_i, [_vp, _vp, _i, _i, _i, C.c_int32, C.c_int32, _i, _vp]),
    "sc_cost_field_weighted_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _i, _i, _vp, _vp]),
    "sc_cost_field_weighted_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _i, _i, _vp, _vp]),
    "sc_field_paths_weighted_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp,
                                           _vp]),
    "sc_field_paths_weighted_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp,
                                                _vp, _vp]),
    "sc_cost_field_multi_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sc_cost_field_multi_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sc_field_paths_multi_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp,
                                        _vp, _vp, _vp]),
    "sc_field_paths_multi_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp,
                                             _vp, _vp, _vp, _vp]),
    "sc_components_batch": (_i, [_vp, _vp, _i, _i, _i, C.c_int32, _vp, _vp, _vp, _vp]),
    "sc_components_batch_host": (_i, [_vp, _vp, _i, _i, _i, C.c_int32, _vp, _vp, _vp, _vp]),
    "sc_reachable_batch": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "sc_reachable_batch_host": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "sc_astar_batch_screened": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, C.c_int32, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_toppra_hermite_batch": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [_i, _vp, _vp, _d, _d] + [_vp] * 5),
    "sc_toppra_hermite_batch_host": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [_i, _vp, _vp, _d, _d] + [_vp] * 5),
    "sc_toppra_sample_batch": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [_d, _i] + [_vp] * 5),
    "sc_toppra_sample_batch_host": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [_d, _i] + [_vp] * 5),
    "sc_fmt_star_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.c_float, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_fmt_star_batch_host": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.c_float, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_edt_nearest_i32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sc_occ_from_rects": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sc_occ_from_polygons": (_i, [_vp, _vp, _i, _i, _i] + [C.c_float] * 4 + [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "sc_occ_from_polygons_host": (_i, [_vp, _vp, _i, _i, _i] + [C.c_float] * 4 + [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "sc_bezier_from_path_batch": (_i, [_vp, _vp, _vp, _i, _i, C.c_float, _vp, _i, _vp]),
    "sc_bezier_from_path_batch_host": (_i, [_vp, _vp, _vp, _i, _i, C.c_float, _vp, _i, _vp]),
    "sc_bezier_shrink_tangent_batch": (_i, [_vp, _vp, _vp, _i, C.c_float, _vp, _i, _vp]),
    "sc_bezier_shrink_tangent_batch_host": (_i, [_vp, _vp, _vp, _i, C.c_float, _vp, _i, _vp]),
    "sc_bezier_eval_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "sc_bezier_eval_batch_host": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "sc_bezier_curve_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp]),
    "sc_bezier_curve_batch_host": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "sc_chebfit_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "sc_chebfit_batch_host": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "sc_chebeval_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "sc_chebeval_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "sc_bezier_arclength_batch_host": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "sc_bezier_arclength_batch": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "sc_bezier_resample_batch": (_i, [_vp] * 5 + [_i, _i, _i, _vp, _vp, _i] + [_vp] * 5),
    "sc_bezier_resample_batch_host": (_i, [_vp] * 5 + [_i, _i, _i, _vp, _vp, _i] + [_vp] * 5),
    "sc_smooth_paths_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16),
    "sc_smooth_paths_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16),
    "sc_cells_to_points_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "sc_speed_limits_batch": (_i, [_vp] * 6 + [_i] * 4 + [_vp] * 3 + [_i, _i] + [C.c_float] * 4 + [_vp] * 3),
    "sc_speed_limits_batch_host": (_i, [_vp] * 6 + [_i] * 4 + [_vp] * 3 + [_i, _i] + [C.c_float] * 4 + [_vp] * 3),
    "sc_smooth_paths_limited_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16 +
                                      [_vp, _i, _vp, _i, _i] + [C.c_float] * 4 + [_vp, _vp]),
    "sc_smooth_paths_limited_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16 +
                                           [_vp, _i, _vp, _i, _i] + [C.c_float] * 4 + [_vp, _vp]),
    "sc_curve_clearance_batch": (_i, [_vp] * 4 + [_i, _vp, _i, _i] + [C.c_float] * 4 + [C.c_int32] + [_vp] * 5),
    "sc_curve_clearance_batch_host": (_i, [_vp] * 4 + [_i, _vp, _i, _i] + [C.c_float] * 4 + [C.c_int32] + [_vp] * 5),
    "sc_curve_clear_batch": (_i, [_vp] * 4 + [_i, _vp, _i, _i] + [C.c_float] * 4 + [C.c_int32, _i] + [_vp] * 5),
    "sc_curve_clear_batch_host": (_i, [_vp] * 4 + [_i, _vp, _i, _i] + [C.c_float] * 4 + [C.c_int32, _i] + [_vp] * 5),
    "sc_smooth_paths_clear_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16 +
                                    [_vp, _i, _vp, _i, _i] + [C.c_float] * 4 + [_vp, _vp] + [C.c_int32, _i] + [_vp] * 3),
    "sc_smooth_paths_clear_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.c_float, _vp, _i, C.c_float, _i, _i, C.c_int64] + [_vp] * 16 +
                                         [_vp, _i, _vp, _i, _i] + [C.c_float] * 4 + [_vp, _vp] + [C.c_int32, _i] + [_vp] * 3),
    "sc_traj_knots_batch": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp]),
    "sc_traj_knots_batch_host": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp]),
    "sc_traj_conflicts_batch": (_i, [_vp] * 3 + [_i, _i, _d, _d, _vp, _vp, _d] + [_vp] * 6),
    "sc_traj_conflicts_batch_host": (_i, [_vp] * 3 + [_i, _i, _d, _d, _vp, _vp, _d] + [_vp] * 6),
    "sc_fleet_conflicts_batch": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp, _vp, _vp, _d] + [_vp] * 6),
    "sc_fleet_conflicts_batch_host": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp, _vp, _vp, _d] + [_vp] * 6),
    "sc_traj_shift_table_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "sc_traj_shift_table_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "sc_traj_schedule_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_traj_schedule_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "sc_traj_shift_knots_batch": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp]),
    "sc_traj_shift_knots_batch_host": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp]),
    "sc_fleet_schedule_batch": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp, _vp, _vp, _i, _i] + [_vp] * 6),
    "sc_fleet_schedule_batch_host": (_i, [_vp] * 6 + [_i, _vp, _vp, _d, _d, _i, _vp, _vp, _vp, _vp, _i, _i] + [_vp] * 6),
    "sc_traj_reserve_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _i] + [C.c_float] * 4 + [_vp]),
    "sc_traj_reserve_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _i] + [C.c_float] * 4 + [_vp]),
    "sc_tplan_batch": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 5 + [C.c_float] * 4 + [_vp]),
    "sc_tplan_batch_host": (_i, [_vp, _vp, _i, _i, C.c_int32, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 5 + [C.c_float] * 4 + [_vp]),
    "sc_fleet_replan_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _i] + [C.c_float] * 4 + [_vp] +
                              [_vp, C.c_int32, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 7 + [_i]),
    "sc_fleet_replan_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _i] + [C.c_float] * 4 + [_vp] +
                                   [_vp, C.c_int32, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 7 + [_i]),
    "sc_field_cost_matrix": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "sc_field_cost_matrix_host": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "sc_assign_batch": (_i, [_vp, _vp, _i, _i, _i] + [_vp] * 5),
    "sc_assign_batch_host": (_i, [_vp, _vp, _i, _i, _i] + [_vp] * 5),
    "sc_fleet_assign_batch": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp] + [_vp] * 6),
    "sc_fleet_assign_batch_host": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp] + [_vp] * 6),
    "sc_known_from_discs": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sc_known_from_discs_host": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sc_d2_known_i32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sc_d2_known_i32_host": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sc_frontier_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_int32, _i, _i] + [_vp] * 7),
    "sc_frontier_batch_host": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_int32, _i, _i] + [_vp] * 7),
    "sc_frontier_cost_matrix": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, C.c_int32, C.c_int32, _vp, _vp]),
    "sc_frontier_cost_matrix_host": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, C.c_int32, C.c_int32, _vp, _vp]),
    "sc_fleet_explore_batch": (_i, [_vp, _vp, _vp, _i, _i, C.c_int32, _i, _i, _vp, _i, C.c_int32, C.c_int32] + [_vp] * 14),
    "sc_fleet_explore_batch_host": (_i, [_vp, _vp, _vp, _i, _i, C.c_int32, _i, _i, _vp, _i, C.c_int32, C.c_int32] + [_vp] * 14),
    "sc_rank_range": (None, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "sc_comm_unique_id": (_i, [_vp]),
    "sc_comm_init": (_i, [_vp, _vp, _i, _i]),
    "sc_comm_adopt": (_i, [_vp, _vp, _i, _i]),
    "sc_comm_destroy": (_i, [_vp]),
    "sc_allgather_paths": (_i, [_vp] * 5 + [_i, _i, _i, _i] + [_vp] * 5 + [C.c_int64, _vp, _vp]),
    "sc_allgather_last_bytes": (_i, [_vp, _i64p]),
    "sc_gather_msg_words": (C.c_int64, [_i, _i, _i]),
    "sc_gather_pack": (_i, [_vp] * 5 + [_i] * 6 + [_vp]),
    "sc_gather_unpack": (_i, [_vp, _vp, _i, _i, _i, _i] + [_vp] * 5 + [C.c_int64, _vp, _vp]),
}
EXPORTS = tuple(_SIGNATURES)


def lib():
    """Load the in-tree HIP library; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeaCurrentError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "or `make -C sea-current_amd` (there is no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (must be contiguous)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous()
    return t.data_ptr()


def _ghw(d2):
    """(G, H, W) of a map-shaped tensor or array: [H,W] is one grid, [G,H,W] a stack."""
    return (1,) + tuple(d2.shape) if len(d2.shape) == 2 else tuple(d2.shape)


def _field_entry(stem, pen, pen_cap, host=False):
    """The single-root field entry `stem` (sc_cost_field / sc_field_paths) for a costmap or none: its name and the
    arguments the weighted form takes after d2."""
    name = stem + ("_batch" if pen is None else "_weighted_batch") + ("_host" if host else "")
    return name, (() if pen is None else (_ptr(pen), pen_cap))


def _paths_out_torch(Q, Lmax, dev, which=False):
    """The uninitialised result dict of a read-out on the GPU (astar_batch's layout; which: the multi-source read-out's)."""
    import torch
    out = dict(path=torch.empty((Q, Lmax), dtype=torch.int32, device=dev))
    for k in ("len", "cost", "status") + (("which",) if which else ()):
        out[k] = torch.empty(Q, dtype=torch.int32, device=dev)
    return out


def _paths_out_numpy(Q, Lmax, which=False):
    """The result dict of a _host read-out: path -1, the rest 0."""
    out = dict(path=np.full((Q, Lmax), -1, dtype=np.int32))
    for k in ("len", "cost", "status") + (("which",) if which else ()):
        out[k] = np.zeros(Q, np.int32)
    return out


class Context:
    """One sc_ctx: one GPU, one stream.  `device` is the HIP device ordinal."""

    def __init__(self, device=0, use_torch_stream=True):
        # torch brings its own HIP runtime: let it initialise first, so that the library binds to the runtime that is already
        # in the process (loaded the other way round, the second runtime finds no GPU)
        import torch
        torch.cuda.is_available()
        self._l = lib()
        h = C.c_void_p()
        st = self._l.sc_ctx_create(device, C.byref(h))
        if st != 0:
            raise SeaCurrentError(f"sc_ctx_create(device={device}): {self._l.sc_status_string(st).decode()} "
                                  "(a gfx950 GPU is required; there is no CPU fallback)")
        self._h = h
        self.device = device
        if use_torch_stream:
            import torch
            self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def _ck(self, st, what):
        if st != 0:
            raise SeaCurrentError(f"{what}: {self._l.sc_status_string(st).decode()}: "
                                  f"{self._l.sc_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            self._l.sc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self._l.sc_ctx_set_stream(self._h, C.c_void_p(hip_stream or None)), "sc_ctx_set_stream")

    def use_own_stream(self):
        self._ck(self._l.sc_ctx_use_own_stream(self._h), "sc_ctx_use_own_stream")

    def synchronize(self):
        self._ck(self._l.sc_ctx_synchronize(self._h), "sc_ctx_synchronize")

    # -- timing
    def set_timing(self, on):
        self._ck(self._l.sc_ctx_set_timing(self._h, int(bool(on))), "sc_ctx_set_timing")

    def reset_timing(self):
        self._ck(self._l.sc_ctx_reset_timing(self._h), "sc_ctx_reset_timing")

    def get_timing(self, kid):
        ms, n = C.c_double(0), C.c_int64(0)
        self._ck(self._l.sc_ctx_get_timing(self._h, kid, C.byref(ms), C.byref(n)), "sc_ctx_get_timing")
        return ms.value, n.value

    def scratch_bytes(self):
        b = C.c_int64(0)
        self._ck(self._l.sc_ctx_scratch_bytes(self._h, C.byref(b)), "sc_ctx_scratch_bytes")
        return b.value

    # -- device-pointer entry points (torch CUDA tensors)
    def edt(self, occ, out=None):
        """occ: uint8 [B,H,W] or [H,W] on the GPU -> int32 d2 of the same shape."""
        import torch
        assert occ.is_cuda and occ.dtype == torch.uint8
        o3 = occ if occ.dim() == 3 else occ.unsqueeze(0)
        B, H, W = o3.shape
        if out is None:
            out = torch.empty(o3.shape, dtype=torch.int32, device=occ.device)
        self._ck(self._l.sc_edt_u8_i32(self._h, _ptr(o3.contiguous()), W, H, B, _ptr(out)), "sc_edt_u8_i32")
        return out if occ.dim() == 3 else out.view(H, W)

    def moves(self, d2, r2=0):
        import torch
        H, W = d2.shape
        out = torch.empty((H, W), dtype=torch.uint8, device=d2.device)
        self._ck(self._l.sc_moves_i32_u8(self._h, _ptr(d2), W, H, r2, _ptr(out)), "sc_moves_i32_u8")
        return out

    def astar_batch(self, d2, start, goal, r2=0, Lmax=4096, out=None, label=None):
        """d2 int32 [H,W]; start/goal int32 [Q] (GPU).  Returns dict of GPU tensors.  label (int32 [H,W], what components
        returned for the same d2 and r2): the screened search (sc_astar_batch_screened), the same results without searching
        the queries whose endpoints lie in different components."""
        import torch
        H, W = d2.shape
        Q = start.shape[0]
        if out is None:
            out = dict(path=torch.empty((Q, Lmax), dtype=torch.int32, device=d2.device),
                       len=torch.empty(Q, dtype=torch.int32, device=d2.device),
                       cost=torch.empty(Q, dtype=torch.int32, device=d2.device),
                       status=torch.empty(Q, dtype=torch.int32, device=d2.device))
        if label is not None:
            self._ck(self._l.sc_astar_batch_screened(self._h, _ptr(d2), _ptr(label), 1, None, W, H, r2, _ptr(start), _ptr(goal), Q, Lmax,
                                                     _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])),
                     "sc_astar_batch_screened")
            return out
        self._ck(self._l.sc_astar_batch(self._h, _ptr(d2), W, H, r2, _ptr(start), _ptr(goal), Q, Lmax,
                                        _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])),
                 "sc_astar_batch")
        return out

    def astar_batch_multi(self, d2, qgrid, start, goal, r2=0, Lmax=4096, out=None, label=None):
        """Several grids in one launch: d2 int32 [G,H,W], qgrid int32 [Q] (grid of every query), start/goal int32 [Q].
        label (int32 [G,H,W] from components): the screened search, as in astar_batch."""
        import torch
        G, H, W = d2.shape
        Q = start.shape[0]
        dev = d2.device
        if out is None:
            out = dict(path=torch.empty((Q, Lmax), dtype=torch.int32, device=dev), len=torch.empty(Q, dtype=torch.int32, device=dev),
                       cost=torch.empty(Q, dtype=torch.int32, device=dev), status=torch.empty(Q, dtype=torch.int32, device=dev))
        if label is not None:
            self._ck(self._l.sc_astar_batch_screened(self._h, _ptr(d2), _ptr(label), G, _ptr(qgrid), W, H, r2, _ptr(start), _ptr(goal), Q,
                                                     Lmax, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])),
                     "sc_astar_batch_screened")
            return out
        self._ck(self._l.sc_astar_batch_multi(self._h, _ptr(d2), G, _ptr(qgrid), W, H, r2, _ptr(start), _ptr(goal), Q, Lmax,
                                              _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"])), "sc_astar_batch_multi")
        return out

    def components(self, d2, r2=0, want_size=False, out=None):
        """Connected components of the traversable cells (sc_components_batch).  d2 int32 [H,W] or [G,H,W] on the GPU.
        Returns dict(label int32 shaped like d2: the smallest cell index of the cell's component, -1 where it is not
        traversable; size int32 shaped like d2 (the cell count at every representative, 0 elsewhere) or None without
        want_size; ncomp int32 [G]; largest int32 [G], -1 on a grid without a traversable cell).  `out`: the dict of an
        earlier call with the same shapes, reused.  Only enqueues."""
        import torch
        G, H, W = (1,) + tuple(d2.shape) if d2.dim() == 2 else tuple(d2.shape)
        dev = d2.device
        if out is None:
            out = dict(label=torch.empty(tuple(d2.shape), dtype=torch.int32, device=dev),
                       size=torch.empty(tuple(d2.shape), dtype=torch.int32, device=dev) if want_size else None,
                       ncomp=torch.empty(G, dtype=torch.int32, device=dev), largest=torch.empty(G, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_components_batch(self._h, _ptr(d2), G, W, H, r2, _ptr(out["label"]), _ptr(out.get("size")), _ptr(out["ncomp"]),
                                             _ptr(out["largest"])), "sc_components_batch")
        return out

    def reachable(self, label, start, goal, qgrid=None):
        """The status astar_batch would give every query, from the labels alone (sc_reachable_batch): label int32 [H,W] or
        [G,H,W] from components, start / goal int32 [Q], qgrid int32 [Q] (None only with one grid), on the GPU.  Returns
        int32 [Q]: Q_BAD_ENDPOINT, Q_NO_PATH, or Q_OK where A* returns Q_OK or Q_TRUNCATED."""
        import torch
        G, H, W = (1,) + tuple(label.shape) if label.dim() == 2 else tuple(label.shape)
        Q = start.shape[0]
        status = torch.empty(Q, dtype=torch.int32, device=label.device)
        self._ck(self._l.sc_reachable_batch(self._h, _ptr(label), G, _ptr(qgrid), W, H, _ptr(start), _ptr(goal), Q, _ptr(status)),
                 "sc_reachable_batch")
        return status

    def clearance_penalty(self, d2, r2=0, r2_soft=36, pen_max=40, out=None):
        """The costmap of the weighted cost fields from d2 (sc_clearance_penalty_u8): d2 int32 [H,W] or [G,H,W] on the GPU ->
        uint8 of the same shape, pen_max next to the hard clearance falling linearly to 0 at distance sqrt(r2_soft)."""
        import torch
        G, H, W = (1,) + tuple(d2.shape) if d2.dim() == 2 else tuple(d2.shape)
        if out is None:
            out = torch.empty(tuple(d2.shape), dtype=torch.uint8, device=d2.device)
        self._ck(self._l.sc_clearance_penalty_u8(self._h, _ptr(d2), W, H, G, r2, r2_soft, pen_max, _ptr(out)), "sc_clearance_penalty_u8")
        return out

    def cost_fields(self, d2, roots, r2=0, fgrid=None, rounds=-1, out=None, pen=None, pen_cap=255):
        """Cost-to-come fields (sc_cost_field_batch).  d2 int32 [H,W] or [G,H,W], roots int32 [F], fgrid int32 [F] (the grid
        of every field; None only with one grid), all on the GPU.  Returns dict(g int32 [F,H,W], status int32 [F]).
        pen (uint8, shaped like d2): the weighted fields (sc_cost_field_weighted_batch), entering cell c costs
        min(pen[c], pen_cap) more."""
        import torch
        G, H, W = _ghw(d2)
        F = roots.shape[0]
        dev = d2.device
        if out is None:
            out = dict(g=torch.empty((F, H, W), dtype=torch.int32, device=dev), status=torch.empty(F, dtype=torch.int32, device=dev))
        name, costmap = _field_entry("sc_cost_field", pen, pen_cap)
        self._ck(getattr(self._l, name)(self._h, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(roots), F, rounds, _ptr(out["g"]),
                                        _ptr(out["status"])), name)
        return out

    def field_paths(self, d2, g, roots, qfield, targets, r2=0, Lmax=4096, to_root=False, fgrid=None, out=None, pen=None, pen_cap=255):
        """Paths read from cost fields (sc_field_paths_batch): query q follows field qfield[q] (g int32 [F,H,W] and roots [F]
        as cost_fields took and returned them) to targets[q].  Returns astar_batch's dict of GPU tensors; to_root=True
        writes every path target..root.  pen, pen_cap: those cost_fields computed g with (sc_field_paths_weighted_batch)."""
        G, H, W = _ghw(d2)
        F = roots.shape[0]
        Q = targets.shape[0]
        if out is None:
            out = _paths_out_torch(Q, Lmax, d2.device)
        name, costmap = _field_entry("sc_field_paths", pen, pen_cap)
        self._ck(getattr(self._l, name)(self._h, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(g), _ptr(roots), F, _ptr(qfield),
                                        _ptr(targets), Q, Lmax, int(bool(to_root)), _ptr(out["path"]), _ptr(out["len"]),
                                        _ptr(out["cost"]), _ptr(out["status"])), name)
        return out

    def cost_fields_multi(self, d2, seeds, seed_off, seed_cost=None, r2=0, fgrid=None, rounds=-1, want_owner=True, pen=None, pen_cap=255,
                          out=None):
        """Multi-source cost fields (sc_cost_field_multi_batch): field f starts from seeds[seed_off[f]:seed_off[f+1]] (cell
        indices on grid fgrid[f]), each with the start cost seed_cost[s] (None: 0).  d2 int32 [H,W] or [G,H,W], seeds /
        seed_cost int32 [n_seed], seed_off int32 [F+1], fgrid int32 [F] (None only with one grid), pen uint8 shaped like d2
        (None: unweighted), all on the GPU.  Returns dict(g int32 [F,H,W], owner int32 [F,H,W]: the index into seeds of the
        seed every cell's path ends at, -1 where g is FIELD_INF, None without want_owner; status int32 [F])."""
        import torch
        G, H, W = _ghw(d2)
        F = seed_off.shape[0] - 1
        dev = d2.device
        if out is None:
            out = dict(g=torch.empty((F, H, W), dtype=torch.int32, device=dev),
                       owner=torch.empty((F, H, W), dtype=torch.int32, device=dev) if want_owner else None,
                       status=torch.empty(F, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_cost_field_multi_batch(self._h, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(seeds),
                                                   _ptr(seed_cost), _ptr(seed_off), seeds.shape[0], F, rounds, _ptr(out["g"]),
                                                   _ptr(out.get("owner")), _ptr(out["status"])), "sc_cost_field_multi_batch")
        return out

    def field_paths_multi(self, d2, fields, seeds, qfield, targets, r2=0, Lmax=4096, to_seed=False, fgrid=None, pen=None, pen_cap=255,
                          out=None):
        """Paths read from multi-source fields (sc_field_paths_multi_batch): query q follows field qfield[q] of `fields` (the
        dict cost_fields_multi returned, with its owner) from targets[q] to the seed that owns it.  Returns astar_batch's dict
        of GPU tensors plus which int32 [Q] (the index into seeds of that seed, -1 without a path); to_seed=True writes every
        path target..seed.  pen, pen_cap: those cost_fields_multi computed the fields with."""
        G, H, W = _ghw(d2)
        F = fields["g"].shape[0]
        Q = targets.shape[0]
        if out is None:
            out = _paths_out_torch(Q, Lmax, d2.device, which=True)
        self._ck(self._l.sc_field_paths_multi_batch(self._h, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(fields["g"]),
                                                    _ptr(fields["owner"]), _ptr(seeds), seeds.shape[0], F, _ptr(qfield), _ptr(targets), Q,
                                                    Lmax, int(bool(to_seed)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]),
                                                    _ptr(out["status"]), _ptr(out["which"])), "sc_field_paths_multi_batch")
        return out

    def path_waypoints(self, d2, res, r2=0, Wmax=None, out=None):
        """Line-of-sight waypoints of astar_batch's paths (sc_path_waypoints_batch).  d2 int32 [H,W] and `res` (the dict
        astar_batch returned, same r2) on the GPU; Wmax defaults to its Lmax.  Returns dict(wp int32 [Q,Wmax] cell indices,
        n int32 [Q], status int32 [Q]) as GPU tensors."""
        import torch
        H, W = d2.shape
        Q, Lmax = res["path"].shape
        if Wmax is None:
            Wmax = Lmax
        dev = d2.device
        if out is None:
            out = dict(wp=torch.empty((Q, Wmax), dtype=torch.int32, device=dev), n=torch.empty(Q, dtype=torch.int32, device=dev),
                       status=torch.empty(Q, dtype=torch.int32, device=dev))
        st = res.get("status")
        self._ck(self._l.sc_path_waypoints_batch(self._h, _ptr(d2), W, H, r2, _ptr(res["path"]), _ptr(res["len"]), _ptr(st), Q, Lmax, Wmax,
                                                 _ptr(out["wp"]), _ptr(out["n"]), _ptr(out["status"])), "sc_path_waypoints_batch")
        return out

    def cells_to_points(self, wr, W, x_min, y_min, res_x, res_y, starts=None, goals=None):
        """path_waypoints' result (dict wp int32 [Q,Wmax], n, status) -> (path float32 [Q,Wmax,2], npts int32 [Q]), the cell
        centres of a W-wide grid (sc_cells_to_points_batch); starts / goals float32 [Q,2] replace the two ends."""
        import torch
        Q, Wmax = wr["wp"].shape
        dev = wr["wp"].device
        path = torch.zeros((Q, Wmax, 2), dtype=torch.float32, device=dev)
        npts = torch.empty(Q, dtype=torch.int32, device=dev)
        self._ck(self._l.sc_cells_to_points_batch(self._h, _ptr(wr["wp"]), _ptr(wr["n"]), _ptr(wr.get("status")), Q, Wmax, W, x_min, y_min,
                                                  res_x, res_y, _ptr(starts), _ptr(goals), _ptr(path), _ptr(npts)), "sc_cells_to_points_batch")
        return path, npts

    @staticmethod
    def _smooth_estimate(wp, npts, limits, dt):
        """Samples to reserve for smooth_paths(capacity=None), the rule of the C++ header's smooth_paths_batch: per path
        (1.5 * polyline length / vel_max + 2 vel_max / acc_max) / dt * 1.25 + 64 (64 where that is not finite).  Only a
        first guess: a call that needs more is repeated with the exact count."""
        import torch
        n_max = wp.shape[1]
        leg = (wp[:, 1:] - wp[:, :-1]).double().norm(dim=-1)
        use = torch.arange(n_max - 1, device=wp.device)[None, :] < (npts.long()[:, None] - 1)
        poly = torch.where(use, leg, torch.zeros_like(leg)).sum(1)
        v = torch.where(limits[:, 1] > 0, limits[:, 1], torch.ones_like(limits[:, 1]))
        a = torch.where(limits[:, 3] > 0, limits[:, 3], torch.ones_like(limits[:, 3]))
        T = 1.5 * poly / v + 2.0 * v / a
        est = torch.where(torch.isfinite(T), (T / dt * 1.25).clamp(max=1e6).floor() + 64, torch.full_like(T, 64.0))
        return int(est.sum().item())

    @staticmethod
    def _frame(d2, frame):
        """(W, H, x_min, y_min, res_x, res_y) of a grid argument; frame = (x_min, y_min, res_x, res_y)."""
        if d2 is None:
            return (0, 0, 0.0, 0.0, 0.0, 0.0)
        if frame is None:
            raise ValueError("d2 needs frame=(x_min, y_min, res_x, res_y)")
        H, W = d2.shape
        return (W, H) + tuple(float(v) for v in frame)

    def speed_limits(self, ctrl, cum, seg_off, arclength, limits, dyn, N=100, J=4, status=None, d2=None, frame=None):
        """Per-stage speed limits of P curves from curvature and clearance (sc_speed_limits_batch; the definition is in
        include/sea_current_hip.h).  GPU tensors: ctrl float32 [S,4,2], cum float32 [S,nsub+1], seg_off int32 [P+1], arclength
        float32 [P], limits / dyn float64 [P,4] or 4 numbers for every curve, dyn = (omega_max, alat_max, clear_floor,
        clear_gain), status int32 [P] or None, d2 int32 [H,W] with frame = (x_min, y_min, res_x, res_y) or None.  Returns
        dict(vhi float64 [P,N+1], min_clear float32 [P], status int32 [P])."""
        import torch
        P = arclength.shape[0]
        dev = arclength.device
        f4 = lambda v: (v if torch.is_tensor(v) else torch.tensor([list(map(float, v))] * P, dtype=torch.float64, device=dev)) \
            .to(torch.float64).expand(P, 4).contiguous()
        limits, dyn = f4(limits), f4(dyn)
        out = dict(vhi=torch.empty((P, N + 1), dtype=torch.float64, device=dev), min_clear=torch.empty(P, dtype=torch.float32, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_speed_limits_batch(self._h, _ptr(ctrl), _ptr(cum), _ptr(seg_off), _ptr(arclength), _ptr(status), P,
                                               cum.shape[-1] - 1, N, J, _ptr(limits), _ptr(dyn), _ptr(d2), *self._frame(d2, frame),
                                               _ptr(out["vhi"]), _ptr(out["min_clear"]), _ptr(out["status"])), "sc_speed_limits_batch")
        return out

    def speed_limits_host(self, ctrl, cum, seg_off, arclength, limits, dyn, N=100, J=4, status=None, d2=None, frame=None):
        """Host form of speed_limits (numpy in, numpy out; sc_speed_limits_batch_host checks the contract of dyn first)."""
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float32)
        cum = np.ascontiguousarray(cum, dtype=np.float32)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        arclength = np.ascontiguousarray(arclength, dtype=np.float32)
        P = arclength.shape[0]
        limits = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, dtype=np.float64), (P, 4)))
        dyn = np.ascontiguousarray(np.broadcast_to(np.asarray(dyn, dtype=np.float64), (P, 4)))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        d2 = None if d2 is None else np.ascontiguousarray(d2, dtype=np.int32)
        out = dict(vhi=np.zeros((P, N + 1)), min_clear=np.zeros(P, np.float32), status=np.zeros(P, np.int32))
        self._ck(self._l.sc_speed_limits_batch_host(self._h, _ptr(ctrl), _ptr(cum), _ptr(seg_off), _ptr(arclength), _ptr(status), P,
                                                    cum.shape[-1] - 1, N, J, _ptr(limits), _ptr(dyn), _ptr(d2), *self._frame(d2, frame),
                                                    _ptr(out["vhi"]), _ptr(out["min_clear"]), _ptr(out["status"])),
                 "sc_speed_limits_batch_host")
        return out

    def curve_clearance(self, ctrl, seg_off, d2, frame, r2_clear=0, status=None):
        """Which cells P curves visit (sc_curve_clearance_batch; the definition is in include/sea_current_hip.h).  GPU tensors:
        ctrl float32 [S,4,2], seg_off int32 [P+1], d2 int32 [H,W] with frame = (x_min, y_min, res_x, res_y), status int32 [P] or
        None.  Returns dict(leg_min int32 [S], path_min, hit_legs, hit_leg int32 [P], hit_t float32 [P]); the legs of skipped
        paths read -1 in leg_min."""
        import torch
        P, S, dev = seg_off.shape[0] - 1, ctrl.shape[0], ctrl.device
        i = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        o = dict(leg_min=torch.full((S,), -1, dtype=torch.int32, device=dev), path_min=i(P), hit_legs=i(P), hit_leg=i(P),
                 hit_t=torch.empty(P, dtype=torch.float32, device=dev))
        self._ck(self._l.sc_curve_clearance_batch(self._h, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2), *self._frame(d2, frame),
                                                  int(r2_clear), *[_ptr(o[k]) for k in ("leg_min", "path_min", "hit_legs", "hit_leg", "hit_t")]),
                 "sc_curve_clearance_batch")
        return o

    def curve_clearance_host(self, ctrl, seg_off, d2, frame, r2_clear=0, status=None):
        """Host form of curve_clearance (numpy in, numpy out)."""
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float32)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        P, S = seg_off.shape[0] - 1, ctrl.shape[0]
        o = dict(leg_min=np.full(S, -1, np.int32), path_min=np.zeros(P, np.int32), hit_legs=np.zeros(P, np.int32),
                 hit_leg=np.zeros(P, np.int32), hit_t=np.zeros(P, np.float32))
        self._ck(self._l.sc_curve_clearance_batch_host(self._h, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2),
                                                       *self._frame(d2, frame), int(r2_clear),
                                                       *[_ptr(o[k]) for k in ("leg_min", "path_min", "hit_legs", "hit_leg", "hit_t")]),
                 "sc_curve_clearance_batch_host")
        return o

    def curve_clear(self, ctrl, seg_off, d2, frame, r2_clear=0, max_level=6, status=None, inplace=False):
        """Shrink the tangents of curves that hit the grid until none does (sc_curve_clear_batch).  Arguments as
        curve_clearance; inplace=True repairs ctrl itself.  Returns dict(ctrl float32 [S,4,2], level uint8 [S+P] (waypoint j of
        path p at seg_off[p] + p + j), rounds int32 [P], leg_min int32 [S] (-1 on the legs of skipped paths), status int32 [P],
        SMOOTH_COLLIDES where shrinking did not help)."""
        import torch
        P, S, dev = seg_off.shape[0] - 1, ctrl.shape[0], ctrl.device
        o = dict(ctrl=ctrl if inplace else torch.empty_like(ctrl), level=torch.empty(S + P, dtype=torch.uint8, device=dev),
                 rounds=torch.empty(P, dtype=torch.int32, device=dev), leg_min=torch.full((S,), -1, dtype=torch.int32, device=dev),
                 status=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_curve_clear_batch(self._h, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2), *self._frame(d2, frame),
                                              int(r2_clear), int(max_level),
                                              *[_ptr(o[k]) for k in ("ctrl", "level", "rounds", "leg_min", "status")]), "sc_curve_clear_batch")
        return o

    def curve_clear_host(self, ctrl, seg_off, d2, frame, r2_clear=0, max_level=6, status=None):
        """Host form of curve_clear (numpy in, numpy out)."""
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float32)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        P, S = seg_off.shape[0] - 1, ctrl.shape[0]
        o = dict(ctrl=np.zeros_like(ctrl), level=np.zeros(S + P, np.uint8), rounds=np.zeros(P, np.int32), leg_min=np.full(S, -1, np.int32),
                 status=np.zeros(P, np.int32))
        self._ck(self._l.sc_curve_clear_batch_host(self._h, _ptr(ctrl), _ptr(seg_off), _ptr(status), P, _ptr(d2), *self._frame(d2, frame),
                                                   int(r2_clear), int(max_level),
                                                   *[_ptr(o[k]) for k in ("ctrl", "level", "rounds", "leg_min", "status")]),
                 "sc_curve_clear_batch_host")
        return o

    def smooth_paths(self, wp, npts, limits, dt=0.02, N=100, nsub=100, start_angle=float("nan"), lines=None, capacity=None, out=None,
                     dyn=None, J=4, d2=None, frame=None, r2_clear=None, max_level=6):
        """The post-planner sequence for a batch of paths in one call (sc_smooth_paths_batch).  wp float32 [P,n_max,2],
        npts int32 [P], limits float64 [P,4] (vel_min, vel_max, acc_min, acc_max) or 4 numbers for every path, lines float32
        [E,4] or None; all on the GPU.  capacity=None: room for an estimate of the samples, the call repeated once with the
        exact count if that was short (reads `needed`: synchronises), and the per-sample outputs cut to `needed`.  With a
        capacity the call only enqueues.  `out`: the dict of an earlier call with the same P, n_max and capacity, reused.
        Returns dict(ctrl [P*(n_max-1),4,2], seg_off, arclength, length, offsets, status, needed [1], and per sample time,
        pos, vel, acc, pts [M,2], curvature, ang_vel, tpar, seg).
        dyn (float64 [P,4] or 4 numbers: omega_max, alat_max, clear_floor, clear_gain) asks for per-stage speed limits from
        curvature and, with d2 int32 [H,W] and frame = (x_min, y_min, res_x, res_y), clearance (sc_smooth_paths_limited_batch,
        J samples to each side of a stage); the dict then also holds vmax_stage float64 [P,N+1] and min_clear float32 [P].
        With dyn None the call is sc_smooth_paths_batch as before.
        r2_clear (needs d2; dyn None then means every speed term off) also keeps the curves clear of the grid
        (sc_smooth_paths_clear_batch): legs that visit a cell with d2 < max(r2_clear, 1) get the tangents at their ends halved,
        up to max_level times; the dict then also holds level uint8 [P*(n_max-1) + P], leg_min int32 [P*(n_max-1)] and rounds
        int32 [P], and a path that shrinking cannot fix reads SMOOTH_COLLIDES.  With r2_clear None the calls are those above."""
        import torch
        P, n_max, _ = wp.shape
        dev = wp.device
        if r2_clear is not None:
            if d2 is None:
                raise ValueError("r2_clear needs d2 and frame")
            if dyn is None:
                dyn = (float("inf"), float("inf"), float("inf"), 0.0)
        if dyn is None and d2 is not None:
            raise ValueError("d2 without dyn: the grid only enters through the speed limits")
        if dyn is not None:
            if not torch.is_tensor(dyn):
                dyn = torch.tensor([list(map(float, dyn))] * P, dtype=torch.float64, device=dev)
            dyn = dyn.to(torch.float64).expand(P, 4).contiguous()
            fr = self._frame(d2, frame)
        if not torch.is_tensor(limits):
            limits = torch.tensor([list(map(float, limits))] * P, dtype=torch.float64, device=dev)
        limits = limits.to(torch.float64).expand(P, 4).contiguous()
        nl = 0 if lines is None else lines.shape[0]
        auto = capacity is None
        cap = min(self._smooth_estimate(wp, npts, limits, dt), 2**31 - 1) if auto else int(capacity)

        def run(cap, o):
            if o is None or o["pos"].shape[0] != cap or o["status"].shape[0] != P or o["ctrl"].shape[0] != P * (n_max - 1):
                f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
                i = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
                o = dict(ctrl=f(P * (n_max - 1), 4, 2), seg_off=i(P + 1), arclength=f(P), length=i(P), offsets=i(P + 1), status=i(P),
                         needed=torch.empty(1, dtype=torch.int64, device=dev), time=torch.empty(cap, dtype=torch.float64, device=dev),
                         pos=f(cap), vel=f(cap), acc=f(cap), pts=f(cap, 2), curvature=f(cap), ang_vel=f(cap), tpar=f(cap), seg=i(cap))
            args = [self._h, _ptr(wp), _ptr(npts), P, n_max, _ptr(limits), start_angle, _ptr(lines) if nl else None, nl, dt, N, nsub, cap,
                    *[_ptr(o[k]) for k in ("ctrl", "seg_off", "arclength", "length", "offsets", "status", "needed", "time", "pos", "vel", "acc",
                                           "pts", "curvature", "ang_vel", "tpar", "seg")]]
            if dyn is None:
                self._ck(self._l.sc_smooth_paths_batch(*args), "sc_smooth_paths_batch")
                return o
            if "vmax_stage" not in o or o["vmax_stage"].shape != (P, N + 1):
                o["vmax_stage"] = torch.empty((P, N + 1), dtype=torch.float64, device=dev)
                o["min_clear"] = torch.empty(P, dtype=torch.float32, device=dev)
            if r2_clear is None:
                self._ck(self._l.sc_smooth_paths_limited_batch(*args, _ptr(dyn), J, _ptr(d2), *fr, _ptr(o["vmax_stage"]), _ptr(o["min_clear"])),
                         "sc_smooth_paths_limited_batch")
                return o
            if "level" not in o:
                S = P * (n_max - 1)
                o["level"] = torch.zeros(S + P, dtype=torch.uint8, device=dev)
                o["leg_min"] = torch.full((S,), -1, dtype=torch.int32, device=dev)
                o["rounds"] = torch.empty(P, dtype=torch.int32, device=dev)
            self._ck(self._l.sc_smooth_paths_clear_batch(*args, _ptr(dyn), J, _ptr(d2), *fr, _ptr(o["vmax_stage"]), _ptr(o["min_clear"]),
                                                         int(r2_clear), int(max_level), _ptr(o["level"]), _ptr(o["leg_min"]), _ptr(o["rounds"])),
                     "sc_smooth_paths_clear_batch")
            return o

        o = run(cap, out)
        if not auto:
            return o
        need = int(o["needed"][0])
        if need > cap:
            o = run(need, None)
        return {k: (v[:need] if k in ("time", "pos", "vel", "acc", "pts", "curvature", "ang_vel", "tpar", "seg") else v) for k, v in o.items()}

    def smooth_paths_host(self, wp, npts, limits, capacity, dt=0.02, N=100, nsub=100, start_angle=float("nan"), lines=None, dyn=None, J=4,
                          d2=None, frame=None, r2_clear=None, max_level=6):
        """Host form (numpy in, numpy out) of smooth_paths with room for `capacity` samples (sc_smooth_paths_batch_host; with
        dyn sc_smooth_paths_limited_batch_host, which adds vmax_stage and min_clear; with r2_clear
        sc_smooth_paths_clear_batch_host, which adds level, leg_min and rounds)."""
        if r2_clear is not None:
            if d2 is None:
                raise ValueError("r2_clear needs d2 and frame")
            if dyn is None:
                dyn = (float("inf"), float("inf"), float("inf"), 0.0)
        wp = np.ascontiguousarray(wp, dtype=np.float32)
        npts = np.ascontiguousarray(npts, dtype=np.int32)
        P, n_max, _ = wp.shape
        limits = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, dtype=np.float64), (P, 4)))
        lines = None if lines is None else np.ascontiguousarray(lines, dtype=np.float32)
        nl = 0 if lines is None else lines.shape[0]
        cap = int(capacity)
        o = dict(ctrl=np.zeros((P * (n_max - 1), 4, 2), np.float32), seg_off=np.zeros(P + 1, np.int32), arclength=np.zeros(P, np.float32),
                 length=np.zeros(P, np.int32), offsets=np.zeros(P + 1, np.int32), status=np.zeros(P, np.int32), needed=np.zeros(1, np.int64),
                 time=np.zeros(cap), pos=np.zeros(cap, np.float32), vel=np.zeros(cap, np.float32), acc=np.zeros(cap, np.float32),
                 pts=np.zeros((cap, 2), np.float32), curvature=np.zeros(cap, np.float32), ang_vel=np.zeros(cap, np.float32),
                 tpar=np.zeros(cap, np.float32), seg=np.zeros(cap, np.int32))
        args = [self._h, _ptr(wp), _ptr(npts), P, n_max, _ptr(limits), start_angle, _ptr(lines) if nl else None, nl, dt, N, nsub, cap,
                *[_ptr(o[k]) for k in ("ctrl", "seg_off", "arclength", "length", "offsets", "status", "needed", "time", "pos", "vel", "acc",
                                       "pts", "curvature", "ang_vel", "tpar", "seg")]]
        if dyn is None:
            if d2 is not None:
                raise ValueError("d2 without dyn: the grid only enters through the speed limits")
            self._ck(self._l.sc_smooth_paths_batch_host(*args), "sc_smooth_paths_batch_host")
            return o
        dyn = np.ascontiguousarray(np.broadcast_to(np.asarray(dyn, dtype=np.float64), (P, 4)))
        d2 = None if d2 is None else np.ascontiguousarray(d2, dtype=np.int32)
        o["vmax_stage"] = np.zeros((P, N + 1))
        o["min_clear"] = np.zeros(P, np.float32)
        if r2_clear is None:
            self._ck(self._l.sc_smooth_paths_limited_batch_host(*args, _ptr(dyn), J, _ptr(d2), *self._frame(d2, frame), _ptr(o["vmax_stage"]),
                                                                _ptr(o["min_clear"])), "sc_smooth_paths_limited_batch_host")
            return o
        S = P * (n_max - 1)
        o["level"], o["leg_min"], o["rounds"] = np.zeros(S + P, np.uint8), np.full(S, -1, np.int32), np.zeros(P, np.int32)
        self._ck(self._l.sc_smooth_paths_clear_batch_host(*args, _ptr(dyn), J, _ptr(d2), *self._frame(d2, frame), _ptr(o["vmax_stage"]),
                                                          _ptr(o["min_clear"]), int(r2_clear), int(max_level), _ptr(o["level"]),
                                                          _ptr(o["leg_min"]), _ptr(o["rounds"])), "sc_smooth_paths_clear_batch_host")
        return o

    # ---- conflicts between timed paths (sc_traj_knots_batch, sc_traj_conflicts_batch, sc_fleet_conflicts_batch) ----
    @staticmethod
    def _traj_ticks(sm, t0, T0, dt_c):
        """K that covers the longest path plus its delay: the last tick at or after max(time[last] + t0) over the paths that
        have samples.  Reads the paths' end times (torch: synchronises)."""
        off, ln = sm["offsets"], sm["length"]
        st = sm.get("status")
        if isinstance(ln, np.ndarray):
            use = (ln >= 1) & ((st == SMOOTH_OK) if st is not None else True)
            if not use.any():
                return 1
            end = sm["time"][(off[:-1] + ln - 1)[use]] + (0.0 if t0 is None else np.asarray(t0, np.float64)[use])
            end = float(end[np.isfinite(end)].max()) if np.isfinite(end).any() else T0
        else:
            import torch
            use = ln >= 1
            if st is not None:
                use = use & (st == SMOOTH_OK)
            idx = (off[:-1].long() + ln.long() - 1)[use]
            if idx.numel() == 0:
                return 1
            end = sm["time"][idx] + (0.0 if t0 is None else t0[use])
            end = end[torch.isfinite(end)]
            end = float(end.max()) if end.numel() else T0
        return int(min(max(np.ceil((end - T0) / dt_c), 1), TRAJ_MAX_TICKS))

    @staticmethod
    def _traj_out(P, dev, want_matrix):
        import torch
        f = lambda: torch.empty(P, dtype=torch.float64, device=dev)
        i = lambda: torch.empty(P, dtype=torch.int32, device=dev)
        # the bits of a row as int32 words (torch has no uint32 arithmetic): bit q % 32 of word q // 32
        return dict(first_t=f(), first_with=i(), min_sep=f(), min_with=i(), n_conf=i(),
                    conflict=torch.empty((P, (P + 31) // 32), dtype=torch.int32, device=dev) if want_matrix else None)

    @staticmethod
    def _traj_out_host(P, want_matrix):
        return dict(first_t=np.zeros(P), first_with=np.zeros(P, np.int32), min_sep=np.zeros(P), min_with=np.zeros(P, np.int32),
                    n_conf=np.zeros(P, np.int32), conflict=np.zeros((P, (P + 31) // 32), np.uint32) if want_matrix else None)

    @staticmethod
    def _per_path(v, P, dtype, dev=None):
        """A per-path argument as a contiguous [P] array / tensor of dtype (a number stands for every path; None stays None)."""
        if v is None:
            return None
        if dev is None:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (P,)))
        import torch
        v = v if torch.is_tensor(v) else torch.tensor(v, dtype=dtype, device=dev)
        return v.to(dtype).expand(P).contiguous()

    def traj_knots(self, sm, t0=None, flags=None, T0=0.0, dt_c=0.1, K=None):
        """The positions of P timed paths on the common clock T0 + k * dt_c, k = 0 .. K (sc_traj_knots_batch; the definition
        is in include/sea_current_hip.h).  sm: the dict smooth_paths returned, or any dict of GPU tensors time float64 [M],
        pts float32 [M,2], offsets int32 [P+1], length int32 [P] and optionally status int32 [P].  t0 float64 [P] start
        delays, flags int32 [P] (bit 0 / 1: stands at its first / last point before / after its run; None = 3).  K=None
        covers the longest path plus its delay (reads the end times: synchronises); with a K the call only enqueues.
        Returns dict(knots float64 [P,K+1,2], NaN where a path is absent; tstatus int32 [P]; K)."""
        import torch
        P = sm["length"].shape[0]
        dev = sm["length"].device
        t0, flags = self._per_path(t0, P, torch.float64, dev), self._per_path(flags, P, torch.int32, dev)
        if K is None:
            K = self._traj_ticks(sm, t0, T0, dt_c)
        out = dict(knots=torch.empty((P, K + 1, 2), dtype=torch.float64, device=dev), tstatus=torch.empty(P, dtype=torch.int32, device=dev), K=K)
        self._ck(self._l.sc_traj_knots_batch(self._h, _ptr(sm["time"]), _ptr(sm["pts"]), _ptr(sm["offsets"]), _ptr(sm["length"]),
                                             _ptr(sm.get("status")), P, _ptr(t0), _ptr(flags), T0, dt_c, K, _ptr(out["knots"]),
                                             _ptr(out["tstatus"])), "sc_traj_knots_batch")
        return out

    def traj_conflicts(self, knots, tstatus, radius, group=None, T0=0.0, dt_c=0.1, sep_cap=float("inf"), want_matrix=False):
        """Who meets whom, when and how close, from knots (sc_traj_conflicts_batch): knots float64 [P,K+1,2] and tstatus int32
        [P] as traj_knots returned them (tstatus is updated: TRAJ_BAD for a radius outside the contract), radius float64 [P]
        or a number, group int32 [P] or None, T0 and dt_c those of the knots.  Returns dict(first_t, first_with, min_sep,
        min_with, n_conf, conflict int32 [P, ceil(P/32)] bit words or None without want_matrix, tstatus).  Only enqueues."""
        import torch
        P, K = knots.shape[0], knots.shape[1] - 1
        dev = knots.device
        radius, group = self._per_path(radius, P, torch.float64, dev), self._per_path(group, P, torch.int32, dev)
        out = self._traj_out(P, dev, want_matrix)
        self._ck(self._l.sc_traj_conflicts_batch(self._h, _ptr(knots), _ptr(tstatus), P, K, T0, dt_c, _ptr(radius), _ptr(group), sep_cap,
                                                 _ptr(out["first_t"]), _ptr(out["first_with"]), _ptr(out["min_sep"]), _ptr(out["min_with"]),
                                                 _ptr(out["n_conf"]), _ptr(out["conflict"])), "sc_traj_conflicts_batch")
        out["tstatus"] = tstatus
        return out

    def fleet_conflicts(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, sep_cap=float("inf"),
                        want_matrix=False, want_knots=False):
        """traj_knots and traj_conflicts in one call behind smooth_paths (sc_fleet_conflicts_batch): sm is the dict
        smooth_paths returned (see traj_knots), the other arguments are those of the two calls.  K=None covers the longest
        path plus its delay (synchronises once to read it); with a K the call only enqueues.  Returns traj_conflicts' dict
        plus K, and knots with want_knots (otherwise they stay in the context's scratch)."""
        import torch
        P = sm["length"].shape[0]
        dev = sm["length"].device
        t0, flags = self._per_path(t0, P, torch.float64, dev), self._per_path(flags, P, torch.int32, dev)
        radius, group = self._per_path(radius, P, torch.float64, dev), self._per_path(group, P, torch.int32, dev)
        if K is None:
            K = self._traj_ticks(sm, t0, T0, dt_c)
        out = self._traj_out(P, dev, want_matrix)
        out["tstatus"] = torch.empty(P, dtype=torch.int32, device=dev)
        out["K"] = K
        if want_knots:
            out["knots"] = torch.empty((P, K + 1, 2), dtype=torch.float64, device=dev)
        self._ck(self._l.sc_fleet_conflicts_batch(self._h, _ptr(sm["time"]), _ptr(sm["pts"]), _ptr(sm["offsets"]), _ptr(sm["length"]),
                                                  _ptr(sm.get("status")), P, _ptr(t0), _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")),
                                                  _ptr(out["tstatus"]), _ptr(radius), _ptr(group), sep_cap, _ptr(out["first_t"]),
                                                  _ptr(out["first_with"]), _ptr(out["min_sep"]), _ptr(out["min_with"]), _ptr(out["n_conf"]),
                                                  _ptr(out["conflict"])), "sc_fleet_conflicts_batch")
        return out

    @staticmethod
    def _traj_host_paths(sm):
        st = sm.get("status")
        return (np.ascontiguousarray(sm["time"], dtype=np.float64), np.ascontiguousarray(sm["pts"], dtype=np.float32),
                np.ascontiguousarray(sm["offsets"], dtype=np.int32), np.ascontiguousarray(sm["length"], dtype=np.int32),
                None if st is None else np.ascontiguousarray(st, dtype=np.int32))

    def traj_knots_host(self, sm, t0=None, flags=None, T0=0.0, dt_c=0.1, K=None):
        """Host form of traj_knots (numpy in, numpy out; sc_traj_knots_batch_host)."""
        time, pts, offsets, length, status = self._traj_host_paths(sm)
        P = length.shape[0]
        t0, flags = self._per_path(t0, P, np.float64), self._per_path(flags, P, np.int32)
        if K is None:
            K = self._traj_ticks(dict(time=time, offsets=offsets, length=length, status=status), t0, T0, dt_c)
        out = dict(knots=np.zeros((P, K + 1, 2)), tstatus=np.zeros(P, np.int32), K=K)
        self._ck(self._l.sc_traj_knots_batch_host(self._h, _ptr(time), _ptr(pts), _ptr(offsets), _ptr(length), _ptr(status), P, _ptr(t0),
                                                  _ptr(flags), T0, dt_c, K, _ptr(out["knots"]), _ptr(out["tstatus"])),
                 "sc_traj_knots_batch_host")
        return out

    def traj_conflicts_host(self, knots, tstatus, radius, group=None, T0=0.0, dt_c=0.1, sep_cap=float("inf"), want_matrix=False):
        """Host form of traj_conflicts (numpy in, numpy out; sc_traj_conflicts_batch_host).  tstatus is copied, not updated in
        place; conflict is uint32 [P, ceil(P/32)]."""
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, group = self._per_path(radius, P, np.float64), self._per_path(group, P, np.int32)
        out = self._traj_out_host(P, want_matrix)
        out["tstatus"] = np.array(tstatus, dtype=np.int32)
        self._ck(self._l.sc_traj_conflicts_batch_host(self._h, _ptr(knots), _ptr(out["tstatus"]), P, K, T0, dt_c, _ptr(radius), _ptr(group),
                                                      sep_cap, _ptr(out["first_t"]), _ptr(out["first_with"]), _ptr(out["min_sep"]),
                                                      _ptr(out["min_with"]), _ptr(out["n_conf"]), _ptr(out["conflict"])),
                 "sc_traj_conflicts_batch_host")
        return out

    def fleet_conflicts_host(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, sep_cap=float("inf"),
                             want_matrix=False, want_knots=False):
        """Host form of fleet_conflicts (numpy in, numpy out; sc_fleet_conflicts_batch_host)."""
        time, pts, offsets, length, status = self._traj_host_paths(sm)
        P = length.shape[0]
        t0, flags = self._per_path(t0, P, np.float64), self._per_path(flags, P, np.int32)
        radius, group = self._per_path(radius, P, np.float64), self._per_path(group, P, np.int32)
        if K is None:
            K = self._traj_ticks(dict(time=time, offsets=offsets, length=length, status=status), t0, T0, dt_c)
        out = self._traj_out_host(P, want_matrix)
        out["tstatus"] = np.zeros(P, np.int32)
        out["K"] = K
        if want_knots:
            out["knots"] = np.zeros((P, K + 1, 2))
        self._ck(self._l.sc_fleet_conflicts_batch_host(self._h, _ptr(time), _ptr(pts), _ptr(offsets), _ptr(length), _ptr(status), P, _ptr(t0),
                                                       _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")), _ptr(out["tstatus"]), _ptr(radius),
                                                       _ptr(group), sep_cap, _ptr(out["first_t"]), _ptr(out["first_with"]),
                                                       _ptr(out["min_sep"]), _ptr(out["min_with"]), _ptr(out["n_conf"]), _ptr(out["conflict"])),
                 "sc_fleet_conflicts_batch_host")
        return out

    # ---- delay schedules for timed paths (sc_traj_shift_table_batch, sc_traj_schedule_batch, sc_traj_shift_knots_batch,
    # sc_fleet_schedule_batch) ----
    def traj_shift_table(self, knots, tstatus, radius, group=None, D=8, stride=1):
        """For every pair of paths and every relative delay of -(D-1) .. D-1 slots of `stride` ticks: do they still meet
        (sc_traj_shift_table_batch; the definition is in include/sea_current_hip.h)?  knots, tstatus, radius and group as in
        traj_conflicts (tstatus is updated).  Returns dict(table int64 [P,P]: bit r + D - 1 of table[p][q] is set iff p,
        started r slots later than q, meets q; tstatus).  Only enqueues."""
        import torch
        P, K = knots.shape[0], knots.shape[1] - 1
        dev = knots.device
        radius, group = self._per_path(radius, P, torch.float64, dev), self._per_path(group, P, torch.int32, dev)
        table = torch.empty((P, P), dtype=torch.int64, device=dev)   # torch has no uint64 arithmetic: the words as int64
        self._ck(self._l.sc_traj_shift_table_batch(self._h, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(group), D, stride, _ptr(table)),
                 "sc_traj_shift_table_batch")
        return dict(table=table, tstatus=tstatus)

    def traj_schedule(self, table, tstatus, D=8, order=None, jmax=None):
        """Start slots by priority from a shift table (sc_traj_schedule_batch): walks order (int32 [P], None = 0, 1, ..) and
        gives every path the first slot <= jmax[p] (int32 [P] or a number, None = D-1, negative = pinned to slot 0) in which
        it meets none of the paths placed before it.  Returns dict(slot int32 [P]: >= 0, SLOT_UNRESOLVED, SLOT_NOT_OK or
        SLOT_UNNAMED; counts int32 [4]: slot 0, slot > 0, unresolved, not scheduled).  Only enqueues."""
        import torch
        P = table.shape[0]
        dev = table.device
        order = None if order is None else (order if torch.is_tensor(order) else torch.tensor(order, device=dev)).to(torch.int32).contiguous()
        if order is not None and order.shape[0] != P:
            raise ValueError("order has P entries")
        jmax = self._per_path(jmax, P, torch.int32, dev)
        out = dict(slot=torch.empty(P, dtype=torch.int32, device=dev), counts=torch.empty(4, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_traj_schedule_batch(self._h, _ptr(table), _ptr(tstatus), P, D, _ptr(order), _ptr(jmax), _ptr(out["slot"]),
                                                _ptr(out["counts"])), "sc_traj_schedule_batch")
        return out

    def traj_shift_knots(self, knots, slot, stride=1):
        """knots with every path held at its first knot for slot[p] * stride ticks; a path with slot < 0 becomes absent
        (sc_traj_shift_knots_batch).  Returns float64 [P,K+1,2].  Only enqueues."""
        import torch
        P, K = knots.shape[0], knots.shape[1] - 1
        out = torch.empty_like(knots)
        self._ck(self._l.sc_traj_shift_knots_batch(self._h, _ptr(knots), P, K, _ptr(slot), stride, _ptr(out)), "sc_traj_shift_knots_batch")
        return out

    def fleet_schedule(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, D=8, stride=1, order=None, jmax=None,
                       want_table=False, want_knots=False):
        """traj_knots, traj_shift_table, traj_schedule and traj_shift_knots in one call behind smooth_paths
        (sc_fleet_schedule_batch).  K=None covers the longest path, its delay and (D-1) * stride more ticks, so that every
        path is at rest where the shifts end and the schedule leaves no conflict among the paths with slot >= 0
        (synchronises once to read the end times); with a K the call only enqueues.  Returns dict(slot, counts, delay float64
        [P] = slot * stride * dt_c seconds, NaN for slot < 0; tstatus, K; table with want_table; knots and knots_out with
        want_knots)."""
        import torch
        P = sm["length"].shape[0]
        dev = sm["length"].device
        t0, flags = self._per_path(t0, P, torch.float64, dev), self._per_path(flags, P, torch.int32, dev)
        radius, group = self._per_path(radius, P, torch.float64, dev), self._per_path(group, P, torch.int32, dev)
        order = None if order is None else (order if torch.is_tensor(order) else torch.tensor(order, device=dev)).to(torch.int32).contiguous()
        if order is not None and order.shape[0] != P:
            raise ValueError("order has P entries")
        jmax = self._per_path(jmax, P, torch.int32, dev)
        if K is None:
            K = min(self._traj_ticks(sm, t0, T0, dt_c) + (D - 1) * stride, TRAJ_MAX_TICKS)
        out = dict(slot=torch.empty(P, dtype=torch.int32, device=dev), counts=torch.empty(4, dtype=torch.int32, device=dev),
                   tstatus=torch.empty(P, dtype=torch.int32, device=dev), K=K)
        if want_table:
            out["table"] = torch.empty((P, P), dtype=torch.int64, device=dev)
        if want_knots:
            out["knots"] = torch.empty((P, K + 1, 2), dtype=torch.float64, device=dev)
            out["knots_out"] = torch.empty((P, K + 1, 2), dtype=torch.float64, device=dev)
        self._ck(self._l.sc_fleet_schedule_batch(self._h, _ptr(sm["time"]), _ptr(sm["pts"]), _ptr(sm["offsets"]), _ptr(sm["length"]),
                                                 _ptr(sm.get("status")), P, _ptr(t0), _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")),
                                                 _ptr(out["tstatus"]), _ptr(radius), _ptr(group), D, stride, _ptr(out.get("table")),
                                                 _ptr(order), _ptr(jmax), _ptr(out["slot"]), _ptr(out["counts"]), _ptr(out.get("knots_out"))),
                 "sc_fleet_schedule_batch")
        out["delay"] = torch.where(out["slot"] >= 0, (out["slot"] * stride).to(torch.float64) * dt_c, float("nan"))
        return out

    def traj_shift_table_host(self, knots, tstatus, radius, group=None, D=8, stride=1):
        """Host form of traj_shift_table (numpy in, numpy out; sc_traj_shift_table_batch_host).  tstatus is copied, not
        updated in place; table is uint64 [P,P]."""
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, group = self._per_path(radius, P, np.float64), self._per_path(group, P, np.int32)
        out = dict(table=np.zeros((P, P), np.uint64), tstatus=np.array(tstatus, dtype=np.int32))
        self._ck(self._l.sc_traj_shift_table_batch_host(self._h, _ptr(knots), _ptr(out["tstatus"]), P, K, _ptr(radius), _ptr(group), D, stride,
                                                        _ptr(out["table"])), "sc_traj_shift_table_batch_host")
        return out

    def traj_schedule_host(self, table, tstatus, D=8, order=None, jmax=None):
        """Host form of traj_schedule (numpy in, numpy out; sc_traj_schedule_batch_host)."""
        table = np.ascontiguousarray(table).view(np.uint64)
        P = table.shape[0]
        tstatus = np.ascontiguousarray(tstatus, dtype=np.int32)
        order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        if order is not None and order.shape[0] != P:
            raise ValueError("order has P entries")
        jmax = self._per_path(jmax, P, np.int32)
        out = dict(slot=np.zeros(P, np.int32), counts=np.zeros(4, np.int32))
        self._ck(self._l.sc_traj_schedule_batch_host(self._h, _ptr(table), _ptr(tstatus), P, D, _ptr(order), _ptr(jmax), _ptr(out["slot"]),
                                                     _ptr(out["counts"])), "sc_traj_schedule_batch_host")
        return out

    def traj_shift_knots_host(self, knots, slot, stride=1):
        """Host form of traj_shift_knots (numpy in, numpy out; sc_traj_shift_knots_batch_host)."""
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        out = np.zeros_like(knots)
        self._ck(self._l.sc_traj_shift_knots_batch_host(self._h, _ptr(knots), knots.shape[0], knots.shape[1] - 1, _ptr(slot), stride, _ptr(out)),
                 "sc_traj_shift_knots_batch_host")
        return out

    def fleet_schedule_host(self, sm, radius, t0=None, flags=None, group=None, T0=0.0, dt_c=0.1, K=None, D=8, stride=1, order=None, jmax=None,
                            want_table=False, want_knots=False):
        """Host form of fleet_schedule (numpy in, numpy out; sc_fleet_schedule_batch_host)."""
        time, pts, offsets, length, status = self._traj_host_paths(sm)
        P = length.shape[0]
        t0, flags = self._per_path(t0, P, np.float64), self._per_path(flags, P, np.int32)
        radius, group = self._per_path(radius, P, np.float64), self._per_path(group, P, np.int32)
        order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        if order is not None and order.shape[0] != P:
            raise ValueError("order has P entries")
        jmax = self._per_path(jmax, P, np.int32)
        if K is None:
            K = min(self._traj_ticks(dict(time=time, offsets=offsets, length=length, status=status), t0, T0, dt_c) + (D - 1) * stride,
                    TRAJ_MAX_TICKS)
        out = dict(slot=np.zeros(P, np.int32), counts=np.zeros(4, np.int32), tstatus=np.zeros(P, np.int32), K=K)
        if want_table:
            out["table"] = np.zeros((P, P), np.uint64)
        if want_knots:
            out["knots"] = np.zeros((P, K + 1, 2))
            out["knots_out"] = np.zeros((P, K + 1, 2))
        self._ck(self._l.sc_fleet_schedule_batch_host(self._h, _ptr(time), _ptr(pts), _ptr(offsets), _ptr(length), _ptr(status), P, _ptr(t0),
                                                      _ptr(flags), T0, dt_c, K, _ptr(out.get("knots")), _ptr(out["tstatus"]), _ptr(radius),
                                                      _ptr(group), D, stride, _ptr(out.get("table")), _ptr(order), _ptr(jmax), _ptr(out["slot"]),
                                                      _ptr(out["counts"]), _ptr(out.get("knots_out"))), "sc_fleet_schedule_batch_host")
        with np.errstate(invalid="ignore"):
            out["delay"] = np.where(out["slot"] >= 0, (out["slot"] * stride).astype(np.float64) * dt_c, np.nan)
        return out

    # ---- re-planning in space-time around the scheduled fleet (sc_traj_reserve_batch, sc_tplan_batch, sc_fleet_replan_batch) ----
    @staticmethod
    def _tplan_out(B, L, H, W, dev, want_knots, want_reach):
        """The result buffers of a plan: torch on `dev`, numpy when dev is None.  Bit words are int32 in torch (it has no uint32
        arithmetic) and uint32 in numpy."""
        Wq = (W + 31) // 32
        if dev is None:
            out = dict(path=np.full((B, L), -1, np.int32), len=np.zeros(B, np.int32), arrive=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
            if want_knots:
                out["knots_out"] = np.zeros((B, L, 2))
            if want_reach:
                out["reach"] = np.zeros((B, L, H, Wq), np.uint32)
            return out
        import torch
        out = dict(path=torch.full((B, L), -1, dtype=torch.int32, device=dev))
        for k in ("len", "arrive", "status"):
            out[k] = torch.empty(B, dtype=torch.int32, device=dev)
        if want_knots:
            out["knots_out"] = torch.empty((B, L, 2), dtype=torch.float64, device=dev)
        if want_reach:
            out["reach"] = torch.empty((B, L, H, Wq), dtype=torch.int32, device=dev)
        return out

    def traj_reserve(self, knots, tstatus, radius, W, H, frame, pad, select=None, res=None):
        """Rasterise knot rows into reservations (sc_traj_reserve_batch; the definition is in include/sea_current_hip.h): cell c
        is reserved at layers k and k+1 when a robot standing at c through interval k would come within radius[q] + pad of path
        q.  knots float64 [P,K+1,2], tstatus int32 [P] or None (all OK; updated like in traj_conflicts), radius float64 [P] or a
        number, frame = (x_min, y_min, res_x, res_y), select int32 [P] or None (0 = leave this path out).  res int32 [K+1, H,
        ceil(W/32)] bit words is ORed into (None: a zeroed one) and returned.  Only enqueues."""
        import torch
        P, K = knots.shape[0], knots.shape[1] - 1
        dev = knots.device
        radius, select = self._per_path(radius, P, torch.float64, dev), self._per_path(select, P, torch.int32, dev)
        if res is None:
            res = torch.zeros((K + 1, H, (W + 31) // 32), dtype=torch.int32, device=dev)
        self._ck(self._l.sc_traj_reserve_batch(self._h, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                                               *(float(v) for v in frame), _ptr(res)), "sc_traj_reserve_batch")
        return res

    def tplan(self, d2, start, goal, res=None, L=None, t_start=None, hold=True, r2=0, frame=None, want_reach=False):
        """Earliest arrival on the time-expanded grid around reservations (sc_tplan_batch).  d2 int32 [H,W]; start, goal int32 [B]
        cells; res int32 [L,H,ceil(W/32)] as traj_reserve returned it, or None (nothing reserved; L must be given); t_start int32
        [B] layers or None = 0; hold: the robot stays at its goal, so it arrives only once the goal is never reserved again.
        Returns dict(path int32 [B,L] (-1 past len), len, arrive, status int32 [B] (TP_OK, TP_NO_PATH, TP_BAD_ENDPOINT,
        TP_START_BLOCKED); knots_out float64 [B,L,2] with a frame = (x_min, y_min, res_x, res_y): rows that traj_conflicts takes
        behind the fleet's; reach int32 [B,L,H,ceil(W/32)] with want_reach, otherwise the layers stay in the context's scratch).
        One stated earliest-arrival path, not the shortest in metres.  Only enqueues."""
        import torch
        H, W = d2.shape
        B = start.shape[0]
        L = res.shape[0] if L is None else L
        out = self._tplan_out(B, L, H, W, d2.device, frame is not None, want_reach)
        fr = (0.0, 0.0, 1.0, 1.0) if frame is None else tuple(float(v) for v in frame)
        self._ck(self._l.sc_tplan_batch(self._h, _ptr(d2), W, H, r2, _ptr(res), L, _ptr(start), _ptr(goal), _ptr(t_start), B, int(bool(hold)),
                                        _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]), _ptr(out["status"]), _ptr(out.get("knots_out")),
                                        *fr, _ptr(out.get("reach"))), "sc_tplan_batch")
        return out

    def fleet_replan(self, knots, tstatus, radius, d2, start, goal, frame, pad, r_new=None, select=None, t_start=None, hold=True, r2=0,
                     sequential=False, res=None, want_reach=False):
        """traj_reserve of the selected fleet rows, then tplan around them, in one call (sc_fleet_replan_batch): the fleet is knots
        / tstatus / radius / select as in traj_reserve (e.g. fleet_schedule's knots_out with select = slot >= 0), the robots are
        start / goal / t_start as in tplan.  pad: r_new + half the grid's diagonal move keeps a robot of radius r_new clear of
        every reserved path (see the header).  sequential=False plans all robots against the fleet at once; sequential=True
        plans robot i, reserves its row (radius r_new[i], the same pad) and goes on to robot i+1: prioritised planning in the
        caller's order (needs r_new, float64 [B] or a number).  Returns tplan's dict (knots_out always) plus res and tstatus.
        Only enqueues."""
        import torch
        P, K = knots.shape[0], knots.shape[1] - 1
        H, W = d2.shape
        B = start.shape[0]
        dev = knots.device
        radius, select = self._per_path(radius, P, torch.float64, dev), self._per_path(select, P, torch.int32, dev)
        r_new = self._per_path(r_new, B, torch.float64, dev)
        if res is None:
            res = torch.zeros((K + 1, H, (W + 31) // 32), dtype=torch.int32, device=dev)
        out = self._tplan_out(B, K + 1, H, W, dev, True, want_reach)
        self._ck(self._l.sc_fleet_replan_batch(self._h, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                                               *(float(v) for v in frame), _ptr(res), _ptr(d2), r2, K + 1, _ptr(start), _ptr(goal), _ptr(t_start),
                                               B, int(bool(hold)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]), _ptr(out["status"]),
                                               _ptr(out["knots_out"]), _ptr(out.get("reach")), _ptr(r_new), int(bool(sequential))),
                 "sc_fleet_replan_batch")
        out["res"] = res
        out["tstatus"] = tstatus
        return out

    def traj_reserve_host(self, knots, tstatus, radius, W, H, frame, pad, select=None, res=None):
        """Host form of traj_reserve (numpy in, numpy out; sc_traj_reserve_batch_host).  Returns (res uint32 [K+1,H,ceil(W/32)],
        tstatus): copies, the arguments are not updated in place."""
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        P, K = knots.shape[0], knots.shape[1] - 1
        radius, select = self._per_path(radius, P, np.float64), self._per_path(select, P, np.int32)
        tstatus = None if tstatus is None else np.array(tstatus, dtype=np.int32)
        res = np.zeros((K + 1, H, (W + 31) // 32), np.uint32) if res is None else np.array(res, dtype=np.uint32)
        self._ck(self._l.sc_traj_reserve_batch_host(self._h, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                                                    *(float(v) for v in frame), _ptr(res)), "sc_traj_reserve_batch_host")
        return res, tstatus

    def tplan_host(self, d2, start, goal, res=None, L=None, t_start=None, hold=True, r2=0, frame=None, want_reach=False):
        """Host form of tplan (numpy in, numpy out; sc_tplan_batch_host)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        H, W = d2.shape
        start, goal = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(goal, dtype=np.int32)
        t_start = None if t_start is None else np.ascontiguousarray(t_start, dtype=np.int32)
        res = None if res is None else np.ascontiguousarray(res).view(np.uint32)
        B = start.shape[0]
        L = res.shape[0] if L is None else L
        out = self._tplan_out(B, L, H, W, None, frame is not None, want_reach)
        fr = (0.0, 0.0, 1.0, 1.0) if frame is None else tuple(float(v) for v in frame)
        self._ck(self._l.sc_tplan_batch_host(self._h, _ptr(d2), W, H, r2, _ptr(res), L, _ptr(start), _ptr(goal), _ptr(t_start), B,
                                             int(bool(hold)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]), _ptr(out["status"]),
                                             _ptr(out.get("knots_out")), *fr, _ptr(out.get("reach"))), "sc_tplan_batch_host")
        return out

    def fleet_replan_host(self, knots, tstatus, radius, d2, start, goal, frame, pad, r_new=None, select=None, t_start=None, hold=True, r2=0,
                          sequential=False, res=None, want_reach=False):
        """Host form of fleet_replan (numpy in, numpy out; sc_fleet_replan_batch_host); res and tstatus are copies."""
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        P, K = knots.shape[0], knots.shape[1] - 1
        H, W = d2.shape
        start, goal = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(goal, dtype=np.int32)
        t_start = None if t_start is None else np.ascontiguousarray(t_start, dtype=np.int32)
        B = start.shape[0]
        radius, select = self._per_path(radius, P, np.float64), self._per_path(select, P, np.int32)
        r_new = self._per_path(r_new, B, np.float64)
        tstatus = None if tstatus is None else np.array(tstatus, dtype=np.int32)
        res = np.zeros((K + 1, H, (W + 31) // 32), np.uint32) if res is None else np.array(res, dtype=np.uint32)
        out = self._tplan_out(B, K + 1, H, W, None, True, want_reach)
        self._ck(self._l.sc_fleet_replan_batch_host(self._h, _ptr(knots), _ptr(tstatus), P, K, _ptr(radius), _ptr(select), float(pad), W, H,
                                                    *(float(v) for v in frame), _ptr(res), _ptr(d2), r2, K + 1, _ptr(start), _ptr(goal),
                                                    _ptr(t_start), B, int(bool(hold)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["arrive"]),
                                                    _ptr(out["status"]), _ptr(out["knots_out"]), _ptr(out.get("reach")), _ptr(r_new),
                                                    int(bool(sequential))), "sc_fleet_replan_batch_host")
        out["res"] = res
        out["tstatus"] = tstatus
        return out

    # ---- robots to goals (sc_field_cost_matrix, sc_assign_batch, sc_fleet_assign_batch) ----
    def field_cost_matrix(self, g, cells, col_cost=None, out=None):
        """The R x F cost matrix of robots at `cells` (int32 [R]) against the fields g (int32 [F,H,W], any of cost_fields' or
        cost_fields_multi's arrays): out[r][f] = g[f][cells[r]] (+ col_cost[f], int32 [F], 0 .. FIELD_SEED_COST_MAX), FIELD_INF
        kept; a cell out of range gives a row of FIELD_INF (sc_field_cost_matrix).  Returns int32 [R,F].  Only enqueues."""
        import torch
        F, H, W = g.shape
        R = cells.shape[0]
        if out is None:
            out = torch.empty((R, F), dtype=torch.int32, device=g.device)
        self._ck(self._l.sc_field_cost_matrix(self._h, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out)), "sc_field_cost_matrix")
        return out

    def assign(self, cost):
        """Optimal one-to-one matchings (sc_assign_batch; the definition is in include/sea_current_hip.h): cost int32 [B,R,C]
        or [R,C] (B = 1), FIELD_INF = forbidden.  Returns dict(col_of int32 [B,R], row_of int32 [B,C], u int64 [B,R], v int64
        [B,C], info int64 [B,4] = matched, total, steps, status), without the leading B for 2-D input.  Only enqueues."""
        import torch
        flat = cost.dim() == 2
        B, R, Cc = (1,) + tuple(cost.shape) if flat else tuple(cost.shape)
        dev = cost.device
        lead = () if flat else (B,)
        out = dict(col_of=torch.empty(lead + (R,), dtype=torch.int32, device=dev), row_of=torch.empty(lead + (Cc,), dtype=torch.int32, device=dev),
                   u=torch.empty(lead + (R,), dtype=torch.int64, device=dev), v=torch.empty(lead + (Cc,), dtype=torch.int64, device=dev),
                   info=torch.empty(lead + (4,), dtype=torch.int64, device=dev))
        self._ck(self._l.sc_assign_batch(self._h, _ptr(cost), B, R, Cc, _ptr(out["col_of"]), _ptr(out["row_of"]), _ptr(out["u"]), _ptr(out["v"]),
                                         _ptr(out["info"])), "sc_assign_batch")
        return out

    def fleet_assign(self, g, cells, col_cost=None, want_cost=False):
        """field_cost_matrix and assign in one call (sc_fleet_assign_batch): robots at `cells` to the goals the fields g are
        rooted at, one goal per robot.  Returns assign's dict for one problem (col_of[r] = the field of robot r or -1: what
        field_paths takes as qfield with to_root=True), plus cost int32 [R,F] with want_cost.  Only enqueues."""
        import torch
        F, H, W = g.shape
        R = cells.shape[0]
        dev = g.device
        out = dict(col_of=torch.empty(R, dtype=torch.int32, device=dev), row_of=torch.empty(F, dtype=torch.int32, device=dev),
                   u=torch.empty(R, dtype=torch.int64, device=dev), v=torch.empty(F, dtype=torch.int64, device=dev),
                   info=torch.empty(4, dtype=torch.int64, device=dev))
        if want_cost:
            out["cost"] = torch.empty((R, F), dtype=torch.int32, device=dev)
        self._ck(self._l.sc_fleet_assign_batch(self._h, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out.get("cost")),
                                               _ptr(out["col_of"]), _ptr(out["row_of"]), _ptr(out["u"]), _ptr(out["v"]), _ptr(out["info"])),
                 "sc_fleet_assign_batch")
        return out

    def field_cost_matrix_host(self, g, cells, col_cost=None, out=None):
        """Host form of field_cost_matrix (numpy in, numpy out; sc_field_cost_matrix_host)."""
        g, cells = np.ascontiguousarray(g, dtype=np.int32), np.ascontiguousarray(cells, dtype=np.int32)
        col_cost = None if col_cost is None else np.ascontiguousarray(col_cost, dtype=np.int32)
        F, H, W = g.shape
        R = cells.shape[0]
        if out is None:
            out = np.zeros((R, F), np.int32)
        self._ck(self._l.sc_field_cost_matrix_host(self._h, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out)),
                 "sc_field_cost_matrix_host")
        return out

    def assign_host(self, cost):
        """Host form of assign (numpy in, numpy out; sc_assign_batch_host)."""
        cost = np.ascontiguousarray(cost, dtype=np.int32)
        flat = cost.ndim == 2
        B, R, Cc = (1,) + cost.shape if flat else cost.shape
        lead = () if flat else (B,)
        out = dict(col_of=np.zeros(lead + (R,), np.int32), row_of=np.zeros(lead + (Cc,), np.int32), u=np.zeros(lead + (R,), np.int64),
                   v=np.zeros(lead + (Cc,), np.int64), info=np.zeros(lead + (4,), np.int64))
        self._ck(self._l.sc_assign_batch_host(self._h, _ptr(cost), B, R, Cc, _ptr(out["col_of"]), _ptr(out["row_of"]), _ptr(out["u"]),
                                              _ptr(out["v"]), _ptr(out["info"])), "sc_assign_batch_host")
        return out

    def fleet_assign_host(self, g, cells, col_cost=None, want_cost=False):
        """Host form of fleet_assign (numpy in, numpy out; sc_fleet_assign_batch_host)."""
        g, cells = np.ascontiguousarray(g, dtype=np.int32), np.ascontiguousarray(cells, dtype=np.int32)
        col_cost = None if col_cost is None else np.ascontiguousarray(col_cost, dtype=np.int32)
        F, H, W = g.shape
        R = cells.shape[0]
        out = dict(col_of=np.zeros(R, np.int32), row_of=np.zeros(F, np.int32), u=np.zeros(R, np.int64), v=np.zeros(F, np.int64),
                   info=np.zeros(4, np.int64))
        if want_cost:
            out["cost"] = np.zeros((R, F), np.int32)
        self._ck(self._l.sc_fleet_assign_batch_host(self._h, _ptr(g), F, W, H, _ptr(cells), R, _ptr(col_cost), _ptr(out.get("cost")),
                                                    _ptr(out["col_of"]), _ptr(out["row_of"]), _ptr(out["u"]), _ptr(out["v"]),
                                                    _ptr(out["info"])), "sc_fleet_assign_batch_host")
        return out

    # ---- exploration frontiers (sc_known_from_discs, sc_d2_known_i32, sc_frontier_batch, sc_frontier_cost_matrix,
    #      sc_fleet_explore_batch) ----
    def known_from_discs(self, discs, W, H, base=None, out=None):
        """The known-space mask of sensing discs (sc_known_from_discs): discs int32 [R,3] = (cx, cy, r2) on the GPU, base uint8
        [H,W] or None (may be `out`).  Returns uint8 [H,W], 1 where base is set or a disc covers the cell.  Only enqueues."""
        import torch
        if out is None:
            out = torch.empty((H, W), dtype=torch.uint8, device=discs.device)
        self._ck(self._l.sc_known_from_discs(self._h, _ptr(base), _ptr(discs), discs.shape[0], W, H, _ptr(out)), "sc_known_from_discs")
        return out

    def d2_known(self, d2, known, out=None):
        """d2 where known, 0 elsewhere (sc_d2_known_i32): d2 int32 and known uint8, [H,W] or [G,H,W] on the GPU; every planner
        run on the result moves through known free space only.  out may be d2.  Only enqueues."""
        import torch
        G, H, W = _ghw(d2)
        if out is None:
            out = torch.empty_like(d2)
        self._ck(self._l.sc_d2_known_i32(self._h, _ptr(d2), _ptr(known), G, W, H, _ptr(out)), "sc_d2_known_i32")
        return out

    @staticmethod
    def _frontier_out(shape, G, Cmax, empty, i32, i64, want_label=True, want_slot=True, want_stats=True):
        return dict(label=empty(shape, i32) if want_label else None, slot=empty(shape, i32) if want_slot else None,
                    ncl=empty((G, 2), i32), rep=empty((G, Cmax), i32), csize=empty((G, Cmax), i32),
                    cbox=empty((G, Cmax, 4), i32) if want_stats else None, csum=empty((G, Cmax, 2), i64) if want_stats else None)

    def frontiers(self, d2, known, r2=0, min_size=1, Cmax=128, want_label=True, want_slot=True, want_stats=True, out=None):
        """Frontier cells and their 8-connected clusters (sc_frontier_batch; the definition is in include/sea_current_hip.h).
        d2 int32 and known uint8, [H,W] or [G,H,W] on the GPU.  Returns dict(label, slot int32 shaped like d2 (None without
        want_label / want_slot), ncl int32 [G,2] = (listed, all), rep, csize int32 [G,Cmax], cbox int32 [G,Cmax,4] and csum int64
        [G,Cmax,2] (None without want_stats)).  `out`: the dict of an earlier call with the same shapes.  Only enqueues."""
        import torch
        G, H, W = _ghw(d2)
        if out is None:
            out = self._frontier_out(tuple(d2.shape), G, Cmax, lambda s, t: torch.empty(s, dtype=t, device=d2.device), torch.int32, torch.int64,
                                     want_label, want_slot, want_stats)
        self._ck(self._l.sc_frontier_batch(self._h, _ptr(d2), _ptr(known), G, W, H, r2, min_size, Cmax, _ptr(out["label"]), _ptr(out["slot"]),
                                           _ptr(out["ncl"]), _ptr(out["rep"]), _ptr(out["csize"]), _ptr(out["cbox"]), _ptr(out["csum"])),
                 "sc_frontier_batch")
        return out

    def frontier_cost_matrix(self, g, fr, gain=0, size_cap=0, fgrid=None):
        """The robots x clusters matrix (sc_frontier_cost_matrix): g int32 [F,H,W] fields rooted at the robots, fr the dict of
        frontiers (its slot and csize), fgrid int32 [F] (None only with one grid).  Returns dict(cost, cell int32 [F,Cmax]):
        assign's layout.  Only enqueues."""
        import torch
        F, H, W = g.shape
        G, Cmax = fr["csize"].shape
        out = dict(cost=torch.empty((F, Cmax), dtype=torch.int32, device=g.device), cell=torch.empty((F, Cmax), dtype=torch.int32, device=g.device))
        self._ck(self._l.sc_frontier_cost_matrix(self._h, _ptr(g), F, _ptr(fgrid), _ptr(fr["slot"]), _ptr(fr["csize"]), G, W, H, Cmax, gain,
                                                 size_cap, _ptr(out["cost"]), _ptr(out["cell"])), "sc_frontier_cost_matrix")
        return out

    def fleet_explore(self, d2, known, g, r2=0, min_size=1, Cmax=128, gain=0, size_cap=0, want_all=False):
        """A frontier goal per robot (sc_fleet_explore_batch): frontiers of (d2, known) [H,W], the matrix of the robots' fields g
        int32 [F,H,W], an optimal matching.  Returns dict(goal int32 [F]: the cell to drive to or -1, gcost int32 [F]); with
        want_all also every intermediate array (frontiers' without the leading G, cost, cell, col_of, row_of, info).  goal is what
        field_paths takes as targets with qfield = arange(F).  Only enqueues."""
        import torch
        H, W = d2.shape
        F = g.shape[0]
        dev = d2.device
        e = lambda s, t=torch.int32: torch.empty(s, dtype=t, device=dev)
        out = dict(goal=e(F), gcost=e(F))
        if want_all:
            out.update(label=e((H, W)), slot=e((H, W)), ncl=e(2), rep=e(Cmax), csize=e(Cmax), cbox=e((Cmax, 4)), csum=e((Cmax, 2), torch.int64),
                       cost=e((F, Cmax)), cell=e((F, Cmax)), col_of=e(F), row_of=e(Cmax), info=e(4, torch.int64))
        self._ck(self._l.sc_fleet_explore_batch(self._h, _ptr(d2), _ptr(known), W, H, r2, min_size, Cmax, _ptr(g), F, gain, size_cap,
                                                *(_ptr(out.get(k)) for k in ("label", "slot", "ncl", "rep", "csize", "cbox", "csum", "cost",
                                                                             "cell", "col_of", "row_of", "info")),
                                                _ptr(out["goal"]), _ptr(out["gcost"])), "sc_fleet_explore_batch")
        return out

    def known_from_discs_host(self, discs, W, H, base=None):
        """Host form of known_from_discs (numpy in, numpy out)."""
        discs = np.ascontiguousarray(discs, dtype=np.int32).reshape(-1, 3)
        base = None if base is None else np.ascontiguousarray(base, dtype=np.uint8)
        out = np.zeros((H, W), np.uint8)
        self._ck(self._l.sc_known_from_discs_host(self._h, _ptr(base), _ptr(discs), discs.shape[0], W, H, _ptr(out)), "sc_known_from_discs_host")
        return out

    def d2_known_host(self, d2, known):
        """Host form of d2_known (numpy in, numpy out)."""
        d2, known = np.ascontiguousarray(d2, dtype=np.int32), np.ascontiguousarray(known, dtype=np.uint8)
        G, H, W = _ghw(d2)
        out = np.zeros_like(d2)
        self._ck(self._l.sc_d2_known_i32_host(self._h, _ptr(d2), _ptr(known), G, W, H, _ptr(out)), "sc_d2_known_i32_host")
        return out

    def frontiers_host(self, d2, known, r2=0, min_size=1, Cmax=128, want_label=True, want_slot=True, want_stats=True):
        """Host form of frontiers (numpy in, numpy out)."""
        d2, known = np.ascontiguousarray(d2, dtype=np.int32), np.ascontiguousarray(known, dtype=np.uint8)
        G, H, W = _ghw(d2)
        out = self._frontier_out(d2.shape, G, Cmax, lambda s, t: np.zeros(s, t), np.int32, np.int64, want_label, want_slot, want_stats)
        self._ck(self._l.sc_frontier_batch_host(self._h, _ptr(d2), _ptr(known), G, W, H, r2, min_size, Cmax, _ptr(out["label"]),
                                                _ptr(out["slot"]), _ptr(out["ncl"]), _ptr(out["rep"]), _ptr(out["csize"]), _ptr(out["cbox"]),
                                                _ptr(out["csum"])), "sc_frontier_batch_host")
        return out

    def frontier_cost_matrix_host(self, g, fr, gain=0, size_cap=0, fgrid=None):
        """Host form of frontier_cost_matrix (numpy in, numpy out)."""
        g = np.ascontiguousarray(g, dtype=np.int32)
        slot, csize = np.ascontiguousarray(fr["slot"], dtype=np.int32), np.ascontiguousarray(fr["csize"], dtype=np.int32)
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        F, H, W = g.shape
        G, Cmax = csize.shape
        out = dict(cost=np.zeros((F, Cmax), np.int32), cell=np.zeros((F, Cmax), np.int32))
        self._ck(self._l.sc_frontier_cost_matrix_host(self._h, _ptr(g), F, _ptr(fgrid), _ptr(slot), _ptr(csize), G, W, H, Cmax, gain, size_cap,
                                                      _ptr(out["cost"]), _ptr(out["cell"])), "sc_frontier_cost_matrix_host")
        return out

    def fleet_explore_host(self, d2, known, g, r2=0, min_size=1, Cmax=128, gain=0, size_cap=0, want_all=False):
        """Host form of fleet_explore (numpy in, numpy out)."""
        d2, known = np.ascontiguousarray(d2, dtype=np.int32), np.ascontiguousarray(known, dtype=np.uint8)
        g = np.ascontiguousarray(g, dtype=np.int32)
        H, W = d2.shape
        F = g.shape[0]
        z = lambda s, t=np.int32: np.zeros(s, t)
        out = dict(goal=z(F), gcost=z(F))
        if want_all:
            out.update(label=z((H, W)), slot=z((H, W)), ncl=z(2), rep=z(Cmax), csize=z(Cmax), cbox=z((Cmax, 4)), csum=z((Cmax, 2), np.int64),
                       cost=z((F, Cmax)), cell=z((F, Cmax)), col_of=z(F), row_of=z(Cmax), info=z(4, np.int64))
        self._ck(self._l.sc_fleet_explore_batch_host(self._h, _ptr(d2), _ptr(known), W, H, r2, min_size, Cmax, _ptr(g), F, gain, size_cap,
                                                     *(_ptr(out.get(k)) for k in ("label", "slot", "ncl", "rep", "csize", "cbox", "csum",
                                                                                  "cost", "cell", "col_of", "row_of", "info")),
                                                     _ptr(out["goal"]), _ptr(out["gcost"])), "sc_fleet_explore_batch_host")
        return out

    # ---- multi-GPU gather (RCCL through the C ABI) ----
    @staticmethod
    def comm_unique_id():
        """128 bytes of an ncclUniqueId (call on one rank, hand to all)."""
        buf = C.create_string_buffer(128)
        st = lib().sc_comm_unique_id(buf)
        if st != 0:
            raise SeaCurrentError(f"sc_comm_unique_id: {lib().sc_status_string(st).decode()}")
        return buf.raw

    def comm_init(self, unique_id, world, rank):
        self._ck(self._l.sc_comm_init(self._h, C.c_char_p(unique_id), world, rank), "sc_comm_init")
        self.world, self.rank = world, rank

    def allgather_paths(self, out, Q_total, cap_cells, want_path=False, bufs=None):
        """Every rank's astar_batch results on every rank, in query order (sc_allgather_paths).  `out` = this rank's dict;
        returns dict(len, cost, status [Q_total], offsets int64 [Q_total+1], cells [world*cap_cells], truncated [1], path?)."""
        import torch
        dev = out["len"].device
        Ql, Lmax = out["path"].shape
        world = getattr(self, "world", 1)
        if bufs is None:
            bufs = dict(len=torch.empty(Q_total, dtype=torch.int32, device=dev), cost=torch.empty(Q_total, dtype=torch.int32, device=dev),
                        status=torch.empty(Q_total, dtype=torch.int32, device=dev),
                        offsets=torch.empty(Q_total + 1, dtype=torch.int64, device=dev),
                        cells=torch.empty(world * cap_cells, dtype=torch.int32, device=dev),
                        truncated=torch.zeros(1, dtype=torch.int32, device=dev))
            if want_path:
                bufs["path"] = torch.empty((Q_total, Lmax), dtype=torch.int32, device=dev)
        self._ck(self._l.sc_allgather_paths(self._h, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]), _ptr(out["status"]), Ql, Q_total, Lmax,
                                            cap_cells, _ptr(bufs["len"]), _ptr(bufs["cost"]), _ptr(bufs["status"]), _ptr(bufs["offsets"]),
                                            _ptr(bufs["cells"]), bufs["cells"].numel(), _ptr(bufs.get("path")), _ptr(bufs["truncated"])),
                 "sc_allgather_paths")
        return bufs

    def gather_pack(self, out, Q_total, world, rank, cap_cells, msg=None, Lmax=None):
        """This rank's message of the gather (sc_gather_pack): int32 [sc_gather_msg_words].  `out` = the rank's astar_batch
        dict (may hold zero queries)."""
        import torch
        Ql = int(out["len"].shape[0])
        if Lmax is None:
            Lmax = int(out["path"].shape[1])
        words = int(self._l.sc_gather_msg_words(Q_total, world, cap_cells))
        if msg is None:
            msg = torch.empty(words, dtype=torch.int32, device=out["len"].device)
        assert msg.numel() == words
        nz = Ql > 0
        self._ck(self._l.sc_gather_pack(self._h, _ptr(out["path"]) if nz else None, _ptr(out["len"]) if nz else None,
                                        _ptr(out["cost"]) if nz else None, _ptr(out["status"]) if nz else None, Ql, Q_total, world, rank,
                                        Lmax, cap_cells, _ptr(msg)), "sc_gather_pack")
        return msg

    def gather_unpack(self, msgs, world, Q_total, Lmax, cap_cells, want_path=False, cells_capacity=None):
        """sc_gather_unpack: `msgs` = the world messages back to back in rank order -> the dict allgather_paths returns."""
        import torch
        dev = msgs.device
        cc = world * cap_cells if cells_capacity is None else cells_capacity
        bufs = dict(len=torch.empty(Q_total, dtype=torch.int32, device=dev), cost=torch.empty(Q_total, dtype=torch.int32, device=dev),
                    status=torch.empty(Q_total, dtype=torch.int32, device=dev), offsets=torch.empty(Q_total + 1, dtype=torch.int64, device=dev),
                    cells=torch.full((cc,), -7, dtype=torch.int32, device=dev), truncated=torch.zeros(1, dtype=torch.int32, device=dev))
        if want_path:
            bufs["path"] = torch.full((Q_total, Lmax), -7, dtype=torch.int32, device=dev)
        self._ck(self._l.sc_gather_unpack(self._h, _ptr(msgs), world, Q_total, Lmax, cap_cells, _ptr(bufs["len"]), _ptr(bufs["cost"]),
                                          _ptr(bufs["status"]), _ptr(bufs["offsets"]), _ptr(bufs["cells"]), cc, _ptr(bufs.get("path")),
                                          _ptr(bufs["truncated"])), "sc_gather_unpack")
        return bufs

    def allgather_last_bytes(self):
        n = C.c_int64()
        self._ck(self._l.sc_allgather_last_bytes(self._h, C.byref(n)), "sc_allgather_last_bytes")
        return n.value

    def astar_last_expansions(self):
        n = C.c_int64(0)
        self._ck(self._l.sc_astar_last_expansions(self._h, C.byref(n)), "sc_astar_last_expansions")
        return n.value

    def astar_debug_stats(self, Q):
        """Per-query (expansions, popped entries, kilo-cycles, steps) of the last astar_batch (synchronises)."""
        out = np.zeros((4, Q), dtype=np.int32)
        self._ck(self._l.sc_astar_debug_stats(self._h, _ptr(out), Q), "sc_astar_debug_stats")
        return out[0], out[1], out[2], out[3]

    def astar_gfield(self, d2, start, goal, r2=0):
        import torch
        H, W = d2.shape
        g = torch.empty((H, W), dtype=torch.int32, device=d2.device)
        cs = torch.empty(2, dtype=torch.int32, device=d2.device)
        self._ck(self._l.sc_astar_gfield(self._h, _ptr(d2), W, H, r2, int(start), int(goal), _ptr(g),
                                         cs.data_ptr(), cs.data_ptr() + 4), "sc_astar_gfield")
        self.synchronize()
        cost, status = cs.cpu().tolist()
        if status == Q_TRUNCATED:  # the path itself is not requested (Lmax = 1)
            status = Q_OK
        return g.cpu().numpy().view(np.uint32), cost, status

    def toppra(self, p0, p1, v0, v1, vlim_lo, vlim_hi, alim_lo, alim_hi, N=100, sd_start=0.0, sd_end=0.0):
        """All inputs float64 GPU tensors [P,dof] (vlim may be [P,N+1,dof])."""
        import torch
        P, dof = p0.shape
        per_stage = int(vlim_lo.dim() == 3)
        dev = p0.device
        out = dict(K=torch.empty((P, N + 1, 2), dtype=torch.float64, device=dev),
                   x=torch.empty((P, N + 1), dtype=torch.float64, device=dev),
                   u=torch.empty((P, N), dtype=torch.float64, device=dev),
                   t=torch.empty((P, N + 1), dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_toppra_hermite_batch(self._h, P, dof, N, _ptr(p0), _ptr(p1), _ptr(v0), _ptr(v1),
                                                 _ptr(vlim_lo), _ptr(vlim_hi), per_stage, _ptr(alim_lo), _ptr(alim_hi),
                                                 sd_start, sd_end, _ptr(out["K"]), _ptr(out["x"]), _ptr(out["u"]),
                                                 _ptr(out["t"]), _ptr(out["status"])), "sc_toppra_hermite_batch")
        return out

    def toppra_sample(self, p0, p1, v0, v1, x, t, dt, max_len):
        import torch
        P, dof = p0.shape
        N = x.shape[1] - 1
        dev = p0.device
        out = dict(pos=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   vel=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   acc=torch.zeros((P, dof, max_len), dtype=torch.float32, device=dev),
                   time=torch.zeros((P, max_len), dtype=torch.float64, device=dev),
                   length=torch.empty(P, dtype=torch.int32, device=dev))
        self._ck(self._l.sc_toppra_sample_batch(self._h, P, dof, N, _ptr(p0), _ptr(p1), _ptr(v0), _ptr(v1), _ptr(x),
                                                _ptr(t), float(dt), max_len, _ptr(out["pos"]), _ptr(out["vel"]),
                                                _ptr(out["acc"]), _ptr(out["time"]), _ptr(out["length"])),
                 "sc_toppra_sample_batch")
        return out

    def fmt_star(self, samples, starts, goals, rn, lines, Lmax=256):
        """FMT* (the reference's planner) for Q queries over shared samples.  GPU float32 tensors: samples [n,2], starts / goals
        [Q,2], lines [E,4] -> dict(path [Q,Lmax,2], len, cost, status)."""
        import torch
        Q = starts.shape[0]
        dev = starts.device
        out = dict(path=torch.zeros((Q, Lmax, 2), dtype=torch.float32, device=dev), len=torch.zeros(Q, dtype=torch.int32, device=dev),
                   cost=torch.zeros(Q, dtype=torch.float32, device=dev), status=torch.zeros(Q, dtype=torch.int32, device=dev))
        E = 0 if lines is None else lines.shape[0]
        self._ck(self._l.sc_fmt_star_batch(self._h, _ptr(samples), samples.shape[0], _ptr(starts), _ptr(goals), Q, float(rn),
                                           _ptr(lines) if E else None, E, Lmax, _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]),
                                           _ptr(out["status"])), "sc_fmt_star_batch")
        return out

    def edt_nearest(self, occ, d2):
        """occ uint8 [B,H,W] or [H,W] and its d2 (GPU) -> int32 index of the nearest occupied cell per cell (-1: none)."""
        import torch
        o3 = occ if occ.dim() == 3 else occ[None]
        B, H, W = o3.shape
        out = torch.empty((B, H, W), dtype=torch.int32, device=occ.device)
        self._ck(self._l.sc_edt_nearest_i32(self._h, _ptr(o3), _ptr(d2), W, H, B, _ptr(out)), "sc_edt_nearest_i32")
        return out if occ.dim() == 3 else out[0]

    def occ_from_rects(self, rects, W, H, base=None, free_border=True, out=None):
        """rects int32 [R,4] (x0,y0,x1,y1 exclusive; GPU) painted over `base` uint8 [H,W] (or an empty grid) -> occ uint8 [H,W]."""
        import torch
        occ = out if out is not None else torch.empty((H, W), dtype=torch.uint8, device=rects.device)
        self._ck(self._l.sc_occ_from_rects(self._h, _ptr(base) if base is not None else None, _ptr(rects), rects.shape[0], W, H,
                                           1 if free_border else 0, _ptr(occ)), "sc_occ_from_rects")
        return occ

    def occ_from_polygons(self, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed=None, box=None, grid_off=None, base=None,
                          out=None):
        """Polygon obstacles -> occupancy grids (sc_occ_from_polygons), GPU tensors: lines float32 [E,4] (x0,y0,x1,y1),
        obs_off int32 [n_obs+1], closed uint8 [n_obs] (None: all closed), box float32 [n_obs,4] in bound_rect order
        (x_max, x_min, y_max, y_min; None: each obstacle's own lines), grid_off int32 [G+1] (None: one grid).  Returns uint8
        [H,W] without grid_off, else [G,H,W]; base (same shape) is painted over, base is out paints in place."""
        import torch
        G = 1 if grid_off is None else grid_off.shape[0] - 1
        shape = (H, W) if grid_off is None else (G, H, W)
        occ = out if out is not None else torch.empty(shape, dtype=torch.uint8, device=obs_off.device)
        n_obs = obs_off.shape[0] - 1
        self._ck(self._l.sc_occ_from_polygons(self._h, _ptr(base), G, W, H, x_min, y_min, res_x, res_y,
                                              _ptr(lines) if lines.shape[0] else None, lines.shape[0], _ptr(obs_off), n_obs,
                                              _ptr(box), _ptr(closed), _ptr(grid_off), _ptr(occ)), "sc_occ_from_polygons")
        return occ

    def bezier_from_path(self, path, npts, start_angle=float("nan"), lines=None):
        """path float32 [P,n_max,2], npts int32 [P] (GPU) -> ctrl float32 [P,n_max-1,4,2]."""
        import torch
        P, n_max, _ = path.shape
        ctrl = torch.empty((P, n_max - 1, 4, 2), dtype=torch.float32, device=path.device)
        nl = 0 if lines is None else lines.shape[0]
        self._ck(self._l.sc_bezier_from_path_batch(self._h, _ptr(path), _ptr(npts), P, n_max, start_angle,
                                                   _ptr(lines) if nl else None, nl, _ptr(ctrl)), "sc_bezier_from_path_batch")
        return ctrl

    def bezier_eval(self, ctrl, seg, t, order=0):
        import torch
        M = t.shape[0]
        out = torch.empty((M, 2), dtype=torch.float32, device=t.device)
        self._ck(self._l.sc_bezier_eval_batch(self._h, _ptr(ctrl), _ptr(seg), _ptr(t), M, order, _ptr(out)), "sc_bezier_eval_batch")
        return out

    def bezier_curve(self, ctrl, seg, t):
        """General degree: ctrl float32 [S, degree+1, 2] (GPU), seg int32 [M], t float32 [M] -> points float32 [M, 2]."""
        import torch
        M = t.shape[0]
        out = torch.empty((M, 2), dtype=torch.float32, device=t.device)
        self._ck(self._l.sc_bezier_curve_batch(self._h, _ptr(ctrl), ctrl.shape[1] - 1, _ptr(seg), _ptr(t), M, _ptr(out)), "sc_bezier_curve_batch")
        return out

    def chebfit(self, x, y, off, degree):
        """B least-squares Chebyshev fits; x, y float32 [total], off int32 [B+1] (all GPU) -> (coef [B, degree], xrange [B, 2])."""
        import torch
        B = off.shape[0] - 1
        coef = torch.empty((B, degree), dtype=torch.float32, device=x.device)
        xr = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        self._ck(self._l.sc_chebfit_batch(self._h, _ptr(x), _ptr(y), _ptr(off), B, x.shape[0], degree, _ptr(coef), _ptr(xr)), "sc_chebfit_batch")
        return coef, xr

    def chebeval(self, x, off, coef, xr):
        import torch
        B, degree = coef.shape
        y = torch.empty_like(x)
        self._ck(self._l.sc_chebeval_batch(self._h, _ptr(x), _ptr(off), B, degree, _ptr(coef), _ptr(xr), _ptr(y)), "sc_chebeval_batch")
        return y

    def bezier_arclength(self, ctrl, nsub=100):
        """ctrl float32 [...,4,2] (GPU) -> (cum float32 [S,nsub+1], seg_len float32 [S])."""
        import torch
        c = ctrl.reshape(-1, 4, 2)
        S = c.shape[0]
        cum = torch.empty((S, nsub + 1), dtype=torch.float32, device=ctrl.device)
        seg_len = torch.empty(S, dtype=torch.float32, device=ctrl.device)
        self._ck(self._l.sc_bezier_arclength_batch(self._h, _ptr(c), S, nsub, _ptr(cum), _ptr(seg_len)), "sc_bezier_arclength_batch")
        return cum, seg_len

    def bezier_resample(self, ctrl, cum, arclength, seg_off, profile_pos, prof_off, nudge=True, want_curvature=True):
        """B splines (GPU tensors): ctrl float32 [S,4,2], cum float32 [S,nsub+1], arclength float32 [B], seg_off int32 [B+1],
        profile_pos float32 [M] (nudged IN PLACE when `nudge`), prof_off int32 [B+1] -> dict(pts [M,2], t [M], seg [M],
        curvature [M], status [B])."""
        import torch
        S, m = cum.shape
        B = arclength.shape[0]
        M = profile_pos.shape[0]
        dev = profile_pos.device
        out = dict(pts=torch.zeros((M, 2), dtype=torch.float32, device=dev), t=torch.zeros(M, dtype=torch.float32, device=dev),
                   seg=torch.zeros(M, dtype=torch.int32, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev),
                   curvature=torch.zeros(M, dtype=torch.float32, device=dev) if want_curvature else None)
        self._ck(self._l.sc_bezier_resample_batch(self._h, _ptr(ctrl), _ptr(cum), _ptr(arclength), _ptr(seg_off), B, S, m - 1,
                                                  _ptr(profile_pos), _ptr(prof_off), 1 if nudge else 0, _ptr(out["pts"]), _ptr(out["t"]),
                                                  _ptr(out["seg"]), _ptr(out["curvature"]) if want_curvature else None,
                                                  _ptr(out["status"])), "sc_bezier_resample_batch")
        return out

    # -- host-pointer entry points (numpy)
    def edt_host(self, occ):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        o3 = occ if occ.ndim == 3 else occ[None]
        B, H, W = o3.shape
        d2 = np.empty(o3.shape, dtype=np.int32)
        self._ck(self._l.sc_edt_u8_i32_host(self._h, _ptr(o3), W, H, B, _ptr(d2)), "sc_edt_u8_i32_host")
        return d2 if occ.ndim == 3 else d2[0]

    def occ_from_polygons_host(self, lines, obs_off, W, H, x_min, y_min, res_x, res_y, closed=None, box=None, grid_off=None,
                               base=None):
        """Host form of occ_from_polygons (numpy in, numpy out; sc_occ_from_polygons_host checks the contract first)."""
        lines = np.ascontiguousarray(lines, dtype=np.float32).reshape(-1, 4)
        obs_off = np.ascontiguousarray(obs_off, dtype=np.int32)
        closed = None if closed is None else np.ascontiguousarray(closed, dtype=np.uint8)
        box = None if box is None else np.ascontiguousarray(box, dtype=np.float32).reshape(-1, 4)
        grid_off = None if grid_off is None else np.ascontiguousarray(grid_off, dtype=np.int32)
        G = 1 if grid_off is None else grid_off.shape[0] - 1
        shape = (H, W) if grid_off is None else (G, H, W)
        occ = np.zeros(shape, np.uint8) if base is None else np.array(base, dtype=np.uint8, copy=True).reshape(shape)
        self._ck(self._l.sc_occ_from_polygons_host(self._h, _ptr(occ) if base is not None else None, G, W, H, x_min, y_min, res_x,
                                                   res_y, _ptr(lines) if lines.shape[0] else None, lines.shape[0], _ptr(obs_off),
                                                   obs_off.shape[0] - 1, _ptr(box), _ptr(closed), _ptr(grid_off), _ptr(occ)),
                 "sc_occ_from_polygons_host")
        return occ

    def astar_batch_host(self, d2, start, goal, r2=0, Lmax=4096):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        goal = np.ascontiguousarray(goal, dtype=np.int32)
        H, W = d2.shape
        Q = start.shape[0]
        out = dict(path=np.full((Q, Lmax), -1, dtype=np.int32), len=np.zeros(Q, np.int32),
                   cost=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
        self._ck(self._l.sc_astar_batch_host(self._h, _ptr(d2), W, H, r2, _ptr(start), _ptr(goal), Q, Lmax,
                                             _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]),
                                             _ptr(out["status"])), "sc_astar_batch_host")
        return out

    def components_host(self, d2, r2=0, want_size=False):
        """Host form of components (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        G, H, W = (1,) + d2.shape if d2.ndim == 2 else d2.shape
        out = dict(label=np.zeros(d2.shape, np.int32), size=np.zeros(d2.shape, np.int32) if want_size else None,
                   ncomp=np.zeros(G, np.int32), largest=np.zeros(G, np.int32))
        self._ck(self._l.sc_components_batch_host(self._h, _ptr(d2), G, W, H, r2, _ptr(out["label"]), _ptr(out["size"]), _ptr(out["ncomp"]),
                                                  _ptr(out["largest"])), "sc_components_batch_host")
        return out

    def reachable_host(self, label, start, goal, qgrid=None):
        """Host form of reachable (numpy in, numpy out)."""
        label = np.ascontiguousarray(label, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        goal = np.ascontiguousarray(goal, dtype=np.int32)
        qgrid = None if qgrid is None else np.ascontiguousarray(qgrid, dtype=np.int32)
        G, H, W = (1,) + label.shape if label.ndim == 2 else label.shape
        Q = start.shape[0]
        status = np.zeros(Q, np.int32)
        self._ck(self._l.sc_reachable_batch_host(self._h, _ptr(label), G, _ptr(qgrid), W, H, _ptr(start), _ptr(goal), Q, _ptr(status)),
                 "sc_reachable_batch_host")
        return status

    def clearance_penalty_host(self, d2, r2=0, r2_soft=36, pen_max=40):
        """Host form of clearance_penalty (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        G, H, W = (1,) + d2.shape if d2.ndim == 2 else d2.shape
        out = np.zeros(d2.shape, np.uint8)
        self._ck(self._l.sc_clearance_penalty_u8_host(self._h, _ptr(d2), W, H, G, r2, r2_soft, pen_max, _ptr(out)),
                 "sc_clearance_penalty_u8_host")
        return out

    def cost_fields_host(self, d2, roots, r2=0, fgrid=None, rounds=-1, pen=None, pen_cap=255):
        """Host form of cost_fields (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        roots = np.ascontiguousarray(roots, dtype=np.int32)
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        pen = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint8)
        G, H, W = _ghw(d2)
        F = roots.shape[0]
        out = dict(g=np.zeros((F, H, W), np.int32), status=np.zeros(F, np.int32))
        name, costmap = _field_entry("sc_cost_field", pen, pen_cap, host=True)
        self._ck(getattr(self._l, name)(self._h, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(roots), F, rounds, _ptr(out["g"]),
                                        _ptr(out["status"])), name)
        return out

    def field_paths_host(self, d2, g, roots, qfield, targets, r2=0, Lmax=4096, to_root=False, fgrid=None, pen=None, pen_cap=255):
        """Host form of field_paths (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        g = np.ascontiguousarray(g, dtype=np.int32)
        roots, qfield, targets = (np.ascontiguousarray(a, dtype=np.int32) for a in (roots, qfield, targets))
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        pen = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint8)
        G, H, W = _ghw(d2)
        F, Q = roots.shape[0], targets.shape[0]
        out = _paths_out_numpy(Q, Lmax)
        name, costmap = _field_entry("sc_field_paths", pen, pen_cap, host=True)
        self._ck(getattr(self._l, name)(self._h, _ptr(d2), *costmap, G, _ptr(fgrid), W, H, r2, _ptr(g), _ptr(roots), F, _ptr(qfield),
                                        _ptr(targets), Q, Lmax, int(bool(to_root)), _ptr(out["path"]), _ptr(out["len"]),
                                        _ptr(out["cost"]), _ptr(out["status"])), name)
        return out

    def cost_fields_multi_host(self, d2, seeds, seed_off, seed_cost=None, r2=0, fgrid=None, rounds=-1, want_owner=True, pen=None,
                               pen_cap=255):
        """Host form of cost_fields_multi (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        seeds, seed_off = (np.ascontiguousarray(a, dtype=np.int32) for a in (seeds, seed_off))
        seed_cost = None if seed_cost is None else np.ascontiguousarray(seed_cost, dtype=np.int32)
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        pen = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint8)
        G, H, W = _ghw(d2)
        F = seed_off.shape[0] - 1
        out = dict(g=np.zeros((F, H, W), np.int32), owner=np.zeros((F, H, W), np.int32) if want_owner else None, status=np.zeros(F, np.int32))
        self._ck(self._l.sc_cost_field_multi_batch_host(self._h, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(seeds),
                                                        _ptr(seed_cost), _ptr(seed_off), seeds.shape[0], F, rounds, _ptr(out["g"]),
                                                        _ptr(out["owner"]), _ptr(out["status"])), "sc_cost_field_multi_batch_host")
        return out

    def field_paths_multi_host(self, d2, fields, seeds, qfield, targets, r2=0, Lmax=4096, to_seed=False, fgrid=None, pen=None, pen_cap=255):
        """Host form of field_paths_multi (numpy in, numpy out)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        g, owner = (np.ascontiguousarray(fields[k], dtype=np.int32) for k in ("g", "owner"))
        seeds, qfield, targets = (np.ascontiguousarray(a, dtype=np.int32) for a in (seeds, qfield, targets))
        fgrid = None if fgrid is None else np.ascontiguousarray(fgrid, dtype=np.int32)
        pen = None if pen is None else np.ascontiguousarray(pen, dtype=np.uint8)
        G, H, W = _ghw(d2)
        F, Q = g.shape[0], targets.shape[0]
        out = _paths_out_numpy(Q, Lmax, which=True)
        self._ck(self._l.sc_field_paths_multi_batch_host(self._h, _ptr(d2), _ptr(pen), pen_cap, G, _ptr(fgrid), W, H, r2, _ptr(g), _ptr(owner),
                                                         _ptr(seeds), seeds.shape[0], F, _ptr(qfield), _ptr(targets), Q, Lmax,
                                                         int(bool(to_seed)), _ptr(out["path"]), _ptr(out["len"]), _ptr(out["cost"]),
                                                         _ptr(out["status"]), _ptr(out["which"])), "sc_field_paths_multi_batch_host")
        return out

    def path_waypoints_host(self, d2, path, lens, status=None, r2=0, Wmax=None):
        """Host form of path_waypoints (numpy in, numpy out): path int32 [Q,Lmax], lens / status int32 [Q] (status may be None)."""
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        path = np.ascontiguousarray(path, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        H, W = d2.shape
        Q, Lmax = path.shape
        Wmax = Lmax if Wmax is None else Wmax
        out = dict(wp=np.full((Q, Wmax), -1, dtype=np.int32), n=np.zeros(Q, np.int32), status=np.zeros(Q, np.int32))
        self._ck(self._l.sc_path_waypoints_batch_host(self._h, _ptr(d2), W, H, r2, _ptr(path), _ptr(lens), _ptr(status), Q, Lmax, Wmax,
                                                      _ptr(out["wp"]), _ptr(out["n"]), _ptr(out["status"])), "sc_path_waypoints_batch_host")
        return out
