"""ctypes mirror of include/gpmp2mi.h: POD structs + helpers that marshal numpy arrays.

Only the structs and marshalling live here; the product library is loaded by `engine.py`.
(The test-only CPU oracle re-uses these structs through tests/oracle.py -- it is never imported
from this package.)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)

OPT_GAUSS_NEWTON, OPT_LM, OPT_DOGLEG = 0, 1, 2
SDF_LAYOUT_ZYX, SDF_LAYOUT_GTSAM = 0, 1
MAX_DOF = 10
MAX_SPHERES = 64

STATUS_NAMES = {0: "converged", 1: "max_iter", 2: "rolled_back", 3: "not_spd", 4: "already_optimal"}


class RobotDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("dof", C.c_int), ("arm_dof", C.c_int),
                ("a", c_double_p), ("alpha", c_double_p), ("d", c_double_p),
                ("theta_bias", c_double_p), ("base_pose", C.c_double * 16),
                ("nr_spheres", C.c_int), ("sphere_link", c_int_p),
                ("sphere_radius", c_double_p), ("sphere_center", c_double_p),
                ("arm2_dof", C.c_int), ("base_pose2", C.c_double * 16), ("base_pose3", C.c_double * 16),
                ("reverse_linact", C.c_int)]


class Settings(C.Structure):
    _fields_ = [("dof", C.c_int), ("total_step", C.c_int), ("total_time", C.c_double),
                ("conf_prior_sigma", C.c_double), ("vel_prior_sigma", C.c_double),
                ("flag_pos_limit", C.c_int), ("flag_vel_limit", C.c_int),
                ("joint_pos_limits_up", c_double_p), ("joint_pos_limits_down", c_double_p),
                ("vel_limits", c_double_p), ("pos_limit_thresh", c_double_p),
                ("vel_limit_thresh", c_double_p), ("pos_limit_sigmas", c_double_p),
                ("vel_limit_sigmas", c_double_p),
                ("epsilon", C.c_double), ("cost_sigma", C.c_double), ("obs_check_inter", C.c_int),
                ("Qc", c_double_p), ("opt_type", C.c_int), ("verbosity", C.c_int),
                ("final_iter_no_increase", C.c_int), ("rel_thresh", C.c_double),
                ("max_iter", C.c_int)]


MAX_WORKSPACE_FACTORS, MAX_SELF_COLLISION_PAIRS = 4, 16
MAX_MOVING_SPHERES = 64
MAX_CARRIED_SPHERES = 256    # GPMP2MI_MAX_CARRIED_SPHERES
HEADER_MAX_SPHERES = 96   # GPMP2MI_MAX_SPHERES
MAX_PLAN_SELF_PAIRS = HEADER_MAX_SPHERES * (HEADER_MAX_SPHERES - 1) // 2   # GPMP2MI_MAX_PLAN_SELF_PAIRS
WORKSPACE_POSITION, WORKSPACE_ORIENTATION, WORKSPACE_POSE = 0, 1, 2


class WorkspaceFactor(C.Structure):
    _fields_ = [("mode", C.c_int), ("link", C.c_int), ("first_state", C.c_int), ("last_state", C.c_int),
                ("sigma", C.c_double), ("des_pose", C.c_double * 16)]


class GraphOpts(C.Structure):
    _fields_ = [("obs_skip_first_state", C.c_int), ("vehicle_dynamics_sigma", C.c_double),
                ("lm_lambda_initial", C.c_double), ("lm_lambda_factor", C.c_double),
                ("lm_lambda_upper", C.c_double), ("lm_lambda_lower", C.c_double),
                ("lm_min_model_fidelity", C.c_double), ("dogleg_delta_initial", C.c_double),
                ("abs_error_tol", C.c_double), ("error_tol", C.c_double),
                ("fixed_iterations", C.c_int),
                ("end_conf_prior_off", C.c_int), ("n_workspace", C.c_int),
                ("workspace", WorkspaceFactor * MAX_WORKSPACE_FACTORS),
                ("n_self_collision", C.c_int), ("self_collision_first", C.c_int), ("self_collision_last", C.c_int),
                ("self_collision", (C.c_double * 4) * MAX_SELF_COLLISION_PAIRS),
                ("max_carried_spheres", C.c_int), ("carried_first", C.c_int), ("carried_last", C.c_int),
                ("carried_epsilon", C.c_double), ("carried_sigma", C.c_double),
                ("workspace_path", C.c_int), ("workspace_path_mode", C.c_int), ("workspace_path_link", C.c_int),
                ("max_self_pairs", C.c_int), ("self_pairs_first", C.c_int), ("self_pairs_last", C.c_int),
                ("max_moving_spheres", C.c_int), ("moving_first", C.c_int), ("moving_last", C.c_int),
                ("moving_epsilon", C.c_double), ("moving_sigma", C.c_double)]


class DebugForms(C.Structure):
    """gpmp2mi_debug_forms (include/gpmp2mi_debug.h): kernel forms forced on a plan; all zero = the plan's own choice."""
    _fields_ = [("lin_split", C.c_int), ("no_fused_finish", C.c_int), ("generic_gn", C.c_int), ("wide_dense", C.c_int),
                ("fail_alloc_at", C.c_int), ("no_early_stop", C.c_int)]


def make_debug_forms(forms):
    """DebugForms from a dict such as {"lin_split": 2}; an unknown name raises."""
    unknown = set(forms) - {name for name, _ in DebugForms._fields_}
    if unknown:
        raise ValueError(f"unknown plan forms: {sorted(unknown)}")
    return DebugForms(**{k: int(v) for k, v in forms.items()})


class QueueStats(C.Structure):
    """gpmp2mi_queue_stats (include/gpmp2mi.h)."""
    _fields_ = [("passes", C.c_int), ("slot_passes", C.c_long), ("busy_slot_passes", C.c_long)]


def declare_queue(lib):
    """argtypes of the queue entry points (gpmp2mi_plan_optimize_queue*, gpmp2mi_plan_queue_stats)."""
    vp, i, d = C.c_void_p, C.c_int, c_double_p
    ip = c_int_p
    lib.gpmp2mi_plan_optimize_queue.argtypes = [vp, i, d, d, d, d, d, d, ip, d, ip, d]
    lib.gpmp2mi_plan_optimize_queue.restype = i
    lib.gpmp2mi_plan_optimize_queue_dev.argtypes = [vp, i] + [vp] * 11
    lib.gpmp2mi_plan_optimize_queue_dev.restype = i
    lib.gpmp2mi_plan_queue_stats.argtypes = [vp, C.POINTER(QueueStats)]
    lib.gpmp2mi_plan_queue_stats.restype = i


MAX_SHARDS = 16


def declare_multi(lib):
    """argtypes of the multi-device plan entry points (gpmp2mi_multi_plan_*, include/gpmp2mi.h) and their debug hooks."""
    vp, i, d, ip = C.c_void_p, C.c_int, c_double_p, c_int_p
    lp = C.POINTER(C.c_long)
    decl = {
        "gpmp2mi_multi_plan_create": [vp, vp, vp, vp, i, i, ip, vp],
        "gpmp2mi_debug_multi_plan_create": [vp, vp, vp, vp, i, i, ip, vp, i, vp],
        "gpmp2mi_multi_plan_shards": [vp, ip, ip, ip],
        "gpmp2mi_multi_plan_set_problem": [vp, d, d, d, d, d],
        "gpmp2mi_multi_plan_optimize": [vp],
        "gpmp2mi_multi_plan_get_result": [vp, d, ip, d, ip, d],
        "gpmp2mi_multi_plan_get_result_dev": [vp, i, vp, vp, vp, vp, vp],
        "gpmp2mi_multi_plan_optimize_queue": [vp, i, d, d, d, d, d, d, ip, d, ip, d],
        "gpmp2mi_multi_plan_queue_stats": [vp, i, C.POINTER(QueueStats)],
        "gpmp2mi_debug_replica_counts": [lp, lp],
        "gpmp2mi_debug_current_device": [i, ip],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_multi_plan_destroy.argtypes = [vp]
    lib.gpmp2mi_multi_plan_destroy.restype = None


def declare_score(lib):
    """argtypes of the scoring entry points (include/gpmp2mi.h "scoring").  The host-pointer forms take typed pointers;
    the `_dev` forms take device addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_score_traj": [vp, vp, f, i, i, i, d, d, d, d, ip, ip],
        "gpmp2mi_score_traj_dev": [vp, vp, f, i, i, i] + [vp] * 7,
        "gpmp2mi_select_best": [i, d, ip, d, ip, f, i, ip, ip],
        "gpmp2mi_select_best_dev": [i, vp, vp, vp, vp, f, i, vp, vp, vp],
        "gpmp2mi_plan_score": [vp, i, d, d, d, ip, ip],
        "gpmp2mi_plan_score_dev": [vp, i] + [vp] * 6,
        "gpmp2mi_plan_select": [vp, i, f, i, ip, ip, d, d],
        "gpmp2mi_plan_select_dev": [vp, i, f, i] + [vp] * 5,
        "gpmp2mi_multi_plan_score": [vp, i, d, d, d, ip, ip],
        "gpmp2mi_multi_plan_select": [vp, i, f, i, ip, ip, d, d],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_self(lib):
    """argtypes of the self-collision check (include/gpmp2mi.h "self-collision check"); the `_dev` forms take device
    addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_self_pairs_create": [vp, i, d, vp],
        "gpmp2mi_self_pairs_generate": [vp, i, i, d, f, f, vp],
        "gpmp2mi_self_pairs_count": [vp],
        "gpmp2mi_self_pairs_get": [vp, d],
        "gpmp2mi_self_score_traj": [vp, vp, f, i, i, i, d, d, d, d, ip, ip],
        "gpmp2mi_self_score_traj_dev": [vp, vp, f, i, i, i] + [vp] * 7,
        "gpmp2mi_plan_self_score": [vp, vp, i, d, d, d, ip, ip],
        "gpmp2mi_plan_self_score_dev": [vp, vp, i] + [vp] * 6,
        "gpmp2mi_plan_select_checked": [vp, i, f, i, vp, f, ip, ip, d, d],
        "gpmp2mi_plan_select_checked_dev": [vp, i, f, i, vp, f] + [vp] * 5,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_self_pairs_destroy.argtypes = [vp]
    lib.gpmp2mi_self_pairs_destroy.restype = None


class MotionLimitsC(C.Structure):
    """gpmp2mi_motion_limits (include/gpmp2mi.h "motion limits"): host arrays [dof] or NULL, and the Cartesian speed."""
    _fields_ = [("pos_down", c_double_p), ("pos_up", c_double_p), ("vel", c_double_p), ("acc", c_double_p),
                ("point_speed", C.c_double)]


def declare_motion(lib):
    """argtypes of the motion-limit entry points (include/gpmp2mi.h "motion limits"); `limits` is a host struct in every
    form, the `_dev` forms take device addresses for everything else."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    lp = C.POINTER(MotionLimitsC)
    decl = {
        "gpmp2mi_motion_score_traj": [vp, lp, f, i, i, i, d, d, d, d, d, d, ip, ip],
        "gpmp2mi_motion_score_traj_dev": [vp, lp, f, i, i, i] + [vp] * 9,
        "gpmp2mi_plan_motion_score": [vp, lp, i, d, d, d, d, d, ip, ip],
        "gpmp2mi_plan_motion_score_dev": [vp, lp, i] + [vp] * 8,
        "gpmp2mi_plan_select_feasible": [vp, i, f, i, vp, f, lp, f, f, ip, ip, d, d, d],
        "gpmp2mi_plan_select_feasible_dev": [vp, i, f, i, vp, f, lp, f, f] + [vp] * 6,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_motion_limits_default.argtypes = [lp]
    lib.gpmp2mi_motion_limits_default.restype = None


def declare_retime(lib):
    """argtypes of the re-timing entry points (include/gpmp2mi.h "re-timing"); `limits` and `acc` are host data in every
    form, the `_dev` forms take device addresses for everything else."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    lp = C.POINTER(MotionLimitsC)
    decl = {
        "gpmp2mi_retime_path": [i, i, i, d, d, d, d, d, f, f, f, f, d, d, d, d, ip, d],
        "gpmp2mi_retime_path_dev": [i, i, i, vp, vp, vp, vp, d, f, f, f, f] + [vp] * 8,
        "gpmp2mi_retime_traj": [vp, lp, f, i, i, i, d, f, f, f, d, d, d, d, ip, d, d],
        "gpmp2mi_retime_traj_dev": [vp, lp, f, i, i, i, vp, f, f, f] + [vp] * 8,
        "gpmp2mi_plan_retime": [vp, lp, i, f, f, f, d, d, d, d, ip, d, d],
        "gpmp2mi_plan_retime_dev": [vp, lp, i, f, f, f] + [vp] * 8,
        "gpmp2mi_plan_select_retimed": [vp, i, f, i, vp, f, lp, f, f, f, f, f, ip, ip, d, d, d, d],
        "gpmp2mi_plan_select_retimed_dev": [vp, i, f, i, vp, f, lp, f, f, f, f, f] + [vp] * 7,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


class DynamicsDescC(C.Structure):
    """gpmp2mi_dynamics_desc (include/gpmp2mi.h "torque limits"): host arrays, gravity, and the limits or NULL."""
    _fields_ = [("mass", c_double_p), ("com", c_double_p), ("inertia", c_double_p), ("gravity", C.c_double * 3),
                ("torque", c_double_p)]


def declare_torque(lib):
    """argtypes of the torque-limit entry points (include/gpmp2mi.h "torque limits"); the description and `limits` are
    host structs in every form, the `_dev` forms take device addresses for everything else."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    lp, dp = C.POINTER(MotionLimitsC), C.POINTER(DynamicsDescC)
    decl = {
        "gpmp2mi_dynamics_create": [vp, dp, vp],
        "gpmp2mi_torque_score_traj": [vp, vp, f, i, i, i, d, d, d, d, ip, ip, d],
        "gpmp2mi_torque_score_traj_dev": [vp, vp, f, i, i, i] + [vp] * 8,
        "gpmp2mi_plan_torque_score": [vp, vp, i, d, d, d, ip, ip, d],
        "gpmp2mi_plan_torque_score_dev": [vp, vp, i] + [vp] * 7,
        "gpmp2mi_plan_select_dynamic": [vp, i, f, i, vp, f, lp, f, f, vp, ip, ip, d, d, d, d],
        "gpmp2mi_plan_select_dynamic_dev": [vp, i, f, i, vp, f, lp, f, f, vp] + [vp] * 7,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_dynamics_desc_default.argtypes = [dp]
    lib.gpmp2mi_dynamics_desc_default.restype = None
    lib.gpmp2mi_dynamics_destroy.argtypes = [vp]
    lib.gpmp2mi_dynamics_destroy.restype = None


def declare_retime_dynamic(lib):
    """argtypes of the entry points of include/gpmp2mi.h "re-timing under torque limits"; `limits`, `acc` and `bound` are
    host data in every form, the `_dev` forms take device addresses for everything else."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    lp = C.POINTER(MotionLimitsC)
    decl = {
        "gpmp2mi_retime_path_affine": [i, i, i, d, d, d, d, d, i, d, d, d, d, d, f, f, f, f, d, d, d, d, ip, d],
        "gpmp2mi_retime_path_affine_dev": [i, i, i, vp, vp, vp, vp, d, i, vp, vp, vp, vp, d, f, f, f, f] + [vp] * 8,
        "gpmp2mi_retime_dynamic_traj": [vp, vp, lp, f, i, i, i, d, f, f, f, d, d, d, d, ip, d, d, d, d],
        "gpmp2mi_retime_dynamic_traj_dev": [vp, vp, lp, f, i, i, i, vp, f, f, f] + [vp] * 10,
        "gpmp2mi_plan_retime_dynamic": [vp, vp, lp, i, f, f, f, d, d, d, d, ip, d, d, d, d],
        "gpmp2mi_plan_retime_dynamic_dev": [vp, vp, lp, i, f, f, f] + [vp] * 10,
        "gpmp2mi_plan_select_retimed_dynamic": [vp, i, f, i, vp, f, lp, f, f, f, f, f, vp, ip, ip, d, d, d, d, d],
        "gpmp2mi_plan_select_retimed_dynamic_dev": [vp, i, f, i, vp, f, lp, f, f, f, f, f, vp] + [vp] * 8,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_moving(lib):
    """argtypes of the moving-obstacle entry points (include/gpmp2mi.h "moving obstacles"); the `_dev` forms take device
    addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_plan_set_moving_spheres": [vp, i, d, d],
        "gpmp2mi_plan_set_moving_spheres_dev": [vp, i, vp, vp, vp],
        "gpmp2mi_moving_sphere_factor": [vp, i, d, f, i, d, d, d, d],
        "gpmp2mi_moving_score_traj": [vp, i, d, d, f, f, i, i, i, d, d, d, d, ip, ip],
        "gpmp2mi_moving_score_traj_dev": [vp, i, vp, vp, f, f, i, i, i] + [vp] * 7,
        "gpmp2mi_plan_moving_score": [vp, i, d, d, d, ip, ip],
        "gpmp2mi_plan_moving_score_dev": [vp, i] + [vp] * 6,
        "gpmp2mi_plan_select_moving": [vp, i, f, i, vp, f, f, ip, ip, d, d],
        "gpmp2mi_plan_select_moving_dev": [vp, i, f, i, vp, f, f] + [vp] * 5,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_carried(lib):
    """argtypes of the carried-object entry points (include/gpmp2mi.h "carried object"); the `_dev` forms take device
    addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_plan_set_carried": [vp, i, i, d, d],
        "gpmp2mi_plan_set_carried_dev": [vp, i, i, vp, vp, vp],
        "gpmp2mi_plan_carried_count": [vp],
        "gpmp2mi_carried_sphere_factor": [vp, vp, i, i, d, d, f, i, d, d, d],
        "gpmp2mi_carried_score_traj": [vp, vp, i, i, d, d, f, i, i, i, d, d, d, d, ip, ip],
        "gpmp2mi_carried_score_traj_dev": [vp, vp, i, i, vp, vp, f, i, i, i] + [vp] * 7,
        "gpmp2mi_plan_carried_score": [vp, i, d, d, d, ip, ip],
        "gpmp2mi_plan_carried_score_dev": [vp, i] + [vp] * 6,
        "gpmp2mi_plan_select_carried": [vp, i, f, i, vp, f, f, ip, ip, d, d],
        "gpmp2mi_plan_select_carried_dev": [vp, i, f, i, vp, f, f] + [vp] * 5,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_selfpair(lib):
    """argtypes of the plan's self-collision table (include/gpmp2mi.h "self-collision table in a plan")"""
    vp, i = C.c_void_p, C.c_int
    for name, args in {"gpmp2mi_plan_set_self_pairs": [vp, vp], "gpmp2mi_plan_self_pairs_count": [vp]}.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_map(lib):
    """argtypes of the live-map entry points (include/gpmp2mi.h "live map") and their stage timer; the `_dev` forms take
    device addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_sdf_reserve_update": [vp],
        "gpmp2mi_sdf_update": [vp, d, i],
        "gpmp2mi_sdf_update_dev": [vp, vp, vp],
        "gpmp2mi_sdf_update_from_occupancy": [vp, d, i],
        "gpmp2mi_sdf_update_from_occupancy_dev": [vp, vp, vp],
        "gpmp2mi_sdf_update_from_points": [vp, i, d, i, vp, d, f, ip],
        "gpmp2mi_sdf_update_from_points_dev": [vp, i, vp, i, vp, vp, f, vp, vp],
        "gpmp2mi_multi_plan_refresh_field": [vp],
        "gpmp2mi_debug_sdf_update_timing": [vp, i, d],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


class EvidenceOpts(C.Structure):
    """gpmp2mi_evidence_opts (include/gpmp2mi.h "sensor map")"""
    _fields_ = [(n, C.c_int) for n in ("hit", "miss", "lo", "hi", "occupied_at", "use_base", "refresh")]


class DepthCamera(C.Structure):
    """gpmp2mi_depth_camera (include/gpmp2mi.h "sensor map")"""
    _fields_ = ([("width", C.c_int), ("height", C.c_int)] +
                [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "depth_min", "depth_max")] +
                [("pose", C.c_double * 12)])


def declare_sensor(lib):
    """argtypes of the sensor-map entry points (include/gpmp2mi.h "sensor map") and their stage timer; the `_dev` forms
    take device addresses; sensor_origin, the camera and the opts are host data in every form."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    op, cam = C.POINTER(EvidenceOpts), C.POINTER(DepthCamera)
    decl = {
        "gpmp2mi_sdf_reserve_evidence": [vp],
        "gpmp2mi_sdf_integrate_points": [vp, i, d, d, vp, d, f, op, ip],
        "gpmp2mi_sdf_integrate_points_dev": [vp, i, vp, d, vp, vp, f, op, vp, vp],
        "gpmp2mi_sdf_integrate_depth": [vp, cam, C.POINTER(C.c_float), vp, d, f, op, ip],
        "gpmp2mi_sdf_integrate_depth_dev": [vp, cam, vp, vp, vp, f, op, vp, vp],
        "gpmp2mi_sdf_refresh_from_evidence": [vp, i, i],
        "gpmp2mi_sdf_refresh_from_evidence_dev": [vp, i, i, vp],
        "gpmp2mi_sdf_evidence_reset": [vp],
        "gpmp2mi_sdf_evidence_reset_dev": [vp, vp],
        "gpmp2mi_sdf_get_evidence": [vp, C.POINTER(C.c_int16)],
        "gpmp2mi_debug_sdf_integrate_timing": [vp, i, d],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_evidence_opts_default.argtypes = [op]
    lib.gpmp2mi_evidence_opts_default.restype = None


SCENE_BOX, SCENE_SPHERE, SCENE_CYLINDER, SCENE_MESH = 0, 1, 2, 3
MAX_SCENE_OBJECTS = 256
MAX_SCENE_TRIANGLES = 1 << 20


class SceneObject(C.Structure):
    """gpmp2mi_scene_object (include/gpmp2mi.h "scene")"""
    _fields_ = [("kind", C.c_int), ("size", C.c_double * 3), ("inflate", C.c_double),
                ("n_vertices", C.c_int), ("vertices", c_double_p), ("n_triangles", C.c_int), ("triangles", c_int_p),
                ("pose", C.c_double * 12), ("enabled", C.c_int)]


def declare_scene(lib):
    """argtypes of the scene entry points (include/gpmp2mi.h "scene") and their stage timer; the `_dev` forms take device
    addresses; objects, poses, enabled flags and the grid origin are host data in every form."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    ob, bp = C.POINTER(SceneObject), C.POINTER(C.c_ubyte)
    decl = {
        "gpmp2mi_scene_create": [i, ob, C.POINTER(vp)],
        "gpmp2mi_scene_count": [vp],
        "gpmp2mi_scene_set_poses": [vp, i, i, d],
        "gpmp2mi_scene_set_enabled": [vp, i, i, ip],
        "gpmp2mi_scene_reserve": [vp, i, i, i],
        "gpmp2mi_scene_rasterize": [vp, i, d, f, i, i, i, bp, ip],
        "gpmp2mi_scene_rasterize_dev": [vp, i, d, f, i, i, i, vp, vp, vp],
        "gpmp2mi_sdf_update_from_scene": [vp, vp, i, i, i, ip],
        "gpmp2mi_sdf_update_from_scene_dev": [vp, vp, i, i, i, vp, vp],
        "gpmp2mi_debug_scene_timing": [vp, i, d],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_scene_destroy.argtypes = [vp]
    lib.gpmp2mi_scene_destroy.restype = None


def declare_path(lib):
    """argtypes of the workspace-path entry points (include/gpmp2mi.h "workspace path"); the `_dev` forms take device
    addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_plan_set_workspace_path": [vp, d, d],
        "gpmp2mi_plan_set_workspace_path_dev": [vp, vp, vp, vp],
        "gpmp2mi_workspace_path_factor": [vp, i, i, i, d, d, d, d],
        "gpmp2mi_path_score_traj": [vp, i, i, d, d, f, i, i, i, d, d, d, ip, d, d, ip],
        "gpmp2mi_path_score_traj_dev": [vp, i, i, vp, vp, f, i, i, i] + [vp] * 8,
        "gpmp2mi_plan_path_score": [vp, i, d, d, ip, d, d, ip],
        "gpmp2mi_plan_path_score_dev": [vp, i] + [vp] * 7,
        "gpmp2mi_plan_select_path": [vp, i, f, i, f, f, ip, ip, d, d],
        "gpmp2mi_plan_select_path_dev": [vp, i, f, i, f, f] + [vp] * 5,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_group(lib):
    """include/gpmp2mi.h "distinct alternatives"; `weights` is a host array in every form"""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_traj_distances": [i, i, i, d, d, i, d],
        "gpmp2mi_traj_distances_dev": [i, i, i, vp, d, i, vp, vp],
        "gpmp2mi_group_rows": [i, d, d, ip, f, ip, ip, ip, ip],
        "gpmp2mi_group_rows_dev": [i, vp, vp, vp, f] + [vp] * 5,
        "gpmp2mi_group_traj": [i, i, i, d, d, i, f, d, ip, ip, ip, ip, ip],
        "gpmp2mi_group_traj_dev": [i, i, i, vp, d, i, f] + [vp] * 7,
        "gpmp2mi_plan_select_distinct": [vp, i, f, i, vp, f, i, d, f, i, ip, ip, ip, ip, d, ip, d, d],
        "gpmp2mi_plan_select_distinct_dev": [vp, i, f, i, vp, f, i, d, f, i] + [vp] * 9,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_posterior(lib):
    """argtypes of the posterior entry points (include/gpmp2mi.h "posterior"); the `_dev` forms take device addresses."""
    vp, i, d, ip = C.c_void_p, C.c_int, c_double_p, c_int_p
    decl = {
        "gpmp2mi_block_tridiag_marginals": [i, i, i, d, d, d, d, ip],
        "gpmp2mi_block_tridiag_sample": [i, i, i, i, d, d, d, d, ip],
        "gpmp2mi_plan_marginals": [vp, d, d, d, ip],
        "gpmp2mi_plan_marginals_dev": [vp, vp, vp, vp, vp],
        "gpmp2mi_plan_sample_posterior": [vp, i, d, d, ip],
        "gpmp2mi_plan_sample_posterior_dev": [vp, i, vp, vp, vp, vp],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


def declare_risk(lib):
    """argtypes of the entry points of the posterior on the executed timeline (include/gpmp2mi.h); the `_dev` forms take
    device addresses."""
    vp, i, d, ip, f = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double
    decl = {
        "gpmp2mi_gp_interpolate_cov": [i, d, f, i, i, i, d, d, d],
        "gpmp2mi_gp_interpolate_cov_dev": [i, vp, f, i, i, i, vp, vp, vp, vp],
        "gpmp2mi_risk_traj": [vp, vp, d, f, i, i, i, d, d, d, ip, f, d, ip, d, ip, d],
        "gpmp2mi_risk_traj_dev": [vp, vp, vp, f, i, i, i, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, vp],
        "gpmp2mi_plan_marginals_dense": [vp, i, d, ip],
        "gpmp2mi_plan_marginals_dense_dev": [vp, i, vp, vp, vp],
        "gpmp2mi_plan_risk": [vp, i, f, d, ip, d, ip, d, ip],
        "gpmp2mi_plan_risk_dev": [vp, i, f, vp, vp, vp, vp, vp, vp, vp],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


RNG_RESTARTS, RNG_POSTERIOR = 1, 2


def declare_seed(lib):
    """argtypes of the seeding entry points (include/gpmp2mi.h "seeding") and their debug read-out; the `_dev` forms take
    device addresses."""
    vp, i, d, ip, f, u64 = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double, C.c_uint64
    decl = {
        "gpmp2mi_normal_fill": [u64, i, i, i, i, i, i, i, d],
        "gpmp2mi_normal_fill_dev": [u64, i, i, i, i, i, i, i, vp, vp],
        "gpmp2mi_plan_seed_restarts": [vp, i, u64, i, f, i, d, d, d, d],
        "gpmp2mi_plan_seed_restarts_dev": [vp, i, u64, i, f, i, vp, vp, vp, vp, vp],
        "gpmp2mi_plan_optimize_queue_seeded": [vp, i, u64, i, f, i, d, d, d, d, d, d, ip, d, ip, d, d],
        "gpmp2mi_plan_optimize_queue_seeded_dev": [vp, i, u64, i, f, i] + [vp] * 12,
        "gpmp2mi_multi_plan_optimize_queue_seeded": [vp, i, u64, i, f, i, d, d, d, d, d, d, ip, d, ip, d, d],
        "gpmp2mi_plan_sample_posterior_seeded": [vp, i, u64, i, i, d, ip],
        "gpmp2mi_plan_sample_posterior_seeded_dev": [vp, i, u64, i, i, vp, vp, vp],
        "gpmp2mi_debug_plan_seed_prior": [vp, d, d],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


RNG_BRIDGE = 3


def declare_sampled(lib):
    """argtypes of the sampled-clearance entry points (include/gpmp2mi.h "sampled clearance") and their debug hook; the
    `_dev` forms take device addresses, except Qc, which stays a host array."""
    vp, i, d, ip, f, u64 = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double, C.c_uint64
    head = [vp, vp, d, f, i, i, i, i]
    decl = {
        "gpmp2mi_sampled_clearance_traj": head + [d, d, ip, u64, i, i, i, f, ip, d, d, ip, d, ip, ip, d],
        "gpmp2mi_sampled_clearance_traj_dev": head + [vp, vp, vp, u64, i, i, i, f] + [vp] * 9,
        "gpmp2mi_plan_collision_probability": [vp, i, i, u64, i, i, i, f, ip, d, d, ip, d, ip, ip, ip],
        "gpmp2mi_plan_collision_probability_dev": [vp, i, i, u64, i, i, i, f] + [vp] * 9,
        "gpmp2mi_plan_sample_dense_seeded": [vp, i, i, u64, i, i, i, d, ip],
        "gpmp2mi_plan_sample_dense_seeded_dev": [vp, i, i, u64, i, i, i, vp, vp, vp],
        "gpmp2mi_debug_sampled_chunk_bytes": [C.c_size_t],
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i


RNG_IK = 4
IK_MAX_ITER = 1000
IK_CONVERGED, IK_MAX_ITER_REACHED, IK_INVALID = 0, 1, 2
WORKSPACE_POSITION, WORKSPACE_ORIENTATION, WORKSPACE_POSE = 0, 1, 2


class IkOptsC(C.Structure):
    """gpmp2mi_ik_opts (include/gpmp2mi.h "goal configurations"); pos_down / pos_up: host arrays [dof] or NULL"""
    _fields_ = [("mode", C.c_int), ("link", C.c_int), ("pos_tol", C.c_double), ("rot_tol", C.c_double),
                ("rot_weight", C.c_double), ("max_iter", C.c_int), ("lambda_initial", C.c_double),
                ("lambda_factor", C.c_double), ("lambda_lower", C.c_double), ("lambda_upper", C.c_double),
                ("pos_down", c_double_p), ("pos_up", c_double_p)]


def declare_ik(lib):
    """argtypes of the inverse-kinematics entry points (include/gpmp2mi.h "goal configurations"); the options, near and
    weights are host data in every form, the `_dev` forms take device addresses for everything else."""
    vp, i, d, ip, f, u64 = C.c_void_p, C.c_int, c_double_p, c_int_p, C.c_double, C.c_uint64
    op = C.POINTER(IkOptsC)
    decl = {
        "gpmp2mi_ik_solve": [vp, op, i, d, i, d, d, d, ip, ip],
        "gpmp2mi_ik_solve_dev": [vp, op, i, vp, i, vp, vp, vp, vp, vp, vp],
        "gpmp2mi_ik_solve_seeded": [vp, op, i, d, i, u64, i, d, d, ip, ip],
        "gpmp2mi_ik_solve_seeded_dev": [vp, op, i, vp, i, u64, i, vp, vp, vp, vp, vp],
        "gpmp2mi_ik_goals": [vp, op, vp, i, d, i, d, u64, i, f, i, d, d, f, i, d, ip, d, ip, ip, ip, ip, ip, d, ip, d, d],
        "gpmp2mi_ik_goals_dev": [vp, op, vp, i, vp, i, vp, u64, i, f, i, d, d, f, i] + [vp] * 13,
    }
    for name, args in decl.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = i
    lib.gpmp2mi_ik_opts_default.argtypes = [op]
    lib.gpmp2mi_ik_opts_default.restype = None


def dptr(a):
    """pointer to a C-contiguous float64 array (None -> NULL)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "need contiguous float64"
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"], "need contiguous int32"
    return a.ctypes.data_as(c_int_p)


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def make_robot_desc(model):
    """(RobotDesc, keepalive) from a gpmp2_amd.robots.RobotModel."""
    fl = model.flat()
    d = RobotDesc()
    d.kind, d.dof, d.arm_dof = fl["kind"], fl["dof"], fl["arm_dof"]
    d.a, d.alpha, d.d, d.theta_bias = dptr(fl["a"]), dptr(fl["alpha"]), dptr(fl["d"]), dptr(fl["theta_bias"])
    for i in range(16):
        d.base_pose[i] = float(fl["base_pose"][i])
    d.nr_spheres = len(fl["sphere_radius"])
    d.sphere_link = iptr(fl["sphere_link"])
    d.sphere_radius = dptr(fl["sphere_radius"])
    d.sphere_center = dptr(fl["sphere_center"])
    d.arm2_dof = int(fl.get("arm2_dof", 0))
    eye = np.eye(4).reshape(16)
    for i in range(16):
        d.base_pose2[i] = float(fl.get("base_pose2", eye)[i])
        d.base_pose3[i] = float(fl.get("base_pose3", eye)[i])
    d.reverse_linact = int(fl.get("reverse_linact", 0))
    return d, fl


def make_settings(setting):
    """(Settings, GraphOpts, keepalive) from a gpmp2_amd.planner.TrajOptimizerSetting."""
    s = Settings()
    keep = {}

    def vec(name, value):
        if value is None:
            return None
        arr = f64(value).reshape(-1)
        if arr.size != setting.dof:
            raise ValueError(f"[TrajOptimizerSetting] {name} dim does not fit dof")
        keep[name] = arr
        return dptr(arr)

    s.dof, s.total_step, s.total_time = setting.dof, setting.total_step, setting.total_time
    s.conf_prior_sigma, s.vel_prior_sigma = setting.conf_prior_sigma, setting.vel_prior_sigma
    s.flag_pos_limit, s.flag_vel_limit = int(setting.flag_pos_limit), int(setting.flag_vel_limit)
    s.joint_pos_limits_up = vec("joint_pos_limits_up", setting.joint_pos_limits_up)
    s.joint_pos_limits_down = vec("joint_pos_limits_down", setting.joint_pos_limits_down)
    s.vel_limits = vec("vel_limits", setting.vel_limits)
    s.pos_limit_thresh = vec("pos_limit_thresh", setting.pos_limit_thresh)
    s.vel_limit_thresh = vec("vel_limit_thresh", setting.vel_limit_thresh)
    s.pos_limit_sigmas = vec("pos_limit_sigmas", setting.pos_limit_sigmas)
    s.vel_limit_sigmas = vec("vel_limit_sigmas", setting.vel_limit_sigmas)
    s.epsilon, s.cost_sigma, s.obs_check_inter = setting.epsilon, setting.cost_sigma, setting.obs_check_inter
    if setting.Qc is not None:
        q = f64(setting.Qc)
        if q.shape != (setting.dof, setting.dof):
            raise ValueError("[TrajOptimizerSetting] Qc dim does not fit dof")
        keep["Qc"] = q
        s.Qc = dptr(q)
    s.opt_type, s.verbosity = setting.opt_type, setting.opt_verbosity
    s.final_iter_no_increase = int(setting.final_iter_no_increase)
    s.rel_thresh, s.max_iter = setting.rel_thresh, setting.max_iter
    o = GraphOpts()
    o.obs_skip_first_state = int(setting.obs_skip_first_state)
    o.vehicle_dynamics_sigma = setting.vehicle_dynamics_sigma
    o.lm_lambda_initial, o.lm_lambda_factor = setting.lm_lambda_initial, setting.lm_lambda_factor
    o.lm_lambda_upper, o.lm_lambda_lower = setting.lm_lambda_upper, setting.lm_lambda_lower
    o.lm_min_model_fidelity = setting.lm_min_model_fidelity
    o.dogleg_delta_initial = setting.dogleg_delta_initial
    o.abs_error_tol, o.error_tol = setting.abs_error_tol, setting.error_tol
    o.fixed_iterations = setting.fixed_iterations
    o.end_conf_prior_off = int(getattr(setting, "end_conf_prior_off", False))
    ws = list(getattr(setting, "workspace_factors", []) or [])
    if len(ws) > MAX_WORKSPACE_FACTORS:
        raise ValueError("too many workspace factors for one plan")
    o.n_workspace = len(ws)
    for k, w in enumerate(ws):
        o.workspace[k].mode, o.workspace[k].link = int(w["mode"]), int(w["link"])
        o.workspace[k].first_state, o.workspace[k].last_state = int(w["first_state"]), int(w["last_state"])
        o.workspace[k].sigma = float(w["sigma"])
        des = f64(w["des_pose"]).reshape(16)
        for t in range(16):
            o.workspace[k].des_pose[t] = des[t]
    sc = getattr(setting, "self_collision", None)
    if sc is not None:
        sc = f64(sc).reshape(-1, 4)
        if sc.shape[0] > MAX_SELF_COLLISION_PAIRS:
            raise ValueError("too many self-collision pairs for one plan")
        o.n_self_collision = sc.shape[0]
        rng_ = getattr(setting, "self_collision_states", None) or (0, setting.total_step)
        o.self_collision_first, o.self_collision_last = int(rng_[0]), int(rng_[1])
        for k in range(sc.shape[0]):
            for t in range(4):
                o.self_collision[k][t] = sc[k, t]
    mv = getattr(setting, "moving_spheres", None)
    if mv is not None:
        if not 0 <= int(mv["capacity"]) <= MAX_MOVING_SPHERES:
            raise ValueError("moving-sphere capacity outside 0..MAX_MOVING_SPHERES")
        o.max_moving_spheres = int(mv["capacity"])
        rng_ = mv.get("states") or (0, setting.total_step)
        o.moving_first, o.moving_last = int(rng_[0]), int(rng_[1])
        o.moving_epsilon, o.moving_sigma = float(mv["epsilon"]), float(mv["sigma"])
    cr = getattr(setting, "carried_spheres", None)
    if cr is not None:
        if not 0 <= int(cr["capacity"]) <= MAX_CARRIED_SPHERES:
            raise ValueError("carried-sphere capacity outside 0..MAX_CARRIED_SPHERES")
        o.max_carried_spheres = int(cr["capacity"])
        rng_ = cr.get("states") or (0, setting.total_step)
        o.carried_first, o.carried_last = int(rng_[0]), int(rng_[1])
        o.carried_epsilon, o.carried_sigma = float(cr["epsilon"]), float(cr["sigma"])
    sp = getattr(setting, "self_pairs", None)
    if sp is not None:
        if not 0 <= int(sp["capacity"]) <= MAX_PLAN_SELF_PAIRS:
            raise ValueError("self-collision table capacity outside 0..MAX_PLAN_SELF_PAIRS")
        o.max_self_pairs = int(sp["capacity"])
        rng_ = sp.get("states") or (0, setting.total_step)
        o.self_pairs_first, o.self_pairs_last = int(rng_[0]), int(rng_[1])
    wp = getattr(setting, "workspace_path", None)
    if wp is not None:
        if int(wp["mode"]) not in (WORKSPACE_POSITION, WORKSPACE_ORIENTATION, WORKSPACE_POSE):
            raise ValueError("workspace path: unknown mode")
        o.workspace_path, o.workspace_path_mode, o.workspace_path_link = 1, int(wp["mode"]), int(wp["link"])
    return s, o, keep
