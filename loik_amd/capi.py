"""ctypes binding of include/loik_amd.h (the drop-in C-ABI) + a host-side mirror of the reference's solver API.

`BatchedLoik` keeps the reference's method names and argument meaning
(`SolveInit`, `Solve`, getters: /root/reference/include/loik/loik-loid-optimized.hpp:335-361, :368-455, :475-580,
:596-695; /root/reference/include/loik/task-solver-base.hpp:87-141) so the parity tests read like the
reference's own tests.  All compute happens in libloik_amd.so on the GPU; nothing here falls back to a CPU path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libloik_amd.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class LoikError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("loik_amd error %d: %s" % (code, msg))
        self.code = code


class ModelDesc(C.Structure):
    _fields_ = [("njoints", C.c_int), ("nq", C.c_int), ("nv", C.c_int), ("parents", _ip), ("jtype", _ip),
                ("axis", _dp), ("idx_q", _ip), ("idx_v", _ip), ("placement", _dp),
                ("comp_first", _ip), ("comp_count", _ip), ("comp_jtype", _ip), ("comp_axis", _dp), ("comp_placement", _dp),
                ("pitch", _dp), ("comp_pitch", _dp)]


class Options(C.Structure):
    _fields_ = [("max_iter", C.c_int),
                ("tol_abs", C.c_double), ("tol_rel", C.c_double), ("tol_primal_inf", C.c_double),
                ("tol_dual_inf", C.c_double), ("rho", C.c_double), ("mu", C.c_double),
                ("mu_equality_scale_factor", C.c_double), ("mu_update_strat", C.c_int),
                ("num_eq_c", C.c_int), ("eq_c_dim", C.c_int), ("warm_start", C.c_int),
                ("tol_tail_solve", C.c_double), ("verbose", C.c_int), ("logging", C.c_int),
                ("batch", C.c_int), ("device", C.c_int), ("precision", C.c_int), ("flags", C.c_int),
                ("max_launch_iters", C.c_int), ("compact_min_instances", C.c_int),
                ("tail_max_instances", C.c_int), ("eq_c_capacity", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("instance_iterations", C.c_ulonglong), ("launches", C.c_int), ("n_unfinished", C.c_int),
                ("compactions", C.c_int), ("tail_instances", C.c_int), ("tail_ms", C.c_double),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("bytes_per_instance_iteration", C.c_double),
                ("tail_instance_iterations", C.c_ulonglong), ("tail_launches", C.c_int), ("team", C.c_int), ("chunks", C.c_int),
                ("solve_busy_ms", C.c_double), ("tail_busy_ms", C.c_double), ("lean_launches", C.c_int),
                ("lean_escaped", C.c_int), ("hslots_ms", C.c_double), ("lean_requeues", C.c_int), ("flat_launches", C.c_int), ("queue_dry_ms", C.c_double),
                ("flat_split_launches", C.c_int), ("flat_ordered", C.c_int), ("flat_built", C.c_int),
                ("flat_probe_launches", C.c_int), ("probe_ms", C.c_double)]


ABI_VERSION = 602   # LOIKB_VERSION of include/loik_amd.h this binding matches (struct layouts, entry points)

# enums of loik_amd.h
F64, F32 = 0, 1
OPT_FIXED_ITERS, OPT_NO_H_CACHE, OPT_NO_COMPACTION, OPT_OWN_STREAM, OPT_F32_ACCURATE, OPT_ORDER_FROM_PREVIOUS = 1, 2, 4, 8, 16, 32
IN_DEVICE, A_SHARED, BOUNDS_SHARED, B_SHARED, Q_SHARED = 1, 2, 4, 8, 16
OUT_DEVICE = 1

_VEC_FIELDS = ["z", "nu", "w", "Stf_plus_w", "r", "Dinv", "vis", "fis", "g", "pis", "UDinv", "His", "liMi", "yis",
               "Aty", "iter", "converged", "primal_infeasible", "status"]
_SCALAR_FIELDS = ["primal_residual", "dual_residual", "primal_residual_task", "primal_residual_slack",
                  "dual_residual_v", "dual_residual_nu", "tol_primal", "tol_dual", "mu", "mu_eq", "mu_ineq",
                  "delta_x_qp_inf_norm", "delta_z_qp_inf_norm", "delta_y_qp_inf_norm", "A_qp_T_delta_y_qp_inf_norm",
                  "ub_qp_T_delta_y_qp_plus", "lb_qp_T_delta_y_qp_minus", "delta_fis_inf_norm", "delta_yis_inf_norm",
                  "delta_w_inf_norm", "delta_vis_inf_norm", "delta_nu_inf_norm", "Av_inf_norm", "nu_inf_norm",
                  "Href_v_inf_norm", "g_inf_norm", "Stf_plus_w_inf_norm", "primal_infeasibility_cond_1",
                  "primal_infeasibility_cond_2", "tail_solve_iter"]
FIELD_ID = {n: i for i, n in enumerate(_VEC_FIELDS)}
FIELD_ID["q"] = 96
FIELD_ID["mu_updates"] = 97
FIELD_ID["primal_residual_vec"] = 98
FIELD_ID["dual_residual_vec"] = 99
FIELD_ID.update({n: 32 + i for i, n in enumerate(_SCALAR_FIELDS)})
INT_FIELDS = ("iter", "converged", "primal_infeasible", "status", "mu_updates")   # int32, the others float64
# what loikb_get writes per instance, after [B]: "nb" bodies (njoints - 1), "nc" constraints in force; "scalars" is loikb_get_results' block.
# r / Dinv / UDinv are inter-sweep temporaries of the device's elimination: per DoF, equal to upstream's per-joint values for 1-DoF joints only
FIELD_DIMS = dict({n: ("nv",) for n in ("z", "nu", "w", "Stf_plus_w", "r", "Dinv")}, **{n: ("nb", 6) for n in ("vis", "fis", "g", "pis")},
                  **{n: ("nc", 6) for n in ("yis", "Aty")}, **{n: ("6nb+nv",) for n in ("primal_residual_vec", "dual_residual_vec")},
                  **{n: () for n in _SCALAR_FIELDS + list(INT_FIELDS)}, UDinv=("nv", 6), His=("nb", 21), liMi=("nb", 12), q=("nq",), scalars=(33,))

# every symbol include/loik_amd.h and include/loik_amd_models.h declare
EXPORTED_SYMBOLS = [
    "loikb_create", "loikb_destroy", "loikb_set_stream", "loikb_solve_init", "loikb_solve", "loikb_solve_full",
    "loikb_solve_tailored", "loikb_set_max_iter", "loikb_set_rho", "loikb_set_mu", "loikb_set_tol",
    "loikb_set_tol_primal_inf", "loikb_set_tol_tail_solve", "loikb_set_warm_start", "loikb_get", "loikb_get_results", "loikb_get_stats",
    "loikb_batch", "loikb_nv", "loikb_njoints", "loikb_last_error", "loikb_status_string", "loikb_version",
    "loikb_device_count", "loikb_sweep_schedule", "loikb_integrate", "loikb_synchronize", "loikb_plan_string", "loikb_pass",
    "loikb_update_references", "loikb_update_eq_constraint", "loikb_add_eq_constraint", "loikb_remove_eq_constraint",
    "loikb_num_eq_c", "loikb_eq_c_capacity", "loikb_active_constraint_ids", "loikb_get_solver_info", "loikb_solver_info_rows_cap", "loikb_solver_info_truncated", "loikb_builtin_model", "loikb_builtin_joint_name",
    "loikb_builtin_joint_id", "loikb_flat_schedule", "loikb_flat_variant"]

# include/loik_amd_pose.h: batched pose IK, its own header and version (EXPORTED_SYMBOLS stays the two headers above)
POSE_ABI_VERSION = 1
POSE_SYMBOLS = ["loikb_pose_version", "loikb_solve_pose", "loikb_forward_kinematics", "loikb_pose_get"]
POSE_TARGET_SHARED = 32
POSE_F_STEPS, POSE_F_STATUS, POSE_F_ERR, POSE_F_TIMING = 0, 1, 2, 3
POSE_ST_REACHED, POSE_ST_NOT_CONVERGED, POSE_ST_INFEASIBLE, POSE_ST_STOPPED = 1, 2, 4, 8


# include/loik_amd_limits.h: joint position limits for the pose loop, the velocity-box update; its own header and version again
LIMITS_ABI_VERSION = 1
LIMITS_SYMBOLS = ["loikb_limits_version", "loikb_set_joint_limits", "loikb_update_ineq_constraints", "loikb_pose_get_limit_flags"]
LIMIT_LOWER, LIMIT_UPPER = 1, 2


# include/loik_amd_tasks.h: tool frames and position-only / orientation-only tasks of the pose loop; its own header and version again
TASKS_ABI_VERSION = 1
TASKS_SYMBOLS = ["loikb_tasks_version", "loikb_pose_set_tasks", "loikb_pose_clear_tasks", "loikb_pose_get_tasks", "loikb_frame_placements"]
TASK_POSE, TASK_POSITION, TASK_ORIENTATION = 0, 1, 2
TASK_KINDS = {"pose": TASK_POSE, "position": TASK_POSITION, "orientation": TASK_ORIENTATION}


# include/loik_amd_multistart.h: device-sampled seeds, restarts and the best seed per goal around the pose loop; its own header and version again
MULTISTART_ABI_VERSION = 1
MULTISTART_SYMBOLS = ["loikb_multistart_version", "loikb_multistart_set_ranges", "loikb_multistart_sample", "loikb_solve_pose_multistart",
                      "loikb_multistart_get"]
MS_PICK_NEAREST, MS_PICK_FIRST = 0, 1
MS_PICKS = {"nearest": MS_PICK_NEAREST, "first": MS_PICK_FIRST}
MS_F_WINNER, MS_F_GOAL_STATUS, MS_F_Q, MS_F_ERR, MS_F_COST, MS_F_NREACHED, MS_F_ROUND, MS_F_TIMING = range(8)
MS_GOAL_REACHED, MS_GOAL_BEST_EFFORT, MS_GOAL_FAILED = 1, 2, 4


# include/loik_amd_path.h: per-instance waypoint paths in the pose loop; its own header and version again
PATH_ABI_VERSION = 1
PATH_SYMBOLS = ["loikb_path_version", "loikb_solve_pose_path", "loikb_path_get"]
PATH_F_CURSOR, PATH_F_STATUS, PATH_F_WSTEPS, PATH_F_Q, PATH_F_TIMING = range(5)
PATH_ST_COMPLETE, PATH_ST_STALLED = 1, 2


# include/loik_amd_track.h: timed pose trajectories with feed-forward in the pose loop; its own header and version again
TRACK_ABI_VERSION = 1
TRACK_SYMBOLS = ["loikb_track_version", "loikb_track_pose", "loikb_track_get"]
TRACK_FF_NONE, TRACK_FF_DIFFERENCE = 0, 1
TRACK_FFS = {"none": TRACK_FF_NONE, "difference": TRACK_FF_DIFFERENCE}
TRACK_REC_Q, TRACK_REC_Z = 1, 2
TRACK_RECS = {"q": TRACK_REC_Q, "z": TRACK_REC_Z}
TRACK_F_Q, TRACK_F_Z, TRACK_F_ERRMAX, TRACK_F_INNER, TRACK_F_ONTRACK, TRACK_F_WORST, TRACK_F_WORST_AT, TRACK_F_TIMING = range(8)
TRACK_IN_NOT_CONVERGED, TRACK_IN_INFEASIBLE, TRACK_IN_LIMIT = 1, 2, 4
TRACK_IN_ACCEL = 8   # (include/loik_amd_accel.h: an acceleration flag of the step is non-zero)
# what loikb_track_get writes per instance, after [B], in the manner of FIELD_DIMS / INT_FIELDS (which describe loikb_get's fields and
# those alone): "T" steps, "T+1" samples
TRACK_FIELD_ID = {"q_traj": TRACK_F_Q, "z_traj": TRACK_F_Z, "errmax": TRACK_F_ERRMAX, "inner": TRACK_F_INNER, "ontrack": TRACK_F_ONTRACK,
                  "worst": TRACK_F_WORST, "worst_at": TRACK_F_WORST_AT}
TRACK_FIELD_DIMS = {"q_traj": ("T+1", "nq"), "z_traj": ("T", "nv"), "errmax": ("T+1",), "inner": ("T",), "ontrack": (), "worst": (), "worst_at": ()}
TRACK_INT_FIELDS = ("inner", "ontrack", "worst_at")   # int32, the others float64


# include/loik_amd_accel.h: joint acceleration limits and braking-aware position limits in the pose loops; its own header and version again
ACCEL_ABI_VERSION = 1
ACCEL_SYMBOLS = ["loikb_accel_version", "loikb_set_joint_accel_limits", "loikb_accel_set_start_velocity", "loikb_accel_get_velocity"]
LIMIT_ACCEL_LOWER, LIMIT_ACCEL_UPPER = 4, 8
# what loikb_accel_get_velocity writes per instance, after [B], in the manner of TRACK_FIELD_DIMS / TRACK_INT_FIELDS
ACCEL_FIELD_DIMS = {"applied_velocity": ("nv",)}
ACCEL_INT_FIELDS = ()   # float64
# include/loik_amd_axis.h: axis-symmetric tool tasks (the rotation about the task frame's z axis is free): a modifier bit on the kinds of
# loik_amd_tasks.h, in a header and version of its own.  TASK_KINDS above stays the tasks header's three; these are the two it adds
AXIS_ABI_VERSION = 1
AXIS_SYMBOLS = ["loikb_axis_version"]
TASK_FREE_Z = 4
TASK_POSE_AXIS, TASK_AXIS = TASK_POSE | TASK_FREE_Z, TASK_ORIENTATION | TASK_FREE_Z
AXIS_TASK_KINDS = {"pose_axis": TASK_POSE_AXIS, "axis": TASK_AXIS}
# include/loik_amd_step.h: backtracking step control and stall detection in SolvePose; its own header and version again
STEP_ABI_VERSION = 1
STEP_SYMBOLS = ["loikb_step_version", "loikb_pose_set_step_control", "loikb_pose_get_step_control", "loikb_step_get"]
POSE_ST_STALLED = 16
STEP_F_ALPHA, STEP_F_BACKTRACKS, STEP_F_FAILED = range(3)
# include/loik_amd_jacobian.h: frame Jacobians and dexterity measures of the resident q, the dexterous multi-start pick; its own header and
# version again (MS_PICKS stays the multi-start header's two)
JACOBIAN_ABI_VERSION = 1
JACOBIAN_SYMBOLS = ["loikb_jacobian_version", "loikb_frame_jacobians", "loikb_frame_dexterity", "loikb_dexterity_set_multistart_pick",
                    "loikb_dexterity_get_multistart_pick"]
JAC_LOCAL, JAC_LOCAL_WORLD_ALIGNED, JAC_WORLD = 0, 1, 2
JAC_REFERENCES = {"local": JAC_LOCAL, "local_world_aligned": JAC_LOCAL_WORLD_ALIGNED, "world": JAC_WORLD}
DEX_SIGMA0, DEX_MANIPULABILITY, DEX_INV_CONDITION, DEX_N = 0, 6, 7, 8
# include/loik_amd_collision.h: clearance of a sphere model against a world of spheres and boxes and against itself, and the
# collision-aware multi-start; its own header and version again (the MS_GOAL_* of the multi-start header stay its three)
COLLISION_ABI_VERSION = 1
COLLISION_SYMBOLS = ["loikb_collision_version", "loikb_collision_set_spheres", "loikb_collision_set_world", "loikb_collision_set_self_pairs",
                     "loikb_collision_num_self_pairs", "loikb_clearance", "loikb_clearance_set_multistart", "loikb_clearance_get_multistart",
                     "loikb_clearance_get_multistart_result"]
CLR_NONE, CLR_WORLD_SPHERE, CLR_WORLD_BOX, CLR_SELF = 0, 1, 2, 3
CLR_MAX_SPHERES = 2048
MS_GOAL_IN_COLLISION = 8
CLR_MS_F_CLEARANCE, CLR_MS_F_WITNESS, CLR_MS_F_NCLEAR, CLR_MS_F_INSTANCE = range(4)
# include/loik_amd_motion.h: certified collision checks of joint-space motions and the inverse of integrate; its own header and version
MOTION_ABI_VERSION = 1
MOTION_SYMBOLS = ["loikb_motion_version", "loikb_difference", "loikb_motion_clearance", "loikb_motion_clearance_path"]
MOTION_FREE, MOTION_BLOCKED, MOTION_UNDECIDED, MOTION_INVALID = 0, 1, 2, 3
# include/loik_amd_avoid.h: collision avoidance in the pose loops and clearance gradients; its own header and version
AVOID_ABI_VERSION = 1
AVOID_SYMBOLS = ["loikb_avoid_version", "loikb_clearance_gradient", "loikb_avoid_set", "loikb_avoid_get", "loikb_avoid_box",
                 "loikb_avoid_get_result"]
AVOID_MAX_SPHERES = 256
AVOID_F_MIN_SEEN, AVOID_F_ACTIVE_STEPS, AVOID_F_FLAGS = range(3)
# include/loik_amd_shortcut.h: certified shortcutting of joint-space paths and their lengths; its own header and version
SHORTCUT_ABI_VERSION = 1
SHORTCUT_SYMBOLS = ["loikb_shortcut_version", "loikb_shortcut_paths", "loikb_path_length"]
# include/loik_amd_retime.h: time-optimal retiming of joint-space paths; its own header and version
RETIME_ABI_VERSION = 1
RETIME_SYMBOLS = ["loikb_retime_version", "loikb_retime_paths"]
RETIME_SNAP = 1
RETIME_TRUNCATED, RETIME_INVALID, RETIME_SKIPPED = 1, 2, 4
# include/loik_amd_plan.h: certified RRT-Connect planning of joint-space paths; its own header and version
PLAN_ABI_VERSION = 1
PLAN_SYMBOLS = ["loikb_plan_version", "loikb_plan_paths"]
PLAN_FOUND, PLAN_EXHAUSTED_ITERS, PLAN_EXHAUSTED_NODES, PLAN_START_BLOCKED, PLAN_GOAL_BLOCKED, PLAN_TOO_LONG, PLAN_INVALID = range(7)
# include/loik_amd_blend.h: certified parabolic blends, retiming through the corners of a path; its own header and version
BLEND_ABI_VERSION = 1
BLEND_SYMBOLS = ["loikb_blend_version", "loikb_blend_paths"]
BLEND_TRUNCATED, BLEND_INVALID, BLEND_SKIPPED = 1, 2, 4
BLEND_TAKEN, BLEND_BLOCKED, BLEND_UNDECIDED, BLEND_COUPLED, BLEND_ZERO_LEG, BLEND_OFF = range(6)

# include/loik_amd_grid.h: voxel worlds, an occupancy grid as a world object; its own header and version
GRID_ABI_VERSION = 1
GRID_SYMBOLS = ["loikb_grid_version", "loikb_collision_set_world_grid", "loikb_collision_get_world_grid"]
CLR_WORLD_GRID = 4
GRID_MAX_DIM, GRID_MAX_VOXELS, GRID_EMPTY = 512, 1 << 26, 0xFFFFFFFF
# include/loik_amd_gridnear.h: the nearest-voxel transform of a voxel world, and avoidance that reads the grid; its own header and version
GRIDNEAR_ABI_VERSION = 1
GRIDNEAR_SYMBOLS = ["loikb_gridnear_version", "loikb_collision_grid_set_nearest", "loikb_collision_grid_get_nearest", "loikb_grid_nearest_query"]
GRID_NO_VOXEL = 0xFFFFFFFF
# include/loik_amd_depth.h: voxel worlds from depth images and point clouds, integrated on the device; its own header and version
DEPTH_ABI_VERSION = 1
DEPTH_SYMBOLS = ["loikb_depth_version", "loikb_collision_grid_integrate_depth", "loikb_collision_grid_integrate_points",
                 "loikb_collision_grid_get_occupancy"]
DEPTH_F32, DEPTH_U16 = 0, 1
DEPTH_REPLACE, DEPTH_FUSE = 0, 1
DEPTH_Q_DEVICE = 2
DEPTH_MAX_IMAGE, DEPTH_MAX_FILTER = 4096, 64


class PoseParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("gain", C.c_double), ("tol_pose", C.c_double), ("max_steps", C.c_int), ("flags", C.c_int)]


class StepParams(C.Structure):
    _fields_ = [("shrink", C.c_double), ("sufficient", C.c_double), ("max_backtracks", C.c_int), ("patience", C.c_int), ("flags", C.c_int)]


class DexterityParams(C.Structure):
    _fields_ = [("length", C.c_double), ("flags", C.c_int)]


class ClearanceParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("flags", C.c_int)]


class MotionParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("tol", C.c_double), ("max_evals", C.c_int), ("flags", C.c_int)]


class DepthCamera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("T_world_cam", C.c_double * 12), ("depth_scale", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double)]


class DepthParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("carve", C.c_int), ("band", C.c_double), ("filter_pad", C.c_double), ("flags", C.c_int)]


class AvoidParams(C.Structure):
    _fields_ = [("d_safe", C.c_double), ("d_influence", C.c_double), ("kappa", C.c_double), ("flags", C.c_int)]


class ShortcutParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("tol", C.c_double), ("max_evals", C.c_int), ("rounds", C.c_int), ("seed", C.c_ulonglong), ("flags", C.c_int)]


class RetimeParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("flags", C.c_int)]


class PlanParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("tol", C.c_double), ("step", C.c_double), ("seed", C.c_ulonglong), ("max_evals", C.c_int),
                ("max_iters", C.c_int), ("max_nodes", C.c_int), ("flags", C.c_int)]


class BlendParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("tol", C.c_double), ("reach", C.c_double), ("dt", C.c_double), ("max_evals", C.c_int),
                ("max_tries", C.c_int), ("flags", C.c_int)]


class MultiStartParams(C.Structure):
    _fields_ = [("seeds_per_goal", C.c_int), ("rounds", C.c_int), ("seed", C.c_ulonglong), ("pick", C.c_int), ("flags", C.c_int)]


class PathParams(C.Structure):
    _fields_ = [("n_waypoints", C.c_int), ("max_steps_per_waypoint", C.c_int), ("record", C.c_int), ("flags", C.c_int)]


class TrackParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("gain", C.c_double), ("tol_track", C.c_double), ("n_steps", C.c_int), ("feedforward", C.c_int),
                ("record", C.c_int), ("flags", C.c_int)]


_lib = None


def lib():
    """Load libloik_amd.so; fail loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError("loik_amd: %s is missing -- build the HIP extension first "
                          "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback"
                          % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    L.loikb_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.loikb_destroy.argtypes = [C.c_void_p]
    L.loikb_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    sig = [C.c_void_p, C.c_void_p, _dp, _dp, _ip, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
           C.c_int]
    L.loikb_solve_init.argtypes = sig
    L.loikb_solve_full.argtypes = sig
    L.loikb_solve.argtypes = [C.c_void_p]
    L.loikb_integrate.argtypes = [C.c_void_p, C.c_double]
    L.loikb_synchronize.argtypes = [C.c_void_p]
    L.loikb_plan_string.argtypes = [C.c_void_p]
    L.loikb_pass.argtypes = [C.c_void_p, C.c_int]
    L.loikb_plan_string.restype = C.c_char_p
    L.loikb_sweep_schedule.argtypes = [_ip, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _ip]
    L.loikb_solve_tailored.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_update_references.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
    L.loikb_update_eq_constraint.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_add_eq_constraint.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_remove_eq_constraint.argtypes = [C.c_void_p, C.c_int]
    L.loikb_num_eq_c.argtypes = [C.c_void_p]
    L.loikb_eq_c_capacity.argtypes = [C.c_void_p]
    L.loikb_active_constraint_ids.argtypes = [C.c_void_p, _ip, C.c_int]
    L.loikb_get_solver_info.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, _ip]
    L.loikb_solver_info_rows_cap.argtypes = [C.c_void_p]
    L.loikb_solver_info_truncated.argtypes = [C.c_void_p]
    L.loikb_set_max_iter.argtypes = [C.c_void_p, C.c_int]
    for n in ["loikb_set_rho", "loikb_set_mu", "loikb_set_tol_primal_inf", "loikb_set_tol_tail_solve"]:
        getattr(L, n).argtypes = [C.c_void_p, C.c_double]
    L.loikb_set_tol.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.loikb_set_warm_start.argtypes = [C.c_void_p, C.c_int]
    L.loikb_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_get_results.argtypes = [C.c_void_p, C.c_uint, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    L.loikb_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    for n in ["loikb_batch", "loikb_nv", "loikb_njoints"]:
        getattr(L, n).argtypes = [C.c_void_p]
    L.loikb_last_error.restype = C.c_char_p
    L.loikb_status_string.argtypes = [C.c_int]
    L.loikb_status_string.restype = C.c_char_p
    L.loikb_builtin_model.argtypes = [C.c_char_p, C.POINTER(ModelDesc), C.POINTER(_dp), C.POINTER(_dp)]
    L.loikb_builtin_joint_name.argtypes = [C.c_char_p, C.c_int]
    L.loikb_builtin_joint_name.restype = C.c_char_p
    L.loikb_builtin_joint_id.argtypes = [C.c_char_p, C.c_char_p]
    L.loikb_flat_schedule.argtypes = [_ip, C.c_int, _ip, C.c_int, _ip]
    L.loikb_flat_variant.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip]
    L.loikb_solve_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PoseParams)]
    L.loikb_forward_kinematics.argtypes = [C.c_void_p, _ip, C.c_int, C.c_void_p, C.c_int]
    L.loikb_pose_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_set_joint_limits.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
    L.loikb_update_ineq_constraints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.loikb_pose_get_limit_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_pose_set_tasks.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
    L.loikb_pose_clear_tasks.argtypes = [C.c_void_p]
    L.loikb_pose_get_tasks.argtypes = [C.c_void_p, _ip, _dp, C.c_int]
    L.loikb_frame_placements.argtypes = [C.c_void_p, _ip, _dp, C.c_int, C.c_void_p, C.c_int]
    L.loikb_multistart_set_ranges.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
    L.loikb_multistart_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_int]
    L.loikb_solve_pose_multistart.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PoseParams), C.POINTER(MultiStartParams)]
    L.loikb_multistart_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_solve_pose_path.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PoseParams), C.POINTER(PathParams)]
    L.loikb_path_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_track_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(TrackParams)]
    L.loikb_track_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_set_joint_accel_limits.argtypes = [C.c_void_p, _dp, C.c_int]
    L.loikb_accel_set_start_velocity.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_accel_get_velocity.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_pose_set_step_control.argtypes = [C.c_void_p, C.POINTER(StepParams)]
    L.loikb_pose_get_step_control.argtypes = [C.c_void_p, C.POINTER(StepParams)]
    L.loikb_step_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_frame_jacobians.argtypes = [C.c_void_p, _ip, _dp, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.loikb_frame_dexterity.argtypes = [C.c_void_p, _ip, _dp, _ip, C.c_int, C.POINTER(DexterityParams), C.c_void_p, C.c_int]
    L.loikb_dexterity_set_multistart_pick.argtypes = [C.c_void_p, C.POINTER(DexterityParams)]
    L.loikb_dexterity_get_multistart_pick.argtypes = [C.c_void_p, C.POINTER(DexterityParams)]
    L.loikb_collision_set_spheres.argtypes = [C.c_void_p, _ip, _dp, C.c_int]
    L.loikb_collision_set_world.argtypes = [C.c_void_p, _dp, C.c_int, _dp, C.c_int]
    L.loikb_collision_set_self_pairs.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
    L.loikb_collision_num_self_pairs.argtypes = [C.c_void_p]
    L.loikb_clearance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_clearance_set_multistart.argtypes = [C.c_void_p, C.POINTER(ClearanceParams)]
    L.loikb_clearance_get_multistart.argtypes = [C.c_void_p, C.POINTER(ClearanceParams)]
    L.loikb_clearance_get_multistart_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_difference.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.loikb_motion_clearance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(MotionParams), C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_motion_clearance_path.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(MotionParams), C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_clearance_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_avoid_set.argtypes = [C.c_void_p, C.POINTER(AvoidParams)]
    L.loikb_avoid_get.argtypes = [C.c_void_p, C.POINTER(AvoidParams)]
    L.loikb_avoid_box.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, _dp, _dp, C.POINTER(AvoidParams), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_avoid_get_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.loikb_shortcut_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ShortcutParams), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_path_length.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.loikb_retime_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(RetimeParams), C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_plan_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.POINTER(PlanParams), C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_blend_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(BlendParams), C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_collision_set_world_grid.argtypes = [C.c_void_p, C.c_void_p, _ip, _dp, C.c_double, C.c_int]
    L.loikb_collision_get_world_grid.argtypes = [C.c_void_p, _ip, _dp, _dp, C.c_void_p, C.c_int]
    L.loikb_collision_grid_set_nearest.argtypes = [C.c_void_p, C.c_int]
    L.loikb_collision_grid_get_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_collision_grid_integrate_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _ip, _dp, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
                                                       C.c_int, C.c_void_p]
    L.loikb_collision_grid_integrate_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                        C.c_void_p]
    L.loikb_collision_grid_get_occupancy.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loikb_grid_nearest_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    if L.loikb_version() != ABI_VERSION:
        raise ImportError("loik_amd: %s has ABI version %d, this binding was written for %d -- rebuild the library"
                          % (_LIB_PATH, L.loikb_version(), ABI_VERSION))
    _lib = L
    return L


def device_count():
    return int(lib().loikb_device_count())


def sweep_schedule(parents, team, direction):
    """Step schedule of a tree sweep for a team of `team` wavefronts (host-only introspection, no device).
    Returns (joint[team][T], flags[team][T], slot[team][T], n_lds_slots); direction 0 = leaf->root, 1 = root->leaf."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    nj = int(parents.shape[0])
    cap = nj
    joint = np.zeros((team, cap), dtype=np.int32)
    flags = np.zeros((team, cap), dtype=np.int32)
    slot = np.zeros((team, cap), dtype=np.int32)
    nslots = C.c_int(0)
    T = lib().loikb_sweep_schedule(parents.ctypes.data_as(_ip), nj, int(team), int(direction), cap,
                                   joint.ctypes.data_as(_ip), flags.ctypes.data_as(_ip), slot.ctypes.data_as(_ip),
                                   C.byref(nslots))
    if T < 0:
        _check(T)
    return joint[:, :T].copy(), flags[:, :T].copy(), slot[:, :T].copy(), int(nslots.value)


def flat_schedule(parents):
    """The flat engine's schedule of a tree (host-only introspection, loikb_flat_schedule): None when the engine does not apply
    (loikb_last_error says why), else a dict: G, nanc, nscan, njmp and per lane depth / size / jmp / anc / red / helper / part."""
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    meta = np.zeros(5, dtype=np.int32)
    L = lib()
    need = L.loikb_flat_schedule(parents.ctypes.data_as(_ip), int(parents.size), None, 0, meta.ctypes.data_as(_ip))
    if need < 0:
        _check(need)
    if not meta[0]:
        return None
    out = np.zeros(need, dtype=np.int32)
    _check(L.loikb_flat_schedule(parents.ctypes.data_as(_ip), int(parents.size), out.ctypes.data_as(_ip), need, meta.ctypes.data_as(_ip)))
    G = int(meta[1])
    rec = out.reshape(G, -1)
    return dict(G=G, nanc=int(meta[2]), nscan=int(meta[3]), njmp=int(meta[4]), depth=rec[:, 0].copy(), size=rec[:, 1].copy(),
                jmp=rec[:, 2:7].copy(), anc=rec[:, 7:23].copy(), red=rec[:, 23:31].copy(), helper=rec[:, 31].copy(),
                part=rec[:, 32:40].copy())


def flat_variant(kind, hm, sliced, logging, mur):
    """(SLICED, HM, LOG, MUR) of the k_flat2 (kind 2) / k_flat1 (kind 1) instantiation a launch runs (host-only, loikb_flat_variant)."""
    out = (C.c_int * 4)()
    _check(lib().loikb_flat_variant(int(kind), int(hm), int(sliced), int(logging), int(mur), out))
    return bool(out[0]), int(out[1]), bool(out[2]), int(out[3])


def _check(rc):
    if rc != 0:
        L = lib()
        msg = L.loikb_last_error().decode() if rc <= -20 or rc == -7 else L.loikb_status_string(rc).decode()
        if not msg:
            msg = L.loikb_status_string(rc).decode()
        raise LoikError(rc, msg)


# JointModelFreeFlyer / Spherical / Translation (LOIKB_J_FREEFLYER, _SPHERICAL, _TRANSLATION)
J_FREEFLYER, J_SPHERICAL, J_TRANSLATION = 9, 10, 11
# JointModelSphericalZYX, JointModelPlanar, JointModelRUBX / RUBY / RUBZ
J_SPHERICAL_ZYX, J_PLANAR, J_RUBX, J_RUBY, J_RUBZ = 12, 13, 14, 15, 16
J_COMPOSITE = 17  # JointModelComposite (Model(..., composite={joint: [(jtype, axis, placement12), ...]}); sub-joints: any type but a composite)
J_RUBU = 18       # JointModelRevoluteUnboundedUnaligned: nq 2 (cos, sin), nv 1, about `axis`
J_HX, J_HY, J_HZ, J_HU = 19, 20, 21, 22   # JointModelHelicalX / Y / Z / Unaligned: nq = nv = 1, S = [pitch a; a] (Model(..., pitch=[nj]))
JOINT_NQ = {J_FREEFLYER: 7, J_SPHERICAL: 4, J_TRANSLATION: 3, J_SPHERICAL_ZYX: 3, J_PLANAR: 4, J_RUBX: 2, J_RUBY: 2, J_RUBZ: 2, J_RUBU: 2}
JOINT_NV = {J_FREEFLYER: 6, J_SPHERICAL: 3, J_TRANSLATION: 3, J_SPHERICAL_ZYX: 3, J_PLANAR: 3}


class Model:
    """Kinematic tree with Pinocchio's member names: njoints, nq, nv, parents, jointPlacements (here `placement`,
    [nj][12] = R row-major + t), joint type / axis / idx_q / idx_v per joint."""

    def __init__(self, parents, jtype, axis, placement, names=None, q_lo=None, q_hi=None, name="custom", composite=None, pitch=None):
        self.parents = np.ascontiguousarray(parents, dtype=np.int32)
        self.jtype = np.ascontiguousarray(jtype, dtype=np.int32)
        self.axis = np.ascontiguousarray(axis, dtype=np.float64).reshape(-1, 3)
        self.placement = np.ascontiguousarray(placement, dtype=np.float64).reshape(-1, 12)
        self.njoints = int(self.parents.size)
        # JointModelHelical*: pitch [njoints] (translation along the axis per radian)
        self.pitch = None if pitch is None else np.ascontiguousarray(pitch, dtype=np.float64).reshape(self.njoints)
        # JointModelComposite: composite[i] = [(sub-joint type, axis [3], placement [12] relative to the previous sub-joint), ...]
        # (a helical sub-joint: a 4-tuple, the pitch last)
        self.composite = {int(i): [(int(e[0]), np.asarray(e[1], dtype=np.float64).reshape(3), np.asarray(e[2], dtype=np.float64).reshape(12))
                                   for e in subs] for i, subs in (composite or {}).items()}
        sub_pitch = {int(i): [float(e[3]) if len(e) > 3 else 0.0 for e in subs] for i, subs in (composite or {}).items()}
        self.comp_first = np.zeros(self.njoints, dtype=np.int32); self.comp_count = np.zeros(self.njoints, dtype=np.int32)
        ct, ca, cp, cpi = [], [], [], []
        for i in sorted(self.composite):
            self.comp_first[i] = len(ct); self.comp_count[i] = len(self.composite[i])
            for (t, a, P), ph in zip(self.composite[i], sub_pitch[i]):
                ct.append(t); ca.append(a); cp.append(P); cpi.append(ph)
        self.comp_pitch = np.ascontiguousarray(cpi if cpi else [0.0], dtype=np.float64)
        self.comp_jtype = np.ascontiguousarray(ct if ct else [0], dtype=np.int32)
        self.comp_axis = np.ascontiguousarray(ca if ca else [[0, 0, 0]], dtype=np.float64).reshape(-1, 3)
        self.comp_placement = np.ascontiguousarray(cp if cp else [[0] * 12], dtype=np.float64).reshape(-1, 12)

        def nq_of(i, t):
            if t == J_COMPOSITE:
                return sum(JOINT_NQ.get(st, 1) for st, _, _ in self.composite[i])
            return JOINT_NQ.get(t, 1)

        def nv_of(i, t):
            return sum(JOINT_NV.get(st, 1) for st, _, _ in self.composite[i]) if t == J_COMPOSITE else JOINT_NV.get(t, 1)
        # joints[i].nq() / nv() / idx_q() / idx_v() of Pinocchio: cumulative in joint order
        nqs = np.array([nq_of(i, int(t)) if i else 0 for i, t in enumerate(self.jtype)], dtype=np.int32)
        nvs = np.array([nv_of(i, int(t)) if i else 0 for i, t in enumerate(self.jtype)], dtype=np.int32)
        self.nqs, self.nvs = nqs, nvs
        self.nq, self.nv = int(nqs.sum()), int(nvs.sum())
        self.idx_q = np.ascontiguousarray(np.concatenate([[0], np.cumsum(nqs)[:-1]]), dtype=np.int32)
        self.idx_v = np.ascontiguousarray(np.concatenate([[0], np.cumsum(nvs)[:-1]]), dtype=np.int32)
        if self.njoints > 1:  # joint 0 (universe) has no coordinates; keep its index at 0 like before
            self.idx_q[0] = 0
            self.idx_v[0] = 0
        self.names = list(names) if names is not None else ["universe"] + ["joint%d" % i for i in range(1, self.njoints)]
        self.q_lo = None if q_lo is None else np.asarray(q_lo, dtype=np.float64)
        self.q_hi = None if q_hi is None else np.asarray(q_hi, dtype=np.float64)
        self.name = name

    def desc(self):
        return ModelDesc(self.njoints, self.nq, self.nv, self.parents.ctypes.data_as(_ip),
                         self.jtype.ctypes.data_as(_ip), self.axis.ctypes.data_as(_dp),
                         self.idx_q.ctypes.data_as(_ip), self.idx_v.ctypes.data_as(_ip),
                         self.placement.ctypes.data_as(_dp), self.comp_first.ctypes.data_as(_ip),
                         self.comp_count.ctypes.data_as(_ip), self.comp_jtype.ctypes.data_as(_ip),
                         self.comp_axis.ctypes.data_as(_dp), self.comp_placement.ctypes.data_as(_dp),
                         None if self.pitch is None else self.pitch.ctypes.data_as(_dp), self.comp_pitch.ctypes.data_as(_dp))

    def getJointId(self, name):
        return self.names.index(name)

    def random_configurations(self, rng, batch):
        """[batch][nq] configurations: uniform in [q_lo, q_hi] (unit box when none was given), the quaternion
        segments of free-flyer / spherical joints replaced by uniformly random unit quaternions (x, y, z, w)"""
        lo = -np.ones(self.nq) if self.q_lo is None else self.q_lo
        hi = np.ones(self.nq) if self.q_hi is None else self.q_hi
        q = rng.uniform(lo, hi, size=(batch, self.nq))
        def manifold_segments(t, o0):
            if t in (J_FREEFLYER, J_SPHERICAL):
                o = o0 + (3 if t == J_FREEFLYER else 0)
                qt = rng.normal(size=(batch, 4))
                q[:, o:o + 4] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
            elif t in (J_PLANAR, J_RUBX, J_RUBY, J_RUBZ, J_RUBU):  # the (cos, sin) pair of a random angle
                o = o0 + (2 if t == J_PLANAR else 0)
                th = rng.uniform(-np.pi, np.pi, size=batch)
                q[:, o] = np.cos(th); q[:, o + 1] = np.sin(th)
        for i in range(1, self.njoints):
            t = int(self.jtype[i])
            if t == J_COMPOSITE:
                o = int(self.idx_q[i])
                for st, _, _ in self.composite[i]:
                    manifold_segments(st, o)
                    o += JOINT_NQ.get(st, 1)
            else:
                manifold_segments(t, int(self.idx_q[i]))
        return q


def builtin_model(name):
    """'panda7' | 'panda9' | 'talos32' | 'talos32_freeflyer' | 'talos44' (tables in loik_amd/csrc/models.c)"""
    L = lib()
    d = ModelDesc()
    lo, hi = _dp(), _dp()
    if L.loikb_builtin_model(name.encode(), C.byref(d), C.byref(lo), C.byref(hi)) != 0:
        raise KeyError(name)
    nj = d.njoints
    arr = lambda p, n, t: np.ctypeslib.as_array(p, shape=(n,)).astype(t).copy()
    names = [L.loikb_builtin_joint_name(name.encode(), i).decode() for i in range(nj)]
    return Model(arr(d.parents, nj, np.int32), arr(d.jtype, nj, np.int32), arr(d.axis, 3 * nj, np.float64),
                 arr(d.placement, 12 * nj, np.float64), names, arr(lo, d.nq, np.float64),
                 arr(hi, d.nq, np.float64), name=name)


def _ptr(a):
    """host numpy array, raw device pointer (int) or object with data_ptr() (torch tensor) -> (void*, is_device)"""
    if a is None:
        return None, False
    if isinstance(a, int):
        return C.c_void_p(a), True
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()), bool(getattr(a, "is_cuda", False))
    return a.ctypes.data_as(C.c_void_p), False


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _outs(out, specs):
    """the outputs of a query call, one per (shape, dtype) of specs.  out None: fresh numpy arrays; else the caller's buffer, or
    with several outputs a tuple of them (an entry None where the C call takes NULL), each as _ptr takes it
    -> ([void* per output], out_flags, the fresh arrays or None)"""
    if out is None:
        arrs = [np.empty(shape, dtype=dtype) for shape, dtype in specs]
        return [a.ctypes.data_as(C.c_void_p) for a in arrs], 0, arrs
    ptrs = [_ptr(o) for o in (out if len(specs) > 1 else (out,))]
    return [p for p, _ in ptrs], OUT_DEVICE if any(dev for _, dev in ptrs) else 0, None


class DeviceArray:
    """a float64 array resident in the HBM of `device` (hipMalloc + one hipMemcpy): what a caller who keeps its inputs on the GPU
    hands to SolveInit / the tailored Solve (LOIKB_IN_DEVICE) -- the bindings take anything with data_ptr() / is_cuda, e.g. a
    torch tensor; this is the same without importing torch (bench.py's C4 mode, the tests)"""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            h = C.CDLL("libamdhip64.so")
            h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            h.hipFree.argtypes = [C.c_void_p]
            cls._hip = h
        return cls._hip

    def __init__(self, a, device=0):
        a = _f64(a)
        self.shape, self.size, self.ndim, self.dtype, self.is_cuda, self.device = a.shape, a.size, a.ndim, a.dtype, True, int(device)
        h = self.hip()
        if h.hipSetDevice(self.device) != 0:
            raise RuntimeError("hipSetDevice(%d) failed" % self.device)
        p = C.c_void_p()
        if h.hipMalloc(C.byref(p), a.nbytes) != 0:
            raise MemoryError("hipMalloc of %d bytes failed" % a.nbytes)
        self._p = p
        if h.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) != 0:   # hipMemcpyHostToDevice
            raise RuntimeError("hipMemcpy failed")

    def data_ptr(self):
        return self._p.value

    def numel(self):
        return self.size

    def free(self):
        if self._p is not None and self._p.value:
            self.hip().hipFree(self._p)
        self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BatchedLoik:
    """`FirstOrderLoikOptimized` over a batch of independent instances, on one MI355X.

    Constructor keywords are the reference constructor's arguments (loik-loid-optimized.hpp:129-134) plus
    `batch`, `device`, `precision`, `flags`, `max_launch_iters`."""

    def __init__(self, model, batch, max_iter=200, tol_abs=1e-3, tol_rel=1e-3, tol_primal_inf=1e-2, tol_dual_inf=1e-2,
                 rho=1e-5, mu=1e-2, mu_equality_scale_factor=1e4, mu_update_strat=0, num_eq_c=1, eq_c_dim=6,
                 warm_start=False, tol_tail_solve=1e-1, verbose=False, logging=False, device=0, precision=F64, flags=0,
                 max_launch_iters=0, compact_min_instances=0, tail_max_instances=0, eq_c_capacity=0):
        self.L = lib()
        self.model = model
        self.batch = int(batch)
        self.nc = int(num_eq_c)
        self.opts = Options(max_iter, tol_abs, tol_rel, tol_primal_inf, tol_dual_inf, rho, mu, mu_equality_scale_factor,
                            mu_update_strat, num_eq_c, eq_c_dim, int(bool(warm_start)), tol_tail_solve,
                            int(bool(verbose)), int(bool(logging)), self.batch, device, precision, flags, max_launch_iters,
                            compact_min_instances, tail_max_instances, int(eq_c_capacity))
        self._desc = model.desc()
        h = C.c_void_p()
        _check(self.L.loikb_create(C.byref(self._desc), C.byref(self.opts), C.byref(h)))
        self.h = h
        self._limits = False   # set_joint_limits left a finite limit on the handle: SolvePose returns limit_flags
        self._accel = False    # set_joint_accel_limits left a finite limit on the handle: the pose loops return limit_flags
        self._ms_goals = 0     # goals of the last SolvePoseMultiStart: the shapes of multistart_get

    def close(self):
        if getattr(self, "h", None):
            self.L.loikb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(self.L.loikb_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ------------------------------------------------------------------------------------------------------
    def SolveInit(self, q, H_ref, v_ref, active_task_constraint_ids, Ais, bis, lb, ub):
        keep, args = self._raw_args(q, H_ref, v_ref, active_task_constraint_ids, Ais, bis, lb, ub)
        _check(self.L.loikb_solve_init(*args))

    def UpdateIneqConstraints(self, lb, ub):
        """UpdateIneqConstraints(lb, ub) of the problem formulation (hpp:325-339; loikb_update_ineq_constraints): replaces the
        velocity box SolveInit set and nothing else.  [nv] = one box for the batch, [batch][nv] (host or device) = per instance."""
        nv = self.model.nv
        nbound = nv
        if not (isinstance(lb, int) or hasattr(lb, "data_ptr")):
            n = int(np.asarray(lb).size)
            if n != nv and n != nv * self.batch:
                if int(np.asarray(ub).size) != n:
                    raise ValueError("lb and ub differ in size")
                nbound = n   # (the library answers with the reference's error)
        lp, ld, lf, k0 = self._prep(lb, "lb", nbound, BOUNDS_SHARED)
        up, ud, uf, k1 = self._prep(ub, "ub", nbound, BOUNDS_SHARED)
        if lf != uf or bool(ld) != bool(ud):
            raise ValueError("lb and ub must both be shared ([nv]) or both be per instance ([batch][nv]), both host or both device")
        _check(self.L.loikb_update_ineq_constraints(self.h, lp, up, nbound, lf | (IN_DEVICE if ld and not lf else 0)))

    def set_joint_limits(self, q_lo, q_hi):
        """joint position limits [nv] (idx_v order, -inf / +inf = none) honoured by every later SolvePose (loikb_set_joint_limits);
        None, None clears them.  Only DoFs whose coordinate a plain sum advances can carry a finite limit."""
        if q_lo is None and q_hi is None:
            _check(self.L.loikb_set_joint_limits(self.h, None, None, 0))
            self._limits = False
            return
        lo = None if q_lo is None else _f64(q_lo).reshape(-1)
        hi = None if q_hi is None else _f64(q_hi).reshape(-1)
        n = int((lo if lo is not None else hi).size)
        if lo is not None and hi is not None and lo.size != hi.size:
            raise ValueError("q_lo and q_hi differ in size")
        _check(self.L.loikb_set_joint_limits(self.h, None if lo is None else lo.ctypes.data_as(_dp),
                                             None if hi is None else hi.ctypes.data_as(_dp), n))
        self._limits = bool(np.isfinite(lo).any() or np.isfinite(hi).any())

    def pose_limit_flags(self):
        """[B][nv] int of the last SolvePose with limits: LIMIT_LOWER / LIMIT_UPPER bits (loikb_pose_get_limit_flags)"""
        out = np.empty((self.batch, self.model.nv), dtype=np.int32)
        _check(self.L.loikb_pose_get_limit_flags(self.h, out.ctypes.data_as(C.c_void_p), 0))
        return out

    # ---- joint acceleration limits (include/loik_amd_accel.h) -------------------------------------------------
    def set_joint_accel_limits(self, a_max):
        """joint acceleration limits [nv] (idx_v order, entries > 0, +inf = none) honoured by every later SolvePose / SolvePosePath /
        TrackPose (loikb_set_joint_accel_limits): per step |z - z_previous| <= a_max dt, and position limits are approached at a
        velocity the joint can brake from.  None clears them."""
        if a_max is None:
            _check(self.L.loikb_set_joint_accel_limits(self.h, None, 0))
            self._accel = False
            return
        a = _f64(a_max).reshape(-1)
        _check(self.L.loikb_set_joint_accel_limits(self.h, a.ctypes.data_as(_dp), int(a.size)))
        self._accel = bool(np.isfinite(a).any())

    def set_start_velocity(self, v0):
        """the velocity [B][nv] the next pose loop on this handle starts from, then forgotten (loikb_accel_set_start_velocity): a
        host array, a raw device pointer or anything with data_ptr(); None = rest"""
        if v0 is None:
            _check(self.L.loikb_accel_set_start_velocity(self.h, None, 0))
            return
        if not (isinstance(v0, int) or (hasattr(v0, "data_ptr") and getattr(v0, "is_cuda", False))):
            v0 = _f64(v0.numpy() if hasattr(v0, "numpy") else v0)
        n = None if isinstance(v0, int) else int(v0.numel() if hasattr(v0, "numel") else v0.size)
        if n is not None and n != self.batch * self.model.nv:
            raise ValueError("v0 has %d elements, expected batch * nv = %d" % (n, self.batch * self.model.nv))
        p, dev = _ptr(v0)
        _check(self.L.loikb_accel_set_start_velocity(self.h, p, IN_DEVICE if dev else 0))

    def get_applied_velocity(self, out=None):
        """[B][nv] the velocity applied in the last step that moved each instance of the last pose loop with acceleration limits
        (loikb_accel_get_velocity; 0: never moved, reached or stopped), as a numpy array or into a device pointer / torch tensor `out`"""
        if out is not None:
            p, dev = _ptr(out)
            _check(self.L.loikb_accel_get_velocity(self.h, p, OUT_DEVICE if dev else 0))
            return out
        d = {"nv": self.model.nv}
        arr = np.empty((self.batch,) + tuple(d[x] for x in ACCEL_FIELD_DIMS["applied_velocity"]),
                       dtype=np.int32 if "applied_velocity" in ACCEL_INT_FIELDS else np.float64)
        _check(self.L.loikb_accel_get_velocity(self.h, arr.ctypes.data_as(C.c_void_p), 0))
        return arr

    # ---- step control (include/loik_amd_step.h) -----------------------------------------------------------------
    def set_step_control(self, shrink=0.5, sufficient=1e-4, max_backtracks=6, patience=0):
        """backtracking step control for every later SolvePose / SolvePoseMultiStart (loikb_pose_set_step_control): per step the
        trials q (+) alpha dt z, alpha = 1, shrink, shrink^2, ... (max_backtracks + 1 of them), the first that brings the squared pose
        error down to (1 - sufficient alpha) of its value is taken, the plain step if none; patience > 0: an instance whose
        searches failed that many times in a row is POSE_ST_STALLED and left where it was"""
        prm = StepParams(float(shrink), float(sufficient), int(max_backtracks), int(patience), 0)
        _check(self.L.loikb_pose_set_step_control(self.h, C.byref(prm)))

    def clear_step_control(self):
        _check(self.L.loikb_pose_set_step_control(self.h, None))

    def step_control(self):
        """dict(shrink, sufficient, max_backtracks, patience) as set, None when step control is not set"""
        prm = StepParams()
        if not self.L.loikb_pose_get_step_control(self.h, C.byref(prm)):
            return None
        return dict(shrink=prm.shrink, sufficient=prm.sufficient, max_backtracks=prm.max_backtracks, patience=prm.patience)

    def step_get(self, name):
        """[B] of the last SolvePose with step control (loikb_step_get): alpha / backtracks / failed"""
        fid, dtype = {"alpha": (STEP_F_ALPHA, np.float64), "backtracks": (STEP_F_BACKTRACKS, np.int32), "failed": (STEP_F_FAILED, np.int32)}[name]
        arr = np.empty(self.batch, dtype=dtype)
        _check(self.L.loikb_step_get(self.h, fid, arr.ctypes.data_as(C.c_void_p), 0))
        return arr

    def set_pose_tasks(self, kinds, frames=None):
        """one task per active constraint (active_task_constraint_ids order) for every later SolvePose (loikb_pose_set_tasks).
        kinds: TASK_POSE / TASK_POSITION / TASK_ORIENTATION or "pose" / "position" / "orientation", or with the rotation about the
        frame's z axis free (include/loik_amd_axis.h) TASK_POSE_AXIS / TASK_AXIS or "pose_axis" / "axis"; frames: iMf of the task frame
        on the constrained link, [nc][4][4] / [nc][12], None = the joint frame.  A formulation edit: every active constraint's A
        becomes the shared A_c = S_c X_c^-1 and its b zero; the handle's A must be shared."""
        kinds = [kinds] if isinstance(kinds, (str, int, np.integer)) else list(kinds)
        k = np.empty(len(kinds), dtype=np.int32)
        for i, x in enumerate(kinds):
            if isinstance(x, str):
                names = dict(TASK_KINDS, **AXIS_TASK_KINDS)
                if x not in names:
                    raise ValueError("task kind %r: expected one of %s" % (x, sorted(names)))
                x = names[x]
            k[i] = int(x)
        fp = None
        if frames is not None:
            f = self._placements12(frames, "frames").reshape(-1, 12)
            if f.shape[0] != k.size:
                raise ValueError("frames: %d placements for %d kinds" % (f.shape[0], k.size))
            fp = f.ctypes.data_as(_dp)
        _check(self.L.loikb_pose_set_tasks(self.h, int(k.size), k.ctypes.data_as(_ip), fp))

    def clear_pose_tasks(self):
        """drops the task specification (loikb_pose_clear_tasks); A and b stay as they are"""
        _check(self.L.loikb_pose_clear_tasks(self.h))

    def pose_tasks(self):
        """the tasks in force (loikb_pose_get_tasks): a list of (kind name, iMf [4][4]) per active constraint; [] when there are none"""
        n = int(self.L.loikb_pose_get_tasks(self.h, None, None, 0))
        if n <= 0:
            return []
        k, f = np.zeros(n, dtype=np.int32), np.zeros((n, 12))
        self.L.loikb_pose_get_tasks(self.h, k.ctypes.data_as(_ip), f.ctypes.data_as(_dp), n)
        names = {v: key for key, v in dict(TASK_KINDS, **AXIS_TASK_KINDS).items()}
        return [(names[int(k[c])], self._to44(f[c:c + 1])[0]) for c in range(n)]

    @staticmethod
    def _to44(a12):
        """[..][12] (R row-major, t) -> [..][4][4]"""
        M = np.zeros(a12.shape[:-1] + (4, 4))
        M[..., :3, :3] = a12[..., :9].reshape(a12.shape[:-1] + (3, 3))
        M[..., :3, 3] = a12[..., 9:]
        M[..., 3, 3] = 1.0
        return M

    def _prep(self, a, what, per, shared_flag):
        """One per-instance input: (void*, is_device, flag).  The C-ABI takes bare pointers without lengths, so the sizes are
        validated HERE: a host array must hold exactly `per` elements (one value shared by the whole batch -> `shared_flag`)
        or `batch * per` (instance-major).  Device pointers / torch tensors are per-instance by contract; a torch tensor's
        numel is checked, a raw integer pointer cannot be."""
        B = self.batch
        if isinstance(a, int):
            return C.c_void_p(a), True, 0, None
        if hasattr(a, "data_ptr"):
            n = int(a.numel()) if hasattr(a, "numel") else None
            if n is not None and n != B * per:
                raise ValueError("%s: device tensor has %d elements, expected batch * %d = %d" % (what, n, per, B * per))
            if getattr(a, "is_cuda", False):
                return C.c_void_p(a.data_ptr()), True, 0, a
            a = a.numpy() if hasattr(a, "numpy") else np.asarray(a)
        a = _f64(a)
        if a.size == B * per and not (B == 1 and shared_flag in (A_SHARED, BOUNDS_SHARED)):
            return a.ctypes.data_as(C.c_void_p), False, 0, a         # (batch 1: q / b count as per-instance, A / box as shared)
        if a.size == per:
            return a.ctypes.data_as(C.c_void_p), False, shared_flag, a
        raise ValueError("%s has %d elements: expected %d (shared by the batch) or batch * %d = %d (instance-major)"
                         % (what, a.size, per, per, B * per))

    def _raw_args(self, q, H_ref, v_ref, c_ids, Ais, bis, lb, ub):
        """marshal SolveInit / Solve(q,H_ref,...) arguments; array lengths are checked here (see _prep), the reference's
        own validation (constraint count, bound dimension, duplicates) is the library's and comes back as its error codes"""
        B, nv, nq = self.batch, self.model.nv, self.model.nq
        H_ref = _f64(H_ref); v_ref = _f64(v_ref)
        if H_ref.size != 36 or v_ref.size != 6:
            raise ValueError("H_ref must be 6x6 and v_ref a 6-vector")
        H_ref = H_ref.reshape(36); v_ref = v_ref.reshape(6)
        c_ids = np.ascontiguousarray(c_ids, dtype=np.int32).reshape(-1)
        ncin = int(c_ids.size)
        # lb/ub dimension: the library compares it with model.nv and returns the reference's error (hpp:328-335)
        nbound = nv
        if not (isinstance(lb, int) or hasattr(lb, "data_ptr")):
            n = int(np.asarray(lb).size)
            if n != nv and n != nv * B:
                if int(np.asarray(ub).size) != n:
                    raise ValueError("lb and ub differ in size")
                nbound = n
        qp, qd, qf, k0 = self._prep(q, "q", nq, Q_SHARED)
        Ap, Ad, Af, k1 = self._prep(Ais, "Ais", 36 * ncin, A_SHARED) if ncin else (None, None, 0, None)
        bp, bd, bf, k2 = self._prep(bis, "bis", 6 * ncin, B_SHARED) if ncin else (None, None, 0, None)
        lp, ld, lf, k3 = self._prep(lb, "lb", nbound, BOUNDS_SHARED)
        up, ud, uf, k4 = self._prep(ub, "ub", nbound, BOUNDS_SHARED)
        if lf != uf:
            raise ValueError("lb and ub must both be shared ([nv]) or both be per instance ([batch][nv])")
        flags = qf | Af | bf | lf
        # device residency is one flag for all per-instance inputs: those that are not shared must agree
        devs = [d for d, f in ((qd, qf), (Ad, Af), (bd, bf), (ld, lf), (ud, uf)) if d is not None and not f]
        if any(devs):
            if not all(devs):
                raise ValueError("per-instance inputs must be all host or all device arrays")
            flags |= IN_DEVICE
        keep = [H_ref, v_ref, c_ids, k0, k1, k2, k3, k4]
        args = (self.h, qp, H_ref.ctypes.data_as(_dp), v_ref.ctypes.data_as(_dp), c_ids.ctypes.data_as(_ip), ncin, Ap,
                bp, lp, up, nbound, flags)
        return keep, args

    def Solve(self, *a):
        """Solve() | Solve(q,H_ref,v_ref,ids,Ais,bis,lb,ub) | Solve(q,c_id,Ai,bi); q=None in the tailored form uses
        the configurations resident on the device (outer loop: integrate(dt) then Solve(None, c_id, Ai, bi))"""
        if len(a) == 0:
            _check(self.L.loikb_solve(self.h))
        elif len(a) == 8:
            keep, args = self._raw_args(*a)
            _check(self.L.loikb_solve_full(*args))
        elif len(a) == 4:
            q, c_id, Ai, bi = a
            qp, qd, qf = None, None, 0
            if q is not None:  # None: the q resident on the device
                qp, qd, qf, k0 = self._prep(q, "q", self.model.nq, Q_SHARED)
            if int(c_id) < 0:  # no constraint update: solve on the set AddEqConstraint / RemoveEqConstraint left
                flags = qf | (IN_DEVICE if qd and not qf else 0)
                _check(self.L.loikb_solve_tailored(self.h, qp, -1, None, None, flags))
                return
            Ap, Ad, Af, k1 = self._prep(Ai, "Ai", 36, A_SHARED)
            bp, bd, bf, k2 = self._prep(bi, "bi", 6, B_SHARED)
            flags = qf | Af | bf
            devs = [d for d, f in ((qd, qf), (Ad, Af), (bd, bf)) if d is not None and not f]
            if any(devs):
                if not all(devs):
                    raise ValueError("per-instance inputs must be all host or all device arrays")
                flags |= IN_DEVICE
            _check(self.L.loikb_solve_tailored(self.h, qp, int(c_id), Ap, bp, flags))
        else:
            raise TypeError("Solve() takes 0, 4 or 8 arguments")

    # IkProblemFormulationOptimized's editing methods (ik-id-description-optimized.hpp; `problem_` is protected upstream)
    def UpdateReferences(self, H_refs, v_refs):
        """one weight [6][6] and one target [6] per joint of the model incl. the universe (hpp:103-121); in force for Solve() /
        the tailored Solve until the next SolveInit broadcasts one pair again"""
        H = _f64(np.asarray(H_refs, dtype=np.float64).reshape(-1, 36)); v = _f64(np.asarray(v_refs, dtype=np.float64).reshape(-1, 6))
        n = H.shape[0] if H.shape[0] == v.shape[0] else -1
        _check(self.L.loikb_update_references(self.h, H.ctypes.data_as(_dp), v.ctypes.data_as(_dp), n))

    def _edit_args(self, Ai, bi):
        Ap, Ad, Af, k1 = (None, None, 0, None) if Ai is None else self._prep(Ai, "Ai", 36, A_SHARED)
        bp, bd, bf, k2 = self._prep(bi, "bi", 6, B_SHARED)
        flags = Af | bf
        devs = [d for d, f in ((Ad, Af), (bd, bf)) if d is not None and not f]
        if any(devs):
            if not all(devs):
                raise ValueError("per-instance inputs must be all host or all device arrays")
            flags |= IN_DEVICE
        return Ap, bp, flags, (k1, k2)

    def UpdateEqConstraint(self, c_id, *a):
        """UpdateEqConstraint(c_id, Ai, bi) (hpp:178-218) | UpdateEqConstraint(c_id, bi) (hpp:224-238)"""
        Ai, bi = (None, a[0]) if len(a) == 1 else a
        Ap, bp, flags, keep = self._edit_args(Ai, bi)
        _check(self.L.loikb_update_eq_constraint(self.h, int(c_id), Ap, bp, flags))

    def AddEqConstraint(self, c_id, Ai, bi):
        """hpp:244-286; needs a free slot (constructor keyword eq_c_capacity)"""
        Ap, bp, flags, keep = self._edit_args(Ai, bi)
        _check(self.L.loikb_add_eq_constraint(self.h, int(c_id), Ap, bp, flags))

    def RemoveEqConstraint(self, c_id):
        """hpp:292-319; False when there was nothing to remove (upstream: a warning on stderr)"""
        rc = self.L.loikb_remove_eq_constraint(self.h, int(c_id))
        if rc < 0:
            _check(rc)
        return rc == 0

    def active_task_constraint_ids(self):
        n = self.L.loikb_num_eq_c(self.h)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self.L.loikb_active_constraint_ids(self.h, out.ctypes.data_as(_ip), n)
        return [int(x) for x in out[:n]]

    # pass-level public methods of the reference (loik-loid-optimized.hpp:192-264): the debug path of loik_passes.hpp
    def _pass(self, k): _check(self.L.loikb_pass(self.h, k))
    def BeginIteration(self): self._pass(0)   # iter_++, UpdatePrev(), ResetInfNorms() (hpp:381-388)
    def FwdPass1(self): self._pass(1)
    def BwdPassOptimizedVisitor(self): self._pass(2)
    def FwdPass2OptimizedVisitor(self): self._pass(3)
    def BoxProj(self): self._pass(4)
    def DualUpdate(self): self._pass(5)
    def ComputeResiduals(self): self._pass(6)
    def CheckConvergence(self): self._pass(7)
    def CheckFeasibility(self): self._pass(8)
    def UpdateMu(self): self._pass(9)

    def plan(self):
        """which kernels this handle's solves use, and why (loikb_plan_string)"""
        return self.L.loikb_plan_string(self.h).decode()

    def synchronize(self):
        """hipDeviceSynchronize on the solver's device (bench.py's timing bracket)"""
        _check(self.L.loikb_synchronize(self.h))

    def integrate(self, dt):
        """outer loop on the device: q <- q (+) dt * z of the last solve, q stays resident in HBM"""
        _check(self.L.loikb_integrate(self.h, float(dt)))

    # ---- batched pose IK (include/loik_amd_pose.h) ----------------------------------------------------------
    def _placements12(self, a, what):
        """host placements [..][4][4] or [..][12] -> float64 [..][12] (R row-major, then t)"""
        a = _f64(a)
        if a.shape[-2:] == (4, 4):
            a = np.concatenate([a[..., :3, :3].reshape(a.shape[:-2] + (9,)), a[..., :3, 3]], axis=-1)
        elif a.shape[-1] != 12:
            raise ValueError("%s: placements are [..][4][4] or [..][12], got shape %s" % (what, a.shape))
        return np.ascontiguousarray(a)

    def SolvePose(self, targets, dt=1.0, gain=1.0, tol_pose=1e-6, max_steps=100, q=None):
        """global IK on the device (loikb_solve_pose): per step e_c = log6(oMi_c^-1 oMdes_c), b_c = A_c (gain / dt) e_c, the
        tailored Solve on the resident q (warm_start as the handle says), q <- q (+) dt z for the instances not yet reached.
        targets: one placement per active constraint (active_task_constraint_ids order), [B][nc][4][4] / [B][nc][12], or
        [nc][4][4] / [nc][12] (/ [4][4] / [12] for one constraint) shared by the batch; a device tensor is [B][nc][12] or
        [nc][12] by its numel.  q: None = the resident configurations, else [B][nq] replaces them first.
        Returns dict(reached [B] bool, steps [B], err [B][nc][6] = e_c of the final q, status [B] POSE_ST_* bits), and with joint
        position limits (set_joint_limits) or acceleration limits (set_joint_accel_limits) on the handle limit_flags [B][nv], and with
        step control (set_step_control) alpha [B], backtracks [B], failed [B] and stalled [B] bool (POSE_ST_STALLED)."""
        B, nc = self.batch, int(self.L.loikb_num_eq_c(self.h))
        flags, keep = 0, []
        if isinstance(targets, int) or (hasattr(targets, "data_ptr") and getattr(targets, "is_cuda", False)):
            n = None if isinstance(targets, int) else int(targets.numel())
            if n is not None and n not in (B * nc * 12, nc * 12):
                raise ValueError("targets: device tensor has %d elements, expected batch * nc * 12 or nc * 12" % n)
            tp = C.c_void_p(targets if isinstance(targets, int) else targets.data_ptr())
            flags |= IN_DEVICE
            if n == nc * 12 and B > 1:
                flags |= POSE_TARGET_SHARED
        else:
            t = self._placements12(targets.numpy() if hasattr(targets, "numpy") else targets, "targets")
            if t.size == B * nc * 12:
                pass
            elif t.size == nc * 12:
                flags |= POSE_TARGET_SHARED
            else:
                raise ValueError("targets: %d placements, expected batch * nc = %d or nc = %d" % (t.size // 12, B * nc, nc))
            keep.append(t)
            tp = t.ctypes.data_as(C.c_void_p)
        qp = None
        if q is not None:
            if isinstance(q, int) or (hasattr(q, "data_ptr") and getattr(q, "is_cuda", False)):
                if not flags & IN_DEVICE:
                    raise ValueError("q and targets must both be host arrays or both device pointers")
                qp = C.c_void_p(q if isinstance(q, int) else q.data_ptr())
            else:
                if flags & IN_DEVICE:
                    raise ValueError("q and targets must both be host arrays or both device pointers")
                qa = _f64(q)
                if qa.size != B * self.model.nq:
                    raise ValueError("q has %d elements, expected batch * nq = %d" % (qa.size, B * self.model.nq))
                keep.append(qa)
                qp = qa.ctypes.data_as(C.c_void_p)
        prm = PoseParams(float(dt), float(gain), float(tol_pose), int(max_steps), 0)
        _check(self.L.loikb_solve_pose(self.h, qp, tp, flags, C.byref(prm)))
        status = np.empty(B, dtype=np.int32)
        steps = np.empty(B, dtype=np.int32)
        err = np.empty((B, nc, 6))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STATUS, status.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STEPS, steps.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_ERR, err.ctypes.data_as(C.c_void_p), 0))
        out = dict(reached=(status & POSE_ST_REACHED) != 0, steps=steps, err=err, status=status)
        if self._limits or self._accel:
            out["limit_flags"] = self.pose_limit_flags()
        self._avoid_results(out)
        if self.step_control() is not None:
            out.update(alpha=self.step_get("alpha"), backtracks=self.step_get("backtracks"), failed=self.step_get("failed"),
                       stalled=(status & POSE_ST_STALLED) != 0)
        return out

    def pose_timing(self):
        """of the last SolvePose: dict(steps, total_ms, solve_ms, other_ms) -- wall clock; other = re-target, b, integrate, read-backs"""
        t = np.zeros(4)
        _check(self.L.loikb_pose_get(self.h, POSE_F_TIMING, t.ctypes.data_as(C.c_void_p), 0))
        return dict(steps=int(t[0]), total_ms=float(t[1]), solve_ms=float(t[2]), other_ms=float(t[3]))

    def forward_kinematics(self, links):
        """world placements oMi of `links` (the caller's joint ids) for the resident q: [B][n][4][4]"""
        links = np.ascontiguousarray(np.atleast_1d(links), dtype=np.int32)
        n = int(links.size)
        out = np.empty((self.batch, n, 12))
        _check(self.L.loikb_forward_kinematics(self.h, links.ctypes.data_as(_ip), n, out.ctypes.data_as(C.c_void_p), 0))
        M = np.zeros((self.batch, n, 4, 4))
        M[..., :3, :3] = out[..., :9].reshape(self.batch, n, 3, 3)
        M[..., :3, 3] = out[..., 9:]
        M[..., 3, 3] = 1.0
        return M

    def frame_placements(self, links, frames=None):
        """world placements oMf = oMi(links[e]) * frames[e] for the resident q (loikb_frame_placements): [B][n][4][4]; frames
        [n][4][4] / [n][12], None = forward_kinematics(links)"""
        links = np.ascontiguousarray(np.atleast_1d(links), dtype=np.int32)
        n = int(links.size)
        fp = None
        if frames is not None:
            f = self._placements12(frames, "frames").reshape(-1, 12)
            if f.shape[0] != n:
                raise ValueError("frames: %d placements for %d links" % (f.shape[0], n))
            fp = f.ctypes.data_as(_dp)
        out = np.empty((self.batch, n, 12))
        _check(self.L.loikb_frame_placements(self.h, links.ctypes.data_as(_ip), fp, n, out.ctypes.data_as(C.c_void_p), 0))
        return self._to44(out)

    # ---- frame Jacobians and dexterity (include/loik_amd_jacobian.h) ----------------------------------------
    def _links_frames(self, links, frames):
        """(links int32 [n], n, frames float64 [n][12] or None) of the two getters"""
        links = np.ascontiguousarray(np.atleast_1d(links), dtype=np.int32)
        n = int(links.size)
        f = None
        if frames is not None:
            f = self._placements12(frames, "frames").reshape(-1, 12)
            if f.shape[0] != n:
                raise ValueError("frames: %d placements for %d links" % (f.shape[0], n))
        return links, n, f

    def frame_jacobians(self, links, frames=None, reference="local", out=None):
        """J [B][n][6][nv] with v_f = J nu for the resident q (loikb_frame_jacobians): v_f = [linear; angular] of the frame
        oMi(links[e]) * frames[e], nu in idx_v order.  frames [n][4][4] / [n][12], None = the joint frames; reference: "local" (in
        the frame), "local_world_aligned" (the frame's origin, the world's axes) or "world", or a JAC_* value.  A numpy array, or
        into a device pointer / torch tensor `out` of B * n * 6 * nv float64."""
        links, n, f = self._links_frames(links, frames)
        if isinstance(reference, str):
            if reference not in JAC_REFERENCES:
                raise ValueError("reference %r: expected one of %s" % (reference, sorted(JAC_REFERENCES)))
            reference = JAC_REFERENCES[reference]
        fp = None if f is None else f.ctypes.data_as(_dp)
        (p,), oflags, new = _outs(out, [((self.batch, n, 6, self.model.nv), np.float64)])
        _check(self.L.loikb_frame_jacobians(self.h, links.ctypes.data_as(_ip), fp, n, int(reference), p, oflags))
        return out if new is None else new[0]

    def frame_dexterity(self, links=None, frames=None, rows=None, length=1.0):
        """singular values, Yoshikawa manipulability and inverse condition number of the task Jacobian of the resident q
        (loikb_frame_dexterity): of D S_r J_local, D = diag(1/length x 3, 1 x 3), S_r the rows the 6-bit mask rows[e] selects (None =
        all six) of the frame oMi(links[e]) * frames[e].  links=None: the handle's tasks -- the active constraint links with the
        frames and rows of set_pose_tasks (identity and all six rows without tasks).
        Returns dict(sigma [B][n][6] descending, zero past the selected rows; manipulability [B][n]; inv_condition [B][n])."""
        prm = DexterityParams(float(length), 0)
        if links is None:
            if frames is not None or rows is not None:
                raise ValueError("links=None takes the frames and rows of the handle's tasks: give neither")
            n = int(self.L.loikb_num_eq_c(self.h))
            lp = fp = rp = None
        else:
            links, n, f = self._links_frames(links, frames)
            lp = links.ctypes.data_as(_ip)
            fp = None if f is None else f.ctypes.data_as(_dp)
            rp = None
            if rows is not None:
                r = np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
                if r.size != n:
                    raise ValueError("rows: %d masks for %d links" % (r.size, n))
                rp = r.ctypes.data_as(_ip)
        out = np.empty((self.batch, max(n, 0), DEX_N))
        _check(self.L.loikb_frame_dexterity(self.h, lp, fp, rp, n, C.byref(prm), out.ctypes.data_as(C.c_void_p), 0))
        return dict(sigma=out[..., :6].copy(), manipulability=out[..., DEX_MANIPULABILITY].copy(), inv_condition=out[..., DEX_INV_CONDITION].copy())

    def set_multistart_pick_dexterous(self, length=1.0):
        """every later SolvePoseMultiStart picks, among the reached seeds of a goal, the one whose worst task has the largest
        smallest singular value (loikb_dexterity_set_multistart_pick): cost = -min_c sigma_min of frame_dexterity(links=None, length)"""
        prm = DexterityParams(float(length), 0)
        _check(self.L.loikb_dexterity_set_multistart_pick(self.h, C.byref(prm)))

    def clear_multistart_pick_dexterous(self):
        _check(self.L.loikb_dexterity_set_multistart_pick(self.h, None))

    def multistart_pick_dexterous(self):
        """dict(length) as set, None when the dexterous pick is not set"""
        prm = DexterityParams()
        if not self.L.loikb_dexterity_get_multistart_pick(self.h, C.byref(prm)):
            return None
        return dict(length=prm.length)

    # ---- collision clearance (include/loik_amd_collision.h) --------------------------------------------------
    def set_collision_spheres(self, links, spheres):
        """the robot's sphere model (loikb_collision_set_spheres): links [ns] joint ids (0 = the universe), spheres [ns][4] = (x, y, z, r) in
        the link's frame.  Empty arrays clear the spheres and the self pairs."""
        links = np.ascontiguousarray(np.atleast_1d(links), dtype=np.int32).reshape(-1)
        sph = _f64(spheres).reshape(-1, 4)
        if sph.shape[0] != links.size:
            raise ValueError("spheres: %d rows for %d links" % (sph.shape[0], links.size))
        _check(self.L.loikb_collision_set_spheres(self.h, links.ctypes.data_as(_ip), sph.ctypes.data_as(_dp), int(links.size)))
        self._n_spheres = int(links.size)   # (avoidance_box sizes its per-sphere outputs by it)

    def set_collision_world(self, spheres=None, boxes=None):
        """the world every instance shares (loikb_collision_set_world): spheres [nws][4] = (x, y, z, r); boxes [nwb][15] = (R row-major, p,
        half extents), or a list of (T [4][4], half_extents [3]).  None, None clears the world."""
        ws = np.zeros((0, 4)) if spheres is None else _f64(spheres).reshape(-1, 4)
        if boxes is None:
            wb = np.zeros((0, 15))
        elif isinstance(boxes, np.ndarray):
            wb = _f64(boxes).reshape(-1, 15)
        else:
            rows = []
            for bx in boxes:
                if len(bx) == 2:
                    T, h = np.asarray(bx[0], dtype=np.float64), np.asarray(bx[1], dtype=np.float64).reshape(3)
                    rows.append(np.concatenate([T[:3, :3].reshape(9), T[:3, 3], h]))
                else:
                    rows.append(np.asarray(bx, dtype=np.float64).reshape(15))
            wb = _f64(rows).reshape(-1, 15)
        _check(self.L.loikb_collision_set_world(self.h, ws.ctypes.data_as(_dp), int(ws.shape[0]), wb.ctypes.data_as(_dp), int(wb.shape[0])))

    def set_self_collision(self, enable=True, ignore=()):
        """self pairs on or off (loikb_collision_set_self_pairs): with enable the sphere pairs (a < b) whose links differ, are not parent
        and child and are not in ignore [(link_i, link_j), ...] (either order)"""
        ig = np.ascontiguousarray(np.asarray(list(ignore), dtype=np.int32).reshape(-1, 2))
        _check(self.L.loikb_collision_set_self_pairs(self.h, 1 if enable else 0, ig.ctypes.data_as(_ip), int(ig.shape[0])))

    def num_self_pairs(self):
        return int(self.L.loikb_collision_num_self_pairs(self.h))

    def clearance(self, q=None, out=None):
        """the minimum clearance of configurations and the pair that achieves it (loikb_clearance).  q None: the resident q of the batch;
        else [n][nq] on the host, or a device pointer / torch tensor (then give n rows by its numel; a raw pointer as (ptr, n)).
        Returns dict(min [n], min_world [n], min_self [n], witness [n][3] = (CLR_* kind, robot sphere, obstacle or other sphere)), or
        with out = (min_dev, witness_dev) device buffers of 3 n float64 / 3 n int32 (witness_dev may be None) writes there and returns out."""
        qp, n, flags, keep = self._q_rows(q)
        (mp, wp), oflags, new = _outs(out, [((n, 3), np.float64), ((n, 3), np.int32)])
        _check(self.L.loikb_clearance(self.h, qp, n, flags, mp, wp, oflags))
        if new is None:
            return out
        mins, wit = new
        return dict(min=mins[:, 0].copy(), min_world=mins[:, 1].copy(), min_self=mins[:, 2].copy(), witness=wit)

    # ---- voxel worlds (include/loik_amd_grid.h) ---------------------------------------------------------------------
    def set_collision_grid(self, occupancy, origin=None, voxel=None):
        """the voxel world every instance shares (loikb_collision_set_world_grid): occupancy [nz][ny][nx] of any integer or bool dtype
        (nonzero = occupied) on the host, or a uint8 device tensor of that shape; origin [3] the world position of the low corner of
        voxel (0, 0, 0); voxel the edge.  The distance field is built on the device before the call returns; clearance, the
        collision-aware multi-start and the motion layer read it beside the world of set_collision_world.  None clears the grid."""
        if occupancy is None:
            _check(self.L.loikb_collision_set_world_grid(self.h, None, None, None, 0.0, 0))
            return
        if origin is None or voxel is None:
            raise ValueError("set_collision_grid: an occupancy needs origin and voxel")
        if hasattr(occupancy, "data_ptr") and getattr(occupancy, "is_cuda", False):
            if getattr(occupancy, "element_size", lambda: 1)() != 1:
                raise ValueError("set_collision_grid: a device occupancy must be uint8")
            if hasattr(occupancy, "is_contiguous") and not occupancy.is_contiguous():
                raise ValueError("set_collision_grid: a device occupancy must be contiguous")
            shape, keep, ptr, flags = tuple(int(d) for d in occupancy.shape), occupancy, C.c_void_p(occupancy.data_ptr()), IN_DEVICE
        else:
            keep = np.ascontiguousarray(np.asarray(occupancy.numpy() if hasattr(occupancy, "numpy") else occupancy) != 0, dtype=np.uint8)
            shape, ptr, flags = keep.shape, keep.ctypes.data_as(C.c_void_p), 0
        if len(shape) != 3:
            raise ValueError("set_collision_grid: occupancy must be [nz][ny][nx]")
        dims = np.array([shape[2], shape[1], shape[0]], dtype=np.int32)
        org = _f64(origin).reshape(3)
        _check(self.L.loikb_collision_set_world_grid(self.h, ptr, dims.ctypes.data_as(_ip), org.ctypes.data_as(_dp), float(voxel), flags))

    def collision_grid(self, field=True):
        """dict(dims (nx, ny, nz), origin [3], voxel, G uint32 [nz][ny][nx]) of the grid that is set (loikb_collision_get_world_grid), None
        when none is.  (voxel / 2) sqrt(G) is the distance from a voxel's centre to the occupied cubes, GRID_EMPTY where nothing is
        occupied.  field=False leaves G out and copies nothing."""
        dims = np.zeros(3, dtype=np.int32)
        org = np.zeros(3)
        h = C.c_double()
        rc = self.L.loikb_collision_get_world_grid(self.h, dims.ctypes.data_as(_ip), org.ctypes.data_as(_dp), C.byref(h), None, 0)
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        out = dict(dims=(int(dims[0]), int(dims[1]), int(dims[2])), origin=org, voxel=h.value)
        if field:
            G = np.empty((int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.uint32)
            rc = self.L.loikb_collision_get_world_grid(self.h, None, None, None, G.ctypes.data_as(C.c_void_p), 0)
            if rc < 0:
                _check(rc)
            out["G"] = G
        return out

    # ---- the nearest-voxel transform (include/loik_amd_gridnear.h) --------------------------------------------------
    def set_collision_grid_nearest(self, on=True):
        """the latch of the nearest-voxel transform (loikb_collision_grid_set_nearest): with it on, every grid that is set gets its
        transform F beside the field, and collision avoidance (set_collision_avoidance, clearance_gradient, avoidance_box) reads the
        grid as one more world object of every sphere.  on=False drops it."""
        _check(self.L.loikb_collision_grid_set_nearest(self.h, int(on)))

    def collision_grid_nearest(self):
        """F uint32 [nz][ny][nx]: for every voxel the linear index (z ny + y) nx + x of the occupied voxel nearest to it, the lowest index
        among several, GRID_NO_VOXEL in an empty grid (loikb_collision_grid_get_nearest); None without a grid or without the latch"""
        rc = self.L.loikb_collision_grid_get_nearest(self.h, None, 0)
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        nx, ny, nz = self.collision_grid(field=False)["dims"]
        F = np.empty((nz, ny, nx), dtype=np.uint32)
        rc = self.L.loikb_collision_grid_get_nearest(self.h, F.ctypes.data_as(C.c_void_p), 0)
        if rc < 0:
            _check(rc)
        return F

    def grid_nearest(self, spheres, out=None):
        """the grid pair with a direction of spheres [n][4] = x y z r in the world frame, host or device (loikb_grid_nearest_query):
        dict(val [n][2] = (the lower bound v, d_u - r with d_u the distance to the chosen cube), vox [n][2] = (the voxel read, the chosen
        cube; -1 in an empty grid), normal [n][3]); or with out = (val_dev, vox_dev, normal_dev) writes there and returns out."""
        sp, n, dev, keep = self._rows(spheres, 4)
        ptrs, oflags, new = _outs(out, [((n, 2), np.float64), ((n, 2), np.int32), ((n, 3), np.float64)])
        _check(self.L.loikb_grid_nearest_query(self.h, sp, n, IN_DEVICE if dev else 0, *ptrs, oflags))
        return out if new is None else dict(zip(("val", "vox", "normal"), new))

    # ---- depth images and point clouds (include/loik_amd_depth.h) ----------------------------------------------------
    def _depth_call(self, what, dims, origin, voxel, mode, carve, band, filter_q, filter_pad, call):
        modes = {"replace": DEPTH_REPLACE, "fuse": DEPTH_FUSE}
        if mode not in modes:
            raise ValueError("%s: mode must be 'replace' or 'fuse'" % what)
        edge = float(voxel)
        cover = 0.5 * np.sqrt(3.0) * edge   # what band and filter_pad must at least cover (loik_amd_depth.h)
        prm = DepthParams(modes[mode], int(bool(carve)), float(cover if band is None else band) if carve else float(band or 0.0),
                          float(cover if filter_pad is None else filter_pad), 0)
        flags, keep = 0, None
        if filter_q is None:
            qp, nf = None, 0
        elif isinstance(filter_q, (int, np.integer)) and not isinstance(filter_q, bool):
            qp, nf = None, int(filter_q)   # the first n resident configurations
        else:
            qp, nf, dev, keep = self._rows(filter_q, self.model.nq)
            flags = DEPTH_Q_DEVICE if dev else 0
        dm = np.asarray(dims, dtype=np.int32).reshape(3)
        org = _f64(origin).reshape(3)
        st = np.zeros(4, dtype=np.int64)
        _check(call(dm.ctypes.data_as(_ip), org.ctypes.data_as(_dp), edge, C.byref(prm), qp, nf, flags, st.ctypes.data_as(C.c_void_p)))
        return dict(returns=int(st[0]), inside=int(st[1]), occupied_before=int(st[2]), occupied_after=int(st[3]))

    def integrate_depth(self, depth, camera, dims, origin, voxel, mode="replace", carve=False, band=None, filter_q=None, filter_pad=None):
        """a depth image into the voxel world (loikb_collision_grid_integrate_depth): depth [height][width] float32 or uint16, a host array
        or a device tensor; camera a DepthCamera or a dict(fx, fy, cx, cy, T_world_cam [12] = (R row-major, p), z_min, z_max,
        depth_scale=1.0) whose width and height come from the image; dims (nx, ny, nz), origin [3] and voxel as set_collision_grid.
        mode "replace": the frame alone; "fuse": onto the occupancy of the grid that is set, with carve=True less the voxels the frame
        sees through by more than band.  filter_q: configurations [n][nq] (host or device) whose collision spheres, padded by filter_pad,
        are cut out; an int n: the first n resident configurations.  band and filter_pad default to (sqrt(3) / 2) voxel.  Returns
        dict(returns, inside, occupied_before, occupied_after)."""
        if hasattr(depth, "data_ptr") and getattr(depth, "is_cuda", False):
            if not depth.is_contiguous():
                raise ValueError("integrate_depth: a device image must be contiguous")
            size = depth.element_size()
            if size not in (2, 4):   # (by element size: four bytes are taken as float32, two as uint16)
                raise ValueError("integrate_depth: a device image must be float32 or uint16")
            shape, keep, ptr, dtype, dflag = tuple(int(d) for d in depth.shape), depth, C.c_void_p(depth.data_ptr()), DEPTH_F32 if size == 4 else DEPTH_U16, IN_DEVICE
        else:
            a = np.asarray(depth.numpy() if hasattr(depth, "numpy") else depth)
            if a.dtype not in (np.float32, np.uint16):
                raise ValueError("integrate_depth: the image must be float32 or uint16")
            keep = np.ascontiguousarray(a)
            shape, ptr, dtype, dflag = keep.shape, keep.ctypes.data_as(C.c_void_p), DEPTH_F32 if keep.dtype == np.float32 else DEPTH_U16, 0
        if len(shape) != 2:
            raise ValueError("integrate_depth: the image must be [height][width]")
        if isinstance(camera, DepthCamera):
            cam = camera
        else:
            T = _f64(camera["T_world_cam"]).reshape(12)
            cam = DepthCamera(int(shape[1]), int(shape[0]), float(camera["fx"]), float(camera["fy"]), float(camera["cx"]), float(camera["cy"]),
                              (C.c_double * 12)(*T), float(camera.get("depth_scale", 1.0)), float(camera["z_min"]), float(camera["z_max"]))
        return self._depth_call("integrate_depth", dims, origin, voxel, mode, carve, band, filter_q, filter_pad,
                                lambda dm, org, edge, prm, qp, nf, qflag, st: self.L.loikb_collision_grid_integrate_depth(
                                    self.h, ptr, dtype, C.byref(cam), dm, org, edge, prm, qp, nf, dflag | qflag, st))

    def integrate_points(self, points, dims, origin, voxel, mode="replace", filter_q=None, filter_pad=None):
        """world points [n][3] (host or device float64) into the voxel world (loikb_collision_grid_integrate_points): as integrate_depth
        from its step 3 on; points have no camera, so nothing is carved"""
        pp, n, dev, keep = self._rows(points, 3)
        return self._depth_call("integrate_points", dims, origin, voxel, mode, False, None, filter_q, filter_pad,
                                lambda dm, org, edge, prm, qp, nf, qflag, st: self.L.loikb_collision_grid_integrate_points(
                                    self.h, pp, n, dm, org, edge, prm, qp, nf, (IN_DEVICE if dev else 0) | qflag, st))

    def collision_occupancy(self):
        """uint8 [nz][ny][nx], 1 = occupied: the occupancy of the grid that is set, whichever call set it
        (loikb_collision_grid_get_occupancy); None without a grid"""
        rc = self.L.loikb_collision_grid_get_occupancy(self.h, None, 0)
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        nx, ny, nz = self.collision_grid(field=False)["dims"]
        occ = np.empty((nz, ny, nx), dtype=np.uint8)
        rc = self.L.loikb_collision_grid_get_occupancy(self.h, occ.ctypes.data_as(C.c_void_p), 0)
        if rc < 0:
            _check(rc)
        return occ

    # ---- collision avoidance (include/loik_amd_avoid.h) -------------------------------------------------------------
    def set_collision_avoidance(self, d_safe, d_influence, kappa=0.5):
        """every later pose loop (SolvePose, SolvePosePath, TrackPose, SolvePoseMultiStart) narrows the velocity box of each step so
        that the spheres keep away from the world and from each other (loikb_avoid_set): a constraint is active below d_influence, one
        step may spend the share kappa of d - d_safe, and at or below d_safe no DoF may approach"""
        prm = AvoidParams(float(d_safe), float(d_influence), float(kappa), 0)
        _check(self.L.loikb_avoid_set(self.h, C.byref(prm)))

    def clear_collision_avoidance(self):
        _check(self.L.loikb_avoid_set(self.h, None))

    def collision_avoidance(self):
        """dict(d_safe, d_influence, kappa) as set, None when collision avoidance is not set"""
        prm = AvoidParams()
        if not self.L.loikb_avoid_get(self.h, C.byref(prm)):
            return None
        return dict(d_safe=prm.d_safe, d_influence=prm.d_influence, kappa=prm.kappa)

    def avoid_get(self, name):
        """one result of the last pose loop that ran with collision avoidance (loikb_avoid_get_result): min_seen [B] / active_steps [B] /
        flags [B][nv]"""
        fid, dtype, per = {"min_seen": (AVOID_F_MIN_SEEN, np.float64, 1), "active_steps": (AVOID_F_ACTIVE_STEPS, np.int32, 1),
                           "flags": (AVOID_F_FLAGS, np.int32, self.model.nv)}[name]
        out = np.empty((self.batch, per) if per > 1 else self.batch, dtype=dtype)
        _check(self.L.loikb_avoid_get_result(self.h, fid, out.ctypes.data_as(C.c_void_p), 0))
        return out

    def _avoid_results(self, out):
        if self.collision_avoidance() is not None:
            out.update(avoid_min_seen=self.avoid_get("min_seen"), avoid_active_steps=self.avoid_get("active_steps"),
                       avoid_flags=self.avoid_get("flags"))

    def _q_rows(self, q):
        """q of a query: None (the resident q), a host array, a device tensor or (ptr, n) -> (void*, n, in_flags, keep-alive)"""
        if q is None:
            return None, self.batch, 0, None
        p, n, dev, keep = self._rows(q, self.model.nq)
        return p, n, IN_DEVICE if dev else 0, keep

    def clearance_gradient(self, q=None, out=None):
        """clearance() plus the derivative of the witness pair's clearance with respect to the joint velocities
        (loikb_clearance_gradient): dict(min [n], min_world [n], min_self [n], witness [n][3], grad [n][nv]) with d(min)/dt = grad . z
        under integrate.  With out = (min_dev, witness_dev, grad_dev) device buffers of 3 n float64 / 3 n int32 / n nv float64 writes there
        and returns out."""
        qp, n, flags, keep = self._q_rows(q)
        (mp, wp, gp), oflags, new = _outs(out, [((n, 3), np.float64), ((n, 3), np.int32), ((n, self.model.nv), np.float64)])
        _check(self.L.loikb_clearance_gradient(self.h, qp, n, flags, mp, wp, gp, oflags))
        if new is None:
            return out
        mins, wit, grad = new
        return dict(min=mins[:, 0].copy(), min_world=mins[:, 1].copy(), min_self=mins[:, 2].copy(), witness=wit, grad=grad)

    def avoidance_box(self, q, dt, lb, ub, d_safe, d_influence, kappa=0.5, out=None):
        """the velocity box a pose step with collision avoidance would hand its inner solve, as a pure query (loikb_avoid_box): the
        shared box [lb, ub] [nv] narrowed for each row of q (None: the resident q).  Returns dict(lo [n][nv], hi [n][nv], pairs [n][ns][2] =
        each sphere's nearest-world and nearest-self clearance, partner [n][ns][2] = the world object (spheres first, then nws + box) /
        the other sphere, or -1), or with out = (lo_dev, hi_dev, pairs_dev, partner_dev) writes there and returns out."""
        qp, n, flags, keep = self._q_rows(q)
        nv = self.model.nv
        lb, ub = self._dof_row(lb), self._dof_row(ub)
        prm = AvoidParams(float(d_safe), float(d_influence), float(kappa), 0)
        ns = getattr(self, "_n_spheres", 0)
        ptrs, oflags, new = _outs(out, [((n, nv), np.float64), ((n, nv), np.float64), ((n, ns, 2), np.float64), ((n, ns, 2), np.int32)])
        _check(self.L.loikb_avoid_box(self.h, qp, n, flags, float(dt), lb.ctypes.data_as(_dp), ub.ctypes.data_as(_dp), C.byref(prm), *ptrs, oflags))
        return out if new is None else dict(zip(("lo", "hi", "pairs", "partner"), new))

    def _dof_row(self, x):
        """a scalar or [nv] -> a contiguous float64 [nv]"""
        return np.ascontiguousarray(np.broadcast_to(_f64(x), (self.model.nv,)))

    # ---- motions (include/loik_amd_motion.h) ----------------------------------------------------------------------
    def _rows(self, a, width):
        """a host array or device tensor of rows of `width` doubles -> (void*, rows, is_device, keep-alive)"""
        if isinstance(a, tuple):
            return C.c_void_p(int(a[0])), int(a[1]), True, None
        if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
            return C.c_void_p(a.data_ptr()), int(a.numel()) // width, True, a
        keep = _f64(a.numpy() if hasattr(a, "numpy") else a).reshape(-1, width)
        return keep.ctypes.data_as(C.c_void_p), int(keep.shape[0]), False, keep

    def difference(self, q0, q1, out=None):
        """v [n][nv] with q0 (+) v = q1 under integrate's arithmetic (loikb_difference).  q0, q1 [n][nq] both on the host or both on the
        device; with out = a device buffer of n nv float64 writes there and returns out."""
        p0, n, dev, k0 = self._rows(q0, self.model.nq)
        p1, n1, dev1, k1 = self._rows(q1, self.model.nq)
        if n != n1 or dev != dev1:
            raise ValueError("difference: q0 and q1 differ in rows or in where they live")
        (pv,), oflags, new = _outs(out, [((n, self.model.nv), np.float64)])
        _check(self.L.loikb_difference(self.h, p0, p1, n, IN_DEVICE if dev else 0, pv, oflags))
        return out if new is None else new[0]

    @staticmethod
    def _motion_result(val, info):
        return dict(status=info[:, 0].copy(), evals=info[:, 1].copy(), s_free=val[:, 0].copy(), min_sampled=val[:, 1].copy(),
                    s_at_min=val[:, 2].copy(), witness=info[:, 2:5].copy())

    def motion_clearance(self, qa, qb=None, dv=None, margin=0.0, tol=1e-3, max_evals=256, out=None):
        """the certified check of the segments q(s) = qa (+) s dv, s in [0, 1] (loikb_motion_clearance), against the sphere model, the
        world and the self pairs of the handle.  Give dv [n][nv], or qb [n][nq] (then dv = difference(qa, qb)); qa and dv / qb both on the
        host or both on the device.  Returns dict(status [n] MOTION_*, evals [n], s_free [n], min_sampled [n], s_at_min [n], witness
        [n][3]), or with out = (val_dev, info_dev) device buffers of 3 n float64 / 5 n int32 writes there and returns out."""
        if (qb is None) == (dv is None):
            raise ValueError("motion_clearance: give exactly one of qb and dv")
        tmp = None
        if dv is None:
            if hasattr(qb, "data_ptr") and getattr(qb, "is_cuda", False):
                tmp = dv = self.difference(qa, qb, out=DeviceArray(np.empty(int(qb.numel()) // self.model.nq * self.model.nv)))
            else:
                dv = self.difference(qa, qb)
        pa, n, dev, ka = self._rows(qa, self.model.nq)
        pd, nd, devd, kd = self._rows(dv, self.model.nv)
        if n != nd or dev != devd:
            raise ValueError("motion_clearance: qa and dv differ in rows or in where they live")
        prm = MotionParams(float(margin), float(tol), int(max_evals), 0)
        (pv, pi), oflags, new = _outs(out, [((n, 3), np.float64), ((n, 5), np.int32)])
        try:
            _check(self.L.loikb_motion_clearance(self.h, pa, pd, n, IN_DEVICE if dev else 0, C.byref(prm), pv, pi, oflags))
        finally:
            if tmp is not None:
                tmp.free()
        return out if new is None else self._motion_result(*new)

    def path_clearance(self, q_path, margin=0.0, tol=1e-3, max_evals=256, out=None):
        """the certified check of every segment between consecutive samples of q_path [B][T][nq] (loikb_motion_clearance_path; a host array,
        or a device tensor with that shape).  Returns the dict of motion_clearance with [B][T-1] leading axes, or writes to out = (val_dev,
        info_dev) of 3 B (T-1) float64 / 5 B (T-1) int32."""
        shape = tuple(q_path.shape)
        if len(shape) != 3 or shape[2] != self.model.nq:
            raise ValueError("path_clearance: q_path must be [B][T][nq]")
        B, T = int(shape[0]), int(shape[1])
        pq, _, dev, keep = self._rows(q_path, self.model.nq)
        prm = MotionParams(float(margin), float(tol), int(max_evals), 0)
        n = B * max(T - 1, 0)
        (pv, pi), oflags, new = _outs(out, [((n, 3), np.float64), ((n, 5), np.int32)])
        _check(self.L.loikb_motion_clearance_path(self.h, pq, B, T, IN_DEVICE if dev else 0, C.byref(prm), pv, pi, oflags))
        if new is None:
            return out
        r = self._motion_result(*new)
        return {k: v.reshape((B, T - 1) + v.shape[1:]) for k, v in r.items()}

    # ---- shortcutting (include/loik_amd_shortcut.h) ---------------------------------------------------------------
    def _paths(self, who, q_path, n_waypoints):
        """q_path [B][T][nq] and n_waypoints [B] (or None) on the host, or both on the device (n_waypoints then int32) ->
        (void* q, void* len, B, T, is_device, keep-alive)"""
        shape = tuple(q_path.shape)
        if len(shape) != 3 or shape[2] != self.model.nq:
            raise ValueError("%s: q_path must be [B][T][nq]" % who)
        B, T = int(shape[0]), int(shape[1])
        pq, _, dev, keep = self._rows(q_path, self.model.nq)
        pl, kl = None, None
        if n_waypoints is not None:
            if hasattr(n_waypoints, "data_ptr") and getattr(n_waypoints, "is_cuda", False):
                if not dev:
                    raise ValueError("%s: q_path and n_waypoints differ in where they live" % who)
                pl, kl = C.c_void_p(n_waypoints.data_ptr()), n_waypoints
            else:
                if dev:
                    raise ValueError("%s: q_path and n_waypoints differ in where they live" % who)
                kl = np.ascontiguousarray(n_waypoints.numpy() if hasattr(n_waypoints, "numpy") else n_waypoints, dtype=np.int32).reshape(-1)
                if kl.size != B:
                    raise ValueError("%s: n_waypoints must be [B]" % who)
                pl = kl.ctypes.data_as(C.c_void_p)
        return pq, pl, B, T, dev, (keep, kl)

    def shortcut_paths(self, q_path, n_waypoints=None, rounds=64, seed=0, margin=0.0, tol=1e-3, max_evals=256, out=None):
        """certified shortcutting of the paths q_path [B][T][nq] (loikb_shortcut_paths): per path `rounds` draws of a sub-path whose straight
        joint-space segment replaces it when the check of motion_clearance certifies the segment FREE.  n_waypoints [B]: the leading rows
        of each path that are waypoints (None: T), e.g. the cursor of SolvePosePath.  q_path and n_waypoints both on the host or both on
        the device (n_waypoints then int32).  Returns dict(q_path [B][T][nq], n_waypoints [B], keep [B][T] (input row indices, -1 after),
        tried, accepted, blocked, undecided, invalid [B], length_in, length_out [B]), or with out = (path_dev, keep_dev, info_dev, val_dev)
        device buffers of B T nq float64 / B T int32 / 6 B int32 / 2 B float64 (keep_dev and val_dev may be None) writes there and
        returns out."""
        pq, pl, B, T, dev, alive = self._paths("shortcut_paths", q_path, n_waypoints)
        prm = ShortcutParams(float(margin), float(tol), int(max_evals), int(rounds), int(seed) % (1 << 64), 0)
        ptrs, oflags, new = _outs(out, [((B, T, self.model.nq), np.float64), ((B, T), np.int32), ((B, 6), np.int32), ((B, 2), np.float64)])
        _check(self.L.loikb_shortcut_paths(self.h, pq, pl, B, T, IN_DEVICE if dev else 0, C.byref(prm), *ptrs, oflags))
        return out if new is None else self._shortcut_result(*new)

    @staticmethod
    def _shortcut_result(path, keep, info, val):
        r = dict(q_path=path, n_waypoints=info[:, 0].copy(), keep=keep)
        for k, name in enumerate(("tried", "accepted", "blocked", "undecided", "invalid")):
            r[name] = info[:, k + 1].copy()
        r["length_in"], r["length_out"] = val[:, 0].copy(), val[:, 1].copy()
        return r

    def path_length(self, q_path, n_waypoints=None, out=None):
        """the joint-space length [B] of the paths q_path [B][T][nq] (loikb_path_length): the sum over consecutive waypoints of the norm of
        their difference().  n_waypoints as shortcut_paths takes it; with out = a device buffer of B float64 writes there and returns out."""
        pq, pl, B, T, dev, alive = self._paths("path_length", q_path, n_waypoints)
        (pn,), oflags, new = _outs(out, [((B,), np.float64)])
        _check(self.L.loikb_path_length(self.h, pq, pl, B, T, IN_DEVICE if dev else 0, pn, oflags))
        return out if new is None else new[0]

    # ---- retiming (include/loik_amd_retime.h) --------------------------------------------------------------------
    def _timed_paths(self, who, fn, prm, q_path, n_waypoints, v_max, a_max, max_samples, out, tail, info_at, pack):
        """the body retime_paths and blend_paths share.  fn: the C entry point, prm its params struct; tail(B, T): the (shape, dtype) of
        its outputs after (traj, vel), number info_at of them info [B][4]; pack(traj, vel, *tail arrays): the result"""
        pq, pl, B, T, dev, alive = self._paths(who, q_path, n_waypoints)
        vm, am = self._dof_row(v_max), self._dof_row(a_max)
        specs = tail(B, T)

        def call(S, ptrs, oflags):
            _check(fn(self.h, pq, pl, B, T, IN_DEVICE if dev else 0, vm.ctypes.data_as(_dp), am.ctypes.data_as(_dp), C.byref(prm), S, *ptrs, oflags))
        if out is not None:
            if max_samples is None:
                raise ValueError("%s: out needs max_samples" % who)
            ptrs, oflags, _ = _outs(out, [None] * (2 + len(specs)))
            call(int(max_samples), ptrs, oflags)
            return out
        ptail, _, arrs = _outs(None, specs)
        if max_samples is None:
            call(0, [None, None] + ptail, 0)
            max_samples = max(int(arrs[info_at][:, 0].max(initial=1)), 1)
        S = int(max_samples)
        traj = vel = None
        if S > 0:
            traj, vel = np.empty((B, S, self.model.nq)), np.empty((B, S, self.model.nv))
        call(S, [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in (traj, vel)] + ptail, 0)
        return pack(traj, vel, *arrs)

    def retime_paths(self, q_path, v_max, a_max, dt, n_waypoints=None, max_samples=None, snap=False, out=None):
        """time-optimal retiming of the paths q_path [B][T][nq] under the per-DoF limits v_max, a_max [nv] (host, or scalars) at the sample
        period dt (loikb_retime_paths): every segment from rest to rest on a trapezoid of its path parameter, so that every sample lies on
        a segment of the input.  n_waypoints as shortcut_paths takes it.  max_samples = the rows S of the result; None sizes S to the
        largest n_samples with a timing-only call first, 0 is a timing-only call.  snap stretches every segment to whole samples
        (RETIME_SNAP).  Returns dict(q_traj [B][S][nq], v_traj [B][S][nv], n_samples, n_waypoints, moved, flags [B], duration [B], seg
        [B][T-1][4] = (t_start, duration, t_acc, peak)); q_traj and v_traj are None after a timing-only call.  With out = (traj_dev,
        vel_dev, seg_dev, duration_dev, info_dev) device buffers of B S nq / B S nv / 4 B (T-1) / B float64 and 4 B int32 (the first three
        may be None; max_samples is then required) writes there and returns out."""
        prm = RetimeParams(float(dt), RETIME_SNAP if snap else 0)
        return self._timed_paths("retime_paths", self.L.loikb_retime_paths, prm, q_path, n_waypoints, v_max, a_max, max_samples, out,
                                 lambda B, T: [((B, max(T - 1, 0), 4), np.float64), ((B,), np.float64), ((B, 4), np.int32)], 2,
                                 self._retime_result)

    @staticmethod
    def _retime_result(traj, vel, seg, dur, info):
        return dict(q_traj=traj, v_traj=vel, n_samples=info[:, 0].copy(), n_waypoints=info[:, 1].copy(), moved=info[:, 2].copy(),
                    flags=info[:, 3].copy(), duration=dur, seg=seg)

    # ---- blending (include/loik_amd_blend.h) ---------------------------------------------------------------------
    def blend_paths(self, q_path, v_max, a_max, dt, reach, n_waypoints=None, max_samples=None, margin=0.0, tol=1e-3, max_evals=256, max_tries=4,
                    out=None):
        """retiming of the paths q_path [B][T][nq] through their corners (loikb_blend_paths): every corner is replaced by a parabola of
        half-length at most `reach` (halved up to max_tries - 1 times) when the advancement of motion_clearance certifies the curve at a
        clearance >= margin against the handle's sphere model, and is then run through at a constant rate; a corner that is not
        certified stops as in retime_paths.  v_max, a_max, dt, n_waypoints and max_samples as retime_paths takes them.  Returns
        dict(q_traj [B][S][nq], v_traj [B][S][nv], n_samples, n_waypoints, taken, flags [B], duration [B], corner [B][T-2][5] = (l, r_in,
        r_out, rate, min_sampled), corner_info [B][T-2][6] = (status BLEND_*, tries, evals, witness kind, a, b), piece [B][2T-3][4] =
        (t_start, duration, v0 or rate, v1 or rate)); q_traj and v_traj are None after a timing-only call.  With out = (traj_dev, vel_dev,
        duration_dev, info_dev, corner_dev, corner_info_dev, piece_dev) device buffers of B S nq / B S nv / B float64, 4 B int32,
        5 B (T-2) float64, 6 B (T-2) int32 and 4 B (2T-3) float64 (all but duration_dev and info_dev may be None; max_samples is then
        required) writes there and returns out."""
        prm = BlendParams(float(margin), float(tol), float(reach), float(dt), int(max_evals), int(max_tries), 0)
        return self._timed_paths("blend_paths", self.L.loikb_blend_paths, prm, q_path, n_waypoints, v_max, a_max, max_samples, out,
                                 lambda B, T: [((B,), np.float64), ((B, 4), np.int32), ((B, max(T - 2, 0), 5), np.float64),
                                               ((B, max(T - 2, 0), 6), np.int32), ((B, max(2 * T - 3, 0), 4), np.float64)], 1,
                                 self._blend_result)

    @staticmethod
    def _blend_result(traj, vel, dur, info, corner, cinfo, piece):
        return dict(q_traj=traj, v_traj=vel, n_samples=info[:, 0].copy(), n_waypoints=info[:, 1].copy(), taken=info[:, 2].copy(),
                    flags=info[:, 3].copy(), duration=dur, corner=corner, corner_info=cinfo, piece=piece)

    # ---- planning (include/loik_amd_plan.h) ----------------------------------------------------------------------
    def plan_paths(self, q_start, q_goal, s_lo, s_hi, T, step=0.5, max_iters=256, max_nodes=256, seed=0, margin=0.0, tol=1e-3, max_evals=256,
                   out=None):
        """certified RRT-Connect planning from q_start [B][nq] to q_goal [B][nq] (loikb_plan_paths), both on the host or both on the device:
        two trees per query grow towards samples drawn from the ranges s_lo, s_hi [nv] (host; a DoF is sampled iff both are finite) by
        edges of at most `step`, and every edge is accepted only when the check of motion_clearance certifies it FREE.  T = the rows of a
        result path.  Returns dict(q_path [B][T][nq] (NaN unless FOUND; the rows after n_waypoints repeat the last), n_waypoints [B],
        status [B] PLAN_*, iterations [B], nodes [B][2], edges_checked, edges_free, evals [B], length [B]), or with out = (path_dev,
        info_dev, length_dev) device buffers of B T nq float64 / 8 B int32 / B float64 (length_dev may be None) writes there and returns
        out."""
        nq, nv = self.model.nq, self.model.nv
        ps, B, dev, k0 = self._rows(q_start, nq)
        pg, Bg, devg, k1 = self._rows(q_goal, nq)
        if B != Bg or dev != devg:
            raise ValueError("plan_paths: q_start and q_goal differ in rows or in where they live")
        lo, hi = self._dof_row(s_lo), self._dof_row(s_hi)
        T = int(T)
        prm = PlanParams(float(margin), float(tol), float(step), int(seed) % (1 << 64), int(max_evals), int(max_iters), int(max_nodes), 0)
        ptrs, oflags, new = _outs(out, [((B, max(T, 0), nq), np.float64), ((B, 8), np.int32), ((B,), np.float64)])
        _check(self.L.loikb_plan_paths(self.h, ps, pg, B, IN_DEVICE if dev else 0, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), C.byref(prm), T,
                                       *ptrs, oflags))
        return out if new is None else self._plan_result(*new)

    @staticmethod
    def _plan_result(path, info, length):
        return dict(q_path=path, n_waypoints=info[:, 1].copy(), status=info[:, 0].copy(), iterations=info[:, 2].copy(), nodes=info[:, 3:5].copy(),
                    edges_checked=info[:, 5].copy(), edges_free=info[:, 6].copy(), evals=info[:, 7].copy(), length=length)

    def set_multistart_clearance(self, margin=0.0):
        """every later SolvePoseMultiStart answers a goal only with a reached seed whose clearance is >= margin
        (loikb_clearance_set_multistart)"""
        prm = ClearanceParams(float(margin), 0)
        _check(self.L.loikb_clearance_set_multistart(self.h, C.byref(prm)))

    def clear_multistart_clearance(self):
        _check(self.L.loikb_clearance_set_multistart(self.h, None))

    def multistart_clearance(self):
        """dict(margin) as set, None when the collision-aware selection is not set"""
        prm = ClearanceParams()
        if not self.L.loikb_clearance_get_multistart(self.h, C.byref(prm)):
            return None
        return dict(margin=prm.margin)

    def multistart_clearance_get(self, name):
        """one result of the last SolvePoseMultiStart that ran with the collision-aware selection
        (loikb_clearance_get_multistart_result): clearance [G] / witness [G][3] / nclear [G] / instance [B]"""
        fid, dtype, per = {"clearance": (CLR_MS_F_CLEARANCE, np.float64, 1), "witness": (CLR_MS_F_WITNESS, np.int32, 3),
                           "nclear": (CLR_MS_F_NCLEAR, np.int32, 1), "instance": (CLR_MS_F_INSTANCE, np.float64, 1)}[name]
        big = np.empty(self.batch * per, dtype=dtype)
        _check(self.L.loikb_clearance_get_multistart_result(self.h, fid, big.ctypes.data_as(C.c_void_p), 0))
        if name == "instance":
            return big
        G = self._ms_goals
        return big[:G * per].reshape((G, 3) if per == 3 else (G,)).copy()

    # ---- multi-start pose IK (include/loik_amd_multistart.h) ------------------------------------------------
    def set_seed_ranges(self, s_lo=None, s_hi=None, weights=None):
        """the ranges [nv] (idx_v order) the seeds are drawn from (loikb_multistart_set_ranges): a DoF is sampled iff both ends are
        finite; None, None = the handle's joint limits.  weights [nv] >= 0 (None = 1): the metric of pick="nearest"."""
        arrs = [None if a is None else _f64(a).reshape(-1) for a in (s_lo, s_hi, weights)]
        sizes = {a.size for a in arrs if a is not None}
        if len(sizes) > 1:
            raise ValueError("s_lo, s_hi and weights differ in size")
        _check(self.L.loikb_multistart_set_ranges(self.h, *[None if a is None else a.ctypes.data_as(_dp) for a in arrs],
                                                  sizes.pop() if sizes else 0))

    def _goal_q0(self, q0, G, device_ok):
        """q0 of the multi-start entry points -> (void*, flags, keep-alive): None, [nq] (shared), [G][nq], or a device [G][nq]"""
        if q0 is None:
            return None, 0, None
        if isinstance(q0, int) or (hasattr(q0, "data_ptr") and getattr(q0, "is_cuda", False)):
            if not device_ok:
                raise ValueError("q0 and targets must both be host arrays or both device pointers (a shared q0 row is a host array)")
            return C.c_void_p(q0 if isinstance(q0, int) else q0.data_ptr()), IN_DEVICE, q0
        a = _f64(q0.numpy() if hasattr(q0, "numpy") else q0)
        nq = self.model.nq
        if a.size == G * nq and not (a.ndim == 1 and G == 1):
            return a.ctypes.data_as(C.c_void_p), 0, a
        if a.size == nq:
            return a.ctypes.data_as(C.c_void_p), Q_SHARED, a
        raise ValueError("q0 has %d elements: expected nq = %d (shared by the goals) or goals * nq = %d" % (a.size, nq, G * nq))

    def sample_seeds(self, seeds_per_goal, seed=0, round=0, q0=None):
        """writes the seeds of `round` into the resident q of all instances (loikb_multistart_sample) and nothing else; q0 as in
        SolvePoseMultiStart"""
        K = int(seeds_per_goal)
        qp, qf, keep = self._goal_q0(q0, self.batch // K if K >= 1 and self.batch % K == 0 else 1, True)
        _check(self.L.loikb_multistart_sample(self.h, qp, qf, int(seed), K, int(round)))

    def SolvePoseMultiStart(self, targets, seeds_per_goal, rounds=1, seed=0, pick="nearest", q0=None, dt=1.0, gain=1.0, tol_pose=1e-6,
                            max_steps=100, length=1.0, clearance_margin=None):
        """G = batch / seeds_per_goal goals, K = seeds_per_goal seeds each (loikb_solve_pose_multistart): instance g * K + k is seed k
        of goal g.  Seeds are drawn on the device inside the seed ranges (set_seed_ranges; default the joint limits), SolvePose
        runs on the whole batch, instances without REACHED are re-seeded for up to rounds - 1 restarts while a goal is
        unanswered, and one winner per goal is selected on the device.
        targets: [G][nc][4][4] / [G][nc][12], or [nc][..] shared by the goals (a device tensor by its numel).  q0: [G][nq], [nq]
        shared, None = the resident q of each goal's instance g * K; seed 0 of round 0 is q0 itself.
        pick: "nearest" (to q0), "first", or "dexterous" (include/loik_amd_jacobian.h: the reached seed whose worst task has the
        largest smallest singular value, linear rows scaled by 1 / length; set for this call alone -- a pick latched with
        set_multistart_pick_dexterous is back in force afterwards, and is what ranks the reached seeds whenever it is set).
        clearance_margin: a number sets the collision-aware selection of include/loik_amd_collision.h for this call alone (a latch set
        with set_multistart_clearance is back in force afterwards): a goal is answered only by a reached seed whose clearance is >= the
        margin, a goal with only colliding answers gets MS_GOAL_IN_COLLISION, and the result gains clearance [G], witness [G][3] and
        nclear [G] (as it does whenever the latch is set).
        Returns dict(winner [G], goal_status [G] MS_GOAL_* bits, q [G][nq], err [G][nc][6], cost [G], nreached [G], round [B],
        rounds_run, timing)."""
        if clearance_margin is not None:
            held = self.multistart_clearance()
            self.set_multistart_clearance(clearance_margin)
            try:
                return self.SolvePoseMultiStart(targets, seeds_per_goal, rounds=rounds, seed=seed, pick=pick, q0=q0, dt=dt, gain=gain,
                                                tol_pose=tol_pose, max_steps=max_steps, length=length)
            finally:
                if held is None:
                    self.clear_multistart_clearance()
                else:
                    self.set_multistart_clearance(held["margin"])
        if pick == "dexterous":
            before = self.multistart_pick_dexterous()
            self.set_multistart_pick_dexterous(length)
            try:
                return self.SolvePoseMultiStart(targets, seeds_per_goal, rounds=rounds, seed=seed, pick=MS_PICK_FIRST, q0=q0, dt=dt, gain=gain,
                                                tol_pose=tol_pose, max_steps=max_steps)
            finally:
                if before is None:
                    self.clear_multistart_pick_dexterous()
                else:
                    self.set_multistart_pick_dexterous(before["length"])
        B, nc, K = self.batch, int(self.L.loikb_num_eq_c(self.h)), int(seeds_per_goal)
        G = B // K if K >= 1 and B % K == 0 else 1   # (a K the library rejects: it says so)
        flags, keep = 0, []
        if isinstance(targets, int) or (hasattr(targets, "data_ptr") and getattr(targets, "is_cuda", False)):
            n = None if isinstance(targets, int) else int(targets.numel())
            if n is not None and n not in (G * nc * 12, nc * 12):
                raise ValueError("targets: device tensor has %d elements, expected goals * nc * 12 or nc * 12" % n)
            tp = C.c_void_p(targets if isinstance(targets, int) else targets.data_ptr())
            flags |= IN_DEVICE
            if n == nc * 12 and G > 1:
                flags |= POSE_TARGET_SHARED
        else:
            t = self._placements12(targets.numpy() if hasattr(targets, "numpy") else targets, "targets")
            if t.size == G * nc * 12:
                pass
            elif t.size == nc * 12:
                flags |= POSE_TARGET_SHARED
            else:
                raise ValueError("targets: %d placements, expected goals * nc = %d or nc = %d" % (t.size // 12, G * nc, nc))
            keep.append(t)
            tp = t.ctypes.data_as(C.c_void_p)
        qp, qf, k0 = self._goal_q0(q0, G, bool(flags & IN_DEVICE))
        if q0 is not None and not qf & Q_SHARED and bool(qf & IN_DEVICE) != bool(flags & IN_DEVICE):
            raise ValueError("q0 and targets must both be host arrays or both device pointers (a shared q0 row is a host array)")
        if isinstance(pick, str):
            if pick not in MS_PICKS:
                raise ValueError("pick %r: expected one of %s" % (pick, sorted(MS_PICKS)))
            pick = MS_PICKS[pick]
        prm = PoseParams(float(dt), float(gain), float(tol_pose), int(max_steps), 0)
        msp = MultiStartParams(K, int(rounds), int(seed), int(pick), 0)
        _check(self.L.loikb_solve_pose_multistart(self.h, qp, tp, flags | qf, C.byref(prm), C.byref(msp)))
        self._ms_goals = G
        out = {name: self.multistart_get(name) for name in ("winner", "goal_status", "q", "err", "cost", "nreached", "round", "timing")}
        out["rounds_run"] = out["timing"]["rounds"]
        if self.multistart_clearance() is not None:
            for name in ("clearance", "witness", "nclear"):
                out[name] = self.multistart_clearance_get(name)
        self._avoid_results(out)
        return out

    def multistart_get(self, name):
        """one result of the last SolvePoseMultiStart (loikb_multistart_get): winner / goal_status / q / err / cost / nreached /
        round / timing (a dict: rounds, total_ms, solve_ms, sample_ms, select_ms, other_ms)"""
        fields = {"winner": (MS_F_WINNER, np.int32), "goal_status": (MS_F_GOAL_STATUS, np.int32), "q": (MS_F_Q, np.float64),
                  "err": (MS_F_ERR, np.float64), "cost": (MS_F_COST, np.float64), "nreached": (MS_F_NREACHED, np.int32),
                  "round": (MS_F_ROUND, np.int32), "timing": (MS_F_TIMING, np.float64)}
        fid, dtype = fields[name]
        if name == "timing":
            t = np.zeros(6)
            _check(self.L.loikb_multistart_get(self.h, fid, t.ctypes.data_as(C.c_void_p), 0))
            return dict(rounds=int(t[0]), total_ms=float(t[1]), solve_ms=float(t[2]), sample_ms=float(t[3]), select_ms=float(t[4]),
                        other_ms=float(t[5]))
        if name == "round":
            arr = np.empty(self.batch, dtype=dtype)
            _check(self.L.loikb_multistart_get(self.h, fid, arr.ctypes.data_as(C.c_void_p), 0))
            return arr
        # (the goal count is the library's: the winners come first, their number sizes the rest)
        nc = int(self.L.loikb_num_eq_c(self.h))
        big = np.empty(self.batch * {"q": self.model.nq, "err": nc * 6}.get(name, 1), dtype=dtype)
        _check(self.L.loikb_multistart_get(self.h, fid, big.ctypes.data_as(C.c_void_p), 0))
        G = self._ms_goals
        shape = {"q": (G, self.model.nq), "err": (G, nc, 6)}.get(name, (G,))
        return big[:int(np.prod(shape))].reshape(shape).copy()

    # ---- waypoint paths (include/loik_amd_path.h) ------------------------------------------------------------
    def SolvePosePath(self, waypoints, dt=1.0, gain=1.0, tol_pose=1e-6, max_steps=100, max_steps_per_waypoint=0, record=True, q=None):
        """SolvePose along a path of T waypoints per instance, each instance at its own pace (loikb_solve_pose_path): an instance that
        reaches its waypoint heads for the next in the same step, whatever the rest of the batch does.  max_steps bounds the steps
        of the WHOLE path, max_steps_per_waypoint (0: no bound) those spent on one waypoint: an instance that exhausts it is
        STALLED and stays where it is.
        waypoints: [B][T][nc][4][4] / [B][T][nc][12], or [T][nc][4][4] / [T][nc][12] shared by the batch.  A device tensor of these
        shapes likewise; a flat one goes by its numel: [B][T][nc][12] when that is a multiple of batch * nc * 12, else [T][nc][12].
        q as in SolvePose.
        Returns dict(reached [B] bool (the whole path), cursor [B] waypoints reached, steps [B] in total, wsteps [B][T] steps per
        waypoint, status [B] POSE_ST_* bits, path_status [B] PATH_ST_* bits, err [B][nc][6] against waypoint min(cursor, T - 1),
        q_path [B][T][nq] = q at each reached waypoint, NaN rows from the cursor on (None with record=False)), and with joint
        position limits on the handle limit_flags [B][nv]."""
        B, nc = self.batch, int(self.L.loikb_num_eq_c(self.h))
        flags, keep = 0, []
        if hasattr(waypoints, "data_ptr") and getattr(waypoints, "is_cuda", False):
            n, shape = int(waypoints.numel()), tuple(getattr(waypoints, "shape", ()))
            if len(shape) == 4 and shape[0] == B and shape[2] == nc:
                T, shared = shape[1], False
            elif len(shape) == 3 and shape[1] == nc:
                T, shared = shape[0], True
            elif n and n % (B * nc * 12) == 0:
                T, shared = n // (B * nc * 12), False
            elif n and n % (nc * 12) == 0:
                T, shared = n // (nc * 12), True
            else:
                raise ValueError("waypoints: device tensor has %d elements, expected batch * T * nc * 12 or T * nc * 12" % n)
            if n != (1 if shared else B) * T * nc * 12:
                raise ValueError("waypoints: device tensor of shape %s is neither [B][T][nc][12] nor [T][nc][12]" % (shape,))
            wp = C.c_void_p(waypoints.data_ptr())
            flags |= IN_DEVICE
        else:
            t = self._placements12(waypoints.numpy() if hasattr(waypoints, "numpy") else waypoints, "waypoints")
            if t.ndim == 4 and t.shape[0] == B and t.shape[2] == nc:
                T, shared = t.shape[1], False
            elif t.ndim == 3 and t.shape[1] == nc:
                T, shared = t.shape[0], True
            else:
                raise ValueError("waypoints: shape %s, expected [batch = %d][T][nc = %d][12] or [T][nc][12]" % (t.shape, B, nc))
            keep.append(t)
            wp = t.ctypes.data_as(C.c_void_p)
        if shared and B > 1:
            flags |= POSE_TARGET_SHARED
        qp = None
        if q is not None:
            if isinstance(q, int) or (hasattr(q, "data_ptr") and getattr(q, "is_cuda", False)):
                if not flags & IN_DEVICE:
                    raise ValueError("q and waypoints must both be host arrays or both device pointers")
                qp = C.c_void_p(q if isinstance(q, int) else q.data_ptr())
            else:
                if flags & IN_DEVICE:
                    raise ValueError("q and waypoints must both be host arrays or both device pointers")
                qa = _f64(q)
                if qa.size != B * self.model.nq:
                    raise ValueError("q has %d elements, expected batch * nq = %d" % (qa.size, B * self.model.nq))
                keep.append(qa)
                qp = qa.ctypes.data_as(C.c_void_p)
        prm = PoseParams(float(dt), float(gain), float(tol_pose), int(max_steps), 0)
        pth = PathParams(int(T), int(max_steps_per_waypoint), int(record), 0)
        _check(self.L.loikb_solve_pose_path(self.h, qp, wp, flags, C.byref(prm), C.byref(pth)))
        self._path_T = int(T)
        status = np.empty(B, dtype=np.int32)
        steps = np.empty(B, dtype=np.int32)
        err = np.empty((B, nc, 6))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STATUS, status.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STEPS, steps.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_ERR, err.ctypes.data_as(C.c_void_p), 0))
        out = dict(reached=(status & POSE_ST_REACHED) != 0, cursor=self.path_get("cursor"), steps=steps, wsteps=self.path_get("wsteps"),
                   status=status, path_status=self.path_get("path_status"), err=err, q_path=self.path_get("q_path") if int(record) == 1 else None)
        if self._limits or self._accel:
            out["limit_flags"] = self.pose_limit_flags()
        self._avoid_results(out)
        return out

    def path_get(self, name):
        """one result of the last SolvePosePath (loikb_path_get): cursor / path_status / wsteps / q_path / timing (a dict as pose_timing)"""
        B, T = self.batch, getattr(self, "_path_T", 1)
        if name == "timing":
            t = np.zeros(4)
            _check(self.L.loikb_path_get(self.h, PATH_F_TIMING, t.ctypes.data_as(C.c_void_p), 0))
            return dict(steps=int(t[0]), total_ms=float(t[1]), solve_ms=float(t[2]), other_ms=float(t[3]))
        fid, dtype, shape = {"cursor": (PATH_F_CURSOR, np.int32, (B,)), "path_status": (PATH_F_STATUS, np.int32, (B,)),
                             "wsteps": (PATH_F_WSTEPS, np.int32, (B, T)), "q_path": (PATH_F_Q, np.float64, (B, T, self.model.nq))}[name]
        arr = np.empty(shape, dtype=dtype)
        _check(self.L.loikb_path_get(self.h, fid, arr.ctypes.data_as(C.c_void_p), 0))
        return arr

    # ---- timed trajectories (include/loik_amd_track.h) -------------------------------------------------------
    def TrackPose(self, samples, dt=1.0, gain=1.0, tol_track=1e-4, feedforward="difference", record=("q", "z"), q=None):
        """closed-loop tracking of a pose trajectory sampled every dt (loikb_track_pose): T + 1 samples X_0 .. X_T per instance, one
        inner solve per step, every instance in step with the clock.  Step k: e against X_k, b_c = A_c ((gain / dt) e_c + f_c) with
        f_c the feed-forward twist from X_k to X_{k+1} over dt (feedforward="difference"; "none": f = 0), the step of SolvePose.
        samples: [B][T+1][nc][4][4] / [B][T+1][nc][12], or [T+1][nc][4][4] / [T+1][nc][12] shared by the batch; a device tensor of
        these shapes likewise, a flat one by its numel as SolvePosePath takes it.  record: any of "q", "z" (or the REC bits).
        q as in SolvePose.
        Returns SolvePose's dict (reached is never set: status carries the inner solves' bits and STOPPED; err is against X_T) plus
        q_traj [B][T+1][nq] and z_traj [B][T][nv] (None when not recorded; NaN rows after a stop), errmax [B][T+1], inner [B][T]
        TRACK_IN_* bits, ontrack [B] samples within tol_track, worst [B] / worst_at [B] = the largest errmax after sample 0."""
        B, nc = self.batch, int(self.L.loikb_num_eq_c(self.h))
        flags, keep = 0, []
        if hasattr(samples, "data_ptr") and getattr(samples, "is_cuda", False):
            n, shape = int(samples.numel()), tuple(getattr(samples, "shape", ()))
            if len(shape) == 4 and shape[0] == B and shape[2] == nc:
                Tn, shared = shape[1], False
            elif len(shape) == 3 and shape[1] == nc:
                Tn, shared = shape[0], True
            elif n and n % (B * nc * 12) == 0:
                Tn, shared = n // (B * nc * 12), False
            elif n and n % (nc * 12) == 0:
                Tn, shared = n // (nc * 12), True
            else:
                raise ValueError("samples: device tensor has %d elements, expected batch * (T + 1) * nc * 12 or (T + 1) * nc * 12" % n)
            if n != (1 if shared else B) * Tn * nc * 12:
                raise ValueError("samples: device tensor of shape %s is neither [B][T+1][nc][12] nor [T+1][nc][12]" % (shape,))
            sp = C.c_void_p(samples.data_ptr())
            flags |= IN_DEVICE
        else:
            t = self._placements12(samples.numpy() if hasattr(samples, "numpy") else samples, "samples")
            if t.ndim == 4 and t.shape[0] == B and t.shape[2] == nc:
                Tn, shared = t.shape[1], False
            elif t.ndim == 3 and t.shape[1] == nc:
                Tn, shared = t.shape[0], True
            else:
                raise ValueError("samples: shape %s, expected [batch = %d][T+1][nc = %d][12] or [T+1][nc][12]" % (t.shape, B, nc))
            keep.append(t)
            sp = t.ctypes.data_as(C.c_void_p)
        if shared and B > 1:
            flags |= POSE_TARGET_SHARED
        qp = None
        if q is not None:
            if isinstance(q, int) or (hasattr(q, "data_ptr") and getattr(q, "is_cuda", False)):
                if not flags & IN_DEVICE:
                    raise ValueError("q and samples must both be host arrays or both device pointers")
                qp = C.c_void_p(q if isinstance(q, int) else q.data_ptr())
            else:
                if flags & IN_DEVICE:
                    raise ValueError("q and samples must both be host arrays or both device pointers")
                qa = _f64(q)
                if qa.size != B * self.model.nq:
                    raise ValueError("q has %d elements, expected batch * nq = %d" % (qa.size, B * self.model.nq))
                keep.append(qa)
                qp = qa.ctypes.data_as(C.c_void_p)
        if isinstance(feedforward, str):
            if feedforward not in TRACK_FFS:
                raise ValueError("feedforward %r: expected one of %s" % (feedforward, sorted(TRACK_FFS)))
            feedforward = TRACK_FFS[feedforward]
        if not isinstance(record, (int, np.integer)):
            bits = 0
            for r in ([record] if isinstance(record, str) else record):
                if r not in TRACK_RECS:
                    raise ValueError("record %r: expected any of %s" % (r, sorted(TRACK_RECS)))
                bits |= TRACK_RECS[r]
            record = bits
        prm = TrackParams(float(dt), float(gain), float(tol_track), int(Tn) - 1, int(feedforward), int(record), 0)
        _check(self.L.loikb_track_pose(self.h, qp, sp, flags, C.byref(prm)))
        self._track_T = int(Tn) - 1
        status = np.empty(B, dtype=np.int32)
        steps = np.empty(B, dtype=np.int32)
        err = np.empty((B, nc, 6))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STATUS, status.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_STEPS, steps.ctypes.data_as(C.c_void_p), 0))
        _check(self.L.loikb_pose_get(self.h, POSE_F_ERR, err.ctypes.data_as(C.c_void_p), 0))
        out = dict(reached=(status & POSE_ST_REACHED) != 0, steps=steps, err=err, status=status)
        recorded = {"q_traj": record & TRACK_REC_Q, "z_traj": record & TRACK_REC_Z}
        for name in TRACK_FIELD_ID:
            out[name] = self.track_get(name) if recorded.get(name, True) else None
        if self._limits or self._accel:
            out["limit_flags"] = self.pose_limit_flags()
        self._avoid_results(out)
        return out

    def track_get(self, name, out=None):
        """one result of the last TrackPose (loikb_track_get): q_traj / z_traj / errmax / inner / ontrack / worst / worst_at as a numpy
        array (or into a device pointer / torch tensor `out`), or timing (a dict as pose_timing)"""
        if name == "timing":
            t = np.zeros(4)
            _check(self.L.loikb_track_get(self.h, TRACK_F_TIMING, t.ctypes.data_as(C.c_void_p), 0))
            return dict(steps=int(t[0]), total_ms=float(t[1]), solve_ms=float(t[2]), other_ms=float(t[3]))
        fid = TRACK_FIELD_ID[name]
        if out is not None:
            p, dev = _ptr(out)
            _check(self.L.loikb_track_get(self.h, fid, p, OUT_DEVICE if dev else 0))
            return out
        T = getattr(self, "_track_T", 1)
        d = {"T": T, "T+1": T + 1, "nq": self.model.nq, "nv": self.model.nv}
        arr = np.empty((self.batch,) + tuple(d[x] for x in TRACK_FIELD_DIMS[name]), dtype=np.int32 if name in TRACK_INT_FIELDS else np.float64)
        _check(self.L.loikb_track_get(self.h, fid, arr.ctypes.data_as(C.c_void_p), 0))
        return arr

    # ------------------------------------------------------------------------------------------------------
    def set_max_iter(self, n):
        _check(self.L.loikb_set_max_iter(self.h, int(n)))
        self.opts.max_iter = int(n)
    def set_rho(self, x): _check(self.L.loikb_set_rho(self.h, float(x)))
    def set_mu(self, x): _check(self.L.loikb_set_mu(self.h, float(x)))
    def set_tol(self, tol_abs, tol_rel): _check(self.L.loikb_set_tol(self.h, float(tol_abs), float(tol_rel)))
    def set_tol_primal_inf(self, x): _check(self.L.loikb_set_tol_primal_inf(self.h, float(x)))
    def set_tol_tail_solve(self, x): _check(self.L.loikb_set_tol_tail_solve(self.h, float(x)))
    def set_warm_start(self, w): _check(self.L.loikb_set_warm_start(self.h, int(bool(w))))

    def _shapes(self, names):
        m, nc = self.model, self.L.loikb_num_eq_c(self.h)
        d = {"nb": m.njoints - 1, "nv": m.nv, "nq": m.nq, "nc": nc, "6nb+nv": 6 * (m.njoints - 1) + m.nv}
        return {n: (self.batch,) + tuple(d.get(x, x) for x in FIELD_DIMS[n]) for n in names}

    def get(self, name, out=None):
        """one field for the whole batch as a numpy array (or into a device pointer / torch tensor `out`)"""
        fid = FIELD_ID[name]
        if out is not None:
            p, dev = _ptr(out)
            _check(self.L.loikb_get(self.h, fid, p, OUT_DEVICE if dev else 0))
            return out
        arr = np.empty(self._shapes([name])[name], dtype=np.int32 if name in INT_FIELDS else np.float64)
        _check(self.L.loikb_get(self.h, fid, arr.ctypes.data_as(C.c_void_p), 0))
        return arr

    RESULT_FIELDS = ("z", "nu", "w", "vis", "fis", "yis", "scalars")   # (bit k of loikb_get_results' mask: LOIKB_RES_*)
    NSCALARS, SCALAR_ITER, SCALAR_STATUS, SCALAR_MU_UPDATES = 33, 30, 31, 32   # (LOIKB_RES_NSCALARS ...: the layout of "scalars")

    def get_results(self, fields=RESULT_FIELDS[:6]):
        """the members of the reference's data object a solve leaves behind (z, nu, w, vis, fis, yis: loik-loid-data-optimized.hpp:118-178), any
        subset, in ONE call (loikb_get_results): {name: array}, the same values as get(name).  "scalars": [B][33] -- the 30 scalar getters'
        fields in FIELD_ID order from "primal_residual", then iter, the status bits, mu_updates (what get_iter() / get_convergence_status() / ...
        read), from the same gather"""
        mask, out, ptrs, shapes = 0, {}, [], self._shapes(self.RESULT_FIELDS)
        for k, name in enumerate(self.RESULT_FIELDS):
            if name in fields:
                mask |= 1 << k
                out[name] = np.empty(shapes[name], dtype=np.float64)
                ptrs.append(out[name].ctypes.data_as(_dp))
            else:
                ptrs.append(None)
        unknown = [f for f in fields if f not in self.RESULT_FIELDS]
        if unknown:
            raise ValueError("get_results: not a result member: %s" % unknown)
        _check(self.L.loikb_get_results(self.h, mask, *ptrs))
        return out

    def His_full(self):
        """ik_id_data.His[i] as full symmetric 6x6 blocks: [B][nb][6][6]"""
        packed = self.get("His")
        B, nb = packed.shape[:2]
        full = np.zeros((B, nb, 6, 6))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                full[:, :, i, j] = packed[:, :, k]
                full[:, :, j, i] = packed[:, :, k]
                k += 1
        return full

    SOLVER_INFO_LISTS = ["primal_residual_task_list", "primal_residual_slack_list", "primal_residual_list", "dual_residual_nu_list",
                         "dual_residual_v_list", "dual_residual_list", "mu_list", "mu_eq_list", "mu_ineq_list"]

    def solver_info(self):
        """LoikSolverInfo of the last solve (constructor keyword logging=True): {list name: [B][max_iter - 1]}, 'rows': [B]
        (max_iter as it was when that solve ran: the library says how many rows it holds)"""
        cap = max(int(self.L.loikb_solver_info_rows_cap(self.h)), 1)
        out = {}
        rows = np.zeros(self.batch, dtype=np.int32)
        for k, name in enumerate(self.SOLVER_INFO_LISTS):
            a = np.zeros((self.batch, cap))
            _check(self.L.loikb_get_solver_info(self.h, k, a.ctypes.data_as(_dp), cap, rows.ctypes.data_as(_ip)))
            out[name] = a
        out["rows"] = rows
        out["truncated_instances"] = int(self.L.loikb_solver_info_truncated(self.h))   # 0 but for a warm start whose mu left the decades
        return out

    def stats(self):
        st = Stats()
        _check(self.L.loikb_get_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    # reference getter names (task-solver-base.hpp:87-102), one value per instance
    def get_iter(self): return self.get("iter")
    def get_convergence_status(self): return self.get("converged").astype(bool)
    def get_primal_infeasibility_status(self): return self.get("primal_infeasible").astype(bool)
    def get_primal_residual(self): return self.get("primal_residual")
    def get_dual_residual(self): return self.get("dual_residual")
    def get_mu(self): return self.get("mu")
