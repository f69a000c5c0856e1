"""ctypes binding of libpioneer_amd.so (the C ABI of include/pioneer_amd.h).

There is no fallback: if the HIP library is missing or a call fails, this
module raises.  ``build_library()`` compiles it in-tree with hipcc for gfx950.
"""
import ctypes as C
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# PNR_LIB_PATH: load another build of the library (A/B experiments such as tools/build_variant.py's); default in-tree
LIB_PATH = os.environ.get("PNR_LIB_PATH") or os.path.join(CSRC, "libpioneer_amd.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pioneer_amd.h")



def _header_abi_version() -> int:
    """PNR_ABI_VERSION as include/pioneer_amd.h states it (the header is the single source)."""
    import re
    with open(HEADER) as f:
        m = re.search(r"^#define\s+PNR_ABI_VERSION\s+(\d+)", f.read(), re.M)
    if not m:
        raise ImportError(f"{HEADER}: no PNR_ABI_VERSION")
    return int(m.group(1))


ABI_VERSION = _header_abi_version()

DOF = 6
OBS_DIM = 137
STATE_WORDS = 24
INFO_DIM = 4
DYN_STATE_WORDS = 36
NUM_LINKS = 11          # pnr_get_link_states: link records per env (Bullet's link_index order, model.LINKS[1:])
LINK_STATE_DIM = 13     # position[3], quaternion x y z w [4], linear velocity[3], angular velocity[3]
CONTACT_SAMPLES = 23    # pnr_get_contacts: sample spheres per env (model.CONTACT_SAMPLE_LINKS names their links); 22 is the pointer
CONTACT_DIM = 9         # distance, normal[3], position on the sample[3], body index, normal force
RAY_DIM = 8             # pnr_ray_test: hit fraction, world position[3], unit world normal[3], pnr_seg label as a float
MAX_RAYS = 1024         # .. rays per env, at most
RAY_HIT_BODIES, RAY_HIT_ARM, RAY_HIT_TARGET = 1, 2, 4      # pnr_ray_params.hit_mask bits (enum pnr_ray_hit)
JACOBIAN_DIM = 36       # pnr_get_jacobian: 6 rows (linear xyz, angular xyz) x 6 joint columns per env
INVDYN_NO_GRAVITY, INVDYN_JOINT_LOSSES = 1, 2      # pnr_inverse_dynamics flags (PNR_INVDYN_*)
MAX_LINK_WRENCHES = 4   # pnr_world_step_wrenches: wrench records per env, at most (PNR_MAX_LINK_WRENCHES)
WRENCH_DIM = 9          # .. force[3], position[3], torque[3] per record
JOINT_STATE_DIM = 4     # pnr_get_joint_states: q, qd, qdd, tau_motor per joint
REACTION_DIM = 6        # .. Fx, Fy, Fz, Mx, My, Mz per joint
BODY_STATE_WORDS = 8    # pnr_set_body_state: the moving sphere's position[3], velocity[3], mass, radius (PNR_BODY_STATE_WORDS)
BODY_GRIP_WORDS = 4     # pnr_get_body_grip: the grip's max_force, then the last sub-step's force on the sphere[3] (PNR_BODY_GRIP_WORDS)
FRAME_LINK, FRAME_WORLD = 1, 2                     # .. a record's frame (PNR_FRAME_*; pybullet's LINK_FRAME / WORLD_FRAME)

PNR_OK = 0
ENV_MAJOR, FEATURE_MAJOR = 0, 1
MODE_KINEMATIC, MODE_DYNAMIC = 0, 1
CONTROL_POSITION, CONTROL_VELOCITY = 0, 1                                   # the engine's PD torque law
CONTROL_POSITION_CONSTRAINT, CONTROL_VELOCITY_CONSTRAINT = 2, 3             # Bullet's constraint motor (set_joint_motor only)


class PnrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pioneer_amd error {code}: {msg}")
        self.code = code


MAX_SCENE = 8
SHAPE_PLANE, SHAPE_BOX, SHAPE_SPHERE = 1, 2, 3


class PnrLinkWrenchSpec(C.Structure):
    """pnr_link_wrench_spec of include/pioneer_amd.h (the call-uniform part of one wrench record of pnr_world_step_wrenches)."""
    _fields_ = [("link", C.c_int32), ("frame", C.c_int32)]


class PnrBodyParams(C.Structure):
    """pnr_body_params of include/pioneer_amd.h (the moving sphere's contact gains, friction and damping)."""
    _fields_ = [("struct_size", C.c_uint32), ("contact_kp", C.c_float), ("contact_kd", C.c_float), ("friction", C.c_float),
                ("slip_eps", C.c_float), ("linear_damping", C.c_float)]


class PnrBodyGripParams(C.Structure):
    """pnr_body_grip_params of include/pioneer_amd.h (the grip's anchor point on the pointer link and its spring)."""
    _fields_ = [("struct_size", C.c_uint32), ("anchor", C.c_float * 3), ("direction", C.c_float * 3), ("grip_kp", C.c_float),
                ("grip_kd", C.c_float)]


class PnrSceneBody(C.Structure):
    _fields_ = [("shape", C.c_int32), ("reserved", C.c_int32), ("position", C.c_double * 3), ("orientation", C.c_double * 4),
                ("size", C.c_double * 3)]


# pnr_render's segmentation labels (enum pnr_seg): background, 1 + URDF link index, the target, 13 + static body index, the moving sphere
SEG_BACKGROUND, SEG_LINK0, SEG_TARGET, SEG_BODY0 = 0, 1, 12, 13
SEG_MOVING_BODY = SEG_BODY0 + MAX_SCENE      # 21; pnr_get_contacts reports the sphere as body MAX_SCENE
# pnr_set_body_queries' bits (enum pnr_body_query): which scene queries see the moving sphere
BODY_IN_RENDER, BODY_IN_RAYS, BODY_IN_CONTACTS = 1, 2, 4


class PnrRenderParams(C.Structure):
    """pnr_render_params of include/pioneer_amd.h (pnr_render's camera, shading and static bodies)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("n_bodies", C.c_int32),
        ("view", C.c_double * 16), ("fov_y", C.c_double), ("near_clip", C.c_double), ("far_clip", C.c_double),
        ("light_direction", C.c_double * 3), ("ambient", C.c_double), ("diffuse", C.c_double),
        ("background", C.c_float * 3), ("target_rgba", C.c_float * 4), ("reserved", C.c_int32),
        ("bodies", PnrSceneBody * MAX_SCENE), ("body_rgba", (C.c_float * 4) * MAX_SCENE),
    ]


class PnrContactParams(C.Structure):
    """pnr_contact_params of include/pioneer_amd.h (pnr_get_contacts's bodies and penalty gains)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_bodies", C.c_int32), ("contact_kp", C.c_double), ("contact_kd", C.c_double),
                ("bodies", PnrSceneBody * MAX_SCENE)]


PATH_SUMMARY_DIM = 8            # pnr_path_clearance: min clearance, its t, sample, body, first violating t, violations, free, 0
MAX_PATH_WAYPOINTS, MAX_PATH_SUBSTEPS = 256, 64
PATH_LANES = (0, 1, 2, 4, 8, 16, 32, 64)                     # pnr_path_params.lanes_per_env (0: auto)


class PnrPathParams(C.Structure):
    """pnr_path_params of include/pioneer_amd.h (pnr_path_clearance's path layout, sample mask, margin and bodies)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_waypoints", C.c_int32), ("substeps", C.c_int32), ("from_current", C.c_int32),
                ("waypoints_per_env", C.c_int32), ("lanes_per_env", C.c_int32), ("sample_mask", C.c_uint32), ("n_bodies", C.c_int32),
                ("margin", C.c_double), ("bodies", PnrSceneBody * MAX_SCENE)]


class PnrRayParams(C.Structure):
    """pnr_ray_params of include/pioneer_amd.h (pnr_ray_test's ray layout, parent link, hit mask and bodies)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_rays", C.c_int32), ("rays_per_env", C.c_int32), ("parent_link", C.c_int32),
                ("hit_mask", C.c_int32), ("n_bodies", C.c_int32), ("bodies", PnrSceneBody * MAX_SCENE)]


class PnrIkParams(C.Structure):
    """pnr_ik_params of include/pioneer_amd.h (pnr_solve_ik's point, iteration cap, damping, step cap and tolerance)."""
    _fields_ = [("struct_size", C.c_uint32), ("link", C.c_int32), ("local_point", C.c_double * 3), ("max_iterations", C.c_int32),
                ("reserved", C.c_int32), ("damping", C.c_double), ("max_step", C.c_double), ("tolerance", C.c_double)]


IK_ORIENT_FULL, IK_ORIENT_AXIS = 0, 1      # pnr_ik_pose_params.mode


class PnrIkPoseParams(C.Structure):
    """pnr_ik_pose_params of include/pioneer_amd.h (pnr_solve_ik_pose's point, orientation mode, damping, weight, tolerances)."""
    _fields_ = [("struct_size", C.c_uint32), ("link", C.c_int32), ("local_point", C.c_double * 3), ("max_iterations", C.c_int32),
                ("mode", C.c_int32), ("local_axis", C.c_double * 3), ("damping", C.c_double), ("error_damping", C.c_double),
                ("orientation_weight", C.c_double), ("max_step", C.c_double), ("tolerance", C.c_double),
                ("angle_tolerance", C.c_double)]


IK_TASK_POSITION, IK_TASK_POSE, IK_TASK_AXIS = 0, 1, 2      # pnr_ik_multi_params.task
IK_MULTI_BEST, IK_MULTI_FIRST = 0, 1                         # pnr_ik_multi_params.policy
IK_MULTI_STARTS = (1, 2, 4, 8, 16, 32, 64)                   # pnr_ik_multi_params.num_starts


class PnrIkMultiParams(C.Structure):
    """pnr_ik_multi_params of include/pioneer_amd.h (pnr_solve_ik_multi's task, policy, starts and the per-start law's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("task", C.c_int32), ("policy", C.c_int32), ("num_starts", C.c_int32),
                ("starts_per_env", C.c_int32), ("link", C.c_int32), ("local_point", C.c_double * 3), ("max_iterations", C.c_int32),
                ("reserved", C.c_int32), ("local_axis", C.c_double * 3), ("damping", C.c_double), ("error_damping", C.c_double),
                ("orientation_weight", C.c_double), ("max_step", C.c_double), ("tolerance", C.c_double),
                ("angle_tolerance", C.c_double)]


class PnrIkMultiBuffers(C.Structure):
    """pnr_ik_multi_buffers of include/pioneer_amd.h (pnr_solve_ik_multi's device pointers: inputs, the winner's and the per-start outputs)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(name, C.c_void_p) for name in (
        "target_pos", "target_quat", "starts", "q_init", "q_ref", "q_out", "residual_out", "angle_out", "iterations_out", "start_out",
        "converged_out", "all_q", "all_residual", "all_angle", "all_iterations")]


IK_PATH_SUMMARY_DIM = 8         # pnr_solve_ik_path: tracked, c_fail, max residual, max angle, travel, max jump, start, tracked starts
IK_PATH_ROWS_AUTO, IK_PATH_ROWS_SECOND_PASS, IK_PATH_ROWS_SECOND_LAUNCH = 0, 1, 2      # pnr_ik_path_params.winner_rows


class PnrIkPathParams(C.Structure):
    """pnr_ik_path_params of include/pioneer_amd.h (pnr_solve_ik_path's task, starts, path layout, the two caps and the law's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("task", C.c_int32), ("num_starts", C.c_int32), ("starts_per_env", C.c_int32),
                ("n_waypoints", C.c_int32), ("waypoints_per_env", C.c_int32), ("substeps", C.c_int32), ("link", C.c_int32),
                ("max_iterations", C.c_int32), ("track_iterations", C.c_int32), ("winner_rows", C.c_int32), ("reserved", C.c_int32),
                ("local_point", C.c_double * 3), ("local_axis", C.c_double * 3), ("damping", C.c_double), ("error_damping", C.c_double),
                ("orientation_weight", C.c_double), ("max_step", C.c_double), ("tolerance", C.c_double),
                ("angle_tolerance", C.c_double)]


class PnrIkPathBuffers(C.Structure):
    """pnr_ik_path_buffers of include/pioneer_amd.h (pnr_solve_ik_path's device pointers: waypoints, starts, the summary, the winner's rows)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(name, C.c_void_p) for name in (
        "waypoint_pos", "waypoint_quat", "starts", "q_init", "q_ref", "summary", "q_path", "residual_path", "angle_path",
        "iterations_path", "all_summary")]


MAX_TRAJ_POINTS, MAX_TRAJ_SAMPLES = 256, 65536      # pnr_retime_path: points of a path; pnr_sample_trajectory: samples of a call
RETIME_SUMMARY_DIM = 8          # pnr_retime_path: feasible, duration, k_fail, reason, largest sdot, largest row utilisation, 0, 0
RETIME_ROW_DIM = 18             # .. the torque rows of one (env, grid point) in the workspace: A[6] | B[6] | c[6]
RETIME_TORQUE = 1               # pnr_retime_params.flags (PNR_RETIME_TORQUE)
RETIME_FEASIBLE, RETIME_EMPTY, RETIME_STUCK, RETIME_NONFINITE = 0, 1, 2, 3      # summary[3] (enum pnr_retime_reason)


class PnrRetimeParams(C.Structure):
    """pnr_retime_params of include/pioneer_amd.h (pnr_retime_path's path layout, flags and the joints' limits)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_points", C.c_int32), ("path_per_env", C.c_int32), ("flags", C.c_int32),
                ("v_max", C.c_double * 6), ("a_max", C.c_double * 6), ("tau_max", C.c_double * 6)]


class PnrRetimeBuffers(C.Structure):
    """pnr_retime_buffers of include/pioneer_amd.h (pnr_retime_path's device pointers)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(name, C.c_void_p) for name in (
        "q_path", "workspace", "summary", "times", "sdot2")]


class PnrTrajSampleParams(C.Structure):
    """pnr_traj_sample_params of include/pioneer_amd.h (pnr_sample_trajectory's path layout and sampling window)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_points", C.c_int32), ("path_per_env", C.c_int32), ("n_samples", C.c_int32),
                ("t0", C.c_double), ("dt", C.c_double)]


class PnrConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
        ("max_v_to_r", C.c_double), ("max_a_to_v", C.c_double), ("done_distance", C.c_double),
        ("award_max", C.c_double), ("award_done", C.c_double),
        ("award_potential_slope", C.c_double), ("penalty_step", C.c_double),
        ("target_lo", C.c_double * 3), ("target_hi", C.c_double * 3), ("target_radius", C.c_double),
        ("timestep", C.c_double), ("frame_skip", C.c_int32), ("gravity", C.c_double),
        ("max_episode_steps", C.c_int32),
        ("auto_reset", C.c_int32), ("obs_layout", C.c_int32), ("action_layout", C.c_int32),
        ("mode", C.c_int32),
        ("pd_kp", C.c_double), ("pd_kd", C.c_double), ("torque_limit", C.c_double),
        ("joint_damping", C.c_double), ("joint_friction", C.c_double),
        ("teleport", C.c_int32), ("randomize", C.c_int32),
        ("rand_mass_lo", C.c_double), ("rand_mass_hi", C.c_double),
        ("rand_friction_lo", C.c_double), ("rand_friction_hi", C.c_double),
        ("rand_damping_lo", C.c_double), ("rand_damping_hi", C.c_double),
        ("ground_z", C.c_double), ("contact_kp", C.c_double), ("contact_kd", C.c_double),
        ("obstacle_position", C.c_double * 3), ("obstacle_half_extents", C.c_double * 3),
        ("pointer_radius", C.c_double),
        ("control_mode", C.c_int32), ("link_contacts", C.c_int32), ("max_velocity", C.c_double),
        ("n_scene", C.c_int32), ("pd_inertia_scaled", C.c_int32), ("scene", PnrSceneBody * MAX_SCENE),
    ]


class PnrConstants(C.Structure):
    _fields_ = [
        ("r_lo", C.c_float * DOF), ("r_hi", C.c_float * DOF),
        ("v_max", C.c_float * DOF), ("a_max", C.c_float * DOF),
        ("dt", C.c_double), ("eps", C.c_double),
    ]


class PnrRolloutStats(C.Structure):
    _fields_ = [("ep_ret", C.c_void_p), ("ep_len", C.c_void_p), ("scratch", C.c_void_p), ("scratch_doubles", C.c_int64),
                ("w_sum", C.c_void_p), ("w_len", C.c_void_p), ("w_cnt", C.c_void_p), ("w_max", C.c_void_p), ("w_min", C.c_void_p),
                ("adv_stats", C.c_void_p)]


class PnrMlpStep(C.Structure):
    """pnr_mlp_step of include/pioneer_amd.h (one PPO minibatch update, pnr_mlp_train_step)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("batch", C.c_int64),
        ("obs", C.c_void_p), ("idx", C.c_void_p),
        ("f_loc", C.c_void_p), ("f_inv", C.c_void_p), ("f_lo", C.c_void_p), ("f_hi", C.c_void_p),
        ("actions", C.c_void_p), ("logp_old", C.c_void_p), ("mean_old", C.c_void_p), ("log_std_old", C.c_void_p),
        ("adv", C.c_void_p), ("value_target", C.c_void_p), ("value_old", C.c_void_p),
        ("kl_coeff", C.c_void_p), ("entropy_coeff", C.c_void_p),
        ("clip_param", C.c_float), ("vf_clip_param", C.c_float), ("vf_loss_coeff", C.c_float),
        ("params", C.c_void_p * 12), ("n3_policy", C.c_int32), ("n3_value", C.c_int32),
        ("wpack", C.c_void_p), ("bias", C.c_void_p),
        ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("adam_step", C.c_void_p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("head", C.c_void_p), ("g_head", C.c_void_p), ("xs", C.c_void_p), ("h1", C.c_void_p), ("h2", C.c_void_p),
        ("dz1", C.c_void_p), ("dz2", C.c_void_p),
        ("partials", C.c_void_p), ("partial_rows", C.c_int64), ("slabs", C.c_void_p), ("slab_floats", C.c_int64),
        ("means", C.c_void_p), ("flat_grad", C.c_void_p), ("xs_in", C.c_void_p),
        ("first_net", C.c_int32), ("n_nets", C.c_int32),
        ("w3_partials", C.c_void_p), ("w3_partial_floats", C.c_int64),
        ("planes", C.c_int32), ("xs_in_plane", C.c_int64),
    ]


# name -> (restype, argtypes); the list tests check against include/pioneer_amd.h
_VP = C.c_void_p
SIGNATURES = {
    "pnr_abi_version": (C.c_int, []),
    "pnr_build_fingerprint": (C.c_char_p, []),
    "pnr_config_default": (C.c_int, [C.POINTER(PnrConfig)]),
    "pnr_get_constants": (C.c_int, [C.POINTER(PnrConfig), C.POINTER(PnrConstants)]),
    "pnr_create": (C.c_int, [C.POINTER(PnrConfig), C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.POINTER(_VP)]),
    "pnr_destroy": (C.c_int, [_VP]),
    "pnr_seed": (C.c_int, [_VP, C.c_uint64]),
    "pnr_reset": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "pnr_step": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pnr_rollout": (C.c_int, [_VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pnr_observe": (C.c_int, [_VP, _VP, _VP]),
    "pnr_world_step": (C.c_int, [_VP, _VP, _VP]),
    "pnr_world_step_torques": (C.c_int, [_VP, _VP, _VP]),
    "pnr_world_step_wrenches": (C.c_int, [_VP, C.POINTER(PnrLinkWrenchSpec), C.c_int, _VP, _VP, C.c_int, _VP]),
    "pnr_world_step_targets": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP]),
    "pnr_set_joint_motor": (C.c_int, [_VP, C.c_int32, C.c_int32] + [C.c_double] * 6),
    "pnr_get_state": (C.c_int, [_VP, _VP, _VP]),
    "pnr_set_state": (C.c_int, [_VP, _VP, _VP]),
    "pnr_get_dyn_state": (C.c_int, [_VP, _VP, _VP]),
    "pnr_set_dyn_state": (C.c_int, [_VP, _VP, _VP]),
    "pnr_body_params_default": (C.c_int, [C.POINTER(PnrBodyParams)]),
    "pnr_set_body_params": (C.c_int, [_VP, C.POINTER(PnrBodyParams)]),
    "pnr_set_body_state": (C.c_int, [_VP, _VP, _VP, _VP]),
    "pnr_get_body_state": (C.c_int, [_VP, _VP, _VP]),
    "pnr_body_grip_params_default": (C.c_int, [C.POINTER(PnrBodyGripParams)]),
    "pnr_set_body_grip_params": (C.c_int, [_VP, C.POINTER(PnrBodyGripParams)]),
    "pnr_set_body_grip": (C.c_int, [_VP, _VP, _VP, _VP]),
    "pnr_get_body_grip": (C.c_int, [_VP, _VP, _VP]),
    "pnr_set_body_queries": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_float * 4)]),
    "pnr_get_link_states": (C.c_int, [_VP, _VP, _VP, _VP]),
    "pnr_get_jacobian": (C.c_int, [_VP, _VP, C.c_int32, C.POINTER(C.c_double * 3), _VP, _VP]),
    "pnr_inverse_dynamics": (C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, _VP]),
    "pnr_mass_matrix": (C.c_int, [_VP, _VP, _VP, _VP]),
    "pnr_get_joint_states": (C.c_int, [_VP, _VP, _VP, C.POINTER(PnrLinkWrenchSpec), C.c_int32, _VP, _VP, _VP, _VP]),
    "pnr_ik_params_default": (C.c_int, [C.POINTER(PnrIkParams)]),
    "pnr_solve_ik": (C.c_int, [_VP, C.POINTER(PnrIkParams), _VP, _VP, _VP, _VP, _VP, _VP]),
    "pnr_ik_pose_params_default": (C.c_int, [C.POINTER(PnrIkPoseParams)]),
    "pnr_solve_ik_pose": (C.c_int, [_VP, C.POINTER(PnrIkPoseParams)] + [_VP] * 8),
    "pnr_ik_multi_params_default": (C.c_int, [C.POINTER(PnrIkMultiParams), C.c_int32]),
    "pnr_solve_ik_multi": (C.c_int, [_VP, C.POINTER(PnrIkMultiParams), C.POINTER(PnrIkMultiBuffers), _VP]),
    "pnr_ik_path_params_default": (C.c_int, [C.POINTER(PnrIkPathParams), C.c_int32]),
    "pnr_solve_ik_path": (C.c_int, [_VP, C.POINTER(PnrIkPathParams), C.POINTER(PnrIkPathBuffers), _VP]),
    "pnr_retime_params_default": (C.c_int, [C.POINTER(PnrRetimeParams)]),
    "pnr_retime_workspace_bytes": (C.c_int, [_VP, C.POINTER(PnrRetimeParams), C.POINTER(C.c_uint64)]),
    "pnr_retime_path": (C.c_int, [_VP, C.POINTER(PnrRetimeParams), C.POINTER(PnrRetimeBuffers), _VP]),
    "pnr_traj_sample_params_default": (C.c_int, [C.POINTER(PnrTrajSampleParams)]),
    "pnr_sample_trajectory": (C.c_int, [_VP, C.POINTER(PnrTrajSampleParams), _VP, _VP, _VP, _VP, _VP, _VP]),
    "pnr_render": (C.c_int, [_VP, _VP, C.POINTER(PnrRenderParams), _VP, _VP, _VP, _VP]),
    "pnr_render_bodies": (C.c_int, [_VP, _VP, C.POINTER(PnrRenderParams), _VP, _VP, _VP, _VP, _VP]),
    "pnr_render_cameras": (C.c_int, [_VP, _VP, C.POINTER(PnrRenderParams), _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "pnr_contact_params_default": (C.c_int, [C.POINTER(PnrContactParams)]),
    "pnr_get_contacts": (C.c_int, [_VP, _VP, C.POINTER(PnrContactParams), _VP, _VP, _VP, _VP, _VP]),
    "pnr_path_params_default": (C.c_int, [C.POINTER(PnrPathParams)]),
    "pnr_path_clearance": (C.c_int, [_VP, C.POINTER(PnrPathParams), _VP, _VP, _VP, _VP, _VP]),
    "pnr_ray_params_default": (C.c_int, [C.POINTER(PnrRayParams)]),
    "pnr_ray_test": (C.c_int, [_VP, _VP, C.POINTER(PnrRayParams), _VP, _VP, _VP, _VP, _VP]),
    "pnr_diag_sincos": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int, _VP]),
    "pnr_ppo_loss": (C.c_int, [C.c_int64] + [_VP] * 12 + [C.c_float] * 3 + [_VP] * 3 + [C.c_int64, _VP, _VP]),
    "pnr_mlp_pack_elems": (C.c_int64, []),
    "pnr_mlp_bias_elems": (C.c_int64, []),
    "pnr_mlp_slab_floats": (C.c_int64, [C.c_int64]),
    "pnr_mlp_w3_partial_floats": (C.c_int64, [C.c_int64]),
    "pnr_mlp_pack": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP]),
    "pnr_mlp_forward": (C.c_int, [C.c_int64] + [_VP] * 12 + [C.c_int32, C.c_int32, C.c_int32, _VP]),
    "pnr_ppo_gae_scratch": (C.c_int64, [C.c_int64]),
    "pnr_ppo_gae": (C.c_int, [C.c_int32, C.c_int64] + [_VP] * 8 + [C.c_double, C.c_double] + [_VP] * 6),
    "pnr_filter_moments_scratch": (C.c_int64, [C.c_int64]),
    "pnr_filter_moments": (C.c_int, [C.c_int64, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "pnr_filter_merge": (C.c_int, [_VP] * 8),
    "pnr_filter_prepare": (C.c_int, [_VP, _VP, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "pnr_permutation": (C.c_int, [C.c_int64, C.c_uint64, C.c_uint64, _VP, _VP]),
    "pnr_mlp_act": (C.c_int, [C.c_int64] + [_VP] * 16 + [C.c_int32, _VP]),
    "pnr_ppo_rollout": (C.c_int, [_VP, C.c_int32] + [_VP] * 18),
    "pnr_mlp_backward": (C.c_int, [C.c_int64] + [_VP] * 8 + [C.c_int64, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "pnr_mlp_grad_floats": (C.c_int64, []),
    "pnr_ppo_pack_record": (C.c_int, [C.c_int64] + [_VP] * 11),
    "pnr_mlp_gather": (C.c_int, [C.c_int64] + [_VP] * 23 + [C.c_int32, _VP]),
    "pnr_mlp_train_step": (C.c_int, [C.POINTER(PnrMlpStep), _VP]),
    "pnr_mlp_adam": (C.c_int, [C.POINTER(PnrMlpStep), _VP, C.c_float, _VP]),
    "pnr_num_envs": (C.c_int64, [_VP]),
    "pnr_last_error": (C.c_char_p, [_VP]),
}


# the library's translation units and what each includes: a unit is recompiled when one of its files is newer than its object
_ENV_HOST = ["pnr_env_host.h", "pnr_host.h", "pnr_device.h", "pnr_model.h", "pnr_dyn.h"]      # what every env-engine unit includes
UNITS = {
    # the env engine's core: its C ABI but for the queries, and every kernel of pnr_env_kernels.h (126, 96 of them dynamics mode's)
    "pnr_api.hip": ["pnr_api.hip", *_ENV_HOST, "pnr_env_kernels.h"],
    # the query entry points of the C ABI and their kernels (61: the three scene queries have a per-env-world form each, pnr_query.h; the renderer a per-env-camera form too; six of pnr_path.h, four of pnr_retime.h)
    "pnr_queries.hip": ["pnr_queries.hip", *_ENV_HOST, "pnr_query.h", "pnr_links.h", "pnr_render.h", "pnr_ik.h", "pnr_invdyn.h",
                        "pnr_jointstate.h", "pnr_contacts.h", "pnr_rays.h", "pnr_path.h", "pnr_retime.h"],
    "pnr_learn.hip": ["pnr_learn.hip", "pnr_host.h", "pnr_device.h", "pnr_model.h", "pnr_ppo.h", "pnr_mlp.h", "pnr_mlp_forward.h",
                      "pnr_mlp_gather.h", "pnr_mlp_backward.h", "pnr_mlp_wgrad.h", "pnr_mlp_adam.h", "pnr_sampler.h"],
}
SOURCES = sorted({f for deps in UNITS.values() for f in deps})      # every file a unit includes: what _stale() watches
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
               "-mllvm", "-amdgpu-kernarg-preload-count=16",      # leading scalar kernel args arrive preloaded in SGPRs
               "-Wall", "-Wno-unused-function"]
# the sources that define the env-side kernels (what the counter passes under profiles/ were taken on)
ENV_KERNEL_SOURCES = ["pnr_env_kernels.h", "pnr_device.h", "pnr_model.h", "pnr_dyn.h"]
# .. and the learner's (profiles/*learner_pmc_traffic.json: the bytes bench.py quotes in ppo_loop.roofline)
LEARNER_KERNEL_SOURCES = ["pnr_learn.hip", *[f for f in UNITS["pnr_learn.hip"] if f.startswith("pnr_mlp")], "pnr_ppo.h"]


def source_fingerprint(files=ENV_KERNEL_SOURCES) -> str:
    """sha256 (first 16 hex digits) over the named csrc files and the compile flags: stored next to looked-up counter values
    (profiles/pmc_traffic.json, the dynamics SQ-counter summary) so that bench.py can tell when the kernels have changed since
    the counter pass."""
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for f in files:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


# the names the units stamp themselves with (g_unit_fp); pnr_build_fingerprint() joins the stamps in this, UNITS', order
UNIT_TAGS = {"pnr_api.hip": "api", "pnr_queries.hip": "queries", "pnr_learn.hip": "learn"}
# the units whose code reads PNR_DIAG_BUILD (the step kernels' timing-only ablations): what a -DPNR_DIAG_BUILD=1 variant rebuilds
DIAG_UNITS = ("pnr_api.hip",)


def unit_fingerprint(unit: str, extra_flags=()) -> str:
    """What a unit's object must have been built from: the compile flags, its own files, the C-ABI header."""
    import hashlib
    h = hashlib.sha256(" ".join([*HIPCC_FLAGS, *extra_flags]).encode())
    for f in UNITS[unit]:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    with open(HEADER, "rb") as fh:
        h.update(b"pioneer_amd.h\0" + fh.read())
    return h.hexdigest()[:16]


def tree_fingerprint(extra_flags=()) -> str:
    """The string pnr_build_fingerprint() of a library built from THIS tree returns."""
    return "".join(f"{UNIT_TAGS[u]}={unit_fingerprint(u, extra_flags)};" for u in UNITS)


def embedded_fingerprints(path: str) -> dict:
    """The pnr_build_fp tags inside an object or library file ({} if there are none): read from the bytes, nothing is loaded."""
    import re
    if not os.path.exists(path):
        return {}
    with open(path, "rb") as f:
        blob = f.read()
    return {m.group(1).decode(): m.group(2).decode() for m in re.finditer(rb"pnr_build_fp:([a-z]+)=([0-9a-f]{16});", blob)}


def _obj_path(unit: str, tag: str = "") -> str:
    return os.path.join(CSRC, os.path.splitext(unit)[0] + tag + ".o")


def _unit_stale(unit: str, obj: str, extra_flags=()) -> bool:
    return embedded_fingerprints(obj).get(UNIT_TAGS[unit]) != unit_fingerprint(unit, extra_flags)


def _stale() -> bool:
    """The in-tree library is stale unless every unit inside it carries the fingerprint of the tree's sources (content, not mtime)."""
    have = embedded_fingerprints(LIB_PATH)
    return any(have.get(UNIT_TAGS[u]) != unit_fingerprint(u) for u in UNITS)


def build_library(force: bool = False, verbose: bool = False, extra_flags=(), out_path: str = None, units=None) -> str:
    """hipcc --offload-arch=gfx950 -> pioneer_amd/csrc/libpioneer_amd.so (in-tree): the translation units are compiled in
    parallel (only those whose object does not carry the fingerprint of the current sources) and linked.  extra_flags / out_path
    build a variant next to it (e.g. -DPNR_DIAG_BUILD=1 for the timing-only ablations), with objects of its own; `units` names the translation units the flags concern (e.g. ("pnr_learn.hip",) for an
    MLP kernel A/B) — the others are linked from the default build's objects.  Measured on 8 cores: a full forced build 92 s, which is
    pnr_api.hip's (pnr_queries.hip ~15 s, ~25 s since pnr_jointstate.h; pnr_learn.hip ~20 s, in parallel; with the queries in that unit it was 129 s); after a
    change to pnr_rays.h 15 s (was 133 s), after one to pnr_env_kernels.h 116 s (was 133 s)."""
    variant = out_path is not None or bool(extra_flags)
    if variant:
        force = True
        if out_path is None:
            raise ValueError("a variant build (extra_flags) needs its own out_path")
    if not force and not _stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libpioneer_amd.so")
    tag = ("." + os.path.splitext(os.path.basename(out_path))[0]) if variant else ""
    procs, objs = [], []
    own = []
    for unit, deps in UNITS.items():
        if variant and units is not None and unit not in units:
            objs.append(_obj_path(unit))                 # the default build's object (build_library() must have run)
            if _unit_stale(unit, objs[-1]):
                raise RuntimeError(f"{objs[-1]} is missing or not built from the current sources: build the default library first")
            continue
        obj = _obj_path(unit, tag)
        objs.append(obj)
        own.append(obj)
        flags = list(extra_flags) if (variant and (units is None or unit in units)) else []
        if not force and not _unit_stale(unit, obj, flags):
            continue
        cmd = [hipcc, *HIPCC_FLAGS, *flags, f'-DPNR_UNIT_FINGERPRINT="{unit_fingerprint(unit, flags)}"', "-c", "-o", obj,
               os.path.join(CSRC, unit)]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out_path or LIB_PATH, *objs]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True, cwd=CSRC)
    if variant:
        for o in own:
            os.remove(o)
    return out_path or LIB_PATH


_lib = None


def load_library():
    """Load the HIP library; raise loudly if it is not there (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  pioneer_amd has no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as ROCm's).  If this
    # library were loaded first it would pull in /opt/rocm's copy, torch would then load its own, and
    # the two runtimes would not see each other's devices/streams.  Importing torch first makes our
    # DT_NEEDED libamdhip64.so.7 resolve to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pnr_abi_version() != ABI_VERSION:
        raise ImportError(f"libpioneer_amd.so reports ABI {lib.pnr_abi_version()}, include/pioneer_amd.h says {ABI_VERSION}; rebuild")
    # the binary must be the one these sources build (content fingerprints baked in at compile time, not file times); a library
    # named explicitly through PNR_LIB_PATH is somebody's A/B variant with flags of its own and is taken as it is
    built, tree = lib.pnr_build_fingerprint().decode(), tree_fingerprint()
    if built != tree and not os.environ.get("PNR_LIB_PATH"):
        raise ImportError(f"{LIB_PATH} was built from other sources (binary {built}, tree {tree}): rebuild it with "
                          "`python -c 'import __graft_entry__ as g; g.build()'`")
    _lib = lib
    return lib


def check(code, handle=None):
    if code != PNR_OK:
        msg = load_library().pnr_last_error(handle)
        raise PnrError(code, msg.decode() if msg else "unknown")
